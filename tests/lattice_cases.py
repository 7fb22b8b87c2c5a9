"""Cases of the lattice-search tests (test_lattice_cpu.py checks them and the restatement without a GPU,
test_gpu_lattice.py runs the device on them)."""
import functools

import numpy as np

import lattice_ref as lr

UNREACHABLE = (-1, -1)

# ---- hand cases: wall-free, one layer.  (rows, cols, goal state, turn_cost, [(start state, expected pair)]) ------------------
HAND = (
    (5, 5, (2, 4, 0), 0, [((2, 0, 0), (4, 0)), ((2, 0, 2), (2, 2)), ((2, 0, 6), (2, 2))]),
    (5, 5, (2, 4, 0), 2, [((2, 0, 2), (10, 2))]),
    (4, 7, (0, 6, 0), 0, [((0, c, 4), pair) for c, pair in
                          enumerate([UNREACHABLE, (3, 5), (4, 4), (5, 4), (6, 4), (7, 4), (6, 4)])]),
    (1, 6, (0, 5, 0), 0, [((0, 0, 0), (5, 0)), ((0, 0, 4), UNREACHABLE)]),
    (7, 7, (3, 5, -1), 0, [((3, 1, 0), (4, 0)), ((3, 1, 4), (2, 5))]),
) + tuple((3, 7, (gr, 6, 0), 0, [((r, c, 4), UNREACHABLE) for r in range(3) for c in range(7)]) for gr in range(3))   # a U-turn needs four rows

# ---- the shapes of the device tests: name -> (rows, cols, wall share or "one" / None, layers, turn costs, extra goals) ------
# `lds` per turn cost is what nfopp_lattice_fields_workspace_bytes must say: a constant that moves names the shape to replace
SHAPES = {
    "1x1": (1, 1, None, 1, (0,), ()),
    "1x2": (1, 2, None, 1, (0,), ()),
    "1x9": (1, 9, None, 1, (0,), ()),
    "3x7": (3, 7, None, 1, (0,), ((1, 6, 0),)),            # U-turn unreachable
    "4x7": (4, 7, None, 1, (0,), ((0, 6, 0),)),            # U-turn hand case
    "5x5": (5, 5, None, 1, (0, 2), ((2, 4, 0),)),
    "1x1w": (1, 1, "one", 1, (0,), ()),
    "1x2w": (1, 2, "one", 1, (0,), ()),
    "1x9w": (1, 9, "one", 1, (0,), ()),
    "3x7w": (3, 7, "one", 1, (0,), ()),
    "4x7w": (4, 7, "one", 1, (0,), ()),
    "5x5w": (5, 5, "one", 1, (0,), ()),
    "9x65": (9, 65, 0.30, 1, (0, 255), ()),                # a row across a 64-cell boundary; 255: the wide form by counts
    "20x23": (20, 23, 0.25, 8, (0, 1, 3), ()),             # a different occupancy per heading
    "40x130": (40, 130, 0.20, 1, (1,), ()),                # the wide form by size
    # the LDS form past one trip of its 512 threads over the lines (every shape above that relaxes in LDS has fewer): 1808 lines,
    # 4 trips, and lines of 300 cells
    "2x300": (2, 300, "one", 1, (0, 3), ()),
    "300x2": (300, 2, "one", 1, (0, 3), ()),
    # row stride 9, padded 512 x 9 = 4608 cells: 8 layers are EXACTLY the 36864 words of LS_LDS_WORDS.  Turn cost 1 relaxes in
    # LDS (counts 57120 <= 65535), 2 is wide by counts (85680); one row more (513 x 9) is wide by size
    "510x7": (510, 7, 0.20, 1, (1, 2), ()),
    "511x7": (511, 7, 0.20, 1, (0,), ()),
    "65x65": (65, 65, 0.25, 1, (0,), ()),                  # the largest square field in LDS: 8 x 67 x 67 = 35912 words
}
# every other (shape, turn cost) relaxes in LDS
WIDE = {("9x65", 255), ("40x130", 1), ("510x7", 2), ("511x7", 0)}
TRACE_SHAPES = (("5x5", 0), ("5x5w", 0), ("9x65", 0), ("20x23", 1), ("2x300", 0), ("510x7", 1))
TRACE_GOALS = {"9x65": 2, "2x300": 1, "510x7": 1}         # goals traced from every state (default 3): the large maps take fewer
# 510 x 7 has 28560 states with paths of up to 439 cells, 24 s of restated traces: every 17th state (17 is coprime to the 7
# columns and the 3570 cells of a heading, so every column and heading, and rows all along the map, still start paths) keeps
# it under 2 s
TRACE_EVERY = {"510x7": 17}
# restated from csrc/lattice_search.hip (tests/test_lattice_cpu.py reads them back from the source)
LS_THREADS = 512             # `constexpr int LATTICE_THREADS = 512;` (csrc/lattice_field.h): the stride of the field kernels over the lines
LS_LDS_WORDS = 36864         # `constexpr int LATTICE_LDS_WORDS = 36864;`: the packed 8-layer field one workgroup's LDS holds


def n_lines(name):
    """The lines a field kernel shares among its threads: rows and columns twice, the diagonals four times."""
    rows, cols = SHAPES[name][:2]
    return 2 * rows + 2 * cols + 4 * (rows + cols - 1)


def lds_words(name):
    """Words of the padded 8-layer field: (rows + 2) rows of odd stride (cols + 2) | 1."""
    rows, cols = SHAPES[name][:2]
    return 8 * (rows + 2) * ((cols + 2) | 1)


@functools.lru_cache(maxsize=None)
def layers_of(name):
    rows, cols, walls, n_layers, _, _ = SHAPES[name]
    layers = np.zeros((n_layers, rows, cols), np.uint8)
    if walls == "one":
        layers[:, rows // 2, cols // 2] = 1
    elif walls is not None:
        rng = np.random.default_rng(rows * 1000 + cols)
        layers[:] = rng.random(layers.shape) < walls       # independent layers when there are eight
    layers.setflags(write=False)
    return layers


@functools.lru_cache(maxsize=None)
def goals_of(name):
    """int32 [G, 3]: a fixed and a free heading on free cells, both on a wall cell where the map has one, two goals outside
    the grid, goal headings 8 and -2, then the shape's own goals."""
    rows, cols, _, _, _, extra = SHAPES[name]
    layers = layers_of(name)
    blocked_all = layers.all(0) if layers.shape[0] == 8 else layers[0] != 0
    free = np.argwhere(~blocked_all)
    rng = np.random.default_rng(7 + rows * cols)
    goals = []
    if len(free):
        a, b = free[rng.integers(len(free))], free[rng.integers(len(free))]
        h = next(h for h in range(8) if not layers[h % layers.shape[0], a[0], a[1]])
        goals += [(a[0], a[1], h), (b[0], b[1], -1)]
    wall = np.argwhere(layers[0] != 0)
    if len(wall):
        w = wall[rng.integers(len(wall))]
        goals += [(w[0], w[1], 0), (w[0], w[1], -1)]
    goals += [(rows, 0, 0), (0, -1, -1), (0, 0, 8), (0, 0, -2)]
    goals += list(extra)
    return np.asarray(goals, np.int32)


@functools.lru_cache(maxsize=None)
def fields_of(name, turn_cost):
    """The restated fields of every goal of the shape, computed once: int32 [G, 8, rows, cols, 2]."""
    layers = layers_of(name)
    out = np.stack([lr.lattice_field(layers, g, turn_cost) for g in goals_of(name)])
    out.setflags(write=False)
    return out


def trace_problems(name, max_goals=None):
    """Starts at every state of the map (blocked ones included; every TRACE_EVERY-th where the map has an entry there) towards
    the first goals of the shape (TRACE_GOALS of them unless `max_goals` says otherwise) -> (starts [B, 3], goal states
    [B, 3], field_index [B]) with B a multiple of the number of start states."""
    rows, cols = SHAPES[name][:2]
    goals = goals_of(name)
    max_goals = TRACE_GOALS.get(name, 3) if max_goals is None else max_goals
    n = min(max_goals, 4 if SHAPES[name][2] is not None else 2)
    states = np.asarray([(r, c, h) for h in range(8) for r in range(rows) for c in range(cols)], np.int32)[::TRACE_EVERY.get(name, 1)]
    starts = np.concatenate([states] * n)
    fidx = np.repeat(np.arange(n, dtype=np.int32), len(states))
    return starts, goals[fidx], fidx


# ---- the one approach of a fixed-heading goal -----------------------------------------------------------------------------
def approach_case():
    """3 x 5, goal (1, 3) heading 0: it is entered from (1, 2) only, which is blocked at every heading.  -> (layers, goal)."""
    layers = np.zeros((1, 3, 5), np.uint8)
    layers[0, 1, 2] = 1
    return layers, (1, 3, 0)
