"""Cases of the tests of the lattice search with reverse moves (test_lattice_gears_cpu.py checks them and the restatement
without a GPU, test_gpu_lattice_gears.py runs the device on them).  Costs are written (turn, reverse, cusp)."""
import functools

import numpy as np

import lattice_gears_ref as gr

UNREACHABLE = (-1, -1)

# ---- hand values: wall-free, one layer.  (rows, cols, goal state, costs, [(start state, expected path cost)]) ------------------
_U = [(0, c, 4) for c in range(7)]
HAND = (
    (1, 6, (0, 0, 0), (0, 0, 0), [((0, 5, 0), (5, 0)), ((0, 5, 4), UNREACHABLE)]),
    (1, 6, (0, 0, 0), (0, 2, 3), [((0, 5, 0), (15, 0))]),               # five reverse moves, no cusp charged
    (1, 6, (0, 5, 0), (0, 0, 0), [((0, 0, 0), (5, 0))]),
    (1, 6, (0, 5, 0), (0, 2, 3), [((0, 0, 0), (5, 0))]),                # reversing never pays
    (1, 7, (0, 6, 0), (0, 0, 0), [(s, UNREACHABLE) for s in _U]),
    (2, 7, (0, 6, 0), (0, 0, 0), list(zip(_U, [(4, 2), (3, 2), (2, 2), (5, 0), (4, 0), (5, 0), (6, 0)]))),
    (3, 7, (0, 6, 0), (0, 0, 0), list(zip(_U, [(4, 2), (3, 2), (2, 2), (5, 0), (4, 0), (5, 0), (4, 1)]))),
    (3, 7, (0, 6, 0), (0, 1, 3), list(zip(_U, [(9, 2), (8, 2), (7, 2), (11, 2), (11, 2), (13, 1), (12, 1)]))),
    (3, 7, (0, 6, 0), (2, 1, 3), list(zip(_U, [(17, 2), (16, 2), (15, 2), (19, 2), (20, 2), (21, 1), (20, 1)]))),
)
# one minimum path of 3 x 7 at (0, 1, 3) from (0, 3, 4) as (row, col, heading, gear of the move into it) and its move costs
HAND_PATH = ((0, 3, 4, None), (0, 2, 4, 0), (0, 3, 5, 1), (1, 4, 6, 1), (0, 5, 7, 0), (0, 6, 0, 0))
HAND_PATH_MOVES = ((1, 0), (1 + 1 + 3, 0), (1, 1), (3, 1), (1, 0))

# restated from csrc/lattice_gears.hip (tests/test_lattice_gears_cpu.py reads them back from the source)
LG_THREADS = 512             # `constexpr int LATTICE_THREADS = 512;` (csrc/lattice_field.h): the stride of the field kernels over the lines
LG_LDS_WORDS = 36864         # `constexpr int LATTICE_LDS_WORDS = 36864;`: the packed 16-layer field one workgroup's LDS holds

# ---- the shapes of the device tests: name -> (rows, cols, wall share or "one" / None, layers, cost sets, extra goals) ---------
SHAPES = {
    "1x1": (1, 1, None, 1, ((0, 0, 0),), ()),
    "1x2": (1, 2, None, 1, ((0, 0, 0),), ()),
    "1x6": (1, 6, None, 1, ((0, 0, 0), (0, 2, 3)), ((0, 0, 0),)),       # the reversing corridor
    "2x7": (2, 7, None, 1, ((0, 0, 0),), ((0, 6, 0),)),
    "3x7": (3, 7, None, 1, ((0, 0, 0), (0, 1, 3), (2, 1, 3)), ((0, 6, 0),)),   # the three-point turn
    "5x5w": (5, 5, "one", 1, ((0, 0, 0), (1, 2, 1)), ()),
    # 16 * 585 * (1 + 2 + 1 + 3) = 65520: the last count the packed form takes on this map
    "9x65": (9, 65, 0.30, 1, ((0, 0, 0), (2, 1, 3)), ()),
    # a cost of 255 at the widest map the 2^21 bound admits with it in this family (16 * 455 * 256 < 2^21; 9 x 65 at cost 255
    # is 16 * 585 * 256 >= 2^21 and refused: test_lattice_gears_cpu.py asserts that): wide by counts
    "7x65": (7, 65, 0.30, 1, ((0, 0, 255),), ()),
    "20x23": (20, 23, 0.25, 8, ((1, 0, 2), (0, 3, 0)), ()),             # a different occupancy per heading
    "40x130": (40, 130, 0.20, 1, ((1, 1, 1),), ()),                     # the wide form by size
    # the LDS form past one trip of its 512 threads over the lines: 1808 lines, 4 trips, and lines of 300 cells
    "2x300": (2, 300, "one", 1, ((0, 0, 0), (1, 1, 1)), ()),
    "300x2": (300, 2, "one", 1, ((0, 1, 0),), ()),
    # row stride 9, padded 256 x 9 = 2304 cells: 16 layers are EXACTLY the 36864 words of LG_LDS_WORDS.  A cost sum of 1 relaxes
    # in LDS (counts 56896 <= 65535), 2 is wide by counts (85344); one row more (257 x 9) is wide by size
    "254x7": (254, 7, 0.20, 1, ((0, 1, 0), (1, 0, 1)), ()),
    "255x7": (255, 7, 0.20, 1, ((0, 0, 0),), ()),
    "45x45": (45, 45, 0.25, 1, ((0, 0, 0),), ()),                       # the largest square field in LDS: 16 x 47 x 47 = 35344 words
}
# every other (shape, costs) relaxes in LDS
WIDE = {("7x65", (0, 0, 255)), ("40x130", (1, 1, 1)), ("254x7", (1, 0, 1)), ("255x7", (0, 0, 0))}
# goals of goals_of() a shape leaves out (default: none).  40 x 130 has 83 200 states, a second of restated Dijkstra per valid
# goal; it drops the wall goal at a fixed heading and keeps the wall goal at heading -1, which is a wall goal too, and every
# refused goal
GOAL_DROP = {"40x130": (2,)}
TRACE_SHAPES = (("5x5w", (1, 2, 1)), ("3x7", (0, 1, 3)), ("2x7", (0, 0, 0)), ("20x23", (1, 0, 2)))


def n_lines(name):
    """The lines a field kernel shares among its threads: rows and columns twice, the diagonals four times."""
    rows, cols = SHAPES[name][:2]
    return 2 * rows + 2 * cols + 4 * (rows + cols - 1)


def lds_words(name):
    """Words of the padded 16-layer field: (rows + 2) rows of odd stride (cols + 2) | 1."""
    rows, cols = SHAPES[name][:2]
    return 16 * (rows + 2) * ((cols + 2) | 1)


def counts(name, costs):
    """The largest count a path over the 16 * rows * cols states can reach."""
    rows, cols = SHAPES[name][:2]
    return 16 * rows * cols * (1 + sum(costs))


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
    the grid, goal headings 8 and -2, then the shape's own goals; without the ones GOAL_DROP names."""
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
    goals = [g for i, g in enumerate(goals) if i not in GOAL_DROP.get(name, ())]
    return np.asarray(goals, np.int32)


@functools.lru_cache(maxsize=None)
def fields_of(name, costs):
    """The restated fields of every goal of the shape, computed once: int32 [G, 2, 8, rows, cols, 2]."""
    layers = layers_of(name)
    out = np.stack([gr.gear_field(layers, g, costs) for g in goals_of(name)])
    out.setflags(write=False)
    return out


def trace_problems(name, max_goals=3):
    """Starts at every state of the map (blocked ones included) towards the first goals of the shape (walls: a fixed and a free
    heading on free cells and one on a wall; wall-free: the two free ones and the shape's own) -> (starts [B, 3], goal states
    [B, 3], field_index [B])."""
    rows, cols = SHAPES[name][:2]
    goals = goals_of(name)
    pick = [0, 1, 2] if SHAPES[name][2] is not None else [0, 1, len(goals) - 1]
    pick = pick[:max_goals]
    states = np.asarray([(r, c, h) for h in range(8) for r in range(rows) for c in range(cols)], np.int32)
    starts = np.concatenate([states] * len(pick))
    fidx = np.repeat(np.asarray(pick, np.int32), len(states))
    return starts, goals[fidx], fidx


@functools.lru_cache(maxsize=None)
def trace_case(name, costs):
    """Every state of the map as a start towards the trace goals, then nine refused problems -> (starts, goals, field_index,
    what lattice_gears_ref.search gives)."""
    rows, cols = SHAPES[name][:2]
    starts, goals, fidx = trace_problems(name)
    g0 = goals_of(name)[0]
    n_goals = len(goals_of(name))
    bad_starts = [(0, 0, 0), (0, 0, 0), (-1, 0, 0), (rows, 0, 0), (0, cols, 0), (0, -1, 0), (0, 0, -1), (0, 0, 8), (0, 0, 0)]
    bad_goals = [g0] * 8 + [(rows, 0, 0)]
    bad_fidx = [-1, n_goals, 0, 0, 0, 0, 0, 0, 4]
    starts = np.concatenate([starts, np.asarray(bad_starts, np.int32)])
    goals = np.concatenate([goals, np.asarray(bad_goals, np.int32)])
    fidx = np.concatenate([fidx, np.asarray(bad_fidx, np.int32)])
    want = gr.search(fields_of(name, costs), (rows, cols), starts, goals, fidx, costs)
    assert (want[4][-9:] == 2).all()
    return starts, goals, fidx, want


# ---- random maps for the consequences (i) - (iii) ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_map(n_layers, seed=5):
    """5 x 6 with 20 % walls, one or eight independent layers."""
    rng = np.random.default_rng(seed + n_layers)
    layers = (rng.random((n_layers, 5, 6)) < 0.2).astype(np.uint8)
    layers.setflags(write=False)
    return layers


# ---- seeding -------------------------------------------------------------------------------------------------------------------
def serpentine(rows=12, cols=40):
    """A lattice path long enough for the global-workspace form of the seeding kernel (7 * (count + 2) + 3 doubles > 64 KiB from
    count = 1168 on): east along row 0, a half turn through headings 1, 2, 3 into row 2, west along it, a half turn through 3, 2, 1 into row 4 ...
    Not a minimum path of any field; the seeding entry takes any cells and headings.  -> (cells [n, 2], headings [n])."""
    cells, heads = [], []
    r, c, h = 0, 2, 0                                       # columns 0 .. 39
    cells.append((r, c)); heads.append(h)
    sweep = 0
    while len(cells) < 1300:
        east = sweep % 2 == 0
        for _ in range(cols - 4):
            c += 1 if east else -1
            cells.append((r, c)); heads.append(0 if east else 4)
        for hn in ((1, 2, 3, 4) if east else (3, 2, 1, 0)):
            r, c = r + gr.DIRS[hn][0], c + gr.DIRS[hn][1]
            cells.append((r, c)); heads.append(hn)
        sweep += 1
    return np.asarray(cells, np.int32), np.asarray(heads, np.int32)
