"""The rule of the heading-aware lattice search (csrc/lattice_search.hip, stated in include/nfopp_hip.h) restated with numpy
and heapq, for the tests.  Integer pairs throughout, ordered by the exact sign test of grid_search_ref.Cost.

State: (cell (row, col), heading h in 0 .. 7), h standing for h * pi / 4.  Direction h as (d row, d col), row = y, col = x:
  0 (0,+1)  1 (+1,+1)  2 (+1,0)  3 (+1,-1)  4 (0,-1)  5 (-1,-1)  6 (-1,0)  7 (-1,+1).
Occupancy: layers [L, rows, cols], L = 1 or 8, non-zero = blocked; state (c, h) reads layer h mod L; cells outside the image
are blocked; no corner rule.  Moves are forward only: from (c, h) to (c + dir(h'), h') with h' in {h, h + 1, h - 1} mod 8 --
along the heading the robot has AFTER the move; the target state must be free.  Cost: a move to an even h' adds (1, 0), to an
odd h' (0, 1), and a move with h' != h a further (turn_cost, 0).  Goal state: (goal cell, goal heading), every heading of the
cell with goal heading -1; goal states cost (0, 0) and are forced free.  Field: the minimum cost from every state to the
goal; (-1, -1) for blocked states, states that cannot reach it, and every state when the goal cell is outside the grid or
the goal heading outside -1 .. 7.  Trace: from (start cell, start heading), not tested for occupancy; at a state with a cost
the first successor in the order h' = h, h + 1, h - 1 whose cost plus the move equals the current cost exactly; the end is
the first state with cost (0, 0).  From a start whose own value is the sentinel the first step goes to the successor with
the smallest d + move (ties: the same order), the path's cost is that sum, and without such a successor the status is 1.
Status: 0 ok, 1 unreachable, 2 start or goal cell outside the grid or start heading outside 0 .. 7."""
import heapq

import numpy as np

from grid_search_ref import Cost

DIRS = ((0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1))
HEADINGS = 8


def successors(h):
    return (h, (h + 1) % 8, (h - 1) % 8)


def move_cost(h, hn, turn_cost):
    """(a, b) of the move from heading h to heading hn."""
    return (0 if hn & 1 else 1) + (turn_cost if hn != h else 0), hn & 1


def goal_ok(shape, goal):
    rows, cols = shape
    return 0 <= goal[0] < rows and 0 <= goal[1] < cols and -1 <= goal[2] <= 7


def free_mask(layers, goal):
    """bool [8, rows, cols]: the states the search may stand in, goal states forced free."""
    layers = np.asarray(layers) != 0
    free = np.stack([~layers[h % layers.shape[0]] for h in range(HEADINGS)])
    if goal_ok(layers.shape[1:], goal):
        for h in range(HEADINGS):
            if goal[2] < 0 or goal[2] == h:
                free[h, goal[0], goal[1]] = True
    return free


def lattice_field(layers, goal, turn_cost=0):
    """-> int32 [8, rows, cols, 2]: Dijkstra from the goal states over the moves reversed."""
    layers = np.asarray(layers)
    _, rows, cols = layers.shape
    goal = tuple(int(v) for v in goal)
    out = np.full((HEADINGS, rows, cols, 2), -1, np.int32)
    if not goal_ok((rows, cols), goal):
        return out
    free = free_mask(layers, goal)
    heap, best, done = [], {}, set()
    for h in range(HEADINGS):
        if goal[2] < 0 or goal[2] == h:
            best[(h, goal[0], goal[1])] = Cost((0, 0))
            heap.append((Cost((0, 0)), h, goal[0], goal[1]))
    heapq.heapify(heap)
    while heap:
        d, hn, r, c = heapq.heappop(heap)
        if (hn, r, c) in done:
            continue
        done.add((hn, r, c))
        out[hn, r, c] = d
        pr, pc = r - DIRS[hn][0], c - DIRS[hn][1]          # the move into (r, c, hn) came along dir(hn)
        if not (0 <= pr < rows and 0 <= pc < cols):
            continue
        for h in successors(hn):                            # h' in {h, h +- 1}  <=>  h in {h', h' +- 1}
            if not free[h, pr, pc] or (h, pr, pc) in done:
                continue
            m = move_cost(h, hn, turn_cost)
            nd = Cost((d[0] + m[0], d[1] + m[1]))
            old = best.get((h, pr, pc))
            if old is None or nd < old:
                best[(h, pr, pc)] = nd
                heapq.heappush(heap, (nd, h, pr, pc))
    return out


def _candidates(field, r, c, h, turn_cost):
    """The successors of (r, c, h) that hold a cost, in rule order: [(hn, nr, nc, (a, b) of field + move)]."""
    _, rows, cols, _ = field.shape
    out = []
    for hn in successors(h):
        nr, nc = r + DIRS[hn][0], c + DIRS[hn][1]
        if 0 <= nr < rows and 0 <= nc < cols and field[hn, nr, nc, 0] >= 0:
            m = move_cost(h, hn, turn_cost)
            out.append((hn, nr, nc, (int(field[hn, nr, nc, 0]) + m[0], int(field[hn, nr, nc, 1]) + m[1])))
    return out


def trace_path(field, start, turn_cost=0):
    """-> (cells int64 [count, 2], headings int64 [count], (a, b)); status 1: (empty, empty, (-1, -1))."""
    r, c, h = (int(v) for v in start)
    cells, heads = [(r, c)], [h]
    cur = (int(field[h, r, c, 0]), int(field[h, r, c, 1]))
    if cur[0] < 0:
        best = None
        for hn, nr, nc, cand in _candidates(field, r, c, h, turn_cost):
            if best is None or Cost(cand) < Cost(best[3]):
                best = (hn, nr, nc, cand)
        if best is None:
            return np.zeros((0, 2), np.int64), np.zeros(0, np.int64), (-1, -1)
        h, r, c, cost = best
        cells.append((r, c))
        heads.append(h)
        cur = (int(field[h, r, c, 0]), int(field[h, r, c, 1]))
    else:
        cost = cur
    while cur != (0, 0):
        for hn, nr, nc, cand in _candidates(field, r, c, h, turn_cost):
            if cand == cur:
                h, r, c = hn, nr, nc
                break
        else:
            raise AssertionError("descent is stuck at (%d, %d, %d): not a fixed-point field" % (r, c, h))
        cells.append((r, c))
        heads.append(h)
        cur = (int(field[h, r, c, 0]), int(field[h, r, c, 1]))
    return np.asarray(cells, np.int64), np.asarray(heads, np.int64), cost


def trace_recursive(field, start, turn_cost=0):
    """The trace order stated a second way, for states with a cost: path(s) = [s] if d(s) = (0, 0), else [s] + path(n) for
    the FIRST n of successors(s) with d(n) + move = d(s).  -> list of (row, col, heading)."""
    r, c, h = (int(v) for v in start)
    cur = (int(field[h, r, c, 0]), int(field[h, r, c, 1]))
    assert cur[0] >= 0
    if cur == (0, 0):
        return [(r, c, h)]
    fits = [(nr, nc, hn) for hn, nr, nc, cand in _candidates(field, r, c, h, turn_cost) if cand == cur]
    return [(r, c, h)] + trace_recursive(field, fits[0], turn_cost)


def check_path(layers, cells, heads, start, goal, turn_cost=0):
    """Every move goes along the new heading, the heading changes by at most one step, every state after the first is free
    (goal states count as free), the path starts in `start` and ends in the goal state.  -> (a, b) summed over the moves."""
    free = free_mask(layers, goal)
    assert (int(cells[0][0]), int(cells[0][1]), int(heads[0])) == tuple(int(v) for v in start), "wrong first state"
    assert tuple(int(v) for v in cells[-1]) == (goal[0], goal[1]) and (goal[2] < 0 or int(heads[-1]) == goal[2]), "wrong last state"
    a = b = 0
    for k in range(1, len(cells)):
        h, hn = int(heads[k - 1]), int(heads[k])
        assert (hn - h) % 8 in (0, 1, 7), "heading jumps"
        assert (int(cells[k][0] - cells[k - 1][0]), int(cells[k][1] - cells[k - 1][1])) == DIRS[hn], "move not along the new heading"
        assert free[hn, cells[k][0], cells[k][1]], "path enters a blocked state"
        m = move_cost(h, hn, turn_cost)
        a, b = a + m[0], b + m[1]
    return a, b


def search(fields, layers_shape, starts, goals, field_index, turn_cost=0):
    """What nfopp_lattice_trace_paths reports for problems over given fields [G, 8, rows, cols, 2]: -> (cells int32
    [B, max(count, 1), 2] zero-padded, headings [B, same], count [B], status [B], cost [B, 2])."""
    rows, cols = layers_shape
    B = len(starts)
    res, status, count, cost = [], np.zeros(B, np.int32), np.zeros(B, np.int32), np.full((B, 2), -1, np.int32)
    for p in range(B):
        s, g, fi = starts[p], goals[p], int(field_index[p])
        if not (0 <= s[0] < rows and 0 <= s[1] < cols and 0 <= s[2] <= 7 and 0 <= g[0] < rows and 0 <= g[1] < cols
                and 0 <= fi < len(fields)):
            status[p] = 2
            res.append(None)
            continue
        cells, heads, c = trace_path(fields[fi], s, turn_cost)
        if len(cells) == 0:
            status[p] = 1
            res.append(None)
            continue
        res.append((cells, heads))
        count[p], cost[p] = len(cells), c
    L = max(int(count.max(initial=0)), 1)
    out_cells, out_heads = np.zeros((B, L, 2), np.int32), np.zeros((B, L), np.int32)
    for p, r in enumerate(res):
        if r is not None:
            out_cells[p, :len(r[0])], out_heads[p, :len(r[1])] = r[0], r[1]
    return out_cells, out_heads, count, status, cost


def heading_index(theta):
    """round(theta / (pi / 4)) in float64, half to even, then mod 8."""
    return int(np.round(np.float64(theta) / (np.pi / 4))) % 8
