"""The rule of the lattice search with reverse moves and gear changes (csrc/lattice_gears.hip, stated in
include/nfopp_hip.h) restated with numpy and heapq, for the tests.  Integer pairs throughout, ordered by the exact sign test
of grid_search_ref.Cost.  Directions, headings, occupancy layers and `heading_index` are lattice_ref's, unchanged.

State: (cell c = (row, col), heading h in 0 .. 7, gear s in {0 forward, 1 reverse}); s is the gear of the move that entered
the state.  Occupancy does not depend on s: state (c, h, s) reads layer h mod L, outside = blocked, no corner rule.
Moves.  Forward, gear 0: from (c, h) to (c + dir(h'), h').  Reverse, gear 1: from (c, h) to (c - dir(h), h') -- a forward move
run backwards in time, so the robot backs along the heading it had BEFORE the move.  In both h' in {h, h + 1, h - 1} mod 8,
and the target state must be free.
Cost: a forward move adds (1, 0) for even h' and (0, 1) for odd h'; a reverse move adds (1, 0) for even h and (0, 1) for odd
h: the parity of the direction it moves along.  Either adds (turn_cost, 0) where h' != h; a reverse move adds a further
(reverse_cost, 0); a move whose gear differs from s adds (cusp_cost, 0).  All three costs are integers 0 .. 255.
Goal: (goal cell, goal heading or -1 for every heading), at both gears; cost (0, 0), forced free.
Field: d(s, h, c) = the minimum cost from the state to the goal, int32 [2, 8, rows, cols, 2]; (-1, -1) for blocked states,
states that cannot reach the goal, and every state of a bad goal (cell outside the grid, heading outside -1 .. 7).
Trace: the start has no gear: its first move is charged no cusp cost; the start state is not tested for occupancy.  A start
that is a goal state gives the one-state path with cost (0, 0).  Otherwise the first move is the one of the six successors
with the smallest d(successor) + move cost without the cusp term, in the order forward h, h + 1, h - 1, then reverse h, h + 1,
h - 1, ties to the first in that order; the path's cost is that sum; without such a successor the status is 1.  After the
first move the next state is the first successor in the same order whose cost plus the move (with the cusp term) equals the
current cost exactly; the end is the first state with cost (0, 0).  This one rule covers blocked starts too.
gears[k] is the gear of the move into state k; gears[0] is the gear of the first move, or 0 for a one-state path.
Status: 0 ok, 1 unreachable, 2 start or goal cell outside the grid or start heading outside 0 .. 7.

Seeding theta (nfopp_lattice_seed_trajectories): see `seed_theta`."""
import heapq

import numpy as np

from grid_search_ref import Cost, polyline
from lattice_ref import DIRS, HEADINGS, free_mask, goal_ok, successors

F32 = np.float32


def length(h):
    """(a, b) of one cell along dir(h)."""
    return (0, 1) if h & 1 else (1, 0)


def moves(r, c, h, costs):
    """The six moves out of (r, c, h) in rule order: [(nr, nc, hn, gear, (a, b) without the cusp term)]; the cell may lie
    outside the grid."""
    tc, rc, _ = costs
    out = []
    for hn in successors(h):                                # forward: along the heading AFTER the move
        a, b = length(hn)
        out.append((r + DIRS[hn][0], c + DIRS[hn][1], hn, 0, (a + (tc if hn != h else 0), b)))
    for hn in successors(h):                                # reverse: against the heading BEFORE the move
        a, b = length(h)
        out.append((r - DIRS[h][0], c - DIRS[h][1], hn, 1, (a + (tc if hn != h else 0) + rc, b)))
    return out


def gear_field(layers, goal, costs=(0, 0, 0)):
    """-> int32 [2, 8, rows, cols, 2]: Dijkstra from the goal states over the moves reversed."""
    layers = np.asarray(layers)
    _, rows, cols = layers.shape
    goal = tuple(int(v) for v in goal)
    tc, rc, cc = costs
    out = np.full((2, HEADINGS, rows, cols, 2), -1, np.int32)
    if not goal_ok((rows, cols), goal):
        return out
    free = free_mask(layers, goal)
    heap, best, done = [], {}, set()
    for s in range(2):
        for h in range(HEADINGS):
            if goal[2] < 0 or goal[2] == h:
                best[(s, h, goal[0], goal[1])] = Cost((0, 0))
                heap.append((Cost((0, 0)), s, h, goal[0], goal[1]))
    heapq.heapify(heap)
    while heap:
        d, sn, hn, r, c = heapq.heappop(heap)
        if (sn, hn, r, c) in done:
            continue
        done.add((sn, hn, r, c))
        out[sn, hn, r, c] = d
        for h in successors(hn):                            # h' in {h, h +- 1}  <=>  h in {h', h' +- 1}
            if sn == 0:                                     # entered forward along dir(hn): from (r, c) - dir(hn)
                pr, pc = r - DIRS[hn][0], c - DIRS[hn][1]
                a, b = length(hn)
            else:                                           # entered in reverse against dir(h): from (r, c) + dir(h)
                pr, pc = r + DIRS[h][0], c + DIRS[h][1]
                a, b = length(h)
                a += rc
            if not (0 <= pr < rows and 0 <= pc < cols) or not free[h, pr, pc]:
                continue
            a += tc if h != hn else 0
            for s in range(2):                              # the gear the predecessor was entered with
                if (s, h, pr, pc) in done:
                    continue
                nd = Cost((d[0] + a + (cc if s != sn else 0), d[1] + b))
                old = best.get((s, h, pr, pc))
                if old is None or nd < old:
                    best[(s, h, pr, pc)] = nd
                    heapq.heappush(heap, (nd, s, h, pr, pc))
    return out


def _candidates(field, r, c, h, s, costs):
    """The successors of (r, c, h) that hold a cost, in rule order: [(nr, nc, hn, gear, (a, b) of field + move)]; the cusp
    term is charged against gear `s`, not at all with s = None (the start has no gear)."""
    rows, cols = len(field[0][0]), len(field[0][0][0])      # a numpy field or its nested lists (search() passes those)
    out = []
    for nr, nc, hn, sn, m in moves(r, c, h, costs):
        if 0 <= nr < rows and 0 <= nc < cols:
            d = field[sn][hn][nr][nc]
            if d[0] >= 0:
                cusp = costs[2] if s is not None and sn != s else 0
                out.append((nr, nc, hn, sn, (int(d[0]) + m[0] + cusp, int(d[1]) + m[1])))
    return out


def trace_path(field, start, costs=(0, 0, 0)):
    """-> (cells int64 [count, 2], headings int64 [count], gears int64 [count], (a, b)); status 1: (empty x 3, (-1, -1))."""
    r, c, h = (int(v) for v in start)
    if tuple(field[0][h][r][c]) == (0, 0):
        return np.asarray([(r, c)], np.int64), np.asarray([h], np.int64), np.zeros(1, np.int64), (0, 0)
    best = None
    for cand in _candidates(field, r, c, h, None, costs):
        if best is None or Cost(cand[4]) < Cost(best[4]):
            best = cand
    if best is None:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), (-1, -1)
    cells, heads = [(r, c)], [h]
    r, c, h, s, cost = best
    gears = [s]
    while True:
        cells.append((r, c))
        heads.append(h)
        gears.append(s)
        cur = (int(field[s][h][r][c][0]), int(field[s][h][r][c][1]))
        if cur == (0, 0):
            break
        for nr, nc, hn, sn, cand in _candidates(field, r, c, h, s, costs):
            if cand == cur:
                r, c, h, s = nr, nc, hn, sn
                break
        else:
            raise AssertionError("descent is stuck at (%d, %d, %d, %d): not a fixed-point field" % (r, c, h, s))
    return np.asarray(cells, np.int64), np.asarray(heads, np.int64), np.asarray(gears, np.int64), cost


def trace_recursive(field, state, costs=(0, 0, 0)):
    """The trace order stated a second way.  path(x) for a state x = (r, c, h, s) with a cost: [x] if d(x) = (0, 0), else [x]
    + path(n) for the FIRST n of the six successors with d(n) + move + cusp = d(x).  For a start (s = None) that is no goal
    state: [start] + path(n) for the first n among those with the smallest d(n) + move.  -> list of (row, col, heading, gear),
    the start's gear None."""
    r, c, h, s = state
    r, c, h = int(r), int(c), int(h)
    if s is None:
        if tuple(field[0][h][r][c]) == (0, 0):
            return [(r, c, h, None)]
        cands = _candidates(field, r, c, h, None, costs)
        low = min(Cost(cand[4]) for cand in cands)
        fits = [cand for cand in cands if Cost(cand[4]) == low]
    else:
        cur = (int(field[s][h][r][c][0]), int(field[s][h][r][c][1]))
        assert cur[0] >= 0
        if cur == (0, 0):
            return [(r, c, h, s)]
        fits = [cand for cand in _candidates(field, r, c, h, s, costs) if cand[4] == cur]
    return [(r, c, h, s)] + trace_recursive(field, fits[0][:4], costs)


def check_path(layers, cells, heads, gears, start, goal, costs=(0, 0, 0)):
    """Move by move: the heading changes by at most one step, the displacement is the one of the move's gear (forward along
    the new heading, reverse against the old one), every entered state is free (goal states count as free), the path starts
    in `start` and ends in the goal state; gears[0] is the first move's gear (0 for a one-state path).  -> ((a, b) summed
    over the moves, the first charged no cusp; gear changes)."""
    tc, rc, cc = costs
    free = free_mask(layers, goal)
    assert (int(cells[0][0]), int(cells[0][1]), int(heads[0])) == tuple(int(v) for v in start), "wrong first state"
    assert tuple(int(v) for v in cells[-1]) == (goal[0], goal[1]) and (goal[2] < 0 or int(heads[-1]) == goal[2]), "wrong last state"
    assert int(gears[0]) == (int(gears[1]) if len(cells) > 1 else 0), "gears[0] is not the first move's gear"
    a = b = changes = 0
    for k in range(1, len(cells)):
        h, hn, s = int(heads[k - 1]), int(heads[k]), int(gears[k])
        assert s in (0, 1) and (hn - h) % 8 in (0, 1, 7), "heading jumps"
        step = (int(cells[k][0] - cells[k - 1][0]), int(cells[k][1] - cells[k - 1][1]))
        want = DIRS[hn] if s == 0 else (-DIRS[h][0], -DIRS[h][1])
        assert step == want, "move does not match its gear"
        assert free[hn, cells[k][0], cells[k][1]], "path enters a blocked state"
        la, lb = length(hn if s == 0 else h)
        a += la + (tc if hn != h else 0) + (rc if s else 0)
        b += lb
        if k > 1 and s != int(gears[k - 1]):
            a += cc
            changes += 1
    return (a, b), changes


def search(fields, layers_shape, starts, goals, field_index, costs=(0, 0, 0)):
    """What nfopp_lattice_gear_trace_paths reports for problems over given fields [G, 2, 8, rows, cols, 2]: -> (cells int32
    [B, max(count, 1), 2] zero-padded, headings [B, same], gears [B, same], count [B], status [B], cost [B, 2])."""
    rows, cols = layers_shape
    B = len(starts)
    res, status, count, cost = [], np.zeros(B, np.int32), np.zeros(B, np.int32), np.full((B, 2), -1, np.int32)
    as_lists = {}                                           # nested lists index several times faster than numpy scalars
    for p in range(B):
        s, g, fi = starts[p], goals[p], int(field_index[p])
        if not (0 <= s[0] < rows and 0 <= s[1] < cols and 0 <= s[2] <= 7 and 0 <= g[0] < rows and 0 <= g[1] < cols
                and 0 <= fi < len(fields)):
            status[p] = 2
            res.append(None)
            continue
        if fi not in as_lists:
            as_lists[fi] = np.asarray(fields[fi]).tolist()
        cells, heads, gears, c = trace_path(as_lists[fi], s, costs)
        if len(cells) == 0:
            status[p] = 1
            res.append(None)
            continue
        res.append((cells, heads, gears))
        count[p], cost[p] = len(cells), c
    L = max(int(count.max(initial=0)), 1)
    out = np.zeros((B, L, 2), np.int32), np.zeros((B, L), np.int32), np.zeros((B, L), np.int32)
    for p, r in enumerate(res):
        if r is not None:
            for o, v in zip(out, r):
                o[p, :len(v)] = v
    return out + (count, status, cost)


def gear_changes(gears, count):
    """Moves 2 .. count - 1 whose gear differs from the one before."""
    g = [int(v) for v in gears[:int(count)]]
    return sum(g[k] != g[k - 1] for k in range(2, len(g)))


# ---- seeding: the body heading over the spline's parameter -------------------------------------------------------------------
def chord_parameter(path):
    """The parameter of the seeding spline at its knots, float64 [m]: fp32 segment lengths + 1e-6 and their fp32 running sum,
    every operation rounded on its own, then divided by the last in float64."""
    path = np.asarray(path, F32)
    acc, par = F32(0), [np.float64(0)]
    for i in range(len(path) - 1):
        dx, dy = F32(path[i + 1, 0] - path[i, 0]), F32(path[i + 1, 1] - path[i, 1])
        d = F32(np.sqrt(F32(F32(dx * dx) + F32(dy * dy))) + F32(1e-6))
        acc = F32(acc + d)
        par.append(np.float64(acc))
    par = np.asarray(par, np.float64)
    return par / par[-1]


def wrap(x):
    return x - (2 * np.pi) * np.rint(x / (2 * np.pi))


def heading_knots(heads, theta_start, theta_goal):
    """float64 [count + 2]: the start angle, the cells' body headings unwound from it, the goal angle unwound from the last."""
    quarter = np.float64(np.pi) / 4
    ths = np.float64(F32(theta_start))
    a1 = ths + wrap(np.float64(int(heads[0])) * quarter - ths)
    knots, u = [ths], 0
    for k in range(len(heads)):
        if k:
            u += ((int(heads[k]) - int(heads[k - 1]) + 4) % 8) - 4      # -1, 0 or +1 between the states of a lattice path
        knots.append(a1 + np.float64(u) * quarter)
    knots.append(knots[-1] + wrap(np.float64(F32(theta_goal)) - knots[-1]))
    return np.asarray(knots, np.float64)


def seed_theta(cells, heads, start, goal, boundaries, resolution, n_waypoints):
    """theta of the n waypoints, fp32.  Waypoint i has q = (i + 1) * (1 / (N + 1)) -- the product the xy spline is evaluated
    at, not the quotient (i + 1) / (N + 1) -- and lies in the knot interval k = the largest index in 0 .. m - 2 with
    PAR_k <= q; theta = A_k + (A_(k+1) - A_k) * ((q - PAR_k) / (PAR_(k+1) - PAR_k)) in float64, rounded to fp32."""
    par = chord_parameter(polyline(cells, start, goal, boundaries, resolution))
    A = heading_knots(heads, start[2], goal[2])
    step = np.float64(1.0) / np.float64(n_waypoints + 1)
    out = np.zeros(n_waypoints, F32)
    for i in range(n_waypoints):
        q = np.float64(i + 1) * step
        k = int(np.searchsorted(par[:-1], q, side="right")) - 1
        w = (q - par[k]) / (par[k + 1] - par[k])
        out[i] = F32(A[k] + (A[k + 1] - A[k]) * w)
    return out
