"""Cases for the space-time grid search tests (tests/test_spacetime_cpu.py on the restatement, tests/test_gpu_spacetime.py on
the device).  A case is a dict(occ [rows, cols] uint8, geo, T, robot_radius, margin, tracks [M, T, S] or None, radius [M],
visible [M] uint8 or None, starts / goals [R, 2] (row, col), order [R] int32 or None).  Hand cases are on dyadic geometry
(res = 1, origin 0, radius 0.25, margin 0, so R = 0.5 against another planned robot or a mover of radius 0.25)."""
import numpy as np

import fleet_schedule_cases as fc
import spacetime_ref as sr

F32 = np.float32
FAR = 64.0   # where a mover of a hand case is while it is "away"


def case(occ, T, starts, goals, tracks=None, radius=None, visible=None, order=None, robot_radius=0.25, margin=0.0, b0=0.0, b2=0.0,
         res=1.0):
    occ = np.ascontiguousarray(np.asarray(occ) != 0, dtype=np.uint8)
    geo = sr.Geometry(occ.shape[0], occ.shape[1], b0, b2, res)
    if tracks is not None:
        tracks = np.asarray(tracks, F32)
        radius = np.broadcast_to(np.asarray(0.25 if radius is None else radius, F32), (len(tracks),)).copy()
        assert tracks.shape[1] == T
    return dict(occ=occ, geo=geo, T=int(T), robot_radius=float(F32(robot_radius)), margin=float(margin), tracks=tracks, radius=radius,
                visible=None if visible is None else np.asarray(visible, np.uint8),
                starts=np.asarray(starts, np.int32).reshape(-1, 2), goals=np.asarray(goals, np.int32).reshape(-1, 2),
                order=None if order is None else np.asarray(order, np.int32))


def reservation(c):
    """The restatement's reservation of case `c` with its movers in."""
    res = sr.Reservation(c["occ"], c["geo"], c["T"], c["robot_radius"], c["margin"])
    if c["tracks"] is not None and len(c["tracks"]):
        res.add(c["tracks"], c["radius"], c["visible"])
    return res


def solve(c):
    """-> (reservation before planning, reservation after, plan) of the restatement."""
    before = reservation(c)
    after = before.copy()
    return before, after, sr.plan_fleet(after, c["starts"], c["goals"], c["order"])


def standing(cell, instants, T, away=(0.5, FAR)):
    """[T, 2]: a mover that stands on the centre of `cell` (row, col; res = 1, origin 0) during `instants` and is far away
    otherwise."""
    out = np.tile(np.asarray(away, F32), (T, 1))
    out[list(instants)] = (cell[1] + 0.5, cell[0] + 0.5)
    return out


def corridor(T=12, bay=True, order=None):
    occ = np.ones((3, 7), np.uint8)
    occ[1, :] = 0
    occ[0, 3] = 0 if bay else 1
    return case(occ, T, [(1, 0), (1, 6)], [(1, 6), (1, 0)], order=order)


def gate(T=12):
    return case(np.zeros((1, 8)), T, [(0, 0)], [(0, 7)], tracks=[standing((0, 4), range(2, 7), T)])


def parked_on_goal(T=10, leaves=None):
    """A mover comes to stand on the goal cell (0, 3) at instant 2: for good, or until it leaves at instant `leaves`."""
    return case(np.zeros((1, 4)), T, [(0, 0)], [(0, 3)], tracks=[standing((0, 3), range(2, T if leaves is None else leaves), T)])


def single_instant(goal, mover_on_goal):
    return case(np.zeros((1, 3)), 1, [(0, 0)], [goal], tracks=[standing((0, 0) if mover_on_goal else (0, 2), [0], 1)])


def strict(closer, T=3):
    """A standing mover exactly R = 0.5 from the centres of cells (0, 0) and (0, 1), or one fp32 step closer to cell (0, 0)."""
    x = float(np.nextafter(F32(1.0), F32(0.0))) if closer else 1.0
    return case(np.zeros((1, 3)), T, [(0, 0)], [(0, 0)], tracks=[np.tile(np.array([x, 0.5], F32), (T, 1))])


# rows x cols x T x movers x robots of the device comparison: the smallest cases, a row of 63 / 64 / 65 cells (one word and the
# word boundary), the size of the re-planning example, and three words a row with more movers than the reserve kernel stages
# per trip (16).  The last has more CELLS (5200) than the search kernel has threads, but only rows * words = 120 WORDS, which is
# what that kernel's loops run over: the sizes past one trip of it are EDGES, below
SIZES = ((1, 1, 1, 0, 1), (1, 2, 2, 1, 1), (3, 7, 8, 0, 2), (5, 63, 9, 2, 3), (5, 64, 9, 3, 3), (5, 65, 9, 3, 3), (24, 24, 41, 8, 8),
         (40, 130, 33, 17, 17))
STRIDES = (2, 3, 4, 2, 3, 4, 3, 2)
WALLS = (False, False, True, True, False, True, False, True)


def sized_case(n, seed=0):
    """Case n of SIZES: non-dyadic geometry, movers that cross the floor on straight lines, random free start and goal cells,
    random walls at about 20 % (WALLS), rows of STRIDES[n] floats with junk behind y, (3 movers or more) a bad mover, a mover with
    a NaN radius and an invisible one, and (3 robots or more) a robot that starts outside the image or on a wall."""
    rows, cols, T, m, r = SIZES[n]
    rng = np.random.default_rng(1000 * n + seed)
    res, b0, b2 = 0.1, -0.3, 0.2
    occ = np.zeros((rows, cols), np.uint8)
    if WALLS[n]:
        occ = (rng.uniform(size=(rows, cols)) < 0.2).astype(np.uint8)
    free = np.argwhere(occ == 0)
    # distinct starts where the floor has room; a goal within reach of its start in about half the instants
    starts = free[rng.permutation(len(free))[:r]] if len(free) >= r else free[rng.integers(0, len(free), r)]
    near = max((T - 1) // 2, 1)
    goals = np.stack([(lambda ok: ok[rng.integers(0, len(ok))])(free[np.abs(free - s).max(axis=1) <= near]) for s in starts])
    if r >= 3:   # a robot that starts outside the image or on a wall
        walls = np.argwhere(occ != 0)
        starts[r - 1] = walls[0] if len(walls) and n % 2 else (-1, 2)
    tracks = radius = visible = None
    if m:
        lo = np.array([b0, b2])
        hi = lo + res * np.array([cols, rows])
        p0, p1 = rng.uniform(lo, hi, (m, 2)), rng.uniform(lo, hi, (m, 2))
        if m >= 2:   # mover 1 ends in the last cell of the last row, mover 2 starts in the first of the first: the ends of a row's words
            p1[1] = lo + res * (np.array([cols, rows]) - 0.5)
        if m >= 3:
            p0[2] = lo + res * 0.5
        lam = (np.arange(T) / max(T - 1, 1))[None, :, None]
        tracks = (p0[:, None] * (1 - lam) + p1[:, None] * lam).astype(F32)
        radius = rng.uniform(0.3, 0.9, m).astype(F32) * F32(res)
        if m >= 3:   # three kinds of mover that must be skipped: all three from 8 movers on, one in rotation below that
            kinds = ((m // 2, 0, m - 1) if m >= 8 else tuple(0 if n % 3 == k else None for k in range(3)))
            visible = np.ones(m, np.uint8)
            if kinds[0] is not None:
                tracks[kinds[0], (T - 1) // 2, 1] = np.inf
            if kinds[1] is not None:
                radius[kinds[1]] = np.nan
            if kinds[2] is not None:
                visible[kinds[2]] = 0
    c = case(occ, T, starts, goals, tracks=tracks, radius=radius, visible=visible, robot_radius=0.35 * res, margin=0.01, b0=b0, b2=b2,
             res=res)
    if tracks is not None:
        c["tracks"] = fc.with_stride(dict(tracks=tracks, obstacles=None), STRIDES[n], seed=n)["tracks"]
    return c


def orders(r, seed=0):
    return fc.orders(r, seed)


# ---- the sizes past one trip of the plan kernels' loops, and the largest frontier ----------------------------------------------
# The constants of csrc/spacetime_search.hip these cases are sized by, restated (tests/test_spacetime_cpu.py reads them back
# from the source and computes what each case reaches): a constant that moves there names the case to replace here.
SEARCH_THREADS = 1024            # `constexpr int ST_SEARCH_THREADS = 1024;`: the stride of st_search_kernel over words and instants
INIT_GRID, INIT_THREADS = 2048, 256   # `init_blocks < 2048 ? init_blocks : 2048` in nfopp_spacetime_plan_fleet, `ST_THREADS = 256`
LDS_BYTES = 160 * 1024           # `NFOPP_REQUIRE(lds <= 160 * 1024, "frontier too large ...` in nfopp_spacetime_plan_fleet
SEARCH_HEAD = 64                 # `constexpr int ST_SEARCH_HEAD = 64;`: lds = ST_SEARCH_HEAD + 2 * rows * words * 8
LARGEST_RW = (LDS_BYTES - SEARCH_HEAD) // 16   # 10236 words: exactly 160 KiB


def words_past_one_trip():
    """1040 x 3, T = 24: one word a row, rows * words = 1040 > 1024 -- the word loop of the search takes a second trip.  A mover
    stands on (1030, 1) throughout; robot 0 goes down column 1 past it, robot 1 comes up from the last row."""
    T = 24
    return case(np.zeros((1040, 3)), T, [(1018, 1), (1039, 0)], [(1036, 1), (1025, 2)], tracks=[standing((1030, 1), range(T), T)])


def carry_past_one_trip():
    """513 x 65, T = 6: two words a row, rows * words = 1026.  The one robot crosses from column 63 to column 64 in the last rows:
    the bit arrives in word 1025 from word 1024, the neighbour-word carry of a second trip."""
    return case(np.zeros((513, 65)), 6, [(510, 60)], [(512, 64)])


def visited_goal(T=1100, comes=1030, leaves=1041):
    """1 x 4: the robot stands on its goal from instant 3 on, until a mover comes to stand there during comes .. leaves - 1; it
    steps aside and is back at `leaves`.  In the parked_on_goal cases the goal is not REACHED before the mover has left, so the
    arrival does not depend on the park scan; here reach holds at the goal from instant 3 on, and only a park scan that
    finds the blocked wait edge at leaves - 1 >= 1024 -- in its second trip -- keeps the arrival from being 3."""
    return case(np.zeros((1, 4)), T, [(0, 0)], [(0, 3)], tracks=[standing((0, 3), range(comes, leaves), T)])


def many_robots(robots=513, T=1025):
    """1 x 4, T = 1025, 513 robots: robots * T = 525825 entries for st_plan_init_kernel's 524288 threads.  `order` visits three
    robots (the last, one of the first, one in the middle), at positions 0, 7 and the last; everyone else keeps what the init
    kernel wrote."""
    starts, goals = np.zeros((robots, 2), np.int32), np.zeros((robots, 2), np.int32)
    visited = [robots - 1, 5, robots // 2]
    starts[visited, 1], goals[visited, 1] = (0, 3, 2), (1, 3, 2)
    order = np.full(robots, -1, np.int32)
    order[[0, 7, robots - 1]] = visited
    return case(np.zeros((1, 4)), T, starts, goals, order=order)


def largest_frontier(rows=LARGEST_RW):
    """rows x 1, T = 3: at 10236 rows both frontiers and the head are exactly 160 KiB of dynamic LDS.  One robot goes from the
    last row but one to the last."""
    return case(np.zeros((rows, 1)), 3, [(rows - 2, 0)], [(rows - 1, 0)])


# name -> (the case, statuses, arrivals of the robots `order` visits, in index order)
EDGES = {
    "1040x3": (words_past_one_trip, [0, 0], [18, 14]),
    "513x65": (carry_past_one_trip, [0], [4]),
    "T=1025": (lambda: parked_on_goal(T=1025, leaves=1024), [0], [1024]),      # hb = 1023 in the first trip, ha = 1024 in the second
    "T=1026": (lambda: parked_on_goal(T=1026, leaves=1025), [0], [1025]),      # hb = 1024: both in the second
    "T=1100": (lambda: parked_on_goal(T=1100, leaves=1060), [0], [1060]),
    "T=1100-back":(visited_goal, [0], [1041]),                               # reached at 3; hb = 1040 is what delays the arrival
    "R=513": (many_robots, [0, 0, 0], [0, 0, 1]),
    "10236x1": (largest_frontier, [0], [1]),
}


def edge_case(name):
    return EDGES[name][0]()


def circle_replan_odd():
    """The circle fleet with a NaN planted in robot 5's track and an odd schedule order (a repeat, a -1, a value >= B): the
    schedule then holds SCHEDULE_BAD_TRACK and SCHEDULE_NOT_ORDERED robots beside scheduled and unresolved ones."""
    case, geo, count = circle_replan()
    case = fc.with_bad(case, robots=(5,))
    return dict(case, order=fc.orders(16, seed=3)["odd"]), geo, count


def circle_replan():
    """The circle family of the schedule tests at 16 robots x 18 instants with 8 candidate delays (fleet_schedule_cases.circle(16,
    18, 7): 8 of 16 unresolved), and the wall-free 24 x 24 grid of 0.25 m over 41 instants the unresolved ones are re-planned on
    -> (schedule case, grid geometry, count)."""
    return fc.circle(16, 18, 7), sr.Geometry(24, 24, -3.0, -3.0, 0.25), 41


def replan_ref(sc, schedule, geo, count, occ=None, margin="snap"):
    """The restatement of FleetSchedule.replan on a schedule case `sc` and its restated `schedule` -> (case, plan, merged [B,
    count, 2]): the scheduled robots' delayed tracks are the movers, the UNRESOLVED ones go from the cell of their first sample
    to the cell of their last, in index order; a robot with a bad track or one the schedule never visited is not searched.
    merged holds NaN rows for a robot that is neither scheduled nor planned."""
    import fleet_schedule_ref as fr
    tracks = np.asarray(sc["tracks"], F32)[:, :, :2]
    b = len(tracks)
    on = schedule["status"] == 0
    moved = fr.delay_tracks(tracks, np.maximum(schedule["delay"], 0), count).astype(F32)

    def cells_of(p):
        p = np.where(np.isfinite(p), p, 0)      # a bad track has no cells; it is never searched, any value serves
        return np.stack([np.floor((p[:, 1].astype(np.float64) - geo.b2) / geo.res), np.floor((p[:, 0].astype(np.float64) - geo.b0) / geo.res)],
                        1).astype(np.int32)
    if margin == "snap":
        margin = sc["margin"] + geo.res / np.sqrt(2.0)
    radius = sc["radius"]
    assert (radius == radius[0]).all()
    order = np.where(schedule["status"] == fr.STATUS_UNRESOLVED, np.arange(b), -1).astype(np.int32)
    c = case(np.zeros((geo.rows, geo.cols)) if occ is None else occ, count, cells_of(tracks[:, 0]), cells_of(tracks[:, -1]), tracks=moved,
             radius=radius, visible=on.astype(np.uint8), order=order, robot_radius=radius[0], margin=margin, b0=geo.b0, b2=geo.b2, res=geo.res)
    _, _, plan = solve(c)
    merged = np.where((plan["status"] == 0)[:, None, None], plan["tracks"], np.where(on[:, None, None], moved, F32(np.nan)))
    return c, plan, merged
