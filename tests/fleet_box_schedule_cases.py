"""Fleets of cars for the box schedule tests (tests/test_fleet_box_schedule_cpu.py on the restatement,
tests/test_gpu_fleet_box_schedule.py on the device).  A case is a dict(tracks [B, K, S >= 3] fp32 (x, y, theta), units [B, K, 2]
float64, max_delay, box [B, 4], radius [B], margin, obstacles [M, K + max_delay, S] or None, obstacle_units, obstacle_box,
obstacle_radius); hand cases are on dyadic coordinates, carry `expect`, and take their unit vectors from the fp32 headings as
the headings pass does: theta = fl32(pi) is not pi, the lanes' boxes are a hair (1e-7) closer than 0.25 m, and the tie that exact
unit vectors would leave at the first halving (0.5 - 0.5 >= 0) is not there.

Hand cases (box CAR = (-1, 1, -0.5, 0.5), circumscribed disc sqrt(1.25), margin 0):
  lanes     two cars pass in neighbouring lanes 1.25 m apart: every disc bit is set; the boxes are 0.25 m apart, and the
            certificate needs two halvings (relative motion 1 m per interval against a gap sum of 0.5)
  convoy    two cars in one lane, 2.125 m centre to centre: the discs overlap for every shift; the boxes only when the car
            behind leaves earlier
  crossing  a perpendicular crossing: boxes and discs agree
The random family is box_conflict_cases.car_tracks with per-track boxes and radii and margin 0.0625, on a floor whose
`extent` is chosen per size so that the share of set off-diagonal bits lies in [0.1, 0.9] (`density`): a mask of all zeros
or all ones would pass otherwise."""
import numpy as np

import box_conflict_cases as bc
import box_conflict_ref as br
import fleet_box_schedule_ref as xr
import fleet_schedule_ref as fr

F32, F64 = np.float32, np.float64
CAR = bc.CAR
DISC = float(np.sqrt(1.25))
UNRESOLVED = fr.STATUS_UNRESOLVED


def bits(text):
    """"11111000000" -> [bool]: the character at index p is bit p (index = shift + max_delay)."""
    return [ch == "1" for ch in text]


def case(tracks, units, max_delay, box=CAR, radius=0.0, margin=0.0, obstacles=None, obstacle_units=None, obstacle_box=None,
         obstacle_radius=None, **expect):
    tracks, units = np.asarray(tracks, F32), np.asarray(units, F64)
    b = len(tracks)
    c = dict(tracks=tracks, units=units, max_delay=int(max_delay), box=np.broadcast_to(np.asarray(box, F32).reshape(-1, 4), (b, 4)).copy(),
             radius=np.broadcast_to(np.asarray(radius, F32), (b,)).copy(), margin=float(margin), obstacles=None, obstacle_units=None,
             obstacle_box=None, obstacle_radius=None, expect=expect)
    if obstacles is not None:
        m = len(obstacles)
        c.update(obstacles=np.asarray(obstacles, F32), obstacle_units=np.asarray(obstacle_units, F64),
                 obstacle_box=np.broadcast_to(np.asarray(box if obstacle_box is None else obstacle_box, F32).reshape(-1, 4), (m, 4)).copy(),
                 obstacle_radius=np.broadcast_to(np.asarray(0.0 if obstacle_radius is None else obstacle_radius, F32), (m,)).copy())
    return c


def kwargs(c, refine=0):
    """The keyword arguments of fleet_box_schedule_ref.shift_masks for case `c`."""
    return dict(box=c["box"], radius=c["radius"], margin=c["margin"], refine=refine, obstacles=c["obstacles"],
                obstacle_units=c["obstacle_units"], obstacle_box=c["obstacle_box"], obstacle_radius=c["obstacle_radius"])


def solve(c, refine=0, order=None):
    """-> (masks, schedule) of the restatement."""
    m = xr.shift_masks(c["tracks"], c["units"], c["max_delay"], **kwargs(c, refine))
    return m, xr.assign(m, order)


def disc_solve(c, order=None):
    """The disc schedule on the same tracks: every car as its circumscribed disc."""
    m = fr.shift_masks(c["tracks"], c["max_delay"], radius=np.full(len(c["tracks"]), DISC, F32), margin=c["margin"])
    return m, fr.assign(m, order)


def _fleet(*tracks):
    t = np.stack([x[0] for x in tracks])
    return t, br.unit_vectors(t)


def hand_cases():
    """name -> case; expect: per refine the bits of pair (0, 1), the delays and statuses in the identity order (and, where
    given, in the order [1, 0]), and the same for the disc schedule."""
    out = {}
    h = np.arange(17.0)
    t, u = _fleet(bc.track(-4.0 + 0.5 * h, 0.0, bc.EAST), bc.track(4.0 - 0.5 * h, 1.25, bc.WEST))
    out["lanes"] = case(t, u, 7, refines={0: ("1" * 15, [0, -1], [0, UNRESOLVED]), 1: ("1" * 15, [0, -1], [0, UNRESOLVED]),
                                          2: ("0" * 15, [0, 0], [0, 0])},
                        disc=("1" * 15, [0, -1], [0, UNRESOLVED]))
    h = np.arange(9.0)
    t, u = _fleet(bc.track(0.5 * h, 0.0, bc.EAST), bc.track(0.5 * h + 2.125, 0.0, bc.EAST))
    out["convoy"] = case(t, u, 5, refines={0: ("11111000000", [0, 0], [0, 0])}, disc=("1" * 11, [0, -1], [0, UNRESOLVED]),
                         reordered={0: ([0, 0], [0, 0])}, disc_reordered=([-1, 0], [UNRESOLVED, 0]))
    h = np.arange(17.0)
    t, u = _fleet(bc.track(-4.0 + 0.5 * h, 0.0, bc.EAST), bc.track(0.0, -4.0 + 0.5 * h, bc.NORTH))
    cross = "0000000001111111111111000000000"
    out["crossing"] = case(t, u, 15, refines={0: (cross, [0, 7], [0, 0])}, disc=(cross, [0, 7], [0, 0]))
    return out


def with_stride(c, stride, seed=0):
    """The case with rows of `stride` floats: columns 3.. hold junk (NaN among it) that must not be read."""
    w = bc.with_stride(dict(a=c["tracks"], b=c["obstacles"]), stride, seed)
    return dict(c, tracks=w["a"], obstacles=w["b"])


def random_case(seed, b, k, max_delay, m=0, stride=3, extent=3.0, bad=False):
    """B cars (box_conflict_cases.car_tracks) on an `extent`-metre floor with per-track boxes and radii, margin 0.0625, and M
    obstacle cars over K + max_delay instants.  `bad` plants each kind of badness once, as far as the sizes allow: robots -- a
    NaN x, an infinite heading, a box with x0 >= x1, a negative radius; obstacles -- an infinite y, a NaN box entry, y0 >= y1,
    a NaN radius.  The unit vectors are numpy's: the GPU test replaces them with the device's."""
    rng = np.random.default_rng(seed)

    def boxes(n):
        bx = (np.tile(np.asarray(bc.SWEPT_BOX, F32), (n, 1)) * rng.uniform(0.6, 1.4, (n, 1))).astype(F32)
        bx[:, 1] += rng.uniform(0.0, 0.2, n).astype(F32)
        return bx
    tracks = bc.car_tracks(rng, b, k, extent)
    box, radius = boxes(b), rng.uniform(0.0, 0.1, b).astype(F32)
    c = dict(tracks=tracks, units=None, max_delay=int(max_delay), box=box, radius=radius, margin=bc.RANDOM_MARGIN, obstacles=None,
             obstacle_units=None, obstacle_box=None, obstacle_radius=None, expect={})
    if m:
        c.update(obstacles=bc.car_tracks(rng, m, k + max_delay, extent), obstacle_box=boxes(m),
                 obstacle_radius=rng.uniform(0.0, 0.1, m).astype(F32))
    if bad:
        if b > 2:
            tracks[b // 2, k // 2, 0] = np.nan
        if b > 4:
            tracks[1, k - 1, 2] = np.inf
            box[b - 1, 0] = box[b - 1, 1]
        if b > 6:
            radius[3] = -0.0625
        if m > 2:
            c["obstacles"][0, k + max_delay - 1, 1] = -np.inf
        if m > 4:
            c["obstacle_box"][1, 2] = np.nan
            c["obstacle_box"][2, 3] = c["obstacle_box"][2, 2]
            c["obstacle_radius"][m - 1] = np.nan
    c = with_stride(c, stride, seed)
    c["units"] = br.unit_vectors(c["tracks"])
    c["obstacle_units"] = None if not m else br.unit_vectors(c["obstacles"])
    return c


def density(masks):
    """The share of set bits among the off-diagonal pairs of good robots (NaN without such a pair)."""
    pb, good = masks["pair_bits"], masks["bad"] == 0
    on = good[:, None] & good[None, :] & ~np.eye(len(good), dtype=bool)
    return float(pb[on].mean()) if on.any() else float("nan")


# (B, K, max_delay) of the device comparison: one robot, one pair, tile edges at 8 (the scheduler's tile) and 32, the 64-bit
# word boundary at 2 * 32 + 1 = 65 bits, the full 127 bits; K = 1 and 2, and 9 and 17 on either side of the 16-instant chunk
SIZES = ((1, 1, 0), (2, 2, 1), (3, 5, 3), (9, 17, 31), (9, 9, 32), (33, 9, 63), (40, 3, 7))
# what rotates over the sizes: refinement depth, row stride, obstacles; the floor per size, chosen for `density` in [0.1, 0.9]
REFINES = (0, 1, 3, 3, 0, 1, 3)
STRIDES = (3, 5, 3, 5, 3, 5, 3)
OBSTACLES = (0, 1, 9, 0, 9, 0, 1)
EXTENTS = (3.0, 2.0, 2.5, 4.0, 4.0, 8.0, 6.0)
SEEDS = (0, 22, 7, 3, 4, 5, 6)


def sized_case(n):
    b, k, md = SIZES[n]
    return random_case(SEEDS[n], b, k, md, m=OBSTACLES[n], stride=STRIDES[n], extent=EXTENTS[n], bad=True)
