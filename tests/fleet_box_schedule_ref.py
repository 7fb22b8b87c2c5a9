"""The rule of nfopp_fleet_box_shift_masks (csrc/fleet_box_schedule.hip, stated in include/nfopp_hip.h) restated in numpy.  The
pair predicate is tests/box_conflict_ref.py's `pairs`, applied to the delayed tracks and their unit vectors, and the packing and
the assignment pass are tests/fleet_schedule_ref.py's: nothing about the box rule, the masks or the assignment is stated a
second time here.  The device is compared with this bit for bit on the device's own unit vectors
(tests/test_gpu_fleet_box_schedule.py)."""
import numpy as np

import box_conflict_ref as br
import fleet_schedule_ref as fr

F32, F64 = np.float32, np.float64
STATUS_OK, STATUS_BAD_TRACK, STATUS_UNRESOLVED, STATUS_NOT_ORDERED = (fr.STATUS_OK, fr.STATUS_BAD_TRACK, fr.STATUS_UNRESOLVED,
                                                                      fr.STATUS_NOT_ORDERED)


def _forbidden(status):
    """not FREE: CONFLICT or UNDECIDED (a pair with a bad track is nobody's)."""
    return (status == br.CONFLICT) | (status == br.UNDECIDED)


def pair_bits(tracks, units, max_delay, *, box, radius=None, margin=0.0, refine=0):
    """[B, B, 2 * max_delay + 1] bool: C_ij(r) at index r + max_delay -- one call of `box_conflict_ref.pairs` in two-set mode
    per r, all tracks delayed by max(r, 0) as A and all delayed by max(-r, 0) as B over K + |r| instants, the unit vectors
    gathered with the tracks; status[i, j] is kept for i < j (i the first box) and mirrored: bit -r of (j, i) is bit r of (i, j)."""
    t, u = np.asarray(tracks, F32), np.asarray(units, F64)
    B, K = t.shape[:2]
    out = np.zeros((B, B, 2 * max_delay + 1), bool)
    upper = np.triu(np.ones((B, B), bool), 1)
    for r in range(-max_delay, max_delay + 1):
        n, da, db = K + abs(r), max(r, 0), max(-r, 0)
        p = br.pairs(fr.delay_tracks(t, da, n), fr.delay_tracks(u, da, n), fr.delay_tracks(t, db, n), fr.delay_tracks(u, db, n),
                     dt=1.0, box_a=box, box_b=box, radius_a=radius, radius_b=radius, margin=margin, refine=refine)
        hit = _forbidden(p["status"]) & upper
        out[:, :, max_delay + r] |= hit
        out[:, :, max_delay - r] |= hit.T
    return out


def bad_tracks(tracks, units, box, radius):
    """[B] bool: the box check's BAD flag (read off `pairs` on the tracks as they are)."""
    return br.pairs(tracks, units, dt=1.0, box_a=box, radius_a=radius)["bad_a"]


def base_bits(tracks, units, max_delay, *, box, radius=None, margin=0.0, refine=0, obstacles=None, obstacle_units=None, obstacle_box=None,
              obstacle_radius=None):
    """[B, max_delay + 1] bool: bit d = robot i delayed by d (the first box) is not FREE against some good obstacle (the second)
    over all K + max_delay instants; the obstacles are in absolute time and never shifted."""
    t, u = np.asarray(tracks, F32), np.asarray(units, F64)
    B, K = t.shape[:2]
    out = np.zeros((B, max_delay + 1), bool)
    if obstacles is None or len(obstacles) == 0:
        return out
    o = np.asarray(obstacles, F32)
    assert o.shape[1] == K + max_delay
    for d in range(max_delay + 1):
        p = br.pairs(fr.delay_tracks(t, d, K + max_delay), fr.delay_tracks(u, d, K + max_delay), o, obstacle_units, dt=1.0, box_a=box,
                     box_b=obstacle_box, radius_a=radius, radius_b=obstacle_radius, margin=margin, refine=refine)
        out[:, d] = _forbidden(p["status"]).any(axis=1)
    return out


def shift_masks(tracks, units, max_delay, *, box, radius=None, margin=0.0, refine=0, obstacles=None, obstacle_units=None,
                obstacle_box=None, obstacle_radius=None):
    """-> dict(pair [B, B, 2] uint64, base [B] uint64, bad [B] int32, pair_bits, base_bits, max_delay): what
    `fleet_schedule_ref.assign` reads."""
    assert 0 <= max_delay <= fr.MAX_DELAY_LIMIT
    pb = pair_bits(tracks, units, max_delay, box=box, radius=radius, margin=margin, refine=refine)
    bb = base_bits(tracks, units, max_delay, box=box, radius=radius, margin=margin, refine=refine, obstacles=obstacles,
                   obstacle_units=obstacle_units, obstacle_box=obstacle_box, obstacle_radius=obstacle_radius)
    bad = bad_tracks(tracks, units, box, radius)
    return dict(pair=fr.pack(pb), base=fr.pack(bb)[..., 0], bad=bad.astype(np.int32), pair_bits=pb, base_bits=bb, max_delay=max_delay)


assign = fr.assign
