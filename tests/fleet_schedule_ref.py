"""The rule of nfopp_fleet_shift_masks and nfopp_fleet_assign_delays (csrc/fleet_schedule.hip, stated in include/nfopp_hip.h)
restated in numpy.  The pair predicate is tests/track_conflict_ref.py's, applied to the delayed tracks: it is not stated a second
time here.  Everything else is integers, so the device is compared with this bit for bit (tests/test_gpu_fleet_schedule.py)."""
import numpy as np

import track_conflict_ref as tr

F32 = np.float32
U64 = np.uint64
STATUS_OK, STATUS_BAD_TRACK, STATUS_UNRESOLVED, STATUS_NOT_ORDERED = 0, 1, 2, 3
MAX_DELAY_LIMIT = 63


def delay_tracks(tracks, delay, count):
    """[B, K, S] -> [B, count, S]: robot i delayed by delay[i] grid steps is at track[clamp(h - delay[i], 0, K - 1)] at instant h --
    it waits at its first sample and stays parked at its last."""
    tracks = np.asarray(tracks)
    delay = np.broadcast_to(np.asarray(delay, np.int64), (len(tracks),))
    idx = np.clip(np.arange(count)[None, :] - delay[:, None], 0, tracks.shape[1] - 1)
    return tracks[np.arange(len(tracks))[:, None], idx]


def _hit(a, b, ra, rb, margin):
    """[Ba, Bb] bool: section 17's conflict predicate (some m_k < R2, the last-instant term included) on tracks as given."""
    return tr.pairs(a, b, dt=1.0, radius_a=ra, radius_b=rb, margin=margin)["tc"] < np.inf


def bad_tracks(tracks, radius):
    t = np.asarray(tracks, F32)[:, :, :2]
    return ~(np.isfinite(t).all(axis=(1, 2)) & np.isfinite(tr._radii(radius, len(t))))


def pair_bits(tracks, max_delay, radius=None, margin=0.0):
    """[B, B, 2 * max_delay + 1] bool: C_ij(r) at index r + max_delay -- robot i delayed by max(r, 0), robot j by max(-r, 0),
    over K + |r| instants.  Zero on the diagonal and for a pair with a bad robot."""
    t = np.asarray(tracks, F32)
    B, K = t.shape[:2]
    bad = bad_tracks(t, radius)
    ok = ~bad[:, None] & ~bad[None, :] & ~np.eye(B, dtype=bool)
    out = np.zeros((B, B, 2 * max_delay + 1), bool)
    for r in range(-max_delay, max_delay + 1):
        n = K + abs(r)
        out[:, :, r + max_delay] = ok & _hit(delay_tracks(t, max(r, 0), n), delay_tracks(t, max(-r, 0), n), radius, radius, margin)
    return out


def base_bits(tracks, max_delay, radius=None, margin=0.0, obstacles=None, obstacle_radius=None):
    """[B, max_delay + 1] bool: bit d = robot i delayed by d conflicts with some good obstacle over all K + max_delay instants
    (the obstacles [M, K + max_delay, >= 2] are in absolute time and never shifted).  Zero rows for bad robots."""
    t = np.asarray(tracks, F32)
    B, K = t.shape[:2]
    out = np.zeros((B, max_delay + 1), bool)
    if obstacles is None or len(obstacles) == 0:
        return out
    o = np.asarray(obstacles, F32)
    assert o.shape[1] == K + max_delay
    ok = ~bad_tracks(t, radius)[:, None] & ~bad_tracks(o, obstacle_radius)[None, :]
    for d in range(max_delay + 1):
        out[:, d] = (ok & _hit(delay_tracks(t, d, K + max_delay), o, radius, obstacle_radius, margin)).any(axis=1)
    return out


def pack(bits):
    """[..., n <= 128] bool -> [..., 2] uint64, bit p in word p // 64 (little-endian words); unused high bits 0."""
    n = bits.shape[-1]
    assert n <= 128
    full = np.zeros(bits.shape[:-1] + (128,), bool)
    full[..., :n] = bits
    w = (full.reshape(bits.shape[:-1] + (2, 64)).astype(U64) << np.arange(64, dtype=U64)).sum(axis=-1, dtype=U64)
    return w


def unpack(words, n):
    """[..., 2] uint64 -> [..., n] bool."""
    words = np.asarray(words, U64)
    bits = ((words[..., :, None] >> np.arange(64, dtype=U64)) & U64(1)).astype(bool)
    return bits.reshape(words.shape[:-1] + (128,))[..., :n]


def shift_masks(tracks, max_delay, radius=None, margin=0.0, obstacles=None, obstacle_radius=None):
    """-> dict(pair [B, B, 2] uint64, base [B] uint64, bad [B] int32, pair_bits, base_bits)."""
    assert 0 <= max_delay <= MAX_DELAY_LIMIT
    pb = pair_bits(tracks, max_delay, radius, margin)
    bb = base_bits(tracks, max_delay, radius, margin, obstacles, obstacle_radius)
    return dict(pair=pack(pb), base=pack(bb)[..., 0], bad=bad_tracks(tracks, radius).astype(np.int32), pair_bits=pb, base_bits=bb,
                max_delay=max_delay)


def assign(masks, order=None):
    """The assignment pass on `shift_masks`' result -> dict(delay [B] int32, status [B] int32, forbidden [B] uint64)."""
    pb, bb, bad, md = masks["pair_bits"], masks["base_bits"], masks["bad"], masks["max_delay"]
    B, D = len(bad), md + 1
    order = np.arange(B, dtype=np.int32) if order is None else np.asarray(order, np.int32)
    assert order.shape == (B,)
    delay = np.full(B, -1, np.int32)
    status = np.full(B, STATUS_NOT_ORDERED, np.int32)
    forbidden = np.zeros((B, D), bool)
    visited = np.zeros(B, bool)
    for i in order:
        if i < 0 or i >= B or visited[i]:
            continue
        visited[i] = True
        if bad[i]:
            status[i] = STATUS_BAD_TRACK
            continue
        f = bb[i].copy()
        for j in np.flatnonzero(delay >= 0):
            # mask_ij >> (max_delay - delay_j), low D bits: bit d is C_ij(d - delay_j)
            lo = md - int(delay[j])
            f |= pb[i, j, lo:lo + D]
        forbidden[i] = f
        free = np.flatnonzero(~f)
        if len(free):
            delay[i], status[i] = free[0], STATUS_OK
        else:
            status[i] = STATUS_UNRESOLVED
    return dict(delay=delay, status=status, forbidden=pack(forbidden)[..., 0])


def schedule(tracks, max_delay, radius=None, margin=0.0, obstacles=None, obstacle_radius=None, order=None):
    m = shift_masks(tracks, max_delay, radius, margin, obstacles, obstacle_radius)
    return m, assign(m, order)
