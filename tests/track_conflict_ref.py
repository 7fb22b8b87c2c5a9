"""The rule of nfopp_track_conflicts (csrc/track_conflict.hip, stated in include/nfopp_hip.h) restated in numpy: every
operation is a separate float64 numpy operation in the header's order, a loop over the intervals, vectorised over the pairs.
The device is compared with this bit for bit (tests/test_gpu_track_conflict.py)."""
import numpy as np

F32, F64 = np.float32, np.float64
NUM_SLOTS = 7
SLOT_MIN_GAP, SLOT_MIN_PARTNER, SLOT_MIN_TIME, SLOT_FIRST_TIME, SLOT_FIRST_PARTNER, SLOT_CONFLICTS, SLOT_STATUS = range(NUM_SLOTS)
STATUS_BAD_TRACK, STATUS_NO_PARTNER = 1, 2
INF = np.inf


def _radii(r, n):
    """None, a number or [n] -> float64 [n] of fp32 values."""
    if r is None:
        return np.zeros(n, F64)
    return np.broadcast_to(np.asarray(r, F32).reshape(-1), (n,)).astype(F64)


def instant(t0, k, dt):
    """t_k = t0 + k * dt: the product rounded, then the sum."""
    return F64(t0) + F64(k) * F64(dt)


def pairs(tracks_a, tracks_b=None, *, dt, t0=0.0, radius_a=None, radius_b=None, margin=0.0):
    """All pairs.  tracks [B, K, >= 2] of fp32 values (columns past the second are not read); tracks_b None = self mode.
    -> dict: M, tstar, gap, tc [Ba, Bb]; bad_a [Ba], bad_b [Bb]; partner [Ba, Bb] bool (a good pair, not the diagonal);
    R, R2; `branches`: how often each branch of the rule was taken on good pairs."""
    self_mode = tracks_b is None
    a32 = np.asarray(tracks_a, F32)
    b32 = a32 if self_mode else np.asarray(tracks_b, F32)
    ra = _radii(radius_a, len(a32))
    rb = ra if self_mode else _radii(radius_b, len(b32))
    ba, K = a32.shape[:2]
    bb = len(b32)
    assert K >= 1 and b32.shape[1] == K
    pa, pb = a32[:, :, :2].astype(F64), b32[:, :, :2].astype(F64)
    bad_a = ~(np.isfinite(pa).all(axis=(1, 2)) & np.isfinite(ra))
    bad_b = ~(np.isfinite(pb).all(axis=(1, 2)) & np.isfinite(rb))
    good = ~bad_a[:, None] & ~bad_b[None, :]
    partner = good & ~np.eye(ba, dtype=bool) if self_mode else good
    dt, t0, margin = F64(dt), F64(t0), F64(margin)
    R = (ra[:, None] + rb[None, :]) + margin
    R2 = R * R
    shape = (ba, bb)
    M, ks, ss, tc = np.full(shape, INF), np.zeros(shape, np.int64), np.zeros(shape), np.full(shape, INF)
    last_only = np.zeros(shape, bool)
    br = dict(a_zero=0, b_nonneg=0, end=0, interior=0, start_inside=0, root=0, disc_clamped=0, disc_positive=0, last_term_only=0)
    with np.errstate(all="ignore"):
        dx = pa[:, None, :, 0] - pb[None, :, :, 0]
        dy = pa[:, None, :, 1] - pb[None, :, :, 1]
        for k in range(K - 1):
            d0x, d0y, d1x, d1y = dx[:, :, k], dy[:, :, k], dx[:, :, k + 1], dy[:, :, k + 1]
            wx, wy = d1x - d0x, d1y - d0y
            c = d0x * d0x + d0y * d0y
            a = wx * wx + wy * wy
            b = d0x * wx + d0y * wy
            e = d1x * d1x + d1y * d1y
            first = (a == 0.0) | (b >= 0.0)
            end = ~first & (-b >= a)
            s_int = (-b) / a
            px, py = d0x + s_int * wx, d0y + s_int * wy
            m_int = px * px + py * py
            s = np.where(first, 0.0, np.where(end, 1.0, s_int))
            m = np.where(first, c, np.where(end, e, m_int))
            upd = m < M
            M, ks, ss = np.where(upd, m, M), np.where(upd, k, ks), np.where(upd, s, ss)
            hit = (m < R2) & ~(tc < INF)
            bsq = b * b
            cr = c - R2
            acr = a * cr
            disc = bsq - acr
            clamped = ~(disc > 0.0)
            disc = np.where(disc > 0.0, disc, 0.0)
            s_in = ((-b) - np.sqrt(disc)) / a
            s_in = np.where(s_in > 0.0, s_in, 0.0)
            s_in = np.where(s_in < s, s_in, s)
            inside = c < R2
            s_in = np.where(inside, 0.0, s_in)
            tc = np.where(hit, instant(t0, k, dt) + s_in * dt, tc)
            g = partner
            br["a_zero"] += int((g & (a == 0.0)).sum())
            br["b_nonneg"] += int((g & (a != 0.0) & (b >= 0.0)).sum())
            br["end"] += int((g & end).sum())
            br["interior"] += int((g & ~first & ~end).sum())
            br["start_inside"] += int((g & hit & inside).sum())
            br["root"] += int((g & hit & ~inside).sum())
            br["disc_clamped"] += int((g & hit & ~inside & clamped).sum())
            br["disc_positive"] += int((g & hit & ~inside & ~clamped).sum())
        # the last instant: s = 0, m = |d_{K-1}|^2
        k = K - 1
        m = dx[:, :, k] * dx[:, :, k] + dy[:, :, k] * dy[:, :, k]
        upd = m < M
        M, ks, ss = np.where(upd, m, M), np.where(upd, k, ks), np.where(upd, 0.0, ss)
        hit = (m < R2) & ~(tc < INF)
        tc = np.where(hit, instant(t0, k, dt) + F64(0.0) * dt, tc)
        last_only = hit
        br["last_term_only"] = int((partner & last_only).sum())
        gap = np.sqrt(M) - R
        tstar = (t0 + ks.astype(F64) * dt) + ss * dt
    return dict(M=M, kstar=ks, sstar=ss, tstar=tstar, gap=gap, tc=tc, bad_a=bad_a, bad_b=bad_b, partner=partner, R=R, R2=R2,
                branches=br, self_mode=self_mode, dx=dx, dy=dy)


def reduce_rows(gap, tstar, tc, partner, bad):
    """summary [rows, 7]: the lexicographic minima on (gap, j) and (tc, j) over the partners of each row, and the count."""
    rows, cols = gap.shape
    out = np.zeros((rows, NUM_SLOTS))
    for i in range(rows):
        if bad[i]:
            out[i, :SLOT_STATUS] = np.nan
            out[i, SLOT_STATUS] = STATUS_BAD_TRACK
            continue
        g, j, t, first, jc, n = INF, -1, np.nan, INF, -1, 0
        for q in range(cols):
            if not partner[i, q]:
                continue
            if gap[i, q] < g:
                g, j, t = gap[i, q], q, tstar[i, q]
            if tc[i, q] < first:
                first, jc = tc[i, q], q
            n += int(tc[i, q] < INF)
        out[i] = [g, j, t, first, jc, n, STATUS_NO_PARTNER if j < 0 else 0]
    return out


def conflicts(tracks_a, tracks_b=None, *, dt, t0=0.0, radius_a=None, radius_b=None, margin=0.0):
    """-> dict(summary [Ba, 7], summary_b [Bb, 7] or None, pair_gap, pair_first [Ba, Bb], pairs = the dict of `pairs`)."""
    p = pairs(tracks_a, tracks_b, dt=dt, t0=t0, radius_a=radius_a, radius_b=radius_b, margin=margin)
    summary = reduce_rows(p["gap"], p["tstar"], p["tc"], p["partner"], p["bad_a"])
    summary_b = None if p["self_mode"] else reduce_rows(p["gap"].T, p["tstar"].T, p["tc"].T, p["partner"].T, p["bad_b"])
    good = ~p["bad_a"][:, None] & ~p["bad_b"][None, :]
    diag = ~p["partner"] & good                          # self mode: the diagonal of good tracks
    pair_gap = np.where(good, np.where(diag, INF, p["gap"]), np.nan)
    pair_first = np.where(good, np.where(diag, INF, p["tc"]), np.nan)
    return dict(summary=summary, summary_b=summary_b, pair_gap=pair_gap, pair_first=pair_first, pairs=p)
