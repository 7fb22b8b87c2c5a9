"""The rule of nfopp_box_track_conflicts (csrc/box_conflict.hip, stated in include/nfopp_hip.h) restated in numpy: every
operation is a separate float64 numpy operation in the header's order.  The intervals are a loop, the pairs are vectorised,
and the dyadic tree of an interval is evaluated level by level: a node's class is a function of the node alone, so the
depth-first walk of the rule (left half, then right half, stop at the first CONFLICT, remember the first UNDECIDED before
it) is the minimum of the CONFLICT times and the minimum of the UNDECIDED times below it.  The device is compared with this
bit for bit on the device's own unit vectors (tests/test_gpu_box_conflict.py).

`pair_radius` and the summaries' conventions are those of tests/track_conflict_ref.py (imported).  That file states the
closest approach only inside its loop over fp32 instants, and a sub-interval's end points are float64, so the five lines are
written out here as `closest_approach`; tests/test_box_conflict_cpu.py holds them to `track_conflict_ref.pairs` bit for bit."""
import numpy as np

import track_conflict_ref as tr

F32, F64 = np.float32, np.float64
INF = np.inf
FREE, CONFLICT, UNDECIDED, BAD_PAIR = 0, 1, 2, -1
NUM_SLOTS = 7
(SLOT_FIRST_TIME, SLOT_FIRST_PARTNER, SLOT_CONFLICTS, SLOT_UNDECIDED_TIME, SLOT_UNDECIDED_PARTNER, SLOT_UNDECIDED,
 SLOT_STATUS) = range(NUM_SLOTS)
STATUS_BAD_TRACK, STATUS_NO_PARTNER = tr.STATUS_BAD_TRACK, tr.STATUS_NO_PARTNER
MAX_REFINE = 8
HALF_PI_UP = float.fromhex("0x1.921fb54442d19p+0")   # the float64 next above pi / 2


def unit_vectors(tracks):
    """[B, K, >= 3] fp32 -> [B, K, 2] float64 (cos, sin) of the widened heading; NaN where it is not finite."""
    th = np.asarray(tracks, F32)[:, :, 2].astype(F64)
    with np.errstate(all="ignore"):
        u = np.stack([np.cos(th), np.sin(th)], -1)
    u[~np.isfinite(th)] = np.nan
    return u


def box_reach(box):
    """[..., 4] fp32 -> fp32: box_reach of csrc/point_cloud.h with hypotf written as the rounded float64 square root."""
    b = np.abs(np.asarray(box, F32))
    mx, my = np.maximum(b[..., 0], b[..., 1]).astype(F64), np.maximum(b[..., 2], b[..., 3]).astype(F64)
    with np.errstate(all="ignore"):
        corner = np.sqrt(mx * mx + my * my).astype(F32)
        return corner * F32(1.000001)


def pair_radius_matrix(radius_a, radius_b, ba, bb, margin):
    """R_ij = (ra_i + rb_j) + margin [Ba, Bb]: track_conflict_ref's own lines, through its `pairs` on tracks of one instant
    (bb None: self mode)."""
    za = np.zeros((ba, 1, 2), F32)
    zb = None if bb is None else np.zeros((bb, 1, 2), F32)
    return tr.pairs(za, zb, dt=1.0, radius_a=radius_a, radius_b=radius_b, margin=margin)["R"]


def closest_approach(x0, y0, cc, d1x, d1y, e):
    """track_pairs.h's closest_approach on arrays -> (a, m)."""
    wx, wy = d1x - x0, d1y - y0
    a = wx * wx + wy * wy
    b = x0 * wx + y0 * wy
    first = (a == 0.0) | (b >= 0.0)
    end = ~first & (-b >= a)
    s = (-b) / a
    px, py = x0 + s * wx, y0 + s * wy
    return a, np.where(first, cc, np.where(end, e, px * px + py * py))


def _max(a, b):
    return np.where(a > b, a, b)


def _min(a, b):
    return np.where(a < b, a, b)


def _axis_gap(t, bx, cx, cy, s0, s1):
    """The gap along one face axis: the other box `bx` [..., 4], seen from the axis' owner, spans t + x * cx + y * cy; the
    owner spans [s0, s1]."""
    a0, a1, b0, b1 = bx[..., 0] * cx, bx[..., 1] * cx, bx[..., 2] * cy, bx[..., 3] * cy
    lo = (t + _min(a0, a1)) + _min(b0, b1)
    hi = (t + _max(a0, a1)) + _max(b0, b1)
    return _max(lo - s1, s0 - hi)


def separation(pi, ui, pj, uj, bi, bj):
    """sep of two boxes at an instant: the largest gap over the four face axes.  p, u [..., 2], b [..., 4], float64."""
    dx, dy = pj[..., 0] - pi[..., 0], pj[..., 1] - pi[..., 1]
    ci, si, cj, sj = ui[..., 0], ui[..., 1], uj[..., 0], uj[..., 1]
    cr = ci * cj + si * sj
    sr = ci * sj - si * cj
    xi = dx * ci + dy * si            # box j's origin in box i's frame
    yi = dy * ci - dx * si
    xj = -(dx * cj + dy * sj)         # box i's origin in box j's frame
    yj = -(dy * cj - dx * sj)
    g1 = _axis_gap(xi, bj, cr, -sr, bi[..., 0], bi[..., 1])
    g2 = _axis_gap(yi, bj, sr, cr, bi[..., 2], bi[..., 3])
    g3 = _axis_gap(xj, bi, cr, sr, bj[..., 0], bj[..., 1])
    g4 = _axis_gap(yj, bi, -sr, cr, bj[..., 2], bj[..., 3])
    return _max(_max(g1, g2), _max(g3, g4))


def classify(n, R, D2, refine_left):
    """Steps 1 .. 5 on the nodes `n` (a dict of arrays: pia, uia, pja, uja, pib, uib, pjb, ujb [N, 2], bi, bj [N, 4], ri, rj
    [N]) -> (code [N]: 0 FREE by the discs, 1 CONFLICT at a, 2 FREE by the certificate, 3 split, 4 UNDECIDED at a; mid: the
    dict of the mid poses)."""
    d0x, d0y = n["pia"][:, 0] - n["pja"][:, 0], n["pia"][:, 1] - n["pja"][:, 1]
    d1x, d1y = n["pib"][:, 0] - n["pjb"][:, 0], n["pib"][:, 1] - n["pjb"][:, 1]
    cc, e = d0x * d0x + d0y * d0y, d1x * d1x + d1y * d1y
    a, m = closest_approach(d0x, d0y, cc, d1x, d1y, e)
    disc_free = m >= D2
    sa = separation(n["pia"], n["uia"], n["pja"], n["uja"], n["bi"], n["bj"])
    hit = (sa - R) < 0.0
    sb = separation(n["pib"], n["uib"], n["pjb"], n["ujb"], n["bi"], n["bj"])
    wn = np.sqrt(a)
    dui, duj = n["uib"] - n["uia"], n["ujb"] - n["uja"]
    ni = np.sqrt(dui[:, 0] * dui[:, 0] + dui[:, 1] * dui[:, 1])
    nj = np.sqrt(duj[:, 0] * duj[:, 0] + duj[:, 1] * duj[:, 1])
    rot = n["ri"] * ni + n["rj"] * nj
    mot = wn + HALF_PI_UP * rot
    cert_free = (((sa + sb) - mot) * 0.5 - R) >= 0.0
    smi, smj = n["uia"] + n["uib"], n["uja"] + n["ujb"]
    li = np.sqrt(smi[:, 0] * smi[:, 0] + smi[:, 1] * smi[:, 1])
    lj = np.sqrt(smj[:, 0] * smj[:, 0] + smj[:, 1] * smj[:, 1])
    can_split = refine_left & (li != 0.0) & (lj != 0.0)
    code = np.where(disc_free, 0, np.where(hit, 1, np.where(cert_free, 2, np.where(can_split, 3, 4))))
    mid = dict(pi=(n["pia"] + n["pib"]) * 0.5, pj=(n["pja"] + n["pjb"]) * 0.5, ui=smi / li[:, None], uj=smj / lj[:, None])
    return code, mid


def _boxes(box, n):
    return np.broadcast_to(np.asarray(box, F32).reshape(-1, 4), (n, 4)).astype(F64)


def bad_shape(box32, r32):
    """[n] bool: a box entry or the radius not finite, x0 >= x1, y0 >= y1, or a negative radius."""
    b, r = np.asarray(box32, F64), np.asarray(r32, F64)
    with np.errstate(all="ignore"):
        return ~(np.isfinite(b).all(axis=-1) & np.isfinite(r) & (b[..., 0] < b[..., 1]) & (b[..., 2] < b[..., 3]) & (r >= 0.0))


def pairs(tracks_a, units_a, tracks_b=None, units_b=None, *, dt, t0=0.0, box_a, box_b=None, radius_a=None, radius_b=None,
          margin=0.0, refine=0):
    """All pairs.  tracks [B, K, >= 3] fp32 (only x, y are read), units [B, K, 2] float64; tracks_b None = self mode.
    -> dict: status [Ba, Bb] int32 (BAD_PAIR for a pair with a bad track), tc, tu [Ba, Bb], bad_a, bad_b, partner, R,
    `decided`: how many visited top-level intervals of good pairs the discs, the certificate at depth 0 and refinement
    decided, and how many stayed undecided."""
    assert 0 <= refine <= MAX_REFINE
    self_mode = tracks_b is None
    a32 = np.asarray(tracks_a, F32)
    ua = np.asarray(units_a, F64)
    b32, ub = (a32, ua) if self_mode else (np.asarray(tracks_b, F32), np.asarray(units_b, F64))
    ba, K = a32.shape[:2]
    bb = len(b32)
    bxa = _boxes(box_a, ba)
    bxb = bxa if self_mode else _boxes(box_b, bb)
    ra = tr._radii(radius_a, ba)
    rb = ra if self_mode else tr._radii(radius_b, bb)
    pa, pb = a32[:, :, :2].astype(F64), b32[:, :, :2].astype(F64)
    bad_a = ~(np.isfinite(pa).all(axis=(1, 2)) & np.isfinite(ua).all(axis=(1, 2))) | bad_shape(bxa, ra)
    bad_b = ~(np.isfinite(pb).all(axis=(1, 2)) & np.isfinite(ub).all(axis=(1, 2))) | bad_shape(bxb, rb)
    good = ~bad_a[:, None] & ~bad_b[None, :]
    if self_mode:   # i < j is evaluated with i as the first box, and mirrored
        todo = good & np.triu(np.ones((ba, ba), bool), 1)
        partner = good & ~np.eye(ba, dtype=bool)
    else:
        todo = partner = good
    dt, t0, margin = F64(dt), F64(t0), F64(margin)
    reach_a, reach_b = box_reach(bxa.astype(F32)).astype(F64), box_reach(bxb.astype(F32)).astype(F64)
    with np.errstate(all="ignore"):
        R = pair_radius_matrix(radius_a, None if self_mode else radius_b, ba, None if self_mode else bb, margin)
        Dr = (reach_a[:, None] + reach_b[None, :]) + R
        D2 = Dr * Dr
    tc, tu = np.full((ba, bb), INF), np.full((ba, bb), INF)
    decided = dict(discs=0, certificate=0, refinement=0, undecided=0, conflict=0)
    ii, jj = np.nonzero(todo)
    with np.errstate(all="ignore"):
        for k in range(K - 1):
            live = ~(tc[ii, jj] < INF)
            i, j = ii[live], jj[live]
            if len(i) == 0:
                break
            tk = tr.instant(t0, k, dt)
            n = dict(pia=pa[i, k], uia=ua[i, k], pja=pb[j, k], uja=ub[j, k], pib=pa[i, k + 1], uib=ua[i, k + 1],
                     pjb=pb[j, k + 1], ujb=ub[j, k + 1], bi=bxa[i], bj=bxb[j], ri=reach_a[i], rj=reach_b[j])
            pos = np.zeros(len(i), np.int64)
            ktc, ktu = np.full(len(i), INF), np.full(len(i), INF)
            root = np.arange(len(i))                       # which top-level interval a node belongs to
            outcome = np.zeros(len(i), np.int64)           # 0 discs, 2 certificate at depth 0, else by refinement
            for depth in range(refine + 1):
                code, mid = classify(n, R[i, j], D2[i, j], np.full(len(i), depth < refine))
                t = tk + (pos.astype(F64) / F64(1 << depth)) * dt
                if depth == 0:
                    outcome = code.copy()
                np.minimum.at(ktc, root[code == 1], t[code == 1])
                np.minimum.at(ktu, root[code == 4], t[code == 4])
                s = code == 3
                if not s.any():
                    break
                left = dict(pia=n["pia"][s], uia=n["uia"][s], pja=n["pja"][s], uja=n["uja"][s], pib=mid["pi"][s], uib=mid["ui"][s],
                            pjb=mid["pj"][s], ujb=mid["uj"][s])
                right = dict(pia=mid["pi"][s], uia=mid["ui"][s], pja=mid["pj"][s], uja=mid["uj"][s], pib=n["pib"][s],
                             uib=n["uib"][s], pjb=n["pjb"][s], ujb=n["ujb"][s])
                nxt = {key: np.concatenate([left[key], right[key]]) for key in left}
                for key in ("bi", "bj", "ri", "rj"):
                    nxt[key] = np.concatenate([n[key][s], n[key][s]])
                n = nxt
                pos = np.concatenate([2 * pos[s], 2 * pos[s] + 1])
                root = np.concatenate([root[s], root[s]])
                i, j = np.concatenate([i[s], i[s]]), np.concatenate([j[s], j[s]])
            i, j = ii[live], jj[live]
            ktu = np.where(ktu < ktc, ktu, INF)            # the first UNDECIDED before the CONFLICT
            first_u = ~(tu[i, j] < INF)
            tu[i, j] = np.where(first_u, ktu, tu[i, j])
            tc[i, j] = ktc
            decided["discs"] += int((outcome == 0).sum())
            decided["certificate"] += int((outcome == 2).sum())
            decided["conflict"] += int((ktc < INF).sum())
            decided["undecided"] += int(((ktu < INF) & ~(ktc < INF)).sum())
            decided["refinement"] += int(((outcome == 3) & ~(ktc < INF) & ~(ktu < INF)).sum())
        # the last instant
        live = ~(tc[ii, jj] < INF)
        i, j = ii[live], jj[live]
        k = K - 1
        lx, ly = pa[i, k, 0] - pb[j, k, 0], pa[i, k, 1] - pb[j, k, 1]
        cl = lx * lx + ly * ly
        sep = separation(pa[i, k], ua[i, k], pb[j, k], ub[j, k], bxa[i], bxb[j])
        hit = ~(cl >= D2[i, j]) & ((sep - R[i, j]) < 0.0)
        t = tr.instant(t0, k, dt) + (F64(0.0) / F64(1.0)) * dt
        tc[i, j] = np.where(hit, t, INF)
    if self_mode:
        tc, tu = np.where(todo.T, tc.T, tc), np.where(todo.T, tu.T, tu)
    status = np.where(tc < INF, CONFLICT, np.where(tu < INF, UNDECIDED, FREE)).astype(np.int32)
    status = np.where(good, status, BAD_PAIR).astype(np.int32)
    return dict(status=status, tc=tc, tu=tu, bad_a=bad_a, bad_b=bad_b, partner=partner, good=good, R=R, decided=decided,
                self_mode=self_mode, reach_a=reach_a, reach_b=reach_b)


def reduce_rows(status, tc, tu, partner, bad):
    """summary [rows, 7]: the lexicographic minima on (tc, j) and (tu, j) over the partners of each row and the two counts."""
    rows, cols = tc.shape
    out = np.zeros((rows, NUM_SLOTS))
    for i in range(rows):
        if bad[i]:
            out[i, :SLOT_STATUS] = np.nan
            out[i, SLOT_STATUS] = STATUS_BAD_TRACK
            continue
        first, jc, nc, und, ju, nu, any_partner = INF, -1, 0, INF, -1, 0, False
        for q in range(cols):
            if not partner[i, q]:
                continue
            any_partner = True
            if tc[i, q] < first:
                first, jc = tc[i, q], q
            if tu[i, q] < und:
                und, ju = tu[i, q], q
            nc += int(status[i, q] == CONFLICT)
            nu += int(status[i, q] == UNDECIDED)
        out[i] = [first, jc, nc, und, ju, nu, 0 if any_partner else STATUS_NO_PARTNER]
    return out


def conflicts(tracks_a, units_a, tracks_b=None, units_b=None, **kw):
    """-> dict(summary [Ba, 7], summary_b [Bb, 7] or None, pair_status int32, pair_first, pair_undecided [Ba, Bb], pairs)."""
    p = pairs(tracks_a, units_a, tracks_b, units_b, **kw)
    summary = reduce_rows(p["status"], p["tc"], p["tu"], p["partner"], p["bad_a"])
    summary_b = None if p["self_mode"] else reduce_rows(p["status"].T, p["tc"].T, p["tu"].T, p["partner"].T, p["bad_b"])
    return dict(summary=summary, summary_b=summary_b, pair_status=p["status"], pair_first=np.where(p["good"], p["tc"], np.nan),
                pair_undecided=np.where(p["good"], p["tu"], np.nan), pairs=p)


# ---- the brute-force side of the soundness test: nothing below is part of the rule -------------------------------------------
def box_corners(p, u, box):
    """World corners [..., 4, 2] of the box at position p [..., 2] with heading unit vector u [..., 2], in ring order."""
    x0, x1, y0, y1 = (box[..., q] for q in range(4))
    bx = np.stack([x0, x1, x1, x0], -1)
    by = np.stack([y0, y0, y1, y1], -1)
    c, s = u[..., 0:1], u[..., 1:2]
    return np.stack([p[..., 0:1] + bx * c - by * s, p[..., 1:2] + bx * s + by * c], -1)


def _point_segment(p, a, b):
    ab, ap = b - a, p - a
    t = np.clip((ap * ab).sum(-1) / (ab * ab).sum(-1), 0.0, 1.0)
    d = ap - t[..., None] * ab
    return np.sqrt((d * d).sum(-1))


def box_distance(ca, cb):
    """Exact distance between two convex quadrilaterals given by their corners [..., 4, 2] (0 when they overlap)."""
    def inside(p, c):      # p [..., 2] in the ring c [..., 4, 2]
        e = np.roll(c, -1, axis=-2) - c
        r = p[..., None, :] - c
        cross = e[..., 0] * r[..., 1] - e[..., 1] * r[..., 0]
        return (cross >= 0).all(-1) | (cross <= 0).all(-1)
    best = np.full(ca.shape[:-2], INF)
    for x, y in ((ca, cb), (cb, ca)):
        for q in range(4):
            for e in range(4):
                best = np.minimum(best, _point_segment(x[..., q, :], y[..., e, :], y[..., (e + 1) % 4, :]))
    over = np.zeros(best.shape, bool)
    for q in range(4):
        over |= inside(ca[..., q, :], cb) | inside(cb[..., q, :], ca)

    def side(a, b, p):
        return (b[..., 0] - a[..., 0]) * (p[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (p[..., 0] - a[..., 0])
    for q in range(4):     # two rectangles can cross without a corner of one inside the other: then two edges cross
        a0, a1 = ca[..., q, :], ca[..., (q + 1) % 4, :]
        for e in range(4):
            b0, b1 = cb[..., e, :], cb[..., (e + 1) % 4, :]
            over |= (side(a0, a1, b0) * side(a0, a1, b1) < 0) & (side(b0, b1, a0) * side(b0, b1, a1) < 0)
    return np.where(over, 0.0, best)
