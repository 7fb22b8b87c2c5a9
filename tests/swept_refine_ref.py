"""numpy restatement of nfopp_swept_refine (include/nfopp_hip.h) in float64 over tests/swept_ref.py and
tests/clearance_ref.py: the box certificate on dyadic pieces of a segment, the rectangle checker's label at their midpoints,
the pre-order walk with its depth and evaluation limits, and the path reduction nfopp_path_refined_labels.  The sub-poses are
formed from the fp32 inputs and rounded to fp32 as the kernel rounds them; everything decided on them is float64, and every
comparison that float64 and fp32 may settle differently marks its segment `ambiguous`.  Every segment of a call walks in
lockstep, one evaluation (a piece test or a midpoint test) per round, so a call costs rounds, not segments, of numpy calls.
Checked by hand-computed cases in tests/test_swept_refine_cpu.py; the GPU tests compare the device with it."""
import numpy as np

import clearance_ref as cr
import swept_ref as sr

F32 = np.float32
FREE, HIT, UNDECIDED = 0, 1, 2
PI_F, TWO_PI_F, INV_TWO_PI_F = F32(3.14159274101257324), F32(6.28318548202514648), F32(0.159154943)
CHUNK = 256            # segments per numpy call: [CHUNK, n_points] float64 temporaries


def wrap_f32(a):
    """wrap_angle of csrc/common.h operation by operation in fp32 (the fma's exact product and sum through float64)."""
    x = (np.asarray(a, F32) + PI_F).astype(F32)
    k = np.floor((x * INV_TWO_PI_F).astype(F32))
    r = (x.astype(np.float64) - k.astype(np.float64) * float(TWO_PI_F)).astype(F32)
    r = np.where(r < 0, (r + TWO_PI_F).astype(F32), r)
    r = np.where(r >= TWO_PI_F, (r - TWO_PI_F).astype(F32), r)
    return (r - PI_F).astype(F32)


def successor(d, i):
    """The stackless pre-order step after node (d, i) is finished: while i is odd, up; then the right sibling.
    Arrays in, (d, i, done) out; done where the walk is over (back at the root)."""
    d, i = np.array(d, np.int64), np.array(i, np.int64)
    while True:
        odd = (i & 1) == 1
        if not odd.any():
            break
        i[odd] >>= 1
        d[odd] -= 1
    done = d == 0
    i[~done] += 1
    return d, i, done


def sub_poses(a, b, i, d):
    """fp32 poses [n, 3] at the parameters i * 2^-d: a and b as they are at 0 and 1 (b with its raw heading), else one fma per
    component along ex, ey (fp32 differences) and dth = wrap_angle(theta_b - theta_a) (fp32)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    i, d = np.asarray(i, np.int64), np.asarray(d, np.int64)
    s = i.astype(np.float64) / (2.0 ** d)
    e = (b[:, :2] - a[:, :2]).astype(F32)
    dth = wrap_f32((b[:, 2] - a[:, 2]).astype(F32))
    step = np.concatenate([e, dth[:, None]], 1).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        out = (s[:, None] * step + a.astype(np.float64)).astype(F32)
    out = np.where((i == 0)[:, None], a, out)
    return np.where((i == 2 ** d)[:, None], b, out).astype(F32)


def hits(poses, points, box):
    """(hit [n] bool, close [n] bool): an obstacle point strictly inside the box at the pose; close where that rests on a
    point within 16 * 2^-24 (|dx| + |dy|) of a box edge and no other point is clearly inside."""
    pts = np.asarray(points, F32).reshape(-1, 2)
    n = len(poses)
    if len(pts) == 0:
        return np.zeros(n, bool), np.zeros(n, bool)
    dx, dy = cr.offsets(poses, pts)
    th = np.asarray(poses, F32).astype(np.float64)[:, 2]
    c, s = np.cos(th)[:, None], np.sin(th)[:, None]
    rx, ry = c * dx + s * dy, c * dy - s * dx
    bx = np.asarray(box, F32).astype(np.float64)
    tol = 16 * 2.0 ** -24 * (np.abs(dx) + np.abs(dy))
    inside = (rx > bx[0]) & (rx < bx[1]) & (ry > bx[2]) & (ry < bx[3])
    near_x = np.minimum(np.abs(rx - bx[0]), np.abs(rx - bx[1])) <= tol
    near_y = np.minimum(np.abs(ry - bx[2]), np.abs(ry - bx[3])) <= tol
    around = (rx > bx[0] - tol) & (rx < bx[1] + tol) & (ry > bx[2] - tol) & (ry < bx[3] + tol)
    near = (near_x | near_y) & around
    clear = (inside & ~near).any(1)
    return inside.any(1), near.any(1) & ~clear


def cert(p, q, points, box, slack):
    """(certified [n] bool, close [n] bool) for the pieces (p, q): swept_ref.box_values > slack; close where the value is
    within 2 slack of slack or the domain rule's delta within 2 slack of 4 reach."""
    v, _ = sr.box_values(p, q, points, box)
    reach = sr.box_reach(box)
    close = np.abs(v - slack) <= 2 * slack
    if len(np.asarray(points).reshape(-1, 2)):
        close |= np.abs(sr.delta(p, q, reach) - 4 * reach) <= 2 * slack
    return v > slack, close


def _chunked(fn, n, *arrays):
    outs = [fn(*(x[k:k + CHUNK] for x in arrays)) for k in range(0, n, CHUNK)]
    return tuple(np.concatenate([o[j] for o in outs]) for j in range(2))


def refine(a, b, points, box, max_depth=8, node_budget=1024):
    """(status uint8, s fp32, depth uint8, ambiguous bool), each [n]: refine(a, b; max_depth, node_budget) of
    include/nfopp_hip.h for every segment."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    n = len(a)
    slack = sr.box_reach(box) * 2.0 ** -16
    status = np.full(n, UNDECIDED, np.uint8)
    s_out = np.full(n, -1.0, F32)
    depth = np.zeros(n, np.int64)
    amb = np.zeros(n, bool)
    ok = sr.finite_segments(a, b, box)                 # 1: a non-finite pose: UNDECIDED, -1, 0
    a0, b0 = np.where(ok[:, None], a, 0).astype(F32), np.where(ok[:, None], b, 0).astype(F32)
    hit_a, close_a = _chunked(lambda x: hits(x, points, box), n, a0) if n else (np.zeros(0, bool),) * 2
    hit_b, close_b = _chunked(lambda x: hits(x, points, box), n, b0) if n else (np.zeros(0, bool),) * 2
    amb |= ok & (close_a | (~hit_a & close_b))
    status[ok & hit_a], s_out[ok & hit_a] = HIT, 0.0   # 2: the end poses
    only_b = ok & ~hit_a & hit_b
    status[only_b], s_out[only_b] = HIT, 1.0
    act = np.flatnonzero(ok & ~hit_a & ~hit_b)          # 3: the walk, all of them one evaluation per round
    d, i = np.zeros(len(act), np.int64), np.zeros(len(act), np.int64)
    evals = np.zeros(len(act), np.int64)
    mid = np.zeros(len(act), bool)                     # the next evaluation is the node's midpoint, not its piece
    und = np.zeros(len(act), bool)
    while len(act):
        spent = evals == node_budget                   # 5: stops UNDECIDED (status holds that already)
        keep = ~spent
        act, d, i, evals, mid, und = act[keep], d[keep], i[keep], evals[keep], mid[keep], und[keep]
        if not len(act):
            break
        evals += 1
        finished = np.zeros(len(act), bool)
        gone = np.zeros(len(act), bool)
        pc = np.flatnonzero(~mid)
        if len(pc):
            seg = act[pc]
            depth[seg] = np.maximum(depth[seg], d[pc])
            p, q = sub_poses(a[seg], b[seg], i[pc], d[pc]), sub_poses(a[seg], b[seg], i[pc] + 1, d[pc])
            good, close = _chunked(lambda x, y: cert(x, y, points, box, slack), len(pc), p, q)
            amb[seg] |= close
            at_limit = ~good & (d[pc] == max_depth)
            und[pc[at_limit]] = True
            finished[pc[good | at_limit]] = True
            mid[pc[~good & ~at_limit]] = True
        pm = np.flatnonzero(mid & ~finished)
        pm = np.setdiff1d(pm, pc)                      # a node whose piece failed this round: its midpoint is the next one's
        if len(pm):
            seg = act[pm]
            m = sub_poses(a[seg], b[seg], 2 * i[pm] + 1, d[pm] + 1)
            h, close = _chunked(lambda x: hits(x, points, box), len(pm), m)
            amb[seg] |= close
            status[seg[h]] = HIT
            s_out[seg[h]] = ((2 * i[pm][h] + 1) / 2.0 ** (d[pm][h] + 1)).astype(F32)
            gone[pm[h]] = True
            down = pm[~h]
            d[down] += 1
            i[down] *= 2
            mid[down] = False
        fin = np.flatnonzero(finished)
        if len(fin):
            nd, ni, done = successor(d[fin], i[fin])
            d[fin], i[fin] = nd, ni
            over = fin[done]
            status[act[over]] = np.where(und[over], UNDECIDED, FREE)   # 4
            gone[over] = True
        keep = ~gone
        act, d, i, evals, mid, und = act[keep], d[keep], i[keep], evals[keep], mid[keep], und[keep]
    return status, s_out, depth.astype(np.uint8), amb


def path_reduction(seg_status, seg_s, labels):
    """nfopp_path_refined_labels for one path: seg_status, seg_s [m - 1], labels [m] -> (labels [m], status, first [2])."""
    seg_status, labels = np.asarray(seg_status), np.array(labels, F32)
    pose_hit = bool((labels != 0).any())
    labels[:-1][seg_status != FREE] = 1.0
    if pose_hit or (seg_status == HIT).any():
        status = 1
    else:
        status = 2 if (seg_status == UNDECIDED).any() else 0
    bad = np.flatnonzero(seg_status != FREE)
    first = (F32(bad[0]), F32(np.asarray(seg_s, F32)[bad[0]])) if len(bad) else (F32(-1), F32(-1))
    return labels, status, first
