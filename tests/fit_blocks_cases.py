"""The cases of the block-by-block gate of the fit gradient (tests/fit_blocks_gate.py): sample counts at every edge of the
chunk count of pass 2 (csrc/onf_wgrad.hip) and of the per-sample path's reduction (csrc/onf_train.hip), and per case the
poses and labels, deterministic from (F, P).  Needs no GPU: tests/test_fit_blocks_cpu.py checks the conditions below on the
CPU, tests/test_gpu_fit_blocks.py launches the same cases.

Pass 2 is a persistent launch of min(C, ceil(P / K)) workgroups on a device of C compute units; workgroup w takes the chunks
w, w + grid, ... of K samples (K = 32 behind the split passes, matrix paths 1 and 2; K = 16 behind the fp32 pass, path 0), two
chunks ahead prefetched.  Counts, for both K:
  small        1, 15, 16, 17, 31, 32, 33 (a ragged chunk, a full one, a chunk and a sample), 63, 64, 65, 129 (the chunk edges
               of the per-sample path's ceil(P / 64) reduction)
  C K          every workgroup one full chunk            C K + 1        one workgroup a second chunk of ONE sample
  2 C K - 1    every workgroup two, the last short by 1  2 C K + K + 5  two workgroups three chunks, the others two
  3 C K + 1    one workgroup four, the others three
  4096, 4097   the per-sample path's cap of 64 reduction chunks
F = 220 and 100 take every count, F = 200 and 120 the three of REDUCED.

Poses are k1_bits_cases.points over-drawn; the first P rows whose float64 distance to a ReLU kink is at least 10 x
float64_ref.KINK are kept, so NO row is left out of any comparison and an fp32 evaluation has the float64 masks.  Labels are
uniform < 0.35 but for two sentinels -- the last sample and the first sample of the last 32-chunk -- which take the label the
float64 logit contradicts: |rho| >= 0.5 / P there, so the tail of every case carries weight."""
import numpy as np

import float64_ref as f64
import k1_bits_cases as kc

F32 = np.float32
KS = (16, 32)
SMALL = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)
PER_SAMPLE_CAP = (4096, 4097)
FULL_DIMS, REDUCED_DIMS = (220, 100), (200, 120)
KINK_MARGIN = 10 * f64.KINK


def grid_edges(C, K):
    return (C * K, C * K + 1, 2 * C * K - 1, 2 * C * K + K + 5, 3 * C * K + 1)


def counts(C):
    """every sample count of a device of C compute units, ascending, each once"""
    return sorted(set(SMALL) | set(PER_SAMPLE_CAP) | {P for K in KS for P in grid_edges(C, K)})


def reduced_counts(C):
    return (33, C * 32 + 1, 2 * C * 32 + 37)


def cases(C):
    """[(F, P)] of a device of C compute units"""
    return [(fin, P) for fin in FULL_DIMS for P in counts(C)] + [(fin, P) for fin in REDUCED_DIMS for P in reduced_counts(C)]


def trip_counts(P, K, C):
    """chunks per workgroup of pass 2, and the samples of the last chunk"""
    n_chunks = -(-P // K)
    grid = min(C, n_chunks)
    trips = np.array([len(range(w, n_chunks, grid)) for w in range(grid)])
    return trips, P - (n_chunks - 1) * K


def sentinels(P):
    """the last sample and the first sample of the last 32-chunk (one row where P = 1 mod 32)"""
    return sorted({P - 1, 32 * ((P - 1) // 32)})


def inputs(fin, P, flat, cfg):
    """-> (poses [P, 2 | 3] fp32, labels [P] fp32) of the case on the network (flat, cfg) = bits_float64_gate.cpu_network(fin)"""
    drawn = kc.points(fin, P + P // 4 + 64, [fin, P])
    c = f64.onf_eval64(flat, cfg, drawn)
    keep = np.flatnonzero(c["kink"] >= KINK_MARGIN)[:P]
    assert len(keep) == P, "too few kink-free rows drawn for F = %d, P = %d" % (fin, P)
    x = np.ascontiguousarray(drawn[keep])
    y = (np.random.default_rng([fin, P, 1]).uniform(size=P) < 0.35).astype(F32)
    s = sentinels(P)
    y[s] = (c["logit"][keep][s] < 0).astype(F32)
    return x, y
