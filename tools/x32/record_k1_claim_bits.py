"""GPU dev tool: record the 32x32 ONF kernel's output bits at the shapes of tests/k1_claim_cases.py (pool edges of both
workgroup shapes, a trajectory launch with retired trajectories) with the CURRENT build into tests/golden/k1_claim_bits.npz:
per case the sha256 of the output bytes and the first and last 64 rows.  Run on the build whose results are to be kept --
the one in front of the change to tiles by claim.
Usage: python tools/x32/record_k1_claim_bits.py [out.npz]        (--check out.npz: compare instead of writing)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "pytorch-motion-planner_amd"), ROOT):
    sys.path.insert(0, p)
import k1_claim_cases as cc  # noqa: E402

args = [a for a in sys.argv[1:] if a != "--check"]
path = args[0] if args else os.path.join(ROOT, "tests", "golden", "k1_claim_bits.npz")
res = cc.record()
again = cc.record()     # the kernel is deterministic: a second run must give the same words
for k in res:
    assert np.array_equal(res[k], again[k]), k
if "--check" in sys.argv[1:]:
    z = np.load(path)
    assert sorted(z.files) == sorted(res), "case lists differ"
    bad = [k for k in res if not np.array_equal(np.asarray(res[k]), z[k])]
    print("%d arrays, %d differ %s" % (len(res), len(bad), bad[:8]))
    sys.exit(1 if bad else 0)
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
np.savez_compressed(path, **res)
print("%s: %d arrays, %d bytes" % (path, len(res), os.path.getsize(path)))
