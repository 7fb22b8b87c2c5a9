"""GPU dev tool: record the 32x32 ONF kernel's output bits at small shapes (tests/k1_bits_cases.py) with the CURRENT build
into tests/golden/k1_bits.npz -- run on the build whose results are to be kept, before the kernel is changed.
Usage: python tools/x32/record_k1_bits.py [out.npz]        (--check out.npz: compare instead of writing)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "pytorch-motion-planner_amd"), ROOT):
    sys.path.insert(0, p)
import k1_bits_cases as kc  # noqa: E402

args = [a for a in sys.argv[1:] if a != "--check"]
path = args[0] if args else os.path.join(ROOT, "tests", "golden", "k1_bits.npz")
res = kc.run_cases()
again = kc.run_cases()     # the kernel is deterministic: a second run must give the same words
for k in res:
    assert np.array_equal(np.ascontiguousarray(res[k]).view(np.uint8), np.ascontiguousarray(again[k]).view(np.uint8)), k
if "--check" in sys.argv[1:]:
    z = np.load(path)
    assert sorted(z.files) == sorted(res), "case lists differ"
    bad = [k for k in res if not np.array_equal(np.ascontiguousarray(np.asarray(res[k])).view(np.uint8),
                                                np.ascontiguousarray(z[k]).view(np.uint8))]
    print("%d arrays, %d differ %s" % (len(res), len(bad), bad[:8]))
    sys.exit(1 if bad else 0)
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
np.savez_compressed(path, **res)
print("%s: %d arrays, %d bytes" % (path, len(res), os.path.getsize(path)))
