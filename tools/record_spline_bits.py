"""GPU dev tool: record the output bits of the path post-processor and of the three seeding entries at the cases of
tests/spline_bits_cases.py into tests/golden/spline_bits.npz -- from the build whose results are to be kept, before a kernel
line is changed.  Every case runs twice; nothing is written if the two runs differ.
Usage: python tools/record_spline_bits.py [--lib path/libnfopp_hip.so] [out.npz]     (--check: compare instead of writing)
Without --lib the product library is used."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "pytorch-motion-planner_amd"), ROOT):
    sys.path.insert(0, p)
import spline_bits_cases as sc  # noqa: E402
from nfopp import _lib  # noqa: E402

args = sys.argv[1:]
check = "--check" in args
args = [a for a in args if a != "--check"]
lib = None
if "--lib" in args:
    i = args.index("--lib")
    lib = ctypes.CDLL(os.path.abspath(args[i + 1]))
    for name, (res, argtypes) in _lib._SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, argtypes
    del args[i:i + 2]
path = args[0] if args else os.path.join(ROOT, "tests", "golden", "spline_bits.npz")

for c in sc.SEED_CASES:
    assert sc.seed_sites_distinct(c), "%s has two equal sites: its output would be NaN" % sc.seed_tag(c)
res = sc.run_cases(lib)
again = sc.run_cases(lib)      # the kernels are deterministic: a second run must give the same words
differ = [k for k in res if not np.array_equal(sc.words(res[k]), sc.words(again[k]))]
if differ:
    sys.exit("two runs of the same build differ in %s: nothing written" % differ)
for k, v in res.items():
    assert k.startswith("post_") or np.isfinite(v).all(), "%s is not finite" % k
if check:
    z = np.load(path)
    assert sorted(z.files) == sorted(res), "case lists differ"
    bad = [k for k in res if res[k].dtype != z[k].dtype or not np.array_equal(sc.words(res[k]), sc.words(z[k]))]
    print("%d arrays, %d differ %s" % (len(res), len(bad), bad[:8]))
    sys.exit(1 if bad else 0)
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
np.savez_compressed(path, **res)
print("%s: %d arrays, %d bytes" % (path, len(res), os.path.getsize(path)))
for name in sc.POST_CASES:
    print("  post_%s: count %s" % (name, res["post_%s_count" % name].tolist()))
