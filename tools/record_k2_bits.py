"""GPU dev tool: record the trajectory-update kernel's output bits at the shapes of tests/k2_bits_cases.py into
tests/golden/k2_bits.npz -- from the build whose results are to be kept, before the kernel is changed.
Usage: python tools/record_k2_bits.py [--lib path/libnfopp_hip.so] [out.npz]     (--check: compare instead of writing)
Without --lib the product library is used."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "pytorch-motion-planner_amd"), ROOT):
    sys.path.insert(0, p)
import k2_bits_cases as kc  # noqa: E402
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
path = args[0] if args else os.path.join(ROOT, "tests", "golden", "k2_bits.npz")


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


res = kc.run_cases(lib)
again = kc.run_cases(lib)     # the kernel is deterministic: a second run must give the same words
for k in res:
    assert np.array_equal(words(res[k]), words(again[k])), k
if check:
    z = np.load(path)
    assert sorted(z.files) == sorted(res), "case lists differ"
    bad = [k for k in res if not np.array_equal(words(res[k]), words(z[k]))]
    for c in kc.CASES:         # the state must not depend on whether the loss terms are asked for
        got = kc.run_case(c, lib, want_terms=False)
        bad += ["%s_%s (no terms)" % (kc.tag(c), k) for k in kc.arrays_of(c)[:-1]
                if not np.array_equal(words(got[k]), words(z["%s_%s" % (kc.tag(c), k)]))]
    print("%d arrays, %d differ %s" % (len(res), len(bad), bad[:8]))
    sys.exit(1 if bad else 0)
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
np.savez_compressed(path, **res)
print("%s: %d arrays, %d bytes" % (path, len(res), os.path.getsize(path)))
