"""Dev tool: record the contract of torch.ops.nfopp.* at the cases of tests/torch_ops_contract_cases.py into
tests/golden/torch_ops_contract.npz -- from the build whose behaviour is to be kept, before csrc/torch_ops.cpp is changed.
Usage: python tools/record_torch_ops_contract.py [out.npz]     (--check: compare instead of writing; -v: print every text)
The schema strings need no GPU: without one they alone are recorded, and the rest of an existing file is kept.  With one,
the refusal texts and the outputs of the accepted edges are recorded too (the second-device texts on a box that has two).
A case that is not refused is reported and the tool exits 1: it has no place in the list (the parent accepts that input)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "pytorch-motion-planner_amd"), ROOT):
    sys.path.insert(0, p)
import torch_ops_contract_cases as cc  # noqa: E402
from nfopp import torch_ops  # noqa: E402

args = sys.argv[1:]
check, verbose = "--check" in args, "-v" in args
args = [a for a in args if a not in ("--check", "-v")]
path = args[0] if args else os.path.join(ROOT, "tests", "golden", "torch_ops_contract.npz")

ops = torch_ops.load()
res = {"schema/" + op: np.array(str(getattr(torch.ops.nfopp, op).default._schema)) for op in torch_ops.OPS}
accepted = []
if torch.cuda.is_available():
    dev = "cuda:0"
    for case in cc.CASES:
        text = cc.run_case(ops, case, dev)
        if text is None:
            accepted.append(case[0])
        else:
            res["refusal/" + case[0]] = np.array(text)
    if torch.cuda.device_count() >= 2:
        for case in cc.DEVICE_CASES:
            text = cc.run_device_case(ops, case, dev, "cuda:1")
            if text is None:
                accepted.append(case[0])
            else:
                res["device/" + case[0]] = np.array(text)
    for name in cc.EDGES:
        got, again = cc.run_edge(ops, name, dev), cc.run_edge(ops, name, dev)
        assert all(a[1:] == b[1:] and np.array_equal(a[0], b[0]) for a, b in zip(got, again)), name + ": two runs differ"
        res["edge/%s/n" % name] = np.array(len(got))
        for i, (raw, shape, stride, dtype) in enumerate(got):
            res["edge/%s/%d/bytes" % (name, i)] = raw
            res["edge/%s/%d/shape" % (name, i)] = np.array(shape, np.int64)
            res["edge/%s/%d/stride" % (name, i)] = np.array(stride, np.int64)
            res["edge/%s/%d/dtype" % (name, i)] = np.array(dtype)
    torch.cuda.synchronize()
elif os.path.exists(path):
    res.update({k: v for k, v in np.load(path, allow_pickle=False).items() if not k.startswith("schema/")})
if verbose:
    for k in sorted(res):
        if res[k].dtype.kind == "U":
            print("%s\t%s" % (k, res[k]))
for name in accepted:
    print("NOT REFUSED: " + name)
if check:
    z = np.load(path, allow_pickle=False)
    bad = sorted(set(z.files) ^ set(res)) + [k for k in res if k in z.files and not (
        z[k].dtype == res[k].dtype and z[k].shape == res[k].shape and z[k].tobytes() == res[k].tobytes())]
    print("%d entries, %d differ %s" % (len(res), len(bad), bad[:8]))
    sys.exit(1 if bad or accepted else 0)
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
np.savez_compressed(path, **res)
print("%s: %d entries (%d refusals, %d on a second device, %d edges), %d bytes" % (
    path, len(res), sum(k.startswith("refusal/") for k in res), sum(k.startswith("device/") for k in res), len(cc.EDGES),
    os.path.getsize(path)))
sys.exit(1 if accepted else 0)
