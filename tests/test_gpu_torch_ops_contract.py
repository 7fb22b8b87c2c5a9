"""GPU: the contract of torch.ops.nfopp.* (csrc/torch_ops.cpp) against its recording, tests/golden/torch_ops_contract.npz
(tools/record_torch_ops_contract.py, from the shim before its rules were stated once).  The cases are those of
tests/torch_ops_contract_cases.py: every refusal keeps its text (the first line of the error: which check fires, and what
it names), every accepted edge its outputs bit for bit, with their shapes, strides and dtypes."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

import torch_ops_contract_cases as cc  # noqa: E402
from nfopp import torch_ops  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def recorded():
    return load_golden("torch_ops_contract.npz")


def test_the_recording_holds_these_cases(recorded):
    keys = set(recorded.files)
    assert {k[len("refusal/"):] for k in keys if k.startswith("refusal/")} == {c[0] for c in cc.CASES}
    assert {k[len("device/"):] for k in keys if k.startswith("device/")} <= {c[0] for c in cc.DEVICE_CASES}
    assert {k.split("/")[1] + "/" + k.split("/")[2] for k in keys if k.startswith("edge/")} == set(cc.EDGES)
    assert {c[1] for c in cc.CASES} == set(torch_ops.OPS)


@pytest.mark.parametrize("op", torch_ops.OPS)
def test_refusals_keep_their_text(op, recorded):
    ops = torch_ops.load()
    wrong = []
    for case in (c for c in cc.CASES if c[1] == op):
        got, want = cc.run_case(ops, case, DEV), str(recorded["refusal/" + case[0]])
        print("%s\t%s" % (case[0], got))
        if got != want:
            wrong.append((case[0], got, want))
    assert not wrong, wrong


def test_second_device_refusals_keep_their_text(recorded):
    cases = [c for c in cc.DEVICE_CASES if "device/" + c[0] in recorded.files]
    if torch.cuda.device_count() < 2 or not cases:
        pytest.skip("needs two visible devices, and a recording from a box that had them")
    ops = torch_ops.load()
    wrong = []
    for case in cases:
        got, want = cc.run_device_case(ops, case, DEV, "cuda:1"), str(recorded["device/" + case[0]])
        if got != want:
            wrong.append((case[0], got, want))
    assert not wrong, wrong


@pytest.mark.parametrize("name", list(cc.EDGES))
def test_accepted_edges_keep_their_outputs(name, recorded):
    got = cc.run_edge(torch_ops.load(), name, DEV)
    assert len(got) == int(recorded["edge/%s/n" % name])
    for i, (raw, shape, stride, dtype) in enumerate(got):
        pre = "edge/%s/%d/" % (name, i)
        assert shape == tuple(recorded[pre + "shape"]) and dtype == str(recorded[pre + "dtype"]), (i, shape, dtype)
        assert stride == tuple(recorded[pre + "stride"]), (i, stride)
        assert raw.tobytes() == recorded[pre + "bytes"].tobytes(), (i, np.flatnonzero(raw != recorded[pre + "bytes"])[:8])
