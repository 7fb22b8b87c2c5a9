"""GPU: the cases of the K1 / K2 bit fixtures, run live, against float64 (tests/float64_ref.py) through the comparer that
tests/test_bits_float64_cpu.py applies to the recorded words (tests/bits_float64_gate.py: 8 x the fp32 oracle's own error on
the same case and array).  A build whose bits have moved fails tests/test_gpu_k1_bits.py, test_gpu_k1_kind_bits.py or
test_gpu_k2_bits.py; this module says whether the new bits are still right, at exactly the shapes those fixtures exist for.

K1  every pose, edge, trajectory and logits case of both case modules on matrix paths 1, 2 and 0 (the recordings are path
    1's: the other two never saw the edge poses), the fit cases on the three paths through the summed gradient, the pass-1
    factors on path 1 (their layout is that path's own)
K2  every case with the loss terms, without them, and with trajectory 1 retired (its rows equal the inputs word for word)

The launches are those of the case modules (run_cases() / run_case and their helpers) and of test_gpu_split_path._fit_grad."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

gc = pytest.importorskip("gpu_common")
from nfopp import _lib  # noqa: E402

import bits_float64_gate as bg  # noqa: E402
import k1_bits_cases as kc  # noqa: E402
import k1_kind_bits_cases as kk  # noqa: E402
import k2_bits_cases as k2  # noqa: E402
from test_gpu_split_path import _fit_grad  # noqa: E402

MODS = {"k1_bits": kc, "k1_kind": kk}
PATHS = (1, 2, 0)


@pytest.fixture(scope="module")
def refs():
    """float64 and oracle32 values of both case modules: computed once, shared, never changed"""
    return {"k1_bits": bg.k1_reference(kc, kc.big_count()), "k1_kind": bg.k1_reference(kk)}


@pytest.fixture(scope="module")
def k2_refs():
    return {c: (bg.k2_reference(c), bg.k2_oracle32(c)) for c in k2.CASES}


def _outputs_on(mod, path, ref):
    """the pose, edge, trajectory and logits cases of a module on a matrix path, by the module's own launch helpers"""
    lib = _lib.load()
    before = lib.nfopp_get_matrix_path()
    _lib.check(lib.nfopp_set_matrix_path(path))
    out = {}
    try:
        assert lib.nfopp_get_matrix_path() == path
        for fin in mod.DIMS:
            onf = kc.make_onf(fin)
            for name, r in ref.items():
                if r["fin"] != fin or r["kind"] == "fit":
                    continue
                if r["kind"] == "traj":
                    out[name] = mod._traj(lib, onf, fin)
                elif r["kind"] == "big":
                    n = kc.big_count()
                    out[name] = kc._eval(lib, lib.nfopp_onf_eval_points, onf, kc.points(fin, n, 900))[bg.big_rows(n)]
                else:
                    fn = lib.nfopp_onf_eval_logits if r["kind"] == "logits" else lib.nfopp_onf_eval_points
                    out[name] = kc._eval(lib, fn, onf, r["x"])
    finally:
        _lib.check(lib.nfopp_set_matrix_path(before))
    return out


def _judge(rows, what):
    print("%s: worst ratio of the device's error to the oracle's %.2f" % (what, bg.worst_ratio(rows)))
    print("\n".join(bg.summary(rows)))
    assert not bg.failures(rows), (what, bg.failures(rows))


@pytest.mark.parametrize("tag", sorted(MODS))
def test_k1_cases_and_fit_factors_on_path_1(tag, refs):
    """run_cases() itself: what the recorders store, the pass-1 factors included"""
    got = MODS[tag].run_cases()
    rows = bg.compare_k1(tag + " path1", got, refs[tag])
    assert any(r.array == "rho_de" for r in rows) and any(r.array == "record u is exact" for r in rows)
    _judge(rows, tag + " on matrix path 1")


@pytest.mark.parametrize("path", PATHS[1:])
@pytest.mark.parametrize("tag", sorted(MODS))
def test_k1_cases_on_the_other_matrix_paths(tag, path, refs):
    ref = refs[tag]
    got = _outputs_on(MODS[tag], path, ref)
    names = [n for n, r in ref.items() if r["kind"] != "fit"]
    assert sorted(got) == sorted(names)
    _judge(bg.compare_k1("%s path%d" % (tag, path), got, ref, only=names), "%s on matrix path %d" % (tag, path))


def test_the_helper_launches_are_those_of_run_cases(refs):
    """_outputs_on on path 1 gives the words of run_cases(): the other paths are judged on the same launches"""
    ref = refs["k1_kind"]
    got, want = _outputs_on(kk, 1, ref), kk.run_cases()
    for name in got:
        assert np.array_equal(got[name].view(np.uint32), want[name].view(np.uint32)), name


@pytest.mark.parametrize("path", PATHS)
def test_fit_gradient_on_every_matrix_path(path, refs):
    rows = []
    for tag, mod in sorted(MODS.items()):
        for name, r in refs[tag].items():
            if r["kind"] == "fit":
                g = _fit_grad(kc.make_onf(r["fin"]), r["x"], r["y"], path)
                rows += bg.compare_fit_grad("%s path%d" % (tag, path), name, g, r)
    assert len(rows) == 3 * 6       # F220 / F100 at P = 33 and 257, F220 / F120 at P = 33: gradient, loss, count
    _judge(rows, "fit gradient on matrix path %d" % path)


@pytest.mark.parametrize("case", k2.CASES, ids=[k2.tag(c) for c in k2.CASES])
def test_k2_cases(case, k2_refs):
    want, o32 = k2_refs[case]
    state = k2.arrays_of(case)[:-1]
    fill = np.full((k2.B, 8), k2.TERMS_FILL)
    rows = bg.compare_k2("k2 terms", case, k2.run_case(case), want, o32)
    got = k2.run_case(case, want_terms=False)
    rows += bg.compare_k2("k2 no terms", case, got, want, o32, names=state)
    assert np.array_equal(got["terms"], fill), "a null terms pointer, yet the buffer was written"
    before = k2.inputs(case)
    for want_terms in (True, False):
        got = k2.run_case(case, want_terms=want_terms, retired=1)
        rows += bg.compare_k2("k2 retired", case, got, want, o32, names=state + (("terms",) if want_terms else ()), rows_of=[0, 2])
        for k in state:
            assert np.array_equal(got[k][1].view(np.uint32), before[k][1].view(np.uint32)), (k, "the retired trajectory moved")
        assert np.array_equal(got["terms"][1], fill[1]) and (want_terms or np.array_equal(got["terms"], fill))
    _judge(rows, k2.tag(case))
