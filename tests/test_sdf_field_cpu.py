"""CPU: the restatement of the distance-field collision model (tests/sdf_ref.py) has the properties the model is defined by,
the committed cases meet the condition under which the GPU tests compare against float64, the restated planner step clears
the behaviour scenario with steps to spare, and the built library exports the three entries."""
import ctypes

import numpy as np
import pytest

import sdf_cases as sc
import sdf_ref as ref
from oracle import nfopp_oracle as orc

F32 = np.float32


# ---- the field -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.FIELD_GRIDS))
@pytest.mark.parametrize("border", [False, True])
def test_sign_and_finiteness(name, border):
    g = sc.FIELD_GRIDS[name]
    sd = ref.signed_distance(g.occupancy, g.resolution, border)
    assert sd.dtype == F32 and np.isfinite(sd).all()
    assert (sd[g.occupancy != 0] < 0).all() and (sd[g.occupancy == 0] > 0).all()
    rows, cols = g.occupancy.shape
    far = F32(g.resolution * (rows + cols))
    if name == "no_walls" and not border:
        assert (sd == far).all()
    if name == "all_walls":
        assert (sd == -far).all()


@pytest.mark.parametrize("name", ["2x2", "2x9", "37x53"])
def test_zero_crossing_on_the_cell_edge(name):
    """Two edge-adjacent cells on either side of a wall's edge hold +resolution and -resolution."""
    g = sc.FIELD_GRIDS[name]
    sd, occ, res = ref.signed_distance(g.occupancy, g.resolution), g.occupancy != 0, F32(g.resolution)
    pairs = 0
    for a, b, sa, sb in ((occ[:, :-1], occ[:, 1:], sd[:, :-1], sd[:, 1:]), (occ[:-1], occ[1:], sd[:-1], sd[1:])):
        edge = a != b
        pairs += int(edge.sum())
        assert (np.abs(sa[edge]) == res).all() and (np.abs(sb[edge]) == res).all()
    assert pairs > 0


# ---- the row ---------------------------------------------------------------------------------------------------------------------
def test_float64_gradient_against_central_differences():
    """Away from cell lines and from disc switches the float64 row's gradient is the derivative of its logit.  The logit is
    bilinear in the disc centre, so a central difference in x or y is exact up to rounding (values up to ~40 over h = 1e-4 m:
    1e-10); in theta the centre moves on a circle of radius <= 0.26 m and the error is h^2 / 6 times a third derivative of the
    order gain * |offset| * (|grad| + |offset| * cross term / resolution) < 1e3, so below 2e-6."""
    grid, discs, margin, gain, border, poses = sc.F64_CASES["trial"]
    field = sc.field_of(grid, discs, margin, gain, border)
    h = 1e-4
    f64 = dict(dtype=np.float64, pose_dtype=np.float64)
    base, choice = ref.eval_points(field, poses, **f64)
    keep = choice[:, 3:].all(1)                  # inside the image along both axes
    slope = []
    for comp in range(3):
        side = []
        for sign in (-1.0, 1.0):
            p = poses.astype(np.float64)
            p[:, comp] += sign * h
            out, ch = ref.eval_points(field, p, **f64)
            keep &= ref.same_branch(ch, choice)  # no cell line and no disc switch within h
            side.append(out[:, 0])
        slope.append((side[1] - side[0]) / (2 * h))
    assert keep.sum() > len(poses) // 4          # the filter leaves a real sample
    for comp in range(3):
        assert np.abs(slope[comp] - base[:, 1 + comp])[keep].max() < 1e-4


def test_box_cover():
    """discs_for_box: n equal discs along the longer axis, every point of the box inside one of them, and no smaller radius
    covers the box's corners."""
    import nfopp
    for box, n in (((-0.3, 0.5, -0.12, 0.12), 5), ((-0.1, 0.1, -0.4, 0.6), 3), ((0.0, 1.0, 0.0, 1.0), 1), ((-0.2, 0.2, -0.1, 0.1), 8)):
        discs = nfopp.DistanceField.discs_for_box(box, n)
        assert discs.shape == (n, 3) and (discs[:, 2] == discs[0, 2]).all()
        longer = 0 if box[1] - box[0] >= box[3] - box[2] else 1
        assert (np.diff(discs[:, longer]) > 0).all() and (discs[:, 1 - longer] == discs[0, 1 - longer]).all()
        x, y = np.meshgrid(np.linspace(box[0], box[1], 81), np.linspace(box[2], box[3], 81))
        d = np.hypot(x[..., None] - discs[:, 0], y[..., None] - discs[:, 1])
        assert (d.min(-1) <= discs[0, 2] * (1 + 1e-12)).all()
        corner = np.hypot(box[0] - discs[:, 0], box[2] - discs[:, 1]).min()
        assert corner >= discs[0, 2] * (1 - 1e-12)      # a smaller disc would leave the corner out


def test_tie_takes_the_lower_index():
    grid, discs, poses, gain = sc.tie_case()
    for order, sign in ((discs, -1.0), (discs[::-1], 1.0)):
        out, choice = ref.eval_points(sc.field_of(grid, order, gain=gain), poses, F32)
        assert (choice[:, 0] == 0).all()
        assert (out[:, 2] == F32(sign * gain)).all() and (out[:, 1] == 0).all()


# ---- the condition of the float64 comparisons --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.F64_CASES))
def test_excluded_share(name):
    grid, discs, margin, gain, border, poses = sc.F64_CASES[name]
    spread, kept = ref.spread(sc.field_of(grid, discs, margin, gain, border), poses)
    share = 1.0 - kept.mean()
    print("%s: excluded %d of %d, SPREAD %s" % (name, (~kept).sum(), len(kept), spread))
    assert share <= sc.MAX_EXCLUDED_SHARE
    assert np.isfinite(spread).all()


# ---- behaviour: the restated pipeline --------------------------------------------------------------------------------------------
def test_restated_pipeline_clears_the_wall():
    """sdf_ref.planner_step from the straight seeds: every seed collides, every path is free from BEHAVIOUR_FIRST_PASS on at the
    latest and still free after the BEHAVIOUR_STEPS steps the GPU test runs."""
    import nfopp
    case = sc.behaviour_case()
    g = case["grid"]
    field = sc.field_of(g, case["discs"], case["margin"], case["gain"])
    hp = orc.Hyper(**case["hyper"])
    B, N = len(case["starts"]), case["n_waypoints"]
    s = dict(traj=nfopp.straight_line_init(case["starts"], case["goals"], N), start=case["starts"], goal=case["goals"],
             lam=np.zeros((B, N + 1), F32), cm=np.zeros((B, N), F32), adam_m=np.zeros((B, N, 3), F32),
             adam_v=np.zeros((B, N, 3), F32), adam_step=0, step_count=0)
    hinv = orc.calculate_inv_hessian(N, 0.5)

    def collides():
        poses, _ = orc.path_interpolate(s["traj"], s["start"], s["goal"], 4)
        return orc.grid_check(poses.reshape(-1, 3)[:, :2], g.occupancy, g.boundaries[0], g.boundaries[2],
                              g.resolution).reshape(B, -1).any(1)

    assert collides().all()
    for k in range(sc.BEHAVIOUR_STEPS):
        ref.planner_step(field, s, case["draws"][k], hp, hinv, case["reparam_freq"])
        if k + 1 >= sc.BEHAVIOUR_FIRST_PASS:
            assert not collides().any(), k + 1


# ---- the library -----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entries():
    from nfopp import _lib
    names = ("nfopp_sdf_eval_points", "nfopp_traj_sdf_collision_eval", "nfopp_traj_steps_sdf")
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert lib.nfopp_abi_version() == 6 == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.SdfFieldC) == 136     # 8 + 2 * 4 + 3 * 4 + 4 + 8 * 3 * 4 + 2 * 4, no padding


def test_library_rejects_bad_arguments_without_a_device():
    """The argument checks come before any launch: they answer on a machine without a GPU too."""
    from nfopp import _lib
    lib = _lib.load()
    good = _lib.SdfFieldC()
    good.sd_dev, good.rows, good.cols, good.n_discs, good.inv_res, good.gain = 4096, 4, 4, 1, 1.0, 1.0

    def field(**changes):
        f = _lib.SdfFieldC.from_buffer_copy(good)
        for key, value in changes.items():
            setattr(f, key, value)
        return f

    offset = field()
    offset.disc[0][0] = 0.1
    bad = [(field(rows=1), 3), (field(cols=1), 3), (field(n_discs=0), 3), (field(n_discs=9), 3), (field(sd_dev=None), 3),
           (offset, 2), (field(n_discs=2), 2), (field(), 4)]
    for f, dim in bad:
        assert lib.nfopp_sdf_eval_points(f, 4096, 1, dim, 4096, None) == -1
        assert lib.nfopp_traj_sdf_collision_eval(f, 4096, 1, 4, dim, 4096, 1, 0, 0, 0, 4096, None, None) == -1
    assert lib.nfopp_sdf_eval_points(None, 4096, 1, 3, 4096, None) == -1
    assert lib.nfopp_sdf_eval_points(good, None, 1, 3, 4096, None) == -1
    assert lib.nfopp_sdf_eval_points(good, 4096, 1, 3, None, None) == -1
    assert lib.nfopp_sdf_eval_points(good, 4096, 1, 3, 4100, None) == -1       # out4 not 16-byte aligned
    assert lib.nfopp_sdf_eval_points(good, 4096, -1, 3, 4096, None) == -1
    for t_mode in (-1, 2):
        assert lib.nfopp_traj_sdf_collision_eval(good, 4096, 1, 4, 3, 4096, t_mode, 0, 0, 0, 4096, None, None) == -1
    assert lib.nfopp_traj_sdf_collision_eval(good, None, 1, 4, 3, 4096, 1, 0, 0, 0, 4096, None, None) == -1
    assert lib.nfopp_traj_sdf_collision_eval(good, 4096, 1, 4, 3, None, 1, 0, 0, 0, 4096, None, None) == -1
    assert lib.nfopp_traj_sdf_collision_eval(good, 4096, 1, 1, 3, 4096, 1, 0, 0, 0, 4096, None, None) == -1
    assert lib.nfopp_traj_steps_sdf(None, None, None, None, 1, None, None, None) == -1
    # n = 0 and batch = 0 launch nothing and succeed
    assert lib.nfopp_sdf_eval_points(good, None, 0, 3, None, None) == 0
    assert lib.nfopp_traj_sdf_collision_eval(good, None, 0, 4, 3, None, 1, 0, 0, 0, None, None, None) == 0
