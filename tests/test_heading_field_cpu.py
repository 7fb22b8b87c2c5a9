"""CPU: the restatement of the heading-layered distance field (tests/heading_field_ref.py) has the properties the model is
defined by, the committed poses take every branch of the row, the hand case separates the model from the disc cover, the
restated planner step clears the behaviour scenario, and the built library exports the three entries and refuses what the
header says it refuses -- all without a device."""
import ctypes

import numpy as np
import pytest

import heading_field_cases as hc
import heading_field_ref as ref
import obstacle_map_ref as omr
import sdf_cases as sc
import sdf_ref
from oracle import nfopp_oracle as orc

F32 = np.float32


# ---- exports and ABI ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_entries():
    import nfopp
    from nfopp import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("nfopp_hdf_eval_points", "nfopp_traj_hdf_collision_eval", "nfopp_traj_steps_hdf"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTED_SYMBOLS
    assert _lib.load().nfopp_abi_version() == 6 == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.HeadingFieldC) == 48     # 8 + 3 * 4 + 3 * 4 + 4 + 2 * 4 = 44, padded to the pointer's 8
    assert nfopp.HeadingDistanceField.point_dim == 3 and "HeadingDistanceField" in nfopp.__all__


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_library_rejects_bad_arguments_without_a_device():
    """The argument checks come before any launch: they answer on a machine without a GPU too."""
    from nfopp import _lib
    lib = _lib.load()
    good = _lib.HeadingFieldC()
    good.sd_dev, good.layers, good.rows, good.cols = 4096, 4, 4, 4
    good.inv_res, good.layers_per_rad, good.gain = 1.0, 4 / (2 * np.pi), 1.0

    def field(**changes):
        f = _lib.HeadingFieldC.from_buffer_copy(good)
        for key, value in changes.items():
            setattr(f, key, value)
        return f

    bad = [field(sd_dev=None), field(layers=1), field(layers=65), field(layers=0), field(layers=-3), field(rows=1), field(cols=1),
           field(layers=64, rows=8192, cols=4096),        # 2^31 elements: one past the largest 32-bit index range
           field(layers=64, rows=2 ** 20, cols=2 ** 20)]
    for name in ("x0", "y0", "inv_res", "layers_per_rad", "margin", "gain"):
        bad += [field(**{name: v}) for v in (np.nan, np.inf, -np.inf)]
    st = _lib.StepScheduleC(1e-2, 0.9, 0.9, 0, 0, 0, 0, 0, 3, 1)
    for f in bad:
        assert lib.nfopp_hdf_eval_points(f, 4096, 1, 4096, None) == -1 and lib.nfopp_last_error()
        assert lib.nfopp_traj_hdf_collision_eval(f, 4096, 1, 4, 4096, 1, 0, 0, 0, 4096, None, None) == -1
    assert lib.nfopp_hdf_eval_points(None, 4096, 1, 4096, None) == -1
    assert lib.nfopp_hdf_eval_points(good, None, 1, 4096, None) == -1
    assert lib.nfopp_hdf_eval_points(good, 4096, 1, None, None) == -1
    assert lib.nfopp_hdf_eval_points(good, 4096, 1, 4100, None) == -1          # out4 not 16-byte aligned
    assert lib.nfopp_hdf_eval_points(good, 4096, -1, 4096, None) == -1
    assert lib.nfopp_hdf_eval_points(good, 4096, 2 ** 31 * 256, 4096, None) == -1     # beyond one launch
    for t_mode in (-1, 2):
        assert lib.nfopp_traj_hdf_collision_eval(good, 4096, 1, 4, 4096, t_mode, 0, 0, 0, 4096, None, None) == -1
    assert lib.nfopp_traj_hdf_collision_eval(None, 4096, 1, 4, 4096, 1, 0, 0, 0, 4096, None, None) == -1
    assert lib.nfopp_traj_hdf_collision_eval(good, None, 1, 4, 4096, 1, 0, 0, 0, 4096, None, None) == -1
    assert lib.nfopp_traj_hdf_collision_eval(good, 4096, 1, 4, None, 1, 0, 0, 0, 4096, None, None) == -1
    assert lib.nfopp_traj_hdf_collision_eval(good, 4096, 1, 4, 4096, 1, 0, 0, 0, None, None, None) == -1
    assert lib.nfopp_traj_hdf_collision_eval(good, 4096, 1, 4, 4096, 1, 0, 0, 0, 4104, None, None) == -1
    assert lib.nfopp_traj_hdf_collision_eval(good, 4096, 1, 1, 4096, 1, 0, 0, 0, 4096, None, None) == -1      # one waypoint
    assert lib.nfopp_traj_hdf_collision_eval(good, 4096, -1, 4, 4096, 1, 0, 0, 0, 4096, None, None) == -1
    assert lib.nfopp_traj_hdf_collision_eval(good, 4096, 2 ** 31, 4, 4096, 1, 0, 0, 0, 4096, None, None) == -1
    assert lib.nfopp_traj_steps_hdf(None, None, None, None, 1, None, None, None) == -1
    # the step loop refuses poses of two components, and a bad field at the first step's collision entry
    hp = _lib.TrajHyperC()
    for dim, f in ((2, good), (3, field(layers=1))):
        buf = _lib.TrajBuffersC(4096, 4096, 4096, None, None, 4096, 4096, 4096, 4096, 4096, 4096, None, None, 1, 4, dim, 1, 0, 4)
        assert lib.nfopp_traj_steps_hdf(f, hp, buf, st, 1, None, None, None) == -1
    # n = 0 and batch = 0 launch nothing and succeed
    assert lib.nfopp_hdf_eval_points(good, None, 0, None, None) == 0
    assert lib.nfopp_traj_hdf_collision_eval(good, None, 0, 4, None, 1, 0, 0, 0, None, None, None) == 0


def test_python_layer_rejects_bad_arguments_without_a_device():
    """The constructor checks its arguments before it touches the device."""
    import nfopp
    H = nfopp.HeadingDistanceField
    ok, b = np.zeros((4, 4, 4), np.uint8), (0.0, 1.0, 0.0, 1.0)
    for layers in (np.zeros((1, 4, 4), np.uint8), np.zeros((65, 4, 4), np.uint8), np.zeros((4, 1, 4), np.uint8),
                   np.zeros((4, 4, 1), np.uint8), np.zeros((4, 4), np.uint8)):
        with pytest.raises(ValueError):
            H(layers, b, 0.25)
    for kw in (dict(boundaries=(0.0, 1.0, 0.0)), dict(boundaries=(0.0, 1.0, np.nan, 1.0)), dict(resolution=0.0),
               dict(resolution=np.inf), dict(margin=np.nan), dict(gain=np.inf)):
        args = dict(layers=ok, boundaries=b, resolution=0.25)
        args.update(kw)
        with pytest.raises(ValueError):
            H(**args)
    import torch
    with pytest.raises(ValueError):
        H(torch.zeros(4, 4, 4, dtype=torch.float32), b, 0.25)

    class NoLabels(object):
        boundaries = b

    with pytest.raises(TypeError):
        H.from_checker(NoLabels(), 0.25)
    with pytest.raises(TypeError):
        H.from_checker(NoLabels(), None)


# ---- the slice rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hc.FIELD_LAYERS))
@pytest.mark.parametrize("border", [False, True])
def test_sign_and_finiteness_of_every_slice(name, border):
    lay = hc.FIELD_LAYERS[name]
    sd = ref.signed_distance_stack(lay.occupancy, lay.resolution, border)
    assert sd.dtype == F32 and sd.shape == lay.occupancy.shape and np.isfinite(sd).all()
    assert (sd[lay.occupancy != 0] < 0).all() and (sd[lay.occupancy == 0] > 0).all()
    # the case holds a slice without a blocked cell and one without a free cell
    blocked = lay.occupancy.reshape(len(sd), -1).sum(1)
    assert (blocked == 0).any() and (blocked == sd[0].size).any()
    far = F32(lay.resolution * (sd.shape[1] + sd.shape[2]))
    assert (sd[blocked == sd[0].size] == -far).all()
    if not border:
        assert (sd[blocked == 0] == far).all()


@pytest.mark.parametrize("name", ["3x2x9", "16x37x53", "64x9x12"])
def test_zero_crossing_on_the_cell_edge(name):
    """In every slice two edge-adjacent cells on either side of a wall's edge hold +resolution and -resolution."""
    lay = hc.FIELD_LAYERS[name]
    sd, occ, res = ref.signed_distance_stack(lay.occupancy, lay.resolution), lay.occupancy != 0, F32(lay.resolution)
    pairs = 0
    for a, b, sa, sb in ((occ[:, :, :-1], occ[:, :, 1:], sd[:, :, :-1], sd[:, :, 1:]), (occ[:, :-1], occ[:, 1:], sd[:, :-1], sd[:, 1:])):
        edge = a != b
        pairs += int(edge.sum())
        assert (np.abs(sa[edge]) == res).all() and (np.abs(sb[edge]) == res).all()
        assert (np.sign(sa[edge]) == -np.sign(sb[edge])).all()
    assert pairs > 0


# ---- the heading index -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_layers", hc.HEADING_LAYER_COUNTS)
def test_heading_index_against_an_independent_statement(n_layers):
    """k0, k1 and fw of the float64 restatement against np.floor and % on Python floats, at the delicate headings."""
    field = ref.Field(np.zeros((n_layers, 2, 2), F32), F32(0), F32(0), F32(1), F32(n_layers / (2 * np.pi)), F32(0), F32(1))
    theta = hc.heading_list(n_layers)
    k0, k1, fw, ok = ref.heading_index(field, theta, np.float64)
    assert ok.all()          # in float64 no committed heading overflows
    for th, a, b, f in zip(theta, k0, k1, fw):
        w = float(th) * float(field.layers_per_rad)
        base = float(np.floor(w))
        assert int(a) == int(base % n_layers) and int(b) == (int(a) + 1) % n_layers, th
        assert float(f) == w - base and 0.0 <= float(f) <= 1.0, th
    # and the float32 statement: in range wherever w is finite, w not finite only for the largest float at L / (2 pi) > 1
    k0, k1, fw, ok = ref.heading_index(field, theta, F32)
    assert ((k0 >= 0) & (k0 < n_layers) & (k1 >= 0) & (k1 < n_layers) & (fw >= 0) & (fw <= 1)).all()
    assert (~ok).sum() == (2 if n_layers / (2 * np.pi) > 1 else 0)


# ---- the gradient ------------------------------------------------------------------------------------------------------------
def test_float64_gradient_against_central_differences():
    """Inside a cell and a slice the float64 row's logit is trilinear in (x, y, theta), so a central difference in each
    component is exact up to rounding (values up to ~40 over h = 1e-4: 1e-10) and up to the cross terms, which a central
    difference of a trilinear function does not see at all.  Step and tolerance are those of tests/test_sdf_field_cpu.py."""
    lay = hc.FIELD_LAYERS["16x37x53"]
    field = hc.field_of(lay)
    poses = hc.random_poses(lay, 4096, 2, outside=0.0)
    h = 1e-4
    f64 = dict(dtype=np.float64, pose_dtype=np.float64)
    base, choice = ref.eval_points(field, poses, **f64)
    keep = choice[:, 4:6].all(1)                 # inside the image along both axes
    slope = []
    for comp in range(3):
        side = []
        for sign in (-1.0, 1.0):
            p = poses.astype(np.float64)
            p[:, comp] += sign * h
            out, ch = ref.eval_points(field, p, **f64)
            keep &= ref.same_branch(ch, choice)  # no cell line and no slice line within h
            side.append(out[:, 0])
        slope.append((side[1] - side[0]) / (2 * h))
    assert keep.sum() > len(poses) // 4          # the filter leaves a real sample
    for comp in range(3):
        assert np.abs(slope[comp] - base[:, 1 + comp])[keep].max() < 1e-4
        assert np.abs(base[:, 1 + comp])[keep].max() > 0


# ---- the hand case -----------------------------------------------------------------------------------------------------------
def test_hand_case_box_in_a_gap():
    """A 2 m x 0.5 m box in a gap of five cells: free by the rectangle checker, free by the layered field (d = +0.1, one cell),
    colliding by the four-disc cover; across the passage and one cell off its centre line the checker and the field both
    say collision.  At 0.2 rad, between two slices, the field is pessimistic: the model's stated limit."""
    import nfopp
    g, layers = hc.hand_case()
    points = omr.grid_points(g.occupancy.astype(F32), g.resolution, (0.0, 0.0, 0.0))
    field = hc.field_of(layers, margin=0.0, gain=10.0)

    def row(pose):
        return ref.eval_points(field, np.asarray([pose], F32))[0][0]

    def checker(pose):
        return bool(omr.rectangle_labels(np.asarray([pose], F32), points, hc.HAND_BOX)[0])

    assert not checker(hc.HAND_FREE)
    free = row(hc.HAND_FREE)
    assert free[0] < 0 and free[0] == F32(10.0) * (F32(0.0) - F32(0.1))
    discs = nfopp.DistanceField.discs_for_box(hc.HAND_BOX, 4)
    disc_row = sdf_ref.eval_points(sc.field_of(g, discs, margin=0.0, gain=10.0), np.asarray([hc.HAND_FREE], F32))[0][0]
    assert disc_row[0] > 0
    for pose in hc.HAND_BLOCKED:
        assert checker(pose) and row(pose)[0] > 0
    assert not checker(hc.HAND_BETWEEN) and row(hc.HAND_BETWEEN)[0] > 0


# ---- coverage ----------------------------------------------------------------------------------------------------------------
def test_committed_poses_take_every_branch():
    layers, poses = hc.coverage_poses()
    n_layers = layers.occupancy.shape[0]
    field = hc.field_of(layers)
    out, choice = ref.eval_points(field, poses, F32)
    k0, k1, in_x, in_y, nan_row = choice[:, 0], choice[:, 1], choice[:, 4], choice[:, 5], choice[:, 6]
    live = nan_row == 0
    assert ((k1 == 0) & (k0 == n_layers - 1) & live).any()                  # the wrap
    with np.errstate(over="ignore"):
        w = poses[:, 2] * field.layers_per_rad
    r = np.fmod(np.floor(np.where(np.isfinite(w), w, 0)), F32(n_layers))
    assert ((r < 0) & live).any()                                            # a negative remainder
    _, _, fw, _ = ref.heading_index(field, np.where(np.isfinite(poses[:, 2]), poses[:, 2], 0), F32)
    assert ((fw == 0) & live).any() and ((fw > 0) & live).any()
    assert ((in_x == 0) & live).any() and ((in_y == 0) & live).any() and ((in_x == 1) & (in_y == 1) & live).any()
    assert nan_row.any() and np.isnan(out[nan_row == 1]).all() and np.isfinite(out[live]).all()
    assert (nan_row[np.isfinite(poses).all(1)] == 1).any()                   # a finite heading whose w overflows
    # the counts the GPU test launches hold a NaN row each, and the larger ones every branch above
    for count in hc.POINT_COUNTS:
        assert ref.eval_points(field, hc.point_poses(layers, count), F32)[1][:, 6].any()


# ---- behaviour: the restated pipeline ----------------------------------------------------------------------------------------
def test_restated_pipeline_clears_the_wall():
    """heading_field_ref.planner_step from the straight seeds: every seed collides by rectangle_labels, and every path is free
    by rectangle_labels at every step from BEHAVIOUR_FIRST_PASS to BEHAVIOUR_STEPS, and not at the step before.  Margin 0.1,
    gain 10 and the weights of sdf_cases.behaviour_case were the first choice; nothing was changed to get here."""
    import nfopp
    case = hc.behaviour_case()
    field = hc.field_of(case["layers"], case["margin"], case["gain"])
    hp = orc.Hyper(**case["hyper"])
    B, N = len(case["starts"]), case["n_waypoints"]
    s = dict(traj=nfopp.straight_line_init(case["starts"], case["goals"], N), start=case["starts"], goal=case["goals"],
             lam=np.zeros((B, N + 1), F32), cm=np.zeros((B, N), F32), adam_m=np.zeros((B, N, 3), F32),
             adam_v=np.zeros((B, N, 3), F32), adam_step=0, step_count=0)
    hinv = orc.calculate_inv_hessian(N, 0.5)

    def collides():
        poses, _ = orc.path_interpolate(s["traj"], s["start"], s["goal"], 4)
        return omr.rectangle_labels(poses.reshape(-1, 3), case["points"], case["box"],
                                    case["grid"].boundaries).reshape(B, -1).any(1)

    assert collides().all()
    for k in range(hc.BEHAVIOUR_STEPS):
        ref.planner_step(field, s, case["draws"][k], hp, hinv, case["reparam_freq"])
        if k + 1 == hc.BEHAVIOUR_FIRST_PASS - 1:
            assert collides().any()
        if k + 1 >= hc.BEHAVIOUR_FIRST_PASS:
            assert not collides().any(), k + 1
