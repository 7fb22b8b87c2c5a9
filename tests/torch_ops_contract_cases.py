"""The contract of torch.ops.nfopp.* (csrc/torch_ops.cpp) as a list of calls: what the shim refuses and with which words, and
what it makes of the empty and one-element edges.  tests/test_gpu_torch_ops_contract.py runs them against
tests/golden/torch_ops_contract.npz, which tools/record_torch_ops_contract.py writes from the build whose behaviour is to
be kept.  The shim holds no arithmetic, so the recording pins argument order, pointer rules and message texts, not numbers.

Every op has one valid call (`BASE[op]`: named arguments, every optional tensor present) at the smallest shapes the checks
allow.  A refusal is that call with ONE thing wrong; ops are called by keyword, so a case names what it changes.  Three kinds:
  * written out below (`_explicit`): one per TORCH_CHECK of the op that is not a per-tensor check, one per shape the op
    states for a tensor, and one C-side refusal (`c_...`) per op family whose scalars the shim forwards unchecked;
  * generated: every tensor argument of every op with another dtype (`dtype_<arg>`) and non-contiguous (`strided_<arg>`);
  * generated, second device only (`DEVICE_CASES`): every tensor argument of an op with two or more on another device.
A refused call launches nothing that reads its malformed argument: the C-side refusals are argument checks of the entry
points (include/nfopp_hip.h), and what an op launches before one (the distance fields of grid_search_init, the headings
of box_track_conflicts, the reservation image of spacetime_reserve) is given valid tensors.

Checks no case reaches: none.  The three that look out of reach are reached without memory: a tracks tensor of 2^31
instants has no rows ([0, 2^31, 2]), the reservation that no int32 indexes is a 4 x 4 image with count 2^31 - 1, and only
"image too large for an index" needs a real allocation, of 2 GiB that nothing reads or writes.

Accepted edges (`EDGES`) return every output of the op, and the tensors it updates in place.  Each of them is fully written
by the parent for these inputs (an empty set A leaves the conflict entries nothing to write and the shim fills summary_b
itself; the lattice traces start from zeros), so none is excluded from the comparison."""
import ctypes

import numpy as np
import torch

from nfopp import _lib

B, N, K, HW, SIDE = 2, 4, 2, 1, 4
F32, F64, I32, I64, U8, I8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8, torch.int8
_OTHER_DTYPE = {F32: F64, F64: F32, I32: I64, I64: I32, U8: I32, I8: I32}
LIMITS = [2.0, 1.0, 1.0, 1.0, 1.0, -0.5]


def onf_cfg(d):
    """one ONF configuration per point dimension"""
    return dict(mean=0.0, sigma=1.0, use_cos=True, has_bias=True, angle_dim=10 if d == 3 else 0)


def n_params(d):
    c = onf_cfg(d)
    cfg = _lib.OnfConfigC(c["mean"], c["sigma"], int(c["use_cos"]), int(c["has_bias"]), c["angle_dim"])
    return int(_lib.load().nfopp_onf_param_count(ctypes.byref(cfg)))


def reservation_words(count=K):
    return int(_lib.load().nfopp_spacetime_reservation_bytes(SIDE, SIDE, count)) // 8


def _f(dev, *shape, seed=0, lo=0.5, hi=3.5):
    return torch.tensor(np.random.RandomState(seed).uniform(lo, hi, shape).astype(np.float32), device=dev)


def _z(dev, *shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype, device=dev)


def _i(dev, rows, width=None):
    """int32 rows; `width` shapes an empty list"""
    t = torch.tensor(rows, dtype=I32, device=dev)
    return t.reshape(0, width) if width is not None and t.numel() == 0 else t


def _params(dev, d):
    return _f(dev, n_params(d), seed=7, lo=-0.1, hi=0.1)


# ---- the valid call of every op ------------------------------------------------------------------------------------------------
def _batch(dev, d, b=B):
    a = dict(traj=_f(dev, b, N, d), start=_f(dev, b, d, seed=1), goal=_f(dev, b, d, seed=2))
    a["lam"], a["cm"] = (_z(dev, b, N + 1), _z(dev, b, N)) if d == 3 else (None, None)
    return a


def _onf_points(dev, d=3, p=2):
    return dict(params=_params(dev, d), points=_f(dev, p, d), **onf_cfg(d))


def _step(dev, d=3):
    a = dict(params=_params(dev, d), **onf_cfg(d), **_batch(dev, d))
    a.update(adam_m=_z(dev, B, N, d), adam_v=_z(dev, B, N, d), t=_z(dev, B, N - 1), seed=0, rng_offset=0, traj_index_offset=0,
             onf_out=_z(dev, B, N - 1, 4), hinv_band=_z(dev, 2 * HW + 1, N), half_width=HW, interior_lo=1, interior_hi=N - 1,
             hyper=[0.0] * 18, terms=_z(dev, B, 8), active=torch.ones(B, dtype=U8, device=dev), live_ws=_z(dev, B + 1, dtype=I32))
    return a


def _traj_step(dev, d=3):
    return dict(_step(dev, d), t_mode=0)


def _traj_steps(dev, d=3):
    return dict(_step(dev, d), t_steps=_z(dev, 1, B, N - 1), u=_f(dev, N, seed=3), adam_lr=1e-2, adam_beta1=0.9, adam_beta2=0.9,
                adam_steps_done=0, step_count=0, reparam_freq=10, n_steps=1)


def _reparametrize(dev, d=3):
    return dict(_batch(dev, d), u=_f(dev, N, seed=3), active=torch.ones(B, dtype=U8, device=dev))


def _update_endpoints(dev, d=3):
    return dict(_batch(dev, d), u=_f(dev, N, seed=3), points=_f(dev, B, d, seed=4), which=1,
                moved=torch.ones(B, dtype=U8, device=dev), min_index=_z(dev, B, dtype=I32))


def _endpoints(dev, d=3, b=B):
    a = _batch(dev, d, b)
    return dict(traj=a["traj"], start=a["start"], goal=a["goal"])


def _grid_search_init(dev, d=3, b=B, g=2):
    cells = [[0, 0], [1, 1]][:b]
    return dict(_endpoints(dev, d, b), occupancy=_z(dev, SIDE, SIDE, dtype=U8), start_cells=_i(dev, cells, 2),
                goal_cells=_i(dev, [[3, 3], [2, 3]][:b], 2), unique_goal_cells=_i(dev, [[3, 3], [2, 3]][:g], 2),
                field_index=_i(dev, [0, 1][:b]), origin_x=0.0, origin_y=0.0, resolution=1.0, angles_with_direction=False)


def _onf_train_grad(dev, d=3):
    return dict(params=_params(dev, d), samples=_f(dev, 2, d), labels=_z(dev, 2), inv_count=0.5, **onf_cfg(d))


_ADAM = dict(beta2=0.9, omb1=0.1, omb2=0.1, eps=1e-8, step_size=0.01, bc2_sqrt=1.0)


def _adam_step(dev):
    return dict(param=_z(dev, 4), grad=_z(dev, 4), m=_z(dev, 4), v=_z(dev, 4), **_ADAM)


def _onf_train_step(dev, d=3):
    n = n_params(d)
    return dict(params=_params(dev, d), m=_z(dev, n), v=_z(dev, n), samples=_f(dev, 2, d), labels=_z(dev, 2), **onf_cfg(d), **_ADAM)


def _path_time_profile(dev, d=3):
    return dict(_endpoints(dev, d), limits=list(LIMITS), v_start=_z(dev, B), v_goal=_z(dev, B))


def _path_time_sample(dev, d=3, count=2):
    return dict(_endpoints(dev, d), limits=list(LIMITS), profile=_z(dev, B, N + 2, 4, dtype=F64),
                gear=torch.ones(B, N + 1, dtype=I8, device=dev), t0=0.0, dt=0.1, count=count)


def _track_conflicts(dev, ba=B, bb=B, k=K, s=2):
    """bb None: self mode"""
    a = dict(tracks_a=_f(dev, ba, k, s), tracks_b=None if bb is None else _f(dev, bb, k, s, seed=1), dt=0.25, t0=0.0,
             radius_a=_f(dev, ba, seed=2, lo=0.1, hi=0.6), radius_b=None if bb is None else _f(dev, bb, seed=3, lo=0.1, hi=0.6),
             margin=0.05, want_pairs=True)
    return a


def _track_headings(dev):
    return dict(tracks=_f(dev, B, K, 3))


def _box_track_conflicts(dev, ba=B, bb=B, k=K):
    a = _track_conflicts(dev, ba, bb, k, 3)
    a.update(box_a=_f(dev, ba, 4, seed=4, lo=0.1, hi=0.6), box_b=None if bb is None else _f(dev, bb, 4, seed=5, lo=0.1, hi=0.6),
             refine=1)
    return a


def _fleet_shift_masks(dev, b=B, m=B):
    """m None: no obstacles"""
    return dict(tracks=_f(dev, b, K, 2), max_delay=1, radius=_f(dev, b, seed=2, lo=0.1, hi=0.6), margin=0.05,
                obstacles=None if m is None else _f(dev, m, K + 1, 2, seed=1),
                obstacle_radius=None if m is None else _f(dev, m, seed=3, lo=0.1, hi=0.6))


def _fleet_assign_delays(dev, b=B):
    return dict(pair=_z(dev, b, b, 2, dtype=I64), base=_z(dev, b, dtype=I64), bad=_z(dev, b, dtype=I32),
                order=torch.arange(b, dtype=I32, device=dev), max_delay=1)


def _image(dev):
    return dict(occupancy=_z(dev, SIDE, SIDE, dtype=U8), count=K, b0=0.0, b2=0.0, resolution=1.0, robot_radius=0.25, margin=0.0)


def _spacetime_reserve(dev, m=B):
    """m None: no tracks"""
    a = dict(_image(dev), reservation=_z(dev, reservation_words(), dtype=I64))
    if m is None:
        return dict(a, tracks=None, radius=None, visible=None)
    return dict(a, tracks=_f(dev, m, K, 2), radius=_f(dev, m, seed=2, lo=0.1, hi=0.6), visible=torch.ones(m, dtype=U8, device=dev))


def _spacetime_plan_fleet(dev, r=B):
    return dict(_image(dev), start_cells=_i(dev, [[0, 0], [3, 3]][:r], 2), goal_cells=_i(dev, [[3, 3], [0, 0]][:r], 2),
                order=torch.arange(r, dtype=I32, device=dev), reservation=_z(dev, reservation_words(), dtype=I64))


def _lattice_fields(dev, g=2):
    return dict(layers=_z(dev, 1, SIDE, SIDE, dtype=U8), goal_states=_i(dev, [[3, 3, 0], [0, 0, -1]][:g], 3), turn_cost=1)


def _lattice_gear_fields(dev, g=2):
    return dict(_lattice_fields(dev, g), reverse_cost=1, cusp_cost=1)


def _lattice_trace_paths(dev, b=B, g=2, gears=False):
    shape = (g, 2, 8, SIDE, SIDE, 2) if gears else (g, 8, SIDE, SIDE, 2)
    a = dict(fields=_z(dev, *shape, dtype=I32), field_first=0, n_total=2, start_states=_i(dev, [[0, 0, 0], [1, 1, 2]][:b], 3),
             goal_states=_i(dev, [[3, 3, 0], [0, 0, -1]][:b], 3), field_index=_i(dev, [0, 1][:b]), turn_cost=1)
    if gears:
        a.update(reverse_cost=1, cusp_cost=1)
    return dict(a, max_len=4)


def _lattice_gear_trace_paths(dev, b=B, g=2):
    return _lattice_trace_paths(dev, b, g, True)


def _lattice_seed_trajectories(dev, b=B):
    return dict(cells=_z(dev, b, 4, 2, dtype=I32), headings=_z(dev, b, 4, dtype=I32), count=_z(dev, b, dtype=I32),
                status=_z(dev, b, dtype=I32), start=_f(dev, b, 3, seed=1), goal=_f(dev, b, 3, seed=2), n_waypoints=N, origin_x=0.0,
                origin_y=0.0, resolution=1.0)


BASE = dict(onf_fwd_bwd_input=_onf_points, onf_logits=_onf_points, traj_step=_traj_step, traj_steps=_traj_steps,
            reparametrize=_reparametrize, update_endpoints=_update_endpoints, onf_train_grad=_onf_train_grad, adam_step=_adam_step,
            onf_train_step=_onf_train_step, grid_search_init=_grid_search_init, path_time_profile=_path_time_profile,
            path_time_sample=_path_time_sample, track_conflicts=_track_conflicts, track_headings=_track_headings,
            box_track_conflicts=_box_track_conflicts, fleet_shift_masks=_fleet_shift_masks, fleet_assign_delays=_fleet_assign_delays,
            spacetime_reserve=_spacetime_reserve, spacetime_plan_fleet=_spacetime_plan_fleet, lattice_fields=_lattice_fields,
            lattice_trace_paths=_lattice_trace_paths, lattice_gear_fields=_lattice_gear_fields,
            lattice_gear_trace_paths=_lattice_gear_trace_paths, lattice_seed_trajectories=_lattice_seed_trajectories)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _grow(x):
    """one more row"""
    return torch.cat([x, x[:1]])


def _wider(x):
    """one more entry in the last dimension"""
    return torch.cat([x, x[..., :1]], -1).contiguous()


def _narrower(x):
    return x[..., :-1].contiguous()


def _strided(x):
    """the same shape and values, not contiguous"""
    return torch.stack([x, x], -1)[..., 0]


def _set(**kw):
    return lambda a: a.update(kw)


def _on(name, f):
    return lambda a: a.update({name: f(a[name])})


def _empty_like_rows(x, *shape):
    return torch.empty(shape, dtype=x.dtype, device=x.device)


# what every op that states a batch through batch_endpoints refuses
_ENDPOINT_CASES = [("traj_not_3d", _on("traj", lambda x: x[0].contiguous())), ("traj_4_wide", _on("traj", _wider)),
                   ("start_flat", _on("start", lambda x: x.reshape(-1))), ("goal_rows", _on("goal", _grow))]
# ... and through batch_state, for an SE(2) batch
_STATE_CASES = _ENDPOINT_CASES + [("one_waypoint", _on("traj", lambda x: x[:, :1].contiguous())), ("lam_absent", _set(lam=None)),
                                  ("cm_absent", _set(cm=None)), ("lam_shape", _on("lam", _narrower)), ("cm_shape", _on("cm", _wider))]
# ... and what traj_step and traj_steps add
_STEP_CASES = _STATE_CASES + [
    ("params_count", _on("params", lambda x: x[:-1])), ("bad_config", _set(sigma=0.0)),
    ("active_shape", _on("active", _grow)), ("live_ws_absent", _set(live_ws=None)), ("live_ws_short", _on("live_ws", lambda x: x[:-1])),
    ("live_ws_without_mask", _set(active=None)),
    ("onf_of_another_dim", lambda a: a.update(angle_dim=0, params=_params(a["traj"].device, 2))),
    ("adam_m_shape", _on("adam_m", _grow)), ("adam_v_shape", _on("adam_v", _wider)), ("t_shape", _on("t", _wider)),
    ("onf_out_shape", _on("onf_out", _narrower)), ("band_of_another_width", _set(half_width=HW + 1)),
    ("terms_shape", _on("terms", _narrower)), ("hyper_short", _set(hyper=[0.0] * 5))]
_LATTICE_COSTS = [("turn_cost_256", _set(turn_cost=256)), ("turn_cost_negative", _set(turn_cost=-1))]
_GEAR_COSTS = _LATTICE_COSTS + [("reverse_cost_256", _set(reverse_cost=256)), ("cusp_cost_negative", _set(cusp_cost=-1))]
_FIELD_CASES = [("layers_2d", _on("layers", lambda x: x[0])), ("goal_states_2_wide", _on("goal_states", _narrower)),
                ("empty_grid", _on("layers", lambda x: x[:, :0])), ("c_two_layers", _on("layers", _grow))]
_TRACE_CASES = [("start_states_2_wide", _on("start_states", _narrower)), ("goal_states_rows", _on("goal_states", _grow)),
                ("field_index_rows", _on("field_index", _grow)), ("max_len_negative", _set(max_len=-1)), ("max_len_2_31", _set(max_len=2 ** 31)),
                ("c_field_range", _set(field_first=1))]
_IMAGE_CASES = [("occupancy_3d", _on("occupancy", lambda x: x[None])), ("occupancy_empty", _on("occupancy", lambda x: x[:0])),
                ("count_0", _set(count=0)), ("count_beyond_an_index", _set(count=2 ** 31 - 1)),
                ("image_beyond_an_index", _on("occupancy", lambda x: _empty_like_rows(x, 2 ** 31, 1))),
                ("reservation_words", _on("reservation", _grow)), ("c_resolution_0", _set(resolution=0.0))]
_TWO_SET_CASES = [("tracks_a_2d", _on("tracks_a", lambda x: x[0])), ("tracks_a_no_instants", _on("tracks_a", lambda x: x[:, :0])),
                  ("tracks_a_2_31_instants", _on("tracks_a", lambda x: _empty_like_rows(x, 0, 2 ** 31, x.shape[2]))),
                  ("tracks_b_2d", _on("tracks_b", lambda x: x[0])), ("tracks_b_other_k", _on("tracks_b", lambda x: torch.cat([x, x[:, :1]], 1))),
                  ("radius_a_rows", _on("radius_a", _grow)), ("radius_b_rows", _on("radius_b", _grow)), ("c_dt_0", _set(dt=0.0)),
                  ("c_margin_inf", _set(margin=float("inf")))]


def _explicit():
    """(op, name, change) of every refusal that is written out"""
    out = []

    def add(op, cases):
        out.extend((op, name, change) for name, change in cases)

    for op in ("onf_fwd_bwd_input", "onf_logits"):
        add(op, [("params_count", _on("params", lambda x: x[:-1])), ("bad_config", _set(sigma=0.0)), ("points_2_wide", _on("points", _narrower)),
                 ("points_1d", _on("points", lambda x: x.reshape(-1))), ("points_on_cpu", _on("points", lambda x: x.cpu()))])
    add("traj_step", _STEP_CASES + [("c_t_mode_2", _set(t_mode=2))])
    add("traj_steps", _STEP_CASES + [("u_shape", _on("u", _grow)), ("reparam_freq_0", _set(reparam_freq=0)), ("n_steps_negative", _set(n_steps=-1)),
                                     ("t_steps_of_another_count", _on("t_steps", _grow))])
    add("reparametrize", _STATE_CASES + [("u_shape", _on("u", _grow)), ("active_shape", _on("active", _grow))])
    add("update_endpoints", _STATE_CASES + [("u_shape", _on("u", _grow)), ("moved_shape", _on("moved", _grow)), ("which_2", _set(which=2)),
                                            ("points_rows", _on("points", _grow)), ("min_index_rows", _on("min_index", _grow))])
    add("grid_search_init", _ENDPOINT_CASES + [
        ("occupancy_3d", _on("occupancy", lambda x: x[None])), ("start_cells_rows", _on("start_cells", _grow)),
        ("goal_cells_rows", _on("goal_cells", _grow)), ("field_index_rows", _on("field_index", _grow)),
        ("unique_goal_cells_3_wide", _on("unique_goal_cells", _wider)), ("c_resolution_0", _set(resolution=0.0))])
    add("onf_train_grad", [("params_count", _on("params", lambda x: x[:-1])), ("bad_config", _set(sigma=0.0)),
                           ("samples_2_wide", _on("samples", _narrower)), ("labels_rows", _on("labels", _grow))])
    add("adam_step", [("grad_short", _on("grad", lambda x: x[:-1])), ("m_rows", _on("m", _grow)), ("v_rows", _on("v", _grow))])
    add("onf_train_step", [("samples_empty", _on("samples", lambda x: x[:0])), ("samples_1d", _on("samples", lambda x: x.reshape(-1))),
                           ("params_count", _on("params", lambda x: x[:-1])), ("labels_rows", _on("labels", _grow)), ("m_rows", _on("m", _grow))])
    add("path_time_profile", _ENDPOINT_CASES + [("limits_short", _set(limits=LIMITS[:5])), ("v_start_rows", _on("v_start", _grow)),
                                                ("v_goal_rows", _on("v_goal", _grow)), ("c_v_max_0", _set(limits=[0.0] + LIMITS[1:]))])
    add("path_time_sample", _ENDPOINT_CASES + [("limits_short", _set(limits=LIMITS[:5])), ("profile_3_slots", _on("profile", _narrower)),
                                               ("gear_shape", _on("gear", _wider)), ("count_negative", _set(count=-1)),
                                               ("count_2_31", _set(count=2 ** 31)), ("c_dt_0", _set(dt=0.0))])
    add("track_conflicts", _TWO_SET_CASES + [("tracks_a_1_wide", _on("tracks_a", lambda x: x[..., :1].contiguous()))])
    add("track_headings", [("tracks_2d", _on("tracks", lambda x: x[0])), ("tracks_2_wide", _on("tracks", _narrower))])
    add("box_track_conflicts", _TWO_SET_CASES + [
        ("box_b_absent", _set(box_b=None)), ("box_b_rows", _on("box_b", _grow)), ("box_a_5_wide", _on("box_a", _wider)),
        ("tracks_a_2_wide", _on("tracks_a", _narrower)), ("tracks_b_2_wide", _on("tracks_b", _narrower)), ("refine_9", _set(refine=9)),
        ("refine_negative", _set(refine=-1)), ("c_margin_nan", _set(margin=float("nan")))])
    add("fleet_shift_masks", [("tracks_2d", _on("tracks", lambda x: x[0])), ("max_delay_64", _set(max_delay=64)),
                              ("max_delay_negative", _set(max_delay=-1)), ("radius_rows", _on("radius", _grow)),
                              ("obstacles_2d", _on("obstacles", lambda x: x[0])), ("obstacles_of_k_instants", _on("obstacles", lambda x: x[:, :K].contiguous())),
                              ("obstacle_radius_rows", _on("obstacle_radius", _grow)), ("c_margin_inf", _set(margin=float("inf")))])
    add("fleet_assign_delays", [("pair_3_words", _on("pair", _wider)), ("pair_not_square", _on("pair", _grow)), ("max_delay_64", _set(max_delay=64)),
                                ("base_rows", _on("base", _grow)), ("bad_rows", _on("bad", _grow)), ("order_rows", _on("order", _grow))])
    add("spacetime_reserve", _IMAGE_CASES + [
        ("radius_without_tracks", _set(tracks=None, visible=None)), ("visible_without_tracks", _set(tracks=None, radius=None)),
        ("tracks_2d", _on("tracks", lambda x: x[0])), ("tracks_of_another_count", _on("tracks", lambda x: torch.cat([x, x[:, :1]], 1))),
        ("radius_rows", _on("radius", _grow)), ("visible_rows", _on("visible", _grow)), ("c_margin_inf", _set(margin=float("inf")))])
    add("spacetime_plan_fleet", _IMAGE_CASES + [("start_cells_3_wide", _on("start_cells", _wider)), ("goal_cells_rows", _on("goal_cells", _grow)),
                                                ("order_rows", _on("order", _grow))])
    add("lattice_fields", _FIELD_CASES + _LATTICE_COSTS)
    add("lattice_gear_fields", _FIELD_CASES + _GEAR_COSTS)
    add("lattice_trace_paths", _TRACE_CASES + _LATTICE_COSTS + [("fields_7_headings", _on("fields", lambda x: x[:, :7].contiguous())),
                                                                ("fields_of_an_empty_grid", _on("fields", lambda x: x[:, :, :0]))])
    add("lattice_gear_trace_paths", _TRACE_CASES + _GEAR_COSTS + [("fields_1_gear", _on("fields", lambda x: x[:, :1].contiguous())),
                                                                  ("fields_of_an_empty_grid", _on("fields", lambda x: x[:, :, :, :0]))])
    add("lattice_seed_trajectories", [("cells_3_wide", _on("cells", _wider)), ("headings_shape", _on("headings", _wider)), ("count_rows", _on("count", _grow)),
                                      ("status_rows", _on("status", _grow)), ("start_2_wide", _on("start", _narrower)), ("goal_rows", _on("goal", _grow)),
                                      ("n_waypoints_0", _set(n_waypoints=0)), ("n_waypoints_2_31", _set(n_waypoints=2 ** 31)),
                                      ("resolution_0", _set(resolution=0.0))])
    # a 2-D batch beside multiplier tensors, in each of the four ops that state one through batch_state
    for op in ("traj_step", "traj_steps", "reparametrize", "update_endpoints"):
        out.append((op, "lam_beside_2d", ("2d", lambda a: a.update(lam=_z(a["traj"].device, B, N + 1)))))
    return out


def _tensor_args(op):
    return [k for k, v in BASE[op]("cpu").items() if isinstance(v, torch.Tensor)]


def _cases():
    cases = []
    for op, name, change in _explicit():
        d = 3
        if isinstance(change, tuple):
            d, change = 2, change[1]
        cases.append(("%s/%s" % (op, name), op, d, change))
    for op in BASE:
        for arg in _tensor_args(op):
            cases.append(("%s/dtype_%s" % (op, arg), op, 3, _on(arg, lambda x: x.to(_OTHER_DTYPE[x.dtype]))))
            cases.append(("%s/strided_%s" % (op, arg), op, 3, _on(arg, _strided)))
    assert len({c[0] for c in cases}) == len(cases)
    return cases


CASES = _cases()        # (id, op, point dimension of the base call, change)
# second device only: (id, op, argument moved there)
DEVICE_CASES = [("%s/device_%s" % (op, arg), op, arg) for op in BASE if len(_tensor_args(op)) >= 2 for arg in _tensor_args(op)]


def base_args(op, dev, d=3):
    return BASE[op](dev, d) if d == 2 else BASE[op](dev)


def refusal(ops, op, args):
    """first line of the RuntimeError of the call, None when it is accepted"""
    try:
        getattr(ops, op)(**args)
    except RuntimeError as e:
        return str(e).splitlines()[0]
    return None


def run_case(ops, case, dev):
    _, op, d, change = case
    args = base_args(op, dev, d)
    change(args)
    return refusal(ops, op, args)


def run_device_case(ops, case, dev, other):
    _, op, arg = case
    args = base_args(op, dev)
    args[arg] = args[arg].to(other)
    return refusal(ops, op, args)


# ---- accepted edges ------------------------------------------------------------------------------------------------------------
def _edge_table():
    """name -> (op, device -> its arguments, the arguments it updates in place)"""
    e = {}

    def edge(name, op, make, also=()):
        e[name] = (op, make, tuple(also))

    two_sets = (("a0_b2", dict(ba=0, bb=2)), ("a2_b0", dict(ba=2, bb=0)), ("self_a0", dict(ba=0, bb=None)), ("k1", dict(k=1)),
                ("self_k1", dict(bb=None, k=1)))
    for tag, kw in two_sets:
        edge("track_conflicts/" + tag, "track_conflicts", lambda dev, kw=kw: _track_conflicts(dev, **kw))
        edge("box_track_conflicts/" + tag, "box_track_conflicts", lambda dev, kw=kw: _box_track_conflicts(dev, **kw))
    edge("track_headings/b0", "track_headings", lambda dev: dict(tracks=_z(dev, 0, K, 3)))
    edge("fleet_shift_masks/b0", "fleet_shift_masks", lambda dev: _fleet_shift_masks(dev, b=0, m=None))
    edge("fleet_shift_masks/m0", "fleet_shift_masks", lambda dev: _fleet_shift_masks(dev, m=0))
    edge("fleet_shift_masks/no_obstacles", "fleet_shift_masks", lambda dev: _fleet_shift_masks(dev, m=None))
    edge("fleet_assign_delays/b0", "fleet_assign_delays", lambda dev: _fleet_assign_delays(dev, b=0))
    edge("path_time_sample/count0", "path_time_sample", lambda dev: _path_time_sample(dev, count=0))
    edge("spacetime_reserve/fresh", "spacetime_reserve", lambda dev: dict(_spacetime_reserve(dev, m=None), reservation=None))
    edge("spacetime_reserve/no_tracks", "spacetime_reserve", lambda dev: _spacetime_reserve(dev, m=None))
    edge("spacetime_reserve/m0", "spacetime_reserve", lambda dev: dict(_spacetime_reserve(dev, m=0), reservation=None))
    edge("spacetime_plan_fleet/r0", "spacetime_plan_fleet", lambda dev: _spacetime_plan_fleet(dev, r=0), ["reservation"])
    edge("lattice_fields/g0", "lattice_fields", lambda dev: _lattice_fields(dev, g=0))
    edge("lattice_gear_fields/g0", "lattice_gear_fields", lambda dev: _lattice_gear_fields(dev, g=0))
    for op, make in (("lattice_trace_paths", _lattice_trace_paths), ("lattice_gear_trace_paths", _lattice_gear_trace_paths)):
        # no field in this call: the problems' fields (0 and 1 of n_total = 2) belong to another chunk, and they stay untouched
        edge(op + "/g0", op, lambda dev, make=make: dict(make(dev, g=0), field_first=2))
        edge(op + "/b0", op, lambda dev, make=make: make(dev, b=0))
    edge("lattice_seed_trajectories/b0", "lattice_seed_trajectories", lambda dev: _lattice_seed_trajectories(dev, b=0))
    edge("grid_search_init/b0", "grid_search_init", lambda dev: _grid_search_init(dev, b=0), ["traj"])
    edge("grid_search_init/b0_g0", "grid_search_init", lambda dev: _grid_search_init(dev, b=0, g=0), ["traj"])
    for d in (3, 2):
        edge("onf_logits/one_point_%dd" % d, "onf_logits", lambda dev, d=d: _onf_points(dev, d, p=1))
        edge("onf_fwd_bwd_input/one_point_%dd" % d, "onf_fwd_bwd_input", lambda dev, d=d: _onf_points(dev, d, p=1))
    return e


EDGES = _edge_table()


def run_edge(ops, name, dev):
    """-> [(the bytes, shape, stride, dtype name)] of every output of the edge, then of what it updates in place"""
    op, make, also = EDGES[name]
    args = make(dev)
    out = getattr(ops, op)(**args)
    out = [out] if isinstance(out, torch.Tensor) else list(out)
    out += [args[k] for k in also]
    torch.cuda.synchronize()
    res = []
    for t in out:
        dense = t.contiguous().cpu().numpy()
        res.append((np.frombuffer(dense.tobytes(), np.uint8), tuple(t.shape), tuple(t.stride()), str(t.dtype)))
    return res
