"""GPU: vehicle-model variants of the step kernel against the reference's AUVSim.step transitions (fixture G3,
tests/golden/g3_auv_step.npz): BlueROV2 joystick (diagonal B), BlueROV2 "direct" (dense 6x8 B), BlueROV2 with the
reference's test XML (other added mass), LAUV, at several step sizes; plus a mixed BlueROV2/LAUV batch that must equal
the two homogeneous batches env for env (divergent-branch path).  The *_asym vehicles (tests/golden/*_asym_params.xml:
x_G, y_G, x_B, y_B, I_xy, I_yz != 0) are outside the structural form, so dockauv_create gives them the general kinetics
expressions (SYM = false); tests/test_oracle_golden.py shows that their expected transitions are >= 100 x the float32
bound away from the symmetric vehicle's, so a pass here is a pass of the general path."""
import copy
import os

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu


def rot_zyx(phi, theta, psi):
    cf, sf, ct, st, cp, sp = np.cos(phi), np.sin(phi), np.cos(theta), np.sin(theta), np.cos(psi), np.sin(psi)
    return np.array([[cp * ct, -sp * cf + cp * st * sf, sp * sf + cp * cf * st],
                     [sp * ct, cp * cf + sf * st * sp, -cp * sf + st * sp * cf],
                     [-st, ct * sf, ct * cf]])


def current_for_body_velocity(att, nu_c):
    """(V_c, V_min, V_max, alpha, beta) whose body-frame current at attitude `att` is nu_c[0:3]."""
    out = np.zeros((att.shape[0], 5))
    for i in range(att.shape[0]):
        v_ned = rot_zyx(*att[i]) @ nu_c[i, 0:3]
        V = np.linalg.norm(v_ned)
        if V == 0:
            continue
        d = v_ned / V
        if d[0] < 0 and abs(d[2]) < 1e-300 and False:
            pass
        # d = (cos a cos b, sin b, sin a cos b) with cos b > 0
        b = np.arcsin(np.clip(d[1], -1, 1))
        a = np.arctan2(d[2], d[0])
        out[i] = [V, V, V, a, b]
    return out


def models():
    from gym_dockauv_amd.objects.vehicle_models import BlueROV2, LAUV
    golden = os.path.join(os.path.dirname(__file__), "golden")
    test_xml = os.path.join(golden, "bluerov2_test_params.xml")
    b_asym, l_asym = os.path.join(golden, "bluerov2_asym_params.xml"), os.path.join(golden, "lauv_asym_params.xml")
    return {"bluerov2": BlueROV2, "bluerov2_direct": lambda: BlueROV2(control_mode="direct"),
            "bluerov2_testxml": lambda: BlueROV2(test_xml), "lauv": LAUV,
            "bluerov2_asym": lambda: BlueROV2(b_asym), "bluerov2_direct_asym": lambda: BlueROV2(b_asym, control_mode="direct"),
            "lauv_asym": lambda: LAUV(l_asym)}


CASES = [("bluerov2", h) for h in (0.1, 0.05, 0.01)] + [("bluerov2_direct", h) for h in (0.1, 0.01)] + \
        [("bluerov2_testxml", 0.05)] + [("lauv", h) for h in (0.02, 0.01)] + \
        [("bluerov2_asym", h) for h in (0.1, 0.05, 0.01)] + [("bluerov2_direct_asym", h) for h in (0.1, 0.01)] + \
        [("lauv_asym", h) for h in (0.02, 0.01)]
# these also run with a ray fan (ObstaclesDocking3d: the ray-fan full instantiation); the ray stage does not feed the state,
# so the expected transition is the same
WITH_RAYS = ("bluerov2_direct", "bluerov2_asym", "bluerov2_direct_asym", "lauv_asym")


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name,h", CASES)
def test_auv_step_transitions(name, h, precision):
    from gym_dockauv_amd import _capi
    from gym_dockauv_amd.config.env_config import BASE_CONFIG
    from gym_dockauv_amd.envs.batched import BatchedDocking3d
    g = H.load("g3_auv_step")
    tag = f"{name}_h{h}"
    st, up, act, nuc = g[tag + "_state"], g[tag + "_u_prev"], g[tag + "_action"], g[tag + "_nu_c"]
    K, n_u = act.shape
    cfg = copy.deepcopy(BASE_CONFIG)
    cfg["t_step_size"] = h
    for scenario in ("SimpleDocking3d",) + (("ObstaclesDocking3d",) if name in WITH_RAYS else ()):
        model = models()[name]()
        env = BatchedDocking3d(cfg, num_envs=K, scenario=scenario, precision=precision, reset_mode="none",
                               vehicle_models=[model], current_mu=0.0, rng="batched")
        try:
            assert env.n_u == n_u
            if scenario != "SimpleDocking3d":      # the obstacle field of a reset; pose, goal and current are set below
                env._gen = np.random.default_rng(3)
                env.reset()
            env.set_field(_capi.F_STATE, st)
            u8 = np.zeros((K, 8))
            u8[:, :n_u] = up
            env.set_field(_capi.F_U, u8)
            env.set_field(_capi.F_CURRENT, current_for_body_velocity(st[:, 3:6], nuc))
            goal = np.zeros((K, 4))
            goal[:, 0] = 1000.0      # far away: nothing terminates
            env.set_field(_capi.F_GOAL, goal)
            env.step(act)
            new = env.state
            tol = 1e-9 if precision == "f64" else 3e-5
            lin = [0, 1, 2, 6, 7, 8, 9, 10, 11]
            ref = g[tag + "_new_state"]
            scale = np.maximum(1.0, np.abs(ref[:, lin]))
            e_lin = (np.abs(new[:, lin] - ref[:, lin]) / scale).max()
            d = np.abs(new[:, 3:6] - ref[:, 3:6])
            e_ang = np.minimum(d, 2 * np.pi - d).max()
            e_u = np.abs(env.u - g[tag + "_new_u"]).max()
            print(f"[auv_step {precision}] {tag} {scenario}: state {max(e_lin, e_ang):.3e} u {e_u:.3e}")
            assert e_lin <= tol, (scenario, e_lin)
            assert e_ang <= tol, (scenario, e_ang)
            np.testing.assert_allclose(env.u, g[tag + "_new_u"], rtol=0, atol=tol * 15)
        finally:
            env.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_general_path_equals_structural_fast_path(precision):
    """The SYM fast path of kinetics_ drops terms that multiply exact zeros; forcing the general expressions
    (envs_per_group = -1 test hook) must give the same trajectory to rounding."""
    from gym_dockauv_amd.envs.batched import BatchedDocking3d
    outs = []
    for force_general in (False, True):
        env = BatchedDocking3d(num_envs=200, scenario="ObstaclesCurrentDocking3d", precision=precision,
                               reset_mode="none", rng="batched")
        if force_general:
            env.close()
            env = BatchedDocking3d.__new__(BatchedDocking3d)
            BatchedDocking3d.__init__(env, num_envs=200, scenario="ObstaclesCurrentDocking3d", precision=precision,
                                      reset_mode="none", rng="batched", _force_general=True)
        env._gen = np.random.default_rng(5)
        env.reset()
        rs = np.random.RandomState(2)
        traj = []
        for t in range(10):
            o, r, d, _ = env.step(rs.uniform(-1, 1, (200, 6)))
            traj.append((o.copy(), r.copy()))
        outs.append(traj)
        env.close()
    tol = 1e-12 if precision == "f64" else 2e-5
    for (o1, r1), (o2, r2) in zip(*outs):
        assert np.abs(o1 - o2).max() <= tol and np.abs(r1 - r2).max() <= tol * 10


def _mixed_equals_homogeneous(precision, mixed_models=None, blue_models=None, lauv_models=None):
    """an interleaved BlueROV2 / LAUV batch against the two homogeneous batches, env for env; the *_models arguments replace the
    shipped vehicles (mixed: [BlueROV2 model, LAUV model])"""
    from gym_dockauv_amd import _capi
    from gym_dockauv_amd.config.env_config import BASE_CONFIG
    from gym_dockauv_amd.envs.batched import BatchedDocking3d
    cfg = copy.deepcopy(BASE_CONFIG)
    cfg["t_step_size"] = 0.02
    N = 150
    kinds = ["BlueROV2" if i % 2 == 0 else "LAUV" for i in range(N)]
    mixed = BatchedDocking3d(cfg, num_envs=N, scenario="ObstaclesCurrentDocking3d", precision=precision,
                             reset_mode="none", rng="batched", vehicles=kinds, vehicle_models=mixed_models)
    cfg_b, cfg_l = copy.deepcopy(cfg), copy.deepcopy(cfg)
    cfg_l["vehicle"] = "LAUV"
    blue = BatchedDocking3d(cfg_b, num_envs=N, scenario="ObstaclesCurrentDocking3d", precision=precision,
                            reset_mode="none", rng="batched", vehicle_models=blue_models)
    lauv = BatchedDocking3d(cfg_l, num_envs=N, scenario="ObstaclesCurrentDocking3d", precision=precision,
                            reset_mode="none", rng="batched", vehicle_models=lauv_models)
    try:
        mixed._gen = np.random.default_rng(11)
        mixed.reset()
        for f in (_capi.F_STATE, _capi.F_GOAL, _capi.F_CURRENT, _capi.F_CAPSULES):
            blue.set_field(f, mixed.get_field(f))
            lauv.set_field(f, mixed.get_field(f))
        rs = np.random.RandomState(4)
        is_b = np.array([k == "BlueROV2" for k in kinds])
        worst = [0.0, 0.0]
        for t in range(12):
            a = rs.uniform(-1, 1, (N, 6))
            om, rm, dm, _ = mixed.step(a)
            ob, rb, db, _ = blue.step(a)
            ol, rl, dl, _ = lauv.step(a[:, :3])
            # an action-penalty subtlety: the mixed batch has n_u_max = 6 columns but a LAUV env only reads 3
            tol = 1e-12 if precision == "f64" else 5e-6   # different instantiations round differently
            worst[0] = max(worst[0], np.abs(om[is_b] - ob[is_b]).max(), np.abs(om[~is_b] - ol[~is_b]).max())
            worst[1] = max(worst[1], np.abs(rm[is_b] - rb[is_b]).max(), np.abs(rm[~is_b] - rl[~is_b]).max())
            assert np.abs(om[is_b] - ob[is_b]).max() <= tol and np.abs(rm[is_b] - rb[is_b]).max() <= tol * 10
            assert np.abs(om[~is_b] - ol[~is_b]).max() <= tol and np.abs(rm[~is_b] - rl[~is_b]).max() <= tol * 10
            assert np.array_equal(dm[is_b], db[is_b]) and np.array_equal(dm[~is_b], dl[~is_b])
        print(f"[mixed {precision}] max |obs - homogeneous| {worst[0]:.3e}, reward {worst[1]:.3e}")
    finally:
        mixed.close(); blue.close(); lauv.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_mixed_batch_equals_homogeneous_batches(precision):
    _mixed_equals_homogeneous(precision)


@pytest.mark.parametrize("asymmetric", ["both", "lauv_only"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_mixed_asymmetric_batch_equals_homogeneous_batches(precision, asymmetric):
    """The mixed kernel with the general kinetics expressions (the structural fast path needs EVERY vehicle of the handle in
    the structural form).  "both": asymmetric BlueROV2 + asymmetric LAUV against the two homogeneous asymmetric batches, which
    test_auv_step_transitions ties to the reference.  "lauv_only": the shipped BlueROV2 beside the asymmetric LAUV -- its envs
    then run the general expressions on a symmetric vehicle and must equal the homogeneous batch on the structural path."""
    m = models()
    if asymmetric == "both":
        _mixed_equals_homogeneous(precision, [m["bluerov2_asym"](), m["lauv_asym"]()], [m["bluerov2_asym"]()], [m["lauv_asym"]()])
    else:
        _mixed_equals_homogeneous(precision, [m["bluerov2"](), m["lauv_asym"]()], None, [m["lauv_asym"]()])


@pytest.mark.parametrize("name", ["bluerov2_asym", "bluerov2_direct"])
def test_step_sequence_of_a_vehicle_without_resident_kernel(name):
    """The resident step-sequence kernels exist for the structural fast path with diagonal or LAUV inputs only; for an
    asymmetric vehicle (and for the dense input matrix) dockauv_step_sequence with the resident option ON must quietly take
    the single launches: no error, and the same bytes as n x dockauv_step."""
    import torch
    from gym_dockauv_amd.envs.batched import BatchedDocking3d
    N, K = 130, 6
    dev = torch.device("cuda", 0)
    outs = []
    for sequence in (False, True):
        env = BatchedDocking3d(num_envs=N, scenario="ObstaclesCurrentDocking3d", precision="f32", reset_mode="device",
                               device_seed=7, rng="batched", vehicle_models=[models()[name]()])
        try:
            env._gen = np.random.default_rng(3)
            env.reset()
            g = torch.Generator(device=dev)
            g.manual_seed(5)
            acts = torch.rand((K, N, env.n_u), device=dev, generator=g) * 2 - 1
            out = torch.zeros((K, N, env.packed_row_words(True)), device=dev, dtype=torch.float32)
            stream = torch.cuda.current_stream().cuda_stream
            if sequence:
                env.set_sequence_resident(True)
                ios = env.make_step_sequence([acts[k].data_ptr() for k in range(K)], [out[k].data_ptr() for k in range(K)])
                env.run_step_sequence(ios, stream=stream)
            else:
                for k in range(K):
                    env.step_device(acts[k].data_ptr(), out[k].data_ptr(), stream=stream, packed=True)
            torch.cuda.synchronize()
            env.synchronize()
            outs.append((out.cpu().numpy().view(np.uint32), env.state.copy()))
        finally:
            env.close()
    assert outs[0][0].any()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
