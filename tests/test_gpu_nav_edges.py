"""GPU: the stage behind the rays -- navigation errors (hardware sqrt / rcp, the minimax atan2_, the ssa_ select), the five done
conditions, the sixteen leading observation entries with their clips, the thirteen reward terms, the two-float heading wrap --
against the oracle on the constructed states of tests/nav_scenes.py: sensor-free and ray kernels, groups of every size, lean
and general kernels (one non-zero current row switches), the sphere-only twin, LAUV and the mixed pair, the full-output, product
and TERM paths, reward set 2 on the full kernels, and for the heading wrap the resident step sequence against single launches.
One step through the C ABI with reset_mode "none" and set_field as in tests/test_gpu_ray_edges.py; every row asserts
threads_in_use, step_uses_current and step_uses_capsules, so that it cannot silently run another kernel.

Bounds (nav_scenes.check_f64 / check_f32).  float64: condition bits and done equal the oracle in EVERY case, the entries the
reference clips are exactly that value, observations, navigation errors, state and all 13 reward terms within helpers.TOL.
float32, on the float32-qualified cases: no bit flip, done equal, clipped entries exact, every other obs[:16] entry within
max(8 e_ref, TOL obs) -- obs[2] directly, sign included --, each reward term and the total within max(8 e_ref, rew_abs +
rew_rel |ref|), the heading within TOL state on the circle; e_ref = the reference's own movement between its evaluation on the
float64 inputs and on what a float32 handle holds, per yardstick group and output; 8 = the margin of DESIGN.md section 7C.  The
largest error / bound per class is printed (and appended to the file DOCKAUV_NAV_EDGES_REPORT names, if set).

Ties (test_one_decision_at_a_tie): goals placed so that the kernel's own squared distance is the threshold's or a neighbour of
it, attitudes within a few ulps of max_attitude (asserted, on both sides), the step counter one short of the limit; either side is accepted, what is
asserted is that every role took the same decision.  The product and TERM kernels serve reset modes "none" and "device" (a
handle in reset mode "pool" is served by the full kernel: dockauv_device.h, needs_full_kernel), so they run with the in-kernel
generator and the full kernels with the staged pool."""
import copy
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import nav_scenes as S

pytestmark = pytest.mark.gpu
assert S.TOL["f64"] == {k: H.TOL["f64"][k] for k in S.TOL["f64"]} and S.TOL["f32"] == {k: H.TOL["f32"][k] for k in S.TOL["f32"]}


def _report(line):
    print(line)
    path = os.environ.get("DOCKAUV_NAV_EDGES_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _config(vehicle, reward_set=1):
    from gym_dockauv_amd.config.env_config import BASE_CONFIG
    cfg = copy.deepcopy(BASE_CONFIG)
    cfg.update(S.OVERRIDES)
    cfg["reward_set"] = reward_set
    if vehicle != "mixed":
        cfg["vehicle"] = vehicle
    return cfg


def _make_env(sc, precision, threads, scenario, vehicle, reset_mode="none", reward_set=1):
    from gym_dockauv_amd.envs.batched import BatchedDocking3d
    N = sc["state"].shape[0]
    return BatchedDocking3d(_config(vehicle, reward_set), num_envs=N, scenario=scenario, precision=precision, reset_mode=reset_mode,
                            rng="batched", max_capsules=sc["max_capsules"], max_spheres=sc["max_spheres"], threads_per_group=threads,
                            vehicles=list(sc["vehicle"]) if vehicle == "mixed" else None)


def _load(env, sc, current_row=None, expect=None):
    from gym_dockauv_amd import _capi
    env.reset()
    env.set_field(_capi.F_STATE, sc["state"])
    env.set_field(_capi.F_U, sc["u"][:, :_capi.MAX_U])
    env.set_field(_capi.F_GOAL, sc["goal"])
    env.set_field(_capi.F_TSTEPS, sc["tsteps"][:, None].astype(float))
    cur = np.array(sc["current"])
    if current_row is not None:
        assert not cur[0].any()
        cur[0] = current_row
    if cur.any() or current_row is not None or sc["with_current"]:
        env.set_field(_capi.F_CURRENT, cur)
    if sc["max_capsules"]:
        env.set_field(_capi.F_CAPSULES, sc["capsules"])
    if sc["max_spheres"]:
        env.set_field(_capi.F_SPHERES, sc["spheres"])
    if expect is not None:
        got = (env.threads_in_use, env.step_uses_current, env.step_uses_capsules)
        assert got == expect, f"(threads, uses current, uses capsules) = {got}, the row is about {expect}"


def _device_steps(env, act, path, steps=1, resident=False, tobs_init=0.0):
    """`steps` packed steps with the same action: ([rows as float32 [N, n_obs + 2]] per step, terminal observations or None)"""
    import torch
    dev = torch.device("cuda", env.device)
    N, n = env.num_envs, env.n_observations
    rows = torch.zeros((steps, N, n + 2), device=dev, dtype=torch.float32)
    tobs = torch.full((N, n), tobs_init, device=dev, dtype=torch.float32) if path == "term" else None
    a = torch.as_tensor(np.ascontiguousarray(act), device=dev, dtype=torch.float64 if env.precision == "f64" else torch.float32).contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    if resident:
        env.set_sequence_resident(True)
        env.run_step_sequence(env.make_step_sequence([a.data_ptr()] * steps, [rows[k].data_ptr() for k in range(steps)], packed=True), stream=stream)
    else:
        for k in range(steps):
            env.step_device(a.data_ptr(), rows[k].data_ptr(), stream=stream, packed=True, terminal_obs_ptr=tobs.data_ptr() if tobs is not None else 0)
    torch.cuda.synchronize()
    env.synchronize()
    return rows.cpu().numpy(), None if tobs is None else tobs.cpu().numpy()


def _run(sc, precision, path, threads, scenario, vehicle="BlueROV2", expect=None, current_row=None, reward_set=1, steps=1, resident=False):
    """`steps` steps of the scene.  path: "full" (host pointers, every optional output), "product" (device pointers, packed
    rows), "term" (product with terminal observations).  Returns the first step's obs [N, 16], reward, done, state, u (and
    bits, nav, terms on the full path), rows (product paths: the packed rows of every step as bits), and state2 / obs2."""
    from gym_dockauv_amd import _capi
    env = _make_env(sc, precision, threads, scenario, vehicle, reward_set=reward_set)
    try:
        _load(env, sc, current_row, expect)
        act = sc["action"][:, :env.n_u]
        out = {}
        if path == "full":
            for k in range(steps):
                obs, rew, done, _ = env.step(act, extras=True)
                if k == 0:
                    out.update(obs=np.asarray(obs[:, :16], np.float64), reward=np.asarray(rew, np.float64), done=np.asarray(done, bool),
                               bits=env._cond.astype(int).copy(), nav=np.asarray(env.nav_errors[:, :3], np.float64).copy(),
                               terms=np.asarray(env.last_reward_arr, np.float64).copy(), state=env.state.copy(), u=env.get_field(_capi.F_U))
                else:
                    out.update(obs2=np.asarray(obs[:, :16], np.float64), state2=env.state.copy())
        else:
            n = env.n_observations
            if steps == 1:
                r, _ = _device_steps(env, act, path)
                out.update(state=env.state.copy(), u=env.get_field(_capi.F_U))
            else:       # the first step's state has to be read between the two
                assert steps == 2
                if resident:
                    r, _ = _device_steps(env, act, path, steps=2, resident=True)
                    out.update(state2=env.state.copy())
                else:
                    r0, _ = _device_steps(env, act, path)
                    out.update(state=env.state.copy(), u=env.get_field(_capi.F_U))
                    r1, _ = _device_steps(env, act, path)
                    out.update(state2=env.state.copy())
                    r = np.concatenate([r0, r1])
                out.update(obs2=np.asarray(r[1][:, :16], np.float64))
            out.update(obs=np.asarray(r[0][:, :16], np.float64), reward=r[0][:, n].astype(np.float64), done=r[0][:, n + 1] > 0.5,
                       rows=r.view(np.int32).copy())
    finally:
        env.close()
    return out


def _check(name, b, out, precision, packed=False):
    sc = b["scene"]
    if precision == "f64":
        worst = S.check_f64(name, b, out)
        _report(f"{name}: max |obs[:16] - ref| {worst:.3e} (bound {S.TOL['f64']['obs']:.0e}); bits, done and clipped entries equal")
    else:
        ratios = S.check_f32(name, b, out, rew_floor=2.0 ** -24 if packed else 0.0)
        _report(f"{name}: error / bound per class: " + "; ".join(f"{c} {ratios[c]:.3f}" for c in S.CLASSES if c in ratios))
    # an action outside [-1, 1] moves the vehicle like the clipped one (the penalty alone sees the raw one: term 7 above)
    raw = np.flatnonzero(sc["twin"] >= 0)
    assert np.array_equal(out["state"][raw], out["state"][sc["twin"][raw]]) and np.array_equal(out["u"][raw], out["u"][sc["twin"][raw]]), \
        f"{name}: a raw action and its clipped twin leave different states"


def _same_bits(name, a, b):
    diff = np.argwhere(a["rows"] != b["rows"])
    assert diff.size == 0, f"{name}: {len(diff)} words of the packed rows differ, first at (step, env, word) {tuple(diff[0])}"
    if "state" in a and "state" in b:
        assert np.array_equal(a["state"], b["state"]), f"{name}: states differ"


def _expect(precision, threads, scenario, vehicle="BlueROV2", reset_mode="none"):
    """(threads_in_use, step_uses_current, step_uses_capsules) of a handle whose current rows are zero unless its scenario draws
    one: the lean twins serve float32 BlueROV2 groups of 256 threads and LAUV ray groups of 512 (dockauv_device.h: nocur_shape);
    a handle in reset mode "pool" is served by the full kernel, which has no lean twin"""
    lean = (precision == "f32" and reset_mode != "pool" and "Current" not in scenario and
            ((vehicle == "BlueROV2" and threads == 256) or (vehicle == "LAUV" and threads == 512 and scenario != "SimpleDocking3d")))
    return (threads, not lean, True)


ONE_ROW = (0.0, 0.0, 0.0, 0.3, 0.0)     # a current row that is not all zeros (a direction: the speeds stay zero)


# ------------------------------------------------------------------------------------------------ sensor-free kernels
@pytest.mark.parametrize("precision,path,threads", [("f64", "full", 256), ("f32", "full", 256), ("f32", "product", 256), ("f32", "product", 128),
                                                    ("f32", "product", 64), ("f32", "term", 256)])
def test_sensor_free_without_current(precision, path, threads):
    b = S.bundle("BlueROV2", False, 0, 0)
    lean = precision == "f32" and threads == 256     # (dockauv_device.h: nocur_shape)
    out = _run(b["scene"], precision, path, threads, "SimpleDocking3d", expect=(threads, not lean, True))
    _check(f"Simple BlueROV2 {precision} {path} {threads}", b, out, precision, packed=path != "full")
    if path == "product" and lean:       # the lean twin against the general kernel, bit for bit
        general = _run(b["scene"], precision, path, threads, "SimpleDocking3d", expect=(threads, True, True), current_row=ONE_ROW)
        _same_bits("sensor-free lean twin vs general kernel", out, general)
    if path == "term":                   # the TERM twin against the plain product kernel
        _same_bits("sensor-free TERM vs plain", out, _run(b["scene"], precision, "product", threads, "SimpleDocking3d",
                                                             expect=(threads, not lean, True)))


@pytest.mark.parametrize("precision,path,threads", [("f64", "full", 256), ("f32", "full", 256), ("f32", "product", 256), ("f32", "product", 64),
                                                    ("f32", "term", 256)])
def test_sensor_free_with_current(precision, path, threads):
    """the general kernels: currents of 3 and 1.9 m/s along each body axis in obs[13:16]"""
    b = S.bundle("BlueROV2", True, 0, 0)
    out = _run(b["scene"], precision, path, threads, "SimpleCurrentDocking3d", expect=(threads, True, True))
    _check(f"SimpleCurrent BlueROV2 {precision} {path} {threads}", b, out, precision, packed=path != "full")
    if path == "term":
        _same_bits("sensor-free TERM vs plain, with current", out, _run(b["scene"], precision, "product", threads, "SimpleCurrentDocking3d",
                                                                           expect=(threads, True, True)))


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_reward_set_two_on_the_full_kernels(precision):
    b = S.bundle("BlueROV2", True, 0, 0, reward_set=2)
    out = _run(b["scene"], precision, "full", 256, "SimpleCurrentDocking3d", expect=(256, True, True), reward_set=2)
    _check(f"SimpleCurrent BlueROV2 reward set 2 {precision} full", b, out, precision)


# ------------------------------------------------------------------------------------------------ ray kernels, obstacles far away
@pytest.mark.parametrize("precision,path,threads", [("f64", "full", 256), ("f32", "full", 256), ("f32", "product", 512), ("f32", "product", 256),
                                                    ("f32", "product", 64), ("f32", "term", 512), ("f32", "term", 256), ("f64", "full", 64)])
def test_ray_kernels_capsule_scenario(precision, path, threads):
    """(with a collision beside an attitude violation, and beside goal and time limit, in the `several` class)"""
    b = S.bundle("BlueROV2", False, 1, 0)
    lean = precision == "f32" and threads == 256
    out = _run(b["scene"], precision, path, threads, "CapsuleDocking3d", expect=(threads, not lean, True))
    _check(f"Capsule BlueROV2 {precision} {path} {threads}", b, out, precision, packed=path != "full")
    if path == "product" and lean:
        general = _run(b["scene"], precision, path, threads, "CapsuleDocking3d", expect=(threads, True, True), current_row=ONE_ROW)
        _same_bits("ray kernel lean twin vs general kernel", out, general)
    if path == "term":
        _same_bits(f"ray kernel TERM vs plain {threads}", out, _run(b["scene"], precision, "product", threads, "CapsuleDocking3d",
                                                                   expect=(threads, not lean, True)))


def test_sphere_only_twin():
    b = S.bundle("BlueROV2", False, 0, 2)
    twin = _run(b["scene"], "f32", "product", 256, "SphereDocking3d", expect=(256, False, False))
    _check("Sphere BlueROV2 f32 product 256 sphere-only twin", b, twin, "f32", packed=True)
    general = _run(b["scene"], "f32", "product", 256, "SphereDocking3d", expect=(256, True, True), current_row=ONE_ROW)
    _same_bits("sphere-only twin vs general kernel", twin, general)
    _check("Sphere BlueROV2 f64 full 256", b, _run(b["scene"], "f64", "full", 256, "SphereDocking3d", expect=(256, True, True)), "f64")


# ------------------------------------------------------------------------------------------------ LAUV and the mixed pair
@pytest.mark.parametrize("vehicle,precision,path,threads", [("LAUV", "f32", "product", 512), ("LAUV", "f32", "product", 256), ("LAUV", "f32", "full", 256),
                                                            ("LAUV", "f64", "full", 256), ("mixed", "f32", "product", 256),
                                                            ("mixed", "f32", "product", 64), ("mixed", "f64", "full", 256)])
def test_other_vehicles(vehicle, precision, path, threads):
    if vehicle == "LAUV":
        b, scenario = S.bundle("LAUV", True, 1, 0), "CapsuleCurrentDocking3d"
    else:
        b, scenario = S.bundle("mixed", False, 0, 0), "SimpleDocking3d"
    out = _run(b["scene"], precision, path, threads, scenario, vehicle=vehicle, expect=(threads, True, True))
    _check(f"{scenario} {vehicle} {precision} {path} {threads}", b, out, precision, packed=path != "full")


# ------------------------------------------------------------------------------------------------ the heading wrap, two steps
INCREMENT_ULPS = 64


def _check_wrap_headings(name, b, out, precision):
    """The heading after each of the two steps, inside [-pi, pi) and -- float32 -- held far below TOL state: the two-float
    heading loses nothing when it is stored or wrapped, so what separates it from the reference is the error of the step's
    INCREMENT alone, bounded by INCREMENT_ULPS = 64 units of float32 roundoff (2^-24) relative to the turn made so far (the
    Fehlberg combination and T_zyx are a dozen float32 operations on terms of the size of the turn, weighted by tableau
    coefficients of up to 8) or by 8 x the reference's own movement.  A low word dropped at the wrap costs up to 3e-7 rad."""
    sc, ev, mv = b["scene"], b["ev64"], b["move"]["heading-wrap"]
    turn1 = S.circle(ev["state"][:, 5], sc["state"][:, 5])
    turn2 = turn1 + S.circle(ev["state2"][:, 5], ev["state"][:, 5])
    worst = []
    for key, turn, e_ref in (("state", turn1, mv["psi"]), ("state2", turn2, mv["psi2"])):
        psi = out[key][:, 5]
        assert (psi >= -np.pi).all() and (psi < np.pi).all(), f"{name}: heading outside [-pi, pi) ({key})"
        err = S.circle(psi, ev[key][:, 5])
        bound = np.full_like(err, S.TOL["f64"]["state"]) if precision == "f64" else np.maximum(8 * e_ref, INCREMENT_ULPS * 2.0 ** -24 * turn)
        k = int((err / bound).argmax())
        assert (err <= bound).all(), f"{name}: heading ({key}) off by {err[k]:.3e}, {err[k] / bound[k]:.2f} x its bound, at env {k} ({sc['sub'][k]})"
        worst.append(float((err / bound).max()))
    move = max(8 * float(mv["obs2"][8:10].max()), 2 * S.TOL[precision]["obs"])     # (two steps accumulate: twice the one-step tolerance)
    oerr = np.abs(out["obs2"][:, 8:10] - ev["obs2"][:, 8:10])
    assert oerr.max() <= move, f"{name}: obs[8:10] off by {oerr.max():.3e} after two steps"
    _report(f"{name}: heading error / bound after step 1 and 2: {worst[0]:.3f}, {worst[1]:.3f}; obs[8:10] after two steps {oerr.max():.3e}")


@pytest.mark.parametrize("vehicle,scenario,C,threads", [("BlueROV2", "SimpleDocking3d", 0, 256), ("BlueROV2", "CapsuleDocking3d", 1, 256),
                                                       ("LAUV", "CapsuleDocking3d", 1, 512)])
def test_heading_wrap_two_steps_and_the_resident_sequence(vehicle, scenario, C, threads):
    """the low word carried across the wrap is used by the second step; the resident sequence of two steps against two single
    launches, bit for bit.  (The C ABI has no query for "served resident": dockauv_step_sequence launches the steps one by one
    where select_sequence has no kernel.  These handles meet its conditions -- float32, structural fast path, packed rows, no
    terminal observations, reward set 1, reset mode "none", a sensor-free handle or a 63-ray fan -- and tests/test_gpu_reset.py
    holds the resident kernels of these shapes to single launches over many steps.)"""
    b = S.bundle(vehicle, False, C, 0, n_envs=80, classes=("heading-wrap",))
    sc = b["scene"]
    expect = _expect("f32", threads, scenario, vehicle)
    single = _run(sc, "f32", "product", threads, scenario, vehicle=vehicle, steps=2, expect=expect)
    _check(f"heading wrap {vehicle} {scenario} f32 product {threads}", b, single, "f32", packed=True)
    _check_wrap_headings(f"heading wrap {vehicle} {scenario} f32 product {threads}", b, single, "f32")
    resident = _run(sc, "f32", "product", threads, scenario, vehicle=vehicle, steps=2, resident=True, expect=expect)
    diff = np.argwhere(single["rows"] != resident["rows"])
    assert diff.size == 0, f"resident sequence vs single launches: {len(diff)} words differ, first (step, env, word) {tuple(diff[0])}"
    assert np.array_equal(single["state2"], resident["state2"])
    full = _run(sc, "f64", "full", 256, scenario, vehicle=vehicle, steps=2, expect=(256, True, True))
    _check(f"heading wrap {vehicle} {scenario} f64 full", b, full, "f64")
    _check_wrap_headings(f"heading wrap {vehicle} {scenario} f64 full", b, full, "f64")


# ------------------------------------------------------------------------------------------------ one decision at a tie
def _ulps(x, k, dtype):
    """x moved by k units in the last place of dtype"""
    x = np.asarray(x, dtype)
    i = x.view(np.int32 if dtype == np.float32 else np.int64)
    return (i + np.where(x >= 0, k, -k).astype(i.dtype)).view(dtype)


def _dist2(g, p, dtype):
    """the kernel's squared distance (dockauv_step.hip.inc: dist2_xyz) in dtype; the fused multiply-adds of the float32 kernels
    are exact in float64 up to a double rounding"""
    d = (g.astype(dtype) - p.astype(dtype)).astype(dtype)
    if dtype == np.float32:
        d = d.astype(np.float64)
        s = (d[..., 0] * d[..., 0]).astype(np.float32).astype(np.float64)
        s = (d[..., 1] * d[..., 1] + s).astype(np.float32).astype(np.float64)
        return (d[..., 2] * d[..., 2] + s).astype(np.float32)
    return d[..., 2] * d[..., 2] + (d[..., 1] * d[..., 1] + d[..., 0] * d[..., 0])


def _dist2_exact(g, p):
    """the same for one float64 goal, with correctly rounded fused multiply-adds"""
    from fractions import Fraction
    d = [Fraction(float(a - b)) for a, b in zip(g, p)]
    s = float(d[0]) * float(d[0])
    for k in (1, 2):
        s = float(d[k] * d[k] + Fraction(s))
    return s


def _tie_goals(post, kind, dtype, rs):
    """goals [N, 3] in dtype whose squared distance from the kernel's own post-step position, as the kernel forms it, is the
    squared threshold moved by env % 5 - 2 units in the last place (the square root maps two neighbours of the square onto one
    value: -2 .. 2 reach both sides of the comparison) -- or as near to it as a search over +-6 units in the last place of each
    goal coordinate gets.  Returns the goals and exact [N]: the kernel's squared distance IS the squared threshold."""
    N = post.shape[0]
    p = post[:, 0:3].astype(dtype)
    goal, exact = np.zeros((N, 3), dtype), np.zeros(N, bool)
    k = np.arange(-6, 7)
    off = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    for i in range(N):
        thr = dtype(S.DTOL if kind[i] == 0 else S.DMAX)
        want = _ulps(thr * thr, i % 5 - 2, dtype)
        d = rs.normal(size=3)
        g0 = (p[i].astype(np.float64) + float(thr) * d / np.linalg.norm(d)).astype(dtype)
        cand = np.stack([_ulps(np.full(off.shape[0], g0[c], dtype), off[:, c], dtype) for c in range(3)], axis=1)
        d2 = _dist2(cand, p[i][None, :], dtype)
        near = np.argsort(np.abs(d2.astype(np.float64) - float(want)))
        goal[i] = cand[near[0]]
        if dtype == np.float64:      # (the search ran without the fused roundings: of its best candidates the one that meets them)
            d2x = [_dist2_exact(cand[j], p[i]) for j in near[:24]]
            hit = [j for j, v in zip(near[:24], d2x) if v == float(want)]
            goal[i] = cand[hit[0]] if hit else goal[i]
        d2 = _dist2(goal[i], p[i], dtype) if dtype == np.float32 else _dist2_exact(goal[i], p[i])
        exact[i] = d2 == thr * thr
    return goal, exact


TIE_LAYOUTS = [("f32", "product", 256, "SimpleDocking3d", 0), ("f32", "product", 128, "SimpleDocking3d", 0), ("f32", "product", 64, "SimpleDocking3d", 0),
               ("f32", "term", 256, "SimpleDocking3d", 0), ("f32", "product", 512, "CapsuleDocking3d", 1), ("f32", "product", 256, "CapsuleDocking3d", 1),
               ("f32", "product", 64, "CapsuleDocking3d", 1), ("f32", "term", 512, "CapsuleDocking3d", 1), ("f32", "term", 256, "CapsuleDocking3d", 1),
               ("f32", "full", 256, "CapsuleCurrentDocking3d", 1), ("f64", "full", 256, "CapsuleCurrentDocking3d", 1), ("f64", "full", 256, "SimpleDocking3d", 0)]


@pytest.mark.parametrize("precision,path,threads,scenario,C", TIE_LAYOUTS)
def test_one_decision_at_a_tie(precision, path, threads, scenario, C):
    """done flag set <=> observation row all zeros <=> terminal observation row written and non-zero <=> t_steps back at 0 <=>
    state replaced by the next episode <=> the reward carries a fired weight; for an env not done, the mirror image of each."""
    from gym_dockauv_amd import _capi
    dtype = np.float64 if precision == "f64" else np.float32
    b = S.bundle("BlueROV2", False, C, 0, n_envs=208, classes=("goal-tol", "goal-far", "attitude"))
    base = b["scene"]
    N = base["state"].shape[0]
    sc = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    sc["tsteps"][:] = S.TMAX - 1
    if "Current" in scenario:      # (the probe and the deciding step must see the same current: not the one a reset draws)
        sc["current"][:] = (0.3, 0.3, 0.3, 0.4, -0.2)
        sc["with_current"] = True
    kind = np.where(base["label"] == "goal-tol", 0, np.where(base["label"] == "goal-far", 1, 2))
    reset_mode = "pool" if path == "full" else "device"

    def one_step(reset, want_probe):
        env = _make_env(sc, precision, threads, scenario, "BlueROV2", reset_mode=reset)
        try:
            _load(env, sc, expect=_expect(precision, threads, scenario, reset_mode=reset))
            act = sc["action"][:, :env.n_u]
            n = env.n_observations
            pool = env.get_field(_capi.F_POOL_POSE) if reset == "pool" else None
            if path == "full":
                obs, rew, done, _ = env.step(act) if not want_probe else env.step(act, extras=True)
                rows, tobs = np.concatenate([obs, np.asarray(rew, np.float32)[:, None], done[:, None].astype(np.float32)], axis=1), env._termobs.copy()
            else:
                r, tobs = _device_steps(env, act, path)
                rows = r[0]
            return dict(obs=rows[:, :n], reward=rows[:, n].astype(np.float64), done=rows[:, n + 1] > 0.5, tobs=tobs, state=env.state.copy(),
                        tsteps=env.t_steps.copy(), pool=pool)
        finally:
            env.close()
    # 1. the kernel's own post-step pose (the same kernel: the reset mode is a run-time constant of it)
    probe = one_step("none", True)
    rs = np.random.RandomState(5)
    # 2. goals at the thresholds as the kernel computes them; attitudes moved by the kernel's own miss of max_attitude
    goals, exact = _tie_goals(probe["state"], kind, dtype, rs)
    sc["goal"][:, 0:3] = goals.astype(np.float64)
    exact &= kind < 2
    att = np.flatnonzero(kind == 2)
    axis = {int(i): (3 if abs(probe["state"][i, 3]) > abs(probe["state"][i, 4]) else 4) for i in att}
    for i in att:
        k = axis[i]
        sc["state"][i, k] -= float(dtype(probe["state"][i, k])) - np.sign(probe["state"][i, k]) * float(dtype(S.MATT))
    sc["goal"][att, 0:3] = probe["state"][att, 0:3] + [3.0, 1.0, 0.5]
    name = f"ties {precision} {path} {threads} {scenario}"
    # (the post-step attitude does not move one to one with the pre-step one -- the restoring moment: further probes with the
    # moved attitudes give the slope, secant steps land the tie; the pre-step value that landed nearest is kept)
    matt = float(dtype(S.MATT))
    col = np.array([axis[int(i)] for i in att])
    x0, y0 = base["state"][att, col], probe["state"][att, col]
    x1 = sc["state"][att, col].copy()
    want = np.sign(y0) * matt
    best_x, best_miss = x1.copy(), np.full(att.size, np.inf)
    for it in range(6):
        y1 = one_step("none", True)["state"][att, col]
        m1 = np.abs(y1 - want)
        better = m1 < best_miss
        best_x[better], best_miss[better] = x1[better], m1[better]
        if (best_miss <= 2 * float(np.spacing(dtype(S.MATT)))).all():
            break
        dy = y1 - y0
        x2 = np.where(dy != 0, x1 - (y1 - want) * (x1 - x0) / np.where(dy != 0, dy, 1.0), x1)
        x2 = x1 + np.clip(x2 - x1, -1e-2, 1e-2)
        x0, y0, x1 = x1, y1, x2
        sc["state"][att, col] = x1
    sc["state"][att, col] = best_x
    landed = one_step("none", True)["state"][att, 3:5]
    miss = np.abs(np.abs(landed).max(axis=1) - matt) / float(np.spacing(dtype(S.MATT)))
    beyond = np.abs(landed).max(axis=1) > matt
    _report(f"{name}: attitude ties land within {miss.max():.1f} ulp of max_attitude, {int(beyond.sum())} of {att.size} beyond it")
    assert miss.max() <= 8.0, f"{name}: an attitude tie landed {miss.max():.1f} ulp from max_attitude"
    assert 0 < beyond.sum() < att.size, f"{name}: the attitude ties all fell on one side"
    # 3. the step that decides
    out = one_step(reset_mode, False)
    done = out["done"]
    assert np.array_equal(done[att], beyond), f"{name}: attitude ties {att[done[att] != beyond][:8]} decided against their own post-step attitude"
    _report(f"{name}: {int(done.sum())} of {N} envs done; per kind (goal, far, attitude) {[int(done[kind == k].sum()) for k in range(3)]} of "
            f"{[int((kind == k).sum()) for k in range(3)]}")
    for k in (0, 1):
        assert 0 < done[kind == k].sum() < (kind == k).sum(), f"{name}: the ties of kind {k} all fell on one side"
    # where the kernel's squared distance IS the squared threshold (0.25, 400: their roots are exact) the distance equals the
    # threshold, and neither `delta_d < tol` nor `delta_d > max` fires (docking3d.py:608-609)
    _report(f"{name}: {int(exact.sum())} envs exactly on a distance threshold, {int(done[exact].sum())} of them done")
    assert exact[kind == 0].sum() >= 5 and exact[kind == 1].sum() >= 5, f"{name}: too few exact ties ({exact[kind == 0].sum()}, {exact[kind == 1].sum()})"
    assert not done[exact].any(), f"{name}: envs {np.flatnonzero(done & exact)[:8]} sit exactly on a distance threshold and are done"
    zero_row = ~out["obs"].any(axis=1)
    assert np.array_equal(zero_row, done), f"{name}: zeroed observation rows {np.flatnonzero(zero_row != done)[:8]} disagree with done"
    if out["tobs"] is not None:
        written = out["tobs"].any(axis=1)
        assert np.array_equal(written, done), f"{name}: terminal observations {np.flatnonzero(written != done)[:8]} disagree with done"
    assert np.array_equal(out["tsteps"] == 0, done) and (out["tsteps"][~done] == S.TMAX).all(), f"{name}: step counters disagree with done"
    fresh = ~out["state"][:, 6:12].any(axis=1)
    assert np.array_equal(fresh, done), f"{name}: replaced states {np.flatnonzero(fresh != done)[:8]} disagree with done"
    if out["pool"] is not None:
        same = (np.abs(out["state"][:, 0:6] - out["pool"]) <= 1e-6 * (1 + np.abs(out["pool"]))).all(axis=1)
        assert same[done].all() and not same[~done].any(), f"{name}: the staged episode is not where done says"
    weight = np.abs(out["reward"]) > 50.0      # (the smallest fired weight is 200 here, the other twelve terms stay below 10)
    assert np.array_equal(weight, done), f"{name}: rewards {np.flatnonzero(weight != done)[:8]} disagree with done"
