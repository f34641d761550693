"""GPU: the ray stage of the step kernel -- obstacle culling, ray vs capsule (shaft / caps) and sphere, the may-be-hit masks, the
smallest-positive rule, the body collision -- against the oracle on the constructed scenes of tests/ray_scenes.py, in every group
layout: eight-, four- and one-wave groups, one-wave groups with the capsule records in registers, the lane = env mapping of fans
wider than 64 rays, the sphere-only and the lean twins, each as full-output (host pointers) and as product (device pointers)
instantiation.  One step from rest through the C ABI as in tests/test_gpu_rays.py (reset_mode "none", set_field); every row
asserts threads_in_use, step_uses_current and step_uses_capsules, so that it cannot silently run another kernel.  The scenes run
with blocksize_reduce = 1: every ray is a cell of the observation, which is all a product kernel emits of it.

Bounds.  float64: EVERY ray of EVERY case within TOL["f64"]["ray"] of the oracle, collision flags equal, observations within
1e-6, reward within TOL["f64"].  float32, on the float32-qualified cases (ray_scenes.qualify): no hit / miss flip, no collision
flip, per ray |d - d_ref| <= max(8 e_ref, TOL["f32"]["ray"]) with e_ref the largest movement of that class's rays between the
oracle on the float64 inputs and the oracle on what a float32 handle holds (the reference's own sensitivity; 8 = the margin of
DESIGN.md section 7C); the same divided by ray_max plus half a float32 ulp for the cells; the reward within TOL["f32"] or 8 x
the reference's own movement.  The largest error / bound per class is printed (and appended to the file DOCKAUV_RAY_EDGES_REPORT
names, if set).  Twins that the project holds bit for bit against their parent do the same here."""
import copy
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import ray_scenes as S

pytestmark = pytest.mark.gpu


def _report(line):
    print(line)
    path = os.environ.get("DOCKAUV_RAY_EDGES_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _config(radar, vehicle):
    from gym_dockauv_amd.config.env_config import BASE_CONFIG
    cfg = copy.deepcopy(BASE_CONFIG)
    cfg["radar"] = dict(radar)
    if vehicle != "mixed":
        cfg["vehicle"] = vehicle
    return cfg


def _run(scene, precision, path, threads, scenario, vehicle="BlueROV2", radar=None, expect=None, current_row=None):
    """One step of the scene.  path: "full" (host pointers, every optional output), "product" (device pointers, packed rows),
    "term" (product with terminal observations).  expect: (threads_in_use, step_uses_current, step_uses_capsules) at the step.
    current_row: written to env 0's current row first (a row that is not all zeros takes the lean twins away).
    Returns dict(dist, collision: full only; obs, reward, done, state, rows: product paths, the packed rows as bits)."""
    import torch
    from gym_dockauv_amd import _capi
    from gym_dockauv_amd.envs.batched import BatchedDocking3d
    N = scene["state"].shape[0]
    C, Sp = scene["max_capsules"], scene["max_spheres"]
    env = BatchedDocking3d(_config(radar or scene["radar"], vehicle), num_envs=N, scenario=scenario, precision=precision, reset_mode="none",
                           rng="batched", max_capsules=C, max_spheres=Sp, threads_per_group=threads,
                           vehicles=list(scene["vehicle"]) if vehicle == "mixed" else None)
    try:
        env.reset()
        env.set_field(_capi.F_STATE, scene["state"])
        env.set_field(_capi.F_GOAL, scene["goal"])
        cur = np.zeros((N, 5))
        if current_row is not None:
            cur[0] = current_row
        env.set_field(_capi.F_CURRENT, cur)
        if C:
            env.set_field(_capi.F_CAPSULES, scene["capsules"])
        if Sp:
            env.set_field(_capi.F_SPHERES, scene["spheres"])
        if expect is not None:
            got = (env.threads_in_use, env.step_uses_current, env.step_uses_capsules)
            assert got == expect, f"(threads, uses current, uses capsules) = {got}, the row is about {expect}"
        out = {}
        act = np.zeros((N, env.n_u))
        if path == "full":
            obs, rew, done, _ = env.step(act, extras=True)
            out.update(dist=np.asarray(env.intersec_dist, np.float64).copy(), collision=env.conditions[:, 4].copy())
        else:
            dev = torch.device("cuda", env.device)
            rows = torch.zeros((N, env.n_observations + 2), device=dev, dtype=torch.float32)
            tobs = torch.zeros((N, env.n_observations), device=dev, dtype=torch.float32) if path == "term" else None
            a = torch.zeros((N, env.n_u), device=dev, dtype=torch.float64 if precision == "f64" else torch.float32)
            env.step_device(a.data_ptr(), rows.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, packed=True,
                            terminal_obs_ptr=tobs.data_ptr() if tobs is not None else 0)
            torch.cuda.synchronize()
            r = rows.cpu().numpy()
            n = env.n_observations
            obs, rew, done = r[:, :n].copy(), r[:, n].astype(np.float64), r[:, n + 1] > 0.5
            out["rows"] = r.view(np.int32).copy()
        out.update(obs=np.asarray(obs, np.float64), reward=np.asarray(rew, np.float64), done=np.asarray(done, bool), state=env.state.copy())
    finally:
        env.close()
    return out


def _check(name, b, out, precision, obs_ref=None):
    """the bounds of the module docstring; obs_ref: the oracle's observation if it is not the bundle's (another block size)"""
    sc, ev, q, move = b["scene"], b["ev64"], b["q"], b["move"]
    R = float(sc["fan"].max_dist)
    tol = H.TOL[precision]
    obs_ref = ev["obs"] if obs_ref is None else obs_ref
    pos_err = np.abs(out["state"][:, 0:3] - ev["pose"][:, 0:3]).max()
    assert pos_err < (1e-9 if precision == "f64" else S.SHIFT), f"{name}: the rays are cast from another pose ({pos_err})"
    rew_err = np.abs(out["reward"] - ev["reward"])
    if precision == "f64":
        if "dist" in out:
            err = np.abs(out["dist"] - ev["dist"])
            w = int(err.max(axis=1).argmax())
            assert not (err > tol["ray"]).any(), (f"{name}: {int((err > tol['ray']).sum())} rays off, worst {err.max():.3e} at env "
                                                 f"{w} ({sc['label'][w]} {sc['sub'][w]})")
            cdiff = np.flatnonzero(out["collision"] != ev["collision"])
            assert cdiff.size == 0, f"{name}: collision flags differ at {cdiff[:8]}"
            _report(f"{name}: max ray error {err.max():.3e} m (bound {tol['ray']:.0e})")
        assert np.array_equal(out["done"], ev["done"]), name
        oerr = np.abs(out["obs"] - obs_ref)
        assert oerr.max() <= 1e-6, f"{name}: observation off by {oerr.max():.3e} at {np.unravel_index(oerr.argmax(), oerr.shape)}"
        bad = rew_err > tol["rew_abs"] + tol["rew_rel"] * np.abs(ev["reward"])
        assert not bad.any(), f"{name}: reward off at envs {np.flatnonzero(bad)[:8]}: {rew_err[bad][:8]}"
        return
    ok = q["qualified"]
    assert ok.sum() >= 0.85 * ok.size
    half_ulp = 2.0 ** -24
    parts = []
    for cls in S.CLASSES:
        m = ok & (sc["label"] == cls)
        if not m.any():
            continue
        bound = max(8 * move[cls]["ray"], tol["ray"])
        ratio_d = None
        if "dist" in out:
            d, d_ref = out["dist"][m], ev["dist"][m]
            flips = (d < R) != (d_ref < R)
            first = np.argwhere(flips)[0] if flips.any() else None
            assert first is None, f"{name} {cls}: {int(flips.sum())} hit / miss flips, first at (case, ray) {first} ({sc['sub'][m][first[0]]})"
            cflip = out["collision"][m] != ev["collision"][m]
            assert not cflip.any(), f"{name} {cls}: collision flips at {sc['sub'][m][cflip][:4]}"
            ratio_d = float(np.abs(d - d_ref).max() / bound)
        dflip = out["done"][m] != ev["done"][m]
        assert not dflip.any(), f"{name} {cls}: done flips at {sc['sub'][m][dflip][:4]}"
        cells, cells_ref = out["obs"][m][:, 16:], obs_ref[m][:, 16:]
        cflips = (cells < 1.0) != (cells_ref < 1.0)
        first = np.argwhere(cflips)[0] if cflips.any() else None
        assert first is None, f"{name} {cls}: {int(cflips.sum())} hit / miss flips in the cells, first {first} ({sc['sub'][m][first[0]]})"
        ratio_c = float(np.abs(cells - cells_ref).max() / (bound / R + half_ulp))
        head = np.abs(out["obs"][m][:, :16] - obs_ref[m][:, :16])
        head[:, 2] = np.minimum(head[:, 2], np.abs(2.0 - head[:, 2]))
        assert head.max() <= tol["obs"], f"{name} {cls}: obs[:16] off by {head.max():.3e}"
        rb = np.maximum(tol["rew_abs"] + tol["rew_rel"] * np.abs(ev["reward"][m]), 8 * move[cls]["reward"])
        ratio_r = float((rew_err[m] / rb).max())
        parts.append((cls, int(m.sum()), ratio_d, ratio_c, ratio_r))
    _report(f"{name}: error / bound per class (cases; rays, cells, reward): "
            + "; ".join(f"{c} ({n}; {'-' if rd is None else f'{rd:.3f}'}, {rc:.3f}, {rr:.3f})" for c, n, rd, rc, rr in parts))
    for cls, n, rd, rc, rr in parts:
        assert rd is None or rd <= 1.0, f"{name} {cls}: ray error {rd:.3f} x its bound"
        assert rc <= 1.0, f"{name} {cls}: cell error {rc:.3f} x its bound"
        assert rr <= 1.0, f"{name} {cls}: reward error {rr:.3f} x its bound"


def _same_bits(name, a, b):
    diff = np.argwhere(a["rows"] != b["rows"])
    assert diff.size == 0, f"{name}: {len(diff)} words of the packed rows differ, first at (env, word) {tuple(diff[0])}"


GENERAL, LEAN = "CapsuleCurrentDocking3d", "CapsuleDocking3d"     # a scenario with a water current (rows zeroed here) / without


# ------------------------------------------------------------------------------------------------ 63 rays, 3 + 3 slots, BlueROV2
@pytest.mark.parametrize("threads", [64, 256, 512])
@pytest.mark.parametrize("precision,path", [("f64", "full"), ("f32", "full"), ("f32", "product"), ("f32", "term")])
def test_default_fan_capsules_and_spheres(precision, path, threads):
    b = S.bundle("7x9", 3, 3)
    out = _run(b["scene"], precision, path, threads, GENERAL, expect=(threads, True, True))
    _check(f"7x9 3+3 BlueROV2 {precision} {path} {threads}", b, out, precision)
    if path == "term":      # the TERM twin against the plain product kernel, bit for bit
        _same_bits(f"7x9 3+3 term vs plain {threads}", out, _run(b["scene"], precision, "product", threads, GENERAL))


def test_default_fan_block_maximum():
    """the default 2 x 2 block maximum over the same scene: cells of four, two and one rays"""
    b = S.bundle("7x9", 3, 3)
    radar = dict(b["scene"]["radar"], blocksize_reduce=2)
    fan2 = S.ray_fan(radar)
    obs_ref = np.concatenate([b["ev64"]["obs"][:, :16],
                              np.stack([np.clip(fan2.reduce(d) / fan2.max_dist, 0, 1) for d in b["ev64"]["dist"]]).astype(np.float32)], axis=1)
    for precision, path, threads in (("f64", "full", 256), ("f32", "product", 256)):
        out = _run(b["scene"], precision, path, threads, GENERAL, radar=radar, expect=(threads, True, True))
        _check(f"7x9 3+3 blocks of 2 {precision} {path} {threads}", b, out, precision, obs_ref=obs_ref)


# ------------------------------------------------------------------------------------------------ capsules only: register records
@pytest.mark.parametrize("n_caps", [3, 5])
@pytest.mark.parametrize("precision,path,threads", [("f32", "full", 64), ("f32", "product", 64), ("f32", "full", 256), ("f32", "product", 256),
                                                    ("f64", "full", 64)])
def test_capsules_only_one_wave_records_in_registers(n_caps, precision, path, threads):
    """float32 one-wave groups keep the completed records of <= kRegCaps = 5 capsules in registers (product kernels; the full
    instantiation and float64 keep them in LDS).  The C ABI has no query for the register-record path: which of the two
    one-wave kernels runs follows from the handle's constants alone (dockauv_device.h: solo_regrec -- float32, no sphere slot,
    1..5 capsule slots, a 64-ray pad), and the rows below meet them; the rows cannot tell a fall-back to LDS records apart."""
    b = S.bundle("7x9", n_caps, 0, n_envs=256)
    out = _run(b["scene"], precision, path, threads, GENERAL, expect=(threads, True, True))
    _check(f"7x9 {n_caps}+0 {precision} {path} {threads}", b, out, precision)


# ------------------------------------------------------------------------------------------------ spheres only: the NOCAP twin
def test_sphere_only_twin_and_general_kernel():
    """A sphere-only handle has no lean (NOCUR) kernel of its own to compare with: select_step gives every handle without a
    capsule slot the sphere-only twin whenever it would give it the lean one (dockauv_device.h: nocap_shape), and losing the
    "no current" property takes both away at once.  So the twin is held, bit for bit, to the general kernel of the same
    handle; the lean twin against the general kernel is the next test's."""
    b = S.bundle("4x4", 0, 8, n_envs=256)
    sc = b["scene"]
    lean = _run(sc, "f32", "product", 256, "SphereDocking3d", expect=(256, False, False))
    _check("4x4 0+8 f32 product 256 sphere-only twin", b, lean, "f32")
    # a current row that is not all zeros (a direction: the speeds stay zero) puts the handle on the general kernel
    general = _run(sc, "f32", "product", 256, "SphereDocking3d", expect=(256, True, True), current_row=(0.0, 0.0, 0.0, 0.3, 0.0))
    _check("4x4 0+8 f32 product 256 general kernel", b, general, "f32")
    _same_bits("sphere-only twin vs general kernel", lean, general)
    _check("4x4 0+8 f64 full 64", b, _run(sc, "f64", "full", 64, "SphereDocking3d", expect=(64, True, True)), "f64")


def test_lean_twin_equals_the_general_kernel_on_the_default_fan():
    b = S.bundle("7x9", 3, 3)
    lean = _run(b["scene"], "f32", "product", 256, LEAN, expect=(256, False, True))
    _check("7x9 3+3 f32 product 256 lean twin", b, lean, "f32")
    _same_bits("lean twin vs general kernel", lean, _run(b["scene"], "f32", "product", 256, GENERAL, expect=(256, True, True)))


# ------------------------------------------------------------------------------------------------ 117 and 4 rays
@pytest.mark.parametrize("fan_name", ["9x13", "2x2"])
@pytest.mark.parametrize("precision,path,threads", [("f64", "full", 256), ("f32", "product", 512), ("f64", "full", 512), ("f32", "product", 256)])
def test_wide_and_tiny_fans(fan_name, precision, path, threads):
    """117 rays: the mapping lane = env, wave = cell; 4 rays: 16 envs per wave pass"""
    b = S.bundle(fan_name, 2, 2, n_envs=256 if fan_name == "2x2" else 384)
    out = _run(b["scene"], precision, path, threads, GENERAL, expect=(threads, True, True))
    _check(f"{fan_name} 2+2 {precision} {path} {threads}", b, out, precision)


# ------------------------------------------------------------------------------------------------ LAUV and the mixed pair
@pytest.mark.parametrize("vehicle,precision,path,threads,scenario,uses_current",
                         [("LAUV", "f32", "product", 512, LEAN, False), ("LAUV", "f32", "product", 256, GENERAL, True),
                          ("LAUV", "f64", "full", 256, GENERAL, True), ("mixed", "f32", "product", 256, GENERAL, True),
                          ("mixed", "f64", "full", 512, GENERAL, True)])
def test_other_vehicles(vehicle, precision, path, threads, scenario, uses_current):
    b = S.bundle("7x9", 3, 3, vehicle=vehicle)
    out = _run(b["scene"], precision, path, threads, scenario, vehicle=vehicle, expect=(threads, uses_current, True))
    _check(f"7x9 3+3 {vehicle} {precision} {path} {threads}", b, out, precision)
    if not uses_current:    # the LAUV's lean twin against its general kernel, bit for bit
        _same_bits("LAUV lean twin vs general kernel", out, _run(b["scene"], precision, path, threads, GENERAL, vehicle=vehicle,
                                                                  expect=(threads, True, True)))


# ------------------------------------------------------------------------------------------------ the recorded edge cases
def _edge_scene():
    """The 14 edge_* cases of tests/golden/g4_rays.npz (ray parallel to the axis, tangent ray, y == 0, ...), one env each: a
    level vehicle at heading 0, the case turned so that its ray is the fan's central ray +x.  Of the four turns that keep the
    capsule's axis on a coordinate axis where the case allows it (axis -> NED +-z or +-y) the one is taken under which the
    ORACLE on the turned scene reproduces the recorded value: the vehicle rises by an inexact 5e-4 m in the step, and a tie
    (tangent ray, y == 0) survives only if that rounding falls on a coordinate the tie does not depend on.  A case that no
    turn reproduces is returned in `unreachable`."""
    from oracle import dockauv_oracle as orc
    g = H.load("g4_rays")
    radar = S.radar_config("7x9")
    fan = S.ray_fan(radar)
    _, _, centre = S.extreme_rays(fan)
    assert np.abs(fan.rd_b[centre] - [1.0, 0.0, 0.0]).max() < 1e-15     # (arange leaves ~1e-17 in the middle angle)
    n = g["edge_origins"].shape[0]
    model = orc.VehicleModel("bluerov2")
    post, _, _ = orc.auv_step(model, np.zeros(12), np.zeros(6), np.zeros(6), np.zeros(6), 0.1)
    assert post[0] == 0 and post[1] == 0 and not post[3:6].any()
    caps = np.zeros((n, 7))
    unreachable = []
    expected = fan.clamp(g["edge_dist"])
    c1, c2, rad = g["edge_cap1"], g["edge_cap2"], float(g["edge_rad"][0])
    axis = (c2 - c1) / np.linalg.norm(c2 - c1)
    for k in range(n):
        e1 = g["edge_dirs"][k] / np.linalg.norm(g["edge_dirs"][k])
        a_perp = axis - float(axis @ e1) * e1
        e2 = a_perp / np.linalg.norm(a_perp) if np.linalg.norm(a_perp) > 1e-9 else np.array([1.0, 0.0, 0.0]) - e1[0] * e1
        e2 = e2 / np.linalg.norm(e2)
        M = np.stack([e1, e2, np.cross(e1, e2)], axis=1)
        for t2 in (np.array([0.0, 0.0, 1.0]), np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, -1.0]), np.array([0.0, -1.0, 0.0])):
            Q = np.stack([np.array([1.0, 0.0, 0.0]), t2, np.cross([1.0, 0.0, 0.0], t2)], axis=1) @ M.T
            row = [*(post[0:3] + Q @ (c1 - g["edge_origins"][k])), *(post[0:3] + Q @ (c2 - g["edge_origins"][k])), rad]
            v = fan.clamp(np.array([orc.ray_capsule(post[0:3], fan.rd_b[centre], np.array(row[0:3]), np.array(row[3:6]), rad)]))[0]
            if abs(v - expected[k]) <= 1e-9:
                caps[k] = row
                break
        else:
            unreachable.append(k)
            caps[k] = row
    state = np.zeros((n, 12))
    goal = np.zeros((n, 4))
    goal[:, 0] = 5.0
    scene = dict(state=state, goal=goal, capsules=caps, spheres=np.zeros((n, 0)), max_capsules=1, max_spheres=0, radar=radar, fan=fan,
                 vehicle=np.array(["BlueROV2"] * n), ncap=np.ones(n, int), nsph=np.zeros(n, int), seed=0)
    return scene, expected, centre, unreachable


def test_recorded_edge_cases_on_the_central_ray():
    """Case 6 (a ray across the axis at the very height of an end: y == 0, the top cap wins and is missed) needs a ray EXACTLY
    across the axis; the fan's central ray is (1, 1.1e-16, 1.1e-16) (np.arange leaves that in the middle angle), under which
    the reference itself enters the other cap at 4 m.  That case is held to the oracle on the turned scene like every other ray
    of the 14 envs; the 13 others to their recorded values."""
    scene, expected, centre, unreachable = _edge_scene()
    assert unreachable == [6]
    ev = S.evaluate(scene)
    keep = np.setdiff1d(np.arange(expected.size), unreachable)
    for threads in (64, 512):
        out = _run(scene, "f64", "full", threads, GENERAL, expect=(threads, True, True))
        err = np.abs(out["dist"][keep, centre] - expected[keep])
        assert err.max() <= H.TOL["f64"]["ray"], f"{threads}: edge cases {keep[err > 1e-8]}: {out['dist'][:, centre]} != {expected}"
        # the other rays of these envs against the oracle, but for those an exact tie decides (a whole column of the fan is
        # tangent to case 8's shaft: rounding answers them, see ray_scenes.axis_aligned)
        for i in range(expected.size):
            a, b, r = S.body_frame(scene, ev, i)[0][0]
            clear = np.abs(S.line_segment_dist(scene["fan"].rd_b, a, b) - r) > 1e-9
            assert np.abs(out["dist"][i] - ev["dist"][i])[clear].max() <= H.TOL["f64"]["ray"], f"{threads}: edge case {i}"
        assert np.array_equal(out["collision"], ev["collision"])
