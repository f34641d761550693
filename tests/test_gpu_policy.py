"""The on-device MLP policy and the closed-loop rollout (include/dockauv.h: dockauv_policy_*, dockauv_rollout) on a real
MI355X: forward against float64, row independence bit for bit, the exploration noise against the Philox statement, a rollout
against the same steps issued one by one (bit for bit), TorchDocking3d.rollout, and refusals on a live handle.

Every policy_mlp_kernel<MT1, MT2> the library ships is launched here (test_every_tile_pair_matches_float64: first hidden widths
17 / 33 / 96 / 128 x second hidden widths 0 / 32 / 63 / 65 / 128, batches of one lane, a tile plus a lane and a group plus a
lane, odd observation widths 25 and 51, sentinel rows behind the action buffer), the largest shape the 160 KiB of LDS take
(133-128-128) and the first one they refuse (159-128-128), one poisoned row inside a tile, saturated tanh units (scaled weights,
bound from a float32 NumPy forward of the same case), per-action log_std with 3 and 8 actions with and without the tanh
output, the rollout of a mixed batch and of direct thruster control, and the closed loop against the oracle driven by the
float64 forward.  Which kernel each test launches: profiles/coverage/kernels.txt.

Measured figures (profiles/policy/forward_error.txt, written by scripts/policy_error.py from the helpers of this file; the
numbers are printed by the tests as well):
  forward, max |a - a_f64| over all shapes and batch sizes of case 1 .... see forward_max_abs_err, bound 1e-5
  exploration, max |z_dev - z_ref| over 65 536 x 6 draws .................. see exploration_max_dev, bound 4 x that, cap 1e-4
  scaled weights, device and float32-NumPy error against float64 ........... see scaled_x4_* / scaled_x16_*, bound 8 x NumPy's
  closed loop against the oracle, max |obs - obs_oracle| over 14 steps ..... see closed_loop_max_obs_dev, bound helpers.TOL
"""
import copy
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "policy", "forward_error.txt")

# (n_in, hidden, n_out, hidden_act, out_act): what the issue names; the env that has these n_obs / n_u is env_for()
SHAPES = [(20, (64, 64), 6, "tanh", "none"), (36, (64, 64), 3, "tanh", "none"), (20, (48, 17), 6, "relu", "tanh"),
          (36, (128,), 8, "tanh", "none")]
# the widest two-layer actor: its packed weights (about 93 KB) are beyond the 64 KiB of LDS a launch gets without asking, so
# it is the shape that takes the launch path with the explicit request; same weights, rows and bound as the others
WIDE = (20, (128, 128), 6, "tanh", "none")
FORWARD_BOUND = 1e-5          # the project's float32 bar (BASELINE.json north_star)
EXPLORATION_CAP = 1e-4


def recorded(key: str) -> float:
    for line in open(RECORD):
        parts = line.split()
        if len(parts) >= 2 and parts[0] == key:
            return float(parts[1])
    raise AssertionError(f"{key} is not recorded in {RECORD}")


def make_mlp(shape, seed=0, log_std=None):
    """torch's default initialisation: weights and biases U(+-1 / sqrt(fan_in))"""
    from gym_dockauv_amd.policy import MLPPolicy
    n_in, hidden, n_out, act, out_act = shape
    rng = np.random.default_rng(seed)
    layers, n = [], n_in
    for w in list(hidden) + [n_out]:
        b = 1.0 / np.sqrt(n)
        layers.append((rng.uniform(-b, b, (w, n)), rng.uniform(-b, b, w)))
        n = w
    return MLPPolicy(layers, act, out_act, log_std)


def env_for(n_in, n_out, n_envs, max_timesteps=None, device_seed=7, precision="f32"):
    """A batch whose n_obs / n_u are (n_in, n_out): (20, 6) config 3 (BlueROV2, 4 x 4 fan, 8 spheres); (36, 3) config 4 (LAUV,
    7 x 9 fan, 5 capsules); (36, 8) BlueROV2 with direct thruster control and the 7 x 9 fan; (36, 6) config 5 (BlueROV2 and LAUV
    interleaved: n_u is the wider vehicle's, the LAUV envs take the first three actions)."""
    import bench
    from gym_dockauv_amd.envs.batched import BatchedDocking3d
    from gym_dockauv_amd.objects.vehicle_models import BlueROV2
    kw = {}
    if (n_in, n_out) == (20, 6):
        wl = bench.workload(3, n_envs)
    elif (n_in, n_out) == (36, 3):
        wl = bench.workload(4, n_envs)
    elif (n_in, n_out) == (36, 8):
        wl = bench.workload(2, n_envs)
        kw["vehicle_models"] = [BlueROV2(control_mode="direct")]
    elif (n_in, n_out) == (36, 6):
        wl = bench.workload(5, n_envs)
        kw["vehicles"] = wl["vehicles"]
    else:
        raise KeyError((n_in, n_out))
    cfg = copy.deepcopy(wl["cfg"])
    if max_timesteps is not None:
        cfg["max_timesteps"] = max_timesteps
    env = BatchedDocking3d(cfg, num_envs=n_envs, scenario=wl["scenario"], device=0, precision=precision, reset_mode="device",
                           device_seed=device_seed, rng="batched", **kw)
    assert (env.n_observations, env.n_u) == (n_in, n_out)
    env._gen = np.random.default_rng(3)
    env.reset()
    return env


def nan_rows(torch, n, n_in, seed):
    """observation columns U(-1, 1); reward and done columns NaN: they must never enter the arithmetic"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    rows = torch.rand((n, n_in + 2), device="cuda", generator=g) * 2 - 1
    rows[:, n_in:] = float("nan")
    return rows.contiguous()


def forward(torch, env, pol, rows, t=0, stochastic=False):
    acts = torch.full((rows.shape[0], env.n_u), float("nan"), device="cuda")
    env.policy_forward_device(pol, rows.data_ptr(), acts.data_ptr(), t=t, stochastic=stochastic,
                              stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return acts


def forward_error(shape, n_envs):
    """max |a - a_f64| of one shape at one batch size (scripts/policy_error.py writes forward_error.txt with it)"""
    import torch
    mlp = make_mlp(shape, seed=1)
    env = env_for(shape[0], shape[2], n_envs)
    try:
        pol = env.make_policy(mlp)
        rows = nan_rows(torch, n_envs, shape[0], seed=2)
        a = forward(torch, env, pol, rows).cpu().numpy()
        assert not np.isnan(a).any(), "NaN in the actions: a reward / done column or an unwritten row got in"
        ref = mlp.forward_reference(rows[:, : shape[0]].cpu().numpy().astype(np.float64))
        return float(np.abs(a - ref).max())
    finally:
        env.close()


@pytest.mark.parametrize("n_envs", [1000, 65536])
@pytest.mark.parametrize("shape", SHAPES + [WIDE], ids=lambda s: f"{s[0]}-{'-'.join(map(str, s[1]))}-{s[2]}-{s[3]}-{s[4]}")
def test_forward_matches_float64(shape, n_envs):
    err = forward_error(shape, n_envs)
    print(f"policy forward {shape} N={n_envs}: max |a - a_f64| = {err:.3e} (bound {FORWARD_BOUND:g})")
    assert err <= FORWARD_BOUND


# ray fans by observation width (16 + block-max cells; RadarLayout): 20 the 4 x 4 fan of config 3; 36 the default 7 x 9 fan,
# 2 x 2 blocks; 25 the same fan, 3 x 3 blocks (ODD: the word behind the last observation is the reward column); 51 a 9 x 13 fan,
# 2 x 2 blocks (odd, 26 layer-1 k steps = two chunks); 133 the 9 x 13 fan unreduced; 159 an 11 x 13 fan unreduced
_DEG = np.pi / 180
FANS = {20: dict(alpha=30 * _DEG, beta=30 * _DEG, ray_per_deg=10 * _DEG, blocksize_reduce=2),
        36: dict(alpha=60 * _DEG, beta=80 * _DEG, ray_per_deg=10 * _DEG, blocksize_reduce=2),
        25: dict(alpha=60 * _DEG, beta=80 * _DEG, ray_per_deg=10 * _DEG, blocksize_reduce=3),
        51: dict(alpha=40 * _DEG, beta=60 * _DEG, ray_per_deg=5 * _DEG, blocksize_reduce=2),
        133: dict(alpha=40 * _DEG, beta=60 * _DEG, ray_per_deg=5 * _DEG, blocksize_reduce=1),
        159: dict(alpha=50 * _DEG, beta=60 * _DEG, ray_per_deg=5 * _DEG, blocksize_reduce=1)}
SENTINEL = -7.0


def fan_env(n_in, n_out, n_envs):
    """A float32 batch with n_obs = n_in (FANS) and n_u = n_out: 3 LAUV, 6 BlueROV2, 8 BlueROV2 with direct thruster control.
    The policy kernel takes nothing else from the handle, so any fan goes with any vehicle here."""
    from gym_dockauv_amd.config.env_config import BASE_CONFIG
    from gym_dockauv_amd.envs.batched import BatchedDocking3d
    from gym_dockauv_amd.objects.radar import RadarLayout
    from gym_dockauv_amd.objects.vehicle_models import BlueROV2
    cfg = copy.deepcopy(BASE_CONFIG)
    cfg["radar"].update(FANS[n_in])
    assert 16 + RadarLayout(**cfg["radar"]).n_rays_reduced == n_in
    kw = {}
    if n_out == 3:
        cfg["vehicle"], cfg["t_step_size"] = "LAUV", 0.02
    elif n_out == 8:
        kw["vehicle_models"] = [BlueROV2(control_mode="direct")]
    env = BatchedDocking3d(cfg, num_envs=n_envs, scenario="ObstaclesDocking3d", device=0, precision="f32", reset_mode="device",
                           device_seed=7, rng="batched", **kw)
    assert (env.n_observations, env.n_u) == (n_in, n_out)
    return env


def forward_guarded(torch, env, pol, rows, t=0, stochastic=False):
    """forward() into a buffer with 64 rows more than the batch, filled with a sentinel that must come back untouched"""
    n = rows.shape[0]
    acts = torch.full((n + 64, env.n_u), SENTINEL, device="cuda")
    env.policy_forward_device(pol, rows.data_ptr(), acts.data_ptr(), t=t, stochastic=stochastic,
                              stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((acts[n:] == SENTINEL).all()), "the kernel wrote behind the last env's actions"
    return acts[:n]


def guarded_error(shape, n_envs):
    """max |a - a_f64| of `shape` on a fan_env of n_envs envs; the rows' reward / done columns are NaN, the action buffer is
    guarded, and no action may be the sentinel (every live env was written)"""
    import torch
    mlp = make_mlp(shape, seed=1)
    env = fan_env(shape[0], shape[2], n_envs)
    try:
        pol = env.make_policy(mlp)
        rows = nan_rows(torch, n_envs, shape[0], seed=2)
        a = forward_guarded(torch, env, pol, rows).cpu().numpy()
        assert not np.isnan(a).any(), "NaN in the actions: a reward / done column or an unwritten row got in"
        assert not (a == SENTINEL).any(), "an action of a live env was not written"
        ref = mlp.forward_reference(rows[:, : shape[0]].cpu().numpy().astype(np.float64))
        return float(np.abs(a - ref).max())
    finally:
        env.close()


# one shape per policy_mlp_kernel<MT1, MT2>: ceil(width / 32) tiles per hidden layer, widths next to the tile edges; the hidden
# and the output activation alternate so that all four pairings occur, the observation width walks through two odd and two even
# ones and the action count through 3 / 6 / 8
TILE_PAIRS = []
for _i, (_h1, _h2) in enumerate((a, b) for a in (17, 33, 96, 128) for b in (0, 32, 63, 65, 128)):
    TILE_PAIRS.append(((25, 51, 20, 36)[_i % 4], (_h1, _h2) if _h2 else (_h1,), (3, 6, 8)[_i % 3], ("tanh", "relu")[_i % 2],
                       ("none", "tanh")[(_i // 2) % 2]))
# the largest shape the kernel's LDS takes: 151 712 B of packed weights (dockauv_device.h: policy_layout)
WIDEST = (133, (128, 128), 6, "tanh", "none")
_shape_id = lambda s: f"{s[0]}-{'-'.join(map(str, s[1]))}-{s[2]}-{s[3]}-{s[4]}"


@pytest.mark.parametrize("shape", TILE_PAIRS + [WIDEST], ids=_shape_id)
def test_every_tile_pair_matches_float64(shape):
    """Each of the 20 instantiations (and the widest accepted shape) against float64 at N = 1 (a single lane), 33 (a tile plus
    one lane) and 129 (a group plus one lane), bound 1e-5 as for the named shapes."""
    for n_envs in (1, 33, 129):
        err = guarded_error(shape, n_envs)
        print(f"policy forward {shape} N={n_envs}: max |a - a_f64| = {err:.3e} (bound {FORWARD_BOUND:g})")
        assert err <= FORWARD_BOUND, (shape, n_envs, err)


def test_poisoned_rows_stay_in_their_lanes():
    """One row of a full 32-env tile all NaN, another +-3e38 in alternating columns, and in the next tile a row with 3e38 in one
    column: exactly those envs' actions change.  The NaN row's actions are NaN; the huge rows' units are saturated tanh (+-1)
    or an overflowed sum, so each of their actions is non-finite or the float64 forward of that row (the one-column row cannot
    meet inf - inf: its actions are finite); every other env of the tile, of the group and of the batch keeps its bits."""
    import torch
    shape = SHAPES[0]
    mlp = make_mlp(shape, seed=1)
    N, i_nan, i_big, i_one = 96, 37, 50, 70          # (lanes 5 and 18 of the second tile, lane 6 of the third)
    env = env_for(20, 6, N)
    try:
        pol = env.make_policy(mlp)
        rows = nan_rows(torch, N, 20, seed=2)
        clean = forward_guarded(torch, env, pol, rows)
        bad = rows.clone()
        bad[i_nan, :20] = float("nan")
        bad[i_big, :20] = torch.tensor([3e38, -3e38] * 10, device="cuda")
        bad[i_one, 3] = 3e38
        got = forward_guarded(torch, env, pol, bad)
        keep = torch.ones(N, dtype=torch.bool, device="cuda")
        keep[[i_nan, i_big, i_one]] = False
        assert torch.equal(got[keep].view(torch.int32), clean[keep].view(torch.int32))
        assert bool(torch.isnan(got[i_nan]).all())
        big = got[i_big].cpu().numpy().astype(np.float64)
        ref = mlp.forward_reference(bad[i_big, :20].cpu().numpy().astype(np.float64))
        fin = np.isfinite(big)
        assert np.all(np.abs(big[fin] - ref[fin]) <= FORWARD_BOUND), (big, ref)
        assert not torch.equal(got[i_big].view(torch.int32), clean[i_big].view(torch.int32))
        one = got[i_one].cpu().numpy().astype(np.float64)
        assert np.isfinite(one).all(), one
        assert not torch.equal(got[i_one].view(torch.int32), clean[i_one].view(torch.int32))
        assert np.abs(one - mlp.forward_reference(bad[i_one, :20].cpu().numpy().astype(np.float64))).max() <= FORWARD_BOUND
    finally:
        env.close()


SCALED = (36, (128, 128), 3, "tanh", "none")


def scaled_errors(w_scale, x_scale, n_envs=1000):
    """(device error, float32-NumPy error, max |a_f64|) of SCALED with every weight and bias x w_scale and the observations
    x x_scale: most tanh units saturated.  Both errors are max |a - a_f64| over the batch; the NumPy forward is the same
    statement in float32 arrays (scripts/policy_error.py writes forward_error.txt with it)."""
    import torch
    from gym_dockauv_amd.policy import MLPPolicy
    base = make_mlp(SCALED, seed=1)
    mlp = MLPPolicy([(W * np.float32(w_scale), b * np.float32(w_scale)) for W, b in base.layers], SCALED[3], SCALED[4])
    env = env_for(36, 3, n_envs)
    try:
        pol = env.make_policy(mlp)
        rows = nan_rows(torch, n_envs, 36, seed=2)
        rows[:, :36] *= x_scale
        a = forward_guarded(torch, env, pol, rows).cpu().numpy().astype(np.float64)
        x32 = rows[:, :36].cpu().numpy()
    finally:
        env.close()
    ref = mlp.forward_reference(x32.astype(np.float64))
    h = x32
    for W, b in mlp.layers[:-1]:
        h = np.tanh(h @ W.T + b)
    W, b = mlp.layers[-1]
    a_np = (h @ W.T + b)
    assert a_np.dtype == np.float32
    return float(np.abs(a - ref).max()), float(np.abs(a_np.astype(np.float64) - ref).max()), float(np.abs(ref).max())


@pytest.mark.parametrize("w_scale,x_scale", [(4, 10), (16, 100)])
def test_saturated_tanh_units_against_float32_numpy(w_scale, x_scale):
    """Outputs of several units to tens of units: the absolute 1e-5 bar is not the yardstick there.  The device's error against
    float64 may be 8 x that of a float32 NumPy forward of the same case (tanh_'s 3e-7 absolute against libm's half ulp, and
    another accumulation order)."""
    dev, ref32, amax = scaled_errors(w_scale, x_scale)
    print(f"policy forward {SCALED} weights x{w_scale} obs x{x_scale}: max |a_f64| {amax:.2f}, device error {dev:.3e}, "
          f"float32 NumPy error {ref32:.3e}")
    assert amax > 4.0, "the case must leave the initialisation scale"
    assert dev <= 8.0 * ref32, (dev, ref32)


def test_widest_refused_shape_names_the_lds():
    """159 observations (an 11 x 13 fan unreduced) with a 128-128 actor: 165 024 B of packed weights, more than the 160 KiB the
    kernel keeps them in -- dockauv_policy_create refuses and hands out no policy."""
    from gym_dockauv_amd import _capi
    lib = _capi.load_library()
    env = fan_env(159, 6, 64)
    try:
        d = make_mlp((159, (128, 128), 6, "tanh", "none")).host_desc()
        p = C.c_void_p()
        rc = lib.dockauv_policy_create(env._handle, C.byref(d), C.byref(p))
        msg = lib.dockauv_last_error(env._handle)
        assert rc == -1 and not p.value and b"exceed" in msg, (rc, msg)
    finally:
        env.close()


@pytest.mark.parametrize("out_act", ["none", "tanh"])
@pytest.mark.parametrize("n_out", [3, 8])
def test_exploration_noise_per_action_log_std(n_out, out_act):
    """log_std distinct per action, 3 (config 4) and 8 (direct thrusters: lane half 1, registers 2 and 3) actions.  Raw output:
    (a_sto - a_det) / exp(log_std[j]) is the Philox statement's normal, column by column, within the float32 Box-Muller bound
    of test_exploration_noise_is_the_philox_statement plus 1e-6 for the float32 difference.  tanh output: the noise goes in
    BEFORE the activation, a_sto = forward_reference(obs, z) within FORWARD_BOUND + max(std) x that bound."""
    import torch
    from gym_dockauv_amd.policy import MLPPolicy
    N, seed, t = 1000, 0xC0FFEE1234, 17
    zb = min(4.0 * recorded("exploration_max_dev"), EXPLORATION_CAP)
    log_std = np.linspace(-1.5, 0.3, n_out)
    mlp = make_mlp((36, (64, 64), n_out, "tanh", out_act), seed=1, log_std=log_std)
    env = env_for(36, n_out, N)
    try:
        pol = env.make_policy(mlp, seed=seed)
        rows = nan_rows(torch, N, 36, seed=2)
        det = forward_guarded(torch, env, pol, rows, t=t).cpu().numpy().astype(np.float64)
        sto = forward_guarded(torch, env, pol, rows, t=t, stochastic=True).cpu().numpy().astype(np.float64)
        obs = rows[:, :36].cpu().numpy().astype(np.float64)
    finally:
        env.close()
    z_ref = MLPPolicy.normals_reference(seed, np.arange(N), t, n_out)
    std = np.exp(mlp.log_std.astype(np.float64))
    if out_act == "none":
        dev = np.abs((sto - det) / std - z_ref).max(axis=0)
        print(f"exploration n_out {n_out}: max |z_dev - z_ref| per column {np.array2string(dev, precision=2)}, bound {zb + 1e-6:.3e}")
        assert np.all(dev <= zb + 1e-6), (dev, zb)
    else:
        err = float(np.abs(sto - mlp.forward_reference(obs, z=z_ref)).max())
        bound = FORWARD_BOUND + float(std.max()) * zb
        print(f"exploration n_out {n_out}, tanh output: max |a_sto - a_f64(z_ref)| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (err, bound)
        assert float(np.abs(det - mlp.forward_reference(obs)).max()) <= FORWARD_BOUND
        assert float(np.abs(sto - det).max()) > 0.1


def test_rows_are_independent_bitwise():
    """An env's action is a function of its row and the weights alone: the 1 000 rows of case 1 inside a 4 096-row batch, at
    offset 777, give the same bits; so do two calls."""
    import torch
    shape = SHAPES[0]
    mlp = make_mlp(shape, seed=1)
    small, big = env_for(20, 6, 1000), env_for(20, 6, 4096)
    try:
        ps, pb = small.make_policy(mlp), big.make_policy(mlp)
        rows = nan_rows(torch, 1000, 20, seed=2)
        a1 = forward(torch, small, ps, rows)
        a2 = forward(torch, small, ps, rows)
        host = nan_rows(torch, 4096, 20, seed=9)
        host[777:1777] = rows
        a3 = forward(torch, big, pb, host)
        assert not torch.isnan(a1).any()
        assert torch.equal(a1.view(torch.int32), a2.view(torch.int32))
        assert torch.equal(a1.view(torch.int32), a3[777:1777].view(torch.int32))
    finally:
        small.close()
        big.close()


def exploration_deviation(check=None):
    """max |z_dev - z_ref| over 65 536 x 6 draws for t in {0, 1, 2^32 - 1} and env_id_offset in {0, 1 000 000}: z_dev =
    a_stochastic - a_deterministic with log_std = 0 (scripts/policy_error.py writes forward_error.txt with it)"""
    import torch
    from gym_dockauv_amd.policy import MLPPolicy
    N, seed = 65536, 0xC0FFEE1234
    mlp = make_mlp(SHAPES[0], seed=1, log_std=np.zeros(6))
    env = env_for(20, 6, N)
    worst = 0.0
    try:
        rows = nan_rows(torch, N, 20, seed=2)
        for off in (0, 1_000_000):
            pol = env.make_policy(mlp, seed=seed, env_id_offset=off)
            det = forward(torch, env, pol, rows, t=5, stochastic=False)
            for t in (0, 1, 2**32 - 1):
                sto = forward(torch, env, pol, rows, t=t, stochastic=True)
                z = (sto - det).cpu().numpy().astype(np.float64)
                ref = MLPPolicy.normals_reference(seed, off + np.arange(N), t, 6)
                dev = float(np.abs(z - ref).max())
                print(f"exploration offset {off} t {t}: max |z_dev - z_ref| = {dev:.3e}, z std {z.std():.4f}")
                worst = max(worst, dev)
                if check is not None:
                    check(dev)
    finally:
        env.close()
    return worst


def test_exploration_noise_is_the_philox_statement():
    bound = min(4.0 * recorded("exploration_max_dev"), EXPLORATION_CAP)

    def check(dev):
        assert dev <= bound, (dev, bound)
    worst = exploration_deviation(check)
    print(f"exploration: max deviation {worst:.3e}, bound {bound:.3e}")


def test_exploration_switches_and_seeds():
    import torch
    mlp = make_mlp(SHAPES[0], seed=1, log_std=np.full(6, -0.7))
    env = env_for(20, 6, 1000)
    try:
        rows = nan_rows(torch, 1000, 20, seed=2)
        plain = env.make_policy(make_mlp(SHAPES[0], seed=1))
        pol = env.make_policy(mlp, seed=11)
        twin = env.make_policy(mlp, seed=11)
        other = env.make_policy(mlp, seed=12)
        bits = lambda x: x.view(torch.int32)
        det = forward(torch, env, plain, rows)
        # stochastic = 0 with a loaded log_std: the deterministic bits; stochastic without a log_std: the same
        assert torch.equal(bits(forward(torch, env, pol, rows, t=3, stochastic=False)), bits(det))
        assert torch.equal(bits(forward(torch, env, plain, rows, t=3, stochastic=True)), bits(det))
        a = forward(torch, env, pol, rows, t=3, stochastic=True)
        assert torch.equal(bits(a), bits(forward(torch, env, twin, rows, t=3, stochastic=True)))
        assert not torch.equal(bits(a), bits(forward(torch, env, pol, rows, t=4, stochastic=True)))
        assert not torch.equal(bits(a), bits(forward(torch, env, other, rows, t=3, stochastic=True)))
        z = ((a - det) / np.exp(-0.7)).cpu().numpy()
        assert abs(z.std() - 1.0) < 0.05 and abs(z.mean()) < 0.05
    finally:
        env.close()


@pytest.mark.parametrize("stochastic", [False, True], ids=["deterministic", "stochastic"])
@pytest.mark.parametrize("case", ["A", "B", "C", "D"])
def test_rollout_equals_stepwise_bitwise(case, stochastic):
    """dockauv_rollout on one handle against K x (dockauv_policy_forward, dockauv_step) on a twin with the same seed: rows,
    actions, terminal observations where done and the final state / episode / step counters, bit for bit.  max_timesteps = 25
    puts in-kernel resets inside the window of K = 60 steps.  A: config 3, B: config 4, C: config 5 at 778 envs (a mixed batch,
    n_out = the wider vehicle's 6), D: direct thruster control at 1 000 envs (n_out = 8)."""
    import torch
    from gym_dockauv_amd import _capi
    n_in, n_out, N = {"A": (20, 6, 4096 + 40), "B": (36, 3, 2048 + 17), "C": (36, 6, 778), "D": (36, 8, 1000)}[case]
    K = 60
    shape = (n_in, (64, 64), n_out, "tanh", "none")
    # (D: eight thrusters driven with noise of std 0.6 leave the stability range of the reference's own integrator at h = 0.1 --
    # roll rate 1.6 -> 5.6 -> -949 rad/s and overflow within three steps, in the float64 oracle as on the device -- and the rows
    # would carry NaN rewards; with std 0.14 the oracle's rates stay below 2.1 rad/s over 150 envs x 60 steps)
    mlp = make_mlp(shape, seed=4, log_std=np.full(n_out, -2.0 if case == "D" else -0.5))
    e1, e2 = env_for(n_in, n_out, N, max_timesteps=25), env_for(n_in, n_out, N, max_timesteps=25)
    try:
        p1, p2 = e1.make_policy(mlp, seed=21), e2.make_policy(mlp, seed=21)
        stream = torch.cuda.current_stream().cuda_stream
        rows0 = torch.zeros((N, n_in + 2), device="cuda")
        mk = lambda *s: torch.zeros(s, device="cuda")
        r1, a1, t1 = mk(K, N, n_in + 2), mk(K, N, n_out), mk(K, N, n_in)
        r2, a2, t2 = mk(K, N, n_in + 2), mk(K, N, n_out), mk(K, N, n_in)
        e1.rollout_device(p1, rows0.data_ptr(), r1.data_ptr(), a1.data_ptr(), K, t0=100, stochastic=stochastic, stream=stream,
                          terminal_obs_ptr=t1.data_ptr())
        for k in range(K):
            src = rows0 if k == 0 else r2[k - 1]
            e2.policy_forward_device(p2, src.data_ptr(), a2[k].data_ptr(), t=100 + k, stochastic=stochastic, stream=stream)
            e2.step_device(a2[k].data_ptr(), r2[k].data_ptr(), stream=stream, packed=True, terminal_obs_ptr=t2[k].data_ptr())
        torch.cuda.synchronize()
        e1.poll_status()
        e2.poll_status()
        bits = lambda x: x.view(torch.int32)
        assert not torch.isnan(r1).any() and not torch.isnan(a1).any()
        assert torch.equal(bits(a1), bits(a2))
        assert torch.equal(bits(r1), bits(r2))
        done = r1[:, :, n_in + 1] > 0.5
        assert int(done.sum()) > 0 and bool(done.any(dim=0).any()), "no episode ended inside the window"
        assert torch.equal(bits(t1)[done], bits(t2)[done])
        assert float(a1.abs().max()) > 0 and not torch.equal(a1[0], a1[K - 1])
        for f in (_capi.F_STATE, _capi.F_EPISODE, _capi.F_TSTEPS):
            assert np.array_equal(e1.get_field(f), e2.get_field(f)), f
        assert e1.get_field(_capi.F_EPISODE).max() >= 1
        if stochastic:   # (and the noise is really there: the deterministic actions of the first step differ)
            d = torch.zeros((N, n_out), device="cuda")
            e2.policy_forward_device(p2, rows0.data_ptr(), d.data_ptr(), t=100, stochastic=False, stream=stream)
            torch.cuda.synchronize()
            assert not torch.equal(bits(d), bits(a1[0]))
    finally:
        e1.close()
        e2.close()


def closed_loop_vs_oracle(n=48, K=14):
    """dockauv_rollout of a deterministic 36-64-64-6 tanh actor on 48 float32 envs of SimpleCurrentDocking3d (no resets, the
    host's per-env episodes) for 14 steps (this actor rolls the first vehicle beyond max_attitude in step 15) against 48 OracleEnvs, each driven by MLPPolicy.forward_reference in float64 on its own
    observations.  Returns (max |obs - obs_oracle| with column 2 modulo 2, max relative reward deviation, done equal, number of
    oracle episodes that ended); scripts/policy_error.py records the first."""
    import torch
    from gym_dockauv_amd.envs.batched import BatchedDocking3d
    from oracle import dockauv_oracle as orc
    mlp = make_mlp((36, (64, 64), 6, "tanh", "none"), seed=4)
    env = BatchedDocking3d(num_envs=n, scenario="SimpleCurrentDocking3d", precision="f32", reset_mode="none", rng="per_env")
    try:
        assert (env.n_observations, env.n_u) == (36, 6)
        env.reset(seed=list(range(100, 100 + n)))
        pol = env.make_policy(mlp)
        rows0 = torch.zeros((n, 38), device="cuda")          # the reset observation (zeros)
        rows = torch.zeros((K, n, 38), device="cuda")
        acts = torch.zeros((K, n, 6), device="cuda")
        env.rollout_device(pol, rows0.data_ptr(), rows.data_ptr(), acts.data_ptr(), K, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        env.poll_status()
        rows = rows.cpu().numpy().astype(np.float64)
    finally:
        env.close()
    obs_ref, rew_ref, done_ref = np.zeros((K, n, 36)), np.zeros((K, n)), np.zeros((K, n), dtype=bool)
    for i in range(n):
        o = orc.OracleEnv("SimpleCurrentDocking3d")
        ob = o.reset(seed=100 + i)
        for k in range(K):
            ob, rew_ref[k, i], done_ref[k, i], _ = o.step(mlp.forward_reference(np.asarray(ob, dtype=np.float64)))
            obs_ref[k, i] = ob
            if done_ref[k, i]:
                break
    d = np.abs(rows[:, :, :36] - obs_ref)
    d[:, :, 2] = np.minimum(d[:, :, 2], np.abs(2.0 - d[:, :, 2]))
    rew = np.abs(rows[:, :, 36] - rew_ref) / np.maximum(1.0, np.abs(rew_ref))
    return float(d.max()), float(rew.max()), bool(np.array_equal(rows[:, :, 37] > 0.5, done_ref)), int(done_ref.sum())


def test_closed_loop_against_the_oracle():
    """The whole loop -- policy kernel, step kernel, the rows fed back -- against the reference's arithmetic in float64, within
    the suite's free-running float32 bar on observations (helpers.TOL["f32"]); no episode ends inside the window."""
    from tests import helpers as H
    dev, rew, done_equal, n_done = closed_loop_vs_oracle()
    tol = H.TOL["f32"]
    print(f"closed loop, 48 envs x 14 steps: max |obs - obs_oracle| = {dev:.3e} (bound {tol['obs']:g}), reward {rew:.3e}")
    assert n_done == 0, "the oracle ended an episode inside the window: shorten K"
    assert done_equal
    assert dev <= tol["obs"], dev


def test_torch_env_rollout():
    import torch
    import bench
    from gym_dockauv_amd.envs.torch_env import TorchDocking3d
    N = 1000
    wl = bench.workload(3, N)
    cfg = copy.deepcopy(wl["cfg"])
    cfg["max_timesteps"] = 25
    shape = SHAPES[0]
    mlp = make_mlp(shape, seed=6)

    def make():
        env = TorchDocking3d(cfg, num_envs=N, scenario=wl["scenario"], device_seed=9)
        env.batch._gen = np.random.default_rng(5)
        env.reset()
        return env
    ea, eb = make(), make()
    try:
        pa, pb = ea.make_policy(mlp), eb.make_policy(mlp)
        obs, act, rew, done = ea.rollout(pa, 20)
        assert tuple(obs.shape) == (20, N, 20) and tuple(act.shape) == (20, N, 6) and tuple(rew.shape) == (20, N)
        assert tuple(done.shape) == (20, N) and done.dtype == torch.bool and obs.dtype == act.dtype == rew.dtype == torch.float32
        assert obs.data_ptr() == rew.data_ptr() - 20 * 4           # views of one packed buffer
        obs2, act2, rew2, done2 = ea.rollout(pa, 40)
        o60, a60, r60, d60 = eb.rollout(pb, 60)
        torch.cuda.synchronize()
        bits = lambda x: x.contiguous().view(torch.int32)
        assert torch.equal(bits(torch.cat([obs, obs2])), bits(o60))
        assert torch.equal(bits(torch.cat([act, act2])), bits(a60))
        assert torch.equal(bits(torch.cat([rew, rew2])), bits(r60))
        assert torch.equal(torch.cat([done, done2]), d60) and bool(d60.any())
        # the buffers are the env's: the next rollout of the same length reuses them
        o3, _, _, _ = ea.rollout(pa, 40)
        assert o3.data_ptr() == obs2.data_ptr()
        # mixing with step(): one trajectory
        ea2, eb2 = make(), make()
        try:
            qa, qb = ea2.make_policy(mlp), eb2.make_policy(mlp)
            xo, xa, _, _ = ea2.rollout(qa, 3)
            yo, ya, _, _ = eb2.rollout(qb, 2)
            so, _, _ = eb2.step(xa[2].clone())
            torch.cuda.synchronize()
            assert torch.equal(bits(xo[2]), bits(so)) and torch.equal(bits(xa[:2]), bits(ya))
            zo, za, _, _ = ea2.rollout(qa, 1)
            wo, wa, _, _ = eb2.rollout(qb, 1)
            torch.cuda.synchronize()
            assert torch.equal(bits(zo), bits(wo)) and torch.equal(bits(za), bits(wa))
        finally:
            ea2.close()
            eb2.close()
        # load_policy from device tensors: the next rollout's first actions are those of the new weights on the last rows
        new = make_mlp(shape, seed=77)
        last = o60[59].clone()
        eb.load_policy(pb, [torch.from_numpy(a).cuda() for Wb in new.layers for a in Wb])
        _, a_new, _, _ = eb.rollout(pb, 2)
        torch.cuda.synchronize()
        ref = new.forward_reference(last.cpu().numpy().astype(np.float64))
        old = mlp.forward_reference(last.cpu().numpy().astype(np.float64))
        err = float(np.abs(a_new[0].cpu().numpy() - ref).max())
        print(f"load_policy from device tensors: max |a - a_f64(new weights)| = {err:.3e}")
        assert err <= FORWARD_BOUND and np.abs(ref - old).max() > 1e-2
        # an nn.Sequential on the device works the same way
        net = torch.nn.Sequential(torch.nn.Linear(20, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                                  torch.nn.Linear(64, 6, bias=False)).cuda()     # (no bias: zeros)
        from gym_dockauv_amd.policy import MLPPolicy
        last = eb._last_rows[:, :20].clone()
        eb.load_policy(pb, net)
        _, a_net, _, _ = eb.rollout(pb, 1)
        torch.cuda.synchronize()
        ref = MLPPolicy.from_torch(net).forward_reference(last.cpu().numpy().astype(np.float64))
        assert float(np.abs(a_net[0].cpu().numpy() - ref).max()) <= FORWARD_BOUND
    finally:
        ea.close()
        eb.close()


def test_errors_on_a_live_handle():
    import torch
    from gym_dockauv_amd import _capi
    lib = _capi.load_library()
    mlp = make_mlp(SHAPES[0], seed=1)
    keep = []

    def rejected(env, d, needle):
        keep.append(d)
        p = C.c_void_p()
        rc = lib.dockauv_policy_create(env._handle, C.byref(d), C.byref(p))
        msg = lib.dockauv_last_error(env._handle)
        assert rc == -1 and not p.value and needle in msg, (rc, msg)

    e64 = env_for(20, 6, 256, precision="f64")
    try:
        rejected(e64, mlp.host_desc(), b"float32")
    finally:
        e64.close()
    env = env_for(20, 6, 256)
    try:
        rejected(env, make_mlp((36, (64, 64), 6, "tanh", "none")).host_desc(), b"n_in")
        rejected(env, make_mlp((20, (64, 64), 3, "tanh", "none")).host_desc(), b"n_out")
        d = mlp.host_desc()
        d.n_hidden[1] = 129
        rejected(env, d, b"n_hidden[1]")
        pol = env.make_policy(mlp)
        rows = torch.zeros((3, 256, 22), device="cuda")
        acts = torch.zeros((3, 256, 6), device="cuda")
        for n in (0, -3):
            rc = lib.dockauv_rollout(env._handle, pol.ptr, rows[0].data_ptr(), rows.data_ptr(), acts.data_ptr(), None, n, 0, 0, None)
            assert rc == -1 and b"n_steps" in lib.dockauv_last_error(env._handle)
        rc = lib.dockauv_rollout(env._handle, pol.ptr, None, rows.data_ptr(), acts.data_ptr(), None, 2, 0, 0, None)
        assert rc == -1 and b"NULL" in lib.dockauv_last_error(env._handle)
        rc = lib.dockauv_policy_forward(env._handle, pol.ptr, None, acts.data_ptr(), 0, 0, None)
        assert rc == -1 and b"NULL" in lib.dockauv_last_error(env._handle)
        # a reload must keep the shapes
        other = make_mlp((20, (64, 32), 6, "tanh", "none"))
        with pytest.raises(_capi.DockAUVError, match="differ from the policy"):
            env.load_policy(pol, other)
        env.load_policy(pol, make_mlp(SHAPES[0], seed=2))     # ... and with them it is taken
        env.rollout_device(pol, rows[0].data_ptr(), rows.data_ptr(), acts.data_ptr(), 3)
        env.synchronize()
    finally:
        env.close()
