"""
Episode monitor: returns, lengths and outcomes of the episodes that finish inside a collection, and the explained variance of
its values -- what the reference's learner logs through SB3 (``rollout/ep_rew_mean``, ``rollout/ep_len_mean``,
``train/explained_variance``, train.py:64-71) and what debug.py:192-194 forms from the info dict (docking3d.py:388-400).

The compute path is the HIP kernel behind ``dockauv_monitor_scan`` (include/dockauv.h states its arithmetic; csrc/
dockauv_monitor.hip).  This module holds the NumPy statement of that kernel for tests and ports -- never a compute path, the
role ``MLPPolicy.gae_reference`` has for GAE -- and the small host objects of a monitor.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

OUTCOMES = ("goal", "out_of_range", "attitude", "time_limit", "collision")   # codes 0..4 (docking3d.py:608-619)
N_STATS = 16


def episode_scan_reference(rows_reward, rows_done, carry_return, carry_length, max_timesteps, terminal_obs=None):
    """NumPy statement of dockauv_monitor_scan.  rows_reward, rows_done: [K, N] (the reward and done columns of the packed
    rows; done is anything that compares > 0.5 where an episode ended); carry_return float32 [N], carry_length int32 [N]: the
    running return and length of every env's episode before step 0; terminal_obs: None or [K, N, n_obs], the last observation
    where done.  Per env and in step order, in float32 / int32:

        ret = carry_return + reward[k];  len = carry_length + 1
        done[k]: the episode finishes with (ret, len) and the carries restart at 0;  else they become (ret, len)

    The outcome of a finished episode is read off the clipped terminal observation t and the length: bit 0 (goal) t[0] == 0,
    bit 1 (out of range) t[0] == 1, bit 2 (attitude) |t[6]| == 1 or |t[7]| == 1, bit 3 (time limit) len > max_timesteps; the
    code is the lowest set bit, 4 (collision) when none is set.

    Returns a dict: ``carry_return`` / ``carry_length`` (new arrays), ``ep_return`` float32, ``ep_length`` int32,
    ``ep_outcome`` / ``ep_bits`` uint8 [K, N] (zero where not done, and everywhere without terminal_obs) and ``stats`` float64
    [16] in the layout of dockauv_monitor_io.stats (sums by ``math.fsum``; entry 14, the explained variance, NaN: see
    ``explained_variance_reference``)."""
    r = np.asarray(rows_reward, dtype=np.float32)
    d = np.asarray(rows_done) > 0.5
    if r.ndim != 2 or d.shape != r.shape:
        raise ValueError("rows_reward, rows_done: [K, N]")
    K, N = r.shape
    c_ret = np.array(carry_return, dtype=np.float32).reshape(-1)
    c_len = np.array(carry_length, dtype=np.int32).reshape(-1)
    if c_ret.shape != (N,) or c_len.shape != (N,):
        raise ValueError("carry_return, carry_length: [N]")
    t = None
    if terminal_obs is not None:
        t = np.asarray(terminal_obs, dtype=np.float32)
        if t.ndim != 3 or t.shape[:2] != (K, N) or t.shape[2] < 8:
            raise ValueError("terminal_obs: [K, N, n_obs] with n_obs >= 8")
    ep_ret = np.zeros((K, N), dtype=np.float32)
    ep_len = np.zeros((K, N), dtype=np.int32)
    ep_bits = np.zeros((K, N), dtype=np.uint8)
    ep_out = np.zeros((K, N), dtype=np.uint8)
    for k in range(K):
        ret = c_ret + r[k]                      # float32 + float32: one rounding, as the kernel's add
        ln = c_len + np.int32(1)
        dk = d[k]
        ep_ret[k, dk] = ret[dk]
        ep_len[k, dk] = ln[dk]
        if t is not None:
            tk = t[k]
            bits = ((tk[:, 0] == np.float32(0.0)).astype(np.uint8)
                    | ((tk[:, 0] == np.float32(1.0)).astype(np.uint8) << 1)
                    | (((np.abs(tk[:, 6]) == np.float32(1.0)) | (np.abs(tk[:, 7]) == np.float32(1.0))).astype(np.uint8) << 2)
                    | ((ln > int(max_timesteps)).astype(np.uint8) << 3))
            code = np.where(bits & 1, 0, np.where(bits & 2, 1, np.where(bits & 4, 2, np.where(bits & 8, 3, 4)))).astype(np.uint8)
            ep_bits[k, dk] = bits[dk]
            ep_out[k, dk] = code[dk]
        c_ret = np.where(dk, np.float32(0.0), ret).astype(np.float32)
        c_len = np.where(dk, np.int32(0), ln).astype(np.int32)
    stats = np.zeros(N_STATS, dtype=np.float64)
    stats[14] = np.nan
    rets = [float(x) for x in ep_ret[d]]
    lens = ep_len[d].astype(np.int64)
    n = len(rets)
    stats[0] = n
    stats[1] = math.fsum(rets)
    stats[2] = math.fsum(x * x for x in rets)
    stats[3] = int(lens.sum())
    stats[4:8] = (min(rets), max(rets), int(lens.min()), int(lens.max())) if n else np.nan
    if t is not None:
        stats[8:13] = np.bincount(ep_out[d], minlength=5)[:5]
        stats[13] = n
    return dict(carry_return=c_ret, carry_length=c_len, ep_return=ep_ret, ep_length=ep_len, ep_outcome=ep_out, ep_bits=ep_bits,
                stats=stats)


def truncation_slots(n_steps: int, max_timesteps: int) -> int:
    """dockauv_truncation_slots: slots per env that hold every truncated step of ``n_steps`` steps.  A truncated episode has
    exactly max_timesteps + 1 steps and the carry before step 0 is at most max_timesteps, so an env truncates at most
    (n_steps - 1) // (max_timesteps + 1) + 1 times; the bound returned is n_steps // (max_timesteps + 1) + 1, never less."""
    if int(n_steps) < 1 or int(max_timesteps) < 1:
        raise ValueError("n_steps and max_timesteps must be >= 1")
    return int(n_steps) // (int(max_timesteps) + 1) + 1


def truncation_scan_reference(rows_done, carry_length, max_timesteps, terminal_obs, n_slots=None):
    """NumPy statement of dockauv_truncation_scan, defined through ``episode_scan_reference`` so that the rule stays in one place:
    a step is truncated iff its ``ep_outcome`` is 3 -- a time limit with no lower bit set, so a goal reached or an attitude
    limit hit on the last allowed step is terminal.  rows_done [K, N]; carry_length int32 [N] (each at most max_timesteps);
    terminal_obs [K, N, n_obs]; n_slots: None = ``truncation_slots(K, max_timesteps)``.

    Returns a dict: ``truncated`` bool [K, N]; ``trunc_step`` int32 [n_slots, N], env's truncated steps in order, padded with
    -1; ``trunc_row`` int64 [n_slots, N], k * N + env of those steps (the row of terminal_obs), env in unused slots;
    ``carry_length`` int32 [N], the new carry."""
    d = np.asarray(rows_done) > 0.5
    if d.ndim != 2:
        raise ValueError("rows_done: [K, N]")
    K, N = d.shape
    need = truncation_slots(K, max_timesteps)
    n_slots = need if n_slots is None else int(n_slots)
    if n_slots < need:
        raise ValueError(f"n_slots {n_slots} is below truncation_slots = {need}")
    res = episode_scan_reference(np.zeros((K, N), np.float32), d, np.zeros(N, np.float32), carry_length, max_timesteps,
                                 terminal_obs=terminal_obs)
    truncated = d & (res["ep_outcome"] == 3)
    count = truncated.sum(axis=0)
    if np.all(np.asarray(carry_length).reshape(-1) <= int(max_timesteps)):
        assert int(count.max(initial=0)) <= (K - 1) // (int(max_timesteps) + 1) + 1 <= need, "the slot bound does not hold"
    step = np.full((n_slots, N), -1, dtype=np.int32)
    row = np.tile(np.arange(N, dtype=np.int64), (n_slots, 1))
    for env in range(N):
        ks = np.flatnonzero(truncated[:, env])[:n_slots]
        step[: ks.size, env] = ks
        row[: ks.size, env] = ks.astype(np.int64) * N + env
    return dict(truncated=truncated, trunc_step=step, trunc_row=row, carry_length=res["carry_length"])


def explained_variance_reference(values, returns) -> float:
    """SB3's explained_variance on a collection, as dockauv_monitor_scan forms it: y = returns [K, N], e = y - values[:K] (the
    subtraction in float32), 1 - var(e) / var(y) in float64; NaN when var(y) is 0."""
    y32 = np.asarray(returns, dtype=np.float32)
    v32 = np.asarray(values, dtype=np.float32)[: y32.shape[0]]
    if v32.shape != y32.shape:
        raise ValueError("returns: [K, N]; values: [K (+ 1), N]")
    y, e = y32.astype(np.float64).ravel(), (y32 - v32).astype(np.float64).ravel()
    sy = math.fsum((y - math.fsum(y) / y.size) ** 2)
    se = math.fsum((e - math.fsum(e) / e.size) ** 2)
    return float("nan") if sy == 0.0 else 1.0 - se / sy


def summary_from_stats(stats) -> dict:
    """The log entries of one collection from a host copy of ``stats`` [16].  The means run over ALL episodes that finished
    inside the scanned rows (SB3's ep_rew_mean / ep_len_mean average over its last 100 episodes instead); without a finished
    episode they are NaN.  The rates are fractions of the classified episodes (NaN without terminal observations)."""
    s = np.asarray(stats, dtype=np.float64).reshape(-1)
    if s.shape != (N_STATS,):
        raise ValueError(f"stats: [{N_STATS}]")
    n, nc = s[0], s[13]
    nan = float("nan")
    mean = s[1] / n if n > 0 else nan
    var = max(s[2] / n - mean * mean, 0.0) if n > 0 else nan      # (population variance, as np.std of the returns)
    out = {"rollout/ep_rew_mean": float(mean), "rollout/ep_len_mean": float(s[3] / n) if n > 0 else nan,
           "ep_rew_std": float(math.sqrt(var)) if n > 0 else nan, "n_episodes": int(n),
           "ep_rew_min": float(s[4]), "ep_rew_max": float(s[5]), "ep_len_min": float(s[6]), "ep_len_max": float(s[7])}
    for i, name in enumerate(OUTCOMES):
        out[name + "_rate"] = float(s[8 + i] / nc) if nc > 0 else nan
    out["train/explained_variance"] = float(s[14])
    return out


class DeviceMonitor:
    """A dockauv_monitor of one BatchedDocking3d handle (made by ``make_monitor``): the per-env carries and the workspace."""

    def __init__(self, ptr: C.c_void_p):
        self.ptr = ptr


class EpisodeMonitor:
    """What ``TorchDocking3d.make_monitor`` returns.  ``scan`` queues dockauv_monitor_scan on the current stream and never
    synchronises; ``summary`` is the one place that does.  ``stats``: the tensor of the latest scan (None before the first);
    ``seen``: the env's generation counter (bumped by every ``reset``, ``step``, ``rollout`` and ``collect``) at which the carries
    were last right -- ``rollout(..., monitor=m)`` and ``collect(..., monitor=m)`` re-read the carries from the handle when it is
    not the env's current one, so any mix of monitored and unmonitored calls stays right.  Field writes that go to
    ``env.batch`` directly are not counted: call ``sync`` after them."""

    def __init__(self, env):
        self.env = env
        self.handle = env.batch.make_monitor()
        self.seen = env._gen
        self.stats = None

    def sync(self) -> None:
        """The carries <- the handle's cumulative rewards and step counters at this point of the current stream: after steps the
        monitor did not see, ``reset`` or field writes."""
        self.env.batch.monitor_sync(self.handle, stream=self.env.torch.cuda.current_stream().cuda_stream)
        self.seen = self.env._gen

    def scan(self, rows, terminal_obs=None, values=None, returns=None, per_row: bool = False):
        """rows: contiguous float32 [K, N, n_obs + 2] packed rows on the env's device, the steps that follow the ones the carries
        have seen; terminal_obs: None or [K, N, n_obs] (outcomes need it); values [K + 1, N] and returns [K, N] (both or
        neither: explained variance).  Returns a fresh ``stats`` float64 [16] device tensor (include/dockauv.h:
        dockauv_monitor_io.stats); with ``per_row`` (stats, ep_return float32, ep_length int32, ep_outcome uint8 or None
        without terminal_obs), each [K, N], zero-filled before the call and written only where done."""
        env, torch = self.env, self.env.torch
        N, stride = env.num_envs, env.n_obs + 2

        def ok(t, shape):
            return t.device == env.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape

        if rows.dim() != 3 or rows.shape[0] < 1 or not ok(rows, (rows.shape[0], N, stride)):
            raise ValueError(f"rows must be a contiguous float32 [K, {N}, {stride}] tensor on {env.device}")
        K = int(rows.shape[0])
        if terminal_obs is not None and not ok(terminal_obs, (K, N, env.n_obs)):
            raise ValueError(f"terminal_obs must be a contiguous float32 [{K}, {N}, {env.n_obs}] tensor on {env.device}")
        if (values is None) != (returns is None):
            raise ValueError("values and returns: both or neither")
        if values is not None and (not ok(values, (K + 1, N)) or not ok(returns, (K, N))):
            raise ValueError(f"values must be [{K + 1}, {N}] and returns [{K}, {N}], contiguous float32 on {env.device}")
        stats = torch.empty((N_STATS,), device=env.device, dtype=torch.float64)
        ep_ret = ep_len = ep_out = None
        if per_row:
            ep_ret = torch.zeros((K, N), device=env.device, dtype=torch.float32)
            ep_len = torch.zeros((K, N), device=env.device, dtype=torch.int32)
            ep_out = torch.zeros((K, N), device=env.device, dtype=torch.uint8) if terminal_obs is not None else None
        ptr = lambda t: 0 if t is None else t.data_ptr()
        env.batch.monitor_scan_device(self.handle, rows.data_ptr(), K, stats.data_ptr(), terminal_obs_ptr=ptr(terminal_obs),
                                      values_ptr=ptr(values), returns_ptr=ptr(returns), ep_return_ptr=ptr(ep_ret),
                                      ep_length_ptr=ptr(ep_len), ep_outcome_ptr=ptr(ep_out),
                                      stream=torch.cuda.current_stream().cuda_stream)
        self.stats = stats
        return (stats, ep_ret, ep_len, ep_out) if per_row else stats

    def carries(self):
        """(running return float32 [N], running length int32 [N]): copies of the carries at this point of the current stream"""
        torch = self.env.torch
        from .parallel import _DevArray
        r_ptr, l_ptr = self.env.batch.monitor_carry(self.handle)
        N = self.env.num_envs
        return (torch.as_tensor(_DevArray(r_ptr, (N,), "<f4"), device=self.env.device).clone(),
                torch.as_tensor(_DevArray(l_ptr, (N,), "<i4"), device=self.env.device).clone())

    def summary(self, stats=None) -> dict:
        """The log entries of ``stats`` (default: the latest scan's) as a dict of Python numbers: rollout/ep_rew_mean,
        rollout/ep_len_mean, ep_rew_std, n_episodes, ep_rew_min / max, ep_len_min / max, goal_rate, out_of_range_rate,
        attitude_rate, time_limit_rate, collision_rate, train/explained_variance.  Copies 128 bytes to the host: the one place
        of the monitor that synchronises.  Over all episodes that finished inside the collection, not SB3's last 100."""
        stats = self.stats if stats is None else stats
        if stats is None:
            raise ValueError("no scan yet")
        return summary_from_stats(stats.detach().cpu().numpy())
