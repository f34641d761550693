"""
Policy evaluation with an episode quota per env: the reference's ``predict(gym_env, model_path, n_episodes)`` (train.py:86-118)
and SB3's ``evaluate_policy(model, env, n_eval_episodes, deterministic=True)`` on the device.

A window of K steps over auto-resetting envs counts many short episodes (collisions, out-of-range failures) and few long ones
(time limits, slow dockings) per env, so the episode monitor's rates over a window are length-biased.  SB3's evaluate_policy
counts only the first ``episode_count_targets[i] = (n_eval_episodes + i) // n_envs`` episodes of env i; this module is that rule.

The compute path is the HIP kernels behind ``dockauv_eval_begin`` / ``dockauv_eval_scan`` (include/dockauv.h states their
arithmetic; csrc/dockauv_eval.hip).  This module holds the NumPy statement of those kernels for tests and ports -- never a
compute path, the role ``monitor.episode_scan_reference`` has for the monitor -- and the host objects of an evaluator.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from .monitor import N_STATS, episode_scan_reference, summary_from_stats

NOT_CLASSIFIED = 255      # ep_outcome of a slot no episode reached, or of an episode recorded without terminal observations


def evaluation_targets(n_eval_episodes: int, n_envs: int) -> np.ndarray:
    """SB3's ``episode_count_targets`` (evaluation.py): int32 [n_envs], (n_eval_episodes + i) // n_envs for env i.  They sum to
    n_eval_episodes; with fewer episodes than envs the first n_envs - n_eval_episodes envs get 0."""
    n, N = int(n_eval_episodes), int(n_envs)
    if n < 1 or N < 1:
        raise ValueError("n_eval_episodes and n_envs must be >= 1")
    return ((n + np.arange(N, dtype=np.int64)) // N).astype(np.int32)


def evaluation_state(targets, max_episodes_per_env: int, carry_return=None, carry_length=None) -> dict:
    """NumPy statement of dockauv_eval_begin: ``target`` clamped to [0, S], ``count`` 0, the slots ``ep_return`` float32 /
    ``ep_length`` int32 / ``ep_outcome`` uint8 [S, N] at 0 / 0 / 255, the carries (None: zeros, the handle right after a reset)."""
    S = int(max_episodes_per_env)
    if S < 1:
        raise ValueError("max_episodes_per_env must be >= 1")
    target = np.clip(np.asarray(targets, dtype=np.int64).reshape(-1), 0, S).astype(np.int32)
    N = target.size
    c_ret = np.zeros(N, np.float32) if carry_return is None else np.array(carry_return, dtype=np.float32).reshape(-1)
    c_len = np.zeros(N, np.int32) if carry_length is None else np.array(carry_length, dtype=np.int32).reshape(-1)
    if c_ret.shape != (N,) or c_len.shape != (N,):
        raise ValueError("carry_return, carry_length: [N]")
    return dict(carry_return=c_ret, carry_length=c_len, count=np.zeros(N, np.int32), target=target,
                ep_return=np.zeros((S, N), np.float32), ep_length=np.zeros((S, N), np.int32),
                ep_outcome=np.full((S, N), NOT_CLASSIFIED, np.uint8))


def evaluation_scan_reference(rows_reward, rows_done, state, max_timesteps, terminal_obs=None):
    """NumPy statement of dockauv_eval_scan, defined through ``episode_scan_reference`` so that the per-step rule stays in one
    place.  rows_reward, rows_done: [K, N]; ``state``: the dict of ``evaluation_state`` or of an earlier call (not modified);
    terminal_obs: None or [K, N, n_obs].  Env i's finished episodes, in step order, go to slot [count[i]][i] while count[i] <
    target[i] (outcome 255 without terminal_obs); later ones only move the carries.

    Returns (new state, stats): stats float64 [16] over ALL recorded slots in the layout of dockauv_monitor_io.stats (sums by
    ``math.fsum``), entry 13 the episodes with an outcome, 14 NaN, 15 the episodes still missing, sum (target - count)."""
    d = np.asarray(rows_done) > 0.5
    res = episode_scan_reference(rows_reward, d, state["carry_return"], state["carry_length"], max_timesteps,
                                 terminal_obs=terminal_obs)
    K, N = d.shape
    new = {k: np.array(v) for k, v in state.items()}
    new["carry_return"], new["carry_length"] = res["carry_return"], res["carry_length"]
    S = new["ep_return"].shape[0]
    if new["ep_return"].shape != (S, N) or new["count"].shape != (N,) or new["target"].shape != (N,):
        raise ValueError("state: slots [S, N], count and target [N]")
    for env in range(N):
        room = int(new["target"][env]) - int(new["count"][env])
        for k in np.flatnonzero(d[:, env])[: max(room, 0)]:
            j = int(new["count"][env])
            new["ep_return"][j, env] = res["ep_return"][k, env]
            new["ep_length"][j, env] = res["ep_length"][k, env]
            new["ep_outcome"][j, env] = res["ep_outcome"][k, env] if terminal_obs is not None else NOT_CLASSIFIED
            new["count"][env] = j + 1
    return new, evaluation_stats(new)


def evaluation_stats(state) -> np.ndarray:
    """stats float64 [16] of the recorded slots of ``state`` (see ``evaluation_scan_reference``)"""
    S, N = state["ep_return"].shape
    rec = np.arange(S)[:, None] < state["count"][None, :]
    rets = [float(x) for x in state["ep_return"][rec]]
    lens = state["ep_length"][rec].astype(np.int64)
    out = state["ep_outcome"][rec]
    n = len(rets)
    stats = np.zeros(N_STATS, dtype=np.float64)
    stats[0] = n
    stats[1] = math.fsum(rets)
    stats[2] = math.fsum(x * x for x in rets)
    stats[3] = int(lens.sum())
    stats[4:8] = (min(rets), max(rets), int(lens.min()), int(lens.max())) if n else np.nan
    stats[8:13] = np.bincount(out[out < 5], minlength=5)[:5]
    stats[13] = int((out < 5).sum())
    stats[14] = np.nan
    stats[15] = int((state["target"].astype(np.int64) - state["count"]).sum())
    return stats


class DeviceEvaluator:
    """A dockauv_eval of one BatchedDocking3d handle (made by ``make_evaluator``): carries, counts, targets, slots, workspace."""

    def __init__(self, ptr: C.c_void_p, n_slots: int):
        self.ptr = ptr
        self.n_slots = int(n_slots)


class Evaluator:
    """What ``TorchDocking3d.make_evaluator`` returns.  ``begin`` and ``scan`` queue on the current stream and never
    synchronise; ``missing`` copies 8 bytes and is the one place of the evaluation loop that waits for the device (``episodes``
    and ``summary`` are read-outs for after it and copy to the host too).  ``stats``: the tensor of the latest scan (None before
    the first); ``n_chunks``: the chunks ``TorchDocking3d.evaluate`` last ran on this evaluator."""

    def __init__(self, env, max_episodes_per_env: int):
        self.env = env
        self.handle = env.batch.make_evaluator(max_episodes_per_env)
        self.n_slots = self.handle.n_slots
        self.stats = None
        self.n_chunks = 0
        self._targets = None

    def _stream(self) -> int:
        return self.env.torch.cuda.current_stream().cuda_stream

    def begin(self, targets=None, uniform: int = 1) -> None:
        """A new evaluation at this point of the current stream (dockauv_eval_begin): the carries are re-read from the handle
        (zero right after ``reset``), counts and slots cleared.  ``targets``: per-env quotas, int [N] (array or tensor; clamped
        to [0, max_episodes_per_env] on the device), or None for ``uniform`` episodes from every env."""
        env, torch = self.env, self.env.torch
        if targets is None:
            self._targets = None
            env.batch.evaluator_begin(self.handle, 0, int(uniform), stream=self._stream())
        else:
            t = torch.as_tensor(np.asarray(targets) if not torch.is_tensor(targets) else targets)
            t = t.to(device=env.device, dtype=torch.int32).contiguous()
            if tuple(t.shape) != (env.num_envs,):
                raise ValueError(f"targets must be [{env.num_envs}]")
            self._targets = t        # (read when the launch runs on the stream)
            env.batch.evaluator_begin(self.handle, t.data_ptr(), 0, stream=self._stream())
        self.stats = None

    def scan(self, rows, terminal_obs=None):
        """rows: contiguous float32 [K, N, n_obs + 2] packed rows on the env's device, the steps that follow the ones the
        evaluator has seen; terminal_obs: None or [K, N, n_obs] (outcomes need it).  Queues dockauv_eval_scan and returns a
        fresh ``stats`` float64 [16] device tensor over every episode recorded since ``begin`` (include/dockauv.h:
        dockauv_eval_scan; entry 15: the episodes still missing)."""
        env, torch = self.env, self.env.torch
        N, stride = env.num_envs, env.n_obs + 2

        def ok(t, shape):
            return t.device == env.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape

        if rows.dim() != 3 or rows.shape[0] < 1 or not ok(rows, (rows.shape[0], N, stride)):
            raise ValueError(f"rows must be a contiguous float32 [K, {N}, {stride}] tensor on {env.device}")
        K = int(rows.shape[0])
        if terminal_obs is not None and not ok(terminal_obs, (K, N, env.n_obs)):
            raise ValueError(f"terminal_obs must be a contiguous float32 [{K}, {N}, {env.n_obs}] tensor on {env.device}")
        stats = torch.empty((N_STATS,), device=env.device, dtype=torch.float64)
        env.batch.evaluator_scan_device(self.handle, rows.data_ptr(), K, stats.data_ptr(),
                                        terminal_obs_ptr=0 if terminal_obs is None else terminal_obs.data_ptr(),
                                        stream=self._stream())
        self.stats = stats
        return stats

    def missing(self) -> int:
        """Episodes the quotas still lack after the latest scan (ValueError between ``begin`` and the first scan).  Copies 8 bytes
        to the host and waits for them."""
        if self.stats is None:
            raise ValueError("no scan since begin")
        return int(self.stats[15].item())

    def state(self) -> dict:
        """Views of the evaluator's own device arrays (dockauv_eval_state), valid until the env closes: ``count`` / ``target`` /
        ``carry_length`` int32 [N], ``carry_return`` float32 [N], ``ep_return`` float32 / ``ep_length`` int32 / ``ep_outcome``
        uint8 [S, N]"""
        from .parallel import _DevArray
        env, torch = self.env, self.env.torch
        N, S = env.num_envs, self.n_slots
        ptrs = env.batch.evaluator_state(self.handle)
        spec = dict(count=((N,), "<i4"), target=((N,), "<i4"), ep_return=((S, N), "<f4"), ep_length=((S, N), "<i4"),
                    ep_outcome=((S, N), "|u1"), carry_return=((N,), "<f4"), carry_length=((N,), "<i4"))
        return {k: torch.as_tensor(_DevArray(ptrs[k], shape, typestr), device=env.device) for k, (shape, typestr) in spec.items()}

    def episodes(self):
        """(returns float32, lengths int32, outcomes uint8, counts int32 [N]) of the recorded episodes at this point of the
        current stream: flat tensors in env-major then slot order -- env 0's episodes in the order they finished, then env
        1's --, ``counts`` how many each env has.  Outcome codes: ``monitor.OUTCOMES``; 255 without terminal observations."""
        torch = self.env.torch
        st = self.state()
        counts = st["count"].clone()
        rec = (torch.arange(self.n_slots, device=self.env.device)[None, :] < counts[:, None])     # [N, S]
        return (st["ep_return"].t()[rec], st["ep_length"].t()[rec], st["ep_outcome"].t()[rec], counts)

    def summary(self, stats=None) -> dict:
        """``monitor.summary_from_stats`` of ``stats`` (default: the latest scan's) -- rollout/ep_rew_mean, ep_rew_std,
        rollout/ep_len_mean, n_episodes, the five outcome rates, .. -- plus ``n_missing``.  Copies 128 bytes to the host."""
        stats = self.stats if stats is None else stats
        if stats is None:
            raise ValueError("no scan since begin")
        s = stats.detach().cpu().numpy()
        out = summary_from_stats(s)
        out["n_missing"] = int(s[15])
        return out
