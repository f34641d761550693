"""
Replay buffer on the device: the ring of transitions (obs, action, reward, next_obs, done) an off-policy learner samples from --
what the reference's ``train()`` gets from SB3 1.5's ``ReplayBuffer.add`` / ``.sample`` with MODEL = SAC or DDPG (train.py;
config/DRL_hyperparams.py: SAC_HYPER_PARAMS_*).

The compute paths are the HIP kernels behind ``dockauv_replay_push`` and ``dockauv_replay_sample`` (include/dockauv.h states the
layout and the index rule; csrc/dockauv_replay.hip).  This module holds the NumPy statements of both for tests and ports --
never a compute path, the role ``MLPPolicy.gae_reference`` has for GAE -- and the host objects of a buffer.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from .policy import _philox4x32_10

REPLAY_STREAM = 4          # word 3 of the Philox counter (0 episode generator, 1 current noise, 2 policy normals, 3 permutation;
                           # 5: the squashed-Gaussian actor's normals on rows, policy.SAC_ROWS_STREAM)
OUTCOME_TIME_LIMIT = 3     # monitor.OUTCOMES.index("time_limit")

# what DeviceReplayBuffer.sample returns: the fields of SB3's ReplayBufferSamples, in its order
ReplaySamples = namedtuple("ReplaySamples", ["observations", "actions", "next_observations", "dones", "rewards"])


def record_floats(n_obs: int, n_u: int) -> int:
    """float32 words of one record [obs | next_obs | action | reward | done | timeout | zero padding]: a multiple of 4"""
    return (2 * int(n_obs) + int(n_u) + 3 + 3) // 4 * 4


def replay_indices_reference(seed: int, draws: int, batch_size: int, n_batches: int, size: int, n_envs: int) -> np.ndarray:
    """The exact statement of the indices dockauv_replay_sample draws: int64 [n_batches, batch_size].  For (g, b):
    (x0, x1, ..) = Philox4x32-10 of counter (b, lo32(draws + g), hi32(draws + g), 4), key = seed; step = (x0 * size) >> 32,
    env = (x1 * n_envs) >> 32, index = step * n_envs + env.  Exact integers throughout."""
    B, G, size, n_envs = int(batch_size), int(n_batches), int(size), int(n_envs)
    if B < 1 or G < 1 or not (1 <= size < 1 << 31) or not (1 <= n_envs < 1 << 31):
        raise ValueError("batch_size, n_batches >= 1; 1 <= size, n_envs < 2^31")
    d = (int(draws) + np.arange(G, dtype=object)) % (1 << 64)
    ctr = np.zeros((G, B, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(B, dtype=np.uint64)[None, :]
    ctr[..., 1] = np.array([int(x) & 0xFFFFFFFF for x in d], dtype=np.uint64)[:, None]
    ctr[..., 2] = np.array([int(x) >> 32 for x in d], dtype=np.uint64)[:, None]
    ctr[..., 3] = REPLAY_STREAM
    x = _philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    step = (x[..., 0] * np.uint64(size)) >> np.uint64(32)
    env = (x[..., 1] * np.uint64(n_envs)) >> np.uint64(32)
    return (step * np.uint64(n_envs) + env).astype(np.int64)


def replay_push_reference(storage, carry, pos, size, rows_in, rows_out, actions, terminal_obs, ep_outcome):
    """NumPy statement of dockauv_replay_push.  storage float32 [capacity_steps, N, record_floats]; carry float32 [N, n_obs];
    rows_in None (the carry) or [N, n_obs + 2]; rows_out [K, N, n_obs + 2]; actions [K, N, n_u]; terminal_obs [K, N, n_obs];
    ep_outcome None or uint8 [K, N].  terminal_obs and ep_outcome are read only where done.  Every value is moved as its 32
    bits.  Returns new (storage, carry, pos, size); the inputs are left alone."""
    st = np.array(storage, dtype=np.float32).view(np.uint32)
    ro = np.ascontiguousarray(rows_out, dtype=np.float32)
    ac = np.ascontiguousarray(actions, dtype=np.float32).view(np.uint32)
    to = np.ascontiguousarray(terminal_obs, dtype=np.float32).view(np.uint32)
    cap, N, R = st.shape
    K, n_obs, n_u = ro.shape[0], ro.shape[2] - 2, ac.shape[2]
    if ro.shape != (K, N, n_obs + 2) or ac.shape != (K, N, n_u) or to.shape != (K, N, n_obs) or R != record_floats(n_obs, n_u):
        raise ValueError("rows_out [K, N, n_obs + 2], actions [K, N, n_u], terminal_obs [K, N, n_obs], storage [.., N, record_floats]")
    if not (1 <= K <= cap) or not (0 <= int(pos) < cap) or not (0 <= int(size) <= cap):
        raise ValueError("1 <= K <= capacity_steps, 0 <= pos < capacity_steps, 0 <= size <= capacity_steps")
    first = (np.ascontiguousarray(carry, dtype=np.float32) if rows_in is None
             else np.ascontiguousarray(rows_in, dtype=np.float32)[:, :n_obs]).view(np.uint32)
    if first.shape != (N, n_obs):
        raise ValueError("carry [N, n_obs] / rows_in [N, n_obs + 2]")
    rw = ro.view(np.uint32)
    one = np.float32(1.0).view(np.uint32)
    o2, o3 = 2 * n_obs, 2 * n_obs + n_u
    for k in range(K):
        done = ro[k, :, n_obs + 1] > np.float32(0.5)
        rec = np.zeros((N, R), dtype=np.uint32)
        rec[:, :n_obs] = first if k == 0 else rw[k - 1, :, :n_obs]
        rec[:, n_obs:o2] = np.where(done[:, None], to[k], rw[k, :, :n_obs])
        rec[:, o2:o3] = ac[k]
        rec[:, o3] = rw[k, :, n_obs]
        rec[:, o3 + 1] = np.where(done, one, np.uint32(0))
        if ep_outcome is not None:
            rec[:, o3 + 2] = np.where(done & (np.asarray(ep_outcome)[k] == OUTCOME_TIME_LIMIT), one, np.uint32(0))
        st[(int(pos) + k) % cap] = rec
    new_carry = rw[K - 1, :, :n_obs].copy().view(np.float32)
    return st.view(np.float32), new_carry, (int(pos) + K) % cap, min(int(size) + K, cap)


class DeviceReplay:
    """A dockauv_replay of one BatchedDocking3d handle (made by ``make_replay``): the ring and the observation carry."""

    def __init__(self, ptr: C.c_void_p):
        self.ptr = ptr


class DeviceReplayBuffer:
    """What ``TorchDocking3d.make_replay_buffer`` returns.  ``rb.rollout(...)``, ``rb.collect(...)`` and
    ``env.step(..., replay=rb)`` store their transitions; ``sample`` draws minibatches.  Nothing here synchronises but
    ``state_dict`` / ``load_state_dict``.

    ``capacity_steps``, ``record_floats``, ``seed``: fixed at create.  ``pos`` (the step slot the next push writes), ``size``
    (step slots filled) and ``draws`` (minibatches drawn: the Philox counter of the next one) are the library's host-side
    counts.  ``storage``: the ring as a [capacity_steps, num_envs, record_floats] tensor over the library's memory, a record
    being [obs | next_obs | action | reward | done | timeout | 0 ..].  ``monitor``: the ``EpisodeMonitor`` whose outcome 3 marks a
    done as a time limit (None with ``handle_timeout_termination=False``: ``dones`` are then the raw dones).  ``seen``: the
    env's generation counter at which the observation carry was last right, as ``EpisodeMonitor.seen``: a call that
    fills the buffer re-reads the carry from the rows it is about to step from when it is not the env's current one, so any mix
    of calls with and without the buffer stays right (the steps in between are simply not stored)."""

    def __init__(self, env, buffer_size: int, seed: int = 0, handle_timeout_termination: bool = True, monitor=None):
        from .parallel import _DevArray
        self.env = env
        if monitor is not None and monitor.env is not env:
            raise ValueError("the monitor belongs to another env")
        if monitor is not None and not handle_timeout_termination:
            raise ValueError("a monitor is only used with handle_timeout_termination")
        self.seed = int(seed)
        self.handle = env.batch.make_replay(buffer_size, seed=self.seed)
        st, _, self.capacity_steps, self.record_floats = env.batch.replay_state(self.handle)
        self.storage = env.torch.as_tensor(_DevArray(st, (self.capacity_steps, env.num_envs, self.record_floats), "<f4"),
                                           device=env.device)
        self.monitor = (monitor if monitor is not None else env.make_monitor()) if handle_timeout_termination else None
        self.seen = None            # (the carry is zeros: the first call reads it from the env's rows)
        self.index = None           # int64 indices of the last sample(..., want_index=True)
        self.last_samples = None    # what the last sample(...) returned: the dense copies of the rows self.index names
        self._sample_bufs = {}

    # ---------------------------------------------------------------------------------------------- counts and state
    @property
    def pos(self) -> int:
        return self.env.batch.replay_counts(self.handle)[0]

    @property
    def size(self) -> int:
        return self.env.batch.replay_counts(self.handle)[1]

    @property
    def draws(self) -> int:
        return self.env.batch.replay_counts(self.handle)[2]

    @property
    def carry(self):
        """The observation carry [num_envs, n_obs] as a tensor over the library's memory.  The library alternates two buffers:
        ask again after every push."""
        from .parallel import _DevArray
        env = self.env
        ptr = env.batch.replay_state(self.handle)[1]
        return env.torch.as_tensor(_DevArray(ptr, (env.num_envs, env.n_obs), "<f4"), device=env.device)

    def _stream(self) -> int:
        return self.env.torch.cuda.current_stream().cuda_stream

    def _ok(self, t, shape, dtype=None) -> bool:
        env = self.env
        return t.device == env.device and t.dtype == (dtype or env.torch.float32) and t.is_contiguous() and tuple(t.shape) == shape

    # ---------------------------------------------------------------------------------------------- filling
    def rollout(self, policy, n_steps: int, stochastic: bool = False, monitor=None):
        """``env.rollout(policy, n_steps, stochastic, want_terminal_obs=True, monitor=monitor)`` that also stores its K
        transitions here: in front of the steps, if the buffer has not seen the env's current generation, the copy of the rows
        the first step reads into the carry; behind them this buffer's monitor's scan and the push.  K at most
        ``capacity_steps``.  Returns what ``env.rollout`` returns; the env's own ``rollout`` keeps its signature and queues
        what it queued."""
        return self.env._rollout(policy, n_steps, stochastic, True, monitor, self)

    def collect(self, policy, value, n_steps: int, gamma: float, gae_lambda: float, stochastic: bool = True, monitor=None,
                bootstrap_truncated: bool = False, reward_norm=None):
        """``env.collect(...)`` with terminal observations that also stores its K transitions (raw rewards) here, as ``rollout``
        does.  Returns the ``Collected`` tuple."""
        return self.env._collect(policy, value, n_steps, gamma, gae_lambda, stochastic, True, monitor, bootstrap_truncated,
                                 reward_norm, self)

    def sync(self, rows) -> None:
        """The carry <- the observation columns of ``rows`` [N, n_obs + 2] (the rows the next step reads), on the current
        stream; ``seen`` <- the env's generation."""
        env = self.env
        if not self._ok(rows, (env.num_envs, env.n_obs + 2)):
            raise ValueError(f"rows must be a contiguous float32 [{env.num_envs}, {env.n_obs + 2}] tensor on {env.device}")
        env.batch.replay_sync_device(self.handle, rows.data_ptr(), stream=self._stream())
        self.seen = env._gen

    def push(self, rows_out, actions, terminal_obs, ep_outcome=None, rows_in=None) -> None:
        """dockauv_replay_push on the current stream: rows_out [K, N, n_obs + 2], actions [K, N, n_u], terminal_obs
        [K, N, n_obs] (read where done), ep_outcome None or uint8 [K, N] (the monitor's per-row outcome), rows_in None (the
        carry) or [N, n_obs + 2].  The env's calls do this themselves; it is public for callers with buffers of their own."""
        env, torch = self.env, self.env.torch
        N, n_obs, n_u = env.num_envs, env.n_obs, env.n_u
        if rows_out.dim() != 3 or not self._ok(rows_out, (rows_out.shape[0], N, n_obs + 2)):
            raise ValueError(f"rows_out must be a contiguous float32 [K, {N}, {n_obs + 2}] tensor on {env.device}")
        K = int(rows_out.shape[0])
        if not self._ok(actions, (K, N, n_u)):
            raise ValueError(f"actions must be a contiguous float32 [{K}, {N}, {n_u}] tensor on {env.device}")
        if terminal_obs is not None and not self._ok(terminal_obs, (K, N, n_obs)):
            raise ValueError(f"terminal_obs must be a contiguous float32 [{K}, {N}, {n_obs}] tensor on {env.device}")
        if ep_outcome is not None and not self._ok(ep_outcome, (K, N), torch.uint8):
            raise ValueError(f"ep_outcome must be a contiguous uint8 [{K}, {N}] tensor on {env.device}")
        if rows_in is not None and not self._ok(rows_in, (N, n_obs + 2)):
            raise ValueError(f"rows_in must be a contiguous float32 [{N}, {n_obs + 2}] tensor on {env.device}")
        ptr = lambda t: 0 if t is None else t.data_ptr()
        env.batch.replay_push_device(self.handle, rows_out.data_ptr(), actions.data_ptr(), ptr(terminal_obs), K,
                                     rows_in_ptr=ptr(rows_in), ep_outcome_ptr=ptr(ep_outcome), stream=self._stream())

    # ---------------------------------------------------------------------------------------------- sampling
    def sample(self, batch_size: int, n_batches: int = 1, want_index: bool = False) -> ReplaySamples:
        """``n_batches`` minibatches of ``batch_size`` stored transitions, uniform with replacement (dockauv_replay_sample on
        the current stream; ``replay_indices_reference`` states the indices).  Returns a ``ReplaySamples`` named tuple
        (observations [B, n_obs], actions [B, n_u], next_observations [B, n_obs], dones [B, 1], rewards [B, 1]), each with a
        leading ``n_batches`` when that is > 1: views of buffers the object owns, reused by the next ``sample`` of the same
        (batch_size, n_batches).  ``dones`` are 0 where the episode ended on its time limit and on nothing else (SB3's
        handle_timeout_termination).  ``want_index``: ``self.index`` holds the int64 indices step * num_envs + env, shaped as
        ``dones`` without the last axis."""
        env, torch = self.env, self.env.torch
        B, G = int(batch_size), int(n_batches)
        if B < 1 or G < 1:
            raise ValueError("batch_size and n_batches must be >= 1")
        bufs = self._sample_bufs.get((B, G))
        if bufs is None:
            z = lambda *shape: torch.zeros(shape, device=env.device, dtype=torch.float32)
            bufs = self._sample_bufs[(B, G)] = dict(obs=z(G, B, env.n_obs), act=z(G, B, env.n_u), nxt=z(G, B, env.n_obs),
                                                    rew=z(G, B, 1), done=z(G, B, 1), idx=None)
        if want_index and bufs["idx"] is None:
            bufs["idx"] = torch.zeros((G, B), device=env.device, dtype=torch.int64)
        idx = bufs["idx"] if want_index else None
        env.batch.replay_sample_device(self.handle, B, G, bufs["obs"].data_ptr(), bufs["act"].data_ptr(), bufs["nxt"].data_ptr(),
                                       bufs["rew"].data_ptr(), bufs["done"].data_ptr(),
                                       index_ptr=0 if idx is None else idx.data_ptr(), stream=self._stream())
        one = (lambda t: t[0]) if G == 1 else (lambda t: t)
        self.index = None if idx is None else one(idx)
        self.last_samples = ReplaySamples(one(bufs["obs"]), one(bufs["act"]), one(bufs["nxt"]), one(bufs["done"]), one(bufs["rew"]))
        return self.last_samples

    # ---------------------------------------------------------------------------------------------- checkpoint
    def state_dict(self) -> dict:
        """Ring, carry, counts and seed.  Waits for the current stream and COPIES THE WHOLE RING (device tensors: move them to
        the host before saving if the device's memory is short)."""
        env = self.env
        env.torch.cuda.current_stream().synchronize()
        pos, size, draws = env.batch.replay_counts(self.handle)
        return dict(storage=self.storage.clone(), carry=self.carry.clone(), pos=pos, size=size, draws=draws, seed=self.seed,
                    capacity_steps=self.capacity_steps, record_floats=self.record_floats)

    def load_state_dict(self, state: dict) -> None:
        """The inverse of ``state_dict`` into a buffer of the same env shape, capacity and seed (the seed is fixed at create:
        ``make_replay_buffer(..., seed=state["seed"])``).  Copies the whole ring and waits for it.  The carry is restored,
        but the next call that fills the buffer re-reads it from the env's rows: the env's own state is not part of the buffer."""
        env = self.env
        if int(state["seed"]) != self.seed:
            raise ValueError(f"the state's seed {state['seed']} is not this buffer's ({self.seed})")
        if int(state["capacity_steps"]) != self.capacity_steps or int(state["record_floats"]) != self.record_floats \
                or tuple(state["storage"].shape) != tuple(self.storage.shape) or tuple(state["carry"].shape) != (env.num_envs, env.n_obs):
            raise ValueError("the state belongs to a buffer of another shape")
        self.storage.copy_(state["storage"].to(env.device))
        self.carry.copy_(state["carry"].to(env.device))
        env.batch.replay_set_counts(self.handle, state["pos"], state["size"], state["draws"])
        env.torch.cuda.current_stream().synchronize()
        self.seen = None
