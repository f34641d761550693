"""
Device-resident env for a learner that lives on the same GPU: actions come in as a CUDA/HIP ``torch.Tensor`` and are
consumed in place, observations / rewards / dones come back as views of one device tensor -- no host copy, no sync
(SURVEY.md section 8f, rank 2).  torch is only the tensor container here: pointers go through the C ABI
(``dockauv_step`` with device pointers on torch's current stream).

The reference's caller is SB3's rollout loop (train.py:64-71): per step ``env.step(a)`` with NumPy arrays on the host.
Here the same loop is::

    env = TorchDocking3d(TRAIN_CONFIG, num_envs=65536, scenario="ObstaclesCurrentDocking3d")
    obs = env.reset()
    for _ in range(n_steps):
        actions = policy(obs)                    # torch, on device
        obs, reward, done = env.step(actions)    # views, valid until the next step()
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import numpy as np

from .. import _capi
from ..config.env_config import BASE_CONFIG
from .batched import BatchedDocking3d


# what TorchDocking3d.sac_gradients returns: three tuples of gradient tensors, then views of buffers the env owns
SacGradients = namedtuple("SacGradients", ["q1", "q2", "actor", "logp", "critic_stats", "actor_stats", "grad_out", "y"])
# what TorchDocking3d.collect returns: views of buffers the env owns
Collected =namedtuple("Collected", ["obs", "actions", "reward", "done", "log_prob", "values", "advantages", "returns"])


class TorchDocking3d:
    def __init__(self, env_config: dict = BASE_CONFIG, num_envs: int = 4096, scenario: str = "SimpleDocking3d",
                 device: int = 0, reset_mode: str = "device", device_seed: int = 0, vehicles=None,
                 double_buffer: bool = True, **kw):
        import torch
        self.torch = torch
        if not torch.cuda.is_available():
            raise RuntimeError("TorchDocking3d needs an MI355X: no HIP device visible (there is no CPU fallback)")
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self.batch = BatchedDocking3d(env_config, num_envs=num_envs, scenario=scenario, device=device, precision="f32",
                                      reset_mode=reset_mode, device_seed=device_seed, rng="batched", vehicles=vehicles,
                                      **kw)
        self.num_envs, self.n_obs, self.n_u = self.batch.num_envs, self.batch.n_observations, self.batch.n_u
        self.observation_space, self.action_space = self.batch.observation_space, self.batch.action_space
        # the kernel writes packed rows [obs | reward | done]; two buffers so that the views handed out by step t
        # stay intact while step t + 1 is being written (a policy may still be reading them)
        n_buf = 2 if double_buffer else 1
        self._packed = [torch.zeros((self.num_envs, self.n_obs + 2), device=self.device, dtype=torch.float32)
                        for _ in range(n_buf)]
        self._terminal = None
        self._i = 0
        # closed loop (rollout): step counter of the trajectory (the exploration noise's counter), the rows the next policy
        # forward reads when they are not in self._packed, buffers per rollout length
        self._t = 0
        self._gen = 0                   # bumped by everything that moves or resets the envs (EpisodeMonitor.seen)
        self._last_rows = None
        self._rollout_bufs = {}
        self._collect_bufs = {}
        self.rollout_terminal_observation = None
        self.evaluator = None           # the Evaluator of the last evaluate(): summary(), episodes(), n_chunks
        # mixed batches built with sort_vehicles=True: row j of every tensor handed in / out belongs to the caller's env
        # perm[j] (kind-sorted on the device, the caller's order within a kind); identity otherwise
        self.perm = torch.as_tensor(self.batch.perm, device=self.device)
        self.vehicles_by_row = None if vehicles is None else [list(vehicles)[int(i)] for i in self.batch.perm]

    def reset(self, seed: Optional[int] = None):
        """All envs: new episodes; returns the reference's reset observation (zeros, docking3d.py:269,322)."""
        self.batch.reset(seed=seed)
        self._gen += 1
        self._last_rows = None
        self._packed[self._i % len(self._packed)].zero_()
        return self._packed[self._i % len(self._packed)][:, : self.n_obs]

    def step(self, actions, want_terminal_obs: bool = False, replay=None):
        """actions: float32 [num_envs, n_u] on this device (contiguous).  Returns (obs, reward, done) views;
        with auto-reset the rows of finished envs already hold the reset observation and, if asked for,
        ``self.terminal_observation`` the last one of the finished episode.
        ``replay`` (``make_replay_buffer``): forces ``want_terminal_obs`` and stores this step's transition as
        ``rb.rollout`` stores its K -- the path of a learner whose actor runs in torch.  ``actions`` are read when the push runs
        on the stream.  Without it not one launch is added or changed."""
        torch = self.torch
        if actions.device != self.device or actions.dtype != torch.float32 or not actions.is_contiguous() \
                or tuple(actions.shape) != (self.num_envs, self.n_u):
            raise ValueError(f"actions must be a contiguous float32 [{self.num_envs}, {self.n_u}] tensor on {self.device}")
        if replay is not None:
            want_terminal_obs = True
            self._replay_before(replay, self._last_rows if self._last_rows is not None else self._packed[self._i % len(self._packed)])
        self._i += 1
        self._t += 1
        self._gen += 1
        self._last_rows = None          # (the rows of this step are the trajectory's last)
        out = self._packed[self._i % len(self._packed)]
        term_ptr = 0
        if want_terminal_obs:
            if self._terminal is None:
                self._terminal = torch.zeros((self.num_envs, self.n_obs), device=self.device, dtype=torch.float32)
            term_ptr = self._terminal.data_ptr()
        self.batch.step_device(actions.data_ptr(), out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream,
                               packed=True, terminal_obs_ptr=term_ptr)
        # the kernels' sticky status word (a tail role that gave up waiting: rows since are invalid) is host-coherent
        # memory: looked at every step without a synchronisation; what it shows belongs to steps that have already run
        self.batch.poll_status()
        if replay is not None:
            self._replay_after(replay, out.unsqueeze(0), actions.unsqueeze(0), self._terminal.unsqueeze(0))
        return out[:, : self.n_obs], out[:, self.n_obs], out[:, self.n_obs + 1] > 0.5

    # ------------------------------------------------------------------------------------------ closed loop
    def make_policy(self, mlp, seed: int = 0):
        """The on-device policy of an ``MLPPolicy`` (gym_dockauv_amd/policy.py) for ``rollout``."""
        return self.batch.make_policy(mlp, seed=seed)

    def make_value(self, mlp):
        """The on-device critic of an ``MLPPolicy`` with one raw output (``MLPPolicy.value_from_torch``) for ``collect``."""
        return self.batch.make_value(mlp)

    # ------------------------------------------------------------------------------------------ SAC: the forward half
    def make_sac_actor(self, mlp_or_module, seed: int = 0):
        """The on-device squashed-Gaussian actor (SAC's) of a ``SquashedGaussianMLP`` or of an SB3-style actor module
        (``latent_pi``, ``mu``, ``log_std``; read through the host once): ``rollout`` / ``rb.rollout`` / ``evaluate`` take it as
        they take a plain actor, ``sac_target`` samples it on minibatch rows.  Widths up to 128 (net_arch=[128, 128] or narrower)."""
        from ..policy import SquashedGaussianMLP
        mlp = mlp_or_module if isinstance(mlp_or_module, SquashedGaussianMLP) else SquashedGaussianMLP.from_torch(mlp_or_module)
        return self.batch.make_sac_actor(mlp, seed=seed)

    def make_q(self, mlp_or_module):
        """An on-device Q critic on [obs | action]: an ``MLPPolicy`` with n_in = n_obs + n_u and one raw output, or an
        ``nn.Sequential`` ending in ``Linear(.., 1)`` (SB3's ``ContinuousCritic.q_networks[i]``)."""
        from ..policy import MLPPolicy
        mlp = mlp_or_module if isinstance(mlp_or_module, MLPPolicy) else MLPPolicy.value_from_torch(mlp_or_module)
        return self.batch.make_q(mlp)

    def _rows_view(self, t, width: int, what: str):
        """(pointer, row stride) of a float32 [n, width] view on this device whose rows are a fixed number of floats apart"""
        torch = self.torch
        if t.device != self.device or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != width or t.stride(1) != 1 \
                or t.stride(0) < width:
            raise ValueError(f"{what} must be a float32 [n, {width}] tensor (or strided view) on {self.device}")
        return t.data_ptr(), int(t.stride(0))

    def _index_ok(self, index) -> int:
        torch = self.torch
        if index.device != self.device or index.dtype != torch.int64 or not index.is_contiguous() or index.numel() < 1:
            raise ValueError(f"index must be a contiguous int64 tensor on {self.device}")
        return int(index.numel())

    def q_values(self, critic, obs, actions, index=None):
        """[B] float32 (a fresh tensor): Q(obs[r], actions[r]) of a ``make_q`` critic on the current stream (dockauv_q_forward),
        r = index[i] (``index`` int64 [B]) or i.  ``obs`` [n, n_obs] and ``actions`` [n, n_u] may be strided views, so the replay
        ring serves as it stands: with R = rb.storage.view(-1, rb.record_floats), ``q_values(q, R[:, :n_obs], R[:, 2 * n_obs:
        2 * n_obs + n_u], rb.index)`` (next_obs: R[:, n_obs:2 * n_obs])."""
        torch = self.torch
        optr, ostride = self._rows_view(obs, self.n_obs, "obs")
        aptr, astride = self._rows_view(actions, self.n_u, "actions")
        if index is None and obs.shape[0] != actions.shape[0]:
            raise ValueError("obs and actions need the same number of rows")
        B = obs.shape[0] if index is None else self._index_ok(index)
        q = torch.empty((B,), device=self.device, dtype=torch.float32)
        self.batch.q_forward_device(critic, optr, aptr, B, q.data_ptr(), obs_stride=ostride, act_stride=astride,
                                    index_ptr=0 if index is None else index.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        return q

    def sac_target(self, actor, q1_target, q2_target, samples_or_buffer, gamma: float, ent_coef=None, log_ent_coef=None, t=None):
        """SB3's ``SAC.train`` target block in ONE host call (dockauv_sac_target: four launches on the current stream, no
        synchronisation): a2, logp2 = actor.sample(next_obs); y = r + gamma (1 - d) (min(Q1', Q2')(next_obs, a2) - alpha logp2).
        ``samples_or_buffer``: the ``ReplaySamples`` of ``rb.sample(...)``, or the ``DeviceReplayBuffer`` itself after
        ``rb.sample(..., want_index=True)`` -- then next_obs, reward, done and timeout are read from the ring through ``rb.index``
        and the sampled copies are not touched: the same bits.  alpha: ``ent_coef`` (a float) or ``log_ent_coef`` (a float32 device
        tensor of one element, read when the kernel runs: no read-back of a learned coefficient).  ``t``: the counter of the
        normals (default: one per call).  Returns y shaped as the sample's rewards, a view of buffers the env owns and reuses for
        the same number of rows; ``self.sac_buffers``: dict(a2 [n, n_u], logp2, q1, q2, y [n]) of this call."""
        torch = self.torch
        if (ent_coef is None) == (log_ent_coef is None):
            raise ValueError("give either ent_coef or log_ent_coef")
        if log_ent_coef is not None and (log_ent_coef.device != self.device or log_ent_coef.dtype != torch.float32 or log_ent_coef.numel() != 1):
            raise ValueError(f"log_ent_coef must be a float32 tensor of one element on {self.device}")
        kw = dict(ent_coef=0.0 if ent_coef is None else float(ent_coef), log_ent_coef_ptr=0 if log_ent_coef is None else log_ent_coef.data_ptr())
        if hasattr(samples_or_buffer, "storage"):
            rb = samples_or_buffer
            if rb.env is not self or rb.index is None:
                raise ValueError("the buffer must be this env's, after rb.sample(..., want_index=True)")
            shape, n = tuple(rb.index.shape) + (1,), self._index_ok(rb.index)
            base, R, o3 = rb.storage.data_ptr(), rb.record_floats, 2 * self.n_obs + self.n_u
            kw.update(next_obs_ptr=base + 4 * self.n_obs, rewards_ptr=base + 4 * o3, dones_ptr=base + 4 * (o3 + 1),
                      timeouts_ptr=(base + 4 * (o3 + 2)) if rb.monitor is not None else 0, next_obs_stride=R, column_stride=R,
                      index_ptr=rb.index.data_ptr())
        else:
            sm = samples_or_buffer
            nxt, rew, done = sm.next_observations, sm.rewards, sm.dones
            for x in (nxt, rew, done):
                if x.device != self.device or x.dtype != torch.float32 or not x.is_contiguous():
                    raise ValueError(f"the samples must be contiguous float32 tensors on {self.device}")
            shape, n = tuple(rew.shape), int(rew.numel())
            if nxt.numel() != n * self.n_obs or done.numel() != n:
                raise ValueError("next_observations [.., n_obs], rewards and dones [.., 1] of one minibatch shape")
            kw.update(next_obs_ptr=nxt.data_ptr(), rewards_ptr=rew.data_ptr(), dones_ptr=done.data_ptr())
        bufs = getattr(self, "_sac_bufs", None)
        if bufs is None:
            bufs = self._sac_bufs = {}
            self._sac_t = 0
        b = bufs.get(n)
        if b is None:
            z = lambda *sh: torch.zeros(sh, device=self.device, dtype=torch.float32)
            b = bufs[n] = dict(a2=z(n, self.n_u), logp2=z(n), q1=z(n), q2=z(n), y=z(n))
        if t is None:
            t, self._sac_t = self._sac_t, self._sac_t + 1
        self.batch.sac_target_device(actor, q1_target, q2_target, n_rows=n, gamma=gamma, a2_ptr=b["a2"].data_ptr(),
                                     logp2_ptr=b["logp2"].data_ptr(), q1_ptr=b["q1"].data_ptr(), q2_ptr=b["q2"].data_ptr(),
                                     y_ptr=b["y"].data_ptr(), t=int(t), stream=torch.cuda.current_stream().cuda_stream, **kw)
        self.sac_buffers = b
        return b["y"].view(shape)

    # ------------------------------------------------------------------------------------------ SAC: the networks' gradients
    def _grad_out_ok(self, t, shape, what: str):
        torch = self.torch
        if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError(f"{what} must be a contiguous float32 {list(shape)} tensor on {self.device}")

    def _grad_arrays(self, shapes, out):
        torch = self.torch
        if out is None:
            return [torch.empty(s, device=self.device, dtype=torch.float32) for s in shapes]
        grads = list(out)
        if len(grads) != len(shapes) or any(g.device != self.device or g.dtype != torch.float32 or not g.is_contiguous()
                                            or tuple(g.shape) != s for g, s in zip(grads, shapes)):
            raise ValueError(f"out must be contiguous float32 tensors of shapes {shapes} on {self.device}")
        return grads

    def sac_actor_heads(self, actor, obs, index=None):
        """[B, 2 n_u] float32 (a fresh tensor): columns 0 .. n_u - 1 are mu, n_u .. 2 n_u - 1 the log-std head BEFORE its clamp
        to [-20, 2], of a ``make_sac_actor`` actor for obs[r], r = index[i] (``index`` int64 [B]) or i: no noise, no tanh
        (dockauv_sac_actor_forward_rows on the current stream).  ``obs`` [n, n_obs] may be a strided view -- the replay ring:
        ``rb.storage.view(-1, rb.record_floats)[:, :n_obs]`` with ``rb.index``."""
        torch = self.torch
        ptr, stride = self._rows_view(obs, self.n_obs, "obs")
        B = obs.shape[0] if index is None else self._index_ok(index)
        out = torch.empty((B, 2 * self.n_u), device=self.device, dtype=torch.float32)
        self.batch.sac_actor_forward_rows_device(actor, ptr, B, out.data_ptr(), row_stride=stride,
                                                 index_ptr=0 if index is None else index.data_ptr(),
                                                 stream=torch.cuda.current_stream().cuda_stream)
        return out

    def sac_actor_backward(self, actor, obs, grad_out, index=None, out=None):
        """The gradients of all weights and biases of the actor for ``grad_out`` [B, 2 n_u] = dL/d(sac_actor_heads(actor, obs,
        index)) (the clamp's mask is the caller's): dockauv_sac_actor_backward on the current stream.  Returns fresh tensors
        (dW1, db1[, dW2, db2], dW_mu, db_mu, dW_ls, db_ls) in torch.nn.Linear layout, or writes into ``out`` (such a sequence)
        and returns it.  Reproducible bit for bit; no gradient with respect to ``obs``."""
        torch = self.torch
        ptr, stride = self._rows_view(obs, self.n_obs, "obs")
        B = obs.shape[0] if index is None else self._index_ok(index)
        self._grad_out_ok(grad_out, (B, 2 * self.n_u), "grad_out")
        widths = [actor.n_in] + actor.n_hidden
        shapes = [s for i in range(len(widths) - 1) for s in ((widths[i + 1], widths[i]), (widths[i + 1],))]
        shapes += [(actor.n_out, widths[-1]), (actor.n_out,)] * 2
        grads = self._grad_arrays(shapes, out)
        ptrs = [g.data_ptr() for g in grads]
        if len(ptrs) == 6:
            ptrs[2:2] = [0, 0]
        self.batch.sac_actor_backward_device(actor, ptr, B, grad_out.data_ptr(), ptrs, row_stride=stride,
                                             index_ptr=0 if index is None else index.data_ptr(),
                                             stream=torch.cuda.current_stream().cuda_stream)
        return tuple(grads)

    def q_backward(self, critic, obs, actions, grad_q, index=None, params=True, grad_actions=False, out=None):
        """A ``make_q`` critic's backward for ``grad_q`` [B] = dL/d(q_values(critic, obs, actions, index)) on the current stream
        (dockauv_q_backward).  Returns (grads, dq_da): ``grads`` = (dW1, db1[, dW2, db2], dW3, db3) with ``params`` (fresh, or
        ``out``), else None; ``dq_da`` [B, n_u] with ``grad_actions`` -- the gradient on the action of position i of the minibatch
        -- else None.  At least one.  ``params=False`` is SAC's actor loss: one launch, no parameter tiles, no workspace, and the
        bits the other form gives.  ``obs`` / ``actions`` may be strided views of the replay ring."""
        torch = self.torch
        if not params and not grad_actions:
            raise ValueError("params and grad_actions are both False: nothing to compute")
        optr, ostride = self._rows_view(obs, self.n_obs, "obs")
        aptr, astride = self._rows_view(actions, self.n_u, "actions")
        if index is None and obs.shape[0] != actions.shape[0]:
            raise ValueError("obs and actions need the same number of rows")
        B = obs.shape[0] if index is None else self._index_ok(index)
        self._grad_out_ok(grad_q, (B,), "grad_q")
        grads = ptrs = None
        if params:
            widths = [critic.n_in] + critic.n_hidden + [1]
            grads = self._grad_arrays([s for i in range(len(widths) - 1) for s in ((widths[i + 1], widths[i]), (widths[i + 1],))], out)
            ptrs = [g.data_ptr() for g in grads]
            if len(ptrs) == 4:
                ptrs[2:2] = [0, 0]
        da = torch.empty((B, self.n_u), device=self.device, dtype=torch.float32) if grad_actions else None
        self.batch.q_backward_device(critic, optr, aptr, B, grad_q.data_ptr(), grad_ptrs=ptrs,
                                     grad_actions_ptr=0 if da is None else da.data_ptr(), obs_stride=ostride, act_stride=astride,
                                     index_ptr=0 if index is None else index.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        return (None if grads is None else tuple(grads)), da

    def sac_actor_apply(self, actor, params, obs, index=None):
        """``sac_actor_heads`` as a differentiable torch operation, in the style of ``mlp_apply``: ``params`` = the learner's
        (W1, b1[, W2, b2], W_mu, b_mu, W_ls, b_ls) device leaves.  They are loaded into ``actor`` on the current stream
        (``load_policy``) and the forward kernel runs; ``.backward()`` runs ``sac_actor_backward`` and hands each parameter its
        gradient.  ``obs`` and ``index`` get none.  mu, log_std = out[:, :n_u], out[:, n_u:].clamp(-20, 2): torch's clamp
        carries the mask."""
        torch = self.torch
        env = self

        class _Apply(torch.autograd.Function):
            @staticmethod
            def forward(ctx, *ps):
                return env.sac_actor_heads(actor, obs, index)

            @staticmethod
            def backward(ctx, grad):
                return env.sac_actor_backward(actor, obs, grad.contiguous(), index)

        params = tuple(params)
        self._load_sac_actor(actor, [p.detach() for p in params])
        return _Apply.apply(*params)

    def q_apply(self, critic, params, obs, actions, index=None):
        """``q_values`` as a differentiable torch operation: [B].  ``params`` = the learner's (W1, b1[, W2, b2], W3, b3) device
        leaves, loaded into ``critic`` on the current stream as ``mlp_apply`` does, each of which gets its gradient; or None --
        the critic's weights stay as loaded and only ``actions`` gets a gradient, through the form without parameter gradients
        (SAC's actor loss: one launch a backward).  ``actions`` gets a gradient only when ``index`` is None (then row i of
        ``actions`` is position i of the minibatch) and it requires one; ``obs`` and ``index`` never do."""
        torch = self.torch
        env = self
        with_params = params is not None
        want_da = index is None and actions.requires_grad
        if not with_params and not want_da:
            raise ValueError("params is None and actions gets no gradient (it needs requires_grad and index=None)")

        class _Apply(torch.autograd.Function):
            @staticmethod
            def forward(ctx, acts, *ps):
                return env.q_values(critic, obs, acts.detach(), index)

            @staticmethod
            def backward(ctx, grad):
                grads, da = env.q_backward(critic, obs, actions.detach(), grad.contiguous(), index, params=with_params,
                                           grad_actions=want_da)
                return (da,) + (tuple(grads) if with_params else ())

        ps = tuple(params) if with_params else ()
        if with_params:
            self.load_policy(critic, [p.detach() for p in ps])
        return _Apply.apply(actions, *ps)

    # ------------------------------------------------------------------------------------------ SAC: the loss head
    def _ent_coef_args(self, ent_coef, log_ent_coef):
        """(ent_coef as a float, device address of log_ent_coef or 0): exactly one of the two is given"""
        torch = self.torch
        if (ent_coef is None) == (log_ent_coef is None):
            raise ValueError("give either ent_coef or log_ent_coef")
        if log_ent_coef is not None and (log_ent_coef.device != self.device or log_ent_coef.dtype != torch.float32 or log_ent_coef.numel() != 1):
            raise ValueError(f"log_ent_coef must be a float32 tensor of one element on {self.device}")
        return (0.0 if ent_coef is None else float(ent_coef)), (0 if log_ent_coef is None else log_ent_coef.data_ptr())

    def sac_sample(self, actor, heads, t: int, row_offset: int = 0):
        """(a [B, n_u], logp [B]) float32, fresh tensors: the squashed-Gaussian actor's sample from ``heads`` [B, 2 n_u]
        (``sac_actor_heads``) with the rows-form normals of counter (row_offset + i, t, j, 5), one launch on the current stream
        (dockauv_sac_sample).  For the same rows, ``t`` and ``row_offset`` these are ``sac_target``'s a2 and logp2 bit for bit; a
        learner gives the actor loss's draw another ``t`` than the target's draw of the same gradient step."""
        torch = self.torch
        B = int(heads.shape[0]) if heads.dim() == 2 else 0
        self._grad_out_ok(heads, (B, 2 * self.n_u), "heads")
        a = torch.empty((B, self.n_u), device=self.device, dtype=torch.float32)
        logp = torch.empty((B,), device=self.device, dtype=torch.float32)
        self.batch.sac_sample_device(actor, heads.data_ptr(), B, a.data_ptr(), logp.data_ptr(), t=int(t), row_offset=int(row_offset),
                                     stream=torch.cuda.current_stream().cuda_stream)
        return a, logp

    def sac_critic_head(self, q1_critic, q1, q2, y):
        """(grad_q1 [B], grad_q2 [B], stats [6]) float32, fresh tensors: SB3's critic_loss = 0.5 (mse(q1, y) + mse(q2, y)) on
        ``q1``, ``q2`` = ``q_values`` of the two critics on the replayed actions and ``y`` = ``sac_target``; grad_q_k = (q_k - y) / B
        is what ``q_backward`` takes; stats = (critic_loss, mse1, mse2, mean q1, mean q2, mean y).  One launch on the current
        stream (dockauv_sac_critic_head); ``q1_critic``: a ``make_q`` critic of this env."""
        torch = self.torch
        B = int(q1.numel())
        for x, what in ((q1, "q1"), (q2, "q2"), (y, "y")):
            self._grad_out_ok(x.view(-1) if x.is_contiguous() else x, (B,), what)
        g1, g2 = (torch.empty((B,), device=self.device, dtype=torch.float32) for _ in range(2))
        stats = torch.empty((6,), device=self.device, dtype=torch.float32)
        self.batch.sac_critic_head_device(q1_critic, q1.data_ptr(), q2.data_ptr(), y.data_ptr(), B, g1.data_ptr(), g2.data_ptr(),
                                          stats.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        return g1, g2, stats

    def sac_actor_head(self, actor, heads, t: int, q1_pi, q2_pi, dq1, dq2, ent_coef=None, log_ent_coef=None, row_offset: int = 0):
        """(grad_out [B, 2 n_u], stats [4]) float32, fresh tensors: SB3's actor_loss = mean(alpha logp - min(q1_pi, q2_pi)) for
        the draw (``t``, ``row_offset``) of ``sac_sample`` on ``heads``.  ``q1_pi``, ``q2_pi`` [B] = ``q_values`` at the sampled
        action; ``dq1``, ``dq2`` [B, n_u] = ``q_backward(.., grad_q=ones, params=False, grad_actions=True)``, pure dq/da.
        grad_out is d actor_loss / d heads with the clamp's mask applied -- what ``sac_actor_backward`` takes; stats =
        (actor_loss, mean logp, mean min q, alpha).  alpha: ``ent_coef`` (a float) or ``log_ent_coef`` (a float32 device tensor of
        one element).  One launch on the current stream (dockauv_sac_actor_head)."""
        torch = self.torch
        ec, lec = self._ent_coef_args(ent_coef, log_ent_coef)
        B = int(heads.shape[0]) if heads.dim() == 2 else 0
        self._grad_out_ok(heads, (B, 2 * self.n_u), "heads")
        for x, shape, what in ((q1_pi, (B,), "q1_pi"), (q2_pi, (B,), "q2_pi"), (dq1, (B, self.n_u), "dq1"), (dq2, (B, self.n_u), "dq2")):
            self._grad_out_ok(x, shape, what)
        grad_out = torch.empty((B, 2 * self.n_u), device=self.device, dtype=torch.float32)
        stats = torch.empty((4,), device=self.device, dtype=torch.float32)
        self.batch.sac_actor_head_device(actor, heads.data_ptr(), q1_pi.data_ptr(), q2_pi.data_ptr(), dq1.data_ptr(), dq2.data_ptr(), B,
                                         grad_out.data_ptr(), stats.data_ptr(), ent_coef=ec, log_ent_coef_ptr=lec, t=int(t),
                                         row_offset=int(row_offset), stream=torch.cuda.current_stream().cuda_stream)
        return grad_out, stats

    def ent_coef_state(self, init: float = 1.0):
        """The learned entropy coefficient's state, a float32 [3] device tensor (log_ent_coef, m, v) = (log(init), 0, 0); SB3's
        ent_coef="auto" is init = 1, "auto_0.1" init = 0.1.  ``state[:1]`` is the ``log_ent_coef`` the other calls take."""
        import math
        if not float(init) > 0.0:
            raise ValueError("init must be > 0")
        return self.torch.tensor([math.log(float(init)), 0.0, 0.0], dtype=self.torch.float32, device=self.device)

    def ent_coef_step(self, state, logp, step: int, lr: float, target_entropy=None, betas=(0.9, 0.999), eps: float = 1e-8, before=None):
        """One Adam step of SB3's ent_coef_loss = -(log_ent_coef * (logp + target_entropy)).mean() on ``state`` (``ent_coef_state``),
        in place, one launch on the current stream (dockauv_sac_ent_coef_step).  ``step``: the caller's count of this step, from 1;
        ``target_entropy``: default -n_u (SB3's "auto"); ``before``: a float32 device tensor of one element that receives
        log_ent_coef as it was -- SB3 evaluates the target and the actor loss at the coefficient from before the step, so that
        is the ``log_ent_coef`` to hand them when the step is queued first.  Returns stats, a fresh float32 [4] = (ent_coef_loss,
        exp(log_ent_coef before), mean(logp + target_entropy), the new log_ent_coef).  Not to be captured in a graph."""
        torch = self.torch
        self._grad_out_ok(state, (3,), "state")
        B = int(logp.numel())
        self._grad_out_ok(logp, (B,), "logp")
        if before is not None and (before.device != self.device or before.dtype != torch.float32 or before.numel() != 1):
            raise ValueError(f"before must be a float32 tensor of one element on {self.device}")
        stats = torch.empty((4,), device=self.device, dtype=torch.float32)
        self.batch.sac_ent_coef_step_device(state.data_ptr(), logp.data_ptr(), B, int(step), float(lr),
                                            float(-self.n_u if target_entropy is None else target_entropy), betas=betas, eps=eps,
                                            before_ptr=0 if before is None else before.data_ptr(), stats_ptr=stats.data_ptr(),
                                            stream=torch.cuda.current_stream().cuda_stream)
        return stats

    def sac_gradients(self, actor, q1, q2, q1_target, q2_target, samples_or_buffer, gamma: float, t: int, ent_coef=None,
                      log_ent_coef=None, out=None):
        """The whole gradient half of one SAC step on the current stream, with no torch arithmetic and no synchronisation:
        every gradient of SB3 1.5's critic loss and actor loss on one minibatch, and the logp ``ent_coef_step`` takes.
        ``samples_or_buffer``: as for ``sac_target`` -- the ``ReplaySamples`` of ``rb.sample(...)``, or the buffer itself after
        ``rb.sample(..., want_index=True)``, then the rows are read from the ring through ``rb.index`` (but for the critics at the sampled action, which
        read the sample's dense observations: the same rows).  Queued in this order:
          1. heads = the actor's two heads on obs                                      1 launch
          2. a, logp = the sample at counter t_pi = 2 t + 1                            1
          3. y = ``sac_target`` at counter 2 t (its own draw on next_obs)              4
          4. q1, q2 on the replayed actions                                            2
          5. the critic head                                                           1
          6. ``q_backward`` of both critics with parameters                            2 x 2
          7. q1_pi, q2_pi at a                                                         2
          8. dq1, dq2: ``q_backward`` without parameters on a cached buffer of ones    2
          9. the actor head                                                            1
         10. ``sac_actor_backward``                                                    2
        20 launches.  All three losses are evaluated at the weights the networks hold at the call.  SB3 steps the critics'
        optimiser before it evaluates q_pi for the actor loss; a learner who wants that order calls the pieces (``sac_target``,
        ``q_values``, ``sac_critic_head``, ``q_backward``, then -- after its critic step and ``load_policy`` -- ``sac_sample``,
        ``sac_actor_head``, ``sac_actor_backward``).  alpha: ``ent_coef`` or ``log_ent_coef`` as for ``sac_target``, used in the
        target and in the actor loss.  ``out``: (q1 grads, q2 grads, actor grads), sequences of tensors to write into (as
        ``q_backward`` / ``sac_actor_backward`` take them); None: fresh tensors.  Returns ``SacGradients(q1, q2, actor, logp,
        critic_stats, actor_stats, grad_out, y)``: the three gradient tuples in torch.nn.Linear layout, logp [B], stats [6] and
        [4] as ``sac_critic_head`` / ``sac_actor_head`` define them, the actor head's grad_out [B, 2 n_u] and the target y [B];
        everything from logp on is a view of buffers the env owns and reuses for the same number of rows."""
        torch = self.torch
        ec, lec = self._ent_coef_args(ent_coef, log_ent_coef)
        n_obs, n_u, st = self.n_obs, self.n_u, torch.cuda.current_stream().cuda_stream
        if hasattr(samples_or_buffer, "storage"):
            rb = samples_or_buffer
            if rb.env is not self or rb.index is None:
                raise ValueError("the buffer must be this env's, after rb.sample(..., want_index=True)")
            n, R, base = self._index_ok(rb.index), rb.record_floats, rb.storage.data_ptr()
            obs_ptr, act_ptr, obs_stride, act_stride, index_ptr = base, base + 4 * 2 * n_obs, R, R, rb.index.data_ptr()
            # (the critics at the sampled action pair a ring row with a dense action row: dockauv_q_forward has one index for
            # both, so those four launches read the sample's dense copy of the same observation rows)
            dense_obs_ptr = rb.last_samples.observations.data_ptr()
        else:
            sm = samples_or_buffer
            for x in (sm.observations, sm.actions):
                if x.device != self.device or x.dtype != torch.float32 or not x.is_contiguous():
                    raise ValueError(f"the samples must be contiguous float32 tensors on {self.device}")
            n = int(sm.rewards.numel())
            if sm.observations.numel() != n * n_obs or sm.actions.numel() != n * n_u:
                raise ValueError("observations [.., n_obs] and actions [.., n_u] of the minibatch's shape")
            obs_ptr, act_ptr, obs_stride, act_stride, index_ptr = sm.observations.data_ptr(), sm.actions.data_ptr(), n_obs, n_u, 0
            dense_obs_ptr = obs_ptr
        ws = getattr(self, "_sac_grad_bufs", None)
        if ws is None:
            ws = self._sac_grad_bufs = {}
        b = ws.get(n)
        if b is None:
            e = lambda *sh: torch.empty(sh, device=self.device, dtype=torch.float32)
            b = ws[n] = dict(heads=e(n, 2 * n_u), a=e(n, n_u), logp=e(n), q1=e(n), q2=e(n), grad_q1=e(n), grad_q2=e(n), q1_pi=e(n),
                             q2_pi=e(n), dq1=e(n, n_u), dq2=e(n, n_u), grad_out=e(n, 2 * n_u), critic_stats=e(6), actor_stats=e(4),
                             ones=torch.ones((n,), device=self.device, dtype=torch.float32))
        p = {k: v.data_ptr() for k, v in b.items()}

        def shapes(net, heads: int):
            widths = [net.n_in] + net.n_hidden
            s = [x for i in range(len(widths) - 1) for x in ((widths[i + 1], widths[i]), (widths[i + 1],))]
            return s + [(net.n_out if heads == 2 else 1, widths[-1]), (net.n_out if heads == 2 else 1,)] * heads

        def eight(grads, net):      # (the device calls take dW2 / db2 = 0 with one hidden layer)
            ptrs = [g.data_ptr() for g in grads]
            if len(net.n_hidden) == 1:
                ptrs[2:2] = [0, 0]
            return ptrs

        out = (None, None, None) if out is None else tuple(out)
        if len(out) != 3:
            raise ValueError("out: (q1 grads, q2 grads, actor grads)")
        g_q1, g_q2 = self._grad_arrays(shapes(q1, 1), out[0]), self._grad_arrays(shapes(q2, 1), out[1])
        g_actor = self._grad_arrays(shapes(actor, 2), out[2])
        bt = self.batch
        bt.sac_actor_forward_rows_device(actor, obs_ptr, n, p["heads"], row_stride=obs_stride, index_ptr=index_ptr, stream=st)
        bt.sac_sample_device(actor, p["heads"], n, p["a"], p["logp"], t=2 * int(t) + 1, stream=st)
        self.sac_target(actor, q1_target, q2_target, samples_or_buffer, gamma, ent_coef=ent_coef, log_ent_coef=log_ent_coef, t=2 * int(t))
        y_ptr = self.sac_buffers["y"].data_ptr()
        for q, key in ((q1, "q1"), (q2, "q2")):
            bt.q_forward_device(q, obs_ptr, act_ptr, n, p[key], obs_stride=obs_stride, act_stride=act_stride, index_ptr=index_ptr, stream=st)
        bt.sac_critic_head_device(q1, p["q1"], p["q2"], y_ptr, n, p["grad_q1"], p["grad_q2"], p["critic_stats"], stream=st)
        for q, key, grads in ((q1, "grad_q1", g_q1), (q2, "grad_q2", g_q2)):
            bt.q_backward_device(q, obs_ptr, act_ptr, n, p[key], grad_ptrs=eight(grads, q), obs_stride=obs_stride, act_stride=act_stride,
                                 index_ptr=index_ptr, stream=st)
        for q, key in ((q1, "q1_pi"), (q2, "q2_pi")):
            bt.q_forward_device(q, dense_obs_ptr, p["a"], n, p[key], stream=st)
        for q, key in ((q1, "dq1"), (q2, "dq2")):
            bt.q_backward_device(q, dense_obs_ptr, p["a"], n, p["ones"], grad_ptrs=None, grad_actions_ptr=p[key], stream=st)
        bt.sac_actor_head_device(actor, p["heads"], p["q1_pi"], p["q2_pi"], p["dq1"], p["dq2"], n, p["grad_out"], p["actor_stats"],
                                 ent_coef=ec, log_ent_coef_ptr=lec, t=2 * int(t) + 1, stream=st)
        bt.sac_actor_backward_device(actor, obs_ptr, n, p["grad_out"], eight(g_actor, actor), row_stride=obs_stride, index_ptr=index_ptr, stream=st)
        return SacGradients(tuple(g_q1), tuple(g_q2), tuple(g_actor), b["logp"], b["critic_stats"], b["actor_stats"], b["grad_out"],
                            self.sac_buffers["y"])

    def _load_sac_actor(self, policy, module_or_tensors) -> None:
        torch = self.torch
        m = module_or_tensors
        if isinstance(m, torch.nn.Module):
            ts = [t for sub in m.latent_pi if isinstance(sub, torch.nn.Linear) for t in (sub.weight, sub.bias)]
            ts += [m.mu.weight, m.mu.bias, m.log_std.weight, m.log_std.bias]
        else:
            ts = list(m)
        ts = [t.detach() for t in ts]
        if len(ts) == 6:
            ts[2:2] = [None, None]
        if len(ts) != 8:
            raise ValueError("expected (W1, b1[, W2, b2], W_mu, b_mu, W_ls, b_ls)")
        widths = [policy.n_in] + policy.n_hidden
        want = [s for i in range(len(widths) - 1) for s in ((widths[i + 1], widths[i]), (widths[i + 1],))]
        if len(policy.n_hidden) == 1:
            want += [None, None]
        want += [(policy.n_out, widths[-1]), (policy.n_out,)] * 2
        for t, w in zip(ts, want):
            if (t is None) != (w is None) or (t is not None and (t.device != self.device or t.dtype != torch.float32
                                                                 or not t.is_contiguous() or tuple(t.shape) != w)):
                raise ValueError(f"actor tensors must be contiguous float32 on {self.device} with shapes {want}")
        self.batch.load_policy(policy, device_ptrs=[0 if t is None else t.data_ptr() for t in ts],
                               stream=torch.cuda.current_stream().cuda_stream)

    def load_policy(self, policy, module_or_tensors, log_std=None) -> None:
        """New weights (an actor's or a critic's) from DEVICE tensors, without a host copy and ordered on the current stream: an ``nn.Sequential`` whose
        Linear layers live on this device, or a sequence (W1, b1[, W2, b2], W3, b3) of contiguous float32 tensors;
        ``log_std``: device tensor [n_u] or None.  The tensors are read when the copy runs on the stream.
        A Q critic (``make_q``) loads as a critic does -- a target network after its Polyak step.  A squashed-Gaussian actor
        (``make_sac_actor``) takes an SB3-style actor module on this device or (W1, b1[, W2, b2], W_mu, b_mu, W_ls, b_ls)."""
        torch = self.torch
        if getattr(policy, "role", None) == "sac":
            if log_std is not None:
                raise ValueError("a squashed-Gaussian actor has a log_std head, not a log_std vector")
            return self._load_sac_actor(policy, module_or_tensors)
        if isinstance(module_or_tensors, torch.nn.Module):
            # a Linear without a bias loads zeros, as MLPPolicy.from_torch does (the allocator keeps the temporary's memory
            # ordered on the current stream, which is the stream the copy runs on)
            ts = [t for m in module_or_tensors if isinstance(m, torch.nn.Linear)
                  for t in (m.weight, m.bias if m.bias is not None else torch.zeros_like(m.weight[:, 0]).contiguous())]
        else:
            ts = list(module_or_tensors)
        ts = [t.detach() for t in ts]
        if len(ts) == 4:
            ts[2:2] = [None, None]
        if len(ts) != 6:
            raise ValueError("expected the weights and biases of two or three Linear layers")
        for t in ts + [log_std]:
            if t is not None and (t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous()):
                raise ValueError(f"policy tensors must be contiguous float32 on {self.device}")
        widths = [policy.n_in] + policy.n_hidden + [policy.n_out]
        got = [t for t in ts if t is not None]
        for i in range(len(widths) - 1):
            if tuple(got[2 * i].shape) != (widths[i + 1], widths[i]) or tuple(got[2 * i + 1].shape) != (widths[i + 1],):
                raise ValueError(f"layer {i}: expected weight [{widths[i + 1]}, {widths[i]}] and bias [{widths[i + 1]}]")
        if log_std is not None and tuple(log_std.shape) != (policy.n_out,):
            raise ValueError(f"log_std must be [{policy.n_out}]")
        self.batch.load_policy(policy, device_ptrs=[0 if t is None else t.data_ptr() for t in ts],
                               log_std_ptr=0 if log_std is None else log_std.detach().data_ptr(),
                               stream=torch.cuda.current_stream().cuda_stream)
        policy.log_std_tensor = log_std       # (mlp_apply reloads the weights with the same log_std)

    def _load_weights(self, policy, tensors) -> None:
        """load_policy with the log_std the policy last got from a device tensor"""
        log_std = getattr(policy, "log_std_tensor", None)
        if policy.has_log_std and log_std is None:
            raise ValueError("the actor's log_std came from host arrays: hand it over as a device tensor once "
                             "(load_policy(policy, params, log_std=...)) so that mlp_apply can keep it")
        self.load_policy(policy, tensors, log_std=log_std)

    def make_monitor(self):
        """An ``EpisodeMonitor`` (gym_dockauv_amd/monitor.py) of this env for ``rollout(..., monitor=m)`` / ``collect(...,
        monitor=m)``: returns, lengths and outcomes of finished episodes and the explained variance, on the device."""
        from ..monitor import EpisodeMonitor
        return EpisodeMonitor(self)

    def make_reward_normalizer(self, gamma: float, clip_reward: float = 10.0, epsilon: float = 1e-8):
        """A ``RewardNormalizer`` (gym_dockauv_amd/normalize.py) of this env for ``collect(..., reward_norm=rn)``: SB3's
        ``VecNormalize(norm_reward=True)`` on the device -- rewards divided by the running standard deviation of the
        discounted return (``gamma``: the learner's) and clipped to +- ``clip_reward``."""
        from ..normalize import RewardNormalizer
        return RewardNormalizer(self, gamma, clip_reward, epsilon)

    def make_evaluator(self, max_episodes_per_env: int):
        """An ``Evaluator`` (gym_dockauv_amd/evaluate.py) of this env for ``evaluate``: an episode quota per env and
        ``max_episodes_per_env`` episode slots per env, on the device."""
        from ..evaluate import Evaluator
        return Evaluator(self, max_episodes_per_env)

    def _monitor_before(self, monitor) -> None:
        """before a monitored call queues its steps: the handle's own counters cover whatever the monitor did not see (``step``,
        ``reset``, unmonitored calls), so its carries are re-read from them unless its last scan ended where the trajectory is"""
        if monitor.env is not self:
            raise ValueError("the monitor belongs to another env")
        if monitor.seen != self._gen:
            monitor.sync()

    def _monitor_after(self, monitor, rows, term, values=None, returns=None) -> None:
        monitor.scan(rows, terminal_obs=term, values=values, returns=returns)
        monitor.seen = self._gen

    def make_replay_buffer(self, buffer_size: int, seed: int = 0, handle_timeout_termination: bool = True, monitor=None):
        """A ``DeviceReplayBuffer`` (gym_dockauv_amd/replay.py) of this env for ``rb.rollout(...)``, ``rb.collect(...)``
        and ``step(..., replay=rb)``: SB3's ``ReplayBuffer(buffer_size, n_envs=num_envs)`` on the device, max(
        buffer_size // num_envs, 1) steps of every env; ``seed``: of its minibatch indices.  ``handle_timeout_termination``
        (SB3's default too): a done that is a time limit and nothing else is sampled as ``dones`` = 0; which dones those are
        comes from ``monitor`` (``make_monitor``; None: one of the buffer's own) through its per-row outcomes."""
        from ..replay import DeviceReplayBuffer
        return DeviceReplayBuffer(self, buffer_size, seed=seed, handle_timeout_termination=handle_timeout_termination, monitor=monitor)

    def _replay_before(self, replay, cur) -> None:
        """before a call with ``replay=`` queues its steps: ``cur`` are the rows the first step's actor reads; they become the
        buffer's observation carry unless its last push ended where the trajectory is"""
        if replay.env is not self:
            raise ValueError("the replay buffer belongs to another env")
        if replay.monitor is not None:
            self._monitor_before(replay.monitor)
        if replay.seen != self._gen:
            replay.sync(cur)

    def _replay_after(self, replay, rows, acts, term, values=None, returns=None) -> None:
        ep_outcome = None
        if replay.monitor is not None:
            ep_outcome = replay.monitor.scan(rows, terminal_obs=term, values=values, returns=returns, per_row=True)[3]
            replay.monitor.seen = self._gen
        replay.push(rows, acts, term, ep_outcome=ep_outcome)
        replay.seen = self._gen

    def rollout(self, policy, n_steps: int, stochastic: bool = False, want_terminal_obs: bool = False, monitor=None):
        """``n_steps`` x (policy, step) queued by ONE host call (dockauv_rollout) on the current stream, starting from the rows
        the env last wrote (``reset``, ``step`` or an earlier ``rollout``: one trajectory).  Returns
        (obs [K, N, n_obs], actions [K, N, n_u], reward [K, N], done [K, N] bool): obs[k] / reward[k] / done[k] are what step k
        returned for actions[k].  Views of buffers the env owns, reused by the next ``rollout`` of the same K; with
        ``want_terminal_obs`` ``self.rollout_terminal_observation`` [K, N, n_obs] holds the last observation where done.
        ``monitor`` (``make_monitor``): forces ``want_terminal_obs`` and queues the episode scan of these K steps behind them on
        the same stream; ``monitor.stats`` holds the result.  Without it no launch is added and none is changed.
        The same call that also stores its K transitions in a replay buffer: ``DeviceReplayBuffer.rollout``."""
        return self._rollout(policy, n_steps, stochastic, want_terminal_obs, monitor, None)

    def _rollout(self, policy, n_steps, stochastic, want_terminal_obs, monitor, replay):
        """``rollout``; ``replay`` (None or a ``DeviceReplayBuffer``: ``rb.rollout``) forces ``want_terminal_obs``; in front of the
        steps, if the buffer has not seen the env's current generation, the copy of the rows the first step reads into its
        carry; behind the steps its monitor's scan and the push of these K transitions (K at most ``replay.capacity_steps``).
        When ``monitor`` is the buffer's own monitor the one scan serves both.  With None not one launch is added or changed."""
        torch = self.torch
        K = int(n_steps)
        if K < 1:
            raise ValueError("n_steps must be >= 1")
        if replay is not None and K > replay.capacity_steps:
            raise ValueError(f"n_steps {K} exceeds the replay buffer's capacity_steps {replay.capacity_steps}")
        if monitor is not None:
            want_terminal_obs = True
            self._monitor_before(monitor)
        if replay is not None:
            want_terminal_obs = True
            self._replay_before(replay, self._last_rows if self._last_rows is not None else self._packed[self._i % len(self._packed)])
        bufs = self._rollout_bufs.get(K)
        if bufs is None:
            bufs = self._rollout_bufs[K] = [torch.zeros((K, self.num_envs, self.n_obs + 2), device=self.device, dtype=torch.float32),
                                            torch.zeros((K, self.num_envs, self.n_u), device=self.device, dtype=torch.float32), None]
        if want_terminal_obs and bufs[2] is None:
            bufs[2] = torch.zeros((K, self.num_envs, self.n_obs), device=self.device, dtype=torch.float32)
        rows, acts, term = bufs
        # the trajectory's last rows: of the last step(), or the last slice of an earlier rollout (also when that is a slice of
        # `rows` itself: the first policy forward has read it before the step kernel that overwrites it starts)
        cur = self._last_rows if self._last_rows is not None else self._packed[self._i % len(self._packed)]
        self.batch.rollout_device(policy, cur.data_ptr(), rows.data_ptr(), acts.data_ptr(), K, t0=self._t, stochastic=stochastic,
                                  stream=torch.cuda.current_stream().cuda_stream,
                                  terminal_obs_ptr=term.data_ptr() if (want_terminal_obs and term is not None) else 0)
        self._t += K
        self._gen += 1
        self._last_rows = rows[K - 1]
        self.rollout_terminal_observation = term if want_terminal_obs else None
        if monitor is not None and not (replay is not None and replay.monitor is monitor):
            self._monitor_after(monitor, rows, term)
        if replay is not None:
            self._replay_after(replay, rows, acts, term)
        return rows[:, :, : self.n_obs], acts, rows[:, :, self.n_obs], rows[:, :, self.n_obs + 1] > 0.5

    def collect(self, policy, value, n_steps: int, gamma: float, gae_lambda: float, stochastic: bool = True,
                want_terminal_obs: bool = False, monitor=None, bootstrap_truncated: bool = False, reward_norm=None):
        """One PPO iteration's collection queued by ONE host call (dockauv_collect) on the current stream: ``rollout`` plus
        log pi(a|s), V(s) of the K + 1 observation sets and GAE.  Continues the trajectory exactly as ``rollout`` does.  Returns
        a ``Collected`` named tuple of views of buffers the env owns (reused by the next ``collect`` of the same K):
        obs [K + 1, N, n_obs] (obs[k], k < K: what the actor saw at step k; obs[K]: the last observation), actions [K, N, n_u],
        reward [K, N], done [K, N] bool (of step k), log_prob [K, N] (None for a policy without log_std or with a tanh output,
        whose log-probability the library does not compute), values [K + 1, N], advantages [K, N], returns [K, N] (None with
        ``value`` None: rollout and log-probabilities only).
        ``monitor`` (``make_monitor``): forces ``want_terminal_obs`` and queues the episode scan of these K steps -- with the
        explained variance of ``values`` / ``returns`` when there is a critic -- behind the collection on the same stream;
        ``monitor.stats`` holds the result.  Without it no launch is added and none is changed.
        ``bootstrap_truncated``: SB3's truncation bootstrap (dockauv_collect_truncated) -- where an episode ends on the time
        limit and on nothing else (the monitor's outcome 3), advantages and returns are those of reward + gamma *
        V(terminal observation) at that step; reward, values and log_prob are what they are without it.  Forces
        ``want_terminal_obs`` and needs a critic; the tuple keeps its fields.  With the default not one launch is added or
        changed.
        ``reward_norm`` (``make_reward_normalizer``): SB3's VecNormalize(norm_reward=True) (dockauv_collect_normalized) -- behind
        the value launches the normaliser's scan of these K steps (``rn.normalized``, ``rn.discounted``, ``rn.step_stats``: its
        outputs, per K; with ``rn.training`` False the statistics are applied and not updated), and ``advantages`` / ``returns``
        are those of the normalised rewards, with ``bootstrap_truncated`` of normalised reward + gamma * V(terminal
        observation).  ``reward`` stays the raw column (the monitor's returns stay sums of raw rewards), values and log_prob are
        what they are without it; the tuple keeps its fields.  Needs a critic and ``rn.gamma == gamma``.  With the default
        not one launch is added or changed.
        The same call that also stores its K transitions in a replay buffer: ``DeviceReplayBuffer.collect``."""
        return self._collect(policy, value, n_steps, gamma, gae_lambda, stochastic, want_terminal_obs, monitor, bootstrap_truncated,
                             reward_norm, None)

    def _collect(self, policy, value, n_steps, gamma, gae_lambda, stochastic, want_terminal_obs, monitor, bootstrap_truncated,
                 reward_norm, replay):
        """``collect``; ``replay`` (None or a ``DeviceReplayBuffer``: ``rb.collect``) stores these K transitions (raw rewards)
        exactly as ``_rollout`` does.  With None not one launch is added or changed."""
        torch = self.torch
        K = int(n_steps)
        if K < 1:
            raise ValueError("n_steps must be >= 1")
        if replay is not None and K > replay.capacity_steps:
            raise ValueError(f"n_steps {K} exceeds the replay buffer's capacity_steps {replay.capacity_steps}")
        if reward_norm is not None:
            if value is None:
                raise ValueError("reward_norm needs a critic: it changes advantages and returns only")
            if reward_norm.env is not self:
                raise ValueError("the reward normaliser belongs to another env")
            if np.float32(reward_norm.gamma) != np.float32(gamma):
                raise ValueError(f"gamma {gamma} is not the reward normaliser's ({reward_norm.gamma})")
        if bootstrap_truncated:
            if value is None:
                raise ValueError("bootstrap_truncated needs a critic: the bootstrap is its value of the terminal observation")
            want_terminal_obs = True
        if monitor is not None:
            want_terminal_obs = True
            self._monitor_before(monitor)
        if replay is not None:
            want_terminal_obs = True
            self._replay_before(replay, self._last_rows if self._last_rows is not None else self._packed[self._i % len(self._packed)])
        N = self.num_envs
        bufs = self._collect_bufs.get(K)
        if bufs is None:
            z = lambda *shape: torch.zeros(shape, device=self.device, dtype=torch.float32)
            bufs = self._collect_bufs[K] = dict(rows=z(K + 1, N, self.n_obs + 2), acts=z(K, N, self.n_u), logp=z(K, N),
                                                values=z(K + 1, N), adv=z(K, N), ret=z(K, N), term=None)
        if want_terminal_obs and bufs["term"] is None:
            bufs["term"] = torch.zeros((K, N, self.n_obs), device=self.device, dtype=torch.float32)
        rows, term = bufs["rows"], bufs["term"] if want_terminal_obs else None
        # rows[0]: a copy of the trajectory's last rows (what the actor reads at step 0), so that obs[0 .. K] is one view
        cur = self._last_rows if self._last_rows is not None else self._packed[self._i % len(self._packed)]
        rows[0].copy_(cur)
        has_v = value is not None
        values, adv, ret = (bufs["values"], bufs["adv"], bufs["ret"]) if has_v else (None, None, None)
        logp = bufs["logp"] if (policy.has_log_std and getattr(policy.shape, "out_act", None) == _capi.ACT_NONE) else None
        ptr = lambda t: 0 if t is None else t.data_ptr()
        common = dict(rows_in_ptr=rows[0].data_ptr(), rows_out_ptr=rows[1].data_ptr(), actions_out_ptr=bufs["acts"].data_ptr(), n_steps=K,
                      gamma=gamma, gae_lambda=gae_lambda, t0=self._t, stochastic=stochastic,
                      stream=torch.cuda.current_stream().cuda_stream, terminal_obs_ptr=ptr(term), log_prob_ptr=ptr(logp),
                      values_ptr=ptr(values), advantages_ptr=ptr(adv), returns_ptr=ptr(ret))
        ws = None
        if bootstrap_truncated:
            ws = bufs.get("trunc")
            if ws is None:      # the four workspaces of dockauv_truncation_io, once per K
                S = self.batch.truncation_slots(K)
                ws = bufs["trunc"] = dict(slots=S, carry=torch.zeros((N,), device=self.device, dtype=torch.int32),
                                          step=torch.zeros((S, N), device=self.device, dtype=torch.int32),
                                          row=torch.zeros((S, N), device=self.device, dtype=torch.int64),
                                          v=torch.zeros((S, N), device=self.device, dtype=torch.float32))
        if reward_norm is not None:
            nws = bufs.get("rewnorm")
            if nws is None:     # the outputs of dockauv_rewnorm_io, once per K
                nws = bufs["rewnorm"] = reward_norm._workspace(K)
            trunc = None if ws is None else dict(n_slots=ws["slots"], length_carry=ws["carry"].data_ptr(),
                                                 trunc_step=ws["step"].data_ptr(), trunc_row=ws["row"].data_ptr(),
                                                 v_terminal=ws["v"].data_ptr())
            self.batch.collect_normalized_device(policy, value, reward_norm.handle, reward_norm_ptr=nws["norm"].data_ptr(),
                                                 discounted_ptr=nws["disc"].data_ptr(), step_stats_ptr=nws["stats"].data_ptr(),
                                                 training=reward_norm.training, trunc=trunc, **common)
            reward_norm._attach(nws)
        elif bootstrap_truncated:
            self.batch.collect_truncated_device(policy, value, n_slots=ws["slots"], length_carry_ptr=ws["carry"].data_ptr(),
                                                trunc_step_ptr=ws["step"].data_ptr(), trunc_row_ptr=ws["row"].data_ptr(),
                                                v_terminal_ptr=ws["v"].data_ptr(), **common)
        else:
            self.batch.collect_device(policy, value, **common)
        self._t += K
        self._gen += 1
        self._last_rows = rows[K]
        self.rollout_terminal_observation = term
        same = replay is not None and monitor is not None and replay.monitor is monitor
        if monitor is not None and not same:
            self._monitor_after(monitor, rows[1:], term, values, ret)
        if replay is not None:
            self._replay_after(replay, rows[1:], bufs["acts"], term, *((values, ret) if same else ()))
        return Collected(rows[:, :, : self.n_obs], bufs["acts"], rows[1:, :, self.n_obs], rows[1:, :, self.n_obs + 1] > 0.5,
                         logp, values, adv, ret)

    def evaluate(self, policy, n_eval_episodes: int, deterministic: bool = True, seed: Optional[int] = None,
                 n_steps: Optional[int] = None, return_episode_rewards: bool = False, evaluator=None):
        """The reference's ``predict`` (train.py:86-118) and SB3's ``evaluate_policy`` in one call: ``reset(seed)``, then chunks of
        ``rollout(policy, K, stochastic=not deterministic, want_terminal_obs=True)`` + the evaluator's scan until every env has
        finished its quota ``evaluation_targets(n_eval_episodes, num_envs)[i]`` of episodes -- SB3's rule, under which short
        episodes (collisions) weigh no more than long ones.  K = ``n_steps``, default min(128, max_timesteps + 1).  One 8-byte
        read per chunk (``Evaluator.missing``) is all that waits for the device.  After a reset every episode ends within
        max_timesteps + 1 steps, so ceil(max(targets) (max_timesteps + 1) / K) chunks always suffice: RuntimeError if episodes
        are still missing after that many.
        Returns (mean_reward, std_reward) over the n_eval_episodes episode returns (np.mean / np.std: the population std, as
        SB3), or with ``return_episode_rewards`` (episode_rewards, episode_lengths), lists in env-major order.  The evaluator
        keeps the details and stays at ``self.evaluator``: ``summary()`` carries the five outcome rates, ``episodes()`` the
        outcomes, ``n_chunks`` the chunks run.  ``evaluator`` (``make_evaluator``, at least max(targets) slots per env); None:
        the last call's when it has slots enough, else a new one."""
        from ..evaluate import evaluation_targets
        targets = evaluation_targets(n_eval_episodes, self.num_envs)
        S = int(targets.max())
        ev = evaluator
        if ev is None:
            ev = self.evaluator if (self.evaluator is not None and self.evaluator.n_slots >= S) else self.make_evaluator(S)
        if ev.env is not self:
            raise ValueError("the evaluator belongs to another env")
        if ev.n_slots < S:
            raise ValueError(f"the evaluator has {ev.n_slots} slots per env, {n_eval_episodes} episodes need {S}")
        self.evaluator = ev
        horizon = int(self.batch.config["max_timesteps"]) + 1
        K = min(128, horizon) if n_steps is None else int(n_steps)
        if K < 1:
            raise ValueError("n_steps must be >= 1")
        self.reset(seed)
        ev.begin(targets)
        max_chunks = -(-S * horizon // K)
        ev.n_chunks = 0
        missing = int(n_eval_episodes)
        while missing and ev.n_chunks < max_chunks:
            self.rollout(policy, K, stochastic=not deterministic, want_terminal_obs=True)
            ev.scan(self._rollout_bufs[K][0], self.rollout_terminal_observation)
            ev.n_chunks += 1
            missing = ev.missing()
        if missing:
            raise RuntimeError(f"{missing} of {n_eval_episodes} episodes are still missing after {ev.n_chunks} chunks of {K} steps: "
                               f"an episode outlived max_timesteps + 1 = {horizon} steps")
        returns, lengths, _, _ = ev.episodes()
        rewards = returns.cpu().numpy().astype(np.float64)
        if return_episode_rewards:
            return rewards.tolist(), lengths.cpu().numpy().tolist()
        return float(np.mean(rewards)), float(np.std(rewards))

    # ------------------------------------------------------------------------------------------ the network's share of the update
    def _mlp_rows(self, policy, rows, index):
        """(pointer to the first packed row, number of rows the call addresses) after validation.  ``rows``: float32 on this device,
        [..., n_obs + 2] packed rows or the [..., n_obs] observation view of such a buffer (``Collected.obs``): last stride 1, the
        leading dimensions one run of rows n_obs + 2 floats apart."""
        torch = self.torch
        stride = self.n_obs + 2
        if rows.device != self.device or rows.dtype != torch.float32 or rows.dim() < 2 or rows.shape[-1] not in (self.n_obs, stride) \
                or policy.n_in != self.n_obs:
            raise ValueError(f"rows must be float32 [..., {stride}] packed rows (or their [..., {self.n_obs}] view) on {self.device}")
        n, expect = 1, stride
        ok = rows.stride(-1) == 1
        for size, st in zip(reversed(rows.shape[:-1]), reversed(rows.stride()[:-1])):
            ok = ok and (size == 1 or st == expect)
            expect *= size
            n *= size
        if not ok or n < 1:
            raise ValueError(f"rows must be a contiguous run of packed rows, {stride} floats apart")
        if index is not None:
            if index.device != self.device or index.dtype != torch.int64 or index.dim() != 1 or not index.is_contiguous() or index.numel() < 1:
                raise ValueError(f"index must be a contiguous int64 [B] tensor on {self.device}")
        return rows.data_ptr(), (n if index is None else int(index.numel()))

    def mlp_forward(self, policy, rows, index=None):
        """[B, n_out]: the output of ``policy`` (an actor or a critic) before its output activation, without noise, for the packed
        ``rows`` (all of them, B = their number) or for rows[index[r]] (``index`` int64 [B], e.g. a slice of torch.randperm):
        dockauv_policy_forward_rows on the current stream.  A fresh tensor."""
        torch = self.torch
        ptr, B = self._mlp_rows(policy, rows, index)
        out = torch.empty((B, policy.n_out), device=self.device, dtype=torch.float32)
        self.batch.policy_forward_rows_device(policy, ptr, B, out.data_ptr(), index_ptr=0 if index is None else index.data_ptr(),
                                              stream=torch.cuda.current_stream().cuda_stream)
        return out

    def mlp_backward(self, policy, rows, grad_out, index=None, out=None):
        """The gradients of all weights and biases of ``policy`` for ``grad_out`` [B, n_out] = dL/d(mlp_forward(policy, rows,
        index)): dockauv_policy_backward on the current stream.  Returns fresh tensors (dW1, db1[, dW2, db2], dW3, db3) in
        torch.nn.Linear layout, or -- ``out``: such a sequence of contiguous float32 device tensors -- writes into those and
        returns them.  Reproducible bit for bit; no gradient with respect to the rows."""
        torch = self.torch
        ptr, B = self._mlp_rows(policy, rows, index)
        if grad_out.device != self.device or grad_out.dtype != torch.float32 or not grad_out.is_contiguous() \
                or tuple(grad_out.shape) != (B, policy.n_out):
            raise ValueError(f"grad_out must be a contiguous float32 [{B}, {policy.n_out}] tensor on {self.device}")
        widths = [policy.n_in] + policy.n_hidden + [policy.n_out]
        shapes = [s for i in range(len(widths) - 1) for s in ((widths[i + 1], widths[i]), (widths[i + 1],))]
        if out is None:
            grads = [torch.empty(s, device=self.device, dtype=torch.float32) for s in shapes]
        else:
            grads = list(out)
            if len(grads) != len(shapes) or any(g.device != self.device or g.dtype != torch.float32 or not g.is_contiguous()
                                                or tuple(g.shape) != s for g, s in zip(grads, shapes)):
                raise ValueError(f"out must be contiguous float32 tensors of shapes {shapes} on {self.device}")
        ptrs = [g.data_ptr() for g in grads]
        if len(ptrs) == 4:
            ptrs[2:2] = [0, 0]
        self.batch.policy_backward_device(policy, ptr, B, grad_out.data_ptr(), ptrs, index_ptr=0 if index is None else index.data_ptr(),
                                          stream=torch.cuda.current_stream().cuda_stream)
        return tuple(grads)

    def mlp_apply(self, policy, params, rows, index=None):
        """``mlp_forward`` as a differentiable torch operation: ``params`` = the learner's (W1, b1[, W2, b2], W3, b3) device
        tensors (leaves that require grad, e.g. ``list(net.parameters())`` of an nn.Sequential of Linear layers).  They are
        loaded into ``policy`` on the current stream (``load_policy``, with the log_std device tensor of the last ``load_policy``) and the forward
        kernel runs; ``.backward()`` runs the backward kernel and hands each parameter its gradient.  ``rows`` and ``index``
        get none."""
        torch = self.torch
        env = self

        class _Apply(torch.autograd.Function):
            @staticmethod
            def forward(ctx, *ps):
                return env.mlp_forward(policy, rows, index)

            @staticmethod
            def backward(ctx, grad):
                return env.mlp_backward(policy, rows, grad.contiguous(), index)

        params = tuple(params)
        self._load_weights(policy, [p.detach() for p in params])
        return _Apply.apply(*params)

    # ------------------------------------------------------------------------------------------ the PPO head
    def ppo_head(self, policy, mean, v, actions, log_prob_old, advantages, returns, index=None, *, clip_range: float,
                 vf_coef: float, ent_coef: float, normalize_advantage: bool = True):
        """The PPO head on one minibatch (dockauv_ppo_head on the current stream; ``policy`` is the actor, whose log_std the
        kernel reads): ``mean`` [B, n_u] and ``v`` [B] (None: no critic) are ``mlp_forward`` of the actor and the critic;
        ``actions`` [M, n_u], ``log_prob_old`` / ``advantages`` / ``returns`` [M] are the collection's arrays, read at
        ``index`` (int64 [B], the one the forward took; None: M == B, in order).  Returns fresh tensors (grad_mean [B, n_u],
        grad_v [B] or None, grad_log_std [n_u], stats [8]): the gradients of SB3's PPO loss on the two network outputs and on
        log_std, and (loss, policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction, advantage mean, advantage std).
        Reproducible bit for bit; does not synchronise."""
        torch = self.torch
        ok = lambda t, shape: t.device == self.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
        if mean.dim() != 2 or not ok(mean, (mean.shape[0], policy.n_out)) or mean.shape[0] < 1:
            raise ValueError(f"mean must be a contiguous float32 [B, {policy.n_out}] tensor on {self.device}")
        B = int(mean.shape[0])
        if v is not None and not ok(v, (B,)):
            raise ValueError(f"v must be a contiguous float32 [{B}] tensor on {self.device} (or None)")
        if index is not None:
            if index.device != self.device or index.dtype != torch.int64 or not index.is_contiguous() or tuple(index.shape) != (B,):
                raise ValueError(f"index must be a contiguous int64 [{B}] tensor on {self.device}")
        M = B if index is None else (int(actions.shape[0]) if actions.dim() == 2 else -1)
        if not ok(actions, (M, policy.n_out)):
            raise ValueError(f"actions must be a contiguous float32 [M, {policy.n_out}] tensor on {self.device} (M = {B} without an index)")
        for name, t in (("log_prob_old", log_prob_old), ("advantages", advantages)) + ((("returns", returns),) if v is not None else ()):
            if not ok(t, (M,)):
                raise ValueError(f"{name} must be a contiguous float32 [{M}] tensor on {self.device}")
        if normalize_advantage and B < 2:
            raise ValueError("normalize_advantage needs at least two rows")
        new = lambda *shape: torch.empty(shape, device=self.device, dtype=torch.float32)
        grad_mean, grad_v, grad_log_std, stats = new(B, policy.n_out), (new(B) if v is not None else None), new(policy.n_out), new(8)
        self.batch.ppo_head_device(policy, B, mean.data_ptr(), 0 if v is None else v.data_ptr(), actions.data_ptr(),
                                   log_prob_old.data_ptr(), advantages.data_ptr(), 0 if v is None else returns.data_ptr(),
                                   grad_mean.data_ptr(), 0 if v is None else grad_v.data_ptr(), grad_log_std.data_ptr(),
                                   stats.data_ptr(), clip_range, vf_coef, ent_coef, normalize_advantage=normalize_advantage,
                                   index_ptr=0 if index is None else index.data_ptr(),
                                   stream=torch.cuda.current_stream().cuda_stream)
        return grad_mean, grad_v, grad_log_std, stats

    def ppo_minibatch(self, policy, value, actor_params, log_std, critic_params, actions, log_prob_old, advantages, returns,
                      rows, index, **head_args):
        """One PPO minibatch step without autograd, up to the optimiser: the weights of ``actor_params`` / ``critic_params``
        (the learner's (W1, b1[, W2, b2], W3, b3) device tensors) and ``log_std`` are loaded into ``policy`` / ``value`` on the
        current stream as ``mlp_apply`` does, then ``mlp_forward`` of both on rows[index], ``ppo_head`` (``head_args``:
        clip_range, vf_coef, ent_coef[, normalize_advantage]) and ``mlp_backward`` of both.  Every parameter's and log_std's
        ``.grad`` is set to its gradient (what was there is replaced, not added to).  Returns ``stats`` [8] as ``ppo_head``
        does, on the device, without a synchronisation; ``clip_grad_norm_`` and ``opt.step()`` stay with the caller."""
        actor_params, critic_params = list(actor_params), list(critic_params)
        self.load_policy(policy, [p.detach() for p in actor_params], log_std=log_std.detach())
        self.load_policy(value, [p.detach() for p in critic_params])
        mean = self.mlp_forward(policy, rows, index)
        v = self.mlp_forward(value, rows, index).view(-1)
        grad_mean, grad_v, grad_log_std, stats = self.ppo_head(policy, mean, v, actions, log_prob_old, advantages, returns, index,
                                                               **head_args)
        for p, g in zip(actor_params, self.mlp_backward(policy, rows, grad_mean, index)):
            p.grad = g
        for p, g in zip(critic_params, self.mlp_backward(value, rows, grad_v.view(-1, 1), index)):
            p.grad = g
        log_std.grad = grad_log_std
        return stats

    # ------------------------------------------------------------------------------------------ the optimiser and the whole update
    def make_optimizer(self, policy, value, actor_params, log_std, critic_params, betas=(0.9, 0.999), eps: float = 1e-5,
                       max_grad_norm: float = 0.5):
        """Adam with gradient-norm clipping on the device (dockauv_optim_*) for the learner's own tensors: ``actor_params`` /
        ``critic_params`` = (W1, b1[, W2, b2], W3, b3) and ``log_std``, contiguous float32 tensors on this device (e.g.
        ``list(net.parameters())``) of the shapes of ``policy`` / ``value``.  The returned ``DeviceAdam`` keeps references to
        them and updates them IN PLACE (an ``nn.Sequential`` that holds them sees the new weights); it owns gradient buffers of
        the same shapes (``opt.grads``).  ``value=None`` together with ``critic_params=None``: actor only.  Defaults: SB3's PPO
        (Adam with eps 1e-5, max_grad_norm 0.5; ``max_grad_norm`` <= 0: no clipping)."""
        return DeviceAdam(self, policy, value, actor_params, log_std, critic_params, betas, eps, max_grad_norm)

    def ppo_update(self, opt, collected, n_epochs: int, batch_size: int, lr: float, *, clip_range: float, vf_coef: float,
                   ent_coef: float, normalize_advantage: bool = True, generator=None):
        """SB3's PPO.train loop on one ``Collected`` (of ``collect`` with the optimiser's actor and critic), queued on the
        current stream without a host synchronisation: per epoch one ``torch.randperm(K * N, device=..., generator=generator)``
        split into minibatches of ``batch_size`` rows (the last may be shorter, as in SB3; refused when it would have one row
        and ``normalize_advantage`` is on); per minibatch ``mlp_forward`` of both networks, the PPO head, ``mlp_backward`` of
        both into ``opt.grads`` and ``opt.step(lr)``.  The weights are loaded once at the start from the optimiser's tensors
        (so the call is right even when the caller changed them in between); inside the loop the optimiser's repack is the load,
        and after the call both networks hold the last step's weights: the next ``collect`` needs no ``load_policy``.  Returns
        stats [n_epochs, n_minibatches, 10] on the device: the head's eight (``ppo_head``), the gradient norm before clipping
        and the clipping coefficient.  SB3's ``target_kl`` early stop needs the host and is left to the caller, who can run
        ``n_epochs=1`` per call and look at column 4 (approx_kl) in between."""
        torch = self.torch
        c, policy, value = collected, opt.policy, opt.value
        n_epochs, batch_size = int(n_epochs), int(batch_size)
        if n_epochs < 1 or batch_size < 1:
            raise ValueError("n_epochs and batch_size must be >= 1")
        if c.log_prob is None or (value is not None and (c.advantages is None or c.returns is None)) or c.advantages is None:
            raise ValueError("collected must hold log_prob and advantages (and returns with a critic): collect() with a critic")
        K, N = int(c.actions.shape[0]), int(c.actions.shape[1])
        M = K * N
        n_mb = (M + batch_size - 1) // batch_size
        if normalize_advantage and M - (n_mb - 1) * batch_size == 1:
            raise ValueError(f"the last minibatch of {M} rows in batches of {batch_size} would have one row: advantage "
                             "normalisation needs two (another batch_size, or normalize_advantage=False)")
        rows = c.obs[:K]
        row_ptr, n_rows = self._mlp_rows(policy, rows, None)
        if n_rows != M:
            raise ValueError("collected.obs must be [K + 1, N, n_obs] for actions [K, N, n_u]")
        flat = {}
        for name, t, tail in (("actions", c.actions, (policy.n_out,)), ("log_prob", c.log_prob, ()), ("advantages", c.advantages, ()),
                              ("returns", c.returns, ())):
            if t is None:
                flat[name] = None
                continue
            if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (K, N) + tail:
                raise ValueError(f"collected.{name} must be a contiguous float32 {(K, N) + tail} tensor on {self.device}")
            flat[name] = t.view((M,) + tail)
        stream = torch.cuda.current_stream().cuda_stream
        opt.load()
        stats = torch.zeros((n_epochs, n_mb, 10), device=self.device, dtype=torch.float32)
        for e in range(n_epochs):
            perm = torch.randperm(M, device=self.device, generator=generator)
            for j, idx in enumerate(perm.split(batch_size)):
                B = int(idx.numel())
                mean = self.mlp_forward(policy, rows, idx)
                v = self.mlp_forward(value, rows, idx).view(-1) if value is not None else None
                grad_mean = torch.empty((B, policy.n_out), device=self.device, dtype=torch.float32)
                grad_v = torch.empty((B,), device=self.device, dtype=torch.float32) if v is not None else None
                st = stats[e, j]
                self.batch.ppo_head_device(policy, B, mean.data_ptr(), 0 if v is None else v.data_ptr(), flat["actions"].data_ptr(),
                                           flat["log_prob"].data_ptr(), flat["advantages"].data_ptr(),
                                           0 if v is None else flat["returns"].data_ptr(), grad_mean.data_ptr(),
                                           0 if v is None else grad_v.data_ptr(), opt.grad_log_std.data_ptr(), st.data_ptr(),
                                           clip_range, vf_coef, ent_coef, normalize_advantage=normalize_advantage,
                                           index_ptr=idx.data_ptr(), stream=stream)
                self.mlp_backward(policy, rows, grad_mean, idx, out=opt.actor_grads)
                if value is not None:
                    self.mlp_backward(value, rows, grad_v.view(-1, 1), idx, out=opt.critic_grads)
                opt.step(lr, stats=st[8:])
        return stats

    def permutation(self, seed: int, epoch: int, n: int):
        """A fresh int64 [n] device tensor: the keyed permutation P_{seed, epoch} of 0 .. n - 1 (dockauv_permutation on the
        current stream; ``MLPPolicy.permutation_reference`` states it exactly).  The shuffle of ``ppo_train``."""
        torch = self.torch
        n = int(n)
        if n < 1 or n > 1 << 31:
            raise ValueError("n must be in 1 .. 2^31")
        out = torch.empty((n,), device=self.device, dtype=torch.int64)
        self.batch.permutation_device(seed, epoch, n, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        return out

    def ppo_train(self, opt, collected, n_epochs: int, batch_size: int, lr: float, *, clip_range: float, vf_coef: float,
                  ent_coef: float, normalize_advantage: bool = True, clip_range_vf=None, target_kl=None, seed: int = 0,
                  first_epoch: int = 0):
        """``ppo_update`` queued by ONE host call (dockauv_ppo_update on the current stream), with the two hyper-parameters
        that one leaves out.  Minibatch j of epoch e is ``permutation(seed, first_epoch + e, K * N)[j * batch_size : ...]``
        (pass a ``first_epoch`` that advances by ``n_epochs`` per call); per minibatch the library queues what ``ppo_update``
        queues -- both forwards, the head, both backwards into ``opt.grads``, the optimiser step with its repack -- on its own
        scratch: no torch allocation, no host synchronisation.  ``clip_range_vf`` (None / 0: off) clips the value to
        ``collected.values`` +- clip_range_vf as SB3 does.  ``target_kl`` (None / 0: off): the first minibatch whose approx_kl
        exceeds 1.5 target_kl is not applied and neither is any after it (SB3's early stop, decided on the device); the
        remaining minibatches still run on the frozen weights, and ``opt.steps()`` afterwards waits for the update and reads
        how many were applied.  The weights are loaded once at the start from the optimiser's tensors, as in ``ppo_update``.
        Returns stats [n_epochs, n_minibatches, 12] on the device: the head's eight, the gradient norm before clipping and
        the clipping coefficient, applied (1 / 0), the Adam step number; columns 8..11 are 0 where nothing was applied."""
        torch = self.torch
        c, policy, value = collected, opt.policy, opt.value
        n_epochs, batch_size = int(n_epochs), int(batch_size)
        if n_epochs < 1 or batch_size < 1:
            raise ValueError("n_epochs and batch_size must be >= 1")
        if c.log_prob is None or (value is not None and (c.advantages is None or c.returns is None)) or c.advantages is None:
            raise ValueError("collected must hold log_prob and advantages (and returns with a critic): collect() with a critic")
        clip_range_vf, target_kl = float(clip_range_vf or 0.0), float(target_kl or 0.0)
        if clip_range_vf < 0.0 or target_kl < 0.0:
            raise ValueError("clip_range_vf and target_kl must be >= 0 (None or 0: off)")
        if clip_range_vf > 0.0 and (value is None or c.values is None):
            raise ValueError("clip_range_vf needs a critic and collected.values")
        K, N = int(c.actions.shape[0]), int(c.actions.shape[1])
        M = K * N
        n_mb = (M + batch_size - 1) // batch_size
        if normalize_advantage and M - (n_mb - 1) * batch_size == 1:
            raise ValueError(f"the last minibatch of {M} rows in batches of {batch_size} would have one row: advantage "
                             "normalisation needs two (another batch_size, or normalize_advantage=False)")
        row_ptr, n_rows = self._mlp_rows(policy, c.obs[:K], None)
        if n_rows != M:
            raise ValueError("collected.obs must be [K + 1, N, n_obs] for actions [K, N, n_u]")
        ptr = {}
        for name, t, tail in (("actions", c.actions, (policy.n_out,)), ("log_prob", c.log_prob, ()), ("advantages", c.advantages, ()),
                              ("returns", c.returns, ())):
            if t is None:
                ptr[name] = 0
                continue
            if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (K, N) + tail:
                raise ValueError(f"collected.{name} must be a contiguous float32 {(K, N) + tail} tensor on {self.device}")
            ptr[name] = t.data_ptr()
        ptr["values"] = 0
        if clip_range_vf > 0.0:
            t = c.values
            if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (K + 1, N):
                raise ValueError(f"collected.values must be a contiguous float32 {(K + 1, N)} tensor on {self.device}")
            ptr["values"] = t.data_ptr()
        opt.load()
        stats = torch.zeros((n_epochs, n_mb, 12), device=self.device, dtype=torch.float32)
        self.batch.ppo_update_device(opt.handle, row_ptr, M, batch_size, n_epochs, lr, ptr["actions"], ptr["log_prob"],
                                     ptr["advantages"], ptr["returns"] if value is not None else 0, stats.data_ptr(),
                                     opt._six(opt.actor_params), opt.log_std.data_ptr(), opt._six(opt.actor_grads),
                                     opt.grad_log_std.data_ptr(),
                                     None if value is None else opt._six(opt.critic_params),
                                     None if value is None else opt._six(opt.critic_grads),
                                     clip_range=clip_range, vf_coef=vf_coef, ent_coef=ent_coef,
                                     normalize_advantage=normalize_advantage, clip_range_vf=clip_range_vf,
                                     values_old_ptr=ptr["values"], target_kl=target_kl, seed=seed, first_epoch=first_epoch,
                                     stream=torch.cuda.current_stream().cuda_stream)
        return stats

    @property
    def terminal_observation(self):
        return self._terminal

    def close(self) -> None:
        """Raises DockAUVError (after releasing everything) if a step kernel of this env reported an internal time-out."""
        err = None
        try:
            if getattr(self.batch, "_handle", None) is not None and self.batch._handle.value:
                self.batch.synchronize()
        except Exception as e:
            err = e
        self.batch.close()
        if err is not None:
            raise err


class DeviceAdam:
    """What ``TorchDocking3d.make_optimizer`` returns: the device optimiser (dockauv_optim) of one actor, its log_std and
    (optionally) one critic, over the caller's own tensors.  ``actor_params`` / ``log_std`` / ``critic_params``: the caller's
    tensors (updated in place by ``step``); ``actor_grads`` / ``grad_log_std`` / ``critic_grads``: gradient buffers of the same
    shapes the optimiser owns, ``grads`` all of them in the optimiser's order (actor, log_std, critic), ``params`` likewise."""

    def __init__(self, env, policy, value, actor_params, log_std, critic_params, betas, eps, max_grad_norm):
        torch = env.torch
        if (value is None) != (critic_params is None):
            raise ValueError("value and critic_params: both or neither (None: actor only)")
        if log_std is None:
            raise ValueError("the optimiser needs the actor's log_std tensor")

        def checked(pol, tensors, what):
            ts = [t.detach() for t in tensors]
            widths = [pol.n_in] + pol.n_hidden + [pol.n_out]
            shapes = [s for i in range(len(widths) - 1) for s in ((widths[i + 1], widths[i]), (widths[i + 1],))]
            if len(ts) != len(shapes) or any(t.device != env.device or t.dtype != torch.float32 or not t.is_contiguous()
                                             or tuple(t.shape) != s for t, s in zip(ts, shapes)):
                raise ValueError(f"{what} must be contiguous float32 tensors of shapes {shapes} on {env.device}")
            return ts

        self.env, self.policy, self.value = env, policy, value
        self.actor_params = checked(policy, actor_params, "actor_params")
        self.critic_params = checked(value, critic_params, "critic_params") if value is not None else None
        self.log_std = log_std.detach()
        if self.log_std.device != env.device or self.log_std.dtype != torch.float32 or not self.log_std.is_contiguous() \
                or tuple(self.log_std.shape) != (policy.n_out,):
            raise ValueError(f"log_std must be a contiguous float32 [{policy.n_out}] tensor on {env.device}")
        self.actor_grads = [torch.zeros_like(t) for t in self.actor_params]
        self.grad_log_std = torch.zeros_like(self.log_std)
        self.critic_grads = [torch.zeros_like(t) for t in self.critic_params] if value is not None else None
        self.params = self.actor_params + [self.log_std] + (self.critic_params or [])
        self.grads = self.actor_grads + [self.grad_log_std] + (self.critic_grads or [])
        self.load()      # (the actor gets its log_std from this tensor before the optimiser is created)
        self.handle = env.batch.make_optim(policy, value, betas=betas, eps=eps, max_grad_norm=max_grad_norm)

    @staticmethod
    def _six(tensors):
        ptrs = [t.data_ptr() for t in tensors]
        if len(ptrs) == 4:
            ptrs[2:2] = [0, 0]
        return ptrs

    def load(self) -> None:
        """``load_policy`` of both networks from the optimiser's tensors, on the current stream"""
        self.env.load_policy(self.policy, self.actor_params, log_std=self.log_std)
        if self.value is not None:
            self.env.load_policy(self.value, self.critic_params)

    def step(self, lr: float, stats=None) -> None:
        """One step on ``grads`` (dockauv_optim_step on the current stream): clip by the global norm, Adam, repack of both
        networks.  ``stats``: None or a contiguous float32 [2] tensor on the device for (norm before clipping, coef).  Does
        not synchronise."""
        torch = self.env.torch
        if stats is not None and (stats.device != self.env.device or stats.dtype != torch.float32 or not stats.is_contiguous()
                                  or tuple(stats.shape) != (2,)):
            raise ValueError(f"stats must be a contiguous float32 [2] tensor on {self.env.device}")
        self.env.batch.optim_step_device(self.handle, lr, self._six(self.actor_params), self.log_std.data_ptr(),
                                         self._six(self.actor_grads), self.grad_log_std.data_ptr(),
                                         None if self.value is None else self._six(self.critic_params),
                                         None if self.value is None else self._six(self.critic_grads),
                                         stats_ptr=0 if stats is None else stats.data_ptr(),
                                         stream=torch.cuda.current_stream().cuda_stream)

    def state(self):
        """(m, v, steps): copies of the two moments as flat float32 device tensors in the order of ``params``, and the number
        of steps taken (dockauv_optim_state)"""
        torch = self.env.torch
        m_ptr, v_ptr, n, t = self.env.batch.optim_state(self.handle)
        from ..parallel import _DevArray
        m, v = (torch.as_tensor(_DevArray(ptr, (n,), "<f4"), device=self.env.device).clone() for ptr in (m_ptr, v_ptr))
        return m, v, t

    def steps(self) -> int:
        """The number of Adam steps taken (dockauv_optim_state).  After a ``ppo_train`` with ``target_kl`` the count is known
        to the device only: the call then waits for that update's stream and reads it back (8 bytes)."""
        return self.env.batch.optim_state(self.handle)[3]


class ShardedTorchDocking3d:
    """
    The same loop over several GPUs, one process per GPU, for a single learner: ``num_envs`` is
    the TOTAL over the ranks of the ``torch.distributed`` group, rank r owns the contiguous range
    ``shard_range(num_envs, world, r)``; ``step`` takes the learner's action batch (global ``[num_envs, n_u]`` -- the
    rank's rows are sliced out in place -- or just the local rows), steps the rank's shard and returns GLOBAL
    ``(obs, reward, done)``: every rank's packed rows, gathered by one RCCL all-gather (``transport="rccl"``, the
    default) or by the peer-to-peer transport (``"p2p"``, gym_dockauv_amd/parallel.py: P2PGather, closed loop: all rows
    of step t are there when the returned views are read on the current stream; accepted only after a bit-exact
    start-up check against RCCL, watched for late peers).  The views stay valid until the next step (rccl) / for two
    further steps (p2p).

        dist.init_process_group("nccl", ...)
        env = ShardedTorchDocking3d(TRAIN_CONFIG, num_envs=8 * 32768, scenario="ObstaclesDocking3d", device=local_rank)
        obs = env.reset()
        obs, reward, done = env.step(policy(obs))        # obs: [262144, n_obs] on every rank
    """

    def __init__(self, env_config: dict = BASE_CONFIG, num_envs: int = 4096, scenario: str = "SimpleDocking3d",
                 device: int = 0, transport: str = "rccl", group=None, device_seed: int = 0, host_seed: Optional[int] = None,
                 vehicles=None, verify_steps: int = 4, check_every: int = 8, p2p_max_spins: int = 8_000_000,
                 gather_dtype: str = "f32", **kw):
        """transport: "rccl" (default: one all_gather_into_tensor per step, what BASELINE.json names) or "p2p" (the
        peer-to-peer push of gym_dockauv_amd/parallel.py).  p2p is only kept if, on EVERY rank, `verify_steps` gathers of
        test rows equal an RCCL all-gather of the same rows bit for bit; otherwise the env falls back to RCCL
        (``self.transport`` says which one runs, ``self.transport_note`` why).  With p2p the time-out word of the
        transport is read every `check_every` steps and in close(): a peer whose step stamp did not arrive within the
        spin bound makes step() raise DockAUVError on every rank that waited for it (the rows it would have returned
        are stale) -- the job is then to be restarted as fresh processes.  The rows of up to `check_every` - 1 steps
        returned BEFORE the raise may already have been stale: a learner discards its last `check_every` steps on that
        error (default 8: one 8-byte read-back every eighth step).
        gather_dtype: "f32" (default: the gathered observations are the kernel's, bit for bit) or "bf16" (RCCL transport:
        the kernel writes the observation columns as bfloat16, round to nearest even, and the links carry half the
        bytes; step() then returns a bfloat16 observation view; reward / done stay float32)."""
        import numpy as np
        import torch
        import torch.distributed as dist
        from ..parallel import P2PShardedStepper, ShardedStepper, shard_range
        from .._capi import DockAUVError
        self.torch = torch
        if not torch.cuda.is_available():
            raise RuntimeError("ShardedTorchDocking3d needs an MI355X: no HIP device visible (there is no CPU fallback)")
        if transport not in ("p2p", "rccl"):
            raise ValueError("transport must be 'p2p' or 'rccl'")
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if self.world > 1 else 0
        if num_envs % self.world:
            raise ValueError("num_envs must be a multiple of the number of ranks (equal shards)")
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self.num_envs = int(num_envs)
        self.first, self.n_local = shard_range(self.num_envs, self.world, self.rank)
        # Mixed batches with sort_vehicles=True (a keyword passed on to the shard's batch): every rank keeps ITS contiguous
        # range of the caller's envs and sorts it by vehicle kind on its device; global row j of the
        # gathered tensors -- and of a global action batch -- then belongs to the caller's env perm[j] (computed identically
        # on every rank from the full vehicle list; identity without the option)
        perm = np.arange(self.num_envs, dtype=np.int64)
        if vehicles is not None:
            vehicles = list(vehicles)
            if len(vehicles) != self.num_envs:
                raise ValueError("len(vehicles) must equal num_envs (the total over all ranks)")
            if kw.get("sort_vehicles"):
                kinds = np.array([0 if v == "BlueROV2" else 1 for v in vehicles])
                for r in range(self.world):
                    f, n = shard_range(self.num_envs, self.world, r)
                    perm[f:f + n] = f + np.argsort(kinds[f:f + n], kind="stable")
            self.vehicles_by_row = [vehicles[int(i)] for i in perm]
            vehicles = vehicles[self.first:self.first + self.n_local]
        else:
            self.vehicles_by_row = None
        self.perm = perm
        self.batch = BatchedDocking3d(env_config, num_envs=self.n_local, scenario=scenario, device=device, precision="f32",
                                      reset_mode="device", device_seed=device_seed + self.rank, rng="batched",
                                      vehicles=vehicles, **kw)
        if host_seed is not None:
            self.batch._gen = np.random.default_rng(host_seed + self.rank)
        self.n_obs, self.n_u = self.batch.n_observations, self.batch.n_u
        self.observation_space, self.action_space = self.batch.observation_space, self.batch.action_space
        self.transport, self.transport_note = transport, None
        if gather_dtype not in ("f32", "bf16"):
            raise ValueError("gather_dtype must be 'f32' or 'bf16'")
        if gather_dtype == "bf16" and transport != "rccl":
            raise ValueError("gather_dtype='bf16' is implemented for the RCCL transport")
        self.gather_dtype = gather_dtype
        packed = "bf16" if gather_dtype == "bf16" else True
        row_words = self.batch.packed_row_words(packed)
        self.check_every = max(1, int(check_every))
        self._steps = 0
        self._DockAUVError = DockAUVError

        def step_fn(actions_local, out_local):
            self.batch.step_device(actions_local.data_ptr(), out_local.data_ptr(),
                                   stream=torch.cuda.current_stream().cuda_stream, packed=packed)

        def rccl_stepper():
            return ShardedStepper(self.n_local, row_words, step_fn, self.device, world=self.world,
                                  rank=self.rank, group=group, overlap=False, gather_dtype=gather_dtype)

        if transport == "p2p":
            p2p, note = None, None
            try:
                p2p = P2PShardedStepper(self.n_local, self.n_obs + 2, step_fn, self.device, world=self.world,
                                        rank=self.rank, group=group, overlap=False, max_spins=p2p_max_spins)
            except (DockAUVError, ValueError) as e:      # (P2PGather agrees across ranks: all raise or none)
                note = f"p2p set-up failed ({e}): RCCL used"
            if p2p is not None and self.world > 1 and verify_steps > 0:
                # the transport itself, without stepping the envs: test rows through the gather vs. an RCCL all-gather
                ok = 1
                ref = torch.empty((self.world * self.n_local, self.n_obs + 2), device=self.device, dtype=torch.float32)
                stream = torch.cuda.current_stream().cuda_stream
                gen = torch.Generator(device=self.device)
                gen.manual_seed(1000 + self.rank)
                for i in range(int(verify_steps)):
                    rows = p2p.rows2[p2p.gather.t & 1]
                    rows.copy_(torch.rand(rows.shape, device=self.device, generator=gen))
                    buf = p2p.gather.gather(rows.data_ptr(), stream)
                    dist.all_gather_into_tensor(ref, rows, group=group)
                    ok &= int(torch.equal(buf.view(torch.int32), ref.view(torch.int32)))
                ok &= int(p2p.gather.timed_out() == 0)
                flag = torch.tensor([ok], device=self.device, dtype=torch.int32)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
                if int(flag.item()) != 1:
                    note = "p2p rows differed from the RCCL all-gather (or a stamp timed out) in the start-up check: RCCL used"
                    p2p.close()
                    p2p = None
            if p2p is None:
                self.transport, self.transport_note = "rccl", note
                self.stepper = rccl_stepper()
            else:
                self.stepper = p2p
        else:
            self.stepper = rccl_stepper()
        self._zeros = None

    def _check_transport(self) -> None:
        """p2p: a peer's stamp that did not arrive within the spin bound is sticky in the status word (every later wait
        returns at once and the gather buffers would hand out rows of an earlier step)."""
        if self.transport != "p2p":
            return
        late = self.stepper.gather.timed_out()
        if late:
            raise self._DockAUVError(f"rank {self.rank}: the step stamps of rank(s) {[r for r in range(self.world) if late >> r & 1]} "
                                     f"did not arrive within the spin bound after {self._steps} steps: the gathered rows are "
                                     "stale; restart the job")

    def reset(self, seed: Optional[int] = None):
        """All envs of this rank's shard: new episodes; returns the reference's reset observation for ALL envs (zeros,
        docking3d.py:269,322)."""
        self.batch.reset(seed=seed)
        if self._zeros is None:
            self._zeros = self.torch.zeros((self.num_envs, self.n_obs), device=self.device, dtype=self.torch.float32)
        return self._zeros

    def step(self, actions):
        """actions: contiguous float32 on this device, [num_envs, n_u] (global; this rank's rows are used) or
        [n_local, n_u].  Returns global (obs [num_envs, n_obs], reward [num_envs], done [num_envs] bool) views."""
        torch = self.torch
        if actions.device != self.device or actions.dtype != torch.float32 or not actions.is_contiguous():
            raise ValueError(f"actions must be a contiguous float32 tensor on {self.device}")
        if tuple(actions.shape) == (self.num_envs, self.n_u) and self.world > 1:
            actions = actions[self.first:self.first + self.n_local]
        elif tuple(actions.shape) != (self.n_local, self.n_u):
            raise ValueError(f"actions must be [{self.num_envs}, {self.n_u}] (global) or [{self.n_local}, {self.n_u}] (local)")
        buf = self.stepper.step(actions)
        self._steps += 1
        self.batch.poll_status()   # (the step kernels' own status word: host-coherent, no synchronisation)
        if self._steps % self.check_every == 0:
            self._check_transport()
        if self.gather_dtype == "bf16":
            from ..parallel import ShardedStepper
            return ShardedStepper.split_bf16(buf, self.n_obs)
        return buf[:, : self.n_obs], buf[:, self.n_obs], buf[:, self.n_obs + 1] > 0.5

    def close(self) -> None:
        err = None
        try:
            self._check_transport()
            if getattr(self.batch, "_handle", None) is not None and self.batch._handle.value:
                self.batch.synchronize()   # (reports the kernels' status word as well)
        except Exception as e:          # still release everything; re-raise afterwards
            err = e
        if hasattr(self.stepper, "close"):
            self.stepper.close()
        self.batch.close()
        if err is not None:
            raise err
