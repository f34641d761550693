"""
The library's own actor for the closed loop: a small MLP (one or two hidden layers of up to 128 units) evaluated on the
device by libdockauv's policy kernel (include/dockauv.h: dockauv_policy_*, dockauv_rollout).  The reference's counterpart
is SB3's ``MlpPolicy``, which train.py:64 instantiates and train.py:64-71 / 86-119 query once per step.

``MLPPolicy`` is a plain host object that holds the arrays; ``BatchedDocking3d.make_policy`` / ``TorchDocking3d.make_policy``
put it on the device.  An ``MLPPolicy`` with one raw output is a critic (SB3's ``mlp_extractor.value_net`` + ``value_net``;
``value_from_torch``, ``make_value``): the PPO collector (dockauv_collect) evaluates it on the rollout's rows.
``SquashedGaussianMLP`` is SAC's actor (two heads, a state-dependent log_std, tanh squashing; ``make_sac_actor``), an ``MLPPolicy``
on [obs | action] with one raw output a Q critic (``make_q``); ``sac_target_reference`` states the TD target's last kernel,
``sac_critic_head_reference``, ``sac_actor_head_reference`` and ``ent_coef_step_reference`` SAC's loss head in float64 (their
``*_float32`` twins and ``normals_float32``: what float32 does to them, the tests' yardstick).
``forward_reference``, ``backward_reference``, ``normals_reference``, ``log_prob_reference``, ``gae_reference``,
``ppo_head_reference``, ``adam_reference`` and ``permutation_reference`` (exact integers) are float64
NumPy statements of what the kernels compute (for tests and for callers who want to check a port); they are never used as a compute path.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _capi

_ACTS = {"none": _capi.ACT_NONE, "tanh": _capi.ACT_TANH, "relu": _capi.ACT_RELU}

# Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11; Random123 constants)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _philox4x32_10(counter: np.ndarray, key: Sequence[int]) -> np.ndarray:
    """counter [..., 4] (values < 2^32), key (k0, k1) -> [..., 4] uint64 words < 2^32"""
    c = [np.array(counter[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return np.stack(c, axis=-1)


def _act(x: np.ndarray, kind: str) -> np.ndarray:
    if kind == "tanh":
        return np.tanh(x)
    if kind == "relu":
        return np.maximum(x, 0.0)
    return x


class MLPPolicy:
    """a = out_act(W3 act(W2 act(W1 obs + b1) + b2) + b3); ``layers``: [(W [out, in], b [out]), ...] of two or three
    Linear layers (torch.nn.Linear layout); ``log_std`` [n_out] or None."""

    def __init__(self, layers, hidden_act: str = "tanh", out_act: str = "none", log_std=None):
        if len(layers) not in (2, 3):
            raise ValueError("MLPPolicy takes one or two hidden layers plus the output layer")
        if hidden_act not in ("tanh", "relu"):
            raise ValueError("hidden_act must be 'tanh' or 'relu'")
        if out_act not in ("none", "tanh"):
            raise ValueError("out_act must be 'none' or 'tanh'")
        self.layers = [(np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)) for W, b in layers]
        n = self.layers[0][0].shape[1]
        for W, b in self.layers:
            if W.ndim != 2 or b.shape != (W.shape[0],) or W.shape[1] != n:
                raise ValueError("layer shapes do not chain: W [out, in], b [out]")
            n = W.shape[0]
        self.hidden_act, self.out_act = hidden_act, out_act
        self.log_std = None if log_std is None else np.ascontiguousarray(log_std, dtype=np.float32).reshape(-1)
        if self.log_std is not None and self.log_std.shape != (self.n_out,):
            raise ValueError("log_std must have n_out entries")

    n_in = property(lambda self: int(self.layers[0][0].shape[1]))
    n_out = property(lambda self: int(self.layers[-1][0].shape[0]))
    n_hidden = property(lambda self: [int(W.shape[0]) for W, _ in self.layers[:-1]])

    # ------------------------------------------------------------------------------------------ construction
    @classmethod
    def from_torch(cls, module_or_state_dict, hidden_act: Optional[str] = None, out_act: Optional[str] = None, log_std=None):
        """An ``nn.Sequential`` of Linear / Tanh / ReLU layers (activations are read off the modules), or an SB3-style
        state dict with ``mlp_extractor.policy_net.{0,2}.*``, ``action_net.*`` and (optionally) ``log_std`` -- there the
        hidden activation is ``hidden_act`` (SB3's default: tanh) and the output is raw unless ``out_act`` says otherwise.
        Needs no stable-baselines3 import."""
        def arr(t):
            return (t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)).astype(np.float32)

        if isinstance(module_or_state_dict, dict) or hasattr(module_or_state_dict, "keys"):
            sd = module_or_state_dict
            layers = []
            for i in (0, 2):
                k = f"mlp_extractor.policy_net.{i}.weight"
                if k in sd:
                    layers.append((arr(sd[k]), arr(sd[f"mlp_extractor.policy_net.{i}.bias"])))
            if not layers or "action_net.weight" not in sd:
                raise ValueError("state dict needs mlp_extractor.policy_net.0.* and action_net.*")
            layers.append((arr(sd["action_net.weight"]), arr(sd["action_net.bias"])))
            if log_std is None and "log_std" in sd:
                log_std = arr(sd["log_std"])
            return cls(layers, hidden_act or "tanh", out_act or "none", log_std)
        layers, acts = [], []
        for m in module_or_state_dict:
            name = type(m).__name__
            if name == "Linear":
                layers.append((arr(m.weight), arr(m.bias) if m.bias is not None else np.zeros(m.weight.shape[0], np.float32)))
                acts.append("none")
            elif name in ("Tanh", "ReLU") and layers:
                if acts[-1] != "none":
                    raise ValueError("two activations in a row")
                acts[-1] = name.lower()
            else:
                raise ValueError(f"unsupported layer {name}: Linear, Tanh and ReLU are")
        if len(layers) not in (2, 3) or len(set(acts[:-1])) != 1 or acts[0] == "none":
            raise ValueError("expected Linear-act-[Linear-act-]Linear[-Tanh] with one kind of hidden activation")
        if (hidden_act and hidden_act != acts[0]) or (out_act and out_act != acts[-1]):
            raise ValueError("the activations asked for are not the module's")
        return cls(layers, acts[0], acts[-1], log_std)

    @classmethod
    def value_from_torch(cls, module_or_state_dict, hidden_act: Optional[str] = None):
        """The critic: an ``nn.Sequential`` ending in ``Linear(.., 1)``, or an SB3-style state dict with
        ``mlp_extractor.value_net.{0,2}.*`` and ``value_net.*`` (hidden activation ``hidden_act``, SB3's default: tanh)."""
        if isinstance(module_or_state_dict, dict) or hasattr(module_or_state_dict, "keys"):
            sd = module_or_state_dict
            if "mlp_extractor.value_net.0.weight" not in sd or "value_net.weight" not in sd:
                raise ValueError("state dict needs mlp_extractor.value_net.0.* and value_net.*")
            renamed = {}
            for i in (0, 2):
                for part in ("weight", "bias"):
                    k = f"mlp_extractor.value_net.{i}.{part}"
                    if k in sd:
                        renamed[f"mlp_extractor.policy_net.{i}.{part}"] = sd[k]
            renamed["action_net.weight"], renamed["action_net.bias"] = sd["value_net.weight"], sd["value_net.bias"]
            critic = cls.from_torch(renamed, hidden_act, "none")
        else:
            critic = cls.from_torch(module_or_state_dict, hidden_act, "none")
        if critic.n_out != 1:
            raise ValueError(f"a critic has one output, this one has {critic.n_out}")
        return critic

    # ------------------------------------------------------------------------------------------ float64 statements
    @staticmethod
    def log_prob_reference(z, log_std) -> np.ndarray:
        """log pi(a|s) of a diagonal Gaussian at a = mean + exp(log_std) z: sum_j (-z_j^2 / 2 - log_std_j - log(2 pi) / 2);
        z [..., n_out] (zeros: the deterministic action), log_std [n_out].  float64 [...]."""
        z = np.asarray(z, dtype=np.float64)
        ls = np.asarray(log_std, dtype=np.float64)
        return (-0.5 * z * z - ls - 0.5 * np.log(2.0 * np.pi)).sum(axis=-1)

    @staticmethod
    def gae_reference(reward, done, values, gamma: float, gae_lambda: float, truncated=None, v_terminal=None):
        """SB3's RolloutBuffer.compute_returns_and_advantage in float64: reward, done [K, N]; values [K + 1, N] with values[k] =
        V of the observation step k acted on and values[K] = V of the last one; every done is terminal.  Returns
        (advantages [K, N], returns [K, N]).
        ``truncated`` bool [K, N] with ``v_terminal`` [K, N] (both or neither; dockauv_gae_truncated): where a step is done and
        truncated its reward is reward + gamma * v_terminal, as SB3's collect_rollouts adds gamma * V(terminal_observation) for
        ``TimeLimit.truncated``; the done stays a done (the advantage does not cross the reset).  ``v_terminal`` is read nowhere
        else."""
        r = np.asarray(reward, dtype=np.float64)
        nt = 1.0 - (np.asarray(done) > 0.5).astype(np.float64)
        v = np.asarray(values, dtype=np.float64)
        K = r.shape[0]
        if v.shape[0] != K + 1 or nt.shape != r.shape or v.shape[1:] != r.shape[1:]:
            raise ValueError("reward, done: [K, N]; values: [K + 1, N]")
        if (truncated is None) != (v_terminal is None):
            raise ValueError("truncated and v_terminal: both or neither")
        if truncated is not None:
            tr = np.asarray(truncated).astype(bool) & (nt == 0.0)
            vt = np.asarray(v_terminal, dtype=np.float64)
            if tr.shape != r.shape or vt.shape != r.shape:
                raise ValueError("truncated, v_terminal: [K, N]")
            r = r.copy()
            r[tr] = r[tr] + gamma * vt[tr]
        adv = np.zeros_like(r)
        gae = np.zeros(r.shape[1:], dtype=np.float64)
        for k in range(K - 1, -1, -1):
            delta = r[k] + gamma * nt[k] * v[k + 1] - v[k]
            gae = delta + gamma * gae_lambda * nt[k] * gae
            adv[k] = gae
        return adv, adv + v[:K]

    @staticmethod
    def ppo_head_reference(mean, v, actions, log_prob_old, advantages, returns, log_std, clip_range: float, vf_coef: float,
                           ent_coef: float, normalize_advantage: bool = True, clip_range_vf=None, values_old=None):
        """float64 statement of dockauv_ppo_head on one minibatch, every array already gathered: mean, actions [B, n_out];
        v (None: no critic), log_prob_old, advantages, returns [B]; log_std [n_out].  The loss is SB3's: the clipped surrogate
        on advantages normalised with the unbiased standard deviation, vf_coef x the squared value error, ent_coef x the
        negative Gaussian entropy.  Returns (grad_mean [B, n_out], grad_v [B] or None, grad_log_std [n_out], stats [8]):
        d loss / d mean, d loss / d v, d loss / d log_std and (loss, policy_loss, value_loss, entropy_loss, approx_kl,
        clip_fraction, advantage mean, advantage std -- 0 and 1 without normalisation).  Where the two surrogates tie (inside
        the clip range, and on its edges) the gradient is the unclipped one, as torch.min and clamp give it.
        ``clip_range_vf`` > 0 with ``values_old`` [B] (dockauv_ppo_update): the value error is taken at v_old + clamp(v - v_old,
        -c, c), whose gradient with respect to v is 1 for |v - v_old| <= c (the edges included, as torch.clamp's backward
        gives it) and 0 beyond.  None / 0: the plain squared error."""
        f = lambda x: np.asarray(x, dtype=np.float64)
        mean, a, lpo, adv, ls = f(mean), f(actions), f(log_prob_old).reshape(-1), f(advantages).reshape(-1), f(log_std).reshape(-1)
        B, n_out = mean.shape
        if a.shape != (B, n_out) or lpo.shape != (B,) or adv.shape != (B,) or ls.shape != (n_out,):
            raise ValueError("mean, actions: [B, n_out]; log_prob_old, advantages: [B]; log_std: [n_out]")
        m, s = 0.0, 1.0
        if normalize_advantage:
            if B < 2:
                raise ValueError("normalize_advantage needs B >= 2")
            m, s = float(adv.mean()), float(adv.std(ddof=1))
            adv = (adv - m) / (s + 1e-8)
        clip = float(clip_range)
        z = (a - mean) * np.exp(-ls)
        lr = MLPPolicy.log_prob_reference(z, ls) - lpo
        ratio = np.exp(lr)
        live = ~(((adv > 0) & (ratio > 1.0 + clip)) | ((adv < 0) & (ratio < 1.0 - clip)))
        policy_loss = -np.minimum(ratio * adv, np.clip(ratio, 1.0 - clip, 1.0 + clip) * adv).mean()
        g = -(adv * ratio * live) / B
        grad_mean = g[:, None] * z * np.exp(-ls)
        grad_log_std = (g[:, None] * (z * z - 1.0)).sum(axis=0) - ent_coef
        entropy_loss = -float((0.5 + 0.5 * np.log(2.0 * np.pi) + ls).sum())
        value_loss, grad_v = 0.0, None
        if v is not None:
            v, ret = f(v).reshape(-1), f(returns).reshape(-1)
            if v.shape != (B,) or ret.shape != (B,):
                raise ValueError("v, returns: [B]")
            dv, inside = v - ret, 1.0
            if clip_range_vf is not None and float(clip_range_vf) > 0.0:
                if values_old is None:
                    raise ValueError("clip_range_vf needs values_old")
                c, vo = float(clip_range_vf), f(values_old).reshape(-1)
                if vo.shape != (B,):
                    raise ValueError("values_old: [B]")
                d = v - vo
                dv, inside = (vo + np.clip(d, -c, c)) - ret, (np.abs(d) <= c).astype(np.float64)
            value_loss = float((dv ** 2).mean())
            grad_v = 2.0 * vf_coef * dv * inside / B
        loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
        stats = np.array([loss, policy_loss, value_loss, entropy_loss, ((ratio - 1.0) - lr).mean(),
                          (np.abs(ratio - 1.0) > clip).mean(), m, s], dtype=np.float64)
        return grad_mean, grad_v, grad_log_std, stats

    @staticmethod
    def adam_reference(params, grads, m, v, t: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-5, max_grad_norm: float = 0.5):
        """float64 statement of dockauv_optim_step on sequences of arrays of matching shapes: the norm over ALL gradients,
        coef = min(1, max_grad_norm / (norm + 1e-6)) (1 with max_grad_norm <= 0: torch's clip_grad_norm_), then step ``t`` >= 1
        of torch.optim.Adam without weight decay or amsgrad on the scaled gradients.  Returns (params, m, v, norm, coef): three
        lists of new float64 arrays and two floats; nothing is changed in place."""
        f = lambda xs: [np.asarray(x, dtype=np.float64) for x in xs]
        params, grads, m, v = f(params), f(grads), f(m), f(v)
        if not (len(params) == len(grads) == len(m) == len(v)) or any(not (p.shape == g.shape == a.shape == b.shape)
                                                                      for p, g, a, b in zip(params, grads, m, v)):
            raise ValueError("params, grads, m, v: sequences of arrays of matching shapes")
        if int(t) < 1:
            raise ValueError("t counts the steps from 1")
        b1, b2 = float(betas[0]), float(betas[1])
        norm = float(np.sqrt(sum(float((g * g).sum()) for g in grads)))
        coef = min(1.0, float(max_grad_norm) / (norm + 1e-6)) if max_grad_norm > 0 else 1.0
        step_size = float(lr) / (1.0 - b1 ** int(t))
        rsq = 1.0 / np.sqrt(1.0 - b2 ** int(t))
        new_p, new_m, new_v = [], [], []
        for p, g, a, b in zip(params, grads, m, v):
            g = g * coef
            a = a + (1.0 - b1) * (g - a)
            b = b2 * b + (1.0 - b2) * g * g
            new_p.append(p - step_size * (a / (np.sqrt(b) * rsq + float(eps))))
            new_m.append(a)
            new_v.append(b)
        return new_p, new_m, new_v, norm, coef

    def forward_reference(self, obs: np.ndarray, z: Optional[np.ndarray] = None) -> np.ndarray:
        """float64 forward of float32 weights: obs [..., n_in] -> [..., n_out]; ``z`` [..., n_out]: exploration normals,
        added as exp(log_std) * z before the output activation."""
        x = np.asarray(obs, dtype=np.float64)
        for W, b in self.layers[:-1]:
            x = _act(x @ W.astype(np.float64).T + b.astype(np.float64), self.hidden_act)
        W, b = self.layers[-1]
        x = x @ W.astype(np.float64).T + b.astype(np.float64)
        if z is not None:
            if self.log_std is None:
                raise ValueError("z given but the policy has no log_std")
            x = x + np.exp(self.log_std.astype(np.float64)) * np.asarray(z, dtype=np.float64)
        return _act(x, self.out_act)

    def backward_reference(self, obs: np.ndarray, grad_out: np.ndarray):
        """float64 statement of dockauv_policy_backward: obs [B, n_in], grad_out [B, n_out] = dL/d(out) with out = W3 h_last +
        b3 (before out_act, no noise).  Returns the gradients in layer order, (dW1, db1[, dW2, db2], dW3, db3), each summed over
        the rows, torch.nn.Linear layout.  tanh' = 1 - h^2; relu' = 1 where the pre-activation is > 0, else 0."""
        x = np.asarray(obs, dtype=np.float64).reshape(-1, self.n_in)
        g = np.asarray(grad_out, dtype=np.float64).reshape(-1, self.n_out)
        if x.shape[0] != g.shape[0]:
            raise ValueError("obs [B, n_in] and grad_out [B, n_out] need the same B")
        hs = [x]
        for W, b in self.layers[:-1]:
            hs.append(_act(hs[-1] @ W.astype(np.float64).T + b.astype(np.float64), self.hidden_act))
        grads = []
        for i in range(len(self.layers) - 1, -1, -1):
            grads[:0] = [g.T @ hs[i], g.sum(axis=0)]
            if i > 0:
                h = hs[i]
                g = (g @ self.layers[i][0].astype(np.float64)) * (1.0 - h * h if self.hidden_act == "tanh" else (h > 0.0).astype(np.float64))
        return tuple(grads)

    def backward_input_reference(self, x: np.ndarray, grad_out: np.ndarray) -> np.ndarray:
        """float64 dL/dx of the same pass: x [B, n_in], grad_out [B, n_out] on the raw output -> [B, n_in] = delta1 W1, row by
        row (no sum over the rows).  Columns n_obs .. of a Q critic's [obs | a] are dockauv_q_backward's grad_actions."""
        x = np.asarray(x, dtype=np.float64).reshape(-1, self.n_in)
        g = np.asarray(grad_out, dtype=np.float64).reshape(-1, self.n_out)
        if x.shape[0] != g.shape[0]:
            raise ValueError("x [B, n_in] and grad_out [B, n_out] need the same B")
        hs = [x]
        for W, b in self.layers[:-1]:
            hs.append(_act(hs[-1] @ W.astype(np.float64).T + b.astype(np.float64), self.hidden_act))
        for i in range(len(self.layers) - 1, -1, -1):
            g = g @ self.layers[i][0].astype(np.float64)
            if i > 0:
                h = hs[i]
                g = g * (1.0 - h * h if self.hidden_act == "tanh" else (h > 0.0).astype(np.float64))
        return g

    @staticmethod
    def normals_reference(seed: int, env_ids, t: int, n_out: int, slot: int = 2) -> np.ndarray:
        """The standard normals the kernel draws for step counter ``t``: Philox4x32-10 counter (env id mod 2^32, t mod 2^32,
        j, slot), key = seed (``slot`` 2: the per-env actors; ``SAC_ROWS_STREAM`` = 5: the rows form of the squashed-Gaussian
        actor, where ``env_ids`` are row_offset + the position in the batch); Box-Muller cos branch on the first two words with u1 = ((x0 >> 8) + 0.5) 2^-24, u2 = (x1 >> 8) 2^-24.
        ``env_ids`` already include the policy's env_id_offset.  Returns float64 [len(env_ids), n_out].

        This is the exact statement.  The kernel forms u1 in float32 (as the step kernel's current noise does), which holds
        the + 0.5 only while x0 >> 8 < 2^23: above that the sum is rounded to even, so u1 is off by up to 2^-25 there and the
        top value x0 >> 8 = 2^24 - 1 gives u1 = 1 and z = 0.  That rounding, amplified by 1 / (u1 sqrt(-2 log u1)) near
        u1 = 1, and the float32 log / sqrt / cos are the whole device-to-reference deviation (a few 1e-5 at most)."""
        env = np.asarray(env_ids, dtype=np.uint64).reshape(-1) & _MASK
        ctr = np.empty((env.size, n_out, 4), dtype=np.uint64)
        ctr[..., 0] = env[:, None]
        ctr[..., 1] = np.uint64(int(t) & 0xFFFFFFFF)
        ctr[..., 2] = np.arange(n_out, dtype=np.uint64)[None, :]
        ctr[..., 3] = np.uint64(int(slot))
        x = _philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
        u1 = ((x[..., 0] >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
        u2 = (x[..., 1] >> np.uint64(8)).astype(np.float64) / 16777216.0
        return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)

    @staticmethod
    def normals_float32(seed: int, env_ids, t: int, n_out: int, slot: int = 2) -> np.ndarray:
        """The float32 restatement of the same draw, as the kernel forms it (dockauv_policy_tile.h: policy_normal_): u1 =
        ((float)(x0 >> 8) + 0.5f) 2^-24 with the sum rounded to float32, u2 = (float)(x1 >> 8) 2^-24, z = sqrtf(-2 logf(u1))
        cospif(2 u2), every operation in float32 NumPy (the cosine of the exactly reduced argument, rounded once).  Returns
        float32 [len(env_ids), n_out]: the yardstick of what float32 does to ``normals_reference``, never a compute path."""
        env = np.asarray(env_ids, dtype=np.uint64).reshape(-1) & _MASK
        ctr = np.empty((env.size, n_out, 4), dtype=np.uint64)
        ctr[..., 0] = env[:, None]
        ctr[..., 1] = np.uint64(int(t) & 0xFFFFFFFF)
        ctr[..., 2] = np.arange(n_out, dtype=np.uint64)[None, :]
        ctr[..., 3] = np.uint64(int(slot))
        x = _philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
        f = np.float32
        u1 = ((x[..., 0] >> np.uint64(8)).astype(np.float32) + f(0.5)) * f(1.0 / 16777216.0)
        u2 = (x[..., 1] >> np.uint64(8)).astype(np.float32) * f(1.0 / 16777216.0)
        z = np.sqrt(f(-2.0) * np.log(u1)) * np.cos(np.pi * (f(2.0) * u2).astype(np.float64)).astype(np.float32)
        assert z.dtype == np.float32
        return z

    @staticmethod
    def permutation_reference(seed: int, epoch: int, n: int) -> np.ndarray:
        """The exact statement of dockauv_permutation: int64 [n], out[i] = P(i) for the keyed bijection P of [0, n) -- an
        eight-round Feistel network on b = max(2, bit_length(n - 1)) bits (left half: the high b // 2 bits) whose round keys
        are the eight words of the Philox4x32-10 blocks of counters (q, epoch mod 2^32, 0, 3), q = 0, 1, key = seed, applied
        again while the result is >= n (cycle-walking: the walk stays on the cycle through i < n, so it ends).  Round r with
        left width w: t = ((R + k_r) mod 2^32) * 0xD2511F53; f = hi32(t) ^ lo32(t); f = (f ^ (f >> 15)) & (2^w - 1);
        (L, R) = (R, L ^ f), and the widths swap.  Integer arithmetic only: the kernel gives the same bits."""
        n = int(n)
        if n < 1 or n > 1 << 31:
            raise ValueError("n must be in 1 .. 2^31")
        ctr = np.zeros((2, 4), dtype=np.uint64)
        ctr[:, 0] = (0, 1)
        ctr[:, 1] = np.uint64(int(epoch) & 0xFFFFFFFF)
        ctr[:, 3] = np.uint64(3)
        keys = _philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)).reshape(8)
        b = max(2, (n - 1).bit_length())
        wl, wr = b // 2, b - b // 2

        def network(x):
            L, R = x >> np.uint64(wr), x & np.uint64((1 << wr) - 1)
            w = [wl, wr]
            for r in range(8):
                t = ((R + keys[r]) & _MASK) * _M0
                f = (t >> _S32) ^ (t & _MASK)
                f = (f ^ (f >> np.uint64(15))) & np.uint64((1 << w[r & 1]) - 1)
                L, R = R, L ^ f
            return (L << np.uint64(wr)) | R

        out = network(np.arange(n, dtype=np.uint64))
        while True:
            walk = np.nonzero(out >= np.uint64(n))[0]
            if walk.size == 0:
                return out.astype(np.int64)
            out[walk] = network(out[walk])

    # ------------------------------------------------------------------------------------------ C ABI
    def shape_desc(self) -> _capi.PolicyDesc:
        """dockauv_policy_desc with the shapes and activations filled in and no arrays"""
        d = _capi.PolicyDesc()
        d.struct_size = C.sizeof(_capi.PolicyDesc)
        d.precision = _capi.F32
        d.n_in, d.n_out = self.n_in, self.n_out
        d.n_hidden[0] = self.n_hidden[0]
        d.n_hidden[1] = self.n_hidden[1] if len(self.n_hidden) == 2 else 0
        d.hidden_act, d.out_act = _ACTS[self.hidden_act], _ACTS[self.out_act]
        return d

    def host_desc(self, seed: int = 0, env_id_offset: int = 0) -> _capi.PolicyDesc:
        """dockauv_policy_desc over this object's host arrays (which must outlive the call that reads it)"""
        d = self.shape_desc()
        d.pointers_on_device = 0
        ptrs = [a.ctypes.data for Wb in self.layers for a in Wb]
        if len(self.layers) == 2:
            ptrs[2:2] = [None, None]
        d.W1, d.b1, d.W2, d.b2, d.W3, d.b3 = ptrs
        d.log_std = None if self.log_std is None else self.log_std.ctypes.data
        d.seed, d.env_id_offset = int(seed), int(env_id_offset)
        return d


SAC_ROWS_STREAM = 5        # word 3 of the Philox counter of the squashed-Gaussian actor's normals on rows (dockauv_sac_target)
_F32 = np.float32


def _fmaf(a, b, c) -> np.ndarray:
    """fmaf on float32 arrays, one rounding: the product of two float32 is exact in float64; its sum with c is rounded to
    float64 and then to float32, and where that first rounding lands on a float32 tie it is undone by the sum's exact error
    (round to odd), so the result is the correctly rounded a * b + c."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    tie = (np.ascontiguousarray(s).view(np.int64) & np.int64(0x1FFFFFFF)) == np.int64(0x10000000)
    adj = tie & (err != 0.0) & np.isfinite(s)
    s = np.where(adj, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def sac_target_reference(q1, q2, logp2, rewards, dones, gamma: float, ent_coef=None, log_ent_coef=None) -> np.ndarray:
    """The exact float32 statement of the last kernel of dockauv_sac_target on arrays of one shape:
    v = fmaf(-alpha, logp2, fminf(q1, q2)); y = fmaf(gamma * (1.0f - d), v, r), with alpha = ``ent_coef`` or, given
    ``log_ent_coef``, float32(exp(log_ent_coef)) (the device takes expf of its own: equal up to that function's last bit).
    ``dones`` are rb.sample's: done * (1 - timeout)."""
    if (ent_coef is None) == (log_ent_coef is None):
        raise ValueError("give either ent_coef or log_ent_coef")
    alpha = _F32(ent_coef) if log_ent_coef is None else _F32(np.exp(np.float64(_F32(log_ent_coef))))
    f = lambda x: np.asarray(x, dtype=np.float32)
    q1, q2, lp, r, d = f(q1), f(q2), f(logp2), f(rewards), f(dones)
    v = _fmaf(-alpha, lp, np.minimum(q1, q2))
    return _fmaf(_F32(gamma) * (_F32(1.0) - d), v, r)


# ------------------------------------------------------------------------------------------ SAC: the loss head
# float64 statements of dockauv_sac_critic_head, dockauv_sac_actor_head and dockauv_sac_ent_coef_step by SB3 1.5's formulas as they
# are written, and their float32 NumPy restatements (include/dockauv.h's expressions through _fmaf and _F32): what float32 can do
# on these expressions -- the yardstick of the device's error, never a compute path.
def _mean32(x) -> np.float32:
    """a float64 sum of float32 terms divided by their count, rounded once: how the head kernels form a mean"""
    x = np.asarray(x)
    assert x.dtype == np.float32
    return _F32(x.astype(np.float64).sum() / x.size)


def _alpha_of(ent_coef, log_ent_coef, f32: bool):
    if (ent_coef is None) == (log_ent_coef is None):
        raise ValueError("give either ent_coef or log_ent_coef")
    if log_ent_coef is None:
        return _F32(ent_coef) if f32 else float(_F32(ent_coef))
    e = np.exp(np.float64(_F32(log_ent_coef)))
    return _F32(e) if f32 else float(e)


def sac_critic_head_reference(q1, q2, y):
    """float64 statement of dockauv_sac_critic_head: SB3's critic_loss = 0.5 * sum_k mse_loss(q_k, y) on arrays [B].  Returns
    (grad_q1, grad_q2, stats [6]) = d critic_loss / d q_k = (q_k - y) / B and (critic_loss, mse1, mse2, mean q1, mean q2, mean y)."""
    q1, q2, y = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (q1, q2, y))
    if not (q1.shape == q2.shape == y.shape) or q1.size < 1:
        raise ValueError("q1, q2, y: [B]")
    B = q1.size
    d1, d2 = q1 - y, q2 - y
    mse1, mse2 = float((d1 * d1).mean()), float((d2 * d2).mean())
    return d1 / B, d2 / B, np.array([0.5 * (mse1 + mse2), mse1, mse2, q1.mean(), q2.mean(), y.mean()], dtype=np.float64)


def sac_critic_head_float32(q1, q2, y):
    """The float32 restatement of dockauv_sac_critic_head: the subtraction and the division are exact IEEE operations, so the two
    gradients are the device's bit for bit; stats as the kernel forms them (float64 sums of float32 terms, rounded once)."""
    q1, q2, y = (np.asarray(x, dtype=np.float32).reshape(-1) for x in (q1, q2, y))
    nf = _F32(q1.size)
    d1, d2 = q1 - y, q2 - y
    mse1, mse2 = _mean32(d1 * d1), _mean32(d2 * d2)
    stats = np.array([_F32(0.5) * (mse1 + mse2), mse1, mse2, _mean32(q1), _mean32(q2), _mean32(y)], dtype=np.float32)
    return d1 / nf, d2 / nf, stats


def sac_actor_head_reference(heads, z, q1_pi, q2_pi, dq1, dq2, ent_coef=None, log_ent_coef=None):
    """float64 statement of dockauv_sac_actor_head by SB3's formulas as they are written: heads [B, 2 n_u] = (mu | raw log-std), z
    [B, n_u] the normals of the draw; x = mu + exp(clamp(raw, -20, 2)) z, a = tanh(x), logp = sum_j Normal(mu, std).log_prob(x) -
    sum_j log(1 - a^2 + 1e-6); actor_loss = mean(alpha logp - min(q1_pi, q2_pi)) with q_pi [B] the critics at a and dq1, dq2
    [B, n_u] their gradients on a.  Returns (grad_out [B, 2 n_u], stats [4], a, logp): d actor_loss / d heads -- zero on the raw
    log-std where it lies outside [-20, 2], the edges included as torch.clamp's backward includes them; the minimum's gradient
    goes to critic 1 on a tie -- and (actor_loss, mean logp, mean min q, alpha)."""
    alpha = _alpha_of(ent_coef, log_ent_coef, False)
    heads = np.asarray(heads, dtype=np.float64)
    B, n_u = heads.shape[0], heads.shape[1] // 2
    z, dq1, dq2 = (np.asarray(x, dtype=np.float64).reshape(B, n_u) for x in (z, dq1, dq2))
    q1, q2 = (np.asarray(x, dtype=np.float64).reshape(B) for x in (q1_pi, q2_pi))
    mu, raw = heads[:, :n_u], heads[:, n_u:]
    ls = np.clip(raw, -20.0, 2.0)
    std = np.exp(ls)
    x = mu + std * z
    a = np.tanh(x)
    s = 1.0 - a * a
    logp = (-((x - mu) ** 2) / (2.0 * std ** 2) - ls - 0.5 * np.log(2.0 * np.pi)).sum(axis=1) - np.log(s + 1e-6).sum(axis=1)
    w = 2.0 * a * s / (s + 1e-6)                       # d logp / d x
    sel = np.where((q1 <= q2)[:, None], dq1, dq2)
    gx = (alpha * w - sel * s) / B
    inside = (raw >= -20.0) & (raw <= 2.0)
    g_ls = np.where(inside, gx * std * z - alpha / B, 0.0)
    mq = np.minimum(q1, q2)
    stats = np.array([(alpha * logp - mq).mean(), logp.mean(), mq.mean(), alpha], dtype=np.float64)
    return np.concatenate([gx, g_ls], axis=1), stats, a, logp


def sac_actor_head_float32(heads, z, q1_pi, q2_pi, dq1, dq2, ent_coef=None, log_ent_coef=None):
    """The float32 restatement of dockauv_sac_actor_head (and, in its last two results, of dockauv_sac_sample): include/dockauv.h's
    expressions in float32 NumPy arrays, ``z`` rounded to float32.  Returns (grad_out, stats [4], a, logp), all float32."""
    f = _F32
    alpha = _alpha_of(ent_coef, log_ent_coef, True)
    heads = np.asarray(heads, dtype=np.float32)
    B, n_u = heads.shape[0], heads.shape[1] // 2
    z, dq1, dq2 = (np.asarray(x, dtype=np.float32).reshape(B, n_u) for x in (z, dq1, dq2))
    q1, q2 = (np.asarray(x, dtype=np.float32).reshape(B) for x in (q1_pi, q2_pi))
    nf = f(B)
    mu, raw = heads[:, :n_u], heads[:, n_u:]
    ls = np.clip(raw, f(-20.0), f(2.0))
    std = np.exp(ls)
    x = _fmaf(std, z, mu)
    a = np.tanh(x)
    gauss = _fmaf(f(-0.5) * z, z, -(ls + f(0.918938533)))
    e = np.exp(f(-2.0) * np.abs(x))
    d = f(1.0) + e
    s = f(4.0) * e / (d * d)
    corr = np.log(s + f(1e-6))
    seq = lambda t: np.add.accumulate(t, axis=1, dtype=np.float32)[:, -1] if t.shape[1] else np.zeros(B, dtype=np.float32)
    logp = (seq(gauss[:, :4]) - seq(corr[:, :4])) + (seq(gauss[:, 4:]) - seq(corr[:, 4:]))
    w = (f(2.0) * a) * (s / (s + f(1e-6)))
    sel = np.where((q1 <= q2)[:, None], dq1, dq2)
    gx = _fmaf(alpha, w, -(sel * s)) / nf
    inside = (raw >= f(-20.0)) & (raw <= f(2.0))
    g_ls = np.where(inside, _fmaf(gx, std * z, -(alpha / nf)), f(0.0)).astype(np.float32)
    mq = np.minimum(q1, q2)
    loss = _fmaf(alpha, logp, -mq)
    stats = np.array([_mean32(loss), _mean32(logp), _mean32(mq), alpha], dtype=np.float32)
    out = np.concatenate([gx, g_ls], axis=1)
    for t in (x, a, s, logp, w, gx, g_ls, out):
        assert t.dtype == np.float32
    return out, stats, a, logp


def ent_coef_step_reference(state, logp, step: int, lr: float, target_entropy: float, betas=(0.9, 0.999), eps: float = 1e-8):
    """float64 statement of dockauv_sac_ent_coef_step: SB3's ent_coef_loss = -(log_ent_coef * (logp + target_entropy)).mean() and
    step ``step`` >= 1 of torch.optim.Adam (no weight decay, no amsgrad) on the scalar.  ``state`` = (log_ent_coef, m, v).  Returns
    (new state [3], stats [4]) = (ent_coef_loss, exp(log_ent_coef) before the step, mean(logp + target_entropy), the new
    log_ent_coef); nothing is changed in place."""
    if int(step) < 1:
        raise ValueError("step counts from 1")
    p, m, v = (float(x) for x in np.asarray(state, dtype=np.float64).reshape(3))
    b1, b2 = float(betas[0]), float(betas[1])
    mean = float((np.asarray(logp, dtype=np.float64).reshape(-1) + float(target_entropy)).mean())
    g = -mean
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    step_size, rsq = float(lr) / (1.0 - b1 ** int(step)), 1.0 / np.sqrt(1.0 - b2 ** int(step))
    p_new = p - step_size * (m / (np.sqrt(v) * rsq + float(eps)))
    return np.array([p_new, m, v], dtype=np.float64), np.array([-(p * mean), np.exp(p), mean, p_new], dtype=np.float64)


def ent_coef_mean_float32(logp, target_entropy: float) -> np.float32:
    """the mean dockauv_sac_ent_coef_step forms: the add in float32, the sum in float64, one rounding"""
    return _mean32(np.asarray(logp, dtype=np.float32).reshape(-1) + _F32(target_entropy))


def ent_coef_step_float32(state, mean, step: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8):
    """The exact float32 statement of dockauv_sac_ent_coef_step's update for a given ``mean`` (``ent_coef_mean_float32``, or the
    device's own from stats[2]): the host scalars in double rounded once, then include/dockauv.h's order.  Returns (new state [3]
    float32, ent_coef_loss float32)."""
    f = _F32
    p, m, v = (f(x) for x in np.asarray(state, dtype=np.float32).reshape(3))
    mean = f(mean)
    c1, c2, b2 = f(1.0 - betas[0]), f(1.0 - betas[1]), f(betas[1])
    step_size, rsq = f(lr / (1.0 - betas[0] ** int(step))), f(1.0 / np.sqrt(1.0 - betas[1] ** int(step)))
    g = -mean
    one = lambda x: f(np.asarray(x).reshape(-1)[0])     # (_fmaf returns at least one dimension)
    m = one(_fmaf(c1, g - m, m))
    v = one(_fmaf(c2 * g, g, b2 * v))
    denom = one(_fmaf(np.sqrt(v), rsq, f(eps)))
    p_new = p - step_size * (m / denom)
    out = np.array([p_new, m, v])
    assert out.dtype == np.float32
    return out, -(p * mean)


class SquashedGaussianMLP:
    """SB3 1.5's ``sac.policies.Actor`` with ``use_sde=False``: latent = MLP(obs) over ``layers`` (one or two hidden (W, b)
    pairs, torch.nn.Linear layout), mu = W_mu latent + b_mu, log_std = clamp(W_ls latent + b_ls, -20, 2) with ``mu`` = (W_mu,
    b_mu) and ``log_std_head`` = (W_ls, b_ls); x = mu + exp(log_std) z, a = tanh(x).  A host object holding the arrays;
    ``make_sac_actor`` puts it on the device.  Widths up to 128: SB3's default net_arch [256, 256] does not fit the kernel."""

    LOG_STD_MIN, LOG_STD_MAX, EPS = -20.0, 2.0, 1e-6

    def __init__(self, layers, mu, log_std_head, hidden_act: str = "relu"):
        if len(layers) not in (1, 2):
            raise ValueError("SquashedGaussianMLP takes one or two hidden layers")
        if hidden_act not in ("tanh", "relu"):
            raise ValueError("hidden_act must be 'tanh' or 'relu'")
        c = lambda Wb: (np.ascontiguousarray(Wb[0], dtype=np.float32), np.ascontiguousarray(Wb[1], dtype=np.float32))
        self.layers, self.mu, self.log_std_head = [c(Wb) for Wb in layers], c(mu), c(log_std_head)
        n = self.layers[0][0].shape[1]
        for W, b in self.layers:
            if W.ndim != 2 or b.shape != (W.shape[0],) or W.shape[1] != n:
                raise ValueError("layer shapes do not chain: W [out, in], b [out]")
            n = W.shape[0]
        for W, b in (self.mu, self.log_std_head):
            if W.ndim != 2 or W.shape[1] != n or b.shape != (W.shape[0],) or W.shape[0] != self.mu[0].shape[0]:
                raise ValueError("mu and log_std_head: W [n_out, n_last], b [n_out], the same n_out")
        self.hidden_act = hidden_act

    n_in = property(lambda self: int(self.layers[0][0].shape[1]))
    n_out = property(lambda self: int(self.mu[0].shape[0]))
    n_hidden = property(lambda self: [int(W.shape[0]) for W, _ in self.layers])

    @classmethod
    def from_torch(cls, module_or_state_dict, hidden_act: Optional[str] = None):
        """An SB3-style actor: a module with ``latent_pi`` (Sequential of Linear / ReLU / Tanh), ``mu`` and ``log_std`` (Linear),
        or its state dict (``latent_pi.{0,2}.*``, ``mu.*``, ``log_std.*``; the hidden activation is then ``hidden_act``, SB3's
        SAC default: relu).  Needs no stable-baselines3 import."""
        def arr(t):
            return (t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)).astype(np.float32)

        if isinstance(module_or_state_dict, dict) or hasattr(module_or_state_dict, "keys"):
            sd = module_or_state_dict
            layers = [(arr(sd[f"latent_pi.{i}.weight"]), arr(sd[f"latent_pi.{i}.bias"])) for i in (0, 2) if f"latent_pi.{i}.weight" in sd]
            if not layers or "mu.weight" not in sd or "log_std.weight" not in sd:
                raise ValueError("state dict needs latent_pi.0.*, mu.* and log_std.*")
            return cls(layers, (arr(sd["mu.weight"]), arr(sd["mu.bias"])), (arr(sd["log_std.weight"]), arr(sd["log_std.bias"])),
                       hidden_act or "relu")
        m = module_or_state_dict
        layers, acts = [], []
        for sub in m.latent_pi:
            name = type(sub).__name__
            if name == "Linear":
                layers.append((arr(sub.weight), arr(sub.bias)))
            elif name in ("Tanh", "ReLU"):
                acts.append(name.lower())
            else:
                raise ValueError(f"unsupported layer {name} in latent_pi: Linear, Tanh and ReLU are")
        if len(acts) != len(layers) or len(set(acts)) != 1 or (hidden_act and hidden_act != acts[0]):
            raise ValueError("latent_pi: expected Linear-act[-Linear-act] with one kind of activation")
        return cls(layers, (arr(m.mu.weight), arr(m.mu.bias)), (arr(m.log_std.weight), arr(m.log_std.bias)), acts[0])

    # ------------------------------------------------------------------------------------------ statements
    def forward_reference(self, obs, z=None):
        """float64, by SB3's formulas as they are written: returns (a, log_prob, mu, log_std) with a = tanh(mu + exp(log_std) z)
        (``z`` None: the deterministic action, z = 0) and log_prob = sum_j Normal(mu_j, std_j).log_prob(x_j) -
        sum_j log(1 - a_j^2 + 1e-6).  obs [..., n_in], z [..., n_out]."""
        x = np.asarray(obs, dtype=np.float64)
        for W, b in self.layers:
            x = _act(x @ W.astype(np.float64).T + b.astype(np.float64), self.hidden_act)
        mu = x @ self.mu[0].astype(np.float64).T + self.mu[1].astype(np.float64)
        ls = np.clip(x @ self.log_std_head[0].astype(np.float64).T + self.log_std_head[1].astype(np.float64),
                     self.LOG_STD_MIN, self.LOG_STD_MAX)
        z = np.zeros_like(mu) if z is None else np.asarray(z, dtype=np.float64)
        std = np.exp(ls)
        pre = mu + std * z
        a = np.tanh(pre)
        gauss = -((pre - mu) ** 2) / (2.0 * std ** 2) - ls - 0.5 * np.log(2.0 * np.pi)
        return a, gauss.sum(axis=-1) - np.log(1.0 - a * a + self.EPS).sum(axis=-1), mu, ls

    def _both_heads(self) -> "MLPPolicy":
        """the plain network whose raw output is (mu | raw log_std): the two heads stacked as one output layer"""
        return MLPPolicy(self.layers + [(np.concatenate([self.mu[0], self.log_std_head[0]]), np.concatenate([self.mu[1], self.log_std_head[1]]))],
                         self.hidden_act, "none")

    def heads_reference(self, obs) -> np.ndarray:
        """float64 statement of dockauv_sac_actor_forward_rows: obs [..., n_in] -> [..., 2 n_out] = (mu | W_ls latent + b_ls), the
        log-std head before its clamp."""
        return self._both_heads().forward_reference(obs)

    def backward_reference(self, obs, grad_out):
        """float64 statement of dockauv_sac_actor_backward: obs [B, n_in], grad_out [B, 2 n_out] on ``heads_reference``.  Returns
        (dW1, db1[, dW2, db2], dW_mu, db_mu, dW_ls, db_ls), summed over the rows, torch.nn.Linear layout."""
        *hidden, dW, db = self._both_heads().backward_reference(obs, np.asarray(grad_out, dtype=np.float64).reshape(-1, 2 * self.n_out))
        n = self.n_out
        return tuple(hidden) + (dW[:n], db[:n], dW[n:], db[n:])

    def forward_float32(self, obs, z=None):
        """The kernel's epilogue expressions in float32 NumPy arrays (include/dockauv.h states them; the matrix products are
        NumPy's float32): (a, log_prob).  What float32 can do on these expressions -- the yardstick of the device's
        log-probability error, never a compute path."""
        f = _F32
        x = np.asarray(obs, dtype=np.float32)
        for W, b in self.layers:
            x = _act(x @ W.T + b, self.hidden_act).astype(np.float32)
        mu = (x @ self.mu[0].T + self.mu[1]).astype(np.float32)
        ls = np.clip((x @ self.log_std_head[0].T + self.log_std_head[1]).astype(np.float32), f(self.LOG_STD_MIN), f(self.LOG_STD_MAX))
        z = np.zeros_like(mu) if z is None else np.asarray(z, dtype=np.float32)
        pre = _fmaf(np.exp(ls), z, mu)
        a = np.tanh(pre)
        gauss = _fmaf(f(-0.5) * z, z, -(ls + f(0.918938533)))
        e = np.exp(f(-2.0) * np.abs(pre))
        d = f(1.0) + e
        corr = np.log(f(4.0) * e / (d * d) + f(1e-6))
        lo = gauss[..., :4].sum(axis=-1, dtype=np.float32) - corr[..., :4].sum(axis=-1, dtype=np.float32)
        hi = gauss[..., 4:].sum(axis=-1, dtype=np.float32) - corr[..., 4:].sum(axis=-1, dtype=np.float32)
        return a, (lo + hi).astype(np.float32)

    def plain_twin(self, out_act: str = "tanh", log_std=None) -> "MLPPolicy":
        """The plain ``MLPPolicy`` with the same hidden layers and W3 = W_mu, b3 = b_mu: its deterministic actions are this
        actor's bit for bit, and with W_ls = 0, b_ls = ``log_std`` so are the stochastic ones."""
        return MLPPolicy(self.layers + [self.mu], self.hidden_act, out_act, log_std)

    # ------------------------------------------------------------------------------------------ C ABI
    def shape_desc(self) -> _capi.SacActorDesc:
        d = _capi.SacActorDesc()
        d.struct_size = C.sizeof(_capi.SacActorDesc)
        d.precision = _capi.F32
        d.n_in, d.n_out = self.n_in, self.n_out
        d.n_hidden[0] = self.n_hidden[0]
        d.n_hidden[1] = self.n_hidden[1] if len(self.n_hidden) == 2 else 0
        d.hidden_act = _ACTS[self.hidden_act]
        return d

    def host_desc(self, seed: int = 0, env_id_offset: int = 0) -> _capi.SacActorDesc:
        """dockauv_sac_actor_desc over this object's host arrays (which must outlive the call that reads it)"""
        d = self.shape_desc()
        d.pointers_on_device = 0
        ptrs = [a.ctypes.data for Wb in self.layers for a in Wb]
        if len(self.layers) == 1:
            ptrs += [None, None]
        d.W1, d.b1, d.W2, d.b2 = ptrs
        d.W_mu, d.b_mu = self.mu[0].ctypes.data, self.mu[1].ctypes.data
        d.W_ls, d.b_ls = self.log_std_head[0].ctypes.data, self.log_std_head[1].ctypes.data
        d.seed, d.env_id_offset = int(seed), int(env_id_offset)
        return d


class DevicePolicy:
    """A dockauv_policy of one BatchedDocking3d handle (made by ``make_policy``, ``make_value``, ``make_sac_actor`` or
    ``make_q``): the handle plus what a reload needs.  ``role``: "actor", "value", "sac" or "q"."""

    def __init__(self, ptr: C.c_void_p, mlp, seed: int, env_id_offset: int, value_role: bool = False, role: Optional[str] = None):
        self.ptr, self.seed, self.env_id_offset = ptr, int(seed), int(env_id_offset)
        self.role = role or ("value" if value_role else "actor")
        self.value_role = self.role == "value"   # a critic (make_value): dockauv_value_create
        self.shape = mlp.shape_desc()
        self.n_in, self.n_hidden, self.n_out = mlp.n_in, mlp.n_hidden, mlp.n_out
        self.has_log_std = self.role == "sac" or (self.role == "actor" and mlp.log_std is not None)


class DeviceOptim:
    """A dockauv_optim of one BatchedDocking3d handle (made by ``make_optim``): Adam's moments and step count for one actor,
    its log_std and (optionally) one critic."""

    def __init__(self, ptr: C.c_void_p, policy: DevicePolicy, value: Optional[DevicePolicy]):
        self.ptr, self.policy, self.value = ptr, policy, value
