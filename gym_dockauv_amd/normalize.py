"""
Reward normalisation: SB3's ``VecNormalize(norm_reward=True, norm_obs=False)`` -- every reward divided by the running standard
deviation of the discounted return, then clipped -- for the collector of ``TorchDocking3d``.

The compute path is the HIP kernels behind ``dockauv_rewnorm_scan`` (include/dockauv.h states the arithmetic and the order of
the sums; csrc/dockauv_rewnorm.hip).  This module holds the NumPy statement of those kernels for tests and ports -- never a
compute path, the role ``monitor.episode_scan_reference`` has for the monitor -- and the host objects of a normaliser.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

INITIAL_STATE = (0.0, 1.0, 1e-4, 0.0)   # running mean, var, count (SB3's RunningMeanStd(epsilon=1e-4)), reserved


def reward_normalize_reference(reward, done, gamma, clip_reward, epsilon, state, carry, training=True):
    """NumPy statement of dockauv_rewnorm_scan.  reward, done: [K, N] (the reward and done columns of the packed rows; done is
    anything that compares > 0.5 where an episode ended); gamma and clip_reward are rounded to float32 as the C ABI takes them,
    epsilon is float64; state: float64 [>= 3] = running mean, var, count; carry: float32 [N], every env's discounted return
    before step 0.  For k = 0 .. K - 1:

        ret = carry * gamma + reward[k]             float32, a rounded product then a rounded sum
        discounted[k] = ret;  carry = 0 where done[k], else ret
        batch_mean, batch_var = moments of discounted[k] over the N envs, float64 (``math.fsum``; the variance about the mean)
        RunningMeanStd.update_from_moments(batch_mean, batch_var, N)
        den = sqrt(var + epsilon);  reward_norm[k] = float32(clip(float64(reward[k]) / den, -clip_reward, clip_reward))

    ``training`` False: only the last line, with the ``var`` handed in for every k; state and carry come back unchanged.

    Returns a dict: ``reward_norm`` float32 [K, N], ``discounted`` float32 [K, N] (zeros when not training), ``step_stats``
    float64 [K, 4] = batch_mean, batch_var, var after step k, den (only den when not training), ``state`` float64 [4] and
    ``carry`` float32 [N] (new arrays)."""
    r = np.asarray(reward, dtype=np.float32)
    d = np.asarray(done) > 0.5
    if r.ndim != 2 or d.shape != r.shape:
        raise ValueError("reward, done: [K, N]")
    K, N = r.shape
    g = np.float32(gamma)
    clip = float(np.float32(clip_reward))
    eps = float(epsilon)
    if not (0.0 <= float(g) <= 1.0) or not clip > 0.0 or not eps >= 0.0:
        raise ValueError("gamma in [0, 1], clip_reward > 0, epsilon >= 0")
    st = np.asarray(state, dtype=np.float64).reshape(-1)
    if st.size < 3:
        raise ValueError("state: [mean, var, count(, reserved)]")
    mean, var, count = float(st[0]), float(st[1]), float(st[2])
    c = np.array(carry, dtype=np.float32).reshape(-1)
    if c.shape != (N,):
        raise ValueError("carry: [N]")
    disc = np.zeros((K, N), dtype=np.float32)
    norm = np.zeros((K, N), dtype=np.float32)
    stats = np.zeros((K, 4), dtype=np.float64)
    n = float(N)
    for k in range(K):
        if training:
            prod = (c * g).astype(np.float32)                # float32 x float32: one rounding
            ret = (prod + r[k]).astype(np.float32)           # and one more
            disc[k] = ret
            c = np.where(d[k], np.float32(0.0), ret).astype(np.float32)
            x = ret.astype(np.float64)
            batch_mean = math.fsum(x) / n
            q = x - batch_mean
            batch_var = math.fsum(q * q) / n
            delta = batch_mean - mean
            tot = count + n
            mean = mean + (delta * n) / tot
            m2 = (var * count + batch_var * n) + (((delta * delta) * count) * n) / tot
            var = m2 / tot
            count = tot
            stats[k, :3] = batch_mean, batch_var, var
        den = math.sqrt(var + eps)
        stats[k, 3] = den
        norm[k] = np.clip(r[k].astype(np.float64) / den, -clip, clip).astype(np.float32)
    return dict(reward_norm=norm, discounted=disc, step_stats=stats, state=np.array([mean, var, count, 0.0], dtype=np.float64),
                carry=c)


class DeviceRewardNormalizer:
    """A dockauv_rewnorm of one BatchedDocking3d handle (made by ``make_reward_normalizer``): the state and the carries."""

    def __init__(self, ptr: C.c_void_p, gamma: float, clip_reward: float, epsilon: float):
        self.ptr = ptr
        self.gamma, self.clip_reward, self.epsilon = float(gamma), float(clip_reward), float(epsilon)


class RewardNormalizer:
    """What ``TorchDocking3d.make_reward_normalizer`` returns.  ``scan`` queues dockauv_rewnorm_scan on the current stream and
    never synchronises, ``collect(..., reward_norm=rn)`` queues it inside the collection; ``mean`` / ``var`` / ``count`` and
    ``state_dict`` copy a few bytes to the host and are the places that do.  ``training``: True updates the statistics and the
    carries with every scan, False (evaluation, SB3's ``training=False``) only applies the current ones.  ``normalized`` /
    ``discounted`` [K, N] float32 and ``step_stats`` [K, 4] float64: views of the latest scan's outputs (None before the first;
    ``discounted`` and the first three columns of ``step_stats`` belong to the latest training scan of that K)."""

    reward_normalize_reference = staticmethod(reward_normalize_reference)

    def __init__(self, env, gamma: float, clip_reward: float = 10.0, epsilon: float = 1e-8):
        self.env = env
        self.handle = env.batch.make_reward_normalizer(gamma, clip_reward, epsilon)
        self.gamma, self.clip_reward, self.epsilon = float(gamma), float(clip_reward), float(epsilon)
        self.training = True
        self.normalized = self.discounted = self.step_stats = None
        self._bufs = {}

    # ---------------------------------------------------------------------------------------------- state
    def _tensors(self):
        """(state float64 [4], carry float32 [N]): torch views of the normaliser's own device arrays"""
        from .parallel import _DevArray
        torch, env = self.env.torch, self.env
        s_ptr, c_ptr = env.batch.reward_normalizer_state(self.handle)
        return (torch.as_tensor(_DevArray(s_ptr, (4,), "<f8"), device=env.device),
                torch.as_tensor(_DevArray(c_ptr, (env.num_envs,), "<f4"), device=env.device))

    def _state_host(self):
        return self._tensors()[0].cpu().numpy()

    @property
    def mean(self) -> float:
        return float(self._state_host()[0])

    @property
    def var(self) -> float:
        return float(self._state_host()[1])

    @property
    def count(self) -> float:
        return float(self._state_host()[2])

    def carries(self):
        """a copy of the discounted-return carries float32 [N] at this point of the current stream"""
        return self._tensors()[1].clone()

    def state_dict(self) -> dict:
        """host copies of everything a checkpoint needs (synchronises)"""
        state, carry = self._tensors()
        return dict(state=state.cpu().numpy().copy(), carry=carry.cpu().numpy().copy(), gamma=self.gamma,
                    clip_reward=self.clip_reward, epsilon=self.epsilon, training=bool(self.training))

    def load_state_dict(self, sd: dict) -> None:
        """the statistics and carries of ``state_dict`` back in, ordered on the current stream; gamma, clip_reward and epsilon
        are fixed at creation and must be the checkpoint's"""
        for name in ("gamma", "clip_reward", "epsilon"):
            if name in sd and np.float32(sd[name]) != np.float32(getattr(self, name)):
                raise ValueError(f"{name}: the checkpoint has {sd[name]}, this normaliser {getattr(self, name)}")
        torch = self.env.torch
        state, carry = self._tensors()
        s = np.asarray(sd["state"], dtype=np.float64).reshape(-1)
        c = np.asarray(sd["carry"], dtype=np.float32).reshape(-1)
        if s.shape != (4,) or c.shape != (self.env.num_envs,):
            raise ValueError(f"state: [4], carry: [{self.env.num_envs}]")
        state.copy_(torch.from_numpy(s.copy()))
        carry.copy_(torch.from_numpy(c.copy()))
        if "training" in sd:
            self.training = bool(sd["training"])

    def reset(self) -> None:
        """statistics <- (0, 1, 1e-4), carries <- 0, on the current stream (dockauv_rewnorm_reset)"""
        self.env.batch.reward_normalizer_reset(self.handle, stream=self.env.torch.cuda.current_stream().cuda_stream)

    # ---------------------------------------------------------------------------------------------- scans
    def _workspace(self, K: int) -> dict:
        """reward_norm, discounted [K, N] and step_stats [K, 4] of a scan of K steps (what ``collect`` keeps per K)"""
        torch, env = self.env.torch, self.env
        return dict(norm=torch.zeros((K, env.num_envs), device=env.device, dtype=torch.float32),
                    disc=torch.zeros((K, env.num_envs), device=env.device, dtype=torch.float32),
                    stats=torch.zeros((K, 4), device=env.device, dtype=torch.float64))

    def _attach(self, ws: dict) -> None:
        self.normalized, self.discounted, self.step_stats = ws["norm"], ws["disc"], ws["stats"]

    def scan(self, rows):
        """rows: contiguous float32 [K, N, n_obs + 2] packed rows on the env's device, the steps that follow the ones the
        carries have seen.  Queues dockauv_rewnorm_scan (four launches when ``training``, one otherwise) and returns
        ``normalized`` [K, N], a buffer this normaliser owns and reuses for the next scan of the same K."""
        env, torch = self.env, self.env.torch
        N, stride = env.num_envs, env.n_obs + 2
        if rows.dim() != 3 or rows.shape[0] < 1 or rows.device != env.device or rows.dtype != torch.float32 \
                or not rows.is_contiguous() or tuple(rows.shape[1:]) != (N, stride):
            raise ValueError(f"rows must be a contiguous float32 [K, {N}, {stride}] tensor on {env.device}")
        K = int(rows.shape[0])
        ws = self._bufs.get(K)
        if ws is None:
            ws = self._bufs[K] = self._workspace(K)
        env.batch.reward_normalizer_scan_device(self.handle, rows.data_ptr(), K, ws["norm"].data_ptr(), ws["disc"].data_ptr(),
                                                ws["stats"].data_ptr(), training=self.training,
                                                stream=torch.cuda.current_stream().cuda_stream)
        self._attach(ws)
        return ws["norm"]
