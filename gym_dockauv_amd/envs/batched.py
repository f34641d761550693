"""
BatchedDocking3d -- N independent docking3d environments stepped by one HIP kernel launch per step.

Host-side mirror of the reference's ``BaseDocking3d`` (envs/docking3d.py:31-704) for a batch: same config schema,
same observation / reward / done semantics, same reset draw order; SB3 ``VecEnv`` call surface (``num_envs``,
``reset``, ``step_async`` / ``step_wait`` / ``step``, auto-reset with ``infos[i]["terminal_observation"]``).
All arithmetic of ``step`` happens in libdockauv.so (gym_dockauv_amd/csrc); this class only builds the C config,
stages episodes (scenario generation stays on the host, like the reference's ``reset``) and moves pointers.
"""
from __future__ import annotations

import copy
import ctypes as C
import types
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

from .. import _capi, scenarios
from ..config.env_config import BASE_CONFIG
from ..objects.radar import RadarLayout
from ..objects.vehicle_models import VehicleModel, make_vehicle

META_DATA_REWARD = ["Nav_delta_d", "Nav_delta_theta", "Nav_delta_psi", "Att_phi", "Att_theta", "Thetadot",
                    "obstacle_avoid", "action", "Done-Goal_reached", "Done-out_pos", "Done-out_att", "Done-max_t",
                    "Done-collision"]                      # envs/docking3d.py:160-178
META_DATA_DONE = META_DATA_REWARD[8:]
_NO_INFO = types.MappingProxyType({})


class Box:
    """Minimal stand-in for gym.spaces.Box (gym is optional); same attributes the reference sets
    (envs/docking3d.py:116-125)."""

    def __init__(self, low, high, dtype=np.float32):
        self.low = np.asarray(low, dtype=dtype)
        self.high = np.asarray(high, dtype=dtype)
        self.dtype = np.dtype(dtype)
        self.shape = self.low.shape

    def sample(self):
        return np.random.uniform(self.low, self.high).astype(self.dtype)

    def contains(self, x):
        x = np.asarray(x)
        return x.shape == self.shape and bool(np.all(x >= self.low) and np.all(x <= self.high))

    def __repr__(self):
        return f"Box({self.low.min()}, {self.high.max()}, {self.shape}, {self.dtype.name})"


def make_box(low, high, dtype=np.float32):
    try:
        import gym  # type: ignore
        return gym.spaces.Box(low=np.asarray(low, dtype=dtype), high=np.asarray(high, dtype=dtype), dtype=dtype)
    except Exception:
        return Box(low, high, dtype)


class BatchedDocking3d:
    """
    :param env_config: dict with the reference's key schema (config/env_config.py)
    :param num_envs: envs on this device
    :param scenario: one of scenarios.SCENARIOS (the reference's env class names + "SphereDocking3d")
    :param device: HIP device ordinal
    :param precision: "f32" (product path) or "f64" (validation instantiation of the same kernels)
    :param auto_reset: VecEnv semantics (in-kernel reset from the host-staged pool); False = gym.Env semantics
    :param rng: "per_env" -> one legacy ``RandomState`` per env, reference draw order incl. the per-step normal burn
                (parity with ``reset(seed)`` of the reference); "batched" -> one vectorised generator (throughput)
    :param vehicles: optional per-env vehicle names for a mixed batch, e.g. ["BlueROV2", "LAUV", ...]
    :param sort_vehicles: mixed batches: keep the envs KIND-SORTED on the device ("for mixed vehicles keep
                each GPU's range vehicle-sorted": every 64-env group but one is then homogeneous, config 5 15.3 -> 14.5 us per
                step).  ``perm[j]`` = the caller's index of the env in device row j (stable: the caller's order within a
                kind), ``inv_perm`` its inverse.  Everything that takes or returns HOST arrays -- step(), reset_envs(),
                get_field / set_field, seeds, infos, episode storage -- stays in the CALLER's order (rows are permuted at the
                C-ABI boundary); the device-pointer entry points (step_device, make_step_sequence, ...) work on device rows:
                row j of the action tensor and of the packed rows belongs to caller env ``perm[j]``.
    """

    def __init__(self, env_config: dict = BASE_CONFIG, num_envs: int = 1, scenario: str = "SimpleDocking3d",
                 device: int = 0, precision: str = "f32", auto_reset: bool = True, rng: str = "per_env",
                 vehicles: Optional[Sequence[str]] = None, max_capsules: Optional[int] = None,
                 max_spheres: Optional[int] = None, threads_per_group: int = 0,
                 vehicle_models: Optional[Sequence[VehicleModel]] = None, current_mu: float = scenarios.CURRENT_MU,
                 reset_mode: Optional[str] = None, device_seed: int = 0, _force_general: bool = False,
                 device_noise: bool = False, sort_vehicles: bool = False):
        if scenario not in scenarios.SCENARIOS:
            raise KeyError(f"Not valid scenario, available options are {scenarios.SCENARIOS}")
        self.config = copy.deepcopy(env_config)
        self.scenario = scenario
        self.num_envs = int(num_envs)
        self.device = int(device)
        self.precision = precision
        # reset_mode: "none" (gym.Env semantics), "pool" (in-kernel reset from host-staged episodes: reference draw
        # order, parity), "device" (in-kernel scenario generation with a Philox counter RNG: throughput)
        if reset_mode is None:
            reset_mode = "pool" if auto_reset else "none"
        if reset_mode not in ("none", "pool", "device"):
            raise ValueError("reset_mode must be 'none', 'pool' or 'device'")
        self.reset_mode = reset_mode
        self.device_seed = int(device_seed)
        # device_noise: the kernel draws the white noise of each env's Gauss-Markov current itself (sigma per env:
        # F_CURRENT_SIGMA, objects/current.py:31,88) whenever step() is not given a noise array
        self.device_noise = bool(device_noise)
        self._force_general = bool(_force_general)   # test hook: general kinetics expressions
        self.auto_reset = reset_mode != "none"
        self.rng_mode = rng
        self.current_mu = float(current_mu)
        self.threads_per_group = int(threads_per_group)
        self._lib = _capi.load_library()
        self._np_t = np.float64 if precision == "f64" else np.float32

        # vehicles
        if vehicle_models is not None:
            self.vehicle_models = list(vehicle_models)
        elif vehicles is not None:
            names = list(dict.fromkeys(vehicles))
            if names not in (["BlueROV2", "LAUV"], ["LAUV", "BlueROV2"], ["BlueROV2"], ["LAUV"]):
                raise ValueError("mixed batches support BlueROV2 + LAUV")
            self.vehicle_models = [make_vehicle(n) for n in (["BlueROV2", "LAUV"] if len(names) == 2 else names)]
        else:
            self.vehicle_models = [make_vehicle(self.config["vehicle"])]
        self.auv = self.vehicle_models[0]          # `env.auv.u_bound` is what train.py touches (train.py:102,191)
        self.n_u = max(int(m.u_bound.shape[0]) for m in self.vehicle_models)
        if vehicles is not None and len(self.vehicle_models) == 2:
            self.vehicle_id = np.array([0 if v == "BlueROV2" else 1 for v in vehicles], dtype=np.float64)
            if self.vehicle_id.shape[0] != self.num_envs:
                raise ValueError("len(vehicles) must equal num_envs")
        else:
            self.vehicle_id = np.zeros(self.num_envs)
        # device row j <- caller env perm[j] (identity unless sort_vehicles reorders a mixed batch)
        self.perm = np.arange(self.num_envs, dtype=np.int64)
        if sort_vehicles and len(self.vehicle_models) == 2:
            self.perm = np.argsort(self.vehicle_id, kind="stable").astype(np.int64)
        self.inv_perm = np.empty_like(self.perm)
        self.inv_perm[self.perm] = np.arange(self.num_envs, dtype=np.int64)
        self._sorted = bool((self.perm != np.arange(self.num_envs)).any())

        # ray fan (envs/docking3d.py:104-105)
        self.radar_args = self.config["radar"]
        self.radar = RadarLayout(**self.radar_args)
        self.n_obs_without_radar = 16
        self.n_observations = self.n_obs_without_radar + self.radar.n_rays_reduced
        self.n_rewards = 13
        self.n_cont_rewards = 8
        self.meta_data_reward = META_DATA_REWARD
        self.meta_data_done = META_DATA_DONE

        self.max_capsules = scenarios.N_CAPSULES[scenario] if max_capsules is None else int(max_capsules)
        self.max_spheres = scenarios.N_SPHERES[scenario] if max_spheres is None else int(max_spheres)

        # spaces (envs/docking3d.py:116-125)
        ub = np.zeros((self.n_u, 2))
        ub[: self.auv.u_bound.shape[0]] = self.auv.u_bound
        self.action_space = make_box(ub[:, 0], ub[:, 1], np.float32)
        obs_low = -np.ones(self.n_observations)
        obs_low[0] = 0
        obs_low[self.n_obs_without_radar:] = 0
        self.observation_space = make_box(obs_low, np.ones(self.n_observations), np.float32)

        self._handle = C.c_void_p()
        self._ray_table = self.radar.ray_table()
        cfg = self._build_config()
        rc = self._lib.dockauv_create(C.byref(cfg), self.device, C.byref(self._handle))
        _capi.check(self._lib, None, rc, "dockauv_create")
        assert self._lib.dockauv_n_obs(self._handle) == self.n_observations
        self.threads_in_use = int(self._lib.dockauv_threads_per_group(self._handle))   # (the library's choice when 0 was asked)
        if len(self.vehicle_models) == 2:
            self.set_field(_capi.F_VEHICLE_ID, self.vehicle_id[:, None])

        # host-side episode bookkeeping
        N = self.num_envs
        self._seeds: Optional[np.ndarray] = None
        self._seed_pending = False      # seeds given (seed() / reset(seed=...)) and not yet applied by a reset
        self._rs: List[Optional[np.random.RandomState]] = [None] * N
        self._gen = np.random.default_rng()
        self._steps_since_reset = np.zeros(N, dtype=np.int64)     # per-step normal draws to burn (current.py:88)
        self.episode = np.zeros(N, dtype=np.int64)
        self.t_total_steps = 0
        self._actions = None
        self._static_spheres: Optional[np.ndarray] = None
        # host output buffers (host-pointer path)
        self._obs = np.zeros((N, self.n_observations), dtype=np.float32)
        self._rew = np.zeros(N, dtype=self._np_t)
        self._done = np.zeros(N, dtype=np.uint8)
        self._terms = np.zeros((N, 13), dtype=self._np_t)
        self._cond = np.zeros(N, dtype=np.uint8)
        self._nav = np.zeros((N, 4), dtype=self._np_t)
        self._ray = np.zeros((N, self.radar.n_rays), dtype=self._np_t)
        self._termobs = np.zeros((N, self.n_observations), dtype=np.float32)
        self._statedot = np.zeros((N, 12), dtype=self._np_t)
        self.episode_storage = None          # BatchEpisodeStorage (enable_episode_storage)

    # ------------------------------------------------------------------------------------------ config
    def _build_config(self) -> _capi.Config:
        c = self.config
        cfg = _capi.Config()
        cfg.struct_size = C.sizeof(_capi.Config)
        cfg.abi_version = _capi.ABI_VERSION
        cfg.n_envs = self.num_envs
        cfg.precision = _capi.F64 if self.precision == "f64" else _capi.F32
        cfg.n_vehicles = len(self.vehicle_models)
        cfg.reset_mode = {"none": _capi.RESET_NONE, "pool": _capi.RESET_POOL, "device": _capi.RESET_DEVICE}[self.reset_mode]
        cfg.scenario = _capi.SCN[self.scenario]
        cfg.max_timesteps = int(c["max_timesteps"])
        cfg.reward_set = int(c["reward_set"])
        cfg.max_capsules = self.max_capsules
        cfg.max_spheres = self.max_spheres
        cfg.n_v, cfg.n_h = self.radar.n_vertical, self.radar.n_horizontal
        cfg.blocksize_reduce = self.radar.blocksize_reduce
        cfg.envs_per_group = -1 if self._force_general else 0
        cfg.threads_per_group = self.threads_per_group
        cfg.seed = self.device_seed
        cfg.t_step_size = float(c["t_step_size"])
        cfg.lowpass_T1 = 0.2
        cfg.current_mu = self.current_mu
        cfg.max_dist_from_goal = float(c["max_dist_from_goal"])
        cfg.max_attitude = float(c["max_attitude"])
        cfg.dist_goal_reached_tol = float(c["dist_goal_reached_tol"])
        cfg.vel_max[:] = [float(c[k]) for k in ("u_max", "v_max", "w_max", "p_max", "q_max", "r_max")]
        cfg.safety_radius = float(self.auv.safety_radius)
        rf = c["reward_factors"]
        cfg.w_d, cfg.w_delta_theta, cfg.w_delta_psi = rf["w_d"], rf["w_delta_theta"], rf["w_delta_psi"]
        cfg.w_phi, cfg.w_theta, cfg.w_Thetadot, cfg.w_oa = rf["w_phi"], rf["w_theta"], rf["w_Thetadot"], rf["w_oa"]
        cfg.w_done[:] = [rf["w_goal"], rf["w_deltad_max"], rf["w_Theta_max"], rf["w_t_max"], rf["w_col"]]
        arf = np.broadcast_to(np.asarray(c["action_reward_factors"], dtype=float), (self.n_u,))
        w = np.zeros(_capi.MAX_U)
        w[: self.n_u] = arf
        cfg.action_reward_factors[:] = w.tolist()
        cfg.radar_max_dist = self.radar.max_dist
        cfg.radar_alpha_max, cfg.radar_beta_max = self.radar.alpha_max, self.radar.beta_max
        cfg.device_noise = 1 if self.device_noise else 0
        cfg.ray_table = self._ray_table.ctypes.data_as(C.POINTER(C.c_double))
        for i, m in enumerate(self.vehicle_models):
            cfg.vehicle[i] = m.to_capi()
        return cfg

    # ------------------------------------------------------------------------------------------ field I/O
    def _raw_set(self, field: int, a: np.ndarray, first: int) -> None:
        rc = self._lib.dockauv_set_field(self._handle, field, first, a.shape[0], a.ctypes.data_as(C.c_void_p))
        _capi.check(self._lib, self._handle, rc, "dockauv_set_field")

    def _raw_runs(self, field: int, dev_idx: np.ndarray, values: np.ndarray) -> None:
        """rows `values` to DEVICE rows dev_idx (any order), as contiguous runs"""
        order = np.argsort(dev_idx, kind="stable")
        dev_idx, values = dev_idx[order], np.ascontiguousarray(values[order])
        breaks = np.flatnonzero(np.diff(dev_idx) != 1) + 1
        for run_idx, run_val in zip(np.split(dev_idx, breaks), np.split(values, breaks)):
            self._raw_set(field, np.ascontiguousarray(run_val), int(run_idx[0]))

    def set_field(self, field: int, values: np.ndarray, first: int = 0) -> None:
        """Rows of envs [first, first + len(values)) in the caller's order (float64 [count][width])."""
        a = np.ascontiguousarray(values, dtype=np.float64)
        if a.ndim == 1:
            a = a[:, None]
        width = self._lib.dockauv_field_width(self._handle, field)
        if width == 0 and a.size == 0:
            return
        if a.shape[1] != width:
            raise ValueError(f"field {field}: expected width {width}, got {a.shape[1]}")
        if self._sorted:
            self._raw_runs(field, self.inv_perm[first:first + a.shape[0]], a)
        else:
            self._raw_set(field, a, first)

    def get_field(self, field: int, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Rows of envs [first, first + count) in the caller's order."""
        count = self.num_envs - first if count is None else count
        width = self._lib.dockauv_field_width(self._handle, field)
        out = np.zeros((count, max(width, 0)), dtype=np.float64)
        if width > 0 and count > 0:
            dev = self.inv_perm[first:first + count] if self._sorted else None
            lo, n = (int(dev.min()), int(dev.max()) - int(dev.min()) + 1) if self._sorted else (first, count)
            raw = out if not self._sorted else np.zeros((n, width), dtype=np.float64)
            rc = self._lib.dockauv_get_field(self._handle, field, lo, n, raw.ctypes.data_as(C.c_void_p))
            _capi.check(self._lib, self._handle, rc, "dockauv_get_field")
            if self._sorted:
                out = raw[dev - lo]
        return out

    def _set_rows(self, field: int, idx: np.ndarray, values: np.ndarray) -> None:
        """set_field for an arbitrary index set (caller's env indices), as contiguous runs of device rows."""
        idx = np.asarray(idx)
        if idx.size == 0:
            return
        values = np.asarray(values, dtype=np.float64)
        if values.ndim == 1:
            values = values[:, None]
        self._raw_runs(field, self.inv_perm[idx] if self._sorted else idx, values)

    # convenience views used by callers of the reference (datastorage.py:298-300, train.py:191)
    @property
    def state(self) -> np.ndarray:
        return self.get_field(_capi.F_STATE)

    @property
    def position(self) -> np.ndarray:
        return self.state[:, 0:3]

    @property
    def attitude(self) -> np.ndarray:
        return self.state[:, 3:6]

    @property
    def u(self) -> np.ndarray:
        return self.get_field(_capi.F_U)[:, : self.n_u]

    @property
    def t_steps(self) -> np.ndarray:
        return self.get_field(_capi.F_TSTEPS)[:, 0].astype(np.int64)

    @property
    def cumulative_reward(self) -> np.ndarray:
        return self.get_field(_capi.F_CUM_REWARD)[:, 0]

    @property
    def goal_location(self) -> np.ndarray:
        return self.get_field(_capi.F_GOAL)[:, 0:3]

    # ------------------------------------------------------------------------------------------ episodes
    def seed(self, seed: Optional[Union[int, Sequence[int]]] = None) -> List[Optional[int]]:
        """VecEnv.seed: env i gets seed + i (SB3 convention) or seed[i]."""
        N = self.num_envs
        if seed is None:
            self._seeds = None
            self._seed_pending = False
            return [None] * N
        seeds = np.asarray(seed)
        if seeds.ndim == 0:
            seeds = int(seeds) + np.arange(N)
        self._seeds = seeds.astype(np.int64)
        self._seed_pending = True
        return self._seeds.tolist()

    def _uniforms(self, idx: np.ndarray, reseed: bool) -> np.ndarray:
        k = scenarios.N_DRAWS[self.scenario]
        if self.rng_mode == "batched":
            return self._gen.random((idx.size, k))
        U = np.empty((idx.size, k))
        for j, i in enumerate(idx):
            if reseed and self._seeds is not None:
                self._rs[i] = np.random.RandomState(int(self._seeds[i]))      # docking3d.py:296-298
            elif self._rs[i] is None:
                self._rs[i] = np.random.RandomState()
            elif self._steps_since_reset[i] > 0:
                self._rs[i].normal(size=int(self._steps_since_reset[i]))       # Q11: one normal per elapsed step
            U[j] = self._rs[i].random_sample(k)
        self._steps_since_reset[idx] = 0
        return U

    def generate_episodes(self, idx: np.ndarray, reseed: bool = False) -> Dict[str, np.ndarray]:
        ep = scenarios.episodes_from_uniforms(self.scenario, self._uniforms(idx, reseed), self.config["max_attitude"],
                                              self.config["max_dist_from_goal"], self.max_capsules, self.max_spheres)
        if self.scenario == "SphereDocking3d":
            if self._static_spheres is None:
                self._static_spheres = np.stack([
                    scenarios.sphere_shell(np.random.RandomState(10_000 + i), np.zeros(3), self.max_spheres).reshape(-1)
                    for i in range(self.num_envs)])
            ep["spheres"] = self._static_spheres[idx]
        return ep

    def load_episodes(self, idx: np.ndarray, ep: Dict[str, np.ndarray], pool: bool = False) -> None:
        """Write episodes into the live arrays (reset) or into the next-episode pool."""
        idx = np.asarray(idx)
        if pool:
            self._set_rows(_capi.F_POOL_POSE, idx, ep["pose"])
            self._set_rows(_capi.F_POOL_GOAL, idx, ep["goal"])
            self._set_rows(_capi.F_POOL_CURRENT, idx, ep["current"])
            if self.max_capsules:
                self._set_rows(_capi.F_POOL_CAPSULES, idx, ep["capsules"])
            if self.max_spheres:
                self._set_rows(_capi.F_POOL_SPHERES, idx, ep["spheres"])
            return
        state = np.zeros((idx.size, 12))
        state[:, 0:6] = ep["pose"]
        self._set_rows(_capi.F_STATE, idx, state)
        self._set_rows(_capi.F_GOAL, idx, ep["goal"])
        self._set_rows(_capi.F_CURRENT, idx, ep["current"])
        if self.max_capsules:
            self._set_rows(_capi.F_CAPSULES, idx, ep["capsules"])
        if self.max_spheres:
            self._set_rows(_capi.F_SPHERES, idx, ep["spheres"])

    def reset(self, seed: Optional[Union[int, Sequence[int]]] = None, return_info: bool = False, options=None):
        """Reset every env (BaseDocking3d.reset, docking3d.py:222-322).  Returns the all-zero observation (Q8)."""
        if seed is not None:
            self.seed(seed)
        idx = np.arange(self.num_envs)
        if self.episode_storage is not None:
            self.episode_storage.on_reset(idx)
        rc = self._lib.dockauv_reset_envs(self._handle, 0, self.num_envs)
        _capi.check(self._lib, self._handle, rc, "dockauv_reset_envs")
        # the streams are (re)seeded by the reset that follows seed() / comes with seed=..., and by that one only: a later
        # reset() without a seed draws on from where the stream stands (envs/docking3d.py:296-298 seeds only `if seed is not
        # None`; round 4: every reset() re-seeded -- the replay of the reference's multi-episode runs found it)
        self.load_episodes(idx, self.generate_episodes(idx, reseed=self._seed_pending))
        self._seed_pending = False
        self.episode += 1
        if self.reset_mode == "pool":
            self.load_episodes(idx, self.generate_episodes_for_pool(idx), pool=True)
        obs = np.zeros((self.num_envs, self.n_observations), dtype=np.float32)
        if return_info:
            return obs, [{} for _ in range(self.num_envs)]
        return obs

    def generate_episodes_for_pool(self, idx: np.ndarray) -> Dict[str, np.ndarray]:
        """Pool entries are drawn when they are CONSUMED in parity mode (the burn count is only known then); at
        staging time we park a valid placeholder drawn from the batched generator."""
        if self.rng_mode == "batched":
            return self.generate_episodes(idx)
        k = scenarios.N_DRAWS[self.scenario]
        ep = scenarios.episodes_from_uniforms(self.scenario, self._gen.random((idx.size, k)), self.config["max_attitude"],
                                              self.config["max_dist_from_goal"], self.max_capsules, self.max_spheres)
        if self.scenario == "SphereDocking3d" and self._static_spheres is not None:
            ep["spheres"] = self._static_spheres[idx]
        return ep

    def reset_envs(self, idx: Sequence[int], episodes: Optional[Dict[str, np.ndarray]] = None) -> None:
        """gym.Env-style reset of selected envs (auto_reset=False callers)."""
        idx = np.asarray(idx, dtype=np.int64)
        if idx.size == 0:
            return
        if self.episode_storage is not None:
            self.episode_storage.on_reset(idx)
        dev = np.sort(self.inv_perm[idx]) if self._sorted else idx
        breaks = np.flatnonzero(np.diff(dev) != 1) + 1
        for run in np.split(dev, breaks):
            rc = self._lib.dockauv_reset_envs(self._handle, int(run[0]), int(run.size))
            _capi.check(self._lib, self._handle, rc, "dockauv_reset_envs")
        self.load_episodes(idx, episodes if episodes is not None else self.generate_episodes(idx))
        self.episode[idx] += 1

    # ------------------------------------------------------------------------------------------ step
    def _io(self, actions: np.ndarray, noise: Optional[np.ndarray], extras: bool) -> _capi.StepIO:
        io = _capi.StepIO()
        io.actions = actions.ctypes.data
        io.noise = noise.ctypes.data if noise is not None else None
        io.obs = self._obs.ctypes.data
        io.reward = self._rew.ctypes.data
        io.done = self._done.ctypes.data
        io.conditions = self._cond.ctypes.data
        io.terminal_obs = self._termobs.ctypes.data if self.auto_reset else None
        if extras:
            io.reward_terms = self._terms.ctypes.data
            io.nav = self._nav.ctypes.data
            io.ray_dist = self._ray.ctypes.data
            io.state_dot = self._statedot.ctypes.data
        return io

    def step_async(self, actions: np.ndarray) -> None:
        self._actions = actions

    def step_wait(self):
        return self.step(self._actions)

    def step(self, actions: np.ndarray, noise: Optional[np.ndarray] = None, extras: bool = False):
        """
        One step of every env through the host-pointer entry point (dockauv_step_host).
        Returns (obs [N, n_obs] float32, reward [N], done [N] bool, infos).
        """
        a = np.ascontiguousarray(actions, dtype=self._np_t).reshape(self.num_envs, self.n_u)
        w = None if noise is None else np.ascontiguousarray(noise, dtype=self._np_t).reshape(self.num_envs)
        if self._sorted:   # the caller's rows -> device rows
            a = np.ascontiguousarray(a[self.perm])
            w = None if w is None else np.ascontiguousarray(w[self.perm])
        self._io_keepalive = (a, w)
        io = self._io(a, w, extras)
        rc = self._lib.dockauv_step_host(self._handle, C.byref(io))
        _capi.check(self._lib, self._handle, rc, "dockauv_step_host")
        if self._sorted:   # ... and the outputs back into the caller's order
            for buf in (self._obs, self._rew, self._done, self._cond) + ((self._termobs,) if self.auto_reset else ()) + \
                       ((self._terms, self._nav, self._ray, self._statedot) if extras else ()):
                buf[...] = buf[self.inv_perm]
        self.t_total_steps += 1
        self._steps_since_reset += 1
        done = self._done.astype(bool)
        if self.episode_storage is not None:
            self.episode_storage.after_step(done)
        # VecEnv contract: one info mapping per env.  Envs that did not finish share ONE read-only empty mapping
        # (building 65 536 dicts per step costs more than the step); finished envs get their own dict.
        infos: List[dict] = [_NO_INFO] * self.num_envs
        didx = np.flatnonzero(done)
        for i in didx:
            cond = int(self._cond[i])
            cidx = [k for k in range(5) if cond >> k & 1]
            infos[i] = {"conditions_true": cidx, "conditions_true_info": [META_DATA_DONE[k] for k in cidx],
                        "collision": bool(cond & 16), "goal_reached": bool(cond & 1), "done": True,
                        "episode_number": int(self.episode[i])}
            if self.auto_reset:
                infos[i]["terminal_observation"] = self._termobs[i].copy()
        if self.reset_mode == "device" and didx.size:
            self.episode[didx] += 1
        elif self.reset_mode == "pool" and didx.size:
            if self.rng_mode == "per_env":
                # parity mode: the kernel reset these envs from a placeholder; overwrite with the episode the
                # reference would have drawn now (stream burned by the elapsed steps), then restage the pool
                self.reset_envs_in_place(didx)
            elif self.rng_mode == "batched":
                self.load_episodes(didx, self.generate_episodes(didx), pool=True)
            self.episode[didx] += 1
        return self._obs.copy(), self._rew.copy(), done, infos

    def reset_envs_in_place(self, idx: np.ndarray) -> None:
        ep = self.generate_episodes(idx)
        self.load_episodes(idx, ep)

    # extras of the last step (parity tests, logging): last_reward_arr, conditions, nav errors, ray distances
    @property
    def last_reward_arr(self) -> np.ndarray:
        return self._terms

    @property
    def conditions(self) -> np.ndarray:
        return (self._cond[:, None] >> np.arange(5)[None, :] & 1).astype(bool)

    @property
    def nav_errors(self) -> np.ndarray:
        return self._nav

    @property
    def intersec_dist(self) -> np.ndarray:
        return self._ray

    @property
    def state_dot(self) -> np.ndarray:
        """AUVSim._state_dot of the last step(extras=True) (objects/auvsim.py:108)."""
        return self._statedot

    # ------------------------------------------------------------------------------------------ episode storage
    def enable_trace(self, env_ids: Sequence[int], capacity: int) -> None:
        """Device ring of the last `capacity` steps of the selected envs (dockauv_trace_enable); [] switches it off."""
        ids = np.ascontiguousarray(sorted(int(i) for i in env_ids), dtype=np.int32)
        dev = np.ascontiguousarray(np.sort(self.inv_perm[ids]), dtype=np.int32) if (self._sorted and ids.size) else ids
        rc = self._lib.dockauv_trace_enable(self._handle, dev.ctypes.data_as(C.c_void_p), int(dev.size), int(capacity))
        _capi.check(self._lib, self._handle, rc, "dockauv_trace_enable")
        # ring row j belongs to the j-th DEVICE row selected: the caller's ids in that order
        self._trace_ids = np.ascontiguousarray(self.perm[dev], dtype=np.int32) if (self._sorted and ids.size) else ids

    def trace_steps(self) -> int:
        return int(self._lib.dockauv_trace_steps(self._handle))

    def read_trace(self, first_step: int, n_steps: int) -> Dict[str, np.ndarray]:
        """Steps [first_step, first_step + n_steps) of the ring as host arrays [n_steps][n_rows][width]."""
        R = int(self._trace_ids.size)
        out = {"state_pre": np.zeros((n_steps, R, 12)), "state": np.zeros((n_steps, R, 12)),
               "state_dot": np.zeros((n_steps, R, 12)), "u": np.zeros((n_steps, R, _capi.MAX_U)),
               "nu_c": np.zeros((n_steps, R, 3)), "obs": np.zeros((n_steps, R, self.n_observations), dtype=np.float32),
               "reward_terms": np.zeros((n_steps, R, 13)), "conditions": np.zeros((n_steps, R), dtype=np.uint8)}
        rc = self._lib.dockauv_trace_read(self._handle, int(first_step), int(n_steps),
                                          *[out[k].ctypes.data_as(C.c_void_p) for k in
                                            ("state_pre", "state", "state_dot", "u", "nu_c", "obs", "reward_terms", "conditions")])
        _capi.check(self._lib, self._handle, rc, "dockauv_trace_read")
        return out

    def enable_episode_storage(self, env_ids: Sequence[int], path_folder: str, title: str = "", capacity: Optional[int] = None):
        """EpisodeDataStorage (utils/datastorage.py:164-343) for selected envs of the batch: the step kernel records
        their per-step arrays in a device ring; every finished episode of a selected env is written as one pickle
        with the reference's schema (docking3d.py:252-259).  Works for the host path (flushed by step()) and for
        device-resident rollouts (call env.episode_storage.flush() at least every `capacity` steps)."""
        from ..utils.datastorage import BatchEpisodeStorage
        cap = int(capacity or (int(self.config["max_timesteps"]) + 2))
        self.enable_trace(env_ids, cap)
        self.episode_storage = BatchEpisodeStorage(self, path_folder, title, cap)
        return self.episode_storage

    # ------------------------------------------------------------------------------------------ device-pointer path
    @staticmethod
    def _pack_mode(packed) -> int:
        """packed: False / True (float32 rows [obs | reward | done]) / "bf16" (observation columns bfloat16, two per word;
        include/dockauv.h: pack_reward_done = 2)"""
        if packed in ("bf16", 2):
            return 2
        return 1 if packed else 0

    def packed_row_words(self, packed=True) -> int:
        """32-bit words per packed row: n_obs + 2 (float32 rows) or ceil(n_obs / 2) + 2 ("bf16")"""
        return (self.n_observations + 1) // 2 + 2 if self._pack_mode(packed) == 2 else self.n_observations + 2

    def step_device(self, actions_ptr: int, obs_ptr: int, reward_ptr: int = 0, done_ptr: int = 0, stream: int = 0,
                    noise_ptr: int = 0, terminal_obs_ptr: int = 0, conditions_ptr: int = 0, packed: bool = False) -> None:
        """Asynchronous step on device pointers (torch tensors' data_ptr()): no host copies, no sync.
        packed=True: obs_ptr is a float32 [N][n_obs + 2] buffer receiving obs | reward | done per env; packed="bf16": a
        uint32 [N][ceil(n_obs / 2) + 2] buffer, observation columns as bfloat16 pairs (packed_row_words)."""
        io = _capi.StepIO()
        io.actions, io.obs = actions_ptr, obs_ptr
        io.reward, io.done = reward_ptr or None, done_ptr or None
        io.pack_reward_done = self._pack_mode(packed)
        io.noise = noise_ptr or None
        io.terminal_obs = terminal_obs_ptr or None
        io.conditions = conditions_ptr or None
        rc = self._lib.dockauv_step(self._handle, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_step")

    def make_step_sequence(self, actions_ptrs, obs_ptrs, packed: bool = True):
        """Prepare an open-loop sequence of steps on device pointers (step i reads actions_ptrs[i], writes
        obs_ptrs[i]); run it with run_step_sequence().  packed as in step_device."""
        n = len(actions_ptrs)
        if len(obs_ptrs) != n:
            raise ValueError("actions_ptrs and obs_ptrs must have the same length")
        if not packed:
            raise ValueError("make_step_sequence writes packed [obs | reward | done] rows")
        ios = (_capi.StepIO * n)()
        for i in range(n):
            ios[i].actions, ios[i].obs = actions_ptrs[i], obs_ptrs[i]
            ios[i].pack_reward_done = self._pack_mode(packed)
        return ios

    def run_step_sequence(self, ios, stream: int = 0) -> None:
        """Queue every step of a prepared sequence on `stream` (asynchronous, one host call): as resident launches of up to
        64 steps each where the product kernels serve them (include/dockauv.h: dockauv_step_sequence), else back to back."""
        rc = self._lib.dockauv_step_sequence(self._handle, ios, len(ios), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_step_sequence")

    @property
    def step_uses_current(self) -> bool:
        """False while the next plain step runs the lean kernel that leaves the water current out (dockauv_step_uses_current:
        a scenario without current and no non-zero current row written since the handle was created)."""
        return bool(self._lib.dockauv_step_uses_current(self._handle))

    @property
    def step_uses_capsules(self) -> bool:
        """False while the next plain step runs the sphere-only kernel (dockauv_step_uses_capsules: the lean kernel of a BlueROV2
        handle with a ray fan, no capsule slot and at least one sphere slot)."""
        return bool(self._lib.dockauv_step_uses_capsules(self._handle))

    def set_sequence_resident(self, on: bool) -> None:
        """Switch the resident fast path of run_step_sequence (on by default) for this handle."""
        rc = self._lib.dockauv_set_option(self._handle, _capi.OPT_SEQUENCE_RESIDENT, 1 if on else 0)
        _capi.check(self._lib, self._handle, rc, "dockauv_set_option")

    # ------------------------------------------------------------------------------------------ closed loop
    def make_policy(self, mlp, seed: int = 0, env_id_offset: int = 0):
        """Put an ``MLPPolicy`` (gym_dockauv_amd/policy.py) on this handle's device: dockauv_policy_create.  ``seed`` keys the
        exploration noise, ``env_id_offset`` is added to the env index in its counter (shards of one batch)."""
        from ..policy import DevicePolicy
        d = mlp.host_desc(seed, env_id_offset)
        ptr = C.c_void_p()
        rc = self._lib.dockauv_policy_create(self._handle, C.byref(d), C.byref(ptr))
        _capi.check(self._lib, self._handle, rc, "dockauv_policy_create")
        pol = DevicePolicy(ptr, mlp, seed, env_id_offset)
        self._policies = getattr(self, "_policies", []) + [pol]
        return pol

    def make_value(self, mlp):
        """Put a critic -- an ``MLPPolicy`` with one raw output (``MLPPolicy.value_from_torch``) -- on this handle's device:
        dockauv_value_create.  ``load_policy`` and ``destroy_policy`` work on what it returns."""
        from ..policy import DevicePolicy
        d = mlp.host_desc()
        ptr = C.c_void_p()
        rc = self._lib.dockauv_value_create(self._handle, C.byref(d), C.byref(ptr))
        _capi.check(self._lib, self._handle, rc, "dockauv_value_create")
        val = DevicePolicy(ptr, mlp, 0, 0, value_role=True)
        self._policies = getattr(self, "_policies", []) + [val]
        return val

    def make_sac_actor(self, mlp, seed: int = 0, env_id_offset: int = 0):
        """Put a ``SquashedGaussianMLP`` (gym_dockauv_amd/policy.py: SAC's actor) on this handle's device:
        dockauv_sac_actor_create.  ``policy_forward_device``, ``rollout_device`` and ``policy_forward_logp_device`` take what it
        returns, ``load_policy`` reloads it, everything of PPO refuses it."""
        from ..policy import DevicePolicy
        d = mlp.host_desc(seed, env_id_offset)
        ptr = C.c_void_p()
        rc = self._lib.dockauv_sac_actor_create(self._handle, C.byref(d), C.byref(ptr))
        _capi.check(self._lib, self._handle, rc, "dockauv_sac_actor_create")
        pol = DevicePolicy(ptr, mlp, seed, env_id_offset, role="sac")
        self._policies = getattr(self, "_policies", []) + [pol]
        return pol

    def make_q(self, mlp):
        """Put a Q critic -- an ``MLPPolicy`` on [obs | action] (n_in = n_obs + n_u) with one raw output -- on this handle's
        device: dockauv_q_create.  ``load_policy`` and ``destroy_policy`` work on what it returns."""
        from ..policy import DevicePolicy
        d = mlp.host_desc()
        ptr = C.c_void_p()
        rc = self._lib.dockauv_q_create(self._handle, C.byref(d), C.byref(ptr))
        _capi.check(self._lib, self._handle, rc, "dockauv_q_create")
        q = DevicePolicy(ptr, mlp, 0, 0, role="q")
        self._policies = getattr(self, "_policies", []) + [q]
        return q

    def q_forward_device(self, critic, obs_ptr: int, actions_ptr: int, n_rows: int, q_ptr: int, obs_stride: int = 0,
                         act_stride: int = 0, index_ptr: int = 0, stream: int = 0) -> None:
        """q float32 [n_rows] = Q([obs row | action row]) (dockauv_q_forward): rows ``obs_stride`` / ``act_stride`` floats apart
        (0: dense, n_obs / n_u), through the int64 ``index_ptr`` when given -- e.g. the replay ring and a sample's index."""
        io = _capi.QIO()
        io.struct_size = C.sizeof(_capi.QIO)
        io.obs_stride, io.act_stride = int(obs_stride) or self.n_observations, int(act_stride) or self.n_u
        io.obs, io.actions, io.row_index = obs_ptr or None, actions_ptr or None, index_ptr or None
        io.n_rows, io.q = int(n_rows), q_ptr or None
        rc = self._lib.dockauv_q_forward(self._handle, critic.ptr, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_q_forward")

    def sac_actor_forward_rows_device(self, actor, rows_ptr: int, n_rows: int, out_ptr: int, row_stride: int = 0, index_ptr: int = 0,
                                      stream: int = 0) -> None:
        """out float32 [n_rows][2 n_u] = (mu | the raw log_std head, before its clamp) of a squashed-Gaussian actor for observation
        rows ``row_stride`` floats apart (0: dense, n_obs), through the int64 ``index_ptr`` when given
        (dockauv_sac_actor_forward_rows): no noise, no tanh; asynchronous."""
        io = _capi.SacRowsIO()
        io.struct_size = C.sizeof(_capi.SacRowsIO)
        io.row_stride = int(row_stride) or self.n_observations
        io.rows, io.row_index, io.n_rows, io.out = rows_ptr or None, index_ptr or None, int(n_rows), out_ptr or None
        rc = self._lib.dockauv_sac_actor_forward_rows(self._handle, actor.ptr, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_sac_actor_forward_rows")

    def sac_actor_backward_device(self, actor, rows_ptr: int, n_rows: int, grad_out_ptr: int, grad_ptrs, row_stride: int = 0,
                                  index_ptr: int = 0, stream: int = 0) -> None:
        """Gradients of all weights and biases of a squashed-Gaussian actor for grad_out float32 [n_rows][2 n_u] on the output of
        ``sac_actor_forward_rows_device`` (dockauv_sac_actor_backward): ``grad_ptrs`` = (dW1, db1, dW2, db2, dW_mu, db_mu, dW_ls,
        db_ls) device addresses, torch.nn.Linear layout (dW2 / db2 0 with one hidden layer), overwritten; asynchronous."""
        io = _capi.SacActorBackwardIO()
        io.struct_size = C.sizeof(_capi.SacActorBackwardIO)
        io.row_stride = int(row_stride) or self.n_observations
        io.rows, io.row_index, io.n_rows, io.grad_out = rows_ptr or None, index_ptr or None, int(n_rows), grad_out_ptr or None
        io.dW1, io.db1, io.dW2, io.db2, io.dW_mu, io.db_mu, io.dW_ls, io.db_ls = [int(x) or None for x in grad_ptrs]
        rc = self._lib.dockauv_sac_actor_backward(self._handle, actor.ptr, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_sac_actor_backward")

    def q_backward_device(self, critic, obs_ptr: int, actions_ptr: int, n_rows: int, grad_q_ptr: int, grad_ptrs=None,
                          grad_actions_ptr: int = 0, obs_stride: int = 0, act_stride: int = 0, index_ptr: int = 0, stream: int = 0) -> None:
        """A Q critic's backward for grad_q float32 [n_rows] on the rows of ``q_forward_device`` (dockauv_q_backward):
        ``grad_ptrs`` = (dW1, db1, dW2, db2, dW3, db3) device addresses or None, ``grad_actions_ptr`` float32 [n_rows][n_u] or 0
        (dq/da scaled by grad_q); at least one.  With ``grad_ptrs`` None it is one launch that touches no workspace."""
        io = _capi.QBackwardIO()
        io.struct_size = C.sizeof(_capi.QBackwardIO)
        io.obs_stride, io.act_stride = int(obs_stride) or self.n_observations, int(act_stride) or self.n_u
        io.obs, io.actions, io.row_index = obs_ptr or None, actions_ptr or None, index_ptr or None
        io.n_rows, io.grad_q, io.grad_actions = int(n_rows), grad_q_ptr or None, grad_actions_ptr or None
        g = None
        if grad_ptrs is not None:
            g = _capi.PolicyGrads()
            g.struct_size = C.sizeof(_capi.PolicyGrads)
            g.dW1, g.db1, g.dW2, g.db2, g.dW3, g.db3 = [int(x) or None for x in grad_ptrs]
            io.grads = C.pointer(g)
        rc = self._lib.dockauv_q_backward(self._handle, critic.ptr, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_q_backward")

    def backward_workspace(self, policy):
        """(device address or 0, floats) of the partial sums the backward calls of ``policy`` share
        (dockauv_policy_backward_workspace): (0, 0) until the first backward with parameter gradients."""
        ptr, n = C.c_void_p(), C.c_longlong()
        rc = self._lib.dockauv_policy_backward_workspace(policy.ptr, C.byref(ptr), C.byref(n))
        _capi.check(self._lib, self._handle, rc, "dockauv_policy_backward_workspace")
        return int(ptr.value or 0), int(n.value)

    def sac_sample_device(self, actor, heads_ptr: int, n_rows: int, a_ptr: int, logp_ptr: int, t: int = 0, row_offset: int = 0,
                          stream: int = 0) -> None:
        """a float32 [n_rows][n_u] and logp [n_rows] of the squashed-Gaussian actor's sample from heads float32 [n_rows][2 n_u]
        (``sac_actor_forward_rows_device``'s output) with the rows-form normals of counter (row_offset + i, t, j, 5): one launch
        (dockauv_sac_sample); the bits of ``sac_target_device``'s a2 / logp2 for the same rows, t and row_offset."""
        io = _capi.SacSampleIO()
        io.struct_size = C.sizeof(_capi.SacSampleIO)
        io.heads, io.n_rows, io.a, io.logp = heads_ptr or None, int(n_rows), a_ptr or None, logp_ptr or None
        io.t, io.row_offset = int(t) & (2 ** 64 - 1), int(row_offset) & (2 ** 64 - 1)
        rc = self._lib.dockauv_sac_sample(self._handle, actor.ptr, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_sac_sample")

    def sac_critic_head_device(self, q1_critic, q1_ptr: int, q2_ptr: int, y_ptr: int, n_rows: int, grad_q1_ptr: int, grad_q2_ptr: int,
                               stats_ptr: int, stream: int = 0) -> None:
        """SAC's critic loss 0.5 (mse(q1, y) + mse(q2, y)) on float32 [n_rows] arrays: grad_q1 / grad_q2 [n_rows] = (q_k - y) /
        n_rows -- what ``q_backward_device`` takes -- and stats float32 [6] = (critic_loss, mse1, mse2, mean q1, mean q2, mean y):
        one launch (dockauv_sac_critic_head)."""
        io = _capi.SacCriticHeadIO()
        io.struct_size = C.sizeof(_capi.SacCriticHeadIO)
        io.q1, io.q2, io.y, io.n_rows = q1_ptr or None, q2_ptr or None, y_ptr or None, int(n_rows)
        io.grad_q1, io.grad_q2, io.stats = grad_q1_ptr or None, grad_q2_ptr or None, stats_ptr or None
        rc = self._lib.dockauv_sac_critic_head(self._handle, q1_critic.ptr, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_sac_critic_head")

    def sac_actor_head_device(self, actor, heads_ptr: int, q1_pi_ptr: int, q2_pi_ptr: int, dq1_ptr: int, dq2_ptr: int, n_rows: int,
                              grad_out_ptr: int, stats_ptr: int, ent_coef: float = 0.0, log_ent_coef_ptr: int = 0, t: int = 0,
                              row_offset: int = 0, stream: int = 0) -> None:
        """SAC's actor loss mean(alpha logp - min(q1_pi, q2_pi)) for the draw (t, row_offset) of ``sac_sample_device`` on heads:
        grad_out float32 [n_rows][2 n_u] on (mu | raw log-std) with the clamp's mask applied -- what ``sac_actor_backward_device``
        takes -- and stats float32 [4] = (actor_loss, mean logp, mean min q, alpha); q1_pi / q2_pi [n_rows] the critics at the
        sampled action, dq1 / dq2 [n_rows][n_u] their dq/da; alpha = ``ent_coef`` or exp of the device scalar at
        ``log_ent_coef_ptr``: one launch (dockauv_sac_actor_head)."""
        io = _capi.SacActorHeadIO()
        io.struct_size = C.sizeof(_capi.SacActorHeadIO)
        io.ent_coef, io.log_ent_coef = float(ent_coef), log_ent_coef_ptr or None
        io.heads, io.q1_pi, io.q2_pi, io.dq1, io.dq2 = heads_ptr or None, q1_pi_ptr or None, q2_pi_ptr or None, dq1_ptr or None, dq2_ptr or None
        io.n_rows, io.t, io.row_offset = int(n_rows), int(t) & (2 ** 64 - 1), int(row_offset) & (2 ** 64 - 1)
        io.grad_out, io.stats = grad_out_ptr or None, stats_ptr or None
        rc = self._lib.dockauv_sac_actor_head(self._handle, actor.ptr, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_sac_actor_head")

    def sac_ent_coef_step_device(self, state_ptr: int, logp_ptr: int, n_rows: int, step: int, lr: float, target_entropy: float,
                                 betas=(0.9, 0.999), eps: float = 1e-8, before_ptr: int = 0, stats_ptr: int = 0, stream: int = 0) -> None:
        """One Adam step on the learned log_ent_coef for the gradient -mean(logp + target_entropy): state float32 [3] =
        (log_ent_coef, m, v) updated in place, ``step`` the caller's count from 1; ``before_ptr`` (one float) receives log_ent_coef
        as it was, ``stats_ptr`` float32 [4] = (ent_coef_loss, exp(log_ent_coef before), the mean, the new log_ent_coef): one
        launch (dockauv_sac_ent_coef_step).  Not to be captured: the step's bias corrections travel in the kernel arguments."""
        io = _capi.SacEntCoefIO()
        io.struct_size = C.sizeof(_capi.SacEntCoefIO)
        io.target_entropy, io.state, io.logp = float(target_entropy), state_ptr or None, logp_ptr or None
        io.n_rows, io.step, io.lr = int(n_rows), int(step), float(lr)
        io.beta1, io.beta2, io.eps = float(betas[0]), float(betas[1]), float(eps)
        io.before, io.stats = before_ptr or None, stats_ptr or None
        rc = self._lib.dockauv_sac_ent_coef_step(self._handle, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_sac_ent_coef_step")

    def sac_target_device(self, actor, q1_target, q2_target, next_obs_ptr: int, rewards_ptr: int, dones_ptr: int, n_rows: int,
                          gamma: float, a2_ptr: int, logp2_ptr: int, q1_ptr: int, q2_ptr: int, y_ptr: int, ent_coef: float = 0.0,
                          log_ent_coef_ptr: int = 0, t: int = 0, row_offset: int = 0, next_obs_stride: int = 0,
                          column_stride: int = 1, timeouts_ptr: int = 0, index_ptr: int = 0, stream: int = 0) -> None:
        """SAC's TD target in one host call, four launches (dockauv_sac_target): a2, logp2 = actor.sample(next_obs); y = r +
        gamma (1 - d) (min(q1, q2) - alpha logp2), alpha = ``ent_coef`` or exp of the device scalar at ``log_ent_coef_ptr``."""
        io = _capi.SacTargetIO()
        io.struct_size = C.sizeof(_capi.SacTargetIO)
        io.next_obs_stride, io.column_stride = int(next_obs_stride) or self.n_observations, int(column_stride)
        io.gamma, io.ent_coef = float(gamma), float(ent_coef)
        io.next_obs, io.row_index = next_obs_ptr or None, index_ptr or None
        io.rewards, io.dones, io.timeouts, io.log_ent_coef = rewards_ptr or None, dones_ptr or None, timeouts_ptr or None, log_ent_coef_ptr or None
        io.n_rows, io.t, io.row_offset = int(n_rows), int(t) & (2 ** 64 - 1), int(row_offset) & (2 ** 64 - 1)
        io.a2, io.logp2, io.q1, io.q2, io.y = a2_ptr or None, logp2_ptr or None, q1_ptr or None, q2_ptr or None, y_ptr or None
        rc = self._lib.dockauv_sac_target(self._handle, actor.ptr, q1_target.ptr, q2_target.ptr, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_sac_target")

    def load_policy(self, policy, mlp=None, device_ptrs=None, log_std_ptr: int = 0, stream: int = 0) -> None:
        """New weights of the same shapes (an actor's or a critic's): dockauv_policy_load.  Either ``mlp`` (host arrays; the call waits for the copies)
        or ``device_ptrs`` = (W1, b1, W2, b2, W3, b3) device addresses of contiguous float32 arrays (W2 / b2 0 with one
        hidden layer) plus ``log_std_ptr``: no host round trip, ordered on ``stream``.  A Q critic loads like a critic; a
        squashed-Gaussian actor (dockauv_sac_actor_load) takes a ``SquashedGaussianMLP`` or ``device_ptrs`` = (W1, b1, W2, b2,
        W_mu, b_mu, W_ls, b_ls)."""
        if (mlp is None) == (device_ptrs is None):
            raise ValueError("give either mlp or device_ptrs")
        if getattr(policy, "role", None) == "sac":
            if mlp is not None:
                d = mlp.host_desc(policy.seed, policy.env_id_offset)
            else:
                d = _capi.SacActorDesc.from_buffer_copy(policy.shape)
                d.pointers_on_device = 1
                d.W1, d.b1, d.W2, d.b2, d.W_mu, d.b_mu, d.W_ls, d.b_ls = [int(x) or None for x in device_ptrs]
                d.seed, d.env_id_offset = policy.seed, policy.env_id_offset
            rc = self._lib.dockauv_sac_actor_load(policy.ptr, C.byref(d), C.c_void_p(stream or None))
            _capi.check(self._lib, self._handle, rc, "dockauv_sac_actor_load")
            return
        if mlp is not None:
            d = mlp.host_desc(policy.seed, policy.env_id_offset)
        else:
            d = _capi.PolicyDesc.from_buffer_copy(policy.shape)
            d.pointers_on_device = 1
            d.W1, d.b1, d.W2, d.b2, d.W3, d.b3 = [int(x) or None for x in device_ptrs]
            d.log_std = int(log_std_ptr) or None
            d.seed, d.env_id_offset = policy.seed, policy.env_id_offset
        rc = self._lib.dockauv_policy_load(policy.ptr, C.byref(d), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_policy_load")
        policy.has_log_std = bool(d.log_std) and getattr(policy, "role", "value" if getattr(policy, "value_role", False) else "actor") == "actor"

    def policy_forward_device(self, policy, rows_ptr: int, actions_ptr: int, t: int = 0, stochastic: bool = False,
                              stream: int = 0) -> None:
        """Asynchronous actor forward on device pointers: rows float32 [N][n_obs + 2] (packed rows; only the observation
        columns are read), actions float32 [N][n_u]."""
        rc = self._lib.dockauv_policy_forward(self._handle, policy.ptr, C.c_void_p(rows_ptr or None), C.c_void_p(actions_ptr or None),
                                              int(t), 1 if stochastic else 0, C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_policy_forward")

    def rollout_device(self, policy, rows_in_ptr: int, rows_out_ptr: int, actions_out_ptr: int, n_steps: int, t0: int = 0,
                       stochastic: bool = False, stream: int = 0, terminal_obs_ptr: int = 0) -> None:
        """n_steps x (policy, step) queued by one host call (dockauv_rollout): rows_out [n_steps][N][n_obs + 2], actions_out
        [n_steps][N][n_u], terminal_obs [n_steps][N][n_obs] or 0.  Asynchronous; raises like poll_status()."""
        rc = self._lib.dockauv_rollout(self._handle, policy.ptr, C.c_void_p(rows_in_ptr or None), C.c_void_p(rows_out_ptr or None),
                                       C.c_void_p(actions_out_ptr or None), C.c_void_p(terminal_obs_ptr or None), int(n_steps),
                                       int(t0), 1 if stochastic else 0, C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_rollout")

    def policy_forward_logp_device(self, policy, rows_ptr: int, actions_ptr: int, log_prob_ptr: int, t: int = 0,
                                   stochastic: bool = False, stream: int = 0) -> None:
        """policy_forward_device that also writes log_prob float32 [N]: the log-probability of the drawn actions
        (dockauv_policy_forward_logp; needs a log_std and a raw output)."""
        rc = self._lib.dockauv_policy_forward_logp(self._handle, policy.ptr, C.c_void_p(rows_ptr or None), C.c_void_p(actions_ptr or None),
                                                   C.c_void_p(log_prob_ptr or None), int(t), 1 if stochastic else 0,
                                                   C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_policy_forward_logp")

    def value_forward_device(self, value, rows_ptr: int, n_rows: int, values_ptr: int, stream: int = 0) -> None:
        """Asynchronous critic forward on device pointers: values float32 [n_rows] of n_rows packed rows [n_obs + 2], any
        number of them (dockauv_value_forward)."""
        rc = self._lib.dockauv_value_forward(self._handle, value.ptr, C.c_void_p(rows_ptr or None), int(n_rows),
                                             C.c_void_p(values_ptr or None), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_value_forward")

    def gae_device(self, rows_out_ptr: int, values_ptr: int, n_steps: int, gamma: float, gae_lambda: float, advantages_ptr: int,
                   returns_ptr: int, stream: int = 0) -> None:
        """GAE over the rows of a rollout (dockauv_gae): rows_out [K][N][n_obs + 2], values [K + 1][N] -> advantages, returns
        [K][N]; asynchronous."""
        rc = self._lib.dockauv_gae(self._handle, C.c_void_p(rows_out_ptr or None), C.c_void_p(values_ptr or None), int(n_steps),
                                   float(gamma), float(gae_lambda), C.c_void_p(advantages_ptr or None), C.c_void_p(returns_ptr or None),
                                   C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_gae")

    def _collect_io(self, rows_in_ptr: int, rows_out_ptr: int, actions_out_ptr: int, n_steps: int, gamma: float, gae_lambda: float,
                    t0: int, stochastic: bool, terminal_obs_ptr: int, log_prob_ptr: int, values_ptr: int, advantages_ptr: int,
                    returns_ptr: int):
        io = _capi.CollectIO()
        io.struct_size = C.sizeof(_capi.CollectIO)
        io.n_steps = int(n_steps)
        io.rows_in, io.rows_out, io.actions_out = rows_in_ptr or None, rows_out_ptr or None, actions_out_ptr or None
        io.terminal_obs, io.log_prob = terminal_obs_ptr or None, log_prob_ptr or None
        io.values, io.advantages, io.returns = values_ptr or None, advantages_ptr or None, returns_ptr or None
        io.t0, io.stochastic = int(t0), 1 if stochastic else 0
        io.gamma, io.gae_lambda = float(gamma), float(gae_lambda)
        return io

    def collect_device(self, policy, value, rows_in_ptr: int, rows_out_ptr: int, actions_out_ptr: int, n_steps: int,
                       gamma: float = 0.99, gae_lambda: float = 0.95, t0: int = 0, stochastic: bool = True, stream: int = 0,
                       terminal_obs_ptr: int = 0, log_prob_ptr: int = 0, values_ptr: int = 0, advantages_ptr: int = 0,
                       returns_ptr: int = 0) -> None:
        """One PPO iteration's collection queued by one host call (dockauv_collect): the rollout (log_prob [K][N] when asked
        for), V of the K + 1 observation sets -> values [K + 1][N], GAE -> advantages, returns [K][N].  ``value`` None: rollout
        and log-probabilities only.  Asynchronous; raises like poll_status()."""
        io = self._collect_io(rows_in_ptr, rows_out_ptr, actions_out_ptr, n_steps, gamma, gae_lambda, t0, stochastic, terminal_obs_ptr,
                              log_prob_ptr, values_ptr, advantages_ptr, returns_ptr)
        rc = self._lib.dockauv_collect(self._handle, policy.ptr, value.ptr if value is not None else None, C.byref(io),
                                       C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_collect")

    def truncation_slots(self, n_steps: int) -> int:
        """Slots per env that hold every time-limit truncation of ``n_steps`` steps (dockauv_truncation_slots):
        n_steps // (max_timesteps + 1) + 1."""
        n = self._lib.dockauv_truncation_slots(self._handle, int(n_steps))
        if n < 1:
            _capi.check(self._lib, self._handle, n, "dockauv_truncation_slots")
        return int(n)

    def _truncation_io(self, n_steps: int, n_slots: int, rows_out_ptr: int, terminal_obs_ptr: int, length_carry_ptr: int,
                       trunc_step_ptr: int, trunc_row_ptr: int, values_ptr: int = 0, v_terminal_ptr: int = 0,
                       advantages_ptr: int = 0, returns_ptr: int = 0, gamma: float = 0.0, gae_lambda: float = 0.0):
        io = _capi.TruncationIO()
        io.struct_size = C.sizeof(_capi.TruncationIO)
        io.n_steps, io.n_slots = int(n_steps), int(n_slots)
        io.gamma, io.gae_lambda = float(gamma), float(gae_lambda)
        io.rows_out, io.terminal_obs, io.values = rows_out_ptr or None, terminal_obs_ptr or None, values_ptr or None
        io.length_carry, io.trunc_step, io.trunc_row = length_carry_ptr or None, trunc_step_ptr or None, trunc_row_ptr or None
        io.v_terminal, io.advantages, io.returns = v_terminal_ptr or None, advantages_ptr or None, returns_ptr or None
        return io

    def truncation_scan_device(self, rows_out_ptr: int, terminal_obs_ptr: int, n_steps: int, n_slots: int, length_carry_ptr: int,
                               trunc_step_ptr: int, trunc_row_ptr: int, stream: int = 0) -> None:
        """The time-limit truncations inside rows_out [K][N][n_obs + 2] (dockauv_truncation_scan): env's s-th truncated step ->
        trunc_step int32 [n_slots][N] (-1: unused) and its terminal_obs row -> trunc_row int64 [n_slots][N]; length_carry int32
        [N] is read (steps of every env's episode before step 0) and written back.  Asynchronous."""
        io = self._truncation_io(n_steps, n_slots, rows_out_ptr, terminal_obs_ptr, length_carry_ptr, trunc_step_ptr, trunc_row_ptr)
        rc = self._lib.dockauv_truncation_scan(self._handle, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_truncation_scan")

    def gae_truncated_device(self, value, rows_out_ptr: int, terminal_obs_ptr: int, values_ptr: int, n_steps: int, n_slots: int,
                             gamma: float, gae_lambda: float, length_carry_ptr: int, trunc_step_ptr: int, trunc_row_ptr: int,
                             v_terminal_ptr: int, advantages_ptr: int, returns_ptr: int, stream: int = 0) -> None:
        """``gae_device`` with SB3's truncation bootstrap (dockauv_gae_truncated): the scan of ``truncation_scan_device``, V of
        the truncated steps' terminal observations -> v_terminal float32 [n_slots][N], then GAE with reward + gamma *
        v_terminal at those steps.  Asynchronous."""
        io = self._truncation_io(n_steps, n_slots, rows_out_ptr, terminal_obs_ptr, length_carry_ptr, trunc_step_ptr, trunc_row_ptr,
                                 values_ptr, v_terminal_ptr, advantages_ptr, returns_ptr, gamma, gae_lambda)
        rc = self._lib.dockauv_gae_truncated(self._handle, value.ptr, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_gae_truncated")

    def collect_truncated_device(self, policy, value, rows_in_ptr: int, rows_out_ptr: int, actions_out_ptr: int, n_steps: int,
                                 n_slots: int, terminal_obs_ptr: int, values_ptr: int, advantages_ptr: int, returns_ptr: int,
                                 length_carry_ptr: int, trunc_step_ptr: int, trunc_row_ptr: int, v_terminal_ptr: int,
                                 gamma: float = 0.99, gae_lambda: float = 0.95, t0: int = 0, stochastic: bool = True,
                                 stream: int = 0, log_prob_ptr: int = 0) -> None:
        """``collect_device`` with the truncation bootstrap (dockauv_collect_truncated): length_carry <- the handle's step
        counters, the rollout, the two value launches, then ``gae_truncated_device``'s three launches in place of the GAE
        launch.  Needs a critic and terminal_obs.  Asynchronous; raises like poll_status()."""
        cio = self._collect_io(rows_in_ptr, rows_out_ptr, actions_out_ptr, n_steps, gamma, gae_lambda, t0, stochastic, terminal_obs_ptr,
                               log_prob_ptr, values_ptr, advantages_ptr, returns_ptr)
        tio = self._truncation_io(n_steps, n_slots, rows_out_ptr, terminal_obs_ptr, length_carry_ptr, trunc_step_ptr, trunc_row_ptr,
                                  values_ptr, v_terminal_ptr, advantages_ptr, returns_ptr, gamma, gae_lambda)
        rc = self._lib.dockauv_collect_truncated(self._handle, policy.ptr, value.ptr if value is not None else None, C.byref(cio),
                                                 C.byref(tio), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_collect_truncated")

    def policy_forward_rows_device(self, policy, rows_ptr: int, n_rows: int, out_ptr: int, index_ptr: int = 0, stream: int = 0) -> None:
        """The MLP's output before its output activation, without noise, for any rows (dockauv_policy_forward_rows; an actor or
        a critic): rows float32 packed rows [n_obs + 2], index int64 [n_rows] or 0 (row r is rows[index[r]]), out float32
        [n_rows][n_out]; asynchronous."""
        rc = self._lib.dockauv_policy_forward_rows(self._handle, policy.ptr, C.c_void_p(rows_ptr or None), C.c_void_p(index_ptr or None),
                                                   int(n_rows), C.c_void_p(out_ptr or None), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_policy_forward_rows")

    def policy_backward_device(self, policy, rows_ptr: int, n_rows: int, grad_out_ptr: int, grad_ptrs, index_ptr: int = 0,
                               stream: int = 0) -> None:
        """Gradients of all weights and biases for grad_out float32 [n_rows][n_out] on the output of
        ``policy_forward_rows_device`` (dockauv_policy_backward): ``grad_ptrs`` = (dW1, db1, dW2, db2, dW3, db3) device
        addresses of float32 arrays in torch.nn.Linear layout (dW2 / db2 0 with one hidden layer), overwritten; asynchronous."""
        g = _capi.PolicyGrads()
        g.struct_size = C.sizeof(_capi.PolicyGrads)
        g.dW1, g.db1, g.dW2, g.db2, g.dW3, g.db3 = [int(x) or None for x in grad_ptrs]
        rc = self._lib.dockauv_policy_backward(self._handle, policy.ptr, C.c_void_p(rows_ptr or None), C.c_void_p(index_ptr or None),
                                               int(n_rows), C.c_void_p(grad_out_ptr or None), C.byref(g), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_policy_backward")

    def ppo_head_device(self, policy, n_rows: int, mean_ptr: int, v_ptr: int, actions_ptr: int, log_prob_old_ptr: int,
                        advantages_ptr: int, returns_ptr: int, grad_mean_ptr: int, grad_v_ptr: int, grad_log_std_ptr: int,
                        stats_ptr: int, clip_range: float, vf_coef: float, ent_coef: float, normalize_advantage: bool = True,
                        index_ptr: int = 0, stream: int = 0) -> None:
        """The PPO head on a minibatch of n_rows rows (dockauv_ppo_head; ``policy`` is the actor, whose log_std is used): mean
        float32 [n_rows][n_u] and v float32 [n_rows] (0: no critic, then grad_v 0 too) are the networks' outputs, the row arrays
        are read at index[r] (int64 [n_rows] or 0); writes grad_mean [n_rows][n_u], grad_v [n_rows], grad_log_std [n_u] and
        stats [8] (loss, policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction, advantage mean and std); asynchronous."""
        io = _capi.PPOHeadIO()
        io.struct_size = C.sizeof(_capi.PPOHeadIO)
        io.normalize_advantage = 1 if normalize_advantage else 0
        io.mean, io.v = mean_ptr or None, v_ptr or None
        io.actions, io.log_prob_old = actions_ptr or None, log_prob_old_ptr or None
        io.advantages, io.returns = advantages_ptr or None, returns_ptr or None
        io.row_index, io.n_rows = index_ptr or None, int(n_rows)
        io.clip_range, io.vf_coef, io.ent_coef = float(clip_range), float(vf_coef), float(ent_coef)
        io.grad_mean, io.grad_v, io.grad_log_std = grad_mean_ptr or None, grad_v_ptr or None, grad_log_std_ptr or None
        io.stats = stats_ptr or None
        rc = self._lib.dockauv_ppo_head(self._handle, policy.ptr, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_ppo_head")

    def make_optim(self, policy, value=None, betas=(0.9, 0.999), eps: float = 1e-5, max_grad_norm: float = 0.5):
        """Adam with gradient-norm clipping for ``policy`` (an actor with a log_std), its log_std and ``value`` (a critic, or
        None): dockauv_optim_create.  The moments start at zero; ``max_grad_norm`` <= 0: no clipping.  ``close`` destroys it
        before the policies."""
        from ..policy import DeviceOptim
        d = _capi.OptimDesc()
        d.struct_size = C.sizeof(_capi.OptimDesc)
        d.beta1, d.beta2, d.eps, d.max_grad_norm = float(betas[0]), float(betas[1]), float(eps), float(max_grad_norm)
        ptr = C.c_void_p()
        rc = self._lib.dockauv_optim_create(self._handle, policy.ptr, value.ptr if value is not None else None, C.byref(d), C.byref(ptr))
        _capi.check(self._lib, self._handle, rc, "dockauv_optim_create")
        opt = DeviceOptim(ptr, policy, value)
        self._optims = getattr(self, "_optims", []) + [opt]
        return opt

    def optim_step_device(self, opt, lr: float, actor_param_ptrs, log_std_ptr: int, actor_grad_ptrs, grad_log_std_ptr: int,
                          critic_param_ptrs=None, critic_grad_ptrs=None, stats_ptr: int = 0, stream: int = 0) -> None:
        """One clipped Adam step on device pointers (dockauv_optim_step): ``*_ptrs`` = (W1, b1, W2, b2, W3, b3) addresses of
        contiguous float32 arrays in torch.nn.Linear layout (W2 / b2 0 with one hidden layer; the critic's None without one),
        the parameters updated in place, the gradients only read; stats float32 [2] or 0 (norm before clipping, coef).  Both
        networks hold the new weights afterwards (no ``load_policy`` needed); asynchronous."""
        io = _capi.OptimIO()
        io.struct_size = C.sizeof(_capi.OptimIO)
        io.lr = float(lr)
        for dst, src in ((io.actor_params, actor_param_ptrs), (io.actor_grads, actor_grad_ptrs),
                         (io.critic_params, critic_param_ptrs), (io.critic_grads, critic_grad_ptrs)):
            for i, x in enumerate(src if src is not None else [0] * 6):
                dst[i] = int(x) or None
        io.log_std, io.grad_log_std, io.stats = log_std_ptr or None, grad_log_std_ptr or None, stats_ptr or None
        rc = self._lib.dockauv_optim_step(self._handle, opt.ptr, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_optim_step")
        opt.policy.has_log_std = True

    def optim_state(self, opt):
        """(device address of m, of v, number of elements of each, steps taken): dockauv_optim_state.  m and v are float32 in
        the order actor W1 b1 W2 b2 W3 b3, log_std, critic W1 b1 W2 b2 W3 b3."""
        m, v, n, t = C.c_void_p(), C.c_void_p(), C.c_longlong(), C.c_longlong()
        rc = self._lib.dockauv_optim_state(opt.ptr, C.byref(m), C.byref(v), C.byref(n), C.byref(t))
        _capi.check(self._lib, self._handle, rc, "dockauv_optim_state")
        return int(m.value or 0), int(v.value or 0), int(n.value), int(t.value)

    def permutation_device(self, seed: int, epoch: int, n: int, out_ptr: int, stream: int = 0) -> None:
        """out int64 [n] <- the keyed permutation P_{seed, epoch} of 0 .. n - 1 (dockauv_permutation, stated exactly by
        ``MLPPolicy.permutation_reference``); asynchronous."""
        rc = self._lib.dockauv_permutation(self._handle, int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1), int(n),
                                           C.c_void_p(out_ptr or None), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_permutation")

    def ppo_update_device(self, opt, rows_ptr: int, n_rows: int, batch_size: int, n_epochs: int, lr: float, actions_ptr: int,
                          log_prob_old_ptr: int, advantages_ptr: int, returns_ptr: int, stats_ptr: int, actor_param_ptrs,
                          log_std_ptr: int, actor_grad_ptrs, grad_log_std_ptr: int, critic_param_ptrs=None, critic_grad_ptrs=None, *,
                          clip_range: float, vf_coef: float, ent_coef: float, normalize_advantage: bool = True,
                          clip_range_vf: float = 0.0, values_old_ptr: int = 0, target_kl: float = 0.0, seed: int = 0,
                          first_epoch: int = 0, stream: int = 0) -> None:
        """SB3's PPO.train loop queued by one host call (dockauv_ppo_update): ``n_epochs`` passes over the ``n_rows`` packed rows
        at ``rows_ptr`` in minibatches of ``batch_size`` shuffled by ``permutation_device(seed, first_epoch + e, n_rows)``; the
        row arrays are float32 [n_rows][n_u] / [n_rows]; the parameter and gradient pointers as in ``optim_step_device``; stats
        float32 [n_epochs][n_minibatches][12].  ``clip_range_vf`` / ``target_kl`` 0: off.  Asynchronous; with ``target_kl`` the
        optimiser's step count is read back by the next call that needs it."""
        io = _capi.PPOUpdateIO()
        io.struct_size = C.sizeof(_capi.PPOUpdateIO)
        io.normalize_advantage = 1 if normalize_advantage else 0
        io.rows = rows_ptr or None
        io.actions, io.log_prob_old = actions_ptr or None, log_prob_old_ptr or None
        io.advantages, io.returns, io.values_old = advantages_ptr or None, returns_ptr or None, values_old_ptr or None
        io.n_rows, io.batch_size, io.n_epochs = int(n_rows), int(batch_size), int(n_epochs)
        io.seed, io.first_epoch = int(seed) & (2 ** 64 - 1), int(first_epoch) & (2 ** 64 - 1)
        io.clip_range, io.clip_range_vf, io.vf_coef, io.ent_coef = float(clip_range), float(clip_range_vf), float(vf_coef), float(ent_coef)
        io.target_kl = float(target_kl)
        io.opt.struct_size = C.sizeof(_capi.OptimIO)
        io.opt.lr = float(lr)
        for dst, src in ((io.opt.actor_params, actor_param_ptrs), (io.opt.actor_grads, actor_grad_ptrs),
                         (io.opt.critic_params, critic_param_ptrs), (io.opt.critic_grads, critic_grad_ptrs)):
            for i, x in enumerate(src if src is not None else [0] * 6):
                dst[i] = int(x) or None
        io.opt.log_std, io.opt.grad_log_std = log_std_ptr or None, grad_log_std_ptr or None
        io.stats = stats_ptr or None
        rc = self._lib.dockauv_ppo_update(self._handle, opt.ptr, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_ppo_update")
        opt.policy.has_log_std = True

    # ------------------------------------------------------------------------------------------ episode monitor
    def make_monitor(self):
        """An episode monitor of this handle (dockauv_monitor_create): per-env running returns and lengths, started from the
        handle's own cumulative rewards and step counters, and the reduction workspace.  Needs a float32 handle with an
        auto-reset mode.  ``close`` destroys it before the handle."""
        from ..monitor import DeviceMonitor
        ptr = C.c_void_p()
        rc = self._lib.dockauv_monitor_create(self._handle, C.byref(ptr))
        _capi.check(self._lib, self._handle, rc, "dockauv_monitor_create")
        mon = DeviceMonitor(ptr)
        self._monitors = getattr(self, "_monitors", []) + [mon]
        return mon

    def monitor_sync(self, monitor, stream: int = 0) -> None:
        """The monitor's carries <- the handle's cumulative rewards / step counters at this point of ``stream``
        (dockauv_monitor_sync): after steps the monitor did not see, ``reset_envs`` or field writes."""
        rc = self._lib.dockauv_monitor_sync(monitor.ptr, C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_monitor_sync")

    def monitor_scan_device(self, monitor, rows_out_ptr: int, n_steps: int, stats_ptr: int, terminal_obs_ptr: int = 0,
                            values_ptr: int = 0, returns_ptr: int = 0, ep_return_ptr: int = 0, ep_length_ptr: int = 0,
                            ep_outcome_ptr: int = 0, stream: int = 0) -> None:
        """Returns, lengths and outcomes of the episodes that finish inside rows_out [K][N][n_obs + 2], continuing the monitor's
        carries (dockauv_monitor_scan): stats float64 [16]; terminal_obs [K][N][n_obs] or 0 (no outcomes); values [K + 1][N] and
        returns [K][N] or both 0 (no explained variance); ep_return float32 / ep_length int32 / ep_outcome uint8 [K][N] or 0,
        written only where done.  Asynchronous."""
        io = _capi.MonitorIO()
        io.struct_size = C.sizeof(_capi.MonitorIO)
        io.n_steps = int(n_steps)
        io.rows_out, io.terminal_obs = rows_out_ptr or None, terminal_obs_ptr or None
        io.values, io.returns = values_ptr or None, returns_ptr or None
        io.ep_return, io.ep_length, io.ep_outcome = ep_return_ptr or None, ep_length_ptr or None, ep_outcome_ptr or None
        io.stats = stats_ptr or None
        rc = self._lib.dockauv_monitor_scan(self._handle, monitor.ptr, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_monitor_scan")

    def monitor_carry(self, monitor):
        """(device address of the running returns float32 [N], of the running lengths int32 [N]): dockauv_monitor_carry"""
        r, ln = C.c_void_p(), C.c_void_p()
        rc = self._lib.dockauv_monitor_carry(monitor.ptr, C.byref(r), C.byref(ln))
        _capi.check(self._lib, self._handle, rc, "dockauv_monitor_carry")
        return int(r.value or 0), int(ln.value or 0)

    def destroy_monitor(self, monitor) -> None:
        if monitor.ptr is not None and monitor.ptr.value:
            self._lib.dockauv_monitor_destroy(monitor.ptr)
            monitor.ptr = C.c_void_p()

    # ------------------------------------------------------------------------------------------ replay buffer
    def make_replay(self, buffer_size: int, seed: int = 0):
        """A replay buffer of this handle (dockauv_replay_create): a zero-filled ring of max(buffer_size // num_envs, 1) step
        slots and the observation carry.  Needs a float32 handle with an auto-reset mode.  ``close`` destroys it before the
        handle."""
        from ..replay import DeviceReplay
        ptr = C.c_void_p()
        rc = self._lib.dockauv_replay_create(self._handle, int(buffer_size), int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(ptr))
        _capi.check(self._lib, self._handle, rc, "dockauv_replay_create")
        rb = DeviceReplay(ptr)
        self._replays = getattr(self, "_replays", []) + [rb]
        return rb

    def replay_sync_device(self, replay, rows_ptr: int, stream: int = 0) -> None:
        """The buffer's observation carry <- the observation columns of rows [N][n_obs + 2] (dockauv_replay_sync): the rows
        the next step reads, after steps the buffer did not see.  Asynchronous."""
        rc = self._lib.dockauv_replay_sync(self._handle, replay.ptr, C.c_void_p(rows_ptr or None), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_replay_sync")

    def replay_push_device(self, replay, rows_out_ptr: int, actions_ptr: int, terminal_obs_ptr: int, n_steps: int,
                           rows_in_ptr: int = 0, ep_outcome_ptr: int = 0, stream: int = 0) -> None:
        """Store the K = n_steps transitions of rows_out [K][N][n_obs + 2], actions [K][N][n_u] and terminal_obs [K][N][n_obs]
        (dockauv_replay_push); rows_in [N][n_obs + 2] or 0 (the carry); ep_outcome uint8 [K][N] or 0 (no time limits).
        Asynchronous."""
        io = _capi.ReplayPushIO()
        io.struct_size = C.sizeof(_capi.ReplayPushIO)
        io.n_steps = n_steps
        io.rows_in, io.rows_out, io.actions = rows_in_ptr or None, rows_out_ptr or None, actions_ptr or None
        io.terminal_obs, io.ep_outcome = terminal_obs_ptr or None, ep_outcome_ptr or None
        rc = self._lib.dockauv_replay_push(self._handle, replay.ptr, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_replay_push")

    def replay_sample_device(self, replay, batch_size: int, n_batches: int, obs_ptr: int, actions_ptr: int, next_obs_ptr: int,
                             rewards_ptr: int, dones_ptr: int, index_ptr: int = 0, stream: int = 0) -> None:
        """n_batches minibatches of batch_size stored transitions (dockauv_replay_sample): obs / next_obs [G][B][n_obs],
        actions [G][B][n_u], rewards / dones [G][B], index int64 [G][B] or 0.  Asynchronous."""
        io = _capi.ReplaySampleIO()
        io.struct_size = C.sizeof(_capi.ReplaySampleIO)
        io.n_batches, io.batch_size = n_batches, batch_size
        io.obs, io.actions, io.next_obs = obs_ptr or None, actions_ptr or None, next_obs_ptr or None
        io.rewards, io.dones, io.index = rewards_ptr or None, dones_ptr or None, index_ptr or None
        rc = self._lib.dockauv_replay_sample(self._handle, replay.ptr, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_replay_sample")

    def replay_counts(self, replay):
        """(pos, size, draws): dockauv_replay_counts"""
        pos, size, draws = C.c_longlong(), C.c_longlong(), C.c_uint64()
        rc = self._lib.dockauv_replay_counts(replay.ptr, C.byref(pos), C.byref(size), C.byref(draws))
        _capi.check(self._lib, self._handle, rc, "dockauv_replay_counts")
        return int(pos.value), int(size.value), int(draws.value)

    def replay_set_counts(self, replay, pos: int, size: int, draws: int) -> None:
        rc = self._lib.dockauv_replay_set_counts(replay.ptr, int(pos), int(size), int(draws))
        _capi.check(self._lib, self._handle, rc, "dockauv_replay_set_counts")

    def replay_state(self, replay):
        """(device address of the ring, of the current carry, capacity_steps, record_floats): dockauv_replay_state"""
        st, ca, cap, rf = C.c_void_p(), C.c_void_p(), C.c_longlong(), C.c_int()
        rc = self._lib.dockauv_replay_state(replay.ptr, C.byref(st), C.byref(ca), C.byref(cap), C.byref(rf))
        _capi.check(self._lib, self._handle, rc, "dockauv_replay_state")
        return int(st.value or 0), int(ca.value or 0), int(cap.value), int(rf.value)

    def destroy_replay(self, replay) -> None:
        if replay.ptr is not None and replay.ptr.value:
            self._lib.dockauv_replay_destroy(replay.ptr)
            replay.ptr = C.c_void_p()

    # ------------------------------------------------------------------------------------------ policy evaluation
    def make_evaluator(self, max_episodes_per_env: int):
        """An evaluator of this handle (dockauv_eval_create): per-env carries, counts and quotas, ``max_episodes_per_env`` episode
        slots per env and the reduction workspace, in the state of a begin with target 0.  Needs a float32 handle with an
        auto-reset mode.  ``close`` destroys it before the handle."""
        from ..evaluate import DeviceEvaluator
        ptr = C.c_void_p()
        rc = self._lib.dockauv_eval_create(self._handle, int(max_episodes_per_env), C.byref(ptr))
        _capi.check(self._lib, self._handle, rc, "dockauv_eval_create")
        ev = DeviceEvaluator(ptr, max_episodes_per_env)
        self._evaluators = getattr(self, "_evaluators", []) + [ev]
        return ev

    def evaluator_begin(self, evaluator, targets_ptr: int = 0, uniform_target: int = 1, stream: int = 0) -> None:
        """A new evaluation at this point of ``stream`` (dockauv_eval_begin): carries <- the handle's cumulative rewards / step
        counters, counts and slots cleared, quotas from the device array int32 [N] at ``targets_ptr`` (clamped to [0,
        max_episodes_per_env] on the device) or, with 0, ``uniform_target`` for every env.  Asynchronous."""
        rc = self._lib.dockauv_eval_begin(evaluator.ptr, C.c_void_p(targets_ptr or None), int(uniform_target),
                                          C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_eval_begin")

    def evaluator_scan_device(self, evaluator, rows_out_ptr: int, n_steps: int, stats_ptr: int, terminal_obs_ptr: int = 0,
                              stream: int = 0) -> None:
        """The episodes that finish inside rows_out [K][N][n_obs + 2] go to the evaluator's slots while their env is below its
        quota (dockauv_eval_scan); stats float64 [16] over everything recorded since the begin; terminal_obs [K][N][n_obs] or 0
        (no outcomes).  Asynchronous."""
        io = _capi.EvalIO()
        io.struct_size = C.sizeof(_capi.EvalIO)
        io.n_steps = int(n_steps)
        io.rows_out, io.terminal_obs, io.stats = rows_out_ptr or None, terminal_obs_ptr or None, stats_ptr or None
        rc = self._lib.dockauv_eval_scan(self._handle, evaluator.ptr, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_eval_scan")

    def evaluator_state(self, evaluator) -> dict:
        """Device addresses of the evaluator's arrays (dockauv_eval_state): count, target, carry_length int32 [N], carry_return
        float32 [N], ep_return float32 / ep_length int32 / ep_outcome uint8 [max_episodes_per_env][N]"""
        names = ("count", "target", "ep_return", "ep_length", "ep_outcome", "carry_return", "carry_length")
        out = [C.c_void_p() for _ in names]
        rc = self._lib.dockauv_eval_state(evaluator.ptr, *[C.byref(p) for p in out])
        _capi.check(self._lib, self._handle, rc, "dockauv_eval_state")
        return {n: int(p.value or 0) for n, p in zip(names, out)}

    def destroy_evaluator(self, evaluator) -> None:
        if evaluator.ptr is not None and evaluator.ptr.value:
            self._lib.dockauv_eval_destroy(evaluator.ptr)
            evaluator.ptr = C.c_void_p()

    # ------------------------------------------------------------------------------------------ reward normalisation
    def make_reward_normalizer(self, gamma: float, clip_reward: float = 10.0, epsilon: float = 1e-8):
        """A reward normaliser of this handle (dockauv_rewnorm_create): SB3's VecNormalize(norm_reward=True) statistics --
        running (mean, var, count) of the discounted return and one carry per env -- on the device.  Needs a float32 handle.
        ``close`` destroys it before the handle."""
        from ..normalize import DeviceRewardNormalizer
        ptr = C.c_void_p()
        rc = self._lib.dockauv_rewnorm_create(self._handle, float(gamma), float(clip_reward), float(epsilon), C.byref(ptr))
        _capi.check(self._lib, self._handle, rc, "dockauv_rewnorm_create")
        rn = DeviceRewardNormalizer(ptr, gamma, clip_reward, epsilon)
        self._rewnorms = getattr(self, "_rewnorms", []) + [rn]
        return rn

    def reward_normalizer_state(self, rn):
        """(device address of the state float64 [4] = mean, var, count, reserved; of the carries float32 [N]):
        dockauv_rewnorm_state"""
        s, c = C.c_void_p(), C.c_void_p()
        rc = self._lib.dockauv_rewnorm_state(rn.ptr, C.byref(s), C.byref(c))
        _capi.check(self._lib, self._handle, rc, "dockauv_rewnorm_state")
        return int(s.value or 0), int(c.value or 0)

    def reward_normalizer_reset(self, rn, stream: int = 0) -> None:
        """state <- (0, 1, 1e-4), carries <- 0 at this point of ``stream`` (dockauv_rewnorm_reset)"""
        rc = self._lib.dockauv_rewnorm_reset(rn.ptr, C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_rewnorm_reset")

    def _rewnorm_io(self, rows_out_ptr: int, n_steps: int, reward_norm_ptr: int, discounted_ptr: int, step_stats_ptr: int,
                    training: bool):
        io = _capi.RewnormIO()
        io.struct_size = C.sizeof(_capi.RewnormIO)
        io.n_steps, io.training = int(n_steps), 1 if training else 0
        io.rows_out, io.reward_norm = rows_out_ptr or None, reward_norm_ptr or None
        io.discounted, io.step_stats = discounted_ptr or None, step_stats_ptr or None
        return io

    def reward_normalizer_scan_device(self, rn, rows_out_ptr: int, n_steps: int, reward_norm_ptr: int, discounted_ptr: int = 0,
                                      step_stats_ptr: int = 0, training: bool = True, stream: int = 0) -> None:
        """Normalised rewards of rows_out [K][N][n_obs + 2] (dockauv_rewnorm_scan): reward_norm float32 [K][N]; discounted
        float32 [K][N] and step_stats float64 [K][4] (batch mean, batch var, running var, divisor), both required when
        ``training``; ``training`` False applies the current statistics and touches neither them nor the carries.
        Asynchronous."""
        io = self._rewnorm_io(rows_out_ptr, n_steps, reward_norm_ptr, discounted_ptr, step_stats_ptr, training)
        rc = self._lib.dockauv_rewnorm_scan(self._handle, rn.ptr, C.byref(io), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_rewnorm_scan")

    def gae_normalized_device(self, value, reward_norm_ptr: int, rows_out_ptr: int, values_ptr: int, n_steps: int, gamma: float,
                              gae_lambda: float, advantages_ptr: int, returns_ptr: int, stream: int = 0, trunc=None) -> None:
        """``gae_device`` with the reward of step k read from reward_norm [K][N] (dockauv_gae_normalized); the done word still
        comes from rows_out.  ``trunc``: None, or a dict(n_slots, terminal_obs, length_carry, trunc_step, trunc_row, v_terminal)
        of device addresses -- ``gae_truncated_device``'s three launches with the GAE on the column (needs ``value``).
        Asynchronous."""
        tio = None
        if trunc is not None:
            tio = self._truncation_io(n_steps, trunc["n_slots"], rows_out_ptr, trunc["terminal_obs"], trunc["length_carry"],
                                      trunc["trunc_step"], trunc["trunc_row"], values_ptr, trunc["v_terminal"], advantages_ptr,
                                      returns_ptr, gamma, gae_lambda)
        rc = self._lib.dockauv_gae_normalized(self._handle, value.ptr if value is not None else None,
                                              C.c_void_p(reward_norm_ptr or None), C.byref(tio) if tio is not None else None,
                                              C.c_void_p(rows_out_ptr or None), C.c_void_p(values_ptr or None), int(n_steps),
                                              float(gamma), float(gae_lambda), C.c_void_p(advantages_ptr or None),
                                              C.c_void_p(returns_ptr or None), C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_gae_normalized")

    def collect_normalized_device(self, policy, value, rn, rows_in_ptr: int, rows_out_ptr: int, actions_out_ptr: int, n_steps: int,
                                  reward_norm_ptr: int, discounted_ptr: int, step_stats_ptr: int, values_ptr: int,
                                  advantages_ptr: int, returns_ptr: int, training: bool = True, gamma: float = 0.99,
                                  gae_lambda: float = 0.95, t0: int = 0, stochastic: bool = True, stream: int = 0,
                                  terminal_obs_ptr: int = 0, log_prob_ptr: int = 0, trunc=None) -> None:
        """``collect_device`` with reward normalisation (dockauv_collect_normalized): the rollout and the two value launches,
        ``reward_normalizer_scan_device``, then ``gae_normalized_device`` -- with ``trunc`` (see there; its terminal_obs is
        ``terminal_obs_ptr``) the truncation bootstrap on the normalised rewards.  Needs a critic.  Asynchronous; raises like
        poll_status()."""
        cio = self._collect_io(rows_in_ptr, rows_out_ptr, actions_out_ptr, n_steps, gamma, gae_lambda, t0, stochastic, terminal_obs_ptr,
                               log_prob_ptr, values_ptr, advantages_ptr, returns_ptr)
        tio = None
        if trunc is not None:
            tio = self._truncation_io(n_steps, trunc["n_slots"], rows_out_ptr, terminal_obs_ptr, trunc["length_carry"],
                                      trunc["trunc_step"], trunc["trunc_row"], values_ptr, trunc["v_terminal"], advantages_ptr,
                                      returns_ptr, gamma, gae_lambda)
        nio = self._rewnorm_io(rows_out_ptr, n_steps, reward_norm_ptr, discounted_ptr, step_stats_ptr, training)
        rc = self._lib.dockauv_collect_normalized(self._handle, policy.ptr, value.ptr if value is not None else None, C.byref(cio),
                                                  C.byref(tio) if tio is not None else None, rn.ptr, C.byref(nio),
                                                  C.c_void_p(stream or None))
        _capi.check(self._lib, self._handle, rc, "dockauv_collect_normalized")

    def destroy_reward_normalizer(self, rn) -> None:
        if rn.ptr is not None and rn.ptr.value:
            self._lib.dockauv_rewnorm_destroy(rn.ptr)
            rn.ptr = C.c_void_p()

    def destroy_optim(self, opt) -> None:
        if opt.ptr is not None and opt.ptr.value:
            self._lib.dockauv_optim_destroy(opt.ptr)
            opt.ptr = C.c_void_p()

    def destroy_policy(self, policy) -> None:
        if policy.ptr is not None and policy.ptr.value:
            self._lib.dockauv_policy_destroy(policy.ptr)
            policy.ptr = C.c_void_p()

    def time_steps_device(self, actions_ptr: int, obs_ptr: int, reward_ptr: int = 0, done_ptr: int = 0, steps: int = 1,
                          stream: int = 0, packed: bool = False, terminal_obs_ptr: int = 0) -> float:
        """Average KERNEL duration in microseconds from per-dispatch HIP events on `stream` (bench.py)."""
        io = _capi.StepIO()
        io.actions, io.obs = actions_ptr, obs_ptr
        io.reward, io.done = reward_ptr or None, done_ptr or None
        io.terminal_obs = terminal_obs_ptr or None
        io.pack_reward_done = self._pack_mode(packed)
        out = C.c_double(0.0)
        rc = self._lib.dockauv_time_steps(self._handle, C.byref(io), C.c_void_p(stream or None), int(steps), C.byref(out))
        _capi.check(self._lib, self._handle, rc, "dockauv_time_steps")
        return out.value

    def synchronize(self) -> None:
        _capi.check(self._lib, self._handle, self._lib.dockauv_synchronize(self._handle), "dockauv_synchronize")

    def poll_status(self) -> None:
        """Raise DockAUVError if a step kernel that has already run reported an internal time-out (the handle's sticky
        status word, host-coherent memory): no synchronisation, a microsecond -- for rollouts on device pointers that
        never call a synchronising entry point."""
        _capi.check(self._lib, self._handle, self._lib.dockauv_poll_status(self._handle), "dockauv_poll_status")

    # ------------------------------------------------------------------------------------------ VecEnv odds and ends
    def close(self) -> None:
        if getattr(self, "_handle", None) is not None and self._handle.value:
            for opt in getattr(self, "_optims", []):     # (an optimiser goes before its policies)
                self.destroy_optim(opt)
            self._optims = []
            for mon in getattr(self, "_monitors", []):   # (a monitor goes before its handle)
                self.destroy_monitor(mon)
            self._monitors = []
            for rb in getattr(self, "_replays", []):     # (a replay buffer goes before its handle)
                self.destroy_replay(rb)
            self._replays = []
            for ev in getattr(self, "_evaluators", []):  # (an evaluator goes before its handle)
                self.destroy_evaluator(ev)
            self._evaluators = []
            for rn in getattr(self, "_rewnorms", []):    # (a reward normaliser goes before its handle)
                self.destroy_reward_normalizer(rn)
            self._rewnorms = []
            for pol in getattr(self, "_policies", []):   # (a policy goes before its handle)
                self.destroy_policy(pol)
            self._policies = []
            self._lib.dockauv_destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def get_attr(self, attr_name, indices=None):
        n = self.num_envs if indices is None else len(np.atleast_1d(indices))
        return [getattr(self, attr_name)] * n

    def set_attr(self, attr_name, value, indices=None):
        setattr(self, attr_name, value)

    def env_method(self, method_name, *args, indices=None, **kwargs):
        return [getattr(self, method_name)(*args, **kwargs)]

    def env_is_wrapped(self, wrapper_class, indices=None):
        return [False] * self.num_envs

    def render(self, mode="human"):
        raise NotImplementedError("rendering is outside the accelerated path (reference: utils/plotutils.py)")
