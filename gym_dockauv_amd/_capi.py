"""
ctypes binding of libdockauv.so (include/dockauv.h).  This is the ONLY compute path of the package: if the HIP
library is missing or no MI355X is visible, loading / creating fails loudly -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libdockauv.so")

ABI_VERSION = 3
OPT_SEQUENCE_RESIDENT = 1
MAX_U = 8
N_REWARDS = 13
N_CONDITIONS = 5
N_OBS_BASE = 16
MAX_CAPSULES = 8
MAX_SPHERES = 16

F32, F64 = 0, 1
VEH_CONSTB, VEH_LAUV = 0, 1
RESET_NONE, RESET_POOL, RESET_DEVICE = 0, 1, 2

(F_STATE, F_U, F_GOAL, F_CURRENT, F_TSTEPS, F_CAPSULES, F_SPHERES, F_VEHICLE_ID, F_CUM_REWARD, F_EPISODE,
 F_CURRENT_SIGMA) = range(11)
(F_POOL_POSE, F_POOL_GOAL, F_POOL_CURRENT, F_POOL_CAPSULES, F_POOL_SPHERES) = range(16, 21)

SCN = {"SimpleDocking3d": 0, "SimpleCurrentDocking3d": 1, "CapsuleDocking3d": 2, "CapsuleCurrentDocking3d": 3,
       "ObstaclesDocking3d": 4, "ObstaclesNoCapDocking3d": 5, "ObstaclesCurrentDocking3d": 6, "SphereDocking3d": 7}


class Vehicle(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("n_u", C.c_int32),
        ("m", C.c_double), ("W", C.c_double), ("BY", C.c_double),
        ("r_G", C.c_double * 3), ("r_B", C.c_double * 3),
        ("I_b", C.c_double * 9),
        ("ma_diag", C.c_double * 6),
        ("d_lin", C.c_double * 6), ("d_quad", C.c_double * 6),
        ("M_inv", C.c_double * 36),
        ("B", C.c_double * (6 * MAX_U)),
        ("u_lo", C.c_double * MAX_U), ("u_hi", C.c_double * MAX_U),
        ("lauv", C.c_double * 20),
    ]


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("abi_version", C.c_uint32),
        ("n_envs", C.c_int32), ("precision", C.c_int32), ("n_vehicles", C.c_int32), ("reset_mode", C.c_int32),
        ("scenario", C.c_int32), ("max_timesteps", C.c_int32), ("reward_set", C.c_int32),
        ("max_capsules", C.c_int32), ("max_spheres", C.c_int32),
        ("n_v", C.c_int32), ("n_h", C.c_int32), ("blocksize_reduce", C.c_int32),
        ("envs_per_group", C.c_int32), ("threads_per_group", C.c_int32),
        ("seed", C.c_uint64),
        ("t_step_size", C.c_double), ("lowpass_T1", C.c_double), ("current_mu", C.c_double),
        ("max_dist_from_goal", C.c_double), ("max_attitude", C.c_double), ("dist_goal_reached_tol", C.c_double),
        ("vel_max", C.c_double * 6),
        ("safety_radius", C.c_double),
        ("w_d", C.c_double), ("w_delta_theta", C.c_double), ("w_delta_psi", C.c_double), ("w_phi", C.c_double),
        ("w_theta", C.c_double), ("w_Thetadot", C.c_double), ("w_oa", C.c_double),
        ("w_done", C.c_double * N_CONDITIONS),
        ("action_reward_factors", C.c_double * MAX_U),
        ("radar_max_dist", C.c_double), ("radar_alpha_max", C.c_double), ("radar_beta_max", C.c_double),
        ("ray_table", C.POINTER(C.c_double)),
        ("vehicle", Vehicle * 2),
        ("device_noise", C.c_int32), ("reserved0", C.c_int32),
    ]


class StepIO(C.Structure):
    _fields_ = [
        ("actions", C.c_void_p), ("noise", C.c_void_p), ("obs", C.c_void_p), ("reward", C.c_void_p),
        ("done", C.c_void_p), ("reward_terms", C.c_void_p), ("conditions", C.c_void_p), ("nav", C.c_void_p),
        ("ray_dist", C.c_void_p), ("terminal_obs", C.c_void_p), ("state_dot", C.c_void_p),
        ("pack_reward_done", C.c_int32), ("reserved", C.c_int32),
    ]


P2P_HANDLE_BYTES = 64
P2P_MAX_PEERS = 15


class P2PPlan(C.Structure):
    _fields_ = [
        ("dsts", C.c_void_p * (P2P_MAX_PEERS + 1)), ("peer_slots", C.c_void_p * P2P_MAX_PEERS),
        ("my_flags", C.c_void_p), ("status", C.c_void_p), ("counter", C.c_void_p),
        ("bytes", C.c_uint64), ("max_spins", C.c_uint64),
        ("n_dsts", C.c_int32), ("n_peers", C.c_int32), ("world", C.c_int32), ("my_rank", C.c_int32),
    ]


ACT_NONE, ACT_TANH, ACT_RELU = 0, 1, 2
POLICY_MAX_WIDTH = 128


class PolicyDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("precision", C.c_int32),
        ("n_in", C.c_int32), ("n_hidden", C.c_int32 * 2), ("n_out", C.c_int32),
        ("hidden_act", C.c_int32), ("out_act", C.c_int32),
        ("pointers_on_device", C.c_int32), ("reserved", C.c_int32),
        ("W1", C.c_void_p), ("b1", C.c_void_p), ("W2", C.c_void_p), ("b2", C.c_void_p), ("W3", C.c_void_p), ("b3", C.c_void_p),
        ("log_std", C.c_void_p),
        ("seed", C.c_uint64), ("env_id_offset", C.c_uint64),
    ]


class CollectIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_steps", C.c_int32),
        ("rows_in", C.c_void_p), ("rows_out", C.c_void_p), ("actions_out", C.c_void_p), ("terminal_obs", C.c_void_p),
        ("log_prob", C.c_void_p), ("values", C.c_void_p), ("advantages", C.c_void_p), ("returns", C.c_void_p),
        ("t0", C.c_uint64), ("stochastic", C.c_int32), ("gamma", C.c_float), ("gae_lambda", C.c_float), ("reserved", C.c_int32),
    ]


class TruncationIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_steps", C.c_int32), ("n_slots", C.c_int32),
        ("gamma", C.c_float), ("gae_lambda", C.c_float), ("reserved", C.c_int32),
        ("rows_out", C.c_void_p), ("terminal_obs", C.c_void_p), ("values", C.c_void_p),
        ("length_carry", C.c_void_p), ("trunc_step", C.c_void_p), ("trunc_row", C.c_void_p), ("v_terminal", C.c_void_p),
        ("advantages", C.c_void_p), ("returns", C.c_void_p),
    ]


class PolicyGrads(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("reserved", C.c_uint32),
        ("dW1", C.c_void_p), ("db1", C.c_void_p), ("dW2", C.c_void_p), ("db2", C.c_void_p), ("dW3", C.c_void_p), ("db3", C.c_void_p),
    ]


class PPOHeadIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("normalize_advantage", C.c_int32),
        ("mean", C.c_void_p), ("v", C.c_void_p),
        ("actions", C.c_void_p), ("log_prob_old", C.c_void_p), ("advantages", C.c_void_p), ("returns", C.c_void_p),
        ("row_index", C.c_void_p), ("n_rows", C.c_longlong),
        ("clip_range", C.c_float), ("vf_coef", C.c_float), ("ent_coef", C.c_float), ("reserved", C.c_int32),
        ("grad_mean", C.c_void_p), ("grad_v", C.c_void_p), ("grad_log_std", C.c_void_p), ("stats", C.c_void_p),
    ]


class OptimDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("reserved", C.c_uint32),
        ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
        ("max_grad_norm", C.c_float), ("reserved1", C.c_float),
    ]


class OptimIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("reserved", C.c_uint32),
        ("lr", C.c_double),
        ("actor_params", C.c_void_p * 6), ("log_std", C.c_void_p),
        ("actor_grads", C.c_void_p * 6), ("grad_log_std", C.c_void_p),
        ("critic_params", C.c_void_p * 6), ("critic_grads", C.c_void_p * 6),
        ("stats", C.c_void_p),
    ]


class PPOUpdateIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("normalize_advantage", C.c_int32),
        ("rows", C.c_void_p),
        ("actions", C.c_void_p), ("log_prob_old", C.c_void_p), ("advantages", C.c_void_p), ("returns", C.c_void_p),
        ("values_old", C.c_void_p),
        ("n_rows", C.c_longlong), ("batch_size", C.c_longlong), ("n_epochs", C.c_int32), ("reserved", C.c_int32),
        ("seed", C.c_uint64), ("first_epoch", C.c_uint64),
        ("clip_range", C.c_float), ("clip_range_vf", C.c_float), ("vf_coef", C.c_float), ("ent_coef", C.c_float),
        ("target_kl", C.c_float), ("reserved1", C.c_float),
        ("opt", OptimIO),
        ("stats", C.c_void_p),
    ]


class MonitorIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_steps", C.c_int32),
        ("rows_out", C.c_void_p), ("terminal_obs", C.c_void_p), ("values", C.c_void_p), ("returns", C.c_void_p),
        ("ep_return", C.c_void_p), ("ep_length", C.c_void_p), ("ep_outcome", C.c_void_p), ("stats", C.c_void_p),
    ]


class RewnormIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_steps", C.c_int32), ("training", C.c_int32), ("reserved", C.c_int32),
        ("rows_out", C.c_void_p), ("reward_norm", C.c_void_p), ("discounted", C.c_void_p), ("step_stats", C.c_void_p),
    ]


class EvalIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_steps", C.c_int32),
        ("rows_out", C.c_void_p), ("terminal_obs", C.c_void_p), ("stats", C.c_void_p),
    ]


class ReplayPushIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_steps", C.c_int32),
        ("rows_in", C.c_void_p), ("rows_out", C.c_void_p), ("actions", C.c_void_p), ("terminal_obs", C.c_void_p),
        ("ep_outcome", C.c_void_p),
    ]


class ReplaySampleIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_batches", C.c_int32), ("batch_size", C.c_longlong),
        ("obs", C.c_void_p), ("actions", C.c_void_p), ("next_obs", C.c_void_p), ("rewards", C.c_void_p), ("dones", C.c_void_p),
        ("index", C.c_void_p),
    ]


class SacActorDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("precision", C.c_int32),
        ("n_in", C.c_int32), ("n_hidden", C.c_int32 * 2), ("n_out", C.c_int32),
        ("hidden_act", C.c_int32), ("pointers_on_device", C.c_int32), ("reserved", C.c_int32 * 2),
        ("W1", C.c_void_p), ("b1", C.c_void_p), ("W2", C.c_void_p), ("b2", C.c_void_p),
        ("W_mu", C.c_void_p), ("b_mu", C.c_void_p), ("W_ls", C.c_void_p), ("b_ls", C.c_void_p),
        ("seed", C.c_uint64), ("env_id_offset", C.c_uint64),
    ]


class QIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("obs_stride", C.c_int32), ("act_stride", C.c_int32), ("reserved", C.c_int32),
        ("obs", C.c_void_p), ("actions", C.c_void_p), ("row_index", C.c_void_p), ("n_rows", C.c_longlong), ("q", C.c_void_p),
    ]


class SacTargetIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("next_obs_stride", C.c_int32), ("column_stride", C.c_int32),
        ("gamma", C.c_float), ("ent_coef", C.c_float), ("reserved", C.c_int32),
        ("next_obs", C.c_void_p), ("row_index", C.c_void_p), ("rewards", C.c_void_p), ("dones", C.c_void_p),
        ("timeouts", C.c_void_p), ("log_ent_coef", C.c_void_p),
        ("n_rows", C.c_longlong), ("t", C.c_uint64), ("row_offset", C.c_uint64),
        ("a2", C.c_void_p), ("logp2", C.c_void_p), ("q1", C.c_void_p), ("q2", C.c_void_p), ("y", C.c_void_p),
    ]


class SacRowsIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("row_stride", C.c_int32),
        ("rows", C.c_void_p), ("row_index", C.c_void_p), ("n_rows", C.c_longlong), ("out", C.c_void_p),
    ]


class SacActorBackwardIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("row_stride", C.c_int32),
        ("rows", C.c_void_p), ("row_index", C.c_void_p), ("n_rows", C.c_longlong), ("grad_out", C.c_void_p),
        ("dW1", C.c_void_p), ("db1", C.c_void_p), ("dW2", C.c_void_p), ("db2", C.c_void_p),
        ("dW_mu", C.c_void_p), ("db_mu", C.c_void_p), ("dW_ls", C.c_void_p), ("db_ls", C.c_void_p),
    ]


class QBackwardIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("obs_stride", C.c_int32), ("act_stride", C.c_int32), ("reserved", C.c_int32),
        ("obs", C.c_void_p), ("actions", C.c_void_p), ("row_index", C.c_void_p), ("n_rows", C.c_longlong), ("grad_q", C.c_void_p),
        ("grads", C.POINTER(PolicyGrads)), ("grad_actions", C.c_void_p),
    ]


class SacSampleIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("reserved", C.c_int32),
        ("heads", C.c_void_p), ("n_rows", C.c_longlong), ("t", C.c_uint64), ("row_offset", C.c_uint64),
        ("a", C.c_void_p), ("logp", C.c_void_p),
    ]


class SacCriticHeadIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("reserved", C.c_int32),
        ("q1", C.c_void_p), ("q2", C.c_void_p), ("y", C.c_void_p), ("n_rows", C.c_longlong),
        ("grad_q1", C.c_void_p), ("grad_q2", C.c_void_p), ("stats", C.c_void_p),
    ]


class SacActorHeadIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("ent_coef", C.c_float),
        ("heads", C.c_void_p), ("q1_pi", C.c_void_p), ("q2_pi", C.c_void_p), ("dq1", C.c_void_p), ("dq2", C.c_void_p),
        ("log_ent_coef", C.c_void_p), ("n_rows", C.c_longlong), ("t", C.c_uint64), ("row_offset", C.c_uint64),
        ("grad_out", C.c_void_p), ("stats", C.c_void_p),
    ]


class SacEntCoefIO(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("target_entropy", C.c_float),
        ("state", C.c_void_p), ("logp", C.c_void_p), ("n_rows", C.c_longlong), ("step", C.c_longlong),
        ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
        ("before", C.c_void_p), ("stats", C.c_void_p),
    ]


# every symbol include/dockauv.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("dockauv_abi_version", C.c_int, []),
    ("dockauv_build_info", C.c_char_p, []),
    ("dockauv_last_error", C.c_char_p, [C.c_void_p]),
    ("dockauv_create", C.c_int, [C.POINTER(Config), C.c_int, C.POINTER(C.c_void_p)]),
    ("dockauv_destroy", C.c_int, [C.c_void_p]),
    ("dockauv_n_obs", C.c_int, [C.c_void_p]),
    ("dockauv_threads_per_group", C.c_int, [C.c_void_p]),
    ("dockauv_step_uses_current", C.c_int, [C.c_void_p]),
    ("dockauv_step_uses_capsules", C.c_int, [C.c_void_p]),
    ("dockauv_n_rays", C.c_int, [C.c_void_p]),
    ("dockauv_n_u", C.c_int, [C.c_void_p]),
    ("dockauv_field_width", C.c_int, [C.c_void_p, C.c_int]),
    ("dockauv_set_field", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    ("dockauv_get_field", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    ("dockauv_reset_envs", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("dockauv_step", C.c_int, [C.c_void_p, C.POINTER(StepIO), C.c_void_p]),
    ("dockauv_step_sequence", C.c_int, [C.c_void_p, C.POINTER(StepIO), C.c_int, C.c_void_p]),
    ("dockauv_set_option", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("dockauv_step_host", C.c_int, [C.c_void_p, C.POINTER(StepIO)]),
    ("dockauv_synchronize", C.c_int, [C.c_void_p]),
    ("dockauv_poll_status", C.c_int, [C.c_void_p]),
    ("dockauv_trace_enable", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    ("dockauv_trace_steps", C.c_longlong, [C.c_void_p]),
    ("dockauv_trace_read", C.c_int, [C.c_void_p, C.c_longlong, C.c_int] + [C.c_void_p] * 8),
    ("dockauv_time_steps", C.c_int, [C.c_void_p, C.POINTER(StepIO), C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
    ("dockauv_p2p_alloc", C.c_int, [C.c_int, C.c_size_t, C.c_int, C.POINTER(C.c_void_p), C.c_char_p]),
    ("dockauv_p2p_free", C.c_int, [C.c_void_p]),
    ("dockauv_p2p_open", C.c_int, [C.c_int, C.c_char_p, C.POINTER(C.c_void_p)]),
    ("dockauv_p2p_close", C.c_int, [C.c_void_p]),
    ("dockauv_p2p_push", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.c_int, C.c_void_p]),
    ("dockauv_p2p_signal_wait", C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_uint32,
                                          C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("dockauv_p2p_gather", C.c_int, [C.POINTER(P2PPlan), C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    ("dockauv_step_gather_sequence", C.c_int, [C.c_void_p, C.POINTER(StepIO), C.c_int, C.POINTER(P2PPlan), C.c_int,
                                               C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]),
    ("dockauv_policy_create", C.c_int, [C.c_void_p, C.POINTER(PolicyDesc), C.POINTER(C.c_void_p)]),
    ("dockauv_policy_load", C.c_int, [C.c_void_p, C.POINTER(PolicyDesc), C.c_void_p]),
    ("dockauv_policy_destroy", C.c_int, [C.c_void_p]),
    ("dockauv_policy_forward", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    ("dockauv_rollout", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                  C.c_uint64, C.c_int, C.c_void_p]),
    ("dockauv_value_create", C.c_int, [C.c_void_p, C.POINTER(PolicyDesc), C.POINTER(C.c_void_p)]),
    ("dockauv_value_forward", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    ("dockauv_policy_forward_logp", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int,
                                              C.c_void_p]),
    ("dockauv_gae", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                              C.c_void_p]),
    ("dockauv_collect", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CollectIO), C.c_void_p]),
    ("dockauv_truncation_slots", C.c_int, [C.c_void_p, C.c_int]),
    ("dockauv_truncation_scan", C.c_int, [C.c_void_p, C.POINTER(TruncationIO), C.c_void_p]),
    ("dockauv_gae_truncated", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(TruncationIO), C.c_void_p]),
    ("dockauv_collect_truncated", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CollectIO), C.POINTER(TruncationIO),
                                            C.c_void_p]),
    ("dockauv_policy_forward_rows", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    ("dockauv_policy_backward", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p,
                                          C.POINTER(PolicyGrads), C.c_void_p]),
    ("dockauv_ppo_head", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PPOHeadIO), C.c_void_p]),
    ("dockauv_optim_create", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(OptimDesc), C.POINTER(C.c_void_p)]),
    ("dockauv_optim_destroy", C.c_int, [C.c_void_p]),
    ("dockauv_optim_step", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(OptimIO), C.c_void_p]),
    ("dockauv_optim_state", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong),
                                      C.POINTER(C.c_longlong)]),
    ("dockauv_permutation", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_longlong, C.c_void_p, C.c_void_p]),
    ("dockauv_ppo_update", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PPOUpdateIO), C.c_void_p]),
    ("dockauv_monitor_create", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    ("dockauv_monitor_destroy", C.c_int, [C.c_void_p]),
    ("dockauv_monitor_sync", C.c_int, [C.c_void_p, C.c_void_p]),
    ("dockauv_monitor_scan", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(MonitorIO), C.c_void_p]),
    ("dockauv_monitor_carry", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    ("dockauv_eval_create", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    ("dockauv_eval_destroy", C.c_int, [C.c_void_p]),
    ("dockauv_eval_begin", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    ("dockauv_eval_scan", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(EvalIO), C.c_void_p]),
    ("dockauv_eval_state", C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 7),
    ("dockauv_rewnorm_create", C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_double, C.POINTER(C.c_void_p)]),
    ("dockauv_rewnorm_destroy", C.c_int, [C.c_void_p]),
    ("dockauv_rewnorm_state", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    ("dockauv_rewnorm_reset", C.c_int, [C.c_void_p, C.c_void_p]),
    ("dockauv_rewnorm_scan", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(RewnormIO), C.c_void_p]),
    ("dockauv_gae_normalized", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TruncationIO), C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("dockauv_collect_normalized", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CollectIO), C.POINTER(TruncationIO),
                                             C.c_void_p, C.POINTER(RewnormIO), C.c_void_p]),
    # (the SAC forward half; the replay entries stay the last ones, which tests/test_replay_host.py pins)
    ("dockauv_sac_actor_create", C.c_int, [C.c_void_p, C.POINTER(SacActorDesc), C.POINTER(C.c_void_p)]),
    ("dockauv_sac_actor_load", C.c_int, [C.c_void_p, C.POINTER(SacActorDesc), C.c_void_p]),
    ("dockauv_q_create", C.c_int, [C.c_void_p, C.POINTER(PolicyDesc), C.POINTER(C.c_void_p)]),
    ("dockauv_q_forward", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(QIO), C.c_void_p]),
    ("dockauv_sac_target", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SacTargetIO), C.c_void_p]),
    # (the networks' share of SAC's gradient half)
    ("dockauv_sac_actor_forward_rows", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(SacRowsIO), C.c_void_p]),
    ("dockauv_sac_actor_backward", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(SacActorBackwardIO), C.c_void_p]),
    ("dockauv_q_backward", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(QBackwardIO), C.c_void_p]),
    ("dockauv_policy_backward_workspace", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)]),
    # (SAC's loss head and the learned entropy coefficient)
    ("dockauv_sac_sample", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(SacSampleIO), C.c_void_p]),
    ("dockauv_sac_critic_head", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(SacCriticHeadIO), C.c_void_p]),
    ("dockauv_sac_actor_head", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(SacActorHeadIO), C.c_void_p]),
    ("dockauv_sac_ent_coef_step", C.c_int, [C.c_void_p, C.POINTER(SacEntCoefIO), C.c_void_p]),
    ("dockauv_replay_create", C.c_int, [C.c_void_p, C.c_longlong, C.c_uint64, C.POINTER(C.c_void_p)]),
    ("dockauv_replay_destroy", C.c_int, [C.c_void_p]),
    ("dockauv_replay_sync", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("dockauv_replay_push", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ReplayPushIO), C.c_void_p]),
    ("dockauv_replay_sample", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ReplaySampleIO), C.c_void_p]),
    ("dockauv_replay_counts", C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_uint64)]),
    ("dockauv_replay_set_counts", C.c_int, [C.c_void_p, C.c_longlong, C.c_longlong, C.c_uint64]),
    ("dockauv_replay_state", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong),
                                       C.POINTER(C.c_int)]),
]

_lib: Optional[C.CDLL] = None


class DockAUVError(RuntimeError):
    pass


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen libdockauv.so and bind every declared symbol.  Raises if the library or a symbol is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("DOCKAUV_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise DockAUVError(f"{p} not found: build it first (python -c 'import __graft_entry__ as g; g.build()' or "
                           f"make -C gym_dockauv_amd/csrc).  There is no CPU fallback.")
    lib = C.CDLL(p)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.dockauv_abi_version() != ABI_VERSION:
        raise DockAUVError(f"libdockauv ABI {lib.dockauv_abi_version()} != binding ABI {ABI_VERSION}")
    if path is None:
        _lib = lib
    return lib


def check(lib: C.CDLL, handle, rc: int, what: str) -> None:
    if rc != 0:
        msg = lib.dockauv_last_error(handle)
        raise DockAUVError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")
