/*
 * dockauv.h -- C ABI of libdockauv.so: batched docking3d step() on MI355X (gfx950).
 *
 * The reference (Erikx3/gym_dockauv) is pure Python and has no FFI; the boundary it offers is the Python class
 * API of gym_dockauv/envs/docking3d.py.  This header is the C-ABI a maintainer would bind underneath that API
 * (ctypes stub: INTEGRATION.md).  Each entry point names the reference interface it replaces.
 *
 * Conventions: every function returns 0 on success and a negative DOCKAUV_E_* code on failure;
 * dockauv_last_error() gives the message.  No exceptions cross the boundary.  All pointers are plain C pointers
 * with explicit sizes; no torch / numpy types.  One host thread drives one handle; work is stream-ordered on the
 * HIP stream passed to dockauv_step (NULL = the default stream).  The library owns the per-env state in HBM until
 * dockauv_destroy; the caller owns every buffer it passes in.
 *
 * Host-side field I/O (dockauv_set_field / dockauv_get_field) is always float64, row-major [count][width]
 * ("array of envs"); the library converts to its struct-of-arrays device layout and device precision.
 */
#ifndef DOCKAUV_H
#define DOCKAUV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DOCKAUV_ABI_VERSION 3
#define DOCKAUV_MAX_U 8          /* inputs: BlueROV2 joystick 6, BlueROV2 direct 8, LAUV 3 */
#define DOCKAUV_N_REWARDS 13     /* envs/docking3d.py:152 */
#define DOCKAUV_N_CONDITIONS 5   /* envs/docking3d.py:597-619 */
#define DOCKAUV_N_OBS_BASE 16    /* envs/docking3d.py:114 */
#define DOCKAUV_MAX_RAYS 1024
#define DOCKAUV_MAX_CAPSULES 8
#define DOCKAUV_MAX_SPHERES 16

/* error codes */
#define DOCKAUV_OK 0
#define DOCKAUV_E_INVALID (-1)   /* bad argument / config */
#define DOCKAUV_E_HIP (-2)       /* HIP runtime error (message has hipGetErrorString) */
#define DOCKAUV_E_NODEVICE (-3)  /* no usable gfx950 device */
#define DOCKAUV_E_RANGE (-4)     /* first/count outside [0, n_envs) */
#define DOCKAUV_E_KERNEL (-5)    /* a step kernel reported an internal time-out in the handle's sticky status word (an
                                    intra-group wait gave up instead of hanging the GPU); reported by the calls that
                                    synchronise: dockauv_synchronize, dockauv_get_field, dockauv_step_host,
                                    dockauv_time_steps, dockauv_trace_read -- and by dockauv_poll_status, which does
                                    not.  Results since are invalid. */

/* device arithmetic type of the path */
#define DOCKAUV_F32 0            /* product path ("within 1e-5 of the float64 reference") */
#define DOCKAUV_F64 1            /* validation path: same kernels instantiated in double */

/* vehicle model kinds */
#define DOCKAUV_VEH_CONSTB 0     /* constant B, diagonal damping: objects/vehicles/BlueROV2.py:27-88 */
#define DOCKAUV_VEH_LAUV 1       /* B(nu) ~ u^2, cross-coupled damping + lift: objects/vehicles/LAUV.py:59-110 */

/* what happens to an env whose episode ended inside dockauv_step */
#define DOCKAUV_RESET_NONE 0     /* nothing: caller resets (single-env gym.Env semantics, docking3d.py:222) */
#define DOCKAUV_RESET_POOL 1     /* in-kernel reset from the host-staged next-episode pool (VecEnv auto-reset) */
#define DOCKAUV_RESET_DEVICE 2   /* in-kernel scenario generation with a counter RNG (throughput mode) */

/* scenario ids for DOCKAUV_RESET_DEVICE (envs/docking3d.py:795-988) */
#define DOCKAUV_SCN_SIMPLE 0
#define DOCKAUV_SCN_SIMPLE_CURRENT 1
#define DOCKAUV_SCN_CAPSULE 2
#define DOCKAUV_SCN_CAPSULE_CURRENT 3
#define DOCKAUV_SCN_OBSTACLES 4
#define DOCKAUV_SCN_OBSTACLES_NOCAP 5
#define DOCKAUV_SCN_OBSTACLES_CURRENT 6
#define DOCKAUV_SCN_SPHERES 7    /* build-defined: SimpleDocking3d + max_spheres spheres in a 3..12 m shell */

/*
 * One vehicle type.  Replaces the per-instance constants of objects/statespace.py:58-197 (StateSpace) and the
 * B / D / u_bound overrides of the two vehicle classes.  The host computes M_inv exactly like the reference
 * (numpy.linalg.inv of M_RB + M_A in float64, statespace.py:190-197) and hands the numbers over.
 */
typedef struct dockauv_vehicle {
    int32_t kind;                 /* DOCKAUV_VEH_* */
    int32_t n_u;                  /* number of inputs, <= DOCKAUV_MAX_U */
    double m;                     /* mass */
    double W, BY;                 /* weight m*g (statespace.py:86-88), buoyancy */
    double r_G[3], r_B[3];        /* CG / CB offsets from CO */
    double I_b[9];                /* inertia about CO, row-major (statespace.py:105-117) */
    double ma_diag[6];            /* diagonal of M_A = -(X_udot..N_rdot) (statespace.py:164-187) */
    double d_lin[6], d_quad[6];   /* X_u..N_r, X_uu..N_rr (statespace.py:288-351) */
    double M_inv[36];             /* row-major */
    double B[6 * DOCKAUV_MAX_U];  /* row-major 6 x DOCKAUV_MAX_U, constant-B kinds only (BlueROV2.py:34-72) */
    double u_lo[DOCKAUV_MAX_U], u_hi[DOCKAUV_MAX_U]; /* u_bound columns (BlueROV2.py:44-50, LAUV.py:103-110) */
    /* LAUV extras (LAUV.py:32-55), order: Y_r Y_rr Y_urf | Z_q Z_qq Z_uqf | M_w M_ww M_uwb+M_uwf |
       N_v N_vv N_uvb+N_uvf | Y_uvb+Y_uvf  Z_uwb+Z_uwf  M_uqf  N_urf | Y_uudr Z_uuds M_uuds N_uudr */
    double lauv[20];
} dockauv_vehicle;

/*
 * Environment batch configuration.  Replaces the reads of the config dict in BaseDocking3d.__init__
 * (envs/docking3d.py:48-220; key schema config/env_config.py:20-91) and Radar.__init__ (objects/sensor.py:43-87).
 */
typedef struct dockauv_config {
    uint32_t struct_size;          /* sizeof(dockauv_config): ABI check */
    uint32_t abi_version;          /* DOCKAUV_ABI_VERSION */
    int32_t n_envs;                /* envs owned by this handle (this GPU's shard) */
    int32_t precision;             /* DOCKAUV_F32 / DOCKAUV_F64 */
    int32_t n_vehicles;            /* 1, or 2 for a per-env vehicle id (mixed batch) */
    int32_t reset_mode;            /* DOCKAUV_RESET_* */
    int32_t scenario;              /* DOCKAUV_SCN_* (used by DOCKAUV_RESET_DEVICE only) */
    int32_t max_timesteps;         /* "max_timesteps" */
    int32_t reward_set;            /* "reward_set": 1 or 2 (docking3d.py:519-582) */
    int32_t max_capsules;          /* per-env capsule slots, 0..DOCKAUV_MAX_CAPSULES */
    int32_t max_spheres;           /* per-env sphere slots, 0..DOCKAUV_MAX_SPHERES */
    int32_t n_v, n_h;              /* ray fan: vertical x horizontal rays (sensor.py:56-63) */
    int32_t blocksize_reduce;      /* "blocksize_reduce" (sensor.py:136-137) */
    int32_t envs_per_group;        /* 0 = auto (64); -1 = test hook: general (non-structural) kinetics expressions */
    int32_t threads_per_group;     /* 0 = auto; 64/128 without obstacles, 64/256/512 with: waves per 64-env group */
    uint64_t seed;                 /* DOCKAUV_RESET_DEVICE: counter-RNG key */
    double t_step_size;            /* "t_step_size" */
    double lowpass_T1;             /* 0.2 (objects/auvsim.py:40) */
    double current_mu;             /* Gauss-Markov mu, 0.005 in every shipped scenario (docking3d.py:820) */
    double max_dist_from_goal, max_attitude, dist_goal_reached_tol;
    double vel_max[6];             /* u_max v_max w_max p_max q_max r_max */
    double safety_radius;          /* 1.0, hard-wired in the reference (objects/auvsim.py:43) */
    double w_d, w_delta_theta, w_delta_psi, w_phi, w_theta, w_Thetadot, w_oa; /* "reward_factors" */
    double w_done[DOCKAUV_N_CONDITIONS];  /* w_goal w_deltad_max w_Theta_max w_t_max w_col (docking3d.py:181-187) */
    double action_reward_factors[DOCKAUV_MAX_U]; /* scalar config value broadcast by the host (docking3d.py:584) */
    double radar_max_dist;         /* "radar.max_dist" */
    double radar_alpha_max, radar_beta_max; /* alpha/2, beta/2 (sensor.py:53-54) */
    /* [n_v*n_h][4] row-major, ray index = iv*n_h + ih: unit body-frame direction normalise(1, sin beta, sin alpha)
     * (sensor.py:66-71) and the obstacle-avoidance weight beta_oa (docking3d.py:786-788).  Read during create only. */
    const double* ray_table;
    dockauv_vehicle vehicle[2];
    /* Gauss-Markov current with sigma > 0 (objects/current.py:88, w = np.random.normal(0, sigma)) when the caller
     * passes no noise array: 0 = w = 0 (what every shipped scenario has: white_noise_std = 0, docking3d.py:820);
     * 1 = the kernel draws w = sigma_env * N(0, 1) itself -- Philox4x32-10 counter (env, episode, t_steps, 1), key =
     * seed, Box-Muller on the first two words (oracle/philox_ref.py: philox_normal); sigma_env = field
     * DOCKAUV_F_CURRENT_SIGMA.  dockauv_step_io.noise, when given, always wins (parity mode). */
    int32_t device_noise;
    int32_t reserved0;
} dockauv_config;

typedef struct dockauv_env_s* dockauv_handle;

/* per-env fields addressable from the host (width = doubles per env) */
#define DOCKAUV_F_STATE 0        /* 12: eta(6), nu_r(6)                       (objects/auvsim.py:37,162-246) */
#define DOCKAUV_F_U 1            /* DOCKAUV_MAX_U: filtered input u           (objects/auvsim.py:277-284) */
#define DOCKAUV_F_GOAL 2         /* 4: goal x y z, heading_goal_reached       (docking3d.py:194,202) */
#define DOCKAUV_F_CURRENT 3      /* 5: V_c V_min V_max alpha beta             (objects/current.py:20-31) */
#define DOCKAUV_F_TSTEPS 4       /* 1: steps in this episode                  (docking3d.py:139) */
#define DOCKAUV_F_CAPSULES 5     /* max_capsules*7: bot xyz, top xyz, radius (radius <= 0: unused slot) */
#define DOCKAUV_F_SPHERES 6      /* max_spheres*4: centre xyz, radius (radius <= 0: unused slot) */
#define DOCKAUV_F_VEHICLE_ID 7   /* 1: index into config.vehicle[] (mixed batches) */
#define DOCKAUV_F_CUM_REWARD 8   /* 1: cumulative reward of the running episode (docking3d.py:156) */
#define DOCKAUV_F_EPISODE 9      /* 1: episode counter (docking3d.py:141) */
#define DOCKAUV_F_CURRENT_SIGMA 10 /* 1: white_noise_std of the env's current (objects/current.py:31); read by device_noise */
/* next-episode pool (DOCKAUV_RESET_POOL): same layouts */
#define DOCKAUV_F_POOL_POSE 16       /* 6: position, attitude */
#define DOCKAUV_F_POOL_GOAL 17       /* 4 */
#define DOCKAUV_F_POOL_CURRENT 18    /* 5 */
#define DOCKAUV_F_POOL_CAPSULES 19   /* max_capsules*7 */
#define DOCKAUV_F_POOL_SPHERES 20    /* max_spheres*4 */

/*
 * Inputs / outputs of one step.  Replaces the arguments and return tuple of BaseDocking3d.step
 * (envs/docking3d.py:346-402) for a batch.  "T" = float (DOCKAUV_F32) or double (DOCKAUV_F64).
 * In dockauv_step every pointer is a DEVICE pointer; in dockauv_step_host every pointer is a HOST pointer.
 * Nullable members may be NULL.
 */
typedef struct dockauv_step_io {
    const void* actions;     /* T [n_envs][n_u_max] row-major, raw policy output (clipped inside, auvsim.py:74) */
    const void* noise;       /* nullable, T [n_envs]: w_k ~ N(0, sigma) of Current.sim (current.py:88); NULL = 0 */
    float* obs;              /* float32 [n_envs][n_obs] row-major (docking3d.py:462-488); with pack_reward_done = 1:
                                float32 [n_envs][n_obs + 2] = obs | reward | done(0.0/1.0), one dense buffer so that a
                                single all-gather ships everything a learner needs; with pack_reward_done = 2 the
                                observation columns are bfloat16 (round to nearest even), two per 32-bit word:
                                uint32 [n_envs][ceil(n_obs / 2) + 2] = obs pairs (low half first; an odd n_obs is padded
                                with 0) | reward (float32) | done (float32) -- half the bytes over xGMI */
    void* reward;            /* T [n_envs] (docking3d.py:593); nullable when pack_reward_done */
    uint8_t* done;           /* [n_envs] 0/1 (docking3d.py:630); nullable when pack_reward_done */
    void* reward_terms;      /* nullable, T [n_envs][13]: last_reward_arr (docking3d.py:513-588) */
    uint8_t* conditions;     /* nullable, [n_envs]: bit i = condition i (docking3d.py:608-619) */
    void* nav;               /* nullable, T [n_envs][4]: delta_d, delta_theta, delta_psi, delta_heading_goal */
    void* ray_dist;          /* nullable, T [n_envs][n_rays]: clamped intersec_dist (sensor.py:113-118) */
    float* terminal_obs;     /* nullable, float32 [n_envs][n_obs]: written only where done (auto-reset modes) */
    void* state_dot;         /* nullable, T [n_envs][12]: AUVSim._state_dot, the right-hand side at the new state with the
                                new input (objects/auvsim.py:108), what EpisodeDataStorage logs as "states_dot"
                                (utils/datastorage.py:272,299) */
    int32_t pack_reward_done; /* 0 / 1 / 2, see obs */
    int32_t reserved;
} dockauv_step_io;

/* library / build info; callable without a GPU */
int dockauv_abi_version(void);
const char* dockauv_build_info(void);
/* message of the last failure on this handle (h may be NULL: last failure of create) */
const char* dockauv_last_error(dockauv_handle h);

/* BaseDocking3d.__init__ (docking3d.py:48-220) for a batch: allocates the SoA state in HBM of `device` */
int dockauv_create(const dockauv_config* cfg, int device, dockauv_handle* out);
int dockauv_destroy(dockauv_handle h);

/* derived sizes: n_obs = 16 + n_rays_reduced (docking3d.py:114-115), n_rays (sensor.py:63), n_u_max */
int dockauv_n_obs(dockauv_handle h);
/* waves x 64 = threads per 64-env group the handle's step kernels run with (dockauv_config::threads_per_group, or the
 * library's choice for this workload and batch size when that was 0).  No reference counterpart: a tuning read-out. */
int dockauv_threads_per_group(dockauv_handle h);
/* 1: the next plain step (mandatory outputs, packed rows) runs the general step kernel; 0: the lean one that leaves the water
 * current out.  The lean kernels exist for the float32 group shapes of BlueROV2 (256 threads) and LAUV-with-fan (512 threads)
 * handles and are picked while the handle has no current: a scenario whose generator draws none (SimpleDocking3d,
 * CapsuleDocking3d, ObstaclesDocking3d, ObstaclesNoCapDocking3d, SphereDocking3d) and no dockauv_set_field of
 * DOCKAUV_F_CURRENT / DOCKAUV_F_POOL_CURRENT rows other than exact zeros since dockauv_create; the first such write switches the
 * handle to the general kernels for good.  Same results either way, bit for bit.  No reference counterpart: a tuning read-out. */
int dockauv_step_uses_current(dockauv_handle h);
/* 1: the next plain step runs a step kernel that carries the capsule code; 0: the sphere-only one -- the lean kernel above for a
 * BlueROV2 handle with a ray fan, 256 threads per group, no capsule slot and at least one sphere slot.  It goes with the lean
 * kernel: the first non-zero current row switches the handle to the general kernels.  Same results either way, bit for bit. */
int dockauv_step_uses_capsules(dockauv_handle h);
int dockauv_n_rays(dockauv_handle h);
int dockauv_n_u(dockauv_handle h);

/* state access: auv.state / position / attitude setters, goal_location, Current(...), capsules, spheres
 * (docking3d.py:803-988 generate_environment; objects/auvsim.py:174-195).  src/dst: double [count][width]. */
int dockauv_field_width(dockauv_handle h, int field);
int dockauv_set_field(dockauv_handle h, int field, int first, int count, const double* src);
int dockauv_get_field(dockauv_handle h, int field, int first, int count, double* dst);

/* AUVSim.reset + counters of BaseDocking3d.reset (objects/auvsim.py:55-65, docking3d.py:262-276) for envs
 * [first, first+count): state, u, t_steps, cumulative reward -> 0; episode += 1.  Pose/goal/... are then set
 * with dockauv_set_field. */
int dockauv_reset_envs(dockauv_handle h, int first, int count);

/* BaseDocking3d.step (docking3d.py:346-402) for all envs of the handle; device pointers, asynchronous on stream */
int dockauv_step(dockauv_handle h, const dockauv_step_io* io, void* hip_stream);
/* `n` consecutive steps, step i with ios[i] (device pointers), queued back-to-back on `hip_stream` by one call:
 * an open-loop action sequence (the manual / scripted loops of train.py:108-117, 238) without a host round trip per
 * step.  Equivalent to n calls of dockauv_step. */
int dockauv_step_sequence(dockauv_handle h, const dockauv_step_io* ios, int n, void* hip_stream);
/* Fast path of dockauv_step_sequence (ABI 3): when the steps are what the float32 product kernels serve (mandatory outputs as
 * packed rows of one kind, reset mode NONE / DEVICE, reward set 1, fans of 9-16 or 33-64 rays, no logging) they run as
 * RESIDENT launches of up to 64 steps each -- every 64-env group walks its envs through all steps of the launch, step k
 * reading ios[k].actions and writing ios[k].obs, with no launch boundary in between.  The bytes written are exactly those of
 * n single launches (tests/test_gpu_reset.py); what differs is WHEN: rows of different groups belong to different steps
 * while the call is in flight, so the buffers must not be consumed before the call has completed on the stream (an
 * open-loop sequence; a policy in the loop uses dockauv_step).  On by default; dockauv_set_option switches it per handle. */
#define DOCKAUV_OPT_SEQUENCE_RESIDENT 1   /* value 0: dockauv_step_sequence launches its steps one by one */
int dockauv_set_option(dockauv_handle h, int option, int value);
/* same with host pointers (staged through the library's pinned buffers; synchronous) */
int dockauv_step_host(dockauv_handle h, const dockauv_step_io* io);
/* block until everything queued on the handle's last-used stream is done */
int dockauv_synchronize(dockauv_handle h);
/* the handle's sticky kernel status WITHOUT any synchronisation (the word lives in host-coherent memory): 0, or
 * DOCKAUV_E_KERNEL once a step kernel that has already run gave up an internal wait.  For device-resident rollouts that
 * never call a synchronising entry point (the reference has no counterpart: its step() raises in the caller's thread);
 * cheap enough for every step. */
int dockauv_poll_status(dockauv_handle h);

/*
 * Episode storage for selected envs of a batch (utils/datastorage.py:164-343 EpisodeDataStorage, hooked at
 * docking3d.py:252-259,363-364): a ring of the last `capacity` steps of `n_rows` chosen envs, kept in HBM and written
 * by the step kernel itself, so that a device-resident rollout (no host round trip per step) can still hand the
 * reference's per-step arrays to its post-analysis.  Per step and selected env the kernel records: the state the step
 * started from, the new state, _state_dot, the filtered input u, nu_c (body frame, first three), the observation
 * BEFORE any auto-reset zeroing, the 13 reward terms and the condition bits.  Row of step k: k % capacity.
 * dockauv_trace_enable(h, env_ids, n_rows, capacity): env_ids host array, strictly increasing; n_rows = 0 switches
 *   the trace off and frees the ring.  The step counter restarts at 0.  Every call first releases the ring of an earlier
 *   enable -- also a call that is then refused (DOCKAUV_E_INVALID: no ids / capacity < 1; DOCKAUV_E_RANGE: ids not strictly
 *   increasing inside [0, n_envs)): after a refused call the trace is off.
 * dockauv_trace_steps(h): steps recorded since enable (or a negative error code).
 * dockauv_trace_read(h, first_step, n_steps, ...): copies steps [first_step, first_step + n_steps) -- they must still be
 *   in the ring -- to host arrays [n_steps][n_rows][width] (float64, obs float32, conditions uint8); any of the output
 *   pointers may be NULL.  Synchronises with the handle's last-used stream.
 */
int dockauv_trace_enable(dockauv_handle h, const int32_t* env_ids, int n_rows, int capacity);
long long dockauv_trace_steps(dockauv_handle h);
int dockauv_trace_read(dockauv_handle h, long long first_step, int n_steps, double* state_pre /*12*/, double* state /*12*/,
                       double* state_dot /*12*/, double* u /*DOCKAUV_MAX_U*/, double* nu_c /*3*/, float* obs /*n_obs*/,
                       double* reward_terms /*13*/, uint8_t* conditions /*1*/);

/* measurement helper (bench.py): run `steps` step launches back-to-back on `stream` re-using the same io, each
 * dispatch carrying its own start/stop HIP events ON THAT STREAM; returns the average KERNEL duration in microseconds
 * (launch gaps excluded -- comparable with rocprofv3 --kernel-trace). */
int dockauv_time_steps(dockauv_handle h, const dockauv_step_io* io, void* hip_stream, int steps, double* avg_us);

/*
 * Multi-GPU: peer-to-peer gather of the packed [obs | reward | done] rows over xGMI ("keep the
 * collective pluggable"; the default transport is one RCCL all-gather issued by the host through torch.distributed,
 * gym_dockauv_amd/parallel.py).  The reference is single-process and has no counterpart; these entry points replace
 * the concatenation of per-env observations a vectorised caller does on the host (train.py:64-71 consumes it).
 * One process per GPU.  Every rank owns a gather buffer and a flag array, exports them as IPC handles (the host
 * exchanges the 64-byte handles over any channel it has), opens its peers' handles, and per step
 *   1. dockauv_p2p_push: copies its rows into its slice of every rank's gather buffer (one kernel, system-scope
 *      write-through 16-byte stores over the fabric, each wave waits for its acknowledgements);
 *   2. dockauv_p2p_signal_wait: raises stamp t in every peer's flag array and waits -- bounded -- until every peer's
 *      stamp has reached `wait_stamp` in its own.
 * All calls are asynchronous on `hip_stream`.  A wait that runs out of `max_spins` sets bit r (r = late rank) in
 * status[0] and stores the stamp in status[1]; every later wait then returns at once (the grid always drains).
 */
#define DOCKAUV_P2P_HANDLE_BYTES 64
#define DOCKAUV_P2P_MAX_PEERS 15
/* device memory a peer process can map; uncached != 0: fine-grained (what a peer stores is seen by a kernel that is
 * already running: required for flag arrays; far too slow for gather buffers, which are read by later kernels only).
 * `handle` (nullable) receives DOCKAUV_P2P_HANDLE_BYTES bytes. */
int dockauv_p2p_alloc(int device, size_t bytes, int uncached, void** dev_ptr, unsigned char* handle);
int dockauv_p2p_free(void* dev_ptr);
/* map / unmap a peer's allocation on `device` */
int dockauv_p2p_open(int device, const unsigned char* handle, void** dev_ptr);
int dockauv_p2p_close(void* dev_ptr);
/* copy `bytes` from src (16-byte aligned) to each of dsts[0..n_dsts) (local or peer-mapped, 16-byte aligned) */
int dockauv_p2p_push(const void* src, size_t bytes, void* const* dsts, int n_dsts, void* hip_stream);
/* peer_slots[p] = &flags_of_peer_p[my_rank]; my_flags = this rank's flag array [world]; status = uint32 [2] in device
 * memory of this rank; stamp / wait_stamp: 0 = skip that half; stamps compare modulo 2^32 */
int dockauv_p2p_signal_wait(uint32_t* const* peer_slots, int n_peers, const uint32_t* my_flags, int world, int my_rank,
                            uint32_t stamp, uint32_t wait_stamp, uint64_t max_spins, uint32_t* status,
                            void* hip_stream);

/*
 * The same gather as ONE kernel: the blocks copy; the block that finishes last (device counter) raises `stamp` at the
 * peers and waits for `wait_stamp`.  A plan is a plain description of one rank's view of one gather buffer.
 */
typedef struct dockauv_p2p_plan {
    void* dsts[DOCKAUV_P2P_MAX_PEERS + 1];        /* this rank's slice in every rank's gather buffer (own included) */
    uint32_t* peer_slots[DOCKAUV_P2P_MAX_PEERS];  /* &flags_of_peer_p[my_rank] */
    const uint32_t* my_flags;                     /* [world], written by the peers */
    uint32_t* status;                             /* [2], this rank */
    uint32_t* counter;                            /* [1], this rank, zero between gathers */
    uint64_t bytes;                               /* size of the slice */
    uint64_t max_spins;
    int32_t n_dsts, n_peers, world, my_rank;
} dockauv_p2p_plan;
int dockauv_p2p_gather(const dockauv_p2p_plan* plan, const void* src, uint32_t stamp, uint32_t wait_stamp,
                       void* hip_stream);
/*
 * n steps with their gathers, queued by one host call: step i (global step number t0 + i) writes its packed rows to
 * ios[i].obs, which must be row buffer (t0 + i) % 2 of the caller's two; its gather uses plan (t0 + i) % n_plans and
 * stamp t0 + i + 1 (raised at the peers and awaited from them).  On return (asynchronous) `compute_stream` is ordered
 * after every gather queued here.
 * gather_stream == compute_stream, lag 0: step kernel, gather kernel, step kernel, ... in order: every rank holds all
 *   rows of step t before step t + 1 starts.
 * gather_stream == compute_stream, lag 1: the gather of step t RIDES in the grid of step kernel t + 1 (extra workgroups
 *   behind the step groups push the previous rows while the step groups integrate: the fabric transfer is hidden
 *   behind the arithmetic, one launch per step); the last gather gets a kernel of its own.  Needs >= 4 plans, float
 *   kernels, slices that are multiples of 16 bytes.
 * gather_stream != compute_stream (lag 0 or 1 = which stamp a gather awaits): gather kernels on a second stream beside the next step kernel; the step
 *   kernel that next writes the same row buffer waits for that gather.  Five stream/event calls per step on the host
 *   and two cross-stream dependencies: measured slower than one stream at every size on one GPU.
 */
int dockauv_step_gather_sequence(dockauv_handle h, const dockauv_step_io* ios, int n, const dockauv_p2p_plan* plans,
                                 int n_plans, uint64_t t0, int lag, void* compute_stream, void* gather_stream);

/*
 * Closed loop: the library's own policy and a rollout queued by one host call.  Replaces the learner's rollout loop
 * (train.py:64-71: SB3's collect_rollouts, policy forward then env.step, per step) and the prediction loop (train.py:86-119:
 * model.predict then env.step) for a policy that is a small MLP actor -- SB3's MlpPolicy, which train.py:64 instantiates
 * (two hidden layers of 64 tanh units by default, an action_net, a state-independent log_std).  The actor is evaluated by a
 * gfx950 matrix kernel directly on the packed [obs | reward | done] rows the step kernel writes, so that neither Python nor
 * torch nor a graph capture sits between two steps.  Arithmetic is float32 throughout: every pre-activation is one fused
 * multiply-add chain from the bias in a k order fixed by the shapes alone; env i's action depends on row i and the weights
 * only.  The critic, the log-probabilities of the drawn actions and GAE are further below (dockauv_value_*,
 * dockauv_policy_forward_logp, dockauv_gae, dockauv_collect): one host call returns everything a PPO update reads.  Of the
 * update, the library computes the network's share -- the MLP's output on any minibatch of those rows and the gradients of
 * all weights and biases for gradients on that output (dockauv_policy_forward_rows, dockauv_policy_backward, at the end of this
 * header) -- and the PPO head between the two: advantage normalisation, log-probability, ratio and clipping, value loss,
 * entropy, the gradients on both networks' outputs and on log_std, and the statistics SB3 logs (dockauv_ppo_head) -- and the
 * tail of the step: gradient-norm clipping and Adam over all parameters in one launch, then the repack of both networks
 * (dockauv_optim_step, the last entry of this header).
 */
#define DOCKAUV_ACT_NONE 0       /* output: raw (PPO; the step kernel clips, objects/auvsim.py:74) */
#define DOCKAUV_ACT_TANH 1       /* hidden: SB3's default; output: SAC-style squashing */
#define DOCKAUV_ACT_RELU 2       /* hidden only */
#define DOCKAUV_POLICY_MAX_WIDTH 128
/* The MLP actor (SB3 MlpPolicy: mlp_extractor.policy_net + action_net + log_std; train.py:64).  Arrays are read during the
 * call that gets the descriptor (create / load) and not kept. */
typedef struct dockauv_policy_desc {
    uint32_t struct_size;          /* sizeof(dockauv_policy_desc): ABI check */
    int32_t precision;             /* DOCKAUV_F32 only for now; the field is there for a later bf16 mode */
    int32_t n_in, n_hidden[2], n_out;  /* n_in = dockauv_n_obs, widths 1..DOCKAUV_POLICY_MAX_WIDTH, n_hidden[1] == 0: one
                                      hidden layer; n_out = dockauv_n_u */
    int32_t hidden_act, out_act;   /* DOCKAUV_ACT_TANH / _RELU; DOCKAUV_ACT_NONE / _TANH */
    int32_t pointers_on_device;    /* 0: host arrays; 1: device arrays, copied stream-ordered */
    int32_t reserved;
    const float *W1, *b1, *W2, *b2, *W3, *b3;  /* row-major [out][in] = torch.nn.Linear.weight; W2/b2 NULL with one layer */
    const float *log_std;          /* nullable [n_out]: exploration noise exp(log_std[j]) * N(0, 1) when asked for */
    uint64_t seed, env_id_offset;  /* exploration: Philox4x32-10 key; added to the env index in the counter (shards) */
} dockauv_policy_desc;
typedef struct dockauv_policy_s* dockauv_policy;

/* MlpPolicy(...) of train.py:64 for the actor part: validates the descriptor (every failure DOCKAUV_E_INVALID, the message
 * names the field; the descriptor's own fields first, then what must match the handle: float32 handle, n_in == dockauv_n_obs,
 * n_out == dockauv_n_u) before any device call, then uploads the weights.  A policy belongs to its handle's device and is
 * destroyed before the handle.  Errors of the policy calls are reported through dockauv_last_error(h). */
int dockauv_policy_create(dockauv_handle h, const dockauv_policy_desc* d, dockauv_policy* out);
/* policy.load_state_dict: new weights of the same shapes and activations (what a learner on the same GPU calls once per
 * iteration, train.py:64-71, with pointers_on_device = 1: no host round trip, ordered on the stream; seed / env_id_offset
 * are taken over as well). */
int dockauv_policy_load(dockauv_policy p, const dockauv_policy_desc* d, void* hip_stream);
int dockauv_policy_destroy(dockauv_policy p);
/* policy.predict / the actor's forward (train.py:86-119) for all envs of the handle; device pointers, asynchronous on stream.
 * rows: float32 [n_envs][n_obs + 2] packed rows (only the first n_obs columns are read); actions: float32 [n_envs][n_u].
 * stochastic != 0 with a loaded log_std: a = mean + exp(log_std[j]) * z before the output activation, z the standard normal
 * of Philox4x32-10 counter (env_id_offset + i, t mod 2^32, j, 2), key = seed, Box-Muller cos branch on the first two words
 * (slots 0 and 1 of the last counter word belong to the episode generator and the current noise). */
int dockauv_policy_forward(dockauv_handle h, dockauv_policy p, const float* rows, float* actions,
                           uint64_t t, int stochastic, void* hip_stream);
/* The rollout loop of train.py:64-71 (learner) / 86-119 (predict): n_steps x (policy, step) queued back to back on the stream
 * by this one call, asynchronous.  rows_out: float32 [n_steps][n_envs][n_obs + 2]; actions_out: float32
 * [n_steps][n_envs][n_u]; terminal_obs: nullable float32 [n_steps][n_envs][n_obs].  Step k: the policy reads rows_in (k = 0)
 * or rows_out[k - 1] and writes actions_out[k] with counter t = t0 + k; dockauv_step reads actions_out[k] and writes
 * rows_out[k] (pack_reward_done = 1, the handle's reset mode, terminal_obs[k] when given).  Exactly the launches of
 * 2 n_steps calls of dockauv_policy_forward / dockauv_step; the resident sequence path is not used.  Returns what
 * dockauv_poll_status returns, looked at once after queueing. */
int dockauv_rollout(dockauv_handle h, dockauv_policy p, const float* rows_in, float* rows_out, float* actions_out,
                    float* terminal_obs, int n_steps, uint64_t t0, int stochastic, void* hip_stream);

/*
 * The PPO collector: what SB3's collect_rollouts + RolloutBuffer.compute_returns_and_advantage (train.py:64-71; gamma /
 * gae_lambda of config/DRL_hyperparams.py) hand to the update -- V(s), log pi(a|s), advantages and returns -- computed on the
 * device from the rollout's own buffers.  All pointers are device pointers, every call is asynchronous on the stream.
 *
 * The critic (SB3 MlpPolicy: mlp_extractor.value_net + value_net) is a dockauv_policy with a value role: the same descriptor,
 * widths (<= 128, one or two hidden layers), packing and upload as the actor, with n_out == 1 and out_act == DOCKAUV_ACT_NONE;
 * log_std, seed and env_id_offset are ignored.  dockauv_policy_load and dockauv_policy_destroy work on it;
 * dockauv_policy_forward, dockauv_rollout and every actor argument refuse it, every critic argument refuses an actor.
 */
int dockauv_value_create(dockauv_handle h, const dockauv_policy_desc* d, dockauv_policy* out);
/* values[r] = V(rows[r][0 .. n_obs)) for n_rows packed rows of stride n_obs + 2: any number of rows, not tied to n_envs, so
 * that the [K][N] rows of a rollout go in one launch (the actor's kernel with one output unit: one group per 128 rows).  A
 * row's value is a function of the row and the weights only. */
int dockauv_value_forward(dockauv_handle h, dockauv_policy critic, const float* rows, long long n_rows, float* values,
                          void* hip_stream);
/* dockauv_policy_forward that also writes the log-probability of what it drew, log_prob: float32 [n_envs]:
 *   log_prob[i] = sum_j (-z_ij^2 / 2 - log_std[j] - log(2 pi) / 2),  z the normal the kernel drew (0 with stochastic == 0).
 * In float32: term_j = fmaf(-0.5f * z, z, -(log_std[j] + 0.918938533f)); (term_0 + .. + term_3) + (term_4 + .. + term_7), each
 * sum from 0.0f in the order of j.  The actions are bit for bit those of dockauv_policy_forward.  Refused when the policy has
 * no log_std, and when out_act == DOCKAUV_ACT_TANH: the log-probability of a squashed action needs the correction
 * -sum_j log(1 - tanh(x_j)^2), which only the squashed-Gaussian actor has (dockauv_sac_actor_create, at the end of this header:
 * for that role this call writes the squashed log-probability stated there). */
int dockauv_policy_forward_logp(dockauv_handle h, dockauv_policy p, const float* rows, float* actions, float* log_prob,
                                uint64_t t, int stochastic, void* hip_stream);
/* RolloutBuffer.compute_returns_and_advantage on the rows of a rollout.  rows_out: float32 [n_steps][n_envs][n_obs + 2] (only
 * the reward and done columns are read); values: float32 [n_steps + 1][n_envs], values[k] = V of the observation the actor saw
 * at step k, values[n_steps] = V(rows_out[n_steps - 1]); advantages, returns: float32 [n_steps][n_envs].  Per env, backwards
 * from k = n_steps - 1 with gae = 0, in exactly this float32 order (the library is built with -ffp-contract=on: only the fmaf
 * written here are fused):
 *   nt    = done[k] > 0.5f ? 0.0f : 1.0f
 *   gnt   = gamma * nt
 *   delta = fmaf(gnt, values[k + 1], reward[k]) - values[k]
 *   gae   = fmaf((gamma * gae_lambda) * nt, gae, delta)
 *   advantages[k] = gae;  returns[k] = gae + values[k]
 * Every done is terminal: the reference's env reports no truncation flag (docking3d.py:630), and the row after a done holds the
 * reset observation, whose value is masked out by nt (dockauv_gae_truncated, below, bootstraps the dones that are time limits).
 * gamma and gae_lambda must lie in [0, 1]. */
int dockauv_gae(dockauv_handle h, const float* rows_out, const float* values, int n_steps, float gamma, float gae_lambda,
                float* advantages, float* returns, void* hip_stream);
/* One PPO iteration's collection. */
typedef struct dockauv_collect_io {
    uint32_t struct_size;          /* sizeof(dockauv_collect_io): ABI check */
    int32_t n_steps;               /* K >= 1 */
    const float* rows_in;          /* [n_envs][n_obs + 2]: the rows the actor reads at step 0 */
    float* rows_out;               /* [K][n_envs][n_obs + 2] */
    float* actions_out;            /* [K][n_envs][n_u] */
    float* terminal_obs;           /* nullable [K][n_envs][n_obs] */
    float* log_prob;               /* nullable [K][n_envs] */
    float* values;                 /* [K + 1][n_envs]; NULL without a critic, like advantages and returns */
    float* advantages;             /* [K][n_envs] */
    float* returns;                /* [K][n_envs] */
    uint64_t t0;                   /* counter of step 0 (dockauv_rollout) */
    int32_t stochastic;
    float gamma, gae_lambda;       /* in [0, 1] */
    int32_t reserved;
} dockauv_collect_io;
/* Queues exactly: the launches of dockauv_rollout (the actor in its dockauv_policy_forward_logp form when io->log_prob is
 * given, writing log_prob[k]); one value launch on rows_in -> values[0]; one value launch on all of rows_out -> values[1 .. K];
 * one GAE launch.  critic == NULL: rollout and log-probabilities only (values / advantages / returns must be NULL).  Returns
 * what dockauv_poll_status returns, looked at once after queueing. */
int dockauv_collect(dockauv_handle h, dockauv_policy actor, dockauv_policy critic, const dockauv_collect_io* io,
                    void* hip_stream);

/*
 * The truncation bootstrap of SB3's collect_rollouts: where an episode ends on the time limit and on nothing else
 * (infos[idx]["TimeLimit.truncated"]), rewards[idx] += gamma * V(terminal_observation).  The reference's env has no such flag
 * (docking3d.py:630) and dockauv_gae treats every done as terminal; in this env time is not part of the observation, so that
 * teaches the critic that a state is worth nothing whenever the clock runs out.  These calls are the opt-in alternative, computed
 * on the device from what a collection already holds; without them every call queues exactly what it queued before.
 *
 * A done at step k is TRUNCATED iff the episode monitor gives it outcome 3 (dockauv_monitor_scan: the same float32 comparisons on
 * the clipped terminal observation t, the same length carry):
 *   len > max_timesteps  and not  (t[0] == 0.0f || t[0] == 1.0f || fabsf(t[6]) == 1.0f || fabsf(t[7]) == 1.0f)
 * so a goal reached or an attitude limit hit on the last allowed step is terminal, and the two limits of the monitor's rule hold
 * here too.  len is the monitor's: length_carry + the steps so far, zero after every done.
 *
 * Slots.  A truncated episode has exactly max_timesteps + 1 steps and the carry before step 0 is at most max_timesteps, so an
 * env truncates at most (K - 1) / (max_timesteps + 1) + 1 times in K steps.  dockauv_truncation_slots returns
 * n_slots = K / (max_timesteps + 1) + 1 (never less; 1 at the default 1000 for K = 128; -1 for a NULL handle or K < 1).  The scan
 * writes env's s-th truncated step, in step order, to slot s of two tables laid out [n_slots][n_envs]:
 *   trunc_step[s][env] = k                      (-1 in unused slots)
 *   trunc_row[s][env]  = k * n_envs + env       (the row of terminal_obs; env in unused slots: a row that exists)
 * and writes the new length carry back.  No atomics and no compaction pass: the per-env slots are the compaction.
 *
 * dockauv_truncation_scan: that scan alone, one launch.  Needs rows_out, terminal_obs, length_carry, trunc_step, trunc_row.
 * dockauv_gae_truncated: three launches -- the scan; the critic on the n_slots * n_envs rows terminal_obs[trunc_row[.]] ->
 *   v_terminal [n_slots][n_envs] (the kernel of dockauv_policy_forward_rows with a row stride of n_obs: a row's value is a
 *   function of the row and the weights only, bit for bit dockauv_value_forward on the same observation; values of unused slots
 *   are unspecified and never used); GAE with the bootstrap.  Per env, backwards as dockauv_gae, in exactly this float32 order:
 *     nt    = done[k] > 0.5f ? 0.0f : 1.0f
 *     gnt   = gamma * nt
 *     rb    = k == trunc_step[s][env] for a slot s ? fmaf(gamma, v_terminal[s][env], reward[k]) : reward[k]
 *     delta = fmaf(gnt, values[k + 1], rb) - values[k]          (nt = 0 there, as for any done: gae does not cross the reset)
 *     gae   = fmaf((gamma * gae_lambda) * nt, gae, delta)
 *     advantages[k] = gae;  returns[k] = gae + values[k]
 *   Without a truncated step the bits are dockauv_gae's.  The reward columns, values and log-probabilities are not touched (the
 *   monitor's returns stay sums of raw rewards, as SB3's Monitor wrapper sees them).
 * dockauv_collect_truncated: dockauv_collect with dockauv_gae_truncated's three launches in place of the GAE launch; in front of
 *   the rollout, on the stream, length_carry <- the handle's own step counters (DOCKAUV_F_TSTEPS; a device-to-device copy, as
 *   dockauv_monitor_sync reads them).  The critic and cio->terminal_obs are required; n_steps, rows_out, terminal_obs, values,
 *   advantages, returns, gamma and gae_lambda of the two blocks must agree.
 * All pointers are device pointers, the workspaces belong to the caller, no call allocates, every call is asynchronous on the
 * stream.  Refused before any device call (DOCKAUV_E_INVALID, the message naming the field): a NULL handle, critic, io or required
 * pointer; a wrong struct_size; n_steps < 1; n_slots below dockauv_truncation_slots; a handle whose max_timesteps is < 1; gamma
 * or gae_lambda outside [0, 1]; a float64 handle; a handle with DOCKAUV_RESET_NONE (an episode does not restart at the row after
 * a done); an actor passed as critic.
 */
typedef struct dockauv_truncation_io {
    uint32_t struct_size;          /* sizeof(dockauv_truncation_io): ABI check */
    int32_t n_steps;               /* K >= 1 */
    int32_t n_slots;               /* >= dockauv_truncation_slots(h, K) */
    float gamma, gae_lambda;       /* in [0, 1] */
    int32_t reserved;
    const float* rows_out;         /* [K][n_envs][n_obs + 2]: the reward and done columns are read */
    const float* terminal_obs;     /* [K][n_envs][n_obs]: read where done (the scan: columns 0, 6, 7; the critic: all) */
    const float* values;           /* [K + 1][n_envs] (dockauv_gae) */
    int32_t* length_carry;         /* [n_envs] workspace: steps of every env's episode before step 0; the scan writes it back */
    int32_t* trunc_step;           /* [n_slots][n_envs] workspace */
    int64_t* trunc_row;            /* [n_slots][n_envs] workspace */
    float* v_terminal;             /* [n_slots][n_envs] workspace */
    float* advantages;             /* [K][n_envs] */
    float* returns;                /* [K][n_envs] */
} dockauv_truncation_io;
int dockauv_truncation_slots(dockauv_handle h, int n_steps);
int dockauv_truncation_scan(dockauv_handle h, const dockauv_truncation_io* io, void* hip_stream);
int dockauv_gae_truncated(dockauv_handle h, dockauv_policy critic, const dockauv_truncation_io* io, void* hip_stream);
int dockauv_collect_truncated(dockauv_handle h, dockauv_policy actor, dockauv_policy critic, const dockauv_collect_io* cio,
                              const dockauv_truncation_io* tio, void* hip_stream);

/*
 * The network's share of the update (PPO.train of train.py:64-71: the MlpPolicy forward on a minibatch and autograd's backward
 * through it), for an actor and for a critic alike.  All pointers are device pointers, both calls are asynchronous on the
 * stream, the weights are the ones the policy holds at that point of the stream (dockauv_policy_load).
 *
 * out[r][0 .. n_out) = W3 h_last + b3 of packed row rows[row_index ? row_index[r] : r], r < n_rows: the output BEFORE out_act
 * and without exploration noise.  rows: float32, row stride n_obs + 2, only the first n_obs columns are read; row_index:
 * nullable int64 [n_rows] (a minibatch, e.g. of torch.randperm; duplicates allowed, the range is the caller's contract); out:
 * float32 [n_rows][n_out].  Bit for bit what dockauv_policy_forward (deterministic, out_act NONE) and dockauv_value_forward give
 * for the same row.
 */
int dockauv_policy_forward_rows(dockauv_handle h, dockauv_policy p, const float* rows, const int64_t* row_index,
                                long long n_rows, float* out, void* hip_stream);
/* The gradients dockauv_policy_backward writes: torch.nn.Linear layout ([out][in], [out]), float32, overwritten (not
 * accumulated).  dW2 / db2 are NULL with one hidden layer. */
typedef struct dockauv_policy_grads {
    uint32_t struct_size;          /* sizeof(dockauv_policy_grads): ABI check */
    uint32_t reserved;
    float *dW1, *db1, *dW2, *db2, *dW3, *db3;
} dockauv_policy_grads;
/* grad_out: float32 [n_rows][n_out] = dL/d(out), out as dockauv_policy_forward_rows defines it.  Per row r, summed over r in
 * float32:  db3 = sum g_r;  dW3 = sum g_r (x) h_last,r;  delta = (W3^T g_r) . act'  and so on down to dW1 = sum delta1,r (x) x_r,
 * with tanh' = 1 - h^2 of the recomputed h and relu' = 1 where the pre-activation is > 0, else 0 (torch's convention).  No
 * gradient with respect to the rows.
 * Reproducible: no floating-point atomics; two calls with the same inputs give the same bits, and rows reached through row_index
 * give the same bits as the same rows laid out densely in that order (the summation order is a function of the position in the
 * minibatch, n_rows and the shapes only).
 * Workspace: the library owns the per-group partial sums (at most 256 groups, each looping over its share of the rows, then a
 * second launch that adds the partials in group order); their size does not depend on n_rows.  They are allocated at the first
 * backward of a policy and freed by dockauv_policy_destroy; later calls allocate nothing.
 * The kernel keeps the weights (torch.nn.Linear layout, padded), one pass's rows, activations and deltas in LDS.  Shapes whose
 * need exceeds the 160 KiB are refused with a message that names it: a 128-128 network takes n_obs <= 62, narrower networks
 * wider observations. */
int dockauv_policy_backward(dockauv_handle h, dockauv_policy p, const float* rows, const int64_t* row_index, long long n_rows,
                            const float* grad_out, const dockauv_policy_grads* grads, void* hip_stream);

/*
 * The PPO head on one minibatch of B = n_rows rows (the loss block of SB3's PPO.train, train.py:64-71): everything between
 * dockauv_policy_forward_rows and dockauv_policy_backward.  All pointers are device pointers, float32; asynchronous on the
 * stream.  mean [B][n_out] and v [B] are the actor's and the critic's dockauv_policy_forward_rows outputs for the minibatch;
 * the row arrays actions [M][n_out], log_prob_old [M], advantages [M], returns [M] are read at i = row_index ? row_index[r] : r
 * (the same index the forward took; duplicates allowed, the range is the caller's contract); log_std is the one the actor
 * holds at this point of the stream (dockauv_policy_load).  For row r, in exactly this float32 order (only the fmaf written
 * here are fused); m and s are the mean and the unbiased (n - 1) standard deviation of the minibatch's advantages:
 *   A      = normalize_advantage ? (adv_i - m) / (s + 1e-8f) : adv_i
 *   z_j    = (a_ij - mean_rj) * expf(-log_std[j])
 *   term_j = fmaf(-0.5f * z_j, z_j, -(log_std[j] + 0.918938533f))
 *   logp   = (term_0 + .. + term_3) + (term_4 + .. + term_7), each sum from 0.0f in the order of j (dockauv_policy_forward_logp)
 *   lr     = logp - log_prob_old_i;  ratio = expf(lr)
 *   live   = !((A > 0 && ratio > 1.0f + clip_range) || (A < 0 && ratio < 1.0f - clip_range))
 *   surr   = fminf(ratio * A, fminf(fmaxf(ratio, 1.0f - clip_range), 1.0f + clip_range) * A)
 *   g      = live ? -(A * ratio) / (float)B : 0.0f                              (= d loss / d logp_r)
 *   grad_mean[r][j] = (g * z_j) * expf(-log_std[j])
 *   dv     = v_r - ret_i;  grad_v[r] = ((2.0f * vf_coef) * dv) / (float)B
 * and the sums over the rows, each accumulated in float64 from the float32 per-row terms and rounded to float32 once:
 *   policy_loss   = -(sum surr) / B;  value_loss = (sum dv * dv) / B
 *   approx_kl     = (sum ((ratio - 1.0f) - lr)) / B;  clip_fraction = (rows with fabsf(ratio - 1.0f) > clip_range) / B
 *   grad_log_std[j] = (float)(sum g * fmaf(z_j, z_j, -1.0f)) - ent_coef
 *   entropy_loss  = -(e_0 + e_1 + ..), e_j = 1.418938533f + log_std[j], from 0.0f in the order of j
 *   loss          = fmaf(vf_coef, value_loss, fmaf(ent_coef, entropy_loss, policy_loss))
 * stats: loss, policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction, m, s (0 and 1 without normalisation).
 * m and s: a group of the first launch forms the float64 sum of its advantages, then -- reading them again -- the float64 sum
 * of the float32 squares (adv - c)^2 about c = the float32 of its own mean; m is the float64 sum of the groups' sums over B, and
 * the squares are moved from the groups' centres to m in float64 (sum (x - m)^2 = sum (x - c)^2 + 2 (c - m) sum (x - c) +
 * n_g (c - m)^2, exact algebra between numbers of the same size: nothing cancels, as it would in sum x^2 - n m^2).
 * v == NULL: no critic; grad_v must be NULL too, value_loss is 0 and returns is not read.
 * Reproducible: no floating-point atomics.  A bounded grid of at most 256 groups of 256 lanes, a lane taking every 256th row of
 * a pass of 1 024; a group's sums are added over the lanes by a fixed tree and the groups' partials in group order, so the
 * bits depend on the inputs, on a row's position in the minibatch and on B only: two calls give the same bits, and rows reached
 * through row_index the bits of the same rows laid out densely.  At most three launches (moments, rows, final sums; two
 * without normalisation).  The workspace (32 KiB) belongs to the actor: allocated at its first head call, freed by
 * dockauv_policy_destroy.  Every head call on one actor uses that one workspace, so the calls on one actor must be ordered on
 * one stream (or by events): two calls on different streams race on it.  The first call on an actor allocates (hipMalloc, which
 * synchronises the device), so make it before a stream capture, not inside one; later calls allocate nothing.  The same two
 * rules hold for dockauv_policy_backward and its partial sums.
 * Refused before any device call, the message naming the field: a NULL handle, policy or io; a critic as `actor`; an actor
 * without log_std or with out_act == DOCKAUV_ACT_TANH (as dockauv_policy_forward_logp); a wrong struct_size; n_rows < 1, or
 * < 2 with normalize_advantage; clip_range <= 0; a NULL mean / actions / log_prob_old / advantages / grad_mean / grad_log_std /
 * stats; returns NULL with a critic; exactly one of v and grad_v NULL.
 */
typedef struct dockauv_ppo_head_io {
    uint32_t struct_size;          /* sizeof(dockauv_ppo_head_io): ABI check */
    int32_t normalize_advantage;
    const float *mean, *v;         /* [B][n_out]; [B], NULL: no critic (value terms 0, grad_v must be NULL) */
    const float *actions, *log_prob_old, *advantages, *returns;   /* row arrays, read at row_index[r] */
    const int64_t* row_index;      /* nullable [B]; duplicates allowed; range is the caller's contract */
    long long n_rows;              /* B >= 1; >= 2 with normalize_advantage */
    float clip_range, vf_coef, ent_coef;   /* clip_range > 0 */
    int32_t reserved;
    float *grad_mean, *grad_v, *grad_log_std;   /* [B][n_out], [B], [n_out]: overwritten; must not alias the inputs */
    float* stats;                  /* [8]: loss, policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction, adv mean, adv std */
} dockauv_ppo_head_io;
int dockauv_ppo_head(dockauv_handle h, dockauv_policy actor, const dockauv_ppo_head_io* io, void* hip_stream);

/*
 * The optimiser: the tail of a PPO minibatch step (SB3's PPO.train, train.py:64-71: clip_grad_norm_ and Adam.step, SB3's
 * Adam with eps 1e-5), in one launch over all parameters, followed by the repack of both networks -- so that a learner on the C
 * ABI needs neither torch nor a dockauv_policy_load between minibatches.  All pointers are device pointers, float32; the step is
 * asynchronous on the stream and does not synchronise.
 *
 * A dockauv_optim belongs to one actor (with a log_std) and, optionally, one critic of the same handle.  It owns the first and
 * second moments m and v (zero at create) and the step count t (0 at create); everything is allocated at create, a step
 * allocates nothing.  Destroy it before its policies.
 *
 * One step covers one index space: actor W1 b1 W2 b2 W3 b3, log_std, critic W1 b1 W2 b2 W3 b3 (torch.nn.Linear layout, the
 * shapes of the policies; W2 / b2 are empty with one hidden layer, the critic's arrays without a critic).
 * The gradient norm: sum = the float64 sum of (double)g * (double)g over the whole index space -- lane t of a group of 1 024
 * takes the elements t, t + 1 024, .. of each array in turn, the lanes of a wave are added by a fixed tree, the sixteen waves in
 * order --, then
 *   norm = (float)sqrt(sum)
 *   coef = max_grad_norm > 0 ? fminf(1.0f, max_grad_norm / (norm + 1e-6f)) : 1.0f          (torch's clip_grad_norm_)
 * Every group of the launch forms the whole sum itself, in that order, so every element is scaled by the same coef bit for bit
 * and no pass between groups is needed.  The host supplies, computed in double from the step count t >= 1 (incremented by the
 * call before use) and rounded once:
 *   c1 = (float)(1 - beta1);  c2 = (float)(1 - beta2);  b2 = (float)beta2
 *   step_size = (float)(lr / (1 - beta1^t));  rsq = (float)(1 / sqrt(1 - beta2^t))
 * and per element, in exactly this float32 order (the library is built with -ffp-contract=on: only the fmaf written here are
 * fused):
 *   g     = grad * coef
 *   m     = fmaf(c1, g - m, m)
 *   v     = fmaf(c2 * g, g, b2 * v)
 *   denom = fmaf(sqrtf(v), rsq, eps)
 *   p     = p - step_size * (m / denom)
 * p, m and v are written in place, the gradients are only read.  No weight decay, no amsgrad (torch.optim.Adam's defaults).
 * stats (nullable [2]): the norm before clipping, coef.
 * Reproducible: no floating-point atomics; the bits depend on the gradients, the state and the shapes only.
 *
 * After the update dockauv_optim_step repacks both networks from the updated arrays (what dockauv_policy_load with
 * pointers_on_device = 1 does, log_std included): at that point of the stream the actor and the critic hold the new weights,
 * and the next dockauv_collect / dockauv_policy_forward_rows needs no dockauv_policy_load.  Launches: the step, then per network
 * the pack (the actor's with the copy of its log_std).
 * Stream capture: the bias corrections are host scalars of the call, so a captured graph would replay ONE step's corrections (and
 * the count would not advance): do not capture the step.
 * After a dockauv_ppo_update with target_kl > 0 on this optimiser the count is pending (how many of its steps were applied is
 * known to the device only): the step then first synchronises the stream that update ran on and reads the count back.
 * Refused before any device call (DOCKAUV_E_INVALID, the message naming the field): a NULL handle, optimiser, desc or io; a wrong
 * struct_size; a critic as `actor` or an actor as `critic`; policies of another handle; an actor without log_std; beta1 or beta2
 * outside [0, 1); eps <= 0; lr < 0 or not finite; a NULL among the pointers the shapes require; a non-NULL pointer where the
 * shapes have none; a grads pointer equal to its params pointer.
 */
typedef struct dockauv_optim_s* dockauv_optim;
typedef struct dockauv_optim_desc {
    uint32_t struct_size;          /* sizeof(dockauv_optim_desc): ABI check */
    uint32_t reserved;
    double beta1, beta2;           /* in [0, 1) */
    double eps;                    /* > 0 (SB3's PPO: 1e-5) */
    float max_grad_norm;           /* <= 0: no clipping */
    float reserved1;
} dockauv_optim_desc;
int dockauv_optim_create(dockauv_handle h, dockauv_policy actor, dockauv_policy critic /* nullable */,
                         const dockauv_optim_desc* d, dockauv_optim* out);
int dockauv_optim_destroy(dockauv_optim o);   /* NULL: 0 */
typedef struct dockauv_optim_io {
    uint32_t struct_size;          /* sizeof(dockauv_optim_io): ABI check */
    uint32_t reserved;
    double lr;                     /* >= 0, finite; per call (SB3 schedules it) */
    float* actor_params[6];        /* W1 b1 W2 b2 W3 b3; index 2, 3 NULL with one hidden layer */
    float* log_std;                /* [n_out] */
    const float* actor_grads[6];
    const float* grad_log_std;
    float* critic_params[6];       /* all NULL without a critic */
    const float* critic_grads[6];
    float* stats;                  /* nullable [2]: gradient norm before clipping, coef */
} dockauv_optim_io;
int dockauv_optim_step(dockauv_handle h, dockauv_optim o, const dockauv_optim_io* io, void* hip_stream);
/* The optimiser's state, for inspection and checkpoints: device pointers to m and v ([*n_elements] each, in index-space order,
 * owned by the optimiser and valid until dockauv_optim_destroy) and the number of steps taken.  Any output may be NULL.
 * While the count is pending (after a dockauv_ppo_update with target_kl > 0) the call first synchronises the stream that update
 * ran on and reads the count back from the device. */
int dockauv_optim_state(dockauv_optim o, float** m, float** v, long long* n_elements, long long* steps);

/*
 * A keyed pseudo-random permutation of 0 .. n - 1 on the device, the shuffle of dockauv_ppo_update (the reference's counterpart:
 * the np.random.permutation of SB3's RolloutBuffer.get): out[i] = P(i), int64 [n] in device memory, P a bijection of [0, n) that
 * is a function of (seed, epoch, n) alone.  One launch, one lane per output, no sort and no workspace; asynchronous on the stream.
 * The construction is the bijective shuffle of Mitchell, Stokes, Frank and Holmes, "Bandwidth-optimal random shuffling for GPUs"
 * (2022) -- a Feistel network on b bits with cycle-walking --, in exact unsigned integer arithmetic:
 *   b  = max(2, bit_length(n - 1));  wl = b / 2 (the left half: the HIGH bits);  wr = b - wl
 *   k_0 .. k_3, k_4 .. k_7 = the words of the Philox4x32-10 blocks of counter (q, epoch mod 2^32, 0, 3), q = 0, 1, key = (seed mod
 *     2^32, seed >> 32).  Counter word 3 names the stream: the episode generator uses 0, the current's noise 1, the policy's
 *     exploration noise 2, this permutation 3.
 *   N(x), x < 2^b:  L = x >> wr;  R = x mod 2^wr;  then eight rounds r = 0 .. 7, w = the width of L (wl in the even rounds, wr in
 *     the odd ones: the two widths swap with the halves):
 *       t = ((R + k_r) mod 2^32) * 0xD2511F53            (a 64-bit product)
 *       f = (t >> 32) ^ (t mod 2^32);  f = (f ^ (f >> 15)) mod 2^w
 *       (L, R) = (R, L ^ f)
 *     N(x) = L * 2^wr + R.  Every round is invertible (L ^ f is undone by the same f of R), so N is a bijection of [0, 2^b).
 *   P(i) = N(i), and while the result is >= n, N of the result again (cycle-walking).
 * The walk follows the cycle of N that contains i; that cycle returns to i < n, so the loop ends -- a theorem, not a
 * probability: it has no bound and cannot hang.  2^b < 2 n for n > 2, so a lane applies N fewer than two times on average; the
 * lanes of a wave walk different lengths and diverge there (the longest walk seen for n <= 100 000: 14 applications, at
 * n = 4 097).
 * Refused before any device call, the message naming the field: a NULL handle or out; n < 1; n > 2^31.
 */
int dockauv_permutation(dockauv_handle h, uint64_t seed, uint64_t epoch, long long n, int64_t* out, void* hip_stream);

/*
 * The whole update of a PPO iteration -- SB3's PPO.train (train.py:64-71): n_epochs passes over the collection in shuffled
 * minibatches -- queued by ONE host call, with no host synchronisation and, after the first call, no allocation.  All pointers
 * are device pointers, float32; asynchronous on the stream.  M = n_rows, B = batch_size, J = ceil(M / B) minibatches an epoch,
 * the last one of M - (J - 1) B rows (shorter, as in SB3).
 *
 * What one call queues: one launch that starts the optimiser's control block; per epoch e one dockauv_permutation(seed,
 * first_epoch + e, M) into the optimiser's index buffer; per minibatch j, with row_index = that buffer + j B: the actor's and
 * the critic's dockauv_policy_forward_rows, the head (dockauv_ppo_head's launches on the same inputs, stats -> columns 0..7),
 * the actor's and the critic's dockauv_policy_backward into opt.actor_grads / opt.critic_grads (grad_log_std: the head), the
 * optimiser's launch and the repack of both networks (dockauv_optim_step).  Without target_kl and clip_range_vf every bit is
 * that of the same calls issued one by one.  The weights the first forward uses are the ones the policies hold at that point of
 * the stream (dockauv_policy_load, or an earlier step's repack), as for the pieces.
 *
 * clip_range_vf > 0 (needs values_old and a critic): the head's rows launch is the same kernel instantiated with the clipped
 * value loss; for row r, v_old = values_old_i read at the row index, in this float32 order, c = clip_range_vf:
 *   d = v_r - v_old;  vc = v_old + fminf(fmaxf(d, -c), c);  dv = vc - ret_i
 *   value_loss = (sum dv * dv) / B
 *   grad_v[r] = (fabsf(d) <= c) ? ((2.0f * vf_coef) * dv) / (float)B : 0.0f        (the edge included: torch.clamp's backward)
 * Everything else is dockauv_ppo_head's arithmetic; with clip_range_vf == 0 so is this.
 *
 * Adam's count lives on the device for the length of the call: the optimiser owns a control block {t, stop, step_size, rsq},
 * written by one thread and read by everyone.  The host computes (step_size, rsq) of the steps t0 + 1 .. t0 + n_epochs J in
 * double exactly as dockauv_optim_step does, t0 the count at the call; the pair of step t0 + 1 + k travels in the kernel
 * arguments of the k-th minibatch's final-sums launch (applied steps are a prefix of the minibatches, so the k-th minibatch is
 * either step t0 + 1 + k or not applied; kernel arguments are copied at the call, so two updates queued back to back on one
 * stream cannot overwrite each other's values).  That launch -- the head's final-sums kernel instantiated for this call --,
 * after writing approx_kl:
 *   stop = already stopped || (target_kl > 0 && approx_kl > 1.5f * target_kl)        (float32, the stored statistic: SB3's rule)
 *   stop:  the flag is set and stays set for the rest of the call
 *   else:  t = t + 1;  the block's (step_size, rsq) = the launch's pair
 * and the optimiser's launch -- dockauv_optim_step's kernel instantiated for this call -- takes step_size and rsq from the block
 * and, with the flag set, leaves p, m and v untouched (the repack after it then packs the same weights again).  So a minibatch
 * that trips the rule is not applied and neither is anything after it, in this epoch or a later one of the call: SB3's break in
 * front of optimizer.step() and out of the epochs.  The remaining forwards, heads and backwards still run, on the frozen
 * weights: that wasted device work is the price of having no host round trip per minibatch.
 *
 * The host's count: with target_kl == 0 the call adds n_epochs J to it.  With target_kl > 0 the count is PENDING after the call:
 * the next dockauv_optim_step, dockauv_optim_state or dockauv_ppo_update on this optimiser first synchronises the stream the
 * update ran on and reads t back (8 bytes); SB3 synchronises once per minibatch there.
 *
 * stats [n_epochs][J][12], per minibatch: columns 0..7 dockauv_ppo_head's statistics (also for the minibatches after a stop; the
 * one that tripped the rule shows the approx_kl that tripped it, as SB3 logs it); 8, 9: the gradient norm before clipping and
 * coef (dockauv_optim_step); 10: applied, 1.0f or 0.0f; 11: the Adam step number used, as a float.  Columns 8..11 are 0 where the
 * minibatch was not applied.
 *
 * The optimiser owns the index buffer (int64 [M]), the head's inputs and outputs (mean, v, grad_mean, grad_v of one minibatch)
 * and the control block: allocated by the first call and grown when a later call needs more (hipMalloc synchronises the device:
 * make the first call outside a stream capture, as for dockauv_ppo_head, whose workspace rules hold here too).  The bias
 * corrections are host scalars of the call: do not capture it (dockauv_optim_step).
 * Refused before any device call, the message naming the field: what dockauv_ppo_head refuses for normalize_advantage, rows,
 * actions, log_prob_old, advantages, returns, clip_range and the actor, and dockauv_optim_step for opt; n_rows < 1 or > 2^31;
 * batch_size < 1; n_epochs < 1; a last minibatch of one row with normalize_advantage; clip_range_vf < 0; target_kl < 0;
 * clip_range_vf > 0 with values_old NULL or without a critic; opt.stats != NULL; a NULL stats; networks whose backward does
 * not fit a group's LDS (dockauv_policy_backward).
 */
typedef struct dockauv_ppo_update_io {
    uint32_t struct_size;          /* sizeof(dockauv_ppo_update_io): ABI check */
    int32_t normalize_advantage;
    const float* rows;             /* packed rows [M][n_obs + 2]: what the actor saw */
    const float *actions, *log_prob_old, *advantages, *returns, *values_old;   /* [M][n_out], [M] ..; returns NULL without a
                                      critic; values_old nullable (clip_range_vf) */
    long long n_rows;              /* M, 1 .. 2^31 */
    long long batch_size;          /* B >= 1 */
    int32_t n_epochs;              /* >= 1 */
    int32_t reserved;
    uint64_t seed, first_epoch;    /* minibatch j of epoch e: P_{seed, first_epoch + e}[j B .. j B + B) */
    float clip_range, clip_range_vf, vf_coef, ent_coef, target_kl, reserved1;   /* clip_range > 0; clip_range_vf, target_kl: 0 = off */
    dockauv_optim_io opt;          /* params, grads (the caller's buffers, as in dockauv_optim_step), lr; stats must be NULL */
    float* stats;                  /* [n_epochs][J][12] */
} dockauv_ppo_update_io;
int dockauv_ppo_update(dockauv_handle h, dockauv_optim o, const dockauv_ppo_update_io* io, void* hip_stream);

/*
 * The episode monitor: what the reference's learner logs about a collection -- rollout/ep_rew_mean, rollout/ep_len_mean and
 * train/explained_variance through SB3 (train.py:64-71), the success and collision rates debug.py:192-194 forms from the info
 * dict's cumulative_reward, t_step, goal_reached, collision and conditions_true (docking3d.py:388-400) -- computed on the device
 * from buffers a collection already writes, by one pass over the reward and done columns AFTER the collection: the step kernels,
 * dockauv_rollout and dockauv_collect queue exactly what they queue without a monitor.  All pointers are device pointers; the
 * scan is asynchronous on the stream and does not synchronise.
 *
 * A dockauv_monitor belongs to one float32 handle with an auto-reset mode (with DOCKAUV_RESET_NONE an episode does not restart at
 * the row after a done).  It owns one running return (float32) and one running length (int32) per env -- the carries -- and its
 * reduction workspace; everything is allocated at create, later calls allocate nothing.  Destroy it before its handle.  The calls
 * on one monitor must be ordered on one stream (or by events): they share the carries and the workspace.
 *
 * Per env, forwards from k = 0, in exactly this order:
 *   ret = carry_return + reward[k]        (float32, one plain add)
 *   len = carry_length + 1                (int32)
 *   if done[k] > 0.5f:  the episode finishes with (ret, len);  carry_return = 0.0f;  carry_length = 0
 *   else:               carry_return = ret;  carry_length = len
 * This is the step kernel's own bookkeeping (cumulative reward <- cumulative reward + reward in float32, zero at an in-kernel
 * reset), so a carry that starts from the handle's DOCKAUV_F_CUM_REWARD / DOCKAUV_F_TSTEPS reproduces them bit for bit, and
 * after a scan of the rows of the steps since then the carries ARE those two fields.
 *
 * The outcome of a finished episode (needs terminal_obs, the last observation where done: dockauv_step_io.terminal_obs,
 * dockauv_rollout, dockauv_collect_io) is read off the clipped terminal observation t and the length, the lowest index winning
 * (the conditions of docking3d.py:608-619):
 *   0 goal reached     t[0] == 0.0f
 *   1 out of range     t[0] == 1.0f
 *   2 attitude limit   fabsf(t[6]) == 1.0f || fabsf(t[7]) == 1.0f
 *   3 time limit       len > max_timesteps  (is_done tests t_steps >= max_timesteps before the increment: max_timesteps + 1 steps)
 *   4 collision        done and none of the above
 * Two limits of this rule: it is a float32 test on a clipped value, so a state within one float32 rounding of a threshold can
 * classify differently from the float64 reference; and a collision that coincides with another condition is reported under the
 * lower index.  The product kernels do not deliver the true condition bits (dockauv_step_io.conditions selects the full kernel).
 *
 * Per-row outputs (each nullable), written ONLY where done -- the semantics of terminal_obs; other entries keep what they held:
 * ep_return float32, ep_length int32, ep_outcome uint8 (NULL without terminal_obs), all [n_steps][n_envs].
 *
 * stats: float64 [16] over the episodes that finished inside the scanned rows (SB3 averages over its last 100 episodes instead):
 *   0 n_episodes   1 sum of returns   2 sum of returns^2   3 sum of lengths
 *   4, 5 min, max return   6, 7 min, max length            (NaN when n_episodes == 0)
 *   8 .. 12 episodes per outcome 0 .. 4   13 episodes classified        (0 without terminal_obs)
 *   14 explained variance (NaN when values / returns are not given)      15 0 (reserved)
 * Sums 1 and 2 are float64 sums of (double)ret and (double)ret * (double)ret; the counts are exact.
 * Explained variance (what SB3 logs after PPO.train) over y = returns[n_steps * n_envs] and e = y - values[0 .. n_steps *
 * n_envs) (the subtraction in float32): a first pass forms the float64 means m_y and m_e, a second the float64 sums of
 * (y - m_y)^2 and (e - m_e)^2; ev = 1 - sum (e - m_e)^2 / sum (y - m_y)^2, NaN when the denominator is 0 (np.var gives SB3 that).
 * Reproducible: no atomics.  A lane per env in groups of 64; the lanes of a group are added by a fixed tree, the groups'
 * partials -- in the monitor's workspace -- by one final group of 1 024 lanes (lane t the groups t, t + 1 024, .. in order, then
 * the same tree, then the sixteen waves in order); the explained variance likewise on at most 256 groups of 256 lanes.  The bits
 * depend on the inputs, n_envs and n_steps only.  Launches: the scan and the final sums; with values / returns two more.
 *
 * dockauv_monitor_create: the carries start from the handle's own cum_reward / t_steps arrays (device copies).
 * dockauv_monitor_sync: re-reads the carries from the handle at this point of the stream -- after steps the monitor did not
 *   see, after dockauv_reset_envs and dockauv_set_field.
 * dockauv_monitor_carry: device pointers to the carries ([n_envs] each), owned by the monitor; either output may be NULL.
 * Refused before any device call (DOCKAUV_E_INVALID, the message naming the field): a NULL handle, monitor, io, rows_out or
 * stats; a wrong struct_size; n_steps < 1; ep_outcome without terminal_obs; exactly one of values / returns; a float64 handle; a
 * handle with DOCKAUV_RESET_NONE; a monitor of another handle.
 */
typedef struct dockauv_monitor_s* dockauv_monitor;
typedef struct dockauv_monitor_io {
    uint32_t struct_size;          /* sizeof(dockauv_monitor_io): ABI check */
    int32_t n_steps;               /* K >= 1 */
    const float* rows_out;         /* [K][n_envs][n_obs + 2]: only the reward and done columns are read */
    const float* terminal_obs;     /* nullable [K][n_envs][n_obs]: columns 0, 6 and 7 are read where done */
    const float* values;           /* nullable [K + 1][n_envs] (dockauv_collect_io.values; the first K are read) */
    const float* returns;          /* nullable [K][n_envs]; values and returns: both or neither */
    float* ep_return;              /* nullable [K][n_envs] */
    int32_t* ep_length;            /* nullable [K][n_envs] */
    uint8_t* ep_outcome;           /* nullable [K][n_envs]; must be NULL without terminal_obs */
    double* stats;                 /* [16] */
} dockauv_monitor_io;
int dockauv_monitor_create(dockauv_handle h, dockauv_monitor* out);
int dockauv_monitor_destroy(dockauv_monitor m);   /* NULL: 0 */
int dockauv_monitor_sync(dockauv_monitor m, void* hip_stream);
int dockauv_monitor_scan(dockauv_handle h, dockauv_monitor m, const dockauv_monitor_io* io, void* hip_stream);
int dockauv_monitor_carry(dockauv_monitor m, float** carry_return, int32_t** carry_length);

/*
 * Policy evaluation: the reference's predict(gym_env, model_path, n_episodes) (train.py:86-118) and SB3's evaluate_policy(model,
 * env, n_eval_episodes) on the device.  The monitor counts every episode that finishes inside a window of K steps; with
 * auto-reset an env whose episodes are short -- in this task the collisions and out-of-range failures -- finishes many in the
 * window and one whose episodes are long -- time limits, slow dockings -- few, so the window's rates are length-biased.  SB3's
 * evaluate_policy gives every env a quota, episode_count_targets[i] = (n_eval_episodes + i) / n_envs, and counts only the first
 * targets[i] episodes of env i.  This is that rule, computed from the buffers dockauv_rollout writes by a pass AFTER it: the
 * step kernels, dockauv_rollout, dockauv_collect* and the monitor queue exactly what they queue without an evaluator.  All
 * pointers are device pointers; begin, scan and state never synchronise.
 *
 * A dockauv_eval belongs to one float32 handle with an auto-reset mode.  It owns, allocated once at create for S =
 * max_episodes_per_env: per env the carries (float32 running return, int32 running length), count and target (int32); the episode
 * slots ep_return float32 [S][n_envs], ep_length int32 [S][n_envs], ep_outcome uint8 [S][n_envs] -- env i's j-th counted episode
 * is at [j][i], as the truncation slots of dockauv_truncation_scan: no compaction, no atomics --; and its reduction workspace.
 * Later calls allocate nothing.  Destroy it before its handle.  The calls on one evaluator must be ordered on one stream (or by
 * events).  Create leaves the state of a begin with target 0 (it waits for what the handle has queued and for its own launch).
 *
 * dockauv_eval_begin (two device copies and one launch):
 *   carries <- the handle's own DOCKAUV_F_CUM_REWARD / DOCKAUV_F_TSTEPS arrays at this point of the stream, as
 *     dockauv_monitor_sync: zero right after a reset, right mid-trajectory too;
 *   count <- 0;  ep_return <- 0.0f;  ep_length <- 0;  ep_outcome <- 255;
 *   target[i] <- min(max(targets[i], 0), S) -- clamped in the kernel --, or uniform_target for every env when targets is NULL; a
 *     uniform_target outside [0, S] is refused on the host.
 *
 * dockauv_eval_scan over K = n_steps steps, per env, forwards from k = 0, in exactly this order -- the monitor's arithmetic and
 * outcome rule (dockauv_monitor_scan), word for word:
 *   ret = carry_return + reward[k]        (float32, one plain add)
 *   len = carry_length + 1                (int32)
 *   if done[k] > 0.5f:  code = outcome(terminal_obs[k][env], len)     (the monitor's five codes; 255 when terminal_obs is NULL)
 *                       if count < target:  slot[count][env] = (ret, len, code);  count += 1
 *                       carry_return = 0.0f;  carry_length = 0
 *   else:               carry_return = ret;  carry_length = len
 * Episodes beyond an env's target are walked, because the carries must stay those of the handle; they are recorded nowhere.
 * Slots that no episode reached keep (0, 0, 255).
 *
 * stats: float64 [16] over ALL episodes recorded since the begin, not only this scan's, in the layout of dockauv_monitor_io.stats:
 *   0 n_episodes   1 sum of returns   2 sum of returns^2   3 sum of lengths
 *   4, 5 min, max return   6, 7 min, max length            (NaN when n_episodes == 0)
 *   8 .. 12 episodes per outcome 0 .. 4   13 episodes classified (those recorded with terminal_obs)
 *   14 NaN         15 the episodes still missing, sum over i of (target[i] - count[i]), exact
 * Sums 1 and 2 are float64 sums of (double)ret and (double)ret * (double)ret; the counts are exact.
 * Reproducible: no atomics.  After its walk a lane adds its own slots j = 0 .. count - 1 in order; the 64 lanes of a group are
 * added by the monitor's fixed tree, the groups' partials -- in the evaluator's workspace -- by one final group of 1 024 lanes
 * (lane t the groups t, t + 1 024, .. in order, then the same tree, then the sixteen waves in order), as the monitor's final
 * launch does.  The bits depend on the inputs, n_envs, S and the union of the steps scanned since the begin only: one scan of
 * 57 steps and three of 19 leave the same bits everywhere.  Launches: two a scan (the walk, the final sums).
 *
 * dockauv_eval_state: device pointers to the per-env arrays ([n_envs]) and the slots ([S][n_envs]), owned by the evaluator; each
 *   output may be NULL.
 * Refused before any device call (DOCKAUV_E_INVALID, the message naming the field): a NULL handle, evaluator, io, rows_out or
 * stats; a wrong struct_size; n_steps < 1; max_episodes_per_env < 1; slot arrays that would reach 2^31 elements; a uniform_target
 * outside [0, S]; a float64 handle; a handle with DOCKAUV_RESET_NONE; an evaluator of another handle.
 */
typedef struct dockauv_eval_s* dockauv_eval;
typedef struct dockauv_eval_io {
    uint32_t struct_size;          /* sizeof(dockauv_eval_io): ABI check */
    int32_t n_steps;               /* K >= 1 */
    const float* rows_out;         /* [K][n_envs][n_obs + 2]: only the reward and done columns are read */
    const float* terminal_obs;     /* nullable [K][n_envs][n_obs]: columns 0, 6 and 7 are read where a counted episode ends */
    double* stats;                 /* [16] */
} dockauv_eval_io;
int dockauv_eval_create(dockauv_handle h, int max_episodes_per_env, dockauv_eval* out);
int dockauv_eval_destroy(dockauv_eval e);   /* NULL: 0 */
int dockauv_eval_begin(dockauv_eval e, const int32_t* targets /* device [n_envs], nullable */, int uniform_target, void* hip_stream);
int dockauv_eval_scan(dockauv_handle h, dockauv_eval e, const dockauv_eval_io* io, void* hip_stream);
int dockauv_eval_state(dockauv_eval e, int32_t** count, int32_t** target, float** ep_return, int32_t** ep_length, uint8_t** ep_outcome,
                       float** carry_return, int32_t** carry_length);   /* each output nullable */

/*
 * Reward normalisation: SB3 1.5's VecNormalize(norm_reward=True, norm_obs=False) with its RunningMeanStd -- every reward divided
 * by the running standard deviation of the discounted return, then clipped -- computed on the device from the reward and done
 * columns of a collection.  The terminal rewards of this env are in the hundreds (config/env_config.py: w_goal 400, w_col -300)
 * on per-step terms of order one; normalised rewards put the returns on the scale vf_coef, max_grad_norm and clip_range_vf were
 * chosen for.  Observations are not normalised (the reference's are bounded in [-1, 1] by construction).  Opt-in: without these
 * calls every other call queues exactly what it queued before.  All pointers are device pointers, the workspaces belong to the
 * caller, no call but create allocates, every call but create and destroy is asynchronous on the stream.
 *
 * A dockauv_rewnorm belongs to one float32 handle.  It owns the running state, float64 [4] = (mean, var, count, reserved),
 * starting at (0, 1, 1e-4, 0), one discounted-return carry per env, float32 [n_envs], starting at 0, and the constants gamma
 * (float32, in [0, 1]), clip_reward (float32, > 0; SB3's default 10) and epsilon (float64, >= 0; SB3's default 1e-8), fixed at
 * create.  Destroy it before its handle.  The calls on one normaliser must be ordered on one stream (or by events).
 *
 * dockauv_rewnorm_scan over K = n_steps steps of N = n_envs envs, for k = 0 .. K - 1 in this order:
 *   1 per env, float32 with two roundings (a product, then a sum: never a fused multiply-add):
 *       ret = carry * gamma + reward[k];   discounted[k][env] = ret;   carry = done[k] > 0.5f ? 0.0f : ret
 *   2 the batch moments of discounted[k][0 .. N) in float64: batch_mean = sum / N, then in a second pass over the same column
 *       batch_var = (sum of (x - batch_mean)^2) / N    (each term accumulated as fma(q, q, sum), q = x - batch_mean)
 *   3 RunningMeanStd.update_from_moments with batch_count = N, every operation a float64 rounding of its own:
 *       delta = batch_mean - mean;   tot = count + N
 *       mean  = mean + (delta * N) / tot
 *       M2    = (var * count + batch_var * N) + (((delta * delta) * count) * N) / tot
 *       var   = M2 / tot;   count = tot
 *   4 den_k = sqrt(var + epsilon) in float64;
 *       reward_norm[k][env] = (float) min(max((double) reward[k][env] / den_k, -clip_reward), clip_reward)
 *     the float64 division SB3 does, stored as float32 the way its rollout buffer stores it.  Step k's reward is divided by the
 *     statistics that include step k, as VecNormalize.step_wait does.
 * training == 0 (SB3's training=False, for evaluation): only 4 runs, every k with den = sqrt(var + epsilon) of the current
 * state; carries and state are not touched, discounted is not written.
 * step_stats: float64 [K][4] = batch_mean, batch_var, var after step k, den_k; with training == 0 nullable, and only den is written.
 * discounted is a workspace the caller owns and an output; required, like step_stats, when training.
 *
 * Reproducible: no atomics.  The sums of 2 run on one group of 1 024 lanes per step: lane t adds the elements t, t + 1 024,
 * t + 2 048, .. in that order, the 64 lanes of a wave are added by a fixed tree (the monitor's), the sixteen waves in order; all
 * groups of 4 divide by the same den_k bits.  The bits depend on the inputs, n_envs and n_steps only.  Launches: four when
 * training (1, 2, 3, 4), one otherwise (4).
 *
 * dockauv_rewnorm_state: device pointers to the state [4] and the carries [n_envs], owned by the normaliser; either output may be
 *   NULL.  A checkpoint is a copy of these two arrays out and in.
 * dockauv_rewnorm_reset: state <- (0, 1, 1e-4, 0), carries <- 0; one launch.
 * dockauv_gae_normalized: dockauv_gae with the reward of step k read from reward_norm[k][env] instead of the rows' reward word
 *   (the done word still comes from the rows): one launch, the same float32 order.  With a truncation block it queues
 *   dockauv_gae_truncated's three launches -- the scan, the critic on the slots' terminal observations, the GAE, here on the
 *   column -- with rb = fmaf(gamma, v_terminal[s][env], reward_norm[k][env]): SB3's order, VecNormalize normalises inside
 *   step_wait and collect_rollouts adds the bootstrap afterwards.  critic may be NULL without a truncation block.  rows_out,
 *   values, n_steps, gamma, gae_lambda, advantages and returns must be the block's.
 * dockauv_collect_normalized: dockauv_collect's launches up to and including the value launches (with tio, in front of them,
 *   dockauv_collect_truncated's copy of the step counters into length_carry), then dockauv_rewnorm_scan, then
 *   dockauv_gae_normalized (with tio: its truncation form).  The critic is required.  nio's n_steps and rows_out must be cio's,
 *   the normaliser's gamma must be cio's, tio must agree with cio as for dockauv_collect_truncated.  The reward column of the rows,
 *   values and log-probabilities are what dockauv_collect writes: the monitor's returns stay sums of raw rewards, as SB3's Monitor
 *   inside VecNormalize sees them.
 * Refused before any device call (DOCKAUV_E_INVALID, the message naming the field): a NULL handle, normaliser, io or required
 * pointer; a wrong struct_size; n_steps < 1; gamma outside [0, 1]; clip_reward <= 0; epsilon < 0; a float64 handle; a normaliser
 * of another handle; blocks whose n_steps, rows_out or gamma disagree.
 */
typedef struct dockauv_rewnorm_s* dockauv_rewnorm;
typedef struct dockauv_rewnorm_io {
    uint32_t struct_size;          /* sizeof(dockauv_rewnorm_io): ABI check */
    int32_t n_steps;               /* K >= 1 */
    int32_t training;              /* 0: frozen statistics (evaluation) */
    int32_t reserved;
    const float* rows_out;         /* [K][n_envs][n_obs + 2]: only the reward and done columns are read */
    float* reward_norm;            /* [K][n_envs] */
    float* discounted;             /* [K][n_envs]; NULL allowed when training == 0 */
    double* step_stats;            /* [K][4]; NULL allowed when training == 0 */
} dockauv_rewnorm_io;
int dockauv_rewnorm_create(dockauv_handle h, float gamma, float clip_reward, double epsilon, dockauv_rewnorm* out);
int dockauv_rewnorm_destroy(dockauv_rewnorm rn);   /* NULL: 0 */
int dockauv_rewnorm_state(dockauv_rewnorm rn, double** state, float** carry);
int dockauv_rewnorm_reset(dockauv_rewnorm rn, void* hip_stream);
int dockauv_rewnorm_scan(dockauv_handle h, dockauv_rewnorm rn, const dockauv_rewnorm_io* io, void* hip_stream);
int dockauv_gae_normalized(dockauv_handle h, dockauv_policy critic, const float* reward_norm, const dockauv_truncation_io* tio,
                           const float* rows_out, const float* values, int n_steps, float gamma, float gae_lambda,
                           float* advantages, float* returns, void* hip_stream);
int dockauv_collect_normalized(dockauv_handle h, dockauv_policy actor, dockauv_policy critic, const dockauv_collect_io* cio,
                               const dockauv_truncation_io* tio, dockauv_rewnorm rn, const dockauv_rewnorm_io* nio,
                               void* hip_stream);

/*
 * The replay buffer: what the reference's train() needs between the env and the learner with MODEL = SAC (or DDPG; train.py
 * with SAC_HYPER_PARAMS_*, config/DRL_hyperparams.py) -- SB3 1.5's ReplayBuffer.add / ReplayBuffer.sample -- as a ring of
 * transitions (obs, action, reward, next_obs, done) in device memory, filled from the buffers a step, dockauv_rollout or
 * dockauv_collect already writes, and sampled in minibatches whose indices the kernel derives from Philox.  Opt-in: without these
 * calls every other call queues exactly what it queued before.  All pointers are device pointers; sync, push and sample are
 * asynchronous on the stream and do not synchronise.
 *
 * A dockauv_replay belongs to one float32 handle with an auto-reset mode (with DOCKAUV_RESET_NONE an episode does not restart at
 * the row after a done).  capacity_steps = max(buffer_size / n_envs, 1) step slots of n_envs records each (SB3's rule).  It owns
 * the ring, zero-filled at create, and the observation carry, float32 [n_envs][n_obs]: the observation the next transition of
 * every env starts from.  Everything is allocated at create, later calls allocate nothing.  Destroy it before its handle.  The
 * calls on one buffer must be ordered on one stream (or by events).
 *
 * Layout (public: a checkpoint is a copy of the ring and the carry out and in, with the counts).  The record of (step slot s,
 * env i) starts at float  (s * n_envs + i) * record_floats  of the ring -- a 64-bit product: the ring may exceed 4 GiB -- and is
 *   [ obs n_obs | next_obs n_obs | action n_u | reward | done | timeout | zero padding ]
 * with record_floats = 2 n_obs + n_u + 3 rounded up to a multiple of 4 (every record starts on a 16-byte boundary).  done and
 * timeout are exactly 0.0f or 1.0f, the padding is written as 0.0f: the ring's bits are a function of what was pushed.
 *
 * dockauv_replay_sync: carry[i] <- rows[i][0 .. n_obs) of rows [n_envs][n_obs + 2]: the rows the next step is about to read,
 *   after steps the buffer did not see.  One launch.
 *
 * dockauv_replay_push (one launch) stores the K = n_steps transitions of every env.  That of step k, env i:
 *   obs       k = 0: rows_in[i][0 .. n_obs), or carry[i] when rows_in is NULL;  k > 0: rows_out[k - 1][i][0 .. n_obs)
 *   action    actions[k][i]
 *   reward    rows_out[k][i][n_obs]
 *   done      rows_out[k][i][n_obs + 1] > 0.5f
 *   next_obs  terminal_obs[k][i] where done, else rows_out[k][i][0 .. n_obs)
 *   timeout   done and ep_outcome[k][i] == 3 (dockauv_monitor_scan's per-row outcome: a time limit and nothing else); 0
 *             everywhere when ep_outcome is NULL
 * terminal_obs and ep_outcome are read ONLY where done (elsewhere they hold whatever they held before).  Every value is a copy:
 * no arithmetic touches it.  The transition goes to step slot (pos + k) mod capacity_steps; afterwards
 *   carry <- rows_out[K - 1][.][0 .. n_obs);   pos <- (pos + K) mod capacity_steps;   size <- min(size + K, capacity_steps)
 * so the ring after one push of K steps is bit for bit what K pushes of one step leave.  The carry is two buffers that
 * alternate: a push reads one and writes the other, so no lane reads what another writes in the same launch;
 * dockauv_replay_state hands out the current one, which changes with every push.
 *
 * dockauv_replay_sample (one launch) draws n_batches = G minibatches of batch_size = B transitions, uniformly over what is
 * stored, with replacement, independently in step and env, as SB3 samples.  For (g, b):
 *   (x0, x1, ..) = Philox4x32-10 of counter (b, lo32(draws + g), hi32(draws + g), 4), key = seed
 *     (word 3 of the counter names the stream: 0 the episode generator, 1 the current noise, 2 the policy's normals, 3 the
 *     minibatch permutation, 4 this one)
 *   step = (x0 * size) >> 32;   env = (x1 * n_envs) >> 32;   index = step * n_envs + env
 * The multiply-shift gives every value floor(2^32 / size) or one more of the 2^32 words: a relative bias of at most size / 2^32
 * (n_envs / 2^32 for env).  obs, actions, next_obs and rewards are copies of the record's fields; dones = done * (1 - timeout),
 * exactly 0.0f or 1.0f: SB3's handle_timeout_termination.  Afterwards draws <- draws + G.  No index buffer, no workspace.
 *
 * pos, size and draws are host-side members, read when a call is made and updated by it: a captured graph would replay one
 * call's values.  dockauv_replay_counts reads them (each output nullable), dockauv_replay_set_counts writes them (a checkpoint's;
 * 0 <= pos < capacity_steps, 0 <= size <= capacity_steps).
 * dockauv_replay_state: device pointers to the ring and the current carry, capacity_steps and record_floats; each output nullable.
 *
 * Refused before any device call (DOCKAUV_E_INVALID, the message naming the field): a NULL handle, buffer, io or required
 * pointer; a wrong struct_size; buffer_size < 1; capacity_steps >= 2^31; n_steps < 1 or > capacity_steps; batch_size < 1,
 * n_batches < 1, or a product of 2^31 or more; a sample while size == 0; counts out of range; a float64 handle; a handle with
 * DOCKAUV_RESET_NONE; a buffer of another handle.
 */
typedef struct dockauv_replay_s* dockauv_replay;
typedef struct dockauv_replay_push_io {
    uint32_t struct_size;          /* sizeof(dockauv_replay_push_io): ABI check */
    int32_t n_steps;               /* K, 1 .. capacity_steps */
    const float* rows_in;          /* nullable [n_envs][n_obs + 2]: what step 0 read; NULL: the carry */
    const float* rows_out;         /* [K][n_envs][n_obs + 2] */
    const float* actions;          /* [K][n_envs][n_u] */
    const float* terminal_obs;     /* [K][n_envs][n_obs]: read where done */
    const uint8_t* ep_outcome;     /* nullable [K][n_envs] (dockauv_monitor_io.ep_outcome): read where done */
} dockauv_replay_push_io;
typedef struct dockauv_replay_sample_io {
    uint32_t struct_size;          /* sizeof(dockauv_replay_sample_io): ABI check */
    int32_t n_batches;             /* G >= 1 */
    long long batch_size;          /* B >= 1 */
    float* obs;                    /* [G][B][n_obs] */
    float* actions;                /* [G][B][n_u] */
    float* next_obs;               /* [G][B][n_obs] */
    float* rewards;                /* [G][B] */
    float* dones;                  /* [G][B] */
    long long* index;              /* nullable [G][B] */
} dockauv_replay_sample_io;
int dockauv_replay_create(dockauv_handle h, long long buffer_size, uint64_t seed, dockauv_replay* out);
int dockauv_replay_destroy(dockauv_replay rb);   /* NULL: 0 */
int dockauv_replay_sync(dockauv_handle h, dockauv_replay rb, const float* rows, void* hip_stream);
int dockauv_replay_push(dockauv_handle h, dockauv_replay rb, const dockauv_replay_push_io* io, void* hip_stream);
int dockauv_replay_sample(dockauv_handle h, dockauv_replay rb, const dockauv_replay_sample_io* io, void* hip_stream);
int dockauv_replay_counts(dockauv_replay rb, long long* pos, long long* size, uint64_t* draws);
int dockauv_replay_set_counts(dockauv_replay rb, long long pos, long long size, uint64_t draws);
int dockauv_replay_state(dockauv_replay rb, float** storage, float** carry, long long* capacity_steps, int* record_floats);

/*
 * SAC, the gradient-free half: what SB3 1.5's SAC computes under torch.no_grad() plus the actor that collect_rollouts queries
 * (train() with MODEL = SAC, SAC_HYPER_PARAMS_*) -- the squashed-Gaussian actor (sac.policies.Actor, use_sde = False), Q critics on
 * [obs | action] (ContinuousCritic) and the TD target of SAC.train -- on the tile body of the MLP actor.  Additive: calls that do
 * not use these objects queue exactly what they queued before.  Of the gradient half the library has the networks' share, every
 * matrix product (dockauv_sac_actor_forward_rows, dockauv_sac_actor_backward, dockauv_q_backward), and what lies between them:
 * the loss head (the elementwise algebra of the actor, critic and ent_coef losses: dockauv_sac_sample, dockauv_sac_critic_head,
 * dockauv_sac_actor_head) and ent_coef itself (dockauv_sac_ent_coef_step), all at the end of this file, so that one SAC gradient
 * computation needs no torch arithmetic.  What remains outside it: the optimiser for these roles and the Polyak update; torch on
 * raw parameter tensors plus dockauv_policy_load / dockauv_sac_actor_load serves until they are.  All pointers below are device
 * pointers unless a descriptor says otherwise; every call is asynchronous on the stream and synchronises nothing.
 *
 * Widths stay <= DOCKAUV_POLICY_MAX_WIDTH (128), one or two hidden layers, tanh or ReLU hidden units.  SB3's SAC default
 * net_arch = [256, 256] does NOT fit: 256 x 256 float32 weights alone exceed the 160 KiB of LDS a group keeps the network in.
 * Use policy_kwargs = dict(net_arch = [128, 128]) or narrower.
 *
 * The actor.  latent = MLP(obs); mu = W_mu latent + b_mu; log_std = clamp(W_ls latent + b_ls, -20, 2);
 *   x = mu + exp(log_std) z;  a = tanh(x);  log_prob = sum_j Normal(mu_j, std_j).log_prob(x_j) - sum_j log(1 - a_j^2 + 1e-6)
 * and deterministic means a = tanh(mu).  A dockauv_policy with a third role (after actor and critic): the same handle ownership,
 * dockauv_policy_destroy, and validation style -- every failure is DOCKAUV_E_INVALID with the field named, before any device call;
 * n_in == dockauv_n_obs, n_out == dockauv_n_u.  Both heads live in the one 32-unit output tile every actor computes (W_mu in units
 * 0 .. n_u - 1, W_ls in units 8 .. 8 + n_u - 1), so the second head costs no further matrix instruction.  Per action j, float32,
 * with mu_j and ls_j each one accumulator chain from its bias as for every other unit:
 *   ls  = fminf(fmaxf(ls_j, -20.0f), 2.0f)
 *   std = expf(ls)                                   (the expf that gives the plain actor's exp(log_std))
 *   x   = stochastic ? fmaf(std, z, mu_j) : mu_j     (z = 0 when not stochastic)
 *   a_j = tanh(x)                                    (the plain actor's output tanh: the same bits)
 *   g_j = fmaf(-0.5f * z, z, -(ls + 0.918938533f))
 *   e = expf(-2.0f * fabsf(x));  d = 1.0f + e;  c_j = logf(4.0f * e / (d * d) + 1e-6f)
 * 1 - tanh(x)^2 is formed as 4 e / (1 + e)^2, not as 1 - a * a: no cancellation where the correction matters, no overflow.
 *   log_prob = (G_lo - C_lo) + (G_hi - C_hi),  G / C the sums of g_j / c_j from 0.0f in the order of j over j = 0..3 (lo) and 4..7 (hi).
 * Consequences that tests hold bit for bit: deterministic actions are those of a plain dockauv_policy with the same hidden layers,
 * W3 = W_mu, b3 = b_mu and out_act = DOCKAUV_ACT_TANH; with W_ls = 0 and b_ls = c in [-20, 2] the stochastic actions are those of
 * that policy with log_std = c, same seed and t.
 * z: in the per-env calls the plain actor's normal, Philox counter (env_id_offset + i, t mod 2^32, j, 2); in the rows form used by
 * dockauv_sac_target a stream of its own, counter (row_offset + i, t mod 2^32, j, 5), i the position in the batch.
 *
 * Accepted by dockauv_policy_forward, dockauv_rollout (and so by the rollout that fills a replay buffer), by
 * dockauv_policy_forward_logp -- which writes the squashed log-probability above for this role; a plain policy with out_act ==
 * DOCKAUV_ACT_TANH is still refused there -- and by evaluation, which is a deterministic rollout.  Refused by name by everything
 * PPO-specific: the dockauv_collect family, dockauv_ppo_head, dockauv_ppo_update, dockauv_policy_backward, dockauv_optim_create; and
 * by dockauv_policy_load (its weights come through dockauv_sac_actor_load) and dockauv_policy_forward_rows.
 */
typedef struct dockauv_sac_actor_desc {
    uint32_t struct_size;          /* sizeof(dockauv_sac_actor_desc): ABI check */
    int32_t precision;             /* DOCKAUV_F32 */
    int32_t n_in, n_hidden[2], n_out;  /* as dockauv_policy_desc: n_in = dockauv_n_obs, n_out = dockauv_n_u */
    int32_t hidden_act;            /* DOCKAUV_ACT_TANH / _RELU (SB3's SAC default is ReLU) */
    int32_t pointers_on_device;    /* 0: host arrays; 1: device arrays, copied stream-ordered */
    int32_t reserved[2];
    const float *W1, *b1, *W2, *b2;            /* latent_pi; W2/b2 NULL with one hidden layer */
    const float *W_mu, *b_mu, *W_ls, *b_ls;    /* the two heads, [n_out][n_last] and [n_out] each (mu, log_std) */
    uint64_t seed, env_id_offset;  /* as dockauv_policy_desc */
} dockauv_sac_actor_desc;
int dockauv_sac_actor_create(dockauv_handle h, const dockauv_sac_actor_desc* d, dockauv_policy* out);
/* new weights of the same shapes and hidden activation; seed / env_id_offset are taken over */
int dockauv_sac_actor_load(dockauv_policy p, const dockauv_sac_actor_desc* d, void* hip_stream);

/*
 * Q critics (SB3's ContinuousCritic, one network per handle; SAC uses two and two targets): a dockauv_policy with a fourth role,
 * created from a dockauv_policy_desc with n_in == dockauv_n_obs + dockauv_n_u, n_out == 1 and out_act == DOCKAUV_ACT_NONE; log_std,
 * seed and env_id_offset are ignored.  dockauv_policy_load (a target network's Polyak-averaged weights, pointers_on_device = 1) and
 * dockauv_policy_destroy work on it; every other call that takes an actor or a value critic refuses it.
 *
 * dockauv_q_forward: q[i] = Q([obs row | action row]) for i < n_rows.  With r = row_index ? row_index[i] : i the layer-1 input
 * column k is obs[r * obs_stride + k] for k < n_obs and actions[r * act_stride + k - n_obs] beyond; everything behind layer 1 is
 * the actor's tile body.  Pointer, strides and index are free, so Q is evaluated straight from the replay ring without a sample
 * copy: obs = storage (or storage + n_obs for next_obs), actions = storage + 2 n_obs, both strides record_floats, row_index = the
 * index dockauv_replay_sample wrote.  A row's q depends on that row and the weights only.
 */
int dockauv_q_create(dockauv_handle h, const dockauv_policy_desc* d, dockauv_policy* out);
typedef struct dockauv_q_io {
    uint32_t struct_size;          /* sizeof(dockauv_q_io): ABI check */
    int32_t obs_stride;            /* floats between observation rows, >= n_obs */
    int32_t act_stride;            /* floats between action rows, >= n_u */
    int32_t reserved;
    const float* obs;
    const float* actions;
    const int64_t* row_index;      /* nullable [n_rows] */
    long long n_rows;              /* >= 1 */
    float* q;                      /* [n_rows] */
} dockauv_q_io;
int dockauv_q_forward(dockauv_handle h, dockauv_policy critic, const dockauv_q_io* io, void* hip_stream);

/*
 * The TD target of SAC.train in one host call:
 *   a2, logp2 = actor.sample(next_obs);   y = r + gamma (1 - d) (min(Q1', Q2')(next_obs, a2) - alpha logp2)
 * Exactly four launches: the actor's log-probability kernel on the rows (stochastic, the slot-5 normals above), the two Q kernels
 * on (next_obs rows, a2), and one row kernel.  With s = row_index ? row_index[i] : i, next_obs row i starts at next_obs +
 * s * next_obs_stride, and r, d are rewards[s * column_stride], dones[s * column_stride]; with timeouts (nullable) d <- d *
 * (1.0f - timeouts[s * column_stride]), exact for the 0.0f / 1.0f the ring holds -- SB3's handle_timeout_termination.  So the call
 * runs on dockauv_replay_sample's dense outputs (row_index NULL, next_obs_stride n_obs, column_stride 1, timeouts NULL: its dones
 * are already done * (1 - timeout)) or on the ring itself (its index; next_obs = storage + n_obs, rewards = storage + 2 n_obs + n_u,
 * dones and timeouts the two floats behind, both strides record_floats): the same bits.  alpha = log_ent_coef ?
 * expf(*log_ent_coef) : ent_coef -- a learned coefficient needs no read-back.  The last kernel, float32:
 *   v = fmaf(-alpha, logp2, fminf(q1, q2));   y = fmaf(gamma * (1.0f - d), v, r)
 * Outputs are the caller's: a2 [n_rows][n_u], logp2, q1, q2, y [n_rows] each, all required.  Fusing the four launches into one
 * kernel would need the three networks in LDS at once, which fits narrow networks only; it is not built.
 * Refused before any device call: NULL arguments, a wrong struct_size, n_rows < 1, gamma outside [0, 1], strides below the row
 * widths, an actor that is not a squashed-Gaussian actor, critics that are not Q critics, objects of another handle.
 */
typedef struct dockauv_sac_target_io {
    uint32_t struct_size;          /* sizeof(dockauv_sac_target_io): ABI check */
    int32_t next_obs_stride;       /* floats between next_obs rows, >= n_obs */
    int32_t column_stride;         /* floats between the entries of rewards / dones / timeouts, >= 1 */
    float gamma;                   /* in [0, 1] */
    float ent_coef;                /* alpha when log_ent_coef is NULL */
    int32_t reserved;
    const float* next_obs;
    const int64_t* row_index;      /* nullable [n_rows] */
    const float* rewards;
    const float* dones;
    const float* timeouts;         /* nullable */
    const float* log_ent_coef;     /* nullable device scalar */
    long long n_rows;              /* >= 1 */
    uint64_t t, row_offset;        /* the normals' counter: (row_offset + i, t mod 2^32, j, 5), key = the actor's seed */
    float *a2, *logp2, *q1, *q2, *y;
} dockauv_sac_target_io;
int dockauv_sac_target(dockauv_handle h, dockauv_policy actor, dockauv_policy q1_target, dockauv_policy q2_target,
                       const dockauv_sac_target_io* io, void* hip_stream);

/*
 * SAC, the networks' share of the gradient half: every matrix product of SAC.train's three backward passes.  The elementwise
 * algebra on [B][n_u] tensors between them (the clamp's mask, exp, tanh and the log-probability of the actor's sample; the three
 * losses) is the loss head below; what stays with the learner, until later calls exist, is the optimiser and the Polyak update.  All pointers are device pointers, float32
 * (row_index: int64); every call is asynchronous on the stream and synchronises nothing; every refusal is DOCKAUV_E_INVALID
 * with the field named, before any device call.  Each call takes its own role only and refuses the three others by name;
 * dockauv_policy_forward_rows and dockauv_policy_backward go on refusing both SAC roles.
 *
 * dockauv_sac_actor_forward_rows: with r = row_index ? row_index[i] : i and the observation row at rows + r * row_stride
 * (row_stride >= n_obs; pointer, stride and index are free, so the replay ring serves as it stands), for i < n_rows
 *   out[i][0 .. n_u) = mu,   out[i][n_u .. 2 n_u) = W_ls latent + b_ls, the log-std head BEFORE the clamp to [-20, 2]
 * without noise and without tanh: the actor's tile body with another epilogue.  Held bit for bit: the mu columns are
 * dockauv_policy_forward_rows of a plain policy with the same hidden layers and W3 = W_mu, b3 = b_mu, the log-std columns those of
 * one with W3 = W_ls, b3 = b_ls -- each unit is one accumulator chain from its bias.
 */
typedef struct dockauv_sac_rows_io {
    uint32_t struct_size;          /* sizeof(dockauv_sac_rows_io): ABI check */
    int32_t row_stride;            /* floats between observation rows, >= n_obs */
    const float* rows;
    const int64_t* row_index;      /* nullable [n_rows] */
    long long n_rows;              /* >= 1 */
    float* out;                    /* [n_rows][2 n_u] */
} dockauv_sac_rows_io;
int dockauv_sac_actor_forward_rows(dockauv_handle h, dockauv_policy actor, const dockauv_sac_rows_io* io, void* hip_stream);

/*
 * dockauv_sac_actor_backward: the contract of dockauv_policy_backward -- the sums over the rows, the activation derivatives, the
 * reproducibility (no floating-point atomics; two calls give the same bits; rows reached through row_index give the bits of the
 * same rows laid out densely in that order), the library's partial sums (allocated at the first backward of the actor, freed by
 * dockauv_policy_destroy; later calls allocate nothing), two launches -- with grad_out [n_rows][2 n_u] = dL/d(out), out as
 * dockauv_sac_actor_forward_rows defines it: columns 0 .. n_u - 1 act on mu, n_u .. 2 n_u - 1 on the raw log-std head.  The clamp's
 * mask (no gradient where the raw value lies outside [-20, 2]) belongs to the head (dockauv_sac_actor_head applies it), which has the raw values.
 * Written, torch.nn.Linear layout, overwritten: dW1 db1 [dW2 db2] of latent_pi, dW_mu db_mu, dW_ls db_ls; a head whose columns of
 * grad_out are all zero gets exact zeros.  The observation rows come through rows / row_stride / row_index as above.  LDS: the
 * kernel of dockauv_policy_backward with 16 rows of output weights and upstream gradients where that has 8: a 36-128-128 actor
 * needs 151 824 B of the 160 KiB; shapes beyond are refused with a message that names the need and the shape.
 */
typedef struct dockauv_sac_actor_backward_io {
    uint32_t struct_size;          /* sizeof(dockauv_sac_actor_backward_io): ABI check */
    int32_t row_stride;            /* floats between observation rows, >= n_obs */
    const float* rows;
    const int64_t* row_index;      /* nullable [n_rows] */
    long long n_rows;              /* >= 1 */
    const float* grad_out;         /* [n_rows][2 n_u] */
    float *dW1, *db1, *dW2, *db2;  /* dW2 / db2 NULL with one hidden layer */
    float *dW_mu, *db_mu, *dW_ls, *db_ls;
} dockauv_sac_actor_backward_io;
int dockauv_sac_actor_backward(dockauv_handle h, dockauv_policy actor, const dockauv_sac_actor_backward_io* io, void* hip_stream);

/*
 * dockauv_q_backward: a Q critic's backward for grad_q [n_rows] = dL/dq on the rows of dockauv_q_forward (obs, actions, two
 * strides, one shared nullable index).  Two outputs, each nullable, at least one required:
 *   grads         the parameter gradients, exactly what dockauv_policy_backward defines for x_r = [obs_r | a_r] (same contract,
 *                 same partial sums -- the critic's own -- and the same two launches);
 *   grad_actions  [n_rows][n_u]: grad_actions[i][j] = sum_u W1[u][n_obs + j] * delta1_u(i), dq/da of position i of the minibatch
 *                 scaled by grad_q[i], float32, overwritten; nothing behind it is written.  One accumulator chain from 0 over
 *                 the hidden units of layer 1 in order, two per step.
 * With grads == NULL -- the actor loss, where the critic's own gradients are thrown away -- the call forms no parameter tile,
 * touches no partial workspace (none is allocated by it) and queues no reduction: ONE launch.  Its grad_actions has the bits of
 * the call that also asks for parameters, which queues that same launch behind its two (SAC asks for one output at a time:
 * parameters on the replayed actions, grad_actions on the actor's).  Same reproducibility as above.  LDS as dockauv_policy_backward for n_in = n_obs + n_u:
 * 44-128-128 needs 151 792 B; shapes beyond the 160 KiB are refused with a message that names the need and the shape.
 */
typedef struct dockauv_q_backward_io {
    uint32_t struct_size;          /* sizeof(dockauv_q_backward_io): ABI check */
    int32_t obs_stride;            /* floats between observation rows, >= n_obs */
    int32_t act_stride;            /* floats between action rows, >= n_u */
    int32_t reserved;
    const float* obs;
    const float* actions;
    const int64_t* row_index;      /* nullable [n_rows] */
    long long n_rows;              /* >= 1 */
    const float* grad_q;           /* [n_rows] */
    const dockauv_policy_grads* grads;   /* nullable */
    float* grad_actions;           /* nullable [n_rows][n_u] */
} dockauv_q_backward_io;
int dockauv_q_backward(dockauv_handle h, dockauv_policy critic, const dockauv_q_backward_io* io, void* hip_stream);
/* The partial-sum workspace of a policy's backward calls and its size in floats: NULL and 0 until the first backward with
 * parameter gradients (dockauv_policy_backward, dockauv_sac_actor_backward, dockauv_q_backward with grads) allocates it.  Read-only
 * bookkeeping, no device call. */
int dockauv_policy_backward_workspace(dockauv_policy p, float** partial, long long* n_floats);

/*
 * SAC, the loss head: everything of SAC.train between the forward calls above and the backward calls above, and the learned
 * entropy coefficient.  Four calls, one launch each, no workspace, nothing allocated.  All pointers are device pointers, float32;
 * every call is asynchronous on the stream and synchronises nothing; every refusal is DOCKAUV_E_INVALID with the field named,
 * before any device call.  Reproducible: no floating-point atomics; the bits depend on the inputs, a row's position in the
 * minibatch, B and n_u only; two calls give the same bits.  The library is built with -ffp-contract=on: only the fmaf written here
 * are fused.
 *
 * Notation.  B = n_rows, n_u = dockauv_n_u.  heads [B][2 n_u] is what dockauv_sac_actor_forward_rows writes, mu | raw log-std;
 * mu_j = heads[i][j], raw_j = heads[i][n_u + j].  z_j is the rows-form normal of the actor, Philox counter (row_offset + i,
 * t mod 2^32, j, 5), key = the actor's seed: slot 5 is the stream dockauv_sac_target draws from, so the learner gives the draw of
 * the actor loss a t (or a row_offset) different from that of the target's draw of the same gradient step (the Python
 * composition sac_gradients: the target at 2 t, the actor loss at 2 t + 1).  Per action, the actor's expressions above, unchanged:
 *   ls = fminf(fmaxf(raw_j, -20.0f), 2.0f);  std = expf(ls);  x = fmaf(std, z_j, mu_j);  a_j = tanh(x)
 *   g_j = fmaf(-0.5f * z_j, z_j, -(ls + 0.918938533f))
 *   e = expf(-2.0f * fabsf(x));  d = 1.0f + e;  s_j = 4.0f * e / (d * d);  c_j = logf(s_j + 1e-6f)
 *   logp = (G_lo - C_lo) + (G_hi - C_hi)          (sums from 0.0f in the order of j, j = 0..3 and 4..7)
 * Sums over the rows: ONE group of 1 024 lanes a call; lane t adds the rows t, t + 1 024, .. in float64, the lanes of a wave are
 * added by a fixed tree, the sixteen waves in order.  A mean is such a float64 sum of float32 per-row terms divided by B and
 * rounded to float32 once.  SAC's minibatches are a few hundred to a few thousand rows, where one launch of one group costs less
 * than a second launch that adds partial sums.
 *
 * dockauv_sac_sample: a [B][n_u] and logp [B] of the expressions above, elementwise over heads.  Held bit for bit: for the same
 * actor, observation rows, t and row_offset, a and logp are the a2 and logp2 dockauv_sac_target writes for those rows.  Refused:
 * NULL arguments, a wrong struct_size, n_rows < 1, an actor that is not a squashed-Gaussian actor, an actor of another handle.
 */
typedef struct dockauv_sac_sample_io {
    uint32_t struct_size;          /* sizeof(dockauv_sac_sample_io): ABI check */
    int32_t reserved;
    const float* heads;            /* [n_rows][2 n_u] */
    long long n_rows;              /* >= 1 */
    uint64_t t, row_offset;        /* the normals' counter: (row_offset + i, t mod 2^32, j, 5), key = the actor's seed */
    float* a;                      /* [n_rows][n_u] */
    float* logp;                   /* [n_rows] */
} dockauv_sac_sample_io;
int dockauv_sac_sample(dockauv_handle h, dockauv_policy actor, const dockauv_sac_sample_io* io, void* hip_stream);

/*
 * dockauv_sac_critic_head: SB3 1.5's critic_loss = 0.5 * sum_k mse_loss(q_k, y) and its gradient on both critics' outputs.
 * q1, q2 [B]: dockauv_q_forward on the replayed actions; y [B]: dockauv_sac_target.  Per row
 *   d1 = q1_i - y_i;  d2 = q2_i - y_i;  grad_q1[i] = d1 / (float)B;  grad_q2[i] = d2 / (float)B
 * which dockauv_q_backward takes as grad_q.  stats [6]: critic_loss = 0.5f * (mse1 + mse2), mse1, mse2 (the means of d1 * d1 and
 * d2 * d2, each product in float32), mean q1, mean q2, mean y.  q1_critic must be a Q critic of the handle (it fixes the device;
 * nothing of it is read).  grad_q1, grad_q2 and stats are overwritten and must not overlap q1, q2, y or one another.
 */
typedef struct dockauv_sac_critic_head_io {
    uint32_t struct_size;          /* sizeof(dockauv_sac_critic_head_io): ABI check */
    int32_t reserved;
    const float *q1, *q2, *y;      /* [n_rows] each */
    long long n_rows;              /* >= 1 */
    float *grad_q1, *grad_q2;      /* [n_rows] each */
    float* stats;                  /* [6] */
} dockauv_sac_critic_head_io;
int dockauv_sac_critic_head(dockauv_handle h, dockauv_policy q1_critic, const dockauv_sac_critic_head_io* io, void* hip_stream);

/*
 * dockauv_sac_actor_head: SB3's actor_loss = mean(alpha logp - min(Q1, Q2)(obs, a)) and its gradient on heads, the clamp's mask
 * applied: grad_out [B][2 n_u] is what dockauv_sac_actor_backward takes.  heads, t, row_offset: the draw of dockauv_sac_sample,
 * which is formed again here (logp has the bits of that call).  q1_pi, q2_pi [B]: dockauv_q_forward at a.  dq1, dq2 [B][n_u]:
 * dockauv_q_backward with grads == NULL and grad_q a buffer of 1.0f, so pure dq/da.  alpha = log_ent_coef ? expf(*log_ent_coef) :
 * ent_coef, as in dockauv_sac_target_io.  Per row and action, in this float32 order:
 *   w_j   = (2.0f * a_j) * (s_j / (s_j + 1e-6f))                 d logp / d x_j
 *   sel_j = (q1_pi_i <= q2_pi_i) ? dq1[i][j] : dq2[i][j]         the minimum's gradient; a tie goes to critic 1
 *   gx    = fmaf(alpha, w_j, -(sel_j * s_j)) / (float)B          d loss / d x_j   (d a / d x = s_j)
 *   grad_out[i][j]       = gx
 *   inside               = raw_j >= -20.0f && raw_j <= 2.0f      torch.clamp's backward: both edges included
 *   grad_out[i][n_u + j] = inside ? fmaf(gx, std * z_j, -(alpha / (float)B)) : 0.0f
 *   loss_i = fmaf(alpha, logp_i, -fminf(q1_pi_i, q2_pi_i))
 * Under reparameterisation the Gaussian term's gradient on mu is 0 and on ls is -1: that is the -alpha / B.  stats [4]: actor_loss
 * (the mean of loss_i), mean logp, mean min q, alpha.  Refused as dockauv_sac_sample, and: a NaN ent_coef when log_ent_coef is
 * NULL; grad_out or stats overlapping an input or one another.
 */
typedef struct dockauv_sac_actor_head_io {
    uint32_t struct_size;          /* sizeof(dockauv_sac_actor_head_io): ABI check */
    float ent_coef;                /* alpha when log_ent_coef is NULL */
    const float* heads;            /* [n_rows][2 n_u] */
    const float *q1_pi, *q2_pi;    /* [n_rows] each */
    const float *dq1, *dq2;        /* [n_rows][n_u] each */
    const float* log_ent_coef;     /* nullable device scalar */
    long long n_rows;              /* >= 1 */
    uint64_t t, row_offset;        /* as dockauv_sac_sample_io */
    float* grad_out;               /* [n_rows][2 n_u] */
    float* stats;                  /* [4] */
} dockauv_sac_actor_head_io;
int dockauv_sac_actor_head(dockauv_handle h, dockauv_policy actor, const dockauv_sac_actor_head_io* io, void* hip_stream);

/*
 * dockauv_sac_ent_coef_step: the learned temperature, with no object behind it -- SB3's ent_coef_loss = -(log_ent_coef * (logp +
 * target_entropy).detach()).mean() and one step of torch.optim.Adam on the scalar.  state: the caller's device float [3] =
 * log_ent_coef, m, v; the caller sets (logf(init), 0, 0), SB3's "auto" is init = 1.  step: the caller's count, >= 1.  logp [B]:
 * dockauv_sac_sample's.  target_entropy: SB3's "auto" is -n_u.
 *   mean = (float)((float64 sum of (double)(logp_i + target_entropy)) / B)          (the add in float32)
 *   g = -mean
 *   m = fmaf(c1, g - m, m);  v = fmaf(c2 * g, g, b2 * v);  denom = fmaf(sqrtf(v), rsq, eps);  p = p - step_size * (m / denom)
 * with c1, c2, b2, step_size, rsq the host's, computed in double from step and rounded once exactly as dockauv_optim_step
 * documents, and eps = (float)eps; no clipping.  before (nullable device float) receives log_ent_coef as it was before the step:
 * SB3 uses the alpha from before the step in the target and in the actor loss, so `before` is the scalar to hand to
 * dockauv_sac_target and dockauv_sac_actor_head as log_ent_coef when the step was queued first.  stats (nullable [4]):
 * ent_coef_loss = -(p_before * mean), expf(p_before), mean, the new p.  Refused: beta1 or beta2 outside [0, 1), eps <= 0, lr < 0 or
 * not finite, step < 1, n_rows < 1, NULL state or logp, before or stats overlapping state.  The step's scalars travel in the kernel
 * arguments: as for the optimiser, do not capture the call in a stream capture.
 */
typedef struct dockauv_sac_ent_coef_io {
    uint32_t struct_size;          /* sizeof(dockauv_sac_ent_coef_io): ABI check */
    float target_entropy;
    float* state;                  /* [3]: log_ent_coef, m, v; updated in place */
    const float* logp;             /* [n_rows] */
    long long n_rows;              /* >= 1 */
    long long step;                /* >= 1 */
    double lr, beta1, beta2, eps;
    float* before;                 /* nullable: one float */
    float* stats;                  /* nullable [4] */
} dockauv_sac_ent_coef_io;
int dockauv_sac_ent_coef_step(dockauv_handle h, const dockauv_sac_ent_coef_io* io, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* DOCKAUV_H */
