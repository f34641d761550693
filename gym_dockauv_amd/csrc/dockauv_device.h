// dockauv_device.h -- parameter blocks passed BY VALUE to the step kernel (kernarg segment => scalar loads,
// wave-uniform SGPR operands) and the struct-of-arrays buffer table.  Internal to libdockauv.so.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dockauv {

constexpr int kMaxU = 8;
constexpr int kNRew = 13;
constexpr int kLoRows = 4;                       // rows of Buffers::pos_lo
constexpr int kLoState[kLoRows] = {0, 1, 2, 5};  // the state rows they belong to

// indices into VehicleP::lauv (same order as dockauv_vehicle::lauv in include/dockauv.h)
enum LauvIdx {
    L_Y_r = 0, L_Y_rr, L_Y_urf, L_Z_q, L_Z_qq, L_Z_uqf, L_M_w, L_M_ww, L_M_uw, L_N_v, L_N_vv, L_N_uv,
    L_Y_uv, L_Z_uw, L_M_uqf, L_N_urf, L_Y_uudr, L_Z_uuds, L_M_uuds, L_N_uudr, L_COUNT
};

// kernel-side vehicle kinds (template parameter VK)
enum VehKind { VK_JOY = 0, VK_DENSEB = 1, VK_LAUV = 2, VK_MIXED = 3 };

template <typename T>
struct VehicleP {
    T m;
    T gWB, gx, gy, gz;   // W-B, x_G W - x_B B, y_G W - y_B B, z_G W - z_B B   (statespace.py:353-397)
    T rg[3];
    T Ib[9];
    T ma[6];
    T dl[6], dq[6];
    T Minv[36];
    T B[6 * kMaxU];      // VK_DENSEB: dense row-major; VK_JOY: only the diagonal B[i*kMaxU+i] is read
    T ulo[kMaxU], uhalf[kMaxU];  // u = ulo + (uhi-ulo) * (clip(a)+1)/2 ; uhalf = (uhi-ulo)
    T lauv[L_COUNT];
    // structural fast path (kinetics_, SYM): coefficients of the Coriolis + added-mass polynomial, combined on the
    // host in float64.  kc = { m+ma0, m+ma1, m+ma2, m*z_G,
    //                          Iy-Iz+ma4-ma5, ma1-ma2,  Iz-Ix+ma5-ma3, ma2-ma0,  Ix-Iy+ma3-ma4, ma0-ma1 }
    T kc[10];
    int n_u;
};

template <typename T>
struct EnvP {
    int n_envs, max_timesteps, reward_set, reset_mode, scenario;
    int n_v, n_h, blk, n_vr, n_hr, n_rays, n_red, n_obs;
    int max_cap, max_sph, n_u_max;
    unsigned long long seed;
    T h, lp_alpha, mu;
    T dmax, dtol, max_att, safety;
    T vel_max[6];
    // reciprocals of configuration constants, prepared on the host in float64
    T inv_dmax, inv_log_tol, inv_log_tol_eps, inv_max_att, inv_ray_max;
    T inv_vel[6];
    T w_d, w_dth, w_dpsi, w_phi, w_th, w_thdot, w_oa;
    T w_done[5];
    T w_act[kMaxU];      // action_reward_factors[i]
    T ray_max, alpha_max, beta_max;
    // ray stage with one lane per ray (fans of <= 64 rays): lanes per env (power of two >= n_rays), the circular cone
    // that contains the fan (cos / sin of its half-angle, widened by 1e-3 rad), the sum of the obstacle-avoidance
    // weights over all rays
    // packed rows with bfloat16 observation columns (dockauv_step_io::pack_reward_done == 2): 32-bit words per row
    // (ceil(n_obs / 2) pairs + reward + done) and the multiplier that divides a word index by it (mul_hi)
    int bf16_wpr;
    unsigned bf16_magic;
    int ray_pad, ray_pad_log2;
    int device_noise;    // 1: the kernel draws the current's white noise itself (dockauv_config::device_noise)
    T fan_cos, fan_sin, sum_beta;
};

// All per-env arrays are struct-of-arrays: element (field k, env i) lives at base[k * stride + i], stride = n_envs
// rounded up to a multiple of 64 so that every row starts 256-B aligned.
struct Buffers {
    void* state;      // T [12][S]
    void* pos_lo;     // T [4][S]   low-order words of the position and of the heading (compensated accumulation, float
                      //            path: x y z psi = state[{0, 1, 2, 5}] + pos_lo[{0, 1, 2, 3}]; zero in float64)
    void* u;          // T [kMaxU][S]
    void* goal;       // T [4][S]   x y z heading
    void* cur;        // T [6][S]   V_c, dir_x, dir_y, dir_z (NED unit vector), V_min, V_max
    void* cum_reward; // T [S]
    int32_t* t_steps; // [S]
    int32_t* episode; // [S]
    uint8_t* veh_id;  // [S]
    void* cur_sigma;  // T [S]      white_noise_std of the env's current (device_noise)
    void* caps;       // T [max_cap][7][S]
    void* sph;        // T [max_sph][4][S]
    // next-episode pool (DOCKAUV_RESET_POOL)
    void* p_pose;     // T [6][S]
    void* p_goal;     // T [4][S]
    void* p_cur;      // T [6][S]
    void* p_caps;     // T [max_cap][7][S]
    void* p_sph;      // T [max_sph][4][S]
    // ray table: T [n_rays][4] = body-frame unit direction xyz, obstacle-avoidance weight beta_oa
    const void* rays;
    // fans of <= 64 rays, lane = ray: what lane l of a wave needs to know about its ray r = l % ray_pad (unit direction
    // (1, 0, 0) and weight 0 for the padding lanes r >= n_rays): T [64][4] = direction xyz, beta_oa; int32 [64] =
    // block-max cell of the ray (sensor.py:131-137)
    const void* lane_tab;
    const int32_t* lane_cell;
    // sticky status word of the handle (device memory, zero = healthy): bit 0 = a tail role of the step kernel gave up
    // waiting for its group's integrating wave (dockauv_step.hip.inc: wait_nav_).  Read by the host wherever it
    // synchronises with the stream anyway; reported as DOCKAUV_E_KERNEL.
    unsigned int* status;
    long stride;
};

struct StepIO {
    const void* actions;
    const void* noise;
    float* obs;
    void* reward;
    uint8_t* done;
    void* reward_terms;
    uint8_t* conditions;
    void* nav;
    void* ray_dist;
    float* terminal_obs;
    void* state_dot;          // T [N][12] or null
    const void* trace;        // TraceDev in device memory or null (library-owned, dockauv_trace_enable)
    long long trace_step;     // index of this step in the trace
    int pack;                 // 0: separate reward / done; 1: packed float32 rows; 2: packed rows, observation columns bfloat16
    int device_noise;         // 1: no noise array given and the handle draws the current's white noise itself
};

// ring of the last `capacity` steps of `n_rows` selected envs (include/dockauv.h: dockauv_trace_*); row-major
// [capacity][n_rows][width]
struct TraceDev {
    const int32_t* slot_of_env;   // [n_envs]: row of the env in the ring, -1 = not selected
    int n_rows, capacity;
    void* state_pre;      // T [..][12]
    void* state;          // T [..][12]
    void* state_dot;      // T [..][12]
    void* u;              // T [..][kMaxU]
    void* nu_c;           // T [..][3]
    float* obs;           // [..][n_obs]
    void* reward_terms;   // T [..][kNRew]
    uint8_t* cond;        // [..]
};

// The scalars the integrating wave of the structural (SYM) float kernels reads in front of stage 2 of the integrator,
// packed in order of first use: COPIES of the EnvP / VehicleP values (pack_hot), so that the wave can request them as one
// batch of wide scalar loads from six adjacent 64-byte lines (dockauv_step.hip.inc: fetch_hot_).
constexpr int minv_sym(int k) {   // the entries of M^-1 kinetics_ reads (SYM)
    const int idx[10] = {0, 4, 7, 9, 14, 19, 21, 24, 28, 35};
    return idx[k];
}
template <typename T>
struct alignas(64) HotP {
    // input stage: current filter, low-pass, action penalty, input range
    T lp_alpha, mu, h;
    T w_act[kMaxU];
    T ulo[kMaxU], uhalf[kMaxU];
    // kinetics
    T bdiag[6];          // B[i][i] (VK_JOY)
    T dl[6], dq[6];
    T kc[10];
    T minv[10];          // Minv[minv_sym(k)]
    T gWB, gz;
    T lauv[L_COUNT];     // (VK_LAUV)
};
static_assert(sizeof(HotP<float>) % 64 == 0 && sizeof(HotP<double>) % 64 == 0, "whole 64-byte lines");

template <typename T>
inline void pack_hot(HotP<T>& H, const EnvP<T>& E, const VehicleP<T>& V) {
    H = HotP<T>{};
    H.lp_alpha = E.lp_alpha; H.mu = E.mu; H.h = E.h;
    for (int i = 0; i < kMaxU; ++i) { H.w_act[i] = E.w_act[i]; H.ulo[i] = V.ulo[i]; H.uhalf[i] = V.uhalf[i]; }
    for (int i = 0; i < 6; ++i) { H.bdiag[i] = V.B[i * kMaxU + i]; H.dl[i] = V.dl[i]; H.dq[i] = V.dq[i]; }
    for (int i = 0; i < 10; ++i) { H.kc[i] = V.kc[i]; H.minv[i] = V.Minv[minv_sym(i)]; }
    H.gWB = V.gWB; H.gz = V.gz;
    for (int i = 0; i < L_COUNT; ++i) H.lauv[i] = V.lauv[i];
}

// The scalars the wave roles read BEHIND the integrator, packed by role: COPIES of the EnvP values (pack_tail), three adjacent
// 64-byte lines in float32, so that a role can request what it needs as one batch of wide scalar loads where it waits
// anyway (dockauv_step.hip.inc: request_tail_ / pin_tail_).  Field names are EnvP's: the kernels that keep their loads at the
// uses read the same expressions from EnvP.
template <typename T>
struct alignas(64) TailP {
    // integrating wave (whoever decides `done`): navigation errors, done conditions, its three observations
    T inv_log_tol, dtol, dmax, max_att;
    int max_timesteps;
    // ... and every role
    int reset_mode, n_obs;
    T inv_dmax;
    // record completion (every wave of a ray group): reach of the fan, safety margin, slot counts
    T ray_max, fan_cos, fan_sin, safety;
    int max_cap, max_sph;
    // pass waves (with ray_max and the slot counts in front)
    int ray_pad, ray_pad_log2, n_rays, n_red;
    T inv_ray_max, sum_beta;
    // observation / resetter wave and bookkeeper
    T inv_vel[6], inv_max_att, inv_log_tol_eps;
    T w_d, w_dth, w_dpsi, w_phi, w_th, w_thdot, w_oa;
    T w_done[5];
};
static_assert(sizeof(TailP<float>) == 192 && sizeof(TailP<double>) % 64 == 0, "whole 64-byte lines");

template <typename T>
inline void pack_tail(TailP<T>& Q, const EnvP<T>& E) {
    Q = TailP<T>{};
    Q.inv_dmax = E.inv_dmax; Q.inv_log_tol = E.inv_log_tol; Q.dtol = E.dtol; Q.dmax = E.dmax; Q.max_att = E.max_att;
    Q.max_timesteps = E.max_timesteps; Q.reset_mode = E.reset_mode; Q.n_obs = E.n_obs;
    Q.ray_max = E.ray_max; Q.fan_cos = E.fan_cos; Q.fan_sin = E.fan_sin; Q.safety = E.safety;
    Q.max_cap = E.max_cap; Q.max_sph = E.max_sph;
    Q.ray_pad = E.ray_pad; Q.ray_pad_log2 = E.ray_pad_log2; Q.n_rays = E.n_rays; Q.n_red = E.n_red;
    Q.inv_ray_max = E.inv_ray_max; Q.sum_beta = E.sum_beta;
    for (int i = 0; i < 6; ++i) Q.inv_vel[i] = E.inv_vel[i];
    Q.inv_max_att = E.inv_max_att; Q.inv_log_tol_eps = E.inv_log_tol_eps;
    Q.w_d = E.w_d; Q.w_dth = E.w_dth; Q.w_dpsi = E.w_dpsi; Q.w_phi = E.w_phi; Q.w_th = E.w_th; Q.w_thdot = E.w_thdot;
    Q.w_oa = E.w_oa;
    for (int i = 0; i < 5; ++i) Q.w_done[i] = E.w_done[i];
}

// Vehicle / reward / fan parameters (~2.5 KB in f32).  They live in a DEVICE buffer that persists across launches
// (uploaded once by dockauv_create) and are read through a constant-address-space pointer: wave-uniform scalar loads
// (s_load -> SGPR operands) that hit in L2 from the second launch on.  Passing them by value in the kernarg segment
// made every launch re-fetch 27 fresh cache lines from memory, one exposed miss per first touch (measured: a lone
// wave spent ~45 % of its life in s_waitcnt).
// Layout: E and V[] hold every parameter once and serve every kernel; H[v] repeats what the integrating wave of vehicle v
// needs in front of stage 2, line-aligned (HotP).  The rule for reading the block: ONE batch of scalar loads per wave role,
// requested where the role waits anyway (behind its row loads, in front of a barrier or a hand-over flag) and pinned
// (pin_sgpr_), never a load that is awaited where its value is used -- each of those is a scalar-cache round trip on the
// role's own instruction stream.  Q repeats what the roles read behind the integrator (TailP), appended: no older field moves.
template <typename T, int NV>
struct ParamBlock {
    EnvP<T> E;
    VehicleP<T> V[NV];
    HotP<T> H[NV];
    TailP<T> Q;
};

// copy groups riding in the launch (dockauv_ride.h); plan == nullptr: none
struct RideLaunch {
    const void* plan = nullptr;   // dockauv_p2p_plan in DEVICE memory
    const void* src = nullptr;    // previous step's rows
    uint32_t stamp = 0, wait_stamp = 0;
    int groups = 0;               // copy groups appended to the grid
};

// Resident step sequence (dockauv_step_sequence's fast path, dockauv_step.hip.inc: step_seq_kernel): the action / row
// pointers of up to kSeqMax consecutive steps travel in the kernarg segment of ONE launch.
constexpr int kSeqMax = 64;
struct SeqArgs {
    const void* actions[kSeqMax];
    float* obs[kSeqMax];
    int n;
};

// host-side bundle of everything a launch needs
template <typename T, int NV>
struct KernelArgs {
    ParamBlock<T, NV> P;      // host copy (grid / LDS sizing, and the source of the device copy)
    const void* params_dev;   // device copy of P
    Buffers B;
    StepIO io;
    RideLaunch ride;
};

// what actually travels in the kernarg segment (29 pointers + 2 ints)
struct DevArgs {
    const void* params;
    Buffers B;
    StepIO io;
    int n_envs;   // also in the parameter block; here so that the first state loads do not wait for that block
};

// LDS hand-over layout between the env phase and the ray stage
constexpr int kCapFields = 10;   // body-frame unit axis d(3), oa_perp(3), oa_par, |ba|, r^2, oa_par - |ba|
constexpr int kSphFields = 4;    // body-frame origin - centre (3), r^2
constexpr int kPoseFields = 16;  // n_cap, n_sph, position (3), body -> NED rotation (9), may-be-hit bit masks (capsules, spheres)
constexpr int kSpecFields = 19;  // pre-drawn next episode of an env: pose (6), goal (4), current rows (8), pillar-ring draw
constexpr int kNavFields = 5;    // integrating wave -> tail roles (SHARE_NAV): distance, delta_theta, delta_psi, condition bits, ready flags;
                                 // they live in spare rows of the obstacle-avoidance sums (dockauv_step.hip.inc: lds_nav)
constexpr int kHxFields = 21;    // env phase -> tail waves: state (12), V_c, action penalty, |euler_dot|^2, collision, nu_c (3), sin/cos psi

// one-wave groups whose completed capsule records stay in registers (dockauv_step.hip.inc: regrec): the 63-ray fan (one env
// per 64-lane pass) against at most kRegCaps capsules and no spheres, float32
constexpr int kRegCaps = 5;
constexpr bool solo_regrec(int max_cap, int max_sph, int ray_pad_log2) {
    return max_sph == 0 && max_cap >= 1 && max_cap <= kRegCaps && ray_pad_log2 == 6;
}

template <typename T>
inline size_t lds_bytes(int epg, int nt, int max_cap, int max_sph, int n_obs, bool rays, int ray_pad_log2 = 0) {
    if (rays && nt / epg == 1 && sizeof(T) == 4 && solo_regrec(max_cap, max_sph, ray_pad_log2)) {
        // raw capsule rows [max_cap][7][epg]; over them, once the records are complete, the tile
        const size_t raw = (size_t)epg * 7 * max_cap * sizeof(T);
        const size_t tile = (size_t)epg * (n_obs + 2) * sizeof(float);
        return ((raw > tile ? raw : tile) + 15) & ~(size_t)15;
    }
    if (rays && nt / epg == 1) {
        // one-wave ray groups (dockauv_step.hip.inc: SOLO): no pose rows (registers); the observation tile overlays the
        // obstacle records; behind the larger of the two: obstacle-avoidance sums (2 rows), the list of active envs (1 row),
        // and the ray cells [epg][n_red] the passes accumulate
        const size_t rec = (size_t)epg * (kCapFields * max_cap + kSphFields * max_sph) * sizeof(T);
        const size_t tile = (size_t)epg * (n_obs + 2) * sizeof(float);
        size_t bytes = ((rec > tile ? rec : tile) + 15) & ~(size_t)15;
        bytes = (bytes + (size_t)epg * 3 * sizeof(T) + 15) & ~(size_t)15;
        return bytes + (size_t)epg * (n_obs - 16) * sizeof(float);
    }
    size_t t_elems = rays ? (size_t)epg * (kPoseFields + kCapFields * max_cap + kSphFields * max_sph + 4 * (nt / epg)) : 0;
    if (nt / epg >= 2) t_elems += (size_t)epg * (kHxFields + kSpecFields);
    size_t bytes = t_elems * sizeof(T);
    bytes = (bytes + 15) & ~(size_t)15;
    return bytes + (size_t)epg * (n_obs + 2) * sizeof(float);   // +2: packed reward | done columns
}

// ------------------------------------------------------------------------------------------ kernel selection (host)
// Which of the compiled step_kernel / step_ride_kernel / step_seq_kernel instantiations serves a call, and the group shape
// dockauv_create picks: plain host logic on a handful of integers, written down HERE and nowhere else.  dockauv_capi.hip
// builds the request (step_request), the launchers of dockauv_step.hip.inc dispatch on the variant;
// tests/test_kernel_selection_host.py pins the table on a CPU.
constexpr int ceil_log2(int n) { int l = 0; while ((1 << l) < n) ++l; return l; }

// what a launch is asked for: the handle's constants and what the step's dockauv_step_io wants
struct StepRequest {
    bool f64, sym;        // precision; structural fast path (see kinetics_)
    int vk;               // VehKind
    bool has_rays;        // obstacles present
    int threads, n_envs, ray_pad_log2, reset_mode, reward_set;
    bool extras;          // any optional input / output other than terminal_obs, the episode-storage trace or device noise
    bool terminal_obs;
    int pack;             // StepIO::pack
    bool ride;            // copy groups ride in this launch (RideLaunch::plan)
    bool no_current;      // the handle's "no water current" property holds (no_current_after_write, below)
    int max_capsules, max_spheres;   // obstacle slots per env (dockauv_config): who has a sphere-only kernel (nocap_shape)
};

// the template arguments of the kernel that serves it (RAYS = has_rays, EPG = 64)
struct StepVariant {
    int NT;
    bool LOG, TERM, WB;
    bool ride;            // step_ride_kernel<..., NT> instead of step_kernel<..., NT, LOG, TERM, WB>
    bool unsupported;     // no such kernel: hipErrorNotSupported (select_sequence: the caller launches the steps one by one)
    bool NOCUR;           // the lean twin without the water current (step_nocur_kernel / _ride_ / _seq_; nocur_shape)
    bool NOCAP;           // on top of NOCUR: the sphere-only twin without capsule code (step_nocap_kernel / _ride_ / _seq_; nocap_shape)
};

// "This handle has no water current": V_c = V_min = V_max = 0 in every env for as long as the property holds, so the lean
// (NOCUR) kernels may leave the current out of the step altogether -- its six row loads, the V_c filter, the hand-over of V_c
// and nu_c, the V_c store, observations 13-15 (exactly +0) and the eight current rows of an episode reset.
//  * It starts true where the scenario's generator (dockauv_step.hip.inc: generate_episode_; scenarios.py) never draws a current:
//    every in-kernel reset of such a handle writes zeros into rows that hold zeros.
//  * The HOST clears it, for good, with the first write of DOCKAUV_F_CURRENT / DOCKAUV_F_POOL_CURRENT rows that are not all
//    exact (+0.0) zeros (dockauv_set_field: the only path from the host into those buffers; dockauv_reset_envs does not touch
//    them).  The speed columns decide what a step computes; the two angle columns are held to zero as well, because a reset of
//    the general kernel would overwrite them with the generator's zeros and the lean kernel leaves the rows alone.
//  * A step with a noise input, device noise or any other extra is served by the full instantiation whatever the property says.
constexpr int kCurrentCols = 5;   // host layout of a current row: V_c, V_min, V_max, alpha, beta
inline bool scenario_without_current(int scenario) {   // DOCKAUV_SCN_*: SIMPLE, CAPSULE, OBSTACLES, OBSTACLES_NOCAP, SPHERES
    return scenario == 0 || scenario == 2 || scenario == 4 || scenario == 5 || scenario == 7;
}
inline bool exact_zero(double x) { return x == 0.0 && !__builtin_signbit(x); }
// the property after the host wrote `count` rows [count][kCurrentCols] into a current buffer
inline bool no_current_after_write(bool no_current, const double* rows, long count) {
    if (!no_current) return false;   // (never comes back)
    for (long i = 0; i < count * kCurrentCols; ++i)
        if (!exact_zero(rows[i])) return false;
    return true;
}

// The product instantiations cover what a throughput rollout runs: mandatory outputs only, reward set 1, reset modes
// NONE (the caller resets) and DEVICE (in-kernel episode generation), fans of 9..16 or 33..64 rays.  Everything else --
// optional inputs / outputs, logging, reset mode POOL (host-staged next episodes), reward set 2, other fan widths -- is
// served by the full instantiation (LOG, one group shape each): with those paths behind run-time branches of one kernel,
// every BASELINE config ran 5-12 % slower.
inline bool needs_full_kernel(const StepRequest& r) {
    const bool odd_fan = r.has_rays && !(r.ray_pad_log2 == 6 || r.ray_pad_log2 == 4);
    return r.extras || r.reset_mode == 1 || r.reward_set == 2 || odd_fan;
}

// the group shapes that exist: sensor-free kernels of 256 / 128 / 64 threads, ray kernels of 512 / 256 / 64
inline int group_threads(bool has_rays, int threads) {
    if (has_rays) return threads >= 512 ? 512 : (threads >= 256 ? 256 : 64);
    return threads >= 256 ? 256 : (threads >= 128 ? 128 : 64);
}

// a launch of more than one round of resident groups (config 3: 262 144 envs 34.5 us write-through / 35.6 write-back;
// 1 048 576: 191 / 165)
inline bool many_rounds(int n_envs) { return n_envs > 262144; }

// The group shapes that have a lean (NOCUR) twin: what dockauv_create picks for BASELINE configs 2, 3 and 4 at their batch
// sizes -- BlueROV2 without sensors and with a ray fan in groups of 256 threads, the LAUV with a ray fan in groups of 512 --
// float32, structural fast path.  Each exists as the plain kernel (written through), its TERM form, the riding kernel and the
// resident sequence kernel.  Mixed batches, one-wave groups, the write-back twins, float64 and every full (LOG) kernel keep
// the general body.
inline bool nocur_shape(const StepRequest& r, int NT) {
    if (r.f64 || !r.sym) return false;
    if (r.vk == VK_JOY) return NT == 256;
    return r.vk == VK_LAUV && r.has_rays && NT == 512;
}

// The group shape that has a sphere-only (NOCAP) twin on top of its lean one: the BlueROV2's ray kernel of 256 threads for a
// handle with no capsule slot and at least one sphere slot (BASELINE config 3) -- the step carries no capsule code.  The slot
// counts are handle constants: what takes the twin away is the loss of no_current, with which the whole twin goes.
inline bool nocap_shape(const StepRequest& r, int NT) {
    return nocur_shape(r, NT) && r.vk == VK_JOY && r.has_rays && r.max_capsules == 0 && r.max_spheres >= 1;   // (nocur_shape: NT == 256)
}

inline StepVariant select_step(const StepRequest& r) {
    const bool fast = !r.f64 && r.sym;   // the float32 kernels of the structural fast path
    // product kernels that also deliver terminal observations (TERM): float32, structural fast path, packed rows, the two
    // default group shapes -- what a device-resident learner runs (TorchDocking3d.step(want_terminal_obs=True))
    const bool term_ok = fast && r.vk != VK_DENSEB;
    const bool term_product = term_ok && r.terminal_obs && r.pack && !r.ride;
    StepVariant v{256, false, false, false, false, false, false, false};
    if (needs_full_kernel(r) || (r.terminal_obs && !term_product)) {
        v.LOG = true;
        v.unsupported = r.ride;   // (the riding gather is a throughput feature)
        return v;
    }
    if (term_product) {
        v.TERM = true;
        if (r.has_rays && r.threads >= 512) v.NT = 512;
        v.NOCUR = r.no_current && nocur_shape(r, v.NT);
        v.NOCAP = v.NOCUR && nocap_shape(r, v.NT);
        return v;
    }
    // write-through stores while the launch is one round of resident groups, write-back beyond (store_global_): the
    // sensor-free kernels of one / two waves per group only ever serve batches > 65 536 (choose_threads), the ray kernel of
    // 256 threads gets a write-back twin for batches > 262 144 (float32 structural fast path).  Copy groups riding in the
    // launch (lag-1 gather sequences) exist for the write-through float32 instantiations of the structural fast path only;
    // the caller falls back to a separate gather kernel otherwise.
    v.NT = group_threads(r.has_rays, r.threads);
    v.WB = r.has_rays ? (v.NT == 256 && term_ok && many_rounds(r.n_envs) && !r.ride) : (v.NT < 256 && !(fast && r.ride));
    v.ride = r.ride && fast && !v.WB;
    v.unsupported = r.ride && !v.ride;
    v.NOCUR = r.no_current && !v.WB && nocur_shape(r, v.NT);
    v.NOCAP = v.NOCUR && nocap_shape(r, v.NT);
    return v;
}

// The resident step sequence (step_seq_kernel): what the plain float32 product kernels of the structural fast path serve,
// with packed rows; everything else is launched step by step.  Same group shape as select_step picks (`ride` is not read:
// copy groups never ride in a resident launch).  Stores: a resident launch pays the end-of-kernel write-back of dirty L2
// lines once per 64 steps, and between its steps every wave waits for its stores to be acknowledged (vmcnt(0) in front of
// the group's barrier) -- by L2 for plain stores, by memory for write-through ones.  Same-box A/B
// (profiles/r4/ab_same_box.txt): write-back stores config 2 3.61 -> 3.39 us per step, config 4 8.72 -> 8.52, but config 3
// 7.05 -> 7.39: the four-wave ray kernels stay written through.
inline StepVariant select_sequence(const StepRequest& r) {
    StepVariant v{group_threads(r.has_rays, r.threads), false, false, false, false, false, false, false};
    v.unsupported = r.f64 || !r.sym || r.vk == VK_DENSEB || needs_full_kernel(r) || r.terminal_obs || r.pack == 0;
    // (the mixed kernel -- two integrating waves writing interleaved lanes of the same lines -- did NOT reproduce the single
    // launches with write-back stores between resident steps, tests/test_gpu_reset.py: written through like config 3's)
    v.WB = !r.has_rays || v.NT == 512 || (v.NT == 256 && many_rounds(r.n_envs) && r.vk != VK_MIXED);
    // (the lean twins: the sequence kernel of each nocur_shape with the stores it has at the BASELINE batch size)
    v.NOCUR = r.no_current && !v.unsupported && nocur_shape(r, v.NT) && !(r.has_rays && v.NT == 256 && v.WB);
    v.NOCAP = v.NOCUR && nocap_shape(r, v.NT);
    return v;
}

// Threads per 64-env group (dockauv_config::threads_per_group == 0: the library's choice): the ray stage spreads over all
// waves of the group.  Heavy fans on small batches (fewer than ~2 resident waves per SIMD at 256 threads) get 8 waves per
// group; measured on MI355X: LAUV, 63 rays x 5 capsules, 32 768 envs: 27.5 -> 22.8 us; at 65 536+ envs 256 threads are
// faster.  Without obstacles extra waves per group (bookkeeper, resetter, second observation wave: the tail of the step cut
// in two or four) shorten the step while the chip has idle SIMDs; at very large batches one wave per group does the least
// total work.
// With obstacles, beyond the batch sizes at which every group is resident at once, ONE wave per group does the least total
// work and -- since round 4, when its LDS footprint was halved (dockauv_step.hip.inc: SOLO; 16 instead of 8 groups per CU for
// config 3's fan) -- keeps the most groups in flight.  Same-box measurements (profiles/r4/threads_large.txt), light
// fan (config 3, 16 beams x 8 spheres) 64 against 256 threads: 131 072 envs 18.4 / 16.7 us, 196 608: 23.0 / 26.0,
// 262 144: 27.0 / 34.3, 524 288: 50.9 / 69.3, 1 048 576: 117.9 / 175.7; heavy fan (config 4, 63 rays x 5 capsules):
// 524 288: 115.6 / 113.7, 1 048 576: 236 / 251; mixed vehicles (config 5): 256 threads at every size (229 / 251 at 1 M).
// One-wave groups of the 63-ray fan against <= 5 capsules keep their completed records in registers (float32:
// dockauv_step.hip.inc: regrec; 8 -> 16 groups per CU); 64 against 256 threads with that (profiles/r4/threads_large.txt,
// second table): config 4 163 840 envs 41.4 / 38.2 us, 196 608: 43.1 / 43.8, 262 144: 51.0 / 56.9, 393 216: 69.3 / 82.8,
// 1 048 576: 154 / 246; config 5 (mixed) 262 144: 53.6 / 50.0, 393 216: 74.5 / 73.9, 524 288: 86.3 / 94.7,
// 1 048 576: 161 / 215 (vehicle-sorted: 154 / 211).
inline int choose_threads(bool f64, int n_envs, int n_rays, int max_capsules, int max_spheres, int n_vehicles, int threads_per_group) {
    if (threads_per_group > 0) return threads_per_group;
    if (max_capsules + max_spheres == 0) return n_envs <= 65536 ? 256 : (n_envs <= 131072 ? 128 : 64);
    const bool light = (long)n_rays * (max_capsules + max_spheres) < 256;
    const bool regrec = !f64 && solo_regrec(max_capsules, max_spheres, ceil_log2(n_rays));
    if (!light && n_envs <= 32768) return 512;
    if (light) return n_envs > 163840 ? 64 : 256;
    if (regrec) return n_envs > (n_vehicles == 1 ? 196608 : 393216) ? 64 : 256;
    return (n_vehicles == 1 && n_envs > 786432) ? 64 : 256;
}

// launch one step with the kernel select_step(r) names; implemented in dockauv_kernels_f32.hip / _f64.hip.  ev0 / ev1:
// optional hipEvent_t recorded at the start / end of this very dispatch (hipExtLaunchKernelGGL).  Returns a hipError_t as int.
int launch_step_f32(const KernelArgs<float, 2>& a, const StepRequest& r, void* stream, void* ev0 = nullptr, void* ev1 = nullptr);
int launch_step_f64(const KernelArgs<double, 2>& a, const StepRequest& r, void* stream, void* ev0 = nullptr, void* ev1 = nullptr);

// n <= kSeqMax steps of the handle in ONE launch (every group walks its 64 envs through all of them) with the kernel
// select_sequence(r) names (dockauv_kernels_seq.hip); hipErrorNotSupported = the caller launches the steps one by one.
// a.io: everything but actions / obs, which come from `seq`.
int launch_sequence_f32(const KernelArgs<float, 2>& a, const StepRequest& r, const SeqArgs& seq, void* stream);

#ifdef __HIPCC__
// Philox4x32-10 (Salmon et al., SC'11): counter-based, integer only -> bit-exact against the NumPy restatement in
// oracle/philox_ref.py.  Counter slot 3 names the stream: 0 = episode generator, 1 = current noise (dockauv_step.hip.inc),
// 2 = policy exploration noise (dockauv_policy.hip), 3 = round keys of the minibatch permutation (dockauv_update.hip),
// 4 = replay minibatch indices (dockauv_replay.hip), 5 = the squashed-Gaussian actor's normals on rows (dockauv_sac.hip).
__device__ __forceinline__ void philox4x32_10_(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];   // one v_mad_u64_u32 each
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
#endif

// ------------------------------------------------------------------------------------------ MLP policy (dockauv_policy.hip)
// a = out_act(W3 act(W2 act(W1 obs + b1) + b2) + b3) on the packed rows of the step kernel, one or two hidden layers.
// The kernel works on 32-unit x 32-env tiles of v_mfma_f32_32x32x2_f32 with the units on the M side: the weights are kept
// in device memory in the order the A operand wants them ("packed", written by policy_pack_kernel from the caller's
// row-major arrays), zero-padded to whole tiles.  Offsets in floats into that buffer:
//   W1: [ks1][mt1][64]       lane l of k step s, tile m: W1[32 m + (l & 31)][2 s + (l >> 5)]
//   W2: [16 mt1][mt2][64]    lane l of k step (m1, r), tile m2: W2[32 m2 + (l & 31)][k], k = 32 m1 + (r & 3) + 8 (r >> 2) +
//                            4 (l >> 5): the unit that accumulator register r of tile m1 holds in that lane half, so that the
//                            activations of one layer are the B operand of the next as they stand
//   W3: [16 mtl][1][64]      the same over the last hidden layer (mtl tiles), units = actions
//   b1 / b2 / b3: [tiles][16][2]  the bias of the unit of (register r, lane half)
//   std: [8]                 exp(log_std[j]) (0 without log_std)
constexpr int kPolMaxWidth = 128;
constexpr int kPolThreads = 256;          // four waves, each one tile of 32 envs
constexpr size_t kPolMaxLds = 160 * 1024;
struct PolicyShape {
    int n_in, n_h1, n_h2, n_out;          // n_h2 == 0: one hidden layer
    int hidden_act, out_act;              // DOCKAUV_ACT_*
    int mt1, mt2, ks1;
    int off_w1, off_w2, off_w3, off_b1, off_b2, off_b3, off_std, total;   // total: multiple of 4
};
inline void policy_layout(PolicyShape& s) {
    s.mt1 = (s.n_h1 + 31) / 32;
    s.mt2 = (s.n_h2 + 31) / 32;
    s.ks1 = (s.n_in + 1) / 2;
    const int mtl = s.mt2 ? s.mt2 : s.mt1;
    int o = 0;
    s.off_w1 = o; o += s.ks1 * s.mt1 * 64;
    s.off_w2 = o; o += 16 * s.mt1 * s.mt2 * 64;
    s.off_w3 = o; o += 16 * mtl * 64;
    s.off_b1 = o; o += s.mt1 * 32;
    s.off_b2 = o; o += s.mt2 * 32;
    s.off_b3 = o; o += 32;
    s.off_std = o; o += 8;
    s.total = o;
}
// LDS of one group: the packed weights (what the launch requests and what create checks against kPolMaxLds)
inline size_t policy_lds_bytes(const PolicyShape& s) { return (size_t)s.total * sizeof(float); }
struct PolicyRaw {   // the caller's arrays, device pointers (row-major [out][in] = torch.nn.Linear.weight)
    const float *W1, *b1, *W2, *b2, *W3, *b3, *log_std;
};
// packed[0 .. s.total) from raw, on stream.  Returns a hipError_t as int.
int launch_policy_pack(const PolicyShape& s, const PolicyRaw& raw, float* packed, void* stream);
// actions[i][0 .. n_out) of env rows i < n (rows: [n][row_stride], only the first n_in columns are read; actions:
// [n][act_stride]); stochastic != 0 adds std[j] * N(0, 1) of Philox counter (env_id_offset + i, t, j, 2), key = seed,
// before the output activation.  log_prob (nullable, [n]) with log_std ([n_out], the raw values, device memory): the
// log-probability of the actions before the output activation, log_prob[i] = sum_j fmaf(-0.5f * z_ij, z_ij, -(log_std[j] +
// log(2 pi) / 2)) summed over j = 0..3 and j = 4..7 separately, then (first sum) + (second sum); z = 0 when not stochastic.
// Returns a hipError_t as int.
int launch_policy_forward(const PolicyShape& s, const float* packed, const float* rows, float* actions, long n, int row_stride,
                          int act_stride, unsigned long long t, int stochastic, unsigned long long seed,
                          unsigned long long env_id_offset, void* stream, float* log_prob = nullptr,
                          const float* log_std = nullptr);
// out[r][0 .. n_out) = W3 h_last + b3 (before out_act, no noise) of row rows[row_index ? row_index[r] : r], r < n: the tile
// body of launch_policy_forward with a gathered row, so the same bits.  out: [n][n_out].  Returns a hipError_t as int.
int launch_policy_forward_rows(const PolicyShape& s, const float* packed, const float* rows, const long long* row_index, long n,
                               int row_stride, float* out, void* stream);

// ------------------------------------------------------------------------------------------ SAC forward half (dockauv_sac.hip)
// The squashed-Gaussian actor keeps both heads in the output tile of the packed image: W_mu / b_mu in output units 0 .. n_u - 1,
// W_ls / b_ls in units 8 .. 8 + n_u - 1 (packed by launch_policy_pack from a [8 + n_u][n_last] array with a shape whose n_out is
// 8 + n_u; the shape the kernels get has n_out = n_u).  The std slot of the image is unused.  include/dockauv.h states the float32
// expressions of the epilogue.
struct SacActorLaunch {
    const float* rows;                    // [..][row_stride], the first n_in columns are read
    const long long* row_index;           // nullable [n]
    float* actions;                       // [n][act_stride]
    float* log_prob;                      // nullable [n]: the form with the log-probability epilogue
    long n;
    int row_stride, act_stride, stochastic;
    unsigned long long t, row_offset, seed;   // the normal of (row, j): Philox counter (row_offset + i, t mod 2^32, j, slot)
    unsigned int slot;                    // 2: the per-env calls (the plain actor's stream), 5: the rows form
};
int launch_sac_actor(const PolicyShape& s, const float* packed, const SacActorLaunch& l, void* stream);
// q[i] = Q([obs row | action row]) of a critic with n_in = n_obs + n_u: layer-1 column k < n_obs from obs[oi * obs_stride + k],
// k >= n_obs from actions[ai * act_stride + k - n_obs], oi / ai = the index's entry or i.  Returns a hipError_t as int.
struct QLaunch {
    const float *obs, *actions;
    const long long *obs_index, *act_index;   // nullable [n] each
    float* q;                             // [n]
    long n;
    int obs_stride, act_stride, n_obs;
};
int launch_q_forward(const PolicyShape& s, const float* packed, const QLaunch& l, void* stream);
// y[i] = fmaf(gamma * (1 - d), fmaf(-alpha, logp2[i], fminf(q1[i], q2[i])), r) with r / d / timeout read at
// (row_index ? row_index[i] : i) * column_stride; d <- d * (1 - timeout) when timeouts is given; alpha = log_ent_coef ?
// expf(*log_ent_coef) : ent_coef.  One launch.
struct SacTargetLaunch {
    const float *rewards, *dones, *timeouts;
    const long long* row_index;
    const float *logp2, *q1, *q2, *log_ent_coef;
    float* y;
    long n;
    int column_stride;
    float gamma, ent_coef;
};
int launch_sac_target_rows(const SacTargetLaunch& l, void* stream);

// ------------------------------------------------------------------------------------------ MLP backward (dockauv_backward.hip)
// Parameter gradients of the MLP for upstream gradients on its raw output (include/dockauv.h: dockauv_policy_backward).  A
// group of four waves walks passes of 32 rt rows.  Everything a pass touches lies in LDS as plain row-major matrices with odd
// strides, so that each is an MFMA A operand (lane = row of the matrix) and a B operand (lane = column) without bank conflicts:
//   W1 [32 mt1][ws1], W2 [32 mt2][ws2], W3 [8][ws3]   torch.nn.Linear layout, zero-padded (un-permuted from `packed` once per group)
//                                                      (W3 and G: 16 rows for the squashed-Gaussian actor's two heads, out_rows)
//   X [2 ks1][rs], G [8][rs]                           the pass's observations and upstream gradients, [column][row of the pass]
//   H1 [32 mt1][rs], H2 [32 max(mt1, mt2)][rs], D [32 mtl][rs]   activations and deltas, [unit][row]; delta 1 of two layers reuses H2
//   ACC [slots][4][1024]                               dW1 tiles a wave holds beyond its two register tiles (wide observations)
// Offsets in floats.  n_params / p_*: one partial (and the reduction's index space): W1 b1 W2 b2 W3 b3 back to back, Linear layout.
constexpr int kBwdMaxGroups = 256;        // the bounded grid: one resident group per CU
struct BackwardLayout {
    int rt, rs, kt1, ws1, ws2, ws3, acc_slots;
    int off_w1, off_w2, off_w3, off_b1, off_b2, off_x, off_g, off_h1, off_h2, off_d, off_acc, total;
    int p_w1, p_b1, p_w2, p_b2, p_w3, p_b3, n_params;
};
inline void backward_layout(const PolicyShape& s, BackwardLayout& l, int out_rows = 8) {   // out_rows: rows of W3 and G
    const int mtl = s.mt2 ? s.mt2 : s.mt1, mtmax = s.mt1 > s.mt2 ? s.mt1 : s.mt2;
    l.rt = mtmax >= 3 ? 1 : (mtmax == 2 ? 2 : 4);
    l.rs = 32 * l.rt + 1;
    l.kt1 = (s.n_in + 31) / 32;
    l.ws1 = 2 * s.ks1 + 1;
    l.ws2 = 32 * s.mt1 + 1;
    l.ws3 = 32 * mtl + 1;
    const int per_wave = (s.mt1 * l.kt1 + 3) / 4;
    l.acc_slots = per_wave > 2 ? per_wave - 2 : 0;
    int o = 0;
    l.off_w1 = o; o += 32 * s.mt1 * l.ws1;
    l.off_w2 = o; o += 32 * s.mt2 * l.ws2;
    l.off_w3 = o; o += out_rows * l.ws3;
    l.off_b1 = o; o += 32 * s.mt1;
    l.off_b2 = o; o += 32 * s.mt2;
    l.off_x = o; o += 2 * s.ks1 * l.rs;
    l.off_g = o; o += out_rows * l.rs;
    l.off_h1 = o; o += 32 * s.mt1 * l.rs;
    l.off_h2 = o; o += (s.mt2 ? 32 * mtmax : 0) * l.rs;   // (delta 1, mt1 tiles, is written here too)
    l.off_d = o; o += 32 * mtl * l.rs;
    l.off_acc = o; o += l.acc_slots * 4 * 1024;
    l.total = o;
    const int n_last = s.n_h2 ? s.n_h2 : s.n_h1;
    int p = 0;
    l.p_w1 = p; p += s.n_h1 * s.n_in;
    l.p_b1 = p; p += s.n_h1;
    l.p_w2 = p; p += s.n_h2 * s.n_h1;
    l.p_b2 = p; p += s.n_h2;
    l.p_w3 = p; p += s.n_out * n_last;
    l.p_b3 = p; p += s.n_out;
    l.n_params = p;
}
inline size_t backward_lds_bytes(const BackwardLayout& l) { return (size_t)l.total * sizeof(float); }
struct PolicyGrads {   // device pointers, Linear layout; dW2 / db2 null with one hidden layer
    float *dW1, *db1, *dW2, *db2, *dW3, *db3;
};
// grads = sum over rows r < n of the gradient for grad_out[r] ([n][n_out]) at row rows[row_index ? row_index[r] : r];
// partial: [kBwdMaxGroups][n_params] floats of workspace.  Two launches on stream: the groups' partial sums, then their sum in
// group order.  backward_lds_bytes must be <= kPolMaxLds (the caller checks).  Returns a hipError_t as int.
int launch_policy_backward(const PolicyShape& s, const float* packed, const float* rows, const long long* row_index, long n,
                           int row_stride, const float* grad_out, float* partial, const PolicyGrads& grads, void* stream);

// ------------------------------------------------------------------------------------------ SAC backward (dockauv_backward.hip)
// The same passes for SAC's networks (include/dockauv.h: dockauv_sac_actor_backward, dockauv_q_backward).  The squashed-Gaussian
// actor: W3 [16][ws3] and G [16][rs] -- W_mu / d mu in rows 0 .. n_u - 1, W_ls / d log_std in rows 8 .. 8 + n_u - 1, as the packed
// output tile holds them -- and a partial whose output block is [2 n_u][n_last] + [2 n_u], mu first (s.n_out = n_u).
inline void sac_actor_backward_layout(const PolicyShape& s, BackwardLayout& l) {
    PolicyShape both = s;
    both.n_out = 2 * s.n_out;             // (only p_b3 and n_params depend on n_out)
    backward_layout(both, l, 16);
}
struct SacActorGrads {   // device pointers, Linear layout; dW2 / db2 null with one hidden layer
    float *dW1, *db1, *dW2, *db2, *dW_mu, *db_mu, *dW_ls, *db_ls;
};
// X row i = [rows[r * row_stride + 0 .. n_obs) | actions[r * act_stride + 0 .. n_in - n_obs)], r = row_index ? row_index[i] : i
// (the actor: n_obs = n_in, actions unread).  grad_out: the actor's [n][2 n_u] on (mu | raw log_std), a critic's [n].
struct SacBackwardLaunch {
    const float *rows, *actions;
    const long long* row_index;           // nullable [n]
    const float* grad_out;
    float* grad_actions;                  // Q only, nullable: [n][n_u] = W1[:, n_obs ..]^T delta1 of row i, overwritten
    long n;
    int row_stride, act_stride, n_obs;
};
// Two launches (partials, their sum in group order into the eight arrays).  partial: [kBwdMaxGroups][n_params of
// sac_actor_backward_layout].  Returns a hipError_t as int.
int launch_sac_actor_backward(const PolicyShape& s, const float* packed, const SacBackwardLaunch& l, float* partial,
                              const SacActorGrads& grads, void* stream);
// grads != nullptr: launch_policy_backward's two launches on x = [obs | action].  grad_actions != nullptr: ONE launch of the form
// without parameter gradients -- no gradient tiles, no bias sums, partial untouched (may be null without grads) -- behind them.
// Returns a hipError_t as int.
int launch_q_backward(const PolicyShape& s, const float* packed, const SacBackwardLaunch& l, float* partial, const PolicyGrads* grads,
                      void* stream);
// out[i][0 .. n_u) = mu, out[i][n_u .. 2 n_u) = the raw log_std head of row rows[(row_index ? row_index[i] : i) * row_stride]: the
// tile body of launch_sac_actor without noise, clamp and tanh (dockauv_sac.hip).  out: [n][2 n_u].  Returns a hipError_t as int.
int launch_sac_actor_heads(const PolicyShape& s, const float* packed, const float* rows, const long long* row_index, long n,
                           int row_stride, float* out, void* stream);

// ------------------------------------------------------------------------------------------ SAC loss head (dockauv_sac_head.hip)
// What lies between SAC's forward calls and its backward calls, and the learned entropy coefficient (include/dockauv.h:
// dockauv_sac_sample, dockauv_sac_critic_head, dockauv_sac_actor_head, dockauv_sac_ent_coef_step state the arithmetic).  The sample
// is elementwise on groups of kSacSampleThreads rows; each of the three calls with sums is ONE group of kSacHeadThreads lanes
// (lane t takes the rows t, t + kSacHeadThreads, ..; float64 sums, a fixed tree in the wave, the waves in order) and needs no
// workspace.  One launch each.  Every launcher returns a hipError_t as int.
constexpr int kSacSampleThreads = 256;
constexpr int kSacHeadThreads = 1024;
struct SacSampleLaunch {
    const float* heads;                   // [n][2 n_u]: mu | raw log-std
    float *a, *logp;                      // [n][n_u], [n]
    long n;
    int n_u;
    unsigned int t_lo, row_off_lo;        // the normal of (row i, j): Philox counter (row_off_lo + i, t_lo, j, 5)
    unsigned long long seed;
};
int launch_sac_sample(const SacSampleLaunch& a, void* stream);
struct SacCriticHeadLaunch {
    const float *q1, *q2, *y;             // [n]
    float *grad_q1, *grad_q2, *stats;     // [n], [n], [6]
    long n;
};
int launch_sac_critic_head(const SacCriticHeadLaunch& a, void* stream);
struct SacActorHeadLaunch {
    const float* heads;                   // [n][2 n_u]
    const float *q1_pi, *q2_pi, *dq1, *dq2;   // [n], [n], [n][n_u], [n][n_u]
    const float* log_ent_coef;            // nullable device scalar
    float *grad_out, *stats;              // [n][2 n_u], [4]
    long n;
    int n_u;
    unsigned int t_lo, row_off_lo;
    unsigned long long seed;
    float ent_coef;
};
int launch_sac_actor_head(const SacActorHeadLaunch& a, void* stream);
struct EntCoefLaunch {
    float* state;                         // [3]: log_ent_coef, m, v
    const float* logp;                    // [n]
    float *before, *stats;                // nullable: one float, [4]
    long n;
    float target_entropy;
    float c1, c2, b2, step_size, rsq, eps;   // host scalars of this step (dockauv_optim_step's)
};
int launch_ent_coef_step(const EntCoefLaunch& a, void* stream);

// ------------------------------------------------------------------------------------------ GAE (dockauv_collect.hip)
// SB3's compute_returns_and_advantage over packed rows: rows [K][N][row_stride] with the reward in column n_obs and done in
// column n_obs + 1 (the observation columns are never read), values [K + 1][N], advantages / returns [K][N]; one lane per
// env walks k = K - 1 .. 0.  The float32 expression order is stated in include/dockauv.h (dockauv_gae).  One kernel, instantiated on
// what the two nullable parts ask for.  trunc_step (with v_terminal and n_slots; the tables of the truncation bootstrap, below): at
// step trunc_step[s][env] the reward is fmaf(gamma, v_terminal[s][env], reward); without a used slot the bits are those without the
// tables.  reward_col [K][N]: the reward is read from it instead of the rows' reward word (the done word still comes from the
// rows).
struct GaeLaunch {                        // (a call's own arguments first: the C ABI initialises those as an aggregate)
    const float* rows;                    // [K][N][n_obs + 2]
    const float* values;                  // [K + 1][N]
    float* advantages;                    // [K][N]
    float* returns;                       // [K][N]
    int n_steps;
    float gamma, gae_lambda;
    const float* reward_col;              // [K][N], nullable
    int n_envs, n_obs;
    const int32_t* trunc_step;            // [n_slots][N], nullable
    const float* v_terminal;              // [n_slots][N]
    int n_slots;
};
// One launch.  Returns a hipError_t as int.
int launch_gae(const GaeLaunch& g, void* stream);

// ------------------------------------------------------------------------------------------ truncation bootstrap (dockauv_collect.hip)
// SB3's rewards[idx] += gamma * V(terminal_observation) for the dones that are time limits (include/dockauv.h:
// dockauv_gae_truncated states the rule and the arithmetic).  The scan finds them -- one lane per env walks k = 0 .. K - 1 with an
// int32 length carry -- and leaves env's s-th truncated step in slot s of two [n_slots][n_envs] tables: trunc_step (the step, -1
// in unused slots) and trunc_row (k n_envs + env: the row of terminal_obs, what launch_policy_forward_rows takes as an index; env
// in unused slots, a row that exists).  A truncated episode has max_timesteps + 1 steps and the carry before step 0 is at most
// max_timesteps, so an env truncates at most (K - 1) / (max_timesteps + 1) + 1 times in K steps: the slots are the compaction.
inline int truncation_slots(int n_steps, int max_timesteps) { return n_steps / (max_timesteps + 1) + 1; }
struct TruncArgs {
    const float* rows;                    // [K][N][row_stride]; only the done column is read
    const float* terminal_obs;            // [K][N][n_obs]; columns 0, 6, 7 are read where a done is a time limit by its length
    int32_t* carry_len;                   // [N], read and written back
    int32_t* trunc_step;                  // [n_slots][N]
    long long* trunc_row;                 // [n_slots][N]
    int n_steps, n_envs, n_obs, row_stride, max_timesteps, n_slots;
};
// One launch.  Returns a hipError_t as int.
int launch_truncation_scan(const TruncArgs& a, void* stream);

// ------------------------------------------------------------------------------------------ PPO head (dockauv_head.hip)
// Loss terms, statistics and the gradients on the networks' raw outputs and on log_std for one minibatch (include/dockauv.h:
// dockauv_ppo_head states the arithmetic).  Groups of kHeadThreads lanes on the backward's bounded grid (kBwdMaxGroups); a lane
// has the loads of kHeadChunk rows in flight, a group takes kHeadPassRows rows a pass.  Workspace, float64, its size independent
// of n: kHeadMoments words a group from the advantage-moment launch (sum, squares about the group's centre, that centre, rows)
// and kHeadSums row sums a group (surrogate, squared value error, KL term, clipped rows, then DOCKAUV_MAX_U of d log_std).
constexpr int kHeadThreads = 256;
constexpr int kHeadChunk = 4;
constexpr int kHeadPassRows = kHeadThreads * kHeadChunk;
constexpr int kHeadMoments = 4;
constexpr int kHeadSums = 4 + 8;          // 8 = DOCKAUV_MAX_U
constexpr size_t kHeadWorkspaceBytes = (size_t)kBwdMaxGroups * (kHeadMoments + kHeadSums) * sizeof(double);
struct HeadArgs {
    static constexpr bool kClipVf = false, kGate = false;   // (what the kernels are instantiated on: dockauv_ppo_head's own)
    const float *mean, *v;                // [n][n_out]; [n] or null (no critic)
    const float *actions, *log_prob_old, *advantages, *returns;   // row arrays, read at row_index[r]
    const long long* row_index;           // nullable [n]
    const float* log_std;                 // [n_out], the actor's
    float *grad_mean, *grad_v, *grad_log_std, *stats;
    double *moments, *partial;            // [kBwdMaxGroups][kHeadMoments], [kBwdMaxGroups][kHeadSums]
    long n;
    int n_out, normalize;
    float clip, vf_coef, ent_coef;
};
// Up to three launches on stream: the advantage moments (normalize only), the rows and the groups' partial sums, their sum in
// group order.  Returns a hipError_t as int.
int launch_ppo_head(const HeadArgs& a, void* stream);

// The optimiser's control block in device memory (dockauv_ppo_update): written by ONE thread -- update_begin_kernel at the start
// of a call, then the gated final-sums kernel of every minibatch -- and read by every thread of the controlled Adam kernel.
struct OptimCtl {
    long long t;                          // Adam steps applied so far (what the host reads back when the count is pending)
    int stop, reserved;                   // sticky for the rest of the call: SB3's target_kl rule tripped
    float step_size, rsq;                 // the bias corrections of step t (the host's double arithmetic, rounded once)
};
// The head inside dockauv_ppo_update: the same kernels instantiated on these argument blocks.
struct HeadArgsVf : HeadArgs {            // rows kernel with clip_range_vf > 0
    static constexpr bool kClipVf = true;
    const float* v_old;                   // [M], read at row_index[r]
    float clip_vf;
};
struct HeadArgsGate : HeadArgs {          // final-sums kernel that decides whether the minibatch is applied
    static constexpr bool kGate = true;
    OptimCtl* ctl;
    float target_kl;                      // 0: no early stop
    float step_size, rsq;                 // of step ctl->t + 1, copied into the block when the minibatch is applied
};
struct HeadUpdate {
    const float* v_old;                   // null: clip_vf unused
    float clip_vf;                        // 0: the shipped rows kernel
    OptimCtl* ctl;
    float target_kl, step_size, rsq;
};
// launch_ppo_head with the gated final sums (stats: [12], columns 8..11 written too) and, with u.clip_vf > 0, the clipped value
// loss.  Returns a hipError_t as int.
int launch_ppo_head_update(const HeadArgs& a, const HeadUpdate& u, void* stream);

// ------------------------------------------------------------------------------------------ optimiser (dockauv_optim.hip)
// Gradient-norm clipping and one Adam step (include/dockauv.h: dockauv_optim_step states the arithmetic) over one index space
// of kOptSegments arrays back to back: actor W1 b1 W2 b2 W3 b3, log_std, critic W1 b1 W2 b2 W3 b3, torch.nn.Linear layout; a
// segment may be empty (len 0, its pointers unread).  One launch of ceil(total / kOptThreads) groups, no workspace: every group
// forms the whole norm itself (a lane has kOptChunk loads in flight), then thread i of the grid updates element i.  m, v: the
// moments, [total] in index-space order.
constexpr int kOptSegments = 13;
constexpr int kOptThreads = 1024;
constexpr int kOptChunk = 4;
struct AdamArgs {
    static constexpr bool kCtl = false;   // (what the kernel is instantiated on: dockauv_optim_step's own)
    float* p[kOptSegments];               // updated in place
    const float* g[kOptSegments];         // read only
    int len[kOptSegments];
    float *m, *v;                         // [total], updated in place
    float* stats;                         // nullable [2]: norm before clipping, coef
    int total;                            // sum of len
    float max_grad_norm;                  // <= 0: no clipping (coef = 1)
    float c1, c2, b2, step_size, rsq, eps;   // host scalars of this step (dockauv_optim_step)
};
// Returns a hipError_t as int.
int launch_adam_step(const AdamArgs& a, void* stream);
// The same kernel instantiated for dockauv_ppo_update: step_size and rsq come from the control block, not from the arguments, and
// with its stop flag set the launch leaves p, m, v and stats untouched.  Returns a hipError_t as int.
struct AdamArgsCtl : AdamArgs {
    static constexpr bool kCtl = true;
    const OptimCtl* ctl;
};
int launch_adam_step_ctl(const AdamArgs& a, const OptimCtl* ctl, void* stream);

// ------------------------------------------------------------------------------------------ whole update (dockauv_update.hip)
// out[i] = P_{seed, epoch}(i), i < n <= 2^31: the keyed bijection include/dockauv.h states (dockauv_permutation), one lane per
// output, no workspace.  Philox counter slot 3 of its round keys:
constexpr uint32_t kPermStream = 3u;
constexpr int kPermThreads = 256;
int launch_permutation(unsigned long long seed, unsigned long long epoch, long long n, long long* out, void* stream);
// ctl <- {t0, no stop}: the first launch of a dockauv_ppo_update.  Returns a hipError_t as int.
int launch_update_begin(OptimCtl* ctl, long long t0, void* stream);

// ------------------------------------------------------------------------------------------ episode monitor (dockauv_monitor.hip)
// Returns, lengths and outcomes of the episodes that end inside the packed rows of a collection, and the explained variance of
// its values (include/dockauv.h: dockauv_monitor_scan states the arithmetic).  The scan runs one lane per env in groups of
// kMonThreads and leaves kMonWords float64 words a group in `partial` ([kMonWords][monitor_groups(n_envs)]); the explained
// variance takes two passes on at most kEvMaxGroups groups with `ev_partial` ([4][kEvMaxGroups]: sums of pass one, squared sums of
// pass two); a final launch of one group adds both in a fixed order and writes stats [16].
constexpr int kMonThreads = 64;           // one wave per group, as the GAE kernel: 65 536 envs are 1 024 groups
constexpr int kMonWords = 13;
constexpr int kEvMaxGroups = 256;
inline int monitor_groups(int n_envs) { return (n_envs + kMonThreads - 1) / kMonThreads; }
inline size_t monitor_workspace_doubles(int n_envs) { return (size_t)kMonWords * (size_t)monitor_groups(n_envs) + 4 * (size_t)kEvMaxGroups; }
struct MonitorArgs {
    const float* rows;                    // [K][N][row_stride]; only the reward and done columns are read
    const float* terminal_obs;            // nullable [K][N][n_obs]; columns 0, 6, 7 are read where done
    const float *values, *returns;        // nullable, both or neither: [K + 1][N] (the first K N are read), [K][N]
    float* carry_ret;                     // [N], read and written back
    int32_t* carry_len;                   // [N]
    float* ep_return;                     // nullable [K][N], written where done
    int32_t* ep_length;                   // nullable [K][N]
    uint8_t* ep_outcome;                  // nullable [K][N]; null without terminal_obs
    double *partial, *ev_partial;         // the workspace: monitor_workspace_doubles, ev_partial behind partial
    double* stats;                        // [16]
    int n_steps, n_envs, n_obs, row_stride, max_timesteps;
};
// Two launches on stream (scan, final sums), four with values / returns.  Returns a hipError_t as int.
int launch_monitor_scan(const MonitorArgs& a, void* stream);

// ------------------------------------------------------------------------------------------ policy evaluation (dockauv_eval.hip)
// The monitor's walk with an episode quota per env (include/dockauv.h: dockauv_eval_scan states the arithmetic and the order of
// the sums): env i's j-th counted episode goes to slot [j][i] of ep_return / ep_length / ep_outcome ([n_slots][N]) while
// count[i] < target[i]; stats [16] covers every slot recorded since the begin.  The scan leaves kEvalWords float64 words a group
// in `partial` ([kEvalWords][eval_groups(n_envs)]).
constexpr int kEvalThreads = 64;          // one wave per group, as the monitor's scan
constexpr int kEvalWords = 14;            // the monitor's thirteen and the episodes still missing
inline int eval_groups(int n_envs) { return (n_envs + kEvalThreads - 1) / kEvalThreads; }
inline size_t eval_workspace_doubles(int n_envs) { return (size_t)kEvalWords * (size_t)eval_groups(n_envs); }
struct EvalArgs {
    const float* rows;                    // [K][N][row_stride]; only the reward and done columns are read
    const float* terminal_obs;            // nullable [K][N][n_obs]; columns 0, 6, 7 are read where a counted episode ends
    float* carry_ret;                     // [N], read and written back
    int32_t* carry_len;                   // [N]
    int32_t* count;                       // [N], read and written back
    const int32_t* target;                // [N], in [0, n_slots]
    float* ep_return;                     // [n_slots][N]
    int32_t* ep_length;                   // [n_slots][N]
    uint8_t* ep_outcome;                  // [n_slots][N]; 255: not classified (no terminal_obs) or not recorded
    double* partial;                      // eval_workspace_doubles
    double* stats;                        // [16]
    int n_steps, n_envs, n_obs, row_stride, max_timesteps, n_slots;
};
// count <- 0, target <- clamp(targets ? targets[env] : uniform_target, 0, n_slots), slots <- (0, 0, 255): one launch.  Needs
// n_envs * n_slots < 2^31.  Returns a hipError_t as int.
int launch_eval_begin(const int32_t* targets, int uniform_target, int32_t* count, int32_t* target, float* ep_return,
                      int32_t* ep_length, uint8_t* ep_outcome, int n_envs, int n_slots, void* stream);
// Two launches on stream (scan, final sums).  Returns a hipError_t as int.
int launch_eval_scan(const EvalArgs& a, void* stream);

// ------------------------------------------------------------------------------------------ reward normalisation (dockauv_rewnorm.hip)
// SB3's VecNormalize(norm_reward=True) on the reward column of the packed rows (include/dockauv.h: dockauv_rewnorm_scan states the
// arithmetic and the order of the sums).  state: float64 [4] = running mean, var, count, reserved; carry: float32 [N], the
// discounted return of every env before step 0; discounted / reward_norm: [K][N]; step_stats: float64 [K][4] = batch mean, batch
// variance, running variance after step k, sqrt(that + epsilon).
constexpr int kRnThreads = 64;            // the scan: one wave per group, as the monitor's
inline int rewnorm_groups(int n_envs) { return (n_envs + kRnThreads - 1) / kRnThreads; }
struct RewnormArgs {
    const float* rows;                    // [K][N][row_stride]; only the reward and done columns are read
    float* carry;                         // [N], read and written back (training)
    double* state;                        // [4], read and written back (training); read (frozen)
    float* discounted;                    // [K][N] (training)
    float* reward_norm;                   // [K][N]
    double* step_stats;                   // [K][4]; nullable when frozen, where only [k][3] is written
    int n_steps, n_envs, n_obs, row_stride, training;
    float gamma, clip_reward;
    double epsilon;
};
// Training: four launches on stream (scan, per-step moments, the K merges, apply); frozen: one (apply on the running variance).
// Returns a hipError_t as int.
int launch_rewnorm_scan(const RewnormArgs& a, void* stream);
// carry <- 0, state <- (0, 1, 1e-4, 0): one launch.  Returns a hipError_t as int.
int launch_rewnorm_reset(float* carry, double* state, int n_envs, void* stream);

#ifdef DOCKAUV_STAMPS
int read_stamps(unsigned long long* out);   // diagnostic build only
int read_span(unsigned long long* out, int groups);
#endif

}  // namespace dockauv
