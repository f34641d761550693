// dockauv_capi.hip -- C ABI of libdockauv.so (include/dockauv.h): handle, HBM buffers, field I/O, step launch.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "dockauv_capi.h"

using namespace dockauv;

namespace dockauv {

thread_local std::string g_create_error;   // dockauv_last_error(NULL)

int fail(dockauv_handle h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}

// Sticky status word of the handle's kernels.  It lives in pinned host memory that the device maps (coherent): a kernel
// that gives up a wait ORs its bit in over the bus (the failure path only), and the host reads the word with a plain load --
// wherever it has just synchronised with the stream, and in dockauv_poll_status without any synchronisation at all (what a
// device-resident rollout calls every few steps).  Non-zero = a step kernel gave up an internal wait: every result since
// is invalid; the handle stays in that state (the caller destroys it).
int check_status(dockauv_handle h) {
    if (!h->status_host) return 0;
    const unsigned int v = *h->status_host;
    if (v != 0)
        return fail(h, DOCKAUV_E_KERNEL, "step kernel status 0x%x: a tail role timed out waiting for its group's integrating wave; "
                    "results since are invalid, destroy the handle", v);
    return 0;
}

int sync_last(dockauv_handle h) {
    if (h->last_stream) HIP_TRY(h, hipStreamSynchronize(h->last_stream)); else HIP_TRY(h, hipDeviceSynchronize());
    return 0;
}

}  // namespace dockauv

namespace {

struct FieldDesc {
    void* base;   // device base of row 0
    int rows;     // device rows
    int kind;     // 0 = T, 1 = int32, 2 = uint8
};

int dalloc(dockauv_handle h, void** p, size_t bytes) {
    if (bytes == 0) bytes = 256;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return fail(h, DOCKAUV_E_HIP, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    e = hipMemset(*p, 0, bytes);
    if (e != hipSuccess) return fail(h, DOCKAUV_E_HIP, "hipMemset failed: %s", hipGetErrorString(e));
    h->allocs.push_back(*p);
    return 0;
}

template <typename T>
void fill_vehicle(VehicleP<T>& d, const dockauv_vehicle& v) {
    d.m = (T)v.m;
    d.gWB = (T)(v.W - v.BY);
    d.gx = (T)(v.r_G[0] * v.W - v.r_B[0] * v.BY);
    d.gy = (T)(v.r_G[1] * v.W - v.r_B[1] * v.BY);
    d.gz = (T)(v.r_G[2] * v.W - v.r_B[2] * v.BY);
    for (int i = 0; i < 3; ++i) d.rg[i] = (T)v.r_G[i];
    for (int i = 0; i < 9; ++i) d.Ib[i] = (T)v.I_b[i];
    for (int i = 0; i < 6; ++i) {
        d.ma[i] = (T)v.ma_diag[i];
        d.dl[i] = (T)v.d_lin[i];
        d.dq[i] = (T)v.d_quad[i];
    }
    for (int i = 0; i < 36; ++i) d.Minv[i] = (T)v.M_inv[i];
    for (int i = 0; i < 6 * kMaxU; ++i) d.B[i] = (T)v.B[i];
    for (int i = 0; i < kMaxU; ++i) {
        d.ulo[i] = (T)v.u_lo[i];
        d.uhalf[i] = (T)(v.u_hi[i] - v.u_lo[i]);
    }
    for (int i = 0; i < L_COUNT; ++i) d.lauv[i] = (T)v.lauv[i];
    {
        const double m = v.m, zg = v.r_G[2];
        const double* a = v.ma_diag;
        const double Ix = v.I_b[0], Iy = v.I_b[4], Iz = v.I_b[8];
        const double kc[10] = {m + a[0], m + a[1], m + a[2], m * zg,
                               Iy - Iz + a[4] - a[5], a[1] - a[2],
                               Iz - Ix + a[5] - a[3], a[2] - a[0],
                               Ix - Iy + a[3] - a[4], a[0] - a[1]};
        for (int i = 0; i < 10; ++i) d.kc[i] = (T)kc[i];
    }
    d.n_u = v.n_u;
}

template <typename T>
void fill_env(EnvP<T>& e, const dockauv_env_s& h) {
    const dockauv_config& c = h.cfg;
    e.n_envs = c.n_envs;
    e.max_timesteps = c.max_timesteps;
    e.reward_set = c.reward_set;
    e.reset_mode = c.reset_mode;
    e.scenario = c.scenario;
    e.n_v = c.n_v;
    e.n_h = c.n_h;
    e.blk = c.blocksize_reduce;
    e.n_vr = (c.n_v + c.blocksize_reduce - 1) / c.blocksize_reduce;
    e.n_hr = (c.n_h + c.blocksize_reduce - 1) / c.blocksize_reduce;
    e.n_rays = h.n_rays;
    e.n_red = h.n_red;
    e.n_obs = h.n_obs;
    e.max_cap = c.max_capsules;
    e.max_sph = c.max_spheres;
    e.n_u_max = h.n_u_max;
    e.bf16_wpr = (h.n_obs + 1) / 2 + 2;
    e.bf16_magic = (unsigned)((0x100000000ull / (unsigned)e.bf16_wpr) + 1ull);   // floor(idx / wpr) = mul_hi(idx, magic), idx < 2^16
    e.seed = c.seed;
    e.h = (T)c.t_step_size;
    e.lp_alpha = (T)(c.t_step_size / (c.t_step_size + c.lowpass_T1));   // utils/lowpassfilter.py:27
    e.mu = (T)c.current_mu;
    e.dmax = (T)c.max_dist_from_goal;
    e.dtol = (T)c.dist_goal_reached_tol;
    e.max_att = (T)c.max_attitude;
    e.safety = (T)c.safety_radius;
    for (int i = 0; i < 6; ++i) {
        e.vel_max[i] = (T)c.vel_max[i];
        e.inv_vel[i] = (T)(1.0 / c.vel_max[i]);
    }
    const double eps = 0.001;   // Reward.log_precision epsilon (envs/docking3d.py:722)
    e.inv_dmax = (T)(1.0 / c.max_dist_from_goal);
    e.inv_log_tol = (T)(1.0 / std::log(c.dist_goal_reached_tol / c.max_dist_from_goal));
    e.inv_log_tol_eps = (T)(1.0 / std::log(std::max(c.dist_goal_reached_tol, eps) / c.max_dist_from_goal));
    e.inv_max_att = (T)(1.0 / c.max_attitude);
    e.inv_ray_max = (T)(1.0 / c.radar_max_dist);
    e.w_d = (T)c.w_d;
    e.w_dth = (T)c.w_delta_theta;
    e.w_dpsi = (T)c.w_delta_psi;
    e.w_phi = (T)c.w_phi;
    e.w_th = (T)c.w_theta;
    e.w_thdot = (T)c.w_Thetadot;
    e.w_oa = (T)c.w_oa;
    for (int i = 0; i < 5; ++i) e.w_done[i] = (T)c.w_done[i];
    for (int i = 0; i < kMaxU; ++i) e.w_act[i] = (T)c.action_reward_factors[i];
    e.ray_max = (T)c.radar_max_dist;
    e.alpha_max = (T)c.radar_alpha_max;
    e.beta_max = (T)c.radar_beta_max;
    e.ray_pad_log2 = ceil_log2(h.n_rays);
    e.ray_pad = 1 << e.ray_pad_log2;
    e.device_noise = c.device_noise ? 1 : 0;
    e.fan_cos = (T)h.fan_cos;
    e.fan_sin = (T)h.fan_sin;
    e.sum_beta = (T)h.sum_beta;
}

// structural fast path of kinetics_: x_G = y_G = x_B = y_B = 0, diagonal I_b, M^-1 = diagonal + (0,4),(1,3) couplings
bool is_symmetric_vehicle(const dockauv_vehicle& v) {
    if (v.r_G[0] != 0.0 || v.r_G[1] != 0.0 || v.r_B[0] != 0.0 || v.r_B[1] != 0.0) return false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            if (i != j && v.I_b[i * 3 + j] != 0.0) return false;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            const bool allowed = (i == j) || (i == 0 && j == 4) || (i == 4 && j == 0) || (i == 1 && j == 3) || (i == 3 && j == 1);
            if (!allowed && std::fabs(v.M_inv[i * 6 + j]) > 1e-14 * std::fabs(v.M_inv[i * 6 + i])) return false;
        }
    return true;
}

bool b_is_diagonal(const dockauv_vehicle& v) {
    if (v.n_u != 6) return false;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < kMaxU; ++j)
            if (i != j && v.B[i * kMaxU + j] != 0.0) return false;
    return true;
}

int field_info(dockauv_handle h, int field, FieldDesc* fd, int* width) {
    const dockauv_config& c = h->cfg;
    switch (field) {
        case DOCKAUV_F_STATE: *fd = {h->B.state, 12, 0}; *width = 12; return 0;
        case DOCKAUV_F_U: *fd = {h->B.u, kMaxU, 0}; *width = kMaxU; return 0;
        case DOCKAUV_F_GOAL: *fd = {h->B.goal, 4, 0}; *width = 4; return 0;
        case DOCKAUV_F_CURRENT: *fd = {h->B.cur, 8, 0}; *width = 5; return 0;
        case DOCKAUV_F_TSTEPS: *fd = {h->B.t_steps, 1, 1}; *width = 1; return 0;
        case DOCKAUV_F_CAPSULES: *fd = {h->B.caps, c.max_capsules * 7, 0}; *width = c.max_capsules * 7; return 0;
        case DOCKAUV_F_SPHERES: *fd = {h->B.sph, c.max_spheres * 4, 0}; *width = c.max_spheres * 4; return 0;
        case DOCKAUV_F_VEHICLE_ID: *fd = {h->B.veh_id, 1, 2}; *width = 1; return 0;
        case DOCKAUV_F_CUM_REWARD: *fd = {h->B.cum_reward, 1, 0}; *width = 1; return 0;
        case DOCKAUV_F_EPISODE: *fd = {h->B.episode, 1, 1}; *width = 1; return 0;
        case DOCKAUV_F_CURRENT_SIGMA: *fd = {h->B.cur_sigma, 1, 0}; *width = 1; return 0;
        case DOCKAUV_F_POOL_POSE: *fd = {h->B.p_pose, 6, 0}; *width = 6; return 0;
        case DOCKAUV_F_POOL_GOAL: *fd = {h->B.p_goal, 4, 0}; *width = 4; return 0;
        case DOCKAUV_F_POOL_CURRENT: *fd = {h->B.p_cur, 8, 0}; *width = 5; return 0;
        case DOCKAUV_F_POOL_CAPSULES: *fd = {h->B.p_caps, c.max_capsules * 7, 0}; *width = c.max_capsules * 7; return 0;
        case DOCKAUV_F_POOL_SPHERES: *fd = {h->B.p_sph, c.max_spheres * 4, 0}; *width = c.max_spheres * 4; return 0;
    }
    return fail(h, DOCKAUV_E_INVALID, "unknown field id %d", field);
}

bool is_current_field(int field) { return field == DOCKAUV_F_CURRENT || field == DOCKAUV_F_POOL_CURRENT; }

size_t elem_size(dockauv_handle h, int kind) { return kind == 0 ? h->tsz : (kind == 1 ? 4 : 1); }

void store_elem(dockauv_handle h, int kind, void* dst, size_t idx, double v) {
    if (kind == 0) {
        if (h->f64) static_cast<double*>(dst)[idx] = v; else static_cast<float*>(dst)[idx] = (float)v;
    } else if (kind == 1) {
        static_cast<int32_t*>(dst)[idx] = (int32_t)llround(v);
    } else {
        static_cast<uint8_t*>(dst)[idx] = (uint8_t)llround(v);
    }
}

double load_elem(dockauv_handle h, int kind, const void* src, size_t idx) {
    if (kind == 0) return h->f64 ? static_cast<const double*>(src)[idx] : (double)static_cast<const float*>(src)[idx];
    if (kind == 1) return (double)static_cast<const int32_t*>(src)[idx];
    return (double)static_cast<const uint8_t*>(src)[idx];
}

void set_io(StepIO& d, const dockauv_step_io& s) {
    d.actions = s.actions;
    d.noise = s.noise;
    d.obs = s.obs;
    d.reward = s.reward;
    d.done = s.done;
    d.reward_terms = s.reward_terms;
    d.conditions = s.conditions;
    d.nav = s.nav;
    d.ray_dist = s.ray_dist;
    d.terminal_obs = s.terminal_obs;
    d.state_dot = s.state_dot;
    d.pack = s.pack_reward_done == 2 ? 2 : (s.pack_reward_done ? 1 : 0);
}

// dockauv_create behind its validation: fills the fresh handle `h` and allocates everything it owns.  A failure is reported
// through fail(h, ...); the caller destroys the handle.
int init_handle(dockauv_handle h, const dockauv_config& c, int device) {
    h->cfg = c;
    h->cfg.ray_table = nullptr;
    h->device = device;
    h->f64 = c.precision == DOCKAUV_F64;
    h->tsz = h->f64 ? 8 : 4;
    h->S = ((long)c.n_envs + 63) / 64 * 64;
    h->n_rays = c.n_v * c.n_h;
    {
        // circular cone around the body x axis that contains every ray of the fan, widened by 1e-3 rad (used to skip
        // obstacles no ray can reach), and the sum of the obstacle-avoidance weights
        double min_bx = 1.0, sb = 0.0;
        for (int r = 0; r < h->n_rays; ++r) {
            const double* q = c.ray_table + (size_t)r * 4;
            const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
            min_bx = std::min(min_bx, q[0] / n);
            sb += q[3];
        }
        const double half = std::min(std::acos(std::max(-1.0, std::min(1.0, min_bx))) + 1e-3, 3.14159265358979);
        h->fan_cos = std::cos(half);
        h->fan_sin = std::sin(half);
        h->sum_beta = sb;
    }
    const int blk = c.blocksize_reduce;
    h->n_red = ((c.n_v + blk - 1) / blk) * ((c.n_h + blk - 1) / blk);
    h->n_obs = DOCKAUV_N_OBS_BASE + h->n_red;
    h->n_u_max = c.vehicle[0].n_u;
    if (c.n_vehicles == 2 && c.vehicle[1].n_u > h->n_u_max) h->n_u_max = c.vehicle[1].n_u;
    h->has_rays = (c.max_capsules + c.max_spheres) > 0;
    h->threads = choose_threads(h->f64, c.n_envs, h->n_rays, c.max_capsules, c.max_spheres, c.n_vehicles, c.threads_per_group);
    h->no_current = scenario_without_current(c.scenario);   // (the current rows start as zeros: dalloc)
    if (c.n_vehicles == 2) {
        if (!(c.vehicle[0].kind == DOCKAUV_VEH_CONSTB && b_is_diagonal(c.vehicle[0]) && c.vehicle[1].kind == DOCKAUV_VEH_LAUV))
            return fail(h, DOCKAUV_E_INVALID, "mixed batches support vehicle[0] = diagonal-B (BlueROV2 joystick), vehicle[1] = LAUV");
        h->vk = VK_MIXED;
    } else if (c.vehicle[0].kind == DOCKAUV_VEH_LAUV) {
        h->vk = VK_LAUV;
    } else {
        h->vk = b_is_diagonal(c.vehicle[0]) ? VK_JOY : VK_DENSEB;
    }

    h->sym = true;
    for (int v = 0; v < c.n_vehicles; ++v) h->sym = h->sym && is_symmetric_vehicle(c.vehicle[v]);
    if (c.envs_per_group == -1) h->sym = false;   // test hook: force the general expressions

    const size_t S = (size_t)h->S, t = h->tsz, N = (size_t)c.n_envs;
    const size_t caps = (size_t)c.max_capsules * 7 * S * t, sph = (size_t)c.max_spheres * 4 * S * t;
    Buffers& B = h->B;
    B.stride = h->S;
    void *rays_dev = nullptr, *lt_dev = nullptr, *lc_dev = nullptr, *pdev = nullptr;   // (lane table: Buffers::lane_tab)
    const size_t pbytes = h->f64 ? sizeof(h->a64.P) : sizeof(h->a32.P);
    // host-pointer staging: the sizes of the arrays of dockauv_step_io
    const size_t stage_bytes[ST_COUNT] = {N * h->n_u_max * t, N * t, N * h->n_obs * 4, N * t, N, N * kNRew * t, N, N * 4 * t,
                                          N * h->n_rays * t, N * h->n_obs * 4, N * 12 * t};
    for (int k = 0; k < ST_COUNT; ++k) h->stage[k].bytes = stage_bytes[k];
    const struct { void** p; size_t bytes; } device_arrays[] = {
        {&B.state, 12 * S * t}, {&B.pos_lo, kLoRows * S * t}, {&B.u, kMaxU * S * t}, {&B.goal, 4 * S * t}, {&B.cur, 8 * S * t},
        {&B.cum_reward, S * t}, {(void**)&B.t_steps, S * 4}, {(void**)&B.episode, S * 4}, {(void**)&B.veh_id, S},
        {&B.cur_sigma, S * t}, {&B.caps, caps}, {&B.sph, sph}, {&B.p_pose, 6 * S * t}, {&B.p_goal, 4 * S * t},
        {&B.p_cur, 8 * S * t}, {&B.p_caps, caps}, {&B.p_sph, sph}, {&rays_dev, (size_t)h->n_rays * 4 * t},
        {&lt_dev, (size_t)64 * 4 * t}, {&lc_dev, (size_t)64 * 4}, {&pdev, pbytes}};
    for (const auto& d : device_arrays)
        if (int rc = dalloc(h, d.p, d.bytes)) return rc;
    for (auto& st : h->stage)
        if (int rc = dalloc(h, &st.dev, st.bytes)) return rc;
    hipError_t e;
    {
        std::vector<unsigned char> tmp((size_t)h->n_rays * 4 * t);
        for (int i = 0; i < h->n_rays * 4; ++i) store_elem(h, 0, tmp.data(), i, c.ray_table[i]);
        e = hipMemcpy(rays_dev, tmp.data(), tmp.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(h, DOCKAUV_E_HIP, "ray table upload: %s", hipGetErrorString(e));
    }
    B.rays = rays_dev;
    if (h->n_rays <= 64) {
        // lane table of the lane = ray stage (dockauv_device.h: Buffers::lane_tab)
        const int pad = 1 << ceil_log2(h->n_rays);
        const int n_hr = (c.n_h + blk - 1) / blk;
        std::vector<unsigned char> tmp((size_t)64 * 4 * t);
        int32_t cells[64];
        for (int l = 0; l < 64; ++l) {
            const int r = l % pad;
            const bool ok = r < h->n_rays;
            const double dir[4] = {ok ? c.ray_table[r * 4 + 0] : 1.0, ok ? c.ray_table[r * 4 + 1] : 0.0,
                                   ok ? c.ray_table[r * 4 + 2] : 0.0, ok ? c.ray_table[r * 4 + 3] : 0.0};
            for (int k = 0; k < 4; ++k) store_elem(h, 0, tmp.data(), (size_t)l * 4 + k, dir[k]);
            const int iv = ok ? r / c.n_h : 0, ih = ok ? r % c.n_h : 0;
            cells[l] = (iv / blk) * n_hr + ih / blk;
        }
        e = hipMemcpy(lt_dev, tmp.data(), tmp.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(lc_dev, cells, sizeof cells, hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(h, DOCKAUV_E_HIP, "lane table upload: %s", hipGetErrorString(e));
    }
    B.lane_tab = lt_dev;
    B.lane_cell = static_cast<const int32_t*>(lc_dev);
    {
        // sticky status word (dockauv_device.h: Buffers::status): host-coherent, mapped (see check_status)
        void* st_host = nullptr;
        void* st_dev = nullptr;
        e = hipHostMalloc(&st_host, 256, hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) {
            memset(st_host, 0, 256);
            h->pinned_allocs.push_back(st_host);
            e = hipHostGetDevicePointer(&st_dev, st_host, 0);
        }
        if (e != hipSuccess) return fail(h, DOCKAUV_E_HIP, "status word (mapped host memory): %s", hipGetErrorString(e));
        h->status_host = static_cast<volatile unsigned int*>(st_host);
        B.status = static_cast<unsigned int*>(st_dev);
    }
    if (h->f64) {
        fill_env(h->a64.P.E, *h);
        for (int v = 0; v < c.n_vehicles; ++v) {
            fill_vehicle(h->a64.P.V[v], c.vehicle[v]);
            pack_hot(h->a64.P.H[v], h->a64.P.E, h->a64.P.V[v]);
        }
        pack_tail(h->a64.P.Q, h->a64.P.E);
        h->a64.B = B;
    } else {
        fill_env(h->a32.P.E, *h);
        for (int v = 0; v < c.n_vehicles; ++v) {
            fill_vehicle(h->a32.P.V[v], c.vehicle[v]);
            pack_hot(h->a32.P.H[v], h->a32.P.E, h->a32.P.V[v]);
        }
        pack_tail(h->a32.P.Q, h->a32.P.E);
        h->a32.B = B;
    }
    // the parameter block is read by the kernel from device memory (dockauv_device.h: ParamBlock)
    e = hipMemcpy(pdev, h->f64 ? (const void*)&h->a64.P : (const void*)&h->a32.P, pbytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(h, DOCKAUV_E_HIP, "parameter block upload: %s", hipGetErrorString(e));
    h->a32.params_dev = h->a64.params_dev = pdev;
    // the dynamic-LDS request must fit the 160 KiB of a gfx950 CU
    const size_t lds = h->f64 ? lds_bytes<double>(64, 512, c.max_capsules, c.max_spheres, h->n_obs, h->has_rays)
                              : lds_bytes<float>(64, 512, c.max_capsules, c.max_spheres, h->n_obs, h->has_rays);
    if (lds > 160 * 1024)
        return fail(h, DOCKAUV_E_INVALID, "configuration needs %zu B of LDS per group (> 160 KiB): fewer rays/obstacles", lds);
    return 0;
}

// what select_step / select_sequence are asked (dockauv_device.h): the handle's constants and what this step's io wants
StepRequest step_request(dockauv_handle h, const dockauv_step_io& io, bool ride) {
    const bool extras = io.noise || io.reward_terms || io.conditions || io.nav || io.ray_dist || io.state_dot || h->trace_dev || h->cfg.device_noise;
    return StepRequest{h->f64, h->sym, h->vk, h->has_rays, h->threads, h->cfg.n_envs, ceil_log2(h->n_rays), h->cfg.reset_mode,
                       h->cfg.reward_set, extras, io.terminal_obs != nullptr, io.pack_reward_done == 2 ? 2 : (io.pack_reward_done ? 1 : 0), ride,
                       h->no_current, h->cfg.max_capsules, h->cfg.max_spheres};
}

}  // namespace

int dockauv::launch(dockauv_handle h, const dockauv_step_io* io, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
    int rc;
    StepIO& sio = h->f64 ? h->a64.io : h->a32.io;
    if (h->trace_dev) {
        // The ring row of a step is a kernel ARGUMENT (host counter): a launch captured into a HIP graph would write the
        // same row on every replay and dockauv_trace_steps would never advance -- refused rather than silently dropped.
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
            return fail(h, DOCKAUV_E_INVALID, "the episode-storage trace (dockauv_trace_enable) cannot be recorded into a HIP graph: "
                        "its ring row is a launch argument; disable the trace or launch the steps directly");
    }
    sio.trace = h->trace_dev;
    sio.trace_step = h->trace_dev ? h->trace_step : 0;
    sio.device_noise = (h->cfg.device_noise && !io->noise) ? 1 : 0;
    set_io(sio, *io);
    const StepRequest r = step_request(h, *io, h->a32.ride.plan != nullptr);
    rc = h->f64 ? launch_step_f64(h->a64, r, stream, ev0, ev1) : launch_step_f32(h->a32, r, stream, ev0, ev1);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "step kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    if (h->trace_dev) ++h->trace_step;   // (only a launch that went out has written its row)
    h->last_stream = stream;
    return 0;
}

extern "C" {

int dockauv_abi_version(void) { return DOCKAUV_ABI_VERSION; }

const char* dockauv_build_info(void) {
#define DOCKAUV_STR_(x) #x
#define DOCKAUV_STR(x) DOCKAUV_STR_(x)
    return "libdockauv gfx950 (HIP), abi " DOCKAUV_STR(DOCKAUV_ABI_VERSION) ", built " __DATE__ " " __TIME__;
}

const char* dockauv_last_error(dockauv_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int dockauv_create(const dockauv_config* cfg, int device, dockauv_handle* out) {
    if (!cfg || !out) return fail(nullptr, DOCKAUV_E_INVALID, "null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(dockauv_config) || cfg->abi_version != DOCKAUV_ABI_VERSION)
        return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_config size/ABI mismatch: got %u/%u, library has %zu/%d",
                    cfg->struct_size, cfg->abi_version, sizeof(dockauv_config), DOCKAUV_ABI_VERSION);
    const dockauv_config& c = *cfg;
    if (c.n_envs <= 0) return fail(nullptr, DOCKAUV_E_INVALID, "n_envs must be > 0");
    if (c.precision != DOCKAUV_F32 && c.precision != DOCKAUV_F64) return fail(nullptr, DOCKAUV_E_INVALID, "bad precision");
    if (c.n_vehicles < 1 || c.n_vehicles > 2) return fail(nullptr, DOCKAUV_E_INVALID, "n_vehicles must be 1 or 2");
    if (c.max_capsules < 0 || c.max_capsules > DOCKAUV_MAX_CAPSULES) return fail(nullptr, DOCKAUV_E_INVALID, "max_capsules out of range");
    if (c.max_spheres < 0 || c.max_spheres > DOCKAUV_MAX_SPHERES) return fail(nullptr, DOCKAUV_E_INVALID, "max_spheres out of range");
    {
        // the kernel forms SoA row offsets in 32-bit arithmetic: row * stride * sizeof(T) must stay below 2^32
        const uint64_t stride = ((uint64_t)c.n_envs + 63) / 64 * 64;
        uint64_t rows = 12;
        if ((uint64_t)c.max_capsules * 7 > rows) rows = (uint64_t)c.max_capsules * 7;
        if ((uint64_t)c.max_spheres * 4 > rows) rows = (uint64_t)c.max_spheres * 4;
        if (rows * stride * (c.precision == DOCKAUV_F64 ? 8 : 4) >= (1ull << 32))
            return fail(nullptr, DOCKAUV_E_INVALID, "n_envs too large for one handle (an SoA array would exceed 4 GiB): shard the batch over several handles");
    }
    if (c.n_v <= 0 || c.n_h <= 0 || (long)c.n_v * c.n_h > DOCKAUV_MAX_RAYS) return fail(nullptr, DOCKAUV_E_INVALID, "bad ray fan %d x %d", c.n_v, c.n_h);
    if (c.blocksize_reduce <= 0) return fail(nullptr, DOCKAUV_E_INVALID, "blocksize_reduce must be > 0");
    if (c.reward_set != 1 && c.reward_set != 2) return fail(nullptr, DOCKAUV_E_INVALID, "reward_set must be 1 or 2");
    if (c.reset_mode < DOCKAUV_RESET_NONE || c.reset_mode > DOCKAUV_RESET_DEVICE)
        return fail(nullptr, DOCKAUV_E_INVALID, "reset_mode %d not supported by this build", c.reset_mode);
    if (c.scenario < DOCKAUV_SCN_SIMPLE || c.scenario > DOCKAUV_SCN_SPHERES) return fail(nullptr, DOCKAUV_E_INVALID, "bad scenario id %d", c.scenario);
    if (c.reset_mode == DOCKAUV_RESET_DEVICE) {
        static const int need[8] = {0, 0, 1, 1, 5, 4, 5, 0};
        if (c.max_capsules < need[c.scenario]) return fail(nullptr, DOCKAUV_E_INVALID, "scenario %d needs %d capsule slots", c.scenario, need[c.scenario]);
    }
    if (!(c.t_step_size > 0)) return fail(nullptr, DOCKAUV_E_INVALID, "t_step_size must be > 0");
    if (!c.ray_table) return fail(nullptr, DOCKAUV_E_INVALID, "ray_table is NULL");
    for (int v = 0; v < c.n_vehicles; ++v) {
        const dockauv_vehicle& vv = c.vehicle[v];
        if (vv.n_u < 1 || vv.n_u > DOCKAUV_MAX_U) return fail(nullptr, DOCKAUV_E_INVALID, "vehicle %d: n_u out of range", v);
        if (vv.kind != DOCKAUV_VEH_CONSTB && vv.kind != DOCKAUV_VEH_LAUV) return fail(nullptr, DOCKAUV_E_INVALID, "vehicle %d: bad kind", v);
        if (vv.kind == DOCKAUV_VEH_LAUV && vv.n_u != 3) return fail(nullptr, DOCKAUV_E_INVALID, "LAUV needs n_u = 3");
    }

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, DOCKAUV_E_NODEVICE, "no HIP device available (%s): libdockauv has no CPU fallback",
                    e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(nullptr, DOCKAUV_E_INVALID, "device %d out of range (have %d)", device, ndev);
    e = hipSetDevice(device);
    if (e != hipSuccess) return fail(nullptr, DOCKAUV_E_HIP, "hipSetDevice: %s", hipGetErrorString(e));

    dockauv_handle h = new dockauv_env_s();
    const int rc = init_handle(h, c, device);
    if (rc != 0) {
        g_create_error = h->err;
        dockauv_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

int dockauv_destroy(dockauv_handle h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    for (void* p : h->allocs) (void)hipFree(p);
    for (void* p : h->pinned_allocs) (void)hipHostFree(p);
    if (h->host_stream) (void)hipStreamDestroy(h->host_stream);
    if (h->ride_plans_dev) (void)hipFree(h->ride_plans_dev);
    for (void* p : h->trace_allocs) (void)hipFree(p);
    if (h->trace_dev) (void)hipFree(h->trace_dev);
    for (int k = 0; k < 2; ++k) {
        if (h->ev_step[k]) (void)hipEventDestroy(h->ev_step[k]);
        if (h->ev_gather[k]) (void)hipEventDestroy(h->ev_gather[k]);
    }
    delete h;
    return 0;
}

int dockauv_n_obs(dockauv_handle h) { return h ? h->n_obs : DOCKAUV_E_INVALID; }
int dockauv_threads_per_group(dockauv_handle h) { return h ? h->threads : DOCKAUV_E_INVALID; }
int dockauv_step_uses_current(dockauv_handle h) {
    if (!h) return DOCKAUV_E_INVALID;
    dockauv_step_io plain{};
    plain.pack_reward_done = 1;
    return select_step(step_request(h, plain, false)).NOCUR ? 0 : 1;
}
int dockauv_step_uses_capsules(dockauv_handle h) {
    if (!h) return DOCKAUV_E_INVALID;
    dockauv_step_io plain{};
    plain.pack_reward_done = 1;
    return select_step(step_request(h, plain, false)).NOCAP ? 0 : 1;
}
int dockauv_n_rays(dockauv_handle h) { return h ? h->n_rays : DOCKAUV_E_INVALID; }
int dockauv_n_u(dockauv_handle h) { return h ? h->n_u_max : DOCKAUV_E_INVALID; }

int dockauv_field_width(dockauv_handle h, int field) {
    if (!h) return DOCKAUV_E_INVALID;
    FieldDesc fd;
    int w = 0;
    int rc = field_info(h, field, &fd, &w);
    return rc ? rc : w;
}

int dockauv_set_field(dockauv_handle h, int field, int first, int count, const double* src) {
    if (!h || !src) return fail(h, DOCKAUV_E_INVALID, "null argument");
    FieldDesc fd;
    int width = 0;
    int rc = field_info(h, field, &fd, &width);
    if (rc) return rc;
    if (first < 0 || count < 0 || (long)first + count > h->cfg.n_envs) return fail(h, DOCKAUV_E_RANGE, "env range [%d, %d) outside [0, %d)", first, first + count, h->cfg.n_envs);
    if (count == 0 || fd.rows == 0) return 0;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t es = elem_size(h, fd.kind);
    std::vector<unsigned char> tmp((size_t)fd.rows * count * es);
    if (is_current_field(field)) {
        // (the handle's "no water current" property survives a write of exact zeros only: before the copy goes out)
        h->no_current = no_current_after_write(h->no_current, src, count);
        // host (V_c, V_min, V_max, alpha, beta) -> device rows (V_c, dir xyz, V_min, V_max, alpha, beta);
        // dir = (cos a cos b, sin b, sin a cos b): objects/current.py:70-74
        for (int i = 0; i < count; ++i) {
            const double* s = src + (size_t)i * 5;
            const double a = s[3], b = s[4];
            const double row[8] = {s[0], std::cos(a) * std::cos(b), std::sin(b), std::sin(a) * std::cos(b), s[1], s[2], a, b};
            for (int k = 0; k < 8; ++k) store_elem(h, 0, tmp.data(), (size_t)k * count + i, row[k]);
        }
    } else {
        for (int i = 0; i < count; ++i)
            for (int k = 0; k < width; ++k) store_elem(h, fd.kind, tmp.data(), (size_t)k * count + i, src[(size_t)i * width + k]);
    }
    unsigned char* dst = static_cast<unsigned char*>(fd.base) + (size_t)first * es;
    HIP_TRY(h, hipMemcpy2D(dst, (size_t)h->S * es, tmp.data(), (size_t)count * es, (size_t)count * es, fd.rows, hipMemcpyHostToDevice));
    if (field == DOCKAUV_F_STATE) {
        // low-order words of position and heading (float path: what the float32 state rows cannot hold of the float64 input)
        std::vector<unsigned char> lo((size_t)kLoRows * count * es);
        for (int i = 0; i < count; ++i)
            for (int k = 0; k < kLoRows; ++k) {
                const double x = src[(size_t)i * width + kLoState[k]];
                store_elem(h, 0, lo.data(), (size_t)k * count + i, h->f64 ? 0.0 : x - (double)(float)x);
            }
        unsigned char* dlo = static_cast<unsigned char*>(h->B.pos_lo) + (size_t)first * es;
        HIP_TRY(h, hipMemcpy2D(dlo, (size_t)h->S * es, lo.data(), (size_t)count * es, (size_t)count * es, kLoRows, hipMemcpyHostToDevice));
    }
    return 0;
}

int dockauv_get_field(dockauv_handle h, int field, int first, int count, double* dst) {
    if (!h || !dst) return fail(h, DOCKAUV_E_INVALID, "null argument");
    FieldDesc fd;
    int width = 0;
    int rc = field_info(h, field, &fd, &width);
    if (rc) return rc;
    if (first < 0 || count < 0 || (long)first + count > h->cfg.n_envs) return fail(h, DOCKAUV_E_RANGE, "env range [%d, %d) outside [0, %d)", first, first + count, h->cfg.n_envs);
    if (count == 0 || fd.rows == 0) return 0;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = sync_last(h)) != 0 || (rc = check_status(h)) != 0) return rc;
    const size_t es = elem_size(h, fd.kind);
    std::vector<unsigned char> tmp((size_t)fd.rows * count * es);
    const unsigned char* srcp = static_cast<const unsigned char*>(fd.base) + (size_t)first * es;
    HIP_TRY(h, hipMemcpy2D(tmp.data(), (size_t)count * es, srcp, (size_t)h->S * es, (size_t)count * es, fd.rows, hipMemcpyDeviceToHost));
    if (is_current_field(field)) {
        static const int rows[5] = {0, 4, 5, 6, 7};
        for (int i = 0; i < count; ++i)
            for (int k = 0; k < 5; ++k) dst[(size_t)i * 5 + k] = load_elem(h, 0, tmp.data(), (size_t)rows[k] * count + i);
    } else {
        for (int i = 0; i < count; ++i)
            for (int k = 0; k < width; ++k) dst[(size_t)i * width + k] = load_elem(h, fd.kind, tmp.data(), (size_t)k * count + i);
    }
    if (field == DOCKAUV_F_STATE && !h->f64) {   // position, heading = their state rows + pos_lo
        std::vector<unsigned char> lo((size_t)kLoRows * count * es);
        const unsigned char* slo = static_cast<const unsigned char*>(h->B.pos_lo) + (size_t)first * es;
        HIP_TRY(h, hipMemcpy2D(lo.data(), (size_t)count * es, slo, (size_t)h->S * es, (size_t)count * es, kLoRows, hipMemcpyDeviceToHost));
        for (int i = 0; i < count; ++i)
            for (int k = 0; k < kLoRows; ++k) dst[(size_t)i * width + kLoState[k]] += load_elem(h, 0, lo.data(), (size_t)k * count + i);
    }
    return 0;
}

int dockauv_reset_envs(dockauv_handle h, int first, int count) {
    if (!h) return DOCKAUV_E_INVALID;
    if (first < 0 || count < 0 || (long)first + count > h->cfg.n_envs) return fail(h, DOCKAUV_E_RANGE, "env range outside [0, %d)", h->cfg.n_envs);
    if (count == 0) return 0;
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = sync_last(h)) return rc;
    const size_t t = h->tsz, S = (size_t)h->S;
    HIP_TRY(h, hipMemset2D(static_cast<unsigned char*>(h->B.state) + first * t, S * t, 0, count * t, 12));
    HIP_TRY(h, hipMemset2D(static_cast<unsigned char*>(h->B.pos_lo) + first * t, S * t, 0, count * t, kLoRows));
    HIP_TRY(h, hipMemset2D(static_cast<unsigned char*>(h->B.u) + first * t, S * t, 0, count * t, kMaxU));
    HIP_TRY(h, hipMemset(static_cast<unsigned char*>(h->B.cum_reward) + first * t, 0, count * t));
    HIP_TRY(h, hipMemset(h->B.t_steps + first, 0, count * 4));
    std::vector<int32_t> ep(count);
    HIP_TRY(h, hipMemcpy(ep.data(), h->B.episode + first, count * 4, hipMemcpyDeviceToHost));
    for (auto& x : ep) x += 1;
    HIP_TRY(h, hipMemcpy(h->B.episode + first, ep.data(), count * 4, hipMemcpyHostToDevice));
    return 0;
}

int dockauv_step(dockauv_handle h, const dockauv_step_io* io, void* hip_stream) {
    if (!h || !io) return fail(h, DOCKAUV_E_INVALID, "null argument");
    if (!io->actions || !io->obs) return fail(h, DOCKAUV_E_INVALID, "actions/obs must not be NULL");
    if (!io->pack_reward_done && (!io->reward || !io->done)) return fail(h, DOCKAUV_E_INVALID, "reward/done must not be NULL unless pack_reward_done");
    HIP_TRY(h, hipSetDevice(h->device));
    return launch(h, io, (hipStream_t)hip_stream);
}

namespace {
// Can the steps ios[0..n) run as ONE resident launch (dockauv_step.hip.inc: step_seq_kernel)?  Steps that select_sequence
// has a kernel for, with packed rows of one kind: everything else is launched step by step.
bool sequence_is_resident_material(dockauv_handle h, const dockauv_step_io* ios, int n) {
    if (!h->seq_resident || n < 2) return false;
    for (int i = 0; i < n; ++i) {
        if (select_sequence(step_request(h, ios[i], false)).unsupported || ios[i].reward || ios[i].done) return false;
        if (ios[i].pack_reward_done != ios[0].pack_reward_done) return false;
    }
    return true;
}
}  // namespace

int dockauv_set_option(dockauv_handle h, int option, int value) {
    if (!h) return DOCKAUV_E_INVALID;
    switch (option) {
        case DOCKAUV_OPT_SEQUENCE_RESIDENT: h->seq_resident = value != 0; return 0;
    }
    return fail(h, DOCKAUV_E_INVALID, "unknown option %d", option);
}

int dockauv_step_sequence(dockauv_handle h, const dockauv_step_io* ios, int n, void* hip_stream) {
    if (!h || !ios || n < 0) return fail(h, DOCKAUV_E_INVALID, "bad argument");
    for (int i = 0; i < n; ++i) {
        if (!ios[i].actions || !ios[i].obs) return fail(h, DOCKAUV_E_INVALID, "step %d: actions/obs must not be NULL", i);
        if (!ios[i].pack_reward_done && (!ios[i].reward || !ios[i].done))
            return fail(h, DOCKAUV_E_INVALID, "step %d: reward/done must not be NULL unless pack_reward_done", i);
    }
    HIP_TRY(h, hipSetDevice(h->device));
    if (sequence_is_resident_material(h, ios, n)) {
        // the fast path: chunks of up to kSeqMax steps, each ONE launch in which every group walks its envs through the
        // chunk's steps (no launch boundary between them); same bytes as the loop below writes
        set_io(h->a32.io, ios[0]);
        h->a32.io.trace = nullptr;
        h->a32.io.trace_step = 0;
        h->a32.io.device_noise = 0;
        bool fell_back = false;
        for (int i0 = 0; i0 < n && !fell_back; i0 += kSeqMax) {
            SeqArgs seq;
            seq.n = std::min(kSeqMax, n - i0);
            for (int k = 0; k < kSeqMax; ++k) {
                const int i = i0 + std::min(k, seq.n - 1);
                seq.actions[k] = ios[i].actions;
                seq.obs[k] = ios[i].obs;
            }
            const int rc = launch_sequence_f32(h->a32, step_request(h, ios[0], false), seq, (hipStream_t)hip_stream);
            if (rc == (int)hipErrorNotSupported && i0 == 0) { fell_back = true; break; }
            if (rc != 0) return fail(h, DOCKAUV_E_HIP, "resident step sequence launch failed: %s", hipGetErrorString((hipError_t)rc));
        }
        if (!fell_back) {
            h->last_stream = (hipStream_t)hip_stream;
            return 0;
        }
    }
    for (int i = 0; i < n; ++i) {
        int rc = launch(h, &ios[i], (hipStream_t)hip_stream);
        if (rc) return rc;
    }
    return 0;
}

int dockauv_step_gather_sequence(dockauv_handle h, const dockauv_step_io* ios, int n, const dockauv_p2p_plan* plans,
                                 int n_plans, uint64_t t0, int lag, void* compute_stream, void* gather_stream) {
    if (!h || !ios || !plans || n < 0 || n_plans < 1 || lag < 0 || lag > 1) return fail(h, DOCKAUV_E_INVALID, "bad argument");
    for (int i = 0; i < n; ++i)
        if (!ios[i].actions || !ios[i].obs || !ios[i].pack_reward_done)
            return fail(h, DOCKAUV_E_INVALID, "step %d: actions/obs must not be NULL and pack_reward_done must be set", i);
    {
        // the plans' slices are rows of the step's packed layout: float32 rows of n_obs + 2 words (pack_reward_done = 1)
        const uint64_t row_bytes = (uint64_t)(h->n_obs + 2) * 4u * (uint64_t)h->cfg.n_envs;
        for (int i = 0; i < n; ++i)
            if (ios[i].pack_reward_done != 1)
                return fail(h, DOCKAUV_E_INVALID, "step %d: the peer-to-peer gather ships float32 packed rows (pack_reward_done = 1); "
                            "bfloat16 rows (2) are gathered over RCCL", i);
        for (int k = 0; k < n_plans; ++k)
            if (plans[k].bytes != row_bytes)
                return fail(h, DOCKAUV_E_INVALID, "plan %d: slice of %llu bytes, the handle's packed rows are %llu", k,
                            (unsigned long long)plans[k].bytes, (unsigned long long)row_bytes);
    }
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t cs = (hipStream_t)compute_stream, gs = (hipStream_t)gather_stream;
    const bool two = cs != gs;
    if (!two && lag == 1) {
        // the gather of step t rides in the grid of step kernel t + 1 (dockauv_ride.h); the last one is flushed by a
        // gather kernel of its own, so that on return everything queued here is covered by the stream
        // float32, structural fast path, and steps the product instantiations serve (dockauv_device.h: select_step); first
        // what the handle alone decides, then what each step asks for
        StepRequest r = step_request(h, dockauv_step_io{}, true);
        if (r.f64 || !r.sym) return fail(h, DOCKAUV_E_INVALID, "lag 1 needs the float kernels of the structural fast path");
        if (needs_full_kernel(r))
            return fail(h, DOCKAUV_E_INVALID, "lag 1 needs the product kernels (no pool reset, reward set 1, fans of 9-16 or 33-64 rays, no logging)");
        for (int i = 0; i < n; ++i) {
            r = step_request(h, ios[i], true);
            if (r.extras || r.terminal_obs)
                return fail(h, DOCKAUV_E_INVALID, "lag 1 needs the product kernels: step %d asks for optional inputs / outputs", i);
        }
        if (n_plans < 4) return fail(h, DOCKAUV_E_INVALID, "lag 1 needs at least 4 plans (gather buffers)");
        for (int i = 1; i < n; ++i)
            if (ios[i].obs == ios[i - 1].obs)
                return fail(h, DOCKAUV_E_INVALID, "step %d: lag 1 needs alternating row buffers (obs of consecutive steps differ)", i);
        for (int k = 0; k < n_plans; ++k)
            if (plans[k].bytes == 0 || plans[k].bytes % 16 != 0 || !plans[k].counter || !plans[k].status || !plans[k].my_flags ||
                plans[k].n_dsts < 1 || plans[k].n_dsts > DOCKAUV_P2P_MAX_PEERS + 1 || plans[k].n_peers < 0 ||
                plans[k].n_peers > DOCKAUV_P2P_MAX_PEERS)
                return fail(h, DOCKAUV_E_INVALID, "plan %d: bad plan (slices must be multiples of 16 bytes)", k);
        const size_t pbytes = sizeof(dockauv_p2p_plan) * (size_t)n_plans;
        if (h->ride_plans_host.size() != pbytes || memcmp(h->ride_plans_host.data(), plans, pbytes) != 0) {
            if (h->ride_plans_host.size() != pbytes) {
                if (h->ride_plans_dev) {
                    HIP_TRY(h, hipStreamSynchronize(cs));
                    HIP_TRY(h, hipFree(h->ride_plans_dev));
                    h->ride_plans_dev = nullptr;
                }
                HIP_TRY(h, hipMalloc(&h->ride_plans_dev, pbytes));
            } else {
                HIP_TRY(h, hipStreamSynchronize(cs));
            }
            HIP_TRY(h, hipMemcpy(h->ride_plans_dev, plans, pbytes, hipMemcpyHostToDevice));
            h->ride_plans_host.assign(reinterpret_cast<const unsigned char*>(plans), reinterpret_cast<const unsigned char*>(plans) + pbytes);
        }
        const unsigned long n16 = plans[0].bytes / 16;
        unsigned long cg = n16 / ((unsigned long)h->threads * 2);
        cg = cg < 8 ? 8 : (cg > 256 ? 256 : cg);
        RideLaunch& ride = h->a32.ride;
        for (int i = 0; i < n; ++i) {
            const uint64_t t = t0 + (uint64_t)i;
            ride = RideLaunch{};
            if (i >= 1) {
                uint32_t stamp = (uint32_t)t;            // gather of step t - 1 carries stamp (t - 1) + 1
                if (stamp == 0) stamp = 1;
                ride.plan = static_cast<const dockauv_p2p_plan*>(h->ride_plans_dev) + ((t - 1) % (uint64_t)n_plans);
                ride.src = ios[i - 1].obs;
                ride.stamp = ride.wait_stamp = stamp;
                ride.groups = (int)cg;
            }
            int rc = launch(h, &ios[i], cs);
            ride = RideLaunch{};
            if (rc) return rc;
        }
        if (n >= 1) {
            const uint64_t t = t0 + (uint64_t)(n - 1);
            uint32_t stamp = (uint32_t)(t + 1);
            if (stamp == 0) stamp = 1;
            int rc = launch_gather(&plans[t % (uint64_t)n_plans], ios[n - 1].obs, stamp, stamp, cs);
            if (rc) return fail(h, rc, "%s", g_create_error.c_str());
        }
        return 0;
    }
    if (two)
        for (int k = 0; k < 2; ++k) {
            if (!h->ev_step[k]) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_step[k], hipEventDisableTiming));
            if (!h->ev_gather[k]) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_gather[k], hipEventDisableTiming));
        }
    for (int i = 0; i < n; ++i) {
        const uint64_t t = t0 + (uint64_t)i;
        const int k = (int)(t & 1);
        if (two && i >= 2) HIP_TRY(h, hipStreamWaitEvent(cs, h->ev_gather[k], 0));   // rows k are free again
        int rc = launch(h, &ios[i], cs);
        if (rc) return rc;
        if (two) {
            HIP_TRY(h, hipEventRecord(h->ev_step[k], cs));
            HIP_TRY(h, hipStreamWaitEvent(gs, h->ev_step[k], 0));
        }
        uint32_t stamp = (uint32_t)(t + 1), wait = t + 1 > (uint64_t)lag ? (uint32_t)(t + 1 - (uint64_t)lag) : 0;
        if (stamp == 0) stamp = 1;
        rc = launch_gather(&plans[t % (uint64_t)n_plans], ios[i].obs, stamp, wait, gs);
        if (rc) return fail(h, rc, "%s", g_create_error.c_str());
        if (two) HIP_TRY(h, hipEventRecord(h->ev_gather[k], gs));
    }
    if (two)
        for (int i = (n >= 2 ? n - 2 : 0); i < n; ++i)
            HIP_TRY(h, hipStreamWaitEvent(cs, h->ev_gather[(t0 + (uint64_t)i) & 1], 0));
    return 0;
}

namespace {
int pinned_alloc(dockauv_handle h, void** p, size_t bytes) {
    if (bytes == 0) bytes = 64;
    hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
    if (e != hipSuccess) return fail(h, DOCKAUV_E_HIP, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    h->pinned_allocs.push_back(*p);
    return 0;
}

int ensure_pinned(dockauv_handle h) {
    if (h->pinned_ready) return 0;
    for (auto& st : h->stage)
        if (int rc = pinned_alloc(h, &st.pin, st.bytes)) return rc;
    HIP_TRY(h, hipStreamCreate(&h->host_stream));   // blocking stream: ordered after the null-stream copies of set_field / reset_envs
    h->pinned_ready = true;
    return 0;
}
}  // namespace

// Host-pointer step: the caller's (pageable) arrays are staged through pinned mirrors so that every transfer is one
// asynchronous DMA on the library's stream: actions up, kernel, requested outputs down, ONE synchronisation.
int dockauv_step_host(dockauv_handle h, const dockauv_step_io* io) {
    if (!h || !io) return fail(h, DOCKAUV_E_INVALID, "null argument");
    if (!io->actions || !io->obs || !io->reward || !io->done) return fail(h, DOCKAUV_E_INVALID, "actions/obs/reward/done must not be NULL");
    if (io->pack_reward_done) return fail(h, DOCKAUV_E_INVALID, "pack_reward_done is a device-pointer feature (dockauv_step)");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = ensure_pinned(h);
    if (rc) return rc;
    // work queued by the caller on another stream (dockauv_step) must be visible first
    if (h->last_stream && h->last_stream != h->host_stream) HIP_TRY(h, hipStreamSynchronize(h->last_stream));
    const size_t N = (size_t)h->cfg.n_envs;
    hipStream_t s = h->host_stream;
    // the caller's array of every slot (null: not asked for) and the device buffer that stands in for it
    void* const user[ST_COUNT] = {const_cast<void*>(io->actions), const_cast<void*>(io->noise), io->obs, io->reward, io->done,
                                  io->reward_terms, io->conditions, io->nav, io->ray_dist, io->terminal_obs, io->state_dot};
    const auto dev = [&](int k) { return user[k] ? h->stage[k].dev : nullptr; };
    for (int k = ST_ACTIONS; k <= ST_NOISE; ++k) {
        const auto& st = h->stage[k];
        if (!user[k]) continue;
        std::memcpy(st.pin, user[k], st.bytes);
        HIP_TRY(h, hipMemcpyAsync(st.dev, st.pin, st.bytes, hipMemcpyHostToDevice, s));
    }
    dockauv_step_io d{};
    d.actions = dev(ST_ACTIONS), d.noise = dev(ST_NOISE), d.obs = (float*)dev(ST_OBS), d.reward = dev(ST_REWARD);
    d.done = (uint8_t*)dev(ST_DONE), d.reward_terms = dev(ST_TERMS), d.conditions = (uint8_t*)dev(ST_COND), d.nav = dev(ST_NAV);
    d.ray_dist = dev(ST_RAYDIST), d.terminal_obs = (float*)dev(ST_TERMOBS), d.state_dot = dev(ST_STATEDOT);
    rc = launch(h, &d, s);
    if (rc) return rc;
    // (terminal observations: only the rows of finished envs, below)
    for (int k = ST_OBS; k < ST_COUNT; ++k)
        if (user[k] && k != ST_TERMOBS)
            HIP_TRY(h, hipMemcpyAsync(h->stage[k].pin, h->stage[k].dev, h->stage[k].bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    if ((rc = check_status(h)) != 0) return rc;
    if (io->terminal_obs) {
        // terminal observations only exist for envs that finished in this step: fetch the rows of those envs only
        // (typically none or a few; the buffer is as large as the observations themselves)
        const uint8_t* dn = static_cast<const uint8_t*>(h->stage[ST_DONE].pin);
        float* const pin_term = static_cast<float*>(h->stage[ST_TERMOBS].pin);
        const float* const dev_term = static_cast<const float*>(h->stage[ST_TERMOBS].dev);
        size_t first = N, last = 0, runs = 0;
        for (size_t i = 0; i < N; ++i)
            if (dn[i]) {
                if (first == N) first = i;
                if (i == 0 || !dn[i - 1]) ++runs;
                last = i;
            }
        if (runs > 0) {
            if (runs <= 4) {
                for (size_t i = first; i <= last;) {
                    if (!dn[i]) { ++i; continue; }
                    size_t j = i;
                    while (j <= last && dn[j]) ++j;
                    HIP_TRY(h, hipMemcpyAsync(pin_term + i * h->n_obs, dev_term + i * h->n_obs,
                                              (j - i) * h->n_obs * 4, hipMemcpyDeviceToHost, s));
                    i = j;
                }
            } else {   // many scattered rows: one DMA over the span beats a launch per row
                HIP_TRY(h, hipMemcpyAsync(pin_term + first * h->n_obs, dev_term + first * h->n_obs,
                                          (last - first + 1) * h->n_obs * 4, hipMemcpyDeviceToHost, s));
            }
            HIP_TRY(h, hipStreamSynchronize(s));
            for (size_t i = first; i <= last; ++i)
                if (dn[i]) std::memcpy(io->terminal_obs + i * h->n_obs, pin_term + i * h->n_obs, (size_t)h->n_obs * 4);
        }
    }
    for (int k = ST_OBS; k < ST_COUNT; ++k)
        if (user[k] && k != ST_TERMOBS) std::memcpy(user[k], h->stage[k].pin, h->stage[k].bytes);
    return 0;
}

// ---------------------------------------------------------------------------------------------- episode-storage trace
namespace {
void trace_free(dockauv_handle h) {
    for (void* p : h->trace_allocs) (void)hipFree(p);
    h->trace_allocs.clear();
    if (h->trace_dev) (void)hipFree(h->trace_dev);
    h->trace_dev = nullptr;
    h->trace = TraceDev{};
    h->trace_step = 0;
}
}  // namespace

int dockauv_trace_enable(dockauv_handle h, const int32_t* env_ids, int n_rows, int capacity) {
    if (!h) return DOCKAUV_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = sync_last(h)) return rc;
    trace_free(h);
    if (n_rows == 0) return 0;
    if (!env_ids || n_rows < 0 || capacity < 1) return fail(h, DOCKAUV_E_INVALID, "bad trace arguments");
    const int N = h->cfg.n_envs;
    std::vector<int32_t> slot((size_t)N, -1);
    for (int j = 0; j < n_rows; ++j) {
        if (env_ids[j] < 0 || env_ids[j] >= N || (j > 0 && env_ids[j] <= env_ids[j - 1]))
            return fail(h, DOCKAUV_E_RANGE, "trace env ids must be strictly increasing inside [0, %d)", N);
        slot[(size_t)env_ids[j]] = j;
    }
    const size_t rows = (size_t)capacity * (size_t)n_rows, t = h->tsz;
    auto alloc = [&](void** p, size_t bytes) -> int {
        hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) return fail(h, DOCKAUV_E_HIP, "hipMalloc(%zu) for the trace failed: %s", bytes, hipGetErrorString(e));
        h->trace_allocs.push_back(*p);
        e = hipMemset(*p, 0, bytes);
        return e == hipSuccess ? 0 : fail(h, DOCKAUV_E_HIP, "hipMemset failed: %s", hipGetErrorString(e));
    };
    TraceDev& tr = h->trace;
    void* slot_dev = nullptr;
    int rc = 0;
    if ((rc = alloc(&slot_dev, (size_t)N * 4)) || (rc = alloc(&tr.state_pre, rows * 12 * t)) || (rc = alloc(&tr.state, rows * 12 * t)) ||
        (rc = alloc(&tr.state_dot, rows * 12 * t)) || (rc = alloc(&tr.u, rows * kMaxU * t)) || (rc = alloc(&tr.nu_c, rows * 3 * t)) ||
        (rc = alloc((void**)&tr.obs, rows * (size_t)h->n_obs * 4)) || (rc = alloc(&tr.reward_terms, rows * kNRew * t)) ||
        (rc = alloc((void**)&tr.cond, rows))) {
        trace_free(h);
        return rc;
    }
    tr.slot_of_env = static_cast<const int32_t*>(slot_dev);
    tr.n_rows = n_rows;
    tr.capacity = capacity;
    hipError_t e = hipMemcpy(slot_dev, slot.data(), (size_t)N * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&h->trace_dev, sizeof(TraceDev));
    if (e == hipSuccess) e = hipMemcpy(h->trace_dev, &tr, sizeof(TraceDev), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        trace_free(h);
        return fail(h, DOCKAUV_E_HIP, "trace set-up failed: %s", hipGetErrorString(e));
    }
    h->trace_step = 0;
    return 0;
}

long long dockauv_trace_steps(dockauv_handle h) { return h ? h->trace_step : (long long)DOCKAUV_E_INVALID; }

int dockauv_trace_read(dockauv_handle h, long long first_step, int n_steps, double* state_pre, double* state, double* state_dot,
                       double* u, double* nu_c, float* obs, double* reward_terms, uint8_t* conditions) {
    if (!h || !h->trace_dev) return fail(h, DOCKAUV_E_INVALID, "trace is not enabled");
    const TraceDev& tr = h->trace;
    if (n_steps < 0 || first_step < 0 || first_step + n_steps > h->trace_step || h->trace_step - first_step > tr.capacity)
        return fail(h, DOCKAUV_E_RANGE, "steps [%lld, %lld) are not in the ring (recorded %lld, capacity %d)", first_step,
                    first_step + n_steps, h->trace_step, tr.capacity);
    if (n_steps == 0) return 0;
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc_ = sync_last(h)) return rc_;
    if (int rc_ = check_status(h)) return rc_;
    const size_t R = (size_t)tr.n_rows;
    std::vector<unsigned char> tmp;
    // one ring array -> host [n_steps][n_rows][w]; kind 0 = T -> double, 1 = float, 2 = uint8
    auto fetch = [&](const void* dev, int w, int kind, void* out) -> int {
        if (!out) return 0;
        const size_t es = kind == 0 ? h->tsz : (kind == 1 ? 4 : 1), row_bytes = R * (size_t)w * es;
        tmp.resize(row_bytes * (size_t)n_steps);
        for (int k = 0; k < n_steps; ++k) {
            const size_t slot = (size_t)((first_step + k) % tr.capacity);
            HIP_TRY(h, hipMemcpy(tmp.data() + (size_t)k * row_bytes, static_cast<const unsigned char*>(dev) + slot * row_bytes, row_bytes, hipMemcpyDeviceToHost));
        }
        const size_t n = (size_t)n_steps * R * (size_t)w;
        if (kind == 0) for (size_t i = 0; i < n; ++i) static_cast<double*>(out)[i] = load_elem(h, 0, tmp.data(), i);
        else std::memcpy(out, tmp.data(), n * es);
        return 0;
    };
    int rc;
    if ((rc = fetch(tr.state_pre, 12, 0, state_pre)) || (rc = fetch(tr.state, 12, 0, state)) || (rc = fetch(tr.state_dot, 12, 0, state_dot)) ||
        (rc = fetch(tr.u, kMaxU, 0, u)) || (rc = fetch(tr.nu_c, 3, 0, nu_c)) || (rc = fetch(tr.obs, h->n_obs, 1, obs)) ||
        (rc = fetch(tr.reward_terms, kNRew, 0, reward_terms)) || (rc = fetch(tr.cond, 1, 2, conditions)))
        return rc;
    return 0;
}

int dockauv_synchronize(dockauv_handle h) {
    if (!h) return DOCKAUV_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = sync_last(h)) return rc;
    return check_status(h);
}

int dockauv_poll_status(dockauv_handle h) {
    if (!h) return DOCKAUV_E_INVALID;
    return check_status(h);   // (a plain load of host memory: no HIP call, no synchronisation)
}

int dockauv_time_steps(dockauv_handle h, const dockauv_step_io* io, void* hip_stream, int steps, double* avg_us) {
    if (!h || !io || !avg_us || steps <= 0) return fail(h, DOCKAUV_E_INVALID, "bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)hip_stream;
    // one start/stop event pair per dispatch, attached to the dispatch itself (hipExtLaunchKernelGGL): the sum of
    // the elapsed times is pure kernel time on this stream, without launch gaps -- what rocprofv3 --kernel-trace
    // reports as the kernel's duration.
    std::vector<hipEvent_t> ev(2 * (size_t)steps);
    for (auto& e : ev) HIP_TRY(h, hipEventCreate(&e));
    for (int i = 0; i < steps; ++i) {
        int rc = launch(h, io, s, ev[2 * i], ev[2 * i + 1]);
        if (rc) return rc;
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    double total_ms = 0.0;
    for (int i = 0; i < steps; ++i) {
        float ms = 0.f;
        HIP_TRY(h, hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
        total_ms += ms;
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    *avg_us = total_ms * 1000.0 / steps;
    return check_status(h);
}

#ifdef DOCKAUV_STAMPS
// diagnostic build only (scripts/stamps.py): 64 groups x 32 s_memtime stamps of the last f32 step
int dockauv_debug_read_stamps(unsigned long long* out) {
    (void)hipDeviceSynchronize();
    return dockauv::read_stamps(out);
}
// start / end of every group of the last f32 step on both clocks (scripts/span.py)
int dockauv_debug_read_span(unsigned long long* out, int groups) {
    (void)hipDeviceSynchronize();
    return dockauv::read_span(out, groups);
}
#endif

}  // extern "C"
