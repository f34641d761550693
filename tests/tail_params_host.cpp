// CPU check of the packed tail part of the parameter block (gym_dockauv_amd/csrc/dockauv_device.h: TailP, pack_tail): every
// EnvP field element gets a value of its own, the fan / slot integers are set as dockauv_create sets them for a sensor-free,
// a 16-ray and a 63-ray config of either vehicle, the block is packed, and every slot must hold the bits of its source.
// Prints one line per failure and "ok <checked slots>" at the end; tests/test_tail_params_host.py compiles and runs it.
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "dockauv_device.h"

using namespace dockauv;

static int failures = 0;

template <typename T>
static bool same_bits(const T& a, const T& b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

template <typename T>
static void expect(const char* what, int i, const T& got, const T& want, int& checked) {
    ++checked;
    if (!same_bits(got, want)) {
        std::printf("FAIL %s[%d]: %.9g != %.9g\n", what, i, (double)got, (double)want);
        ++failures;
    }
}

// every T-sized word of a parameter struct gets its own value (integers included: they are overwritten where it matters)
template <typename T, typename S>
static void fill_distinct(S& s, double first) {
    T words[sizeof(S) / sizeof(T)];
    for (size_t i = 0; i < sizeof(S) / sizeof(T); ++i) words[i] = (T)(first + 0.37 * (double)i);
    std::memset(&s, 0, sizeof(S));
    std::memcpy(&s, words, sizeof(words));
}

// vehicle: 0 = BlueROV2 (six inputs), 1 = LAUV (three); n_rays: 0 (sensor-free), 16 (one row of beams), 63 (7 x 9 fan)
template <typename T>
static int check_config(const char* name, int vehicle, int n_rays) {
    ParamBlock<T, 2> P;
    std::memset(&P, 0xff, sizeof(P));
    fill_distinct<T>(P.E, 1000.0 + 100.0 * vehicle + n_rays);
    EnvP<T>& E = P.E;
    E.n_envs = 66; E.max_timesteps = 7; E.reward_set = 1; E.reset_mode = 2; E.scenario = 3;
    E.n_v = n_rays == 63 ? 7 : (n_rays ? 1 : 0); E.n_h = n_rays == 63 ? 9 : n_rays; E.blk = n_rays == 63 ? 3 : 2;
    E.n_rays = n_rays; E.n_red = n_rays == 63 ? 9 : n_rays / 2; E.n_obs = 16 + E.n_red;
    E.max_cap = n_rays == 63 ? 5 : 0; E.max_sph = n_rays == 16 ? 8 : 0; E.n_u_max = vehicle ? 3 : 6;
    E.ray_pad = n_rays ? (n_rays == 63 ? 64 : 16) : 0; E.ray_pad_log2 = n_rays ? (n_rays == 63 ? 6 : 4) : 0;
    E.bf16_wpr = (E.n_obs + 1) / 2 + 2; E.bf16_magic = 0x12345678u + (unsigned)n_rays; E.device_noise = 0;
    pack_tail(P.Q, P.E);
    const TailP<T>& Q = P.Q;
    int checked = 0;
    expect("inv_log_tol", 0, Q.inv_log_tol, E.inv_log_tol, checked);
    expect("dtol", 0, Q.dtol, E.dtol, checked);
    expect("dmax", 0, Q.dmax, E.dmax, checked);
    expect("max_att", 0, Q.max_att, E.max_att, checked);
    expect("max_timesteps", 0, Q.max_timesteps, E.max_timesteps, checked);
    expect("reset_mode", 0, Q.reset_mode, E.reset_mode, checked);
    expect("n_obs", 0, Q.n_obs, E.n_obs, checked);
    expect("inv_dmax", 0, Q.inv_dmax, E.inv_dmax, checked);
    expect("ray_max", 0, Q.ray_max, E.ray_max, checked);
    expect("fan_cos", 0, Q.fan_cos, E.fan_cos, checked);
    expect("fan_sin", 0, Q.fan_sin, E.fan_sin, checked);
    expect("safety", 0, Q.safety, E.safety, checked);
    expect("max_cap", 0, Q.max_cap, E.max_cap, checked);
    expect("max_sph", 0, Q.max_sph, E.max_sph, checked);
    expect("ray_pad", 0, Q.ray_pad, E.ray_pad, checked);
    expect("ray_pad_log2", 0, Q.ray_pad_log2, E.ray_pad_log2, checked);
    expect("n_rays", 0, Q.n_rays, E.n_rays, checked);
    expect("n_red", 0, Q.n_red, E.n_red, checked);
    expect("inv_ray_max", 0, Q.inv_ray_max, E.inv_ray_max, checked);
    expect("sum_beta", 0, Q.sum_beta, E.sum_beta, checked);
    for (int i = 0; i < 6; ++i) expect("inv_vel", i, Q.inv_vel[i], E.inv_vel[i], checked);
    expect("inv_max_att", 0, Q.inv_max_att, E.inv_max_att, checked);
    expect("inv_log_tol_eps", 0, Q.inv_log_tol_eps, E.inv_log_tol_eps, checked);
    expect("w_d", 0, Q.w_d, E.w_d, checked);
    expect("w_dth", 0, Q.w_dth, E.w_dth, checked);
    expect("w_dpsi", 0, Q.w_dpsi, E.w_dpsi, checked);
    expect("w_phi", 0, Q.w_phi, E.w_phi, checked);
    expect("w_th", 0, Q.w_th, E.w_th, checked);
    expect("w_thdot", 0, Q.w_thdot, E.w_thdot, checked);
    expect("w_oa", 0, Q.w_oa, E.w_oa, checked);
    for (int i = 0; i < 5; ++i) expect("w_done", i, Q.w_done[i], E.w_done[i], checked);
    // all slots of the block are accounted for: nothing but padding is left (integers are 4 bytes in either precision)
    const size_t n_int = 9, n_real = 31;
    if ((size_t)checked != n_int + n_real || n_int * 4 + n_real * sizeof(T) > sizeof(TailP<T>) ||
        sizeof(TailP<T>) - (n_int * 4 + n_real * sizeof(T)) >= 64 + (sizeof(T) == 8 ? 32 : 0)) {
        std::printf("FAIL %s: %d slots checked, %zu expected, block of %zu bytes\n", name, checked, n_int + n_real, sizeof(TailP<T>));
        ++failures;
    }
    // layout: whole 64-byte lines at a 64-byte offset, appended -- behind the hot blocks, which keep their offset
    typedef ParamBlock<T, 2> PB;
    const size_t off = offsetof(PB, Q), hot = offsetof(PB, H);
    if (sizeof(TailP<T>) % 64 || alignof(TailP<T>) != 64 || off % 64 || sizeof(PB) % 64 || off != hot + 2 * sizeof(HotP<T>) ||
        off + sizeof(TailP<T>) != sizeof(PB) || offsetof(PB, E) != 0 || offsetof(PB, V) != sizeof(EnvP<T>)) {
        std::printf("FAIL %s: sizeof(TailP) %zu, alignof %zu, offset %zu, hot blocks at %zu, sizeof(ParamBlock) %zu\n", name,
                    sizeof(TailP<T>), alignof(TailP<T>), off, hot, sizeof(PB));
        ++failures;
    }
    // the groups a role asks for are adjacent: the integrating wave's batch (decision + every role + record completion) lies in
    // the block's first line in float32
    if (sizeof(T) == 4 && (offsetof(TailP<T>, inv_log_tol) != 0 || offsetof(TailP<T>, safety) + sizeof(T) > 64 ||
                           offsetof(TailP<T>, reset_mode) != offsetof(TailP<T>, max_timesteps) + 4 ||
                           offsetof(TailP<T>, ray_max) != offsetof(TailP<T>, inv_dmax) + sizeof(T))) {
        std::printf("FAIL %s: the integrating wave's groups are not one run of words in the first line\n", name);
        ++failures;
    }
    std::printf("%s: %d slots, TailP %zu bytes at offset %zu of %zu\n", name, checked, sizeof(TailP<T>), off, sizeof(PB));
    return checked;
}

int main() {
    int n = 0;
    const int fans[3] = {0, 16, 63};
    const char* vname[2] = {"BlueROV2", "LAUV"};
    char name[96];
    for (int v = 0; v < 2; ++v) {
        for (int f = 0; f < 3; ++f) {
            std::snprintf(name, sizeof(name), "f32 %s %d rays", vname[v], fans[f]);
            n += check_config<float>(name, v, fans[f]);
            std::snprintf(name, sizeof(name), "f64 %s %d rays", vname[v], fans[f]);
            n += check_config<double>(name, v, fans[f]);
        }
    }
    if (failures) return 1;
    std::printf("ok %d\n", n);
    return 0;
}
