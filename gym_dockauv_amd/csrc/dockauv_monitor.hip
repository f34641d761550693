// dockauv_monitor.hip -- episode monitor on the packed rows of a collection, for gfx950 (MI355X)
// (include/dockauv.h: dockauv_monitor_scan; the reference's counterparts are SB3's rollout/ep_rew_mean, rollout/ep_len_mean and
// train/explained_variance, and the success / collision rates debug.py:192-194 forms from the info dict of docking3d.py:388-400).
//
// Scan: one lane per env walks its K steps forwards, carrying the running return and length of its episode; the carries come
// from and go back to the monitor's per-env arrays.  The load shape is gae_kernel's (dockauv_collect.hip): the reward / done
// words of kMonChunk steps are requested together and unconditionally -- a chunk that reaches past step K - 1 reads step K - 1
// again and drops the result --, every offset is 64-bit, lanes >= N neither read nor write, the observation columns are never
// touched.  Only a lane whose episode ends loads anything else: three words of that step's terminal observation, inside the
// branch, because it is rare.
// Totals: a lane keeps its own (counts as integers, the two return sums in float64), the 64 lanes of a group are added by a
// fixed butterfly, the group's kMonWords words go to the monitor's workspace ([word][group]: the final launch reads them
// coalesced), and one final group of kMonFinalThreads lanes adds them -- lane t the groups t, t + 1 024, .. in order, the lanes
// by the same butterfly, the sixteen waves in order.  No atomics: the bits depend on the inputs, N and K only.
// Explained variance: two passes over the contiguous returns / values on a bounded grid, float64 sums in the same fixed order;
// every group of the second pass forms the means itself from the first pass's partials, so all groups centre on the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dockauv_device.h"

namespace dockauv {
namespace {

constexpr int kMonChunk = 8;            // steps whose loads are in flight together
constexpr int kMonFinalThreads = 1024;  // 1 048 576 envs are 16 384 groups: sixteen partials a lane
constexpr int kEvThreads = 256;
constexpr int kEvChunk = 4;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmin(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}
// words of a partial: 0 episodes, 1 sum return, 2 sum return^2, 3 sum length, 4 / 5 min / max return, 6 / 7 min / max length,
// 8..12 outcome counts; in the final launch 13 / 14 carry the two squared sums of the explained variance
__device__ __forceinline__ constexpr bool word_is_min(int i) { return i == 4 || i == 6; }
__device__ __forceinline__ constexpr bool word_is_max(int i) { return i == 5 || i == 7; }
__device__ __forceinline__ double word_identity(int i) {
    return word_is_min(i) ? (double)INFINITY : word_is_max(i) ? -(double)INFINITY : 0.0;
}
__device__ __forceinline__ double word_combine(int i, double a, double b) {
    return word_is_min(i) ? fmin(a, b) : word_is_max(i) ? fmax(a, b) : a + b;
}
__device__ __forceinline__ double word_wave(int i, double v) {
    return word_is_min(i) ? wave_min(v) : word_is_max(i) ? wave_max(v) : wave_sum(v);
}

__global__ __launch_bounds__(kMonThreads) void monitor_scan_kernel(const MonitorArgs a) {
    const int env = blockIdx.x * kMonThreads + threadIdx.x;
    int n_ep = 0, len_min = 0x7fffffff, len_max = 0;
    int oc0 = 0, oc1 = 0, oc2 = 0, oc3 = 0, oc4 = 0;
    long long len_sum = 0;
    double s1 = 0.0, s2 = 0.0;
    float ret_min = INFINITY, ret_max = -INFINITY;
    if (env < a.n_envs) {
        const size_t N = (size_t)a.n_envs, stride = (size_t)a.row_stride;
        const float* rd = a.rows + (size_t)env * stride + (size_t)a.n_obs;   // reward word of (step 0, env); step k: + k N stride
        float c_ret = a.carry_ret[env];
        int c_len = a.carry_len[env];
        for (int k0 = 0; k0 < a.n_steps; k0 += kMonChunk) {
            float r[kMonChunk], d[kMonChunk];
#pragma unroll
            for (int j = 0; j < kMonChunk; ++j) {
                const int k = k0 + j < a.n_steps ? k0 + j : a.n_steps - 1;   // (past the last step: that step again, dropped below)
                const float* p = rd + (size_t)k * N * stride;
                r[j] = p[0];
                d[j] = p[1];
            }
#pragma unroll
            for (int j = 0; j < kMonChunk; ++j) {
                const int k = k0 + j;
                if (k < a.n_steps) {
                    // include/dockauv.h (dockauv_monitor_scan) states this order
                    const float ret = c_ret + r[j];
                    const int len = c_len + 1;
                    if (d[j] > 0.5f) {
                        const size_t o = (size_t)k * N + (size_t)env;
                        if (a.terminal_obs) {
                            const float* to = a.terminal_obs + o * (size_t)a.n_obs;
                            const float t0 = to[0], t6 = to[6], t7 = to[7];
                            const int code = t0 == 0.0f ? 0 : t0 == 1.0f ? 1 : (fabsf(t6) == 1.0f || fabsf(t7) == 1.0f) ? 2
                                             : len > a.max_timesteps ? 3 : 4;
                            oc0 += code == 0;
                            oc1 += code == 1;
                            oc2 += code == 2;
                            oc3 += code == 3;
                            oc4 += code == 4;
                            if (a.ep_outcome) a.ep_outcome[o] = (uint8_t)code;
                        }
                        if (a.ep_return) a.ep_return[o] = ret;
                        if (a.ep_length) a.ep_length[o] = len;
                        n_ep += 1;
                        len_sum += len;
                        s1 += (double)ret;
                        s2 += (double)ret * (double)ret;
                        ret_min = fminf(ret_min, ret);
                        ret_max = fmaxf(ret_max, ret);
                        len_min = len < len_min ? len : len_min;
                        len_max = len > len_max ? len : len_max;
                        c_ret = 0.0f;
                        c_len = 0;
                    } else {
                        c_ret = ret;
                        c_len = len;
                    }
                }
            }
        }
        a.carry_ret[env] = c_ret;
        a.carry_len[env] = c_len;
    }
    double w[kMonWords] = {(double)n_ep, s1, s2, (double)len_sum, (double)ret_min, (double)ret_max,
                           n_ep ? (double)len_min : (double)INFINITY, n_ep ? (double)len_max : -(double)INFINITY,
                           (double)oc0, (double)oc1, (double)oc2, (double)oc3, (double)oc4};
#pragma unroll
    for (int i = 0; i < kMonWords; ++i) w[i] = word_wave(i, w[i]);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kMonWords; ++i) a.partial[(size_t)i * (size_t)gridDim.x + blockIdx.x] = w[i];
    }
}

// sum over the lanes of a group of kEvThreads: the waves by the butterfly, then the four waves in order; every lane gets it
__device__ __forceinline__ double ev_group_sum(double v, double* sh) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __syncthreads();
    return s;
}

// lane t of group g takes the elements (g kEvThreads + t) + j (groups kEvThreads), kEvChunk of them in flight.  SECOND: the
// sums of squares about the means, which every group forms itself from the first pass's partials [2][kEvMaxGroups]
template <bool SECOND>
__global__ __launch_bounds__(kEvThreads) void monitor_ev_kernel(const float* __restrict__ returns, const float* __restrict__ values,
                                                                 long long n, const double* __restrict__ first, double* __restrict__ out) {
    __shared__ double sh[kEvThreads / 64];
    double my = 0.0, me = 0.0;
    if (SECOND) {
        const bool has = (int)threadIdx.x < (int)gridDim.x;
        const double py = has ? first[threadIdx.x] : 0.0, pe = has ? first[kEvMaxGroups + threadIdx.x] : 0.0;
        my = ev_group_sum(py, sh) / (double)n;
        me = ev_group_sum(pe, sh) / (double)n;
    }
    const long long step = (long long)gridDim.x * kEvThreads;
    double sy = 0.0, se = 0.0;
    for (long long i0 = (long long)blockIdx.x * kEvThreads + threadIdx.x; i0 < n; i0 += step * kEvChunk) {
        float y[kEvChunk], v[kEvChunk];
#pragma unroll
        for (int j = 0; j < kEvChunk; ++j) {
            const long long i = i0 + j * step < n ? i0 + j * step : i0;   // (past the end: the first again, dropped below)
            y[j] = returns[i];
            v[j] = values[i];
        }
#pragma unroll
        for (int j = 0; j < kEvChunk; ++j) {
            if (i0 + j * step < n) {
                const double dy = (double)y[j], de = (double)(y[j] - v[j]);   // (the error in float32, as SB3 forms it)
                if (SECOND) {
                    const double qy = dy - my, qe = de - me;
                    sy = fma(qy, qy, sy);
                    se = fma(qe, qe, se);
                } else {
                    sy += dy;
                    se += de;
                }
            }
        }
    }
    sy = ev_group_sum(sy, sh);
    se = ev_group_sum(se, sh);
    if (threadIdx.x == 0) {
        out[blockIdx.x] = sy;
        out[kEvMaxGroups + blockIdx.x] = se;
    }
}

// one group: the scan's partials [kMonWords][n_groups] and the explained variance's second-pass partials -> stats [16]
__global__ __launch_bounds__(kMonFinalThreads) void monitor_final_kernel(const double* __restrict__ partial, int n_groups,
                                                                         const double* __restrict__ ev2, int n_ev_groups, int classified,
                                                                         double* __restrict__ stats) {
    constexpr int kWords = kMonWords + 2, kWaves = kMonFinalThreads / 64;
    __shared__ double sh[kWaves][kWords];
    __shared__ double res[kWords];
    double w[kWords];
#pragma unroll
    for (int i = 0; i < kWords; ++i) w[i] = word_identity(i);
    for (int g = threadIdx.x; g < n_groups; g += kMonFinalThreads) {
#pragma unroll
        for (int i = 0; i < kMonWords; ++i) w[i] = word_combine(i, w[i], partial[(size_t)i * (size_t)n_groups + g]);
    }
    if ((int)threadIdx.x < n_ev_groups) {
        w[kMonWords] = ev2[threadIdx.x];
        w[kMonWords + 1] = ev2[kEvMaxGroups + threadIdx.x];
    }
#pragma unroll
    for (int i = 0; i < kWords; ++i) w[i] = word_wave(i, w[i]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < kWords; ++i) sh[threadIdx.x >> 6][i] = w[i];
    }
    __syncthreads();
    if (threadIdx.x < kWords) {
        const int i = threadIdx.x;
        double v = sh[0][i];
        for (int wv = 1; wv < kWaves; ++wv) v = word_combine(i, v, sh[wv][i]);
        res[i] = v;
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        const int i = threadIdx.x;
        const double n_ep = res[0], nan = __longlong_as_double(0x7ff8000000000000LL);
        double v = 0.0;
        if (i < 4) v = res[i];
        else if (i < 8) v = n_ep > 0.0 ? res[i] : nan;
        else if (i < 13) v = classified ? res[i] : 0.0;
        else if (i == 13) v = classified ? n_ep : 0.0;
        else if (i == 14) v = (n_ev_groups > 0 && res[kMonWords] != 0.0) ? 1.0 - res[kMonWords + 1] / res[kMonWords] : nan;
        stats[i] = v;
    }
}

}  // namespace

int launch_monitor_scan(const MonitorArgs& a, void* stream) {
    if (a.n_steps < 1 || a.n_envs < 1 || a.n_obs < 8) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const int groups = monitor_groups(a.n_envs);
    hipLaunchKernelGGL(monitor_scan_kernel, dim3((unsigned)groups), dim3(kMonThreads), 0, s, a);
    int n_ev = 0;
    if (a.returns && a.values) {
        const long long n = (long long)a.n_steps * (long long)a.n_envs;
        const long long want = (n + kEvThreads - 1) / kEvThreads;
        n_ev = (int)(want < kEvMaxGroups ? want : kEvMaxGroups);
        hipLaunchKernelGGL(monitor_ev_kernel<false>, dim3((unsigned)n_ev), dim3(kEvThreads), 0, s, a.returns, a.values, n,
                           (const double*)nullptr, a.ev_partial);
        hipLaunchKernelGGL(monitor_ev_kernel<true>, dim3((unsigned)n_ev), dim3(kEvThreads), 0, s, a.returns, a.values, n,
                           (const double*)a.ev_partial, a.ev_partial + 2 * kEvMaxGroups);
    }
    hipLaunchKernelGGL(monitor_final_kernel, dim3(1), dim3(kMonFinalThreads), 0, s, (const double*)a.partial, groups,
                       (const double*)(a.ev_partial + 2 * kEvMaxGroups), n_ev, a.terminal_obs ? 1 : 0, a.stats);
    return (int)hipGetLastError();
}

}  // namespace dockauv
