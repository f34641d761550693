// dockauv_rewnorm.hip -- reward normalisation on the packed rows of a collection, for gfx950 (MI355X)
// (include/dockauv.h: dockauv_rewnorm_scan; the counterpart is SB3 1.5's VecNormalize(norm_reward=True, norm_obs=False) with its
// RunningMeanStd: every reward divided by the running standard deviation of the discounted return, then clipped).
//
// Training mode, FOUR launches on the stream; frozen mode (training == 0), ONE (the last of the four, on the current variance):
//  1 rewnorm_scan_kernel     one lane per env in groups of 64 walks its K steps forwards with the discounted-return carry,
//                            ret = carry * gamma + reward[k] in float32 with two roundings (__fmul_rn, __fadd_rn: never an fma),
//                            and stores discounted[k][env].  The load shape is monitor_scan_kernel's (dockauv_monitor.hip): the
//                            reward / done words of kRnChunk steps are requested together and unconditionally -- a chunk that
//                            reaches past step K - 1 reads step K - 1 again and drops the result --, every offset is 64-bit, lanes
//                            >= N neither read nor write, the observation columns are never touched.  The raw reward is parked
//                            in reward_norm[k][env], so that launch 4 streams one contiguous column in place and the strided
//                            rows (a 64-byte line per 4-byte reward) are fetched once per scan, not twice.
//  2 rewnorm_moments_kernel  one group of kRnMomThreads lanes per step: the float64 mean of discounted[k][0 .. N) and, in a second
//                            pass over the same (contiguous, coalesced) column, the population variance about that mean.
//  3 rewnorm_merge_kernel    one wave: the K merges of SB3's update_from_moments, in step order.  Every lane carries the same
//                            chain on the same values (the per-step moments are loaded 64 steps at a time, one step a lane, and
//                            handed round by __shfl); lane j keeps and stores the variance and the divisor of step k0 + j.
//  4 rewnorm_apply_kernel    streaming over [K][N]: reward_norm = (float) clamp((double) reward / den_k, -clip, clip), den_k read
//                            from step_stats by every group -- the same bits for all of them.  Frozen: the reward comes from
//                            the rows and every group forms den = sqrt(var + epsilon) itself from the one running variance.
// Order of the sums (no atomics; the bits depend on the inputs, N and K only): in the moments kernel lane t adds the elements
// t, t + 1 024, t + 2 048, .. in that order (kRnMomChunk loads in flight), the 64 lanes of a wave are added by the fixed butterfly
// of dockauv_monitor.hip (wave_sum), the sixteen waves in index order; the second pass accumulates fma(q, q, sum), q = x - mean.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dockauv_device.h"

namespace dockauv {
namespace {

constexpr int kRnChunk = 8;             // steps whose loads are in flight together (the monitor's)
constexpr int kRnMomThreads = 1024;     // 65 536 envs: 64 elements a lane and pass
constexpr int kRnMomChunk = 4;
constexpr int kRnApplyThreads = 256;
constexpr unsigned kRnApplyMaxY = 65535;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(kRnThreads) void rewnorm_scan_kernel(const RewnormArgs a) {
    const int env = blockIdx.x * kRnThreads + threadIdx.x;
    if (env >= a.n_envs) return;
    const size_t N = (size_t)a.n_envs, stride = (size_t)a.row_stride;
    const float* rd = a.rows + (size_t)env * stride + (size_t)a.n_obs;   // reward word of (step 0, env); step k: + k N stride
    float carry = a.carry[env];
    for (int k0 = 0; k0 < a.n_steps; k0 += kRnChunk) {
        float r[kRnChunk], d[kRnChunk];
#pragma unroll
        for (int j = 0; j < kRnChunk; ++j) {
            const int k = k0 + j < a.n_steps ? k0 + j : a.n_steps - 1;   // (past the last step: that step again, dropped below)
            const float* p = rd + (size_t)k * N * stride;
            r[j] = p[0];
            d[j] = p[1];
        }
#pragma unroll
        for (int j = 0; j < kRnChunk; ++j) {
            const int k = k0 + j;
            if (k < a.n_steps) {
                // include/dockauv.h (dockauv_rewnorm_scan) states this order: two roundings
                const float ret = __fadd_rn(__fmul_rn(carry, a.gamma), r[j]);
                const size_t o = (size_t)k * N + (size_t)env;
                a.discounted[o] = ret;
                a.reward_norm[o] = r[j];   // parked for the apply pass: it reads a contiguous column, not the rows again
                carry = d[j] > 0.5f ? 0.0f : ret;
            }
        }
    }
    a.carry[env] = carry;
}

// sum over the lanes of a group of kRnMomThreads: the waves by the butterfly, then the sixteen waves in order; every lane gets it
__device__ __forceinline__ double mom_group_sum(double v, double* sh) {
    constexpr int kWaves = kRnMomThreads / 64;
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = sh[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s += sh[w];
    __syncthreads();
    return s;
}

// group k: step_stats[k][0] = mean, [1] = population variance of discounted[k][0 .. N)
__global__ __launch_bounds__(kRnMomThreads) void rewnorm_moments_kernel(const float* __restrict__ discounted, int n_envs,
                                                                         double* __restrict__ step_stats) {
    __shared__ double sh[kRnMomThreads / 64];
    const int k = blockIdx.x;
    const float* x = discounted + (size_t)k * (size_t)n_envs;
    constexpr int kSpan = kRnMomThreads * kRnMomChunk;
    double mean = 0.0, res[2] = {0.0, 0.0};
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        double s = 0.0;
        for (int i0 = threadIdx.x; i0 < n_envs; i0 += kSpan) {
            float v[kRnMomChunk];
#pragma unroll
            for (int j = 0; j < kRnMomChunk; ++j) {
                const int i = i0 + j * kRnMomThreads;
                v[j] = x[i < n_envs ? i : i0];   // (past the end: the first again, dropped below)
            }
#pragma unroll
            for (int j = 0; j < kRnMomChunk; ++j) {
                if (i0 + j * kRnMomThreads < n_envs) {
                    if (pass == 0) {
                        s += (double)v[j];
                    } else {
                        const double q = (double)v[j] - mean;
                        s = fma(q, q, s);
                    }
                }
            }
        }
        res[pass] = mom_group_sum(s, sh) / (double)n_envs;
        mean = res[0];
    }
    if (threadIdx.x == 0) {
        step_stats[(size_t)k * 4 + 0] = res[0];
        step_stats[(size_t)k * 4 + 1] = res[1];
    }
}

// one wave: state (mean, var, count) <- the K merges; step_stats[k][2] = var after step k, [3] = sqrt(var + epsilon)
__global__ __launch_bounds__(64) void rewnorm_merge_kernel(double* __restrict__ state, double* __restrict__ step_stats, int n_steps,
                                                           int n_envs, double epsilon) {
    const int lane = threadIdx.x;
    double mean = state[0], var = state[1], count = state[2];
    const double bn = (double)n_envs;
    for (int k0 = 0; k0 < n_steps; k0 += 64) {
        const int kl = k0 + lane < n_steps ? k0 + lane : n_steps - 1;
        const double bm = step_stats[(size_t)kl * 4 + 0], bv = step_stats[(size_t)kl * 4 + 1];
        double my_var = 0.0;
        const int n = n_steps - k0 < 64 ? n_steps - k0 : 64;
        for (int j = 0; j < n; ++j) {
            const double batch_mean = __shfl(bm, j, 64), batch_var = __shfl(bv, j, 64);
            // include/dockauv.h (dockauv_rewnorm_scan) states this order; no multiply-add is written, so none is fused
            const double delta = batch_mean - mean;
            const double tot = count + bn;
            const double step = delta * bn;
            mean = mean + step / tot;
            const double m_a = var * count;
            const double m_b = batch_var * bn;
            const double d2 = delta * delta;
            const double cross = d2 * count;
            const double cross_n = cross * bn;
            const double m2 = (m_a + m_b) + cross_n / tot;
            var = m2 / tot;
            count = tot;
            my_var = lane == j ? var : my_var;
        }
        if (lane < n) {
            step_stats[(size_t)(k0 + lane) * 4 + 2] = my_var;
            step_stats[(size_t)(k0 + lane) * 4 + 3] = sqrt(my_var + epsilon);
        }
    }
    if (lane == 0) {
        state[0] = mean;
        state[1] = var;
        state[2] = count;
    }
}

// reward_norm[k][env] for env = blockIdx.x kRnApplyThreads + threadIdx.x and the steps blockIdx.y, blockIdx.y + gridDim.y, ..
// FROZEN: one divisor for every step, formed from the running variance; step_stats (nullable): [k][3] = that divisor
template <bool FROZEN>
__global__ __launch_bounds__(kRnApplyThreads) void rewnorm_apply_kernel(const RewnormArgs a) {
    const int env = blockIdx.x * kRnApplyThreads + threadIdx.x;
    const size_t N = (size_t)a.n_envs, stride = (size_t)a.row_stride;
    const double clip = (double)a.clip_reward;
    double den = 0.0;
    if (FROZEN) den = sqrt(a.state[1] + a.epsilon);
    for (int k = blockIdx.y; k < a.n_steps; k += gridDim.y) {
        if (FROZEN) {
            if (a.step_stats && blockIdx.x == 0 && threadIdx.x == 0) a.step_stats[(size_t)k * 4 + 3] = den;
        } else {
            den = a.step_stats[(size_t)k * 4 + 3];
        }
        if (env < a.n_envs) {
            const size_t o = (size_t)k * N + (size_t)env;
            const float r = FROZEN ? a.rows[o * stride + (size_t)a.n_obs] : a.reward_norm[o];   // (training: parked by the scan)
            const double q = (double)r / den;
            a.reward_norm[o] = (float)fmin(fmax(q, -clip), clip);
        }
    }
}

__global__ __launch_bounds__(kRnApplyThreads) void rewnorm_reset_kernel(float* __restrict__ carry, double* __restrict__ state, int n_envs) {
    const int i = blockIdx.x * kRnApplyThreads + threadIdx.x;
    if (i < n_envs) carry[i] = 0.0f;
    if (i < 4) state[i] = i == 1 ? 1.0 : i == 2 ? 1e-4 : 0.0;
}

}  // namespace

int launch_rewnorm_scan(const RewnormArgs& a, void* stream) {
    if (a.n_steps < 1 || a.n_envs < 1 || a.n_obs < 1) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const unsigned ax = (unsigned)((a.n_envs + kRnApplyThreads - 1) / kRnApplyThreads);
    const unsigned ay = (unsigned)a.n_steps < kRnApplyMaxY ? (unsigned)a.n_steps : kRnApplyMaxY;
    if (a.training) {
        hipLaunchKernelGGL(rewnorm_scan_kernel, dim3((unsigned)rewnorm_groups(a.n_envs)), dim3(kRnThreads), 0, s, a);
        hipLaunchKernelGGL(rewnorm_moments_kernel, dim3((unsigned)a.n_steps), dim3(kRnMomThreads), 0, s, (const float*)a.discounted,
                           a.n_envs, a.step_stats);
        hipLaunchKernelGGL(rewnorm_merge_kernel, dim3(1), dim3(64), 0, s, a.state, a.step_stats, a.n_steps, a.n_envs, a.epsilon);
        hipLaunchKernelGGL(rewnorm_apply_kernel<false>, dim3(ax, ay), dim3(kRnApplyThreads), 0, s, a);
    } else {
        hipLaunchKernelGGL(rewnorm_apply_kernel<true>, dim3(ax, ay), dim3(kRnApplyThreads), 0, s, a);
    }
    return (int)hipGetLastError();
}

int launch_rewnorm_reset(float* carry, double* state, int n_envs, void* stream) {
    if (n_envs < 1) return (int)hipErrorInvalidValue;
    const unsigned groups = (unsigned)((n_envs + kRnApplyThreads - 1) / kRnApplyThreads);
    hipLaunchKernelGGL(rewnorm_reset_kernel, dim3(groups), dim3(kRnApplyThreads), 0, (hipStream_t)stream, carry, state, n_envs);
    return (int)hipGetLastError();
}

}  // namespace dockauv
