// dockauv_eval.hip -- policy evaluation with an episode quota per env, for gfx950 (MI355X)
// (include/dockauv.h: dockauv_eval_begin / dockauv_eval_scan; the reference's counterpart is predict(gym_env, model_path,
// n_episodes), train.py:86-118, SB3's is evaluate_policy: only the first target[i] episodes of env i count, so that an env with
// short episodes -- the collisions -- weighs no more than one with long ones).
//
// Begin: one lane per env zeroes its count and its S slots (outcome 255) and clamps its target to [0, S].
// Scan: the monitor's (dockauv_monitor.hip: monitor_scan_kernel) -- one lane per env walks its K steps forwards with the reward /
// done words of kEvalChunk steps requested together and unconditionally (a chunk that reaches past step K - 1 reads step K - 1
// again and drops the result), every offset 64-bit, lanes >= N neither read nor write, three words of the terminal observation
// loaded inside the done branch -- with the same float32 add and the same outcome rule.  A finished episode goes to
// slot [count][env] while count < target; past the target the walk goes on (the carries stay the handle's) and records nothing.
// Totals: AFTER the walk a lane adds its own slots j = 0 .. count - 1 in order, whichever scan wrote them (counts as integers, the
// two return sums in float64), the 64 lanes of a group are added by the monitor's butterfly, the group's kEvalWords words go to the
// evaluator's workspace ([word][group]) and one final group of kEvalFinalThreads lanes adds them as monitor_final_kernel does:
// lane t the groups t, t + 1 024, .. in order, the lanes by the same butterfly, the sixteen waves in order.  No atomics: the bits
// depend on the inputs, N, S and the union of the scans' steps only.  TWO launches a scan (the walk, the final sums), one a begin.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dockauv_device.h"

namespace dockauv {
namespace {

constexpr int kEvalChunk = 8;             // steps whose loads are in flight together
constexpr int kEvalFinalThreads = 1024;   // 1 048 576 envs are 16 384 groups: sixteen partials a lane

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
// words of a partial: the monitor's thirteen (0 episodes, 1 sum return, 2 sum return^2, 3 sum length, 4 / 5 min / max return,
// 6 / 7 min / max length, 8..12 outcome counts), then 13 the episodes still missing
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
__device__ __forceinline__ int clamp_int(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__global__ __launch_bounds__(kEvalThreads) void eval_begin_kernel(const int32_t* __restrict__ targets, int uniform_target,
                                                                  int32_t* __restrict__ count, int32_t* __restrict__ target,
                                                                  float* __restrict__ ep_return, int32_t* __restrict__ ep_length,
                                                                  uint8_t* __restrict__ ep_outcome, int n_envs, int n_slots) {
    const int env = blockIdx.x * kEvalThreads + threadIdx.x;
    if (env >= n_envs) return;
    count[env] = 0;
    target[env] = clamp_int(targets ? targets[env] : uniform_target, 0, n_slots);
    for (int j = 0; j < n_slots; ++j) {
        const size_t o = (size_t)j * (size_t)n_envs + (size_t)env;
        ep_return[o] = 0.0f;
        ep_length[o] = 0;
        ep_outcome[o] = (uint8_t)255;
    }
}

__global__ __launch_bounds__(kEvalThreads) void eval_scan_kernel(const EvalArgs a) {
    const int env = blockIdx.x * kEvalThreads + threadIdx.x;
    int n_ep = 0, len_min = 0x7fffffff, len_max = 0, missing = 0;
    int oc0 = 0, oc1 = 0, oc2 = 0, oc3 = 0, oc4 = 0;
    long long len_sum = 0;
    double s1 = 0.0, s2 = 0.0;
    float ret_min = INFINITY, ret_max = -INFINITY;
    if (env < a.n_envs) {
        const size_t N = (size_t)a.n_envs, stride = (size_t)a.row_stride;
        const float* rd = a.rows + (size_t)env * stride + (size_t)a.n_obs;   // reward word of (step 0, env); step k: + k N stride
        float c_ret = a.carry_ret[env];
        int c_len = a.carry_len[env];
        // (begin leaves 0 <= count <= target <= S; the clamps keep the slot stores inside the arrays whatever the caller wrote
        // through dockauv_eval_state's pointers)
        const int tgt = clamp_int(a.target[env], 0, a.n_slots);
        int cnt = clamp_int(a.count[env], 0, tgt);
        for (int k0 = 0; k0 < a.n_steps; k0 += kEvalChunk) {
            float r[kEvalChunk], d[kEvalChunk];
#pragma unroll
            for (int j = 0; j < kEvalChunk; ++j) {
                const int k = k0 + j < a.n_steps ? k0 + j : a.n_steps - 1;   // (past the last step: that step again, dropped below)
                const float* p = rd + (size_t)k * N * stride;
                r[j] = p[0];
                d[j] = p[1];
            }
#pragma unroll
            for (int j = 0; j < kEvalChunk; ++j) {
                const int k = k0 + j;
                if (k < a.n_steps) {
                    // include/dockauv.h (dockauv_eval_scan) states this order: the monitor's
                    const float ret = c_ret + r[j];
                    const int len = c_len + 1;
                    if (d[j] > 0.5f) {
                        if (cnt < tgt) {
                            int code = 255;
                            if (a.terminal_obs) {
                                const float* to = a.terminal_obs + ((size_t)k * N + (size_t)env) * (size_t)a.n_obs;
                                const float t0 = to[0], t6 = to[6], t7 = to[7];
                                code = t0 == 0.0f ? 0 : t0 == 1.0f ? 1 : (fabsf(t6) == 1.0f || fabsf(t7) == 1.0f) ? 2
                                       : len > a.max_timesteps ? 3 : 4;
                            }
                            const size_t o = (size_t)cnt * N + (size_t)env;
                            a.ep_return[o] = ret;
                            a.ep_length[o] = len;
                            a.ep_outcome[o] = (uint8_t)code;
                            cnt += 1;
                        }
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
        a.count[env] = cnt;
        missing = tgt - cnt;
        // the lane's own slots, in order: what this scan and the earlier ones since begin recorded (its own stores: program order)
        for (int j = 0; j < cnt; ++j) {
            const size_t o = (size_t)j * N + (size_t)env;
            const float ret = a.ep_return[o];
            const int len = a.ep_length[o];
            const int code = a.ep_outcome[o];
            oc0 += code == 0;
            oc1 += code == 1;
            oc2 += code == 2;
            oc3 += code == 3;
            oc4 += code == 4;
            n_ep += 1;
            len_sum += len;
            s1 += (double)ret;
            s2 += (double)ret * (double)ret;
            ret_min = fminf(ret_min, ret);
            ret_max = fmaxf(ret_max, ret);
            len_min = len < len_min ? len : len_min;
            len_max = len > len_max ? len : len_max;
        }
    }
    double w[kEvalWords] = {(double)n_ep, s1, s2, (double)len_sum, (double)ret_min, (double)ret_max,
                            n_ep ? (double)len_min : (double)INFINITY, n_ep ? (double)len_max : -(double)INFINITY,
                            (double)oc0, (double)oc1, (double)oc2, (double)oc3, (double)oc4, (double)missing};
#pragma unroll
    for (int i = 0; i < kEvalWords; ++i) w[i] = word_wave(i, w[i]);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kEvalWords; ++i) a.partial[(size_t)i * (size_t)gridDim.x + blockIdx.x] = w[i];
    }
}

// one group: the scan's partials [kEvalWords][n_groups] -> stats [16] in the layout of dockauv_monitor_io.stats
__global__ __launch_bounds__(kEvalFinalThreads) void eval_final_kernel(const double* __restrict__ partial, int n_groups,
                                                                       double* __restrict__ stats) {
    constexpr int kWaves = kEvalFinalThreads / 64;
    __shared__ double sh[kWaves][kEvalWords];
    __shared__ double res[kEvalWords];
    double w[kEvalWords];
#pragma unroll
    for (int i = 0; i < kEvalWords; ++i) w[i] = word_identity(i);
    for (int g = threadIdx.x; g < n_groups; g += kEvalFinalThreads) {
#pragma unroll
        for (int i = 0; i < kEvalWords; ++i) w[i] = word_combine(i, w[i], partial[(size_t)i * (size_t)n_groups + g]);
    }
#pragma unroll
    for (int i = 0; i < kEvalWords; ++i) w[i] = word_wave(i, w[i]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < kEvalWords; ++i) sh[threadIdx.x >> 6][i] = w[i];
    }
    __syncthreads();
    if (threadIdx.x < kEvalWords) {
        const int i = threadIdx.x;
        double v = sh[0][i];
        for (int wv = 1; wv < kWaves; ++wv) v = word_combine(i, v, sh[wv][i]);
        res[i] = v;
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        const int i = threadIdx.x;
        const double n_ep = res[0], nan = __longlong_as_double(0x7ff8000000000000LL);
        double v;
        if (i < 4) v = res[i];
        else if (i < 8) v = n_ep > 0.0 ? res[i] : nan;
        else if (i < 13) v = res[i];
        else if (i == 13) v = (((res[8] + res[9]) + res[10]) + res[11]) + res[12];   // classified: exact integers
        else if (i == 14) v = nan;
        else v = res[13];
        stats[i] = v;
    }
}

}  // namespace

int launch_eval_begin(const int32_t* targets, int uniform_target, int32_t* count, int32_t* target, float* ep_return,
                      int32_t* ep_length, uint8_t* ep_outcome, int n_envs, int n_slots, void* stream) {
    if (n_envs < 1 || n_slots < 1 || (long long)n_envs * (long long)n_slots >= (1LL << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(eval_begin_kernel, dim3((unsigned)eval_groups(n_envs)), dim3(kEvalThreads), 0, (hipStream_t)stream, targets,
                       uniform_target, count, target, ep_return, ep_length, ep_outcome, n_envs, n_slots);
    return (int)hipGetLastError();
}

int launch_eval_scan(const EvalArgs& a, void* stream) {
    if (a.n_steps < 1 || a.n_envs < 1 || a.n_obs < 8 || a.n_slots < 1 || (long long)a.n_envs * (long long)a.n_slots >= (1LL << 31))
        return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const int groups = eval_groups(a.n_envs);
    hipLaunchKernelGGL(eval_scan_kernel, dim3((unsigned)groups), dim3(kEvalThreads), 0, s, a);
    hipLaunchKernelGGL(eval_final_kernel, dim3(1), dim3(kEvalFinalThreads), 0, s, (const double*)a.partial, groups, a.stats);
    return (int)hipGetLastError();
}

}  // namespace dockauv
