// dockauv_head.hip -- the PPO head on one minibatch for gfx950 (MI355X): advantage normalisation, the Gaussian log-probability,
// ratio and clipping, value loss, entropy, the gradients on the actor's and the critic's raw outputs and on log_std, and the
// statistics SB3 logs (include/dockauv.h: dockauv_ppo_head states every float32 expression; the reference's counterpart is the
// loss block of SB3's PPO.train, train.py:64-71).  It sits between dockauv_policy_forward_rows and dockauv_policy_backward.
//
// Up to three launches on a bounded grid of G = min(passes, kBwdMaxGroups) groups of four waves; a pass is kHeadPassRows rows,
// a group walks the passes b = blockIdx.x, blockIdx.x + G, ...; lane t of a pass takes the rows t, t + 256, t + 512, t + 768 of it,
// so that a wave-instruction reads 256 contiguous bytes of every dense array and the loads of kHeadChunk rows are in flight
// together (the kernel is bound by the latency of a dependent load -- the index, then the row arrays -- not by traffic; the
// loads are unconditional: rows behind the minibatch and actions behind n_out read a valid neighbour again and are dropped).
//   ppo_head_moments_kernel (normalize_advantage only): per group the float64 sum of its advantages, then -- re-reading them --
//     the float64 sum of float32 squares centred on the GROUP's float32 mean.  One partial (sum, squares, centre, count) a group.
//   ppo_head_rows_kernel: a group fetches the moment partials into LDS in one trip (a lane four words), and every thread adds
//     them from there in group order (head_moments_: the squares are moved from the groups' centres to the minibatch mean in
//     float64, which is exact algebra and has nothing to cancel; broadcast reads, the same bits in every thread), then the rows:
//     grad_mean, grad_v, and kHeadSums float64 sums of float32 per-row terms; a group's sums are added over the lanes of a wave
//     by a fixed shuffle tree and over the waves in order, and written as one partial.
//   ppo_head_final_kernel: thread k adds sum k of the partials in group order, rounds once, and the statistics are formed.
// No floating-point atomics: every bit is a function of the inputs, a row's position in the minibatch and n_rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dockauv.h"
#include "dockauv_device.h"

namespace dockauv {
namespace {

constexpr float kHalfLog2Pi = 0.91893853320467274f;    // log(2 pi) / 2 (dockauv_policy.hip)
constexpr float kEntropyConst = 1.41893853320467274f;  // 0.5 + log(2 pi) / 2

// lane 0 gets the sum over the 64 lanes, added in the order of this tree
__device__ __forceinline__ double wave_sum_(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// position in the minibatch of chunk slot c of lane tid in pass b
__device__ __forceinline__ long head_row_(long b, int c, int tid) { return b * kHeadPassRows + c * kHeadThreads + tid; }

// the advantage moments from the groups' partials, the same bits in every thread: m = mean, s = unbiased standard deviation
__device__ __forceinline__ void head_moments_(const double* mom, int groups, long n, float& m, float& s) {
    double sum = 0.0;
    for (int g = 0; g < groups; ++g) sum += mom[kHeadMoments * g];
    const double mean = sum / (double)n;
    double m2 = 0.0;
    for (int g = 0; g < groups; ++g) {
        const double sg = mom[kHeadMoments * g], qg = mom[kHeadMoments * g + 1], cg = mom[kHeadMoments * g + 2], ng = mom[kHeadMoments * g + 3];
        const double dc = cg - mean;
        // sum (x - mean)^2 = sum (x - c)^2 + 2 (c - mean) sum (x - c) + n_g (c - mean)^2 over the group's rows
        m2 += qg + (2.0 * dc * (sg - ng * cg) + ng * dc * dc);
    }
    m = (float)mean;
    s = (float)sqrt(fmax(m2, 0.0) / (double)(n - 1));
}

__global__ __launch_bounds__(kHeadThreads) void ppo_head_moments_kernel(const HeadArgs a) {
    __shared__ double red[kHeadThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long passes = (a.n + kHeadPassRows - 1) / kHeadPassRows;
    double part[2] = {0.0, 0.0};            // the group's sum; its centred squares
    float centre = 0.0f;
    long count = 0;
    for (int phase = 0; phase < 2; ++phase) {
        double acc = 0.0;
        for (long b = blockIdx.x; b < passes; b += gridDim.x) {
            long at[kHeadChunk];
            float x[kHeadChunk];
#pragma unroll
            for (int c = 0; c < kHeadChunk; ++c) {
                const long r = head_row_(b, c, tid), rc = r < a.n ? r : a.n - 1;
                at[c] = a.row_index ? (long)a.row_index[rc] : rc;
            }
#pragma unroll
            for (int c = 0; c < kHeadChunk; ++c) x[c] = a.advantages[at[c]];
#pragma unroll
            for (int c = 0; c < kHeadChunk; ++c) {
                if (head_row_(b, c, tid) < a.n) {
                    const float d = x[c] - centre;          // (phase 0: centre = 0)
                    acc += (double)(phase ? d * d : d);
                }
            }
            if (phase == 0) {
                const long left = a.n - b * kHeadPassRows;
                count += left < kHeadPassRows ? left : kHeadPassRows;
            }
        }
        const double w = wave_sum_(acc);
        __syncthreads();                    // (the waves have read red[] of phase 0)
        if (lane == 0) red[wave] = w;
        __syncthreads();
        part[phase] = ((red[0] + red[1]) + red[2]) + red[3];
        if (phase == 0) centre = (float)(part[0] / (double)count);
    }
    if (tid == 0) {
        double* out = a.moments + kHeadMoments * blockIdx.x;
        out[0] = part[0];
        out[1] = part[1];
        out[2] = (double)centre;
        out[3] = (double)count;
    }
}

// Args: HeadArgs (dockauv_ppo_head) or HeadArgsVf (dockauv_ppo_update with clip_range_vf > 0: the value error is taken at the
// value clipped to v_old +- clip_vf, include/dockauv.h: dockauv_ppo_update)
template <class Args>
__global__ __launch_bounds__(kHeadThreads) void ppo_head_rows_kernel(const Args a) {
    __shared__ double red[kHeadThreads / 64][kHeadSums];
    __shared__ double mom[kBwdMaxGroups * kHeadMoments];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_u = a.n_out;
    float m = 0.0f, s = 1.0f, den = 1.0f;
    if (a.normalize) {      // (the same in every thread)
        for (int i = tid; i < (int)gridDim.x * kHeadMoments; i += kHeadThreads) mom[i] = a.moments[i];
        __syncthreads();
        head_moments_(mom, (int)gridDim.x, a.n, m, s);
        den = s + 1e-8f;
    }
    if (blockIdx.x == 0 && tid == 0) {
        a.stats[6] = m;
        a.stats[7] = s;
    }
    float ls[DOCKAUV_MAX_U], inv_std[DOCKAUV_MAX_U];
#pragma unroll
    for (int j = 0; j < DOCKAUV_MAX_U; ++j) {
        ls[j] = a.log_std[j < n_u ? j : n_u - 1];
        inv_std[j] = expf(-ls[j]);
    }
    const float nf = (float)a.n, lo = 1.0f - a.clip, hi = 1.0f + a.clip, two_vf = 2.0f * a.vf_coef;
    double acc[kHeadSums];
#pragma unroll
    for (int k = 0; k < kHeadSums; ++k) acc[k] = 0.0;

    // without a critic the two value loads read arrays of the same extent instead and their results are dropped
    const bool critic = a.v != nullptr;
    const float* ret_src = critic ? a.returns : a.advantages;
    const float* v_src = critic ? a.v : a.mean;
    const long passes = (a.n + kHeadPassRows - 1) / kHeadPassRows;
    for (long b = blockIdx.x; b < passes; b += gridDim.x) {
        long pos[kHeadChunk], at[kHeadChunk];
        float adv[kHeadChunk], lpo[kHeadChunk], ret[kHeadChunk], val[kHeadChunk], act[kHeadChunk][DOCKAUV_MAX_U], mu[kHeadChunk][DOCKAUV_MAX_U];
        float vold[kHeadChunk];
#pragma unroll
        for (int c = 0; c < kHeadChunk; ++c) {
            const long r = head_row_(b, c, tid);
            pos[c] = r < a.n ? r : a.n - 1;     // (behind the minibatch: its last row again, dropped below)
            at[c] = a.row_index ? (long)a.row_index[pos[c]] : pos[c];
        }
#pragma unroll
        for (int c = 0; c < kHeadChunk; ++c) {
            adv[c] = a.advantages[at[c]];
            lpo[c] = a.log_prob_old[at[c]];
            ret[c] = ret_src[at[c]];
            val[c] = v_src[pos[c]];
            if constexpr (Args::kClipVf) vold[c] = a.v_old[at[c]];
#pragma unroll
            for (int j = 0; j < DOCKAUV_MAX_U; ++j) {
                const int jc = j < n_u ? j : n_u - 1;   // (behind n_out: the last action again, dropped below)
                act[c][j] = a.actions[at[c] * n_u + jc];
                mu[c][j] = a.mean[pos[c] * n_u + jc];
            }
        }
#pragma unroll
        for (int c = 0; c < kHeadChunk; ++c) {
            if (head_row_(b, c, tid) >= a.n) continue;
            // include/dockauv.h (dockauv_ppo_head) states this order; -ffp-contract=on fuses nothing but the fmaf written here
            const float A = a.normalize ? (adv[c] - m) / den : adv[c];
            float z[DOCKAUV_MAX_U], lp0 = 0.0f, lp1 = 0.0f;
#pragma unroll
            for (int j = 0; j < DOCKAUV_MAX_U; ++j) {
                if (j < n_u) {
                    z[j] = (act[c][j] - mu[c][j]) * inv_std[j];
                    const float term = fmaf(-0.5f * z[j], z[j], -(ls[j] + kHalfLog2Pi));
                    if (j < 4) lp0 += term; else lp1 += term;
                }
            }
            const float lr = (lp0 + lp1) - lpo[c];
            const float ratio = expf(lr);
            const bool live = !((A > 0.0f && ratio > hi) || (A < 0.0f && ratio < lo));
            const float clamped = fminf(fmaxf(ratio, lo), hi);
            const float surrogate = fminf(ratio * A, clamped * A);
            const float g = live ? -(A * ratio) / nf : 0.0f;
            [[maybe_unused]] float vc = 0.0f;
            [[maybe_unused]] bool vlive = true;
            if constexpr (Args::kClipVf) {
                const float d = val[c] - vold[c];
                vc = vold[c] + fminf(fmaxf(d, -a.clip_vf), a.clip_vf);
                vlive = fabsf(d) <= a.clip_vf;      // (the inclusive edge: torch.clamp's backward)
            }
            const float dv = critic ? (Args::kClipVf ? vc : val[c]) - ret[c] : 0.0f;
            acc[0] += (double)surrogate;
            acc[1] += (double)(dv * dv);
            acc[2] += (double)((ratio - 1.0f) - lr);
            acc[3] += (double)(fabsf(ratio - 1.0f) > a.clip ? 1.0f : 0.0f);
            float* gm = a.grad_mean + pos[c] * n_u;
#pragma unroll
            for (int j = 0; j < DOCKAUV_MAX_U; ++j) {
                if (j < n_u) {
                    gm[j] = (g * z[j]) * inv_std[j];
                    acc[4 + j] += (double)(g * fmaf(z[j], z[j], -1.0f));
                }
            }
            if (critic) a.grad_v[pos[c]] = (Args::kClipVf && !vlive) ? 0.0f : (two_vf * dv) / nf;
        }
    }

#pragma unroll
    for (int k = 0; k < kHeadSums; ++k) {
        const double w = wave_sum_(acc[k]);
        if (lane == 0) red[wave][k] = w;
    }
    __syncthreads();
    if (tid < kHeadSums) a.partial[(long)blockIdx.x * kHeadSums + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// sum k = partial[0][k] + partial[1][k] + ... in group order, rounded to float32 once
// Args: HeadArgs, or HeadArgsGate (dockauv_ppo_update): thread 0 then decides whether the optimiser applies this minibatch
template <class Args>
__global__ __launch_bounds__(64) void ppo_head_final_kernel(const Args a, int groups) {
    __shared__ double total[kHeadSums];
    const int tid = threadIdx.x;
    if (tid < kHeadSums) {
        double s = 0.0;
        for (int g = 0; g < groups; ++g) s += a.partial[(long)g * kHeadSums + tid];
        total[tid] = s;
    }
    __syncthreads();
    if (tid < a.n_out) a.grad_log_std[tid] = (float)total[4 + tid] - a.ent_coef;
    if (tid == 0) {
        const double n = (double)a.n;
        const float policy_loss = (float)(-total[0] / n), value_loss = (float)(total[1] / n);
        float e = 0.0f;
        for (int j = 0; j < a.n_out; ++j) e += kEntropyConst + a.log_std[j];
        const float entropy_loss = -e;
        a.stats[0] = fmaf(a.vf_coef, value_loss, fmaf(a.ent_coef, entropy_loss, policy_loss));
        a.stats[1] = policy_loss;
        a.stats[2] = value_loss;
        a.stats[3] = entropy_loss;
        a.stats[4] = (float)(total[2] / n);
        a.stats[5] = (float)(total[3] / n);
        if constexpr (Args::kGate) {
            // SB3's rule on the stored statistic, in float32; once stopped, stopped for the rest of the call
            const float approx_kl = (float)(total[2] / n);
            const bool stop = a.ctl->stop != 0 || (a.target_kl > 0.0f && approx_kl > 1.5f * a.target_kl);
            float applied = 0.0f, step = 0.0f;
            if (stop) {
                a.ctl->stop = 1;
            } else {
                const long long t = a.ctl->t + 1;
                a.ctl->t = t;
                a.ctl->step_size = a.step_size;
                a.ctl->rsq = a.rsq;
                applied = 1.0f;
                step = (float)t;
            }
            a.stats[8] = 0.0f;      // (norm and coef: the optimiser's launch, when it applies the step)
            a.stats[9] = 0.0f;
            a.stats[10] = applied;
            a.stats[11] = step;
        }
    }
}

}  // namespace

int launch_ppo_head(const HeadArgs& a, void* stream) {
    if (a.n < 1 || (a.normalize && a.n < 2) || a.n_out < 1 || a.n_out > DOCKAUV_MAX_U) return (int)hipErrorInvalidValue;
    const long passes = (a.n + kHeadPassRows - 1) / kHeadPassRows;
    const unsigned groups = (unsigned)(passes < kBwdMaxGroups ? passes : kBwdMaxGroups);
    hipStream_t st = (hipStream_t)stream;
    if (a.normalize) hipLaunchKernelGGL(ppo_head_moments_kernel, dim3(groups), dim3(kHeadThreads), 0, st, a);
    hipLaunchKernelGGL(ppo_head_rows_kernel<HeadArgs>, dim3(groups), dim3(kHeadThreads), 0, st, a);
    hipLaunchKernelGGL(ppo_head_final_kernel<HeadArgs>, dim3(1), dim3(64), 0, st, a, (int)groups);
    return (int)hipGetLastError();
}

int launch_ppo_head_update(const HeadArgs& a, const HeadUpdate& u, void* stream) {
    if (a.n < 1 || (a.normalize && a.n < 2) || a.n_out < 1 || a.n_out > DOCKAUV_MAX_U || !u.ctl) return (int)hipErrorInvalidValue;
    if (u.clip_vf > 0.0f && (!u.v_old || !a.v)) return (int)hipErrorInvalidValue;
    const long passes = (a.n + kHeadPassRows - 1) / kHeadPassRows;
    const unsigned groups = (unsigned)(passes < kBwdMaxGroups ? passes : kBwdMaxGroups);
    hipStream_t st = (hipStream_t)stream;
    if (a.normalize) hipLaunchKernelGGL(ppo_head_moments_kernel, dim3(groups), dim3(kHeadThreads), 0, st, a);
    if (u.clip_vf > 0.0f) {
        HeadArgsVf x;
        static_cast<HeadArgs&>(x) = a;
        x.v_old = u.v_old;
        x.clip_vf = u.clip_vf;
        hipLaunchKernelGGL(ppo_head_rows_kernel<HeadArgsVf>, dim3(groups), dim3(kHeadThreads), 0, st, x);
    } else {
        hipLaunchKernelGGL(ppo_head_rows_kernel<HeadArgs>, dim3(groups), dim3(kHeadThreads), 0, st, a);
    }
    HeadArgsGate g;
    static_cast<HeadArgs&>(g) = a;
    g.ctl = u.ctl;
    g.target_kl = u.target_kl;
    g.step_size = u.step_size;
    g.rsq = u.rsq;
    hipLaunchKernelGGL(ppo_head_final_kernel<HeadArgsGate>, dim3(1), dim3(64), 0, st, g, (int)groups);
    return (int)hipGetLastError();
}

}  // namespace dockauv
