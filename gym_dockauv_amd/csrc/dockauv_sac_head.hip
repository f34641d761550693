// dockauv_sac_head.hip -- SAC's loss head for gfx950 (MI355X): everything of SAC.train between the networks' forward calls and their
// backward calls, and the learned entropy coefficient (include/dockauv.h: dockauv_sac_sample, dockauv_sac_critic_head,
// dockauv_sac_actor_head, dockauv_sac_ent_coef_step state every float32 expression; the reference's counterpart is SB3 1.5's
// SAC.train, which train() runs with MODEL = SAC).
//
//   sac_sample_kernel       one thread a row of `heads` (mu | raw log-std, what dockauv_sac_actor_forward_rows writes): the epilogue of
//                           sac_actor_tile_<.., true> (dockauv_sac.hip) with stochastic != 0 as an elementwise kernel -- the same
//                           expressions in the same order, so the bits of dockauv_sac_target's a2 and logp2 on the same rows.
//   sac_critic_head_kernel  d(0.5 (mse1 + mse2)) / dq of both critics and the statistics.
//   sac_actor_head_kernel   the draw again (sac_action_: the same function, the same bits), the gradient of mean(alpha logp - min q) on
//                           (mu | raw log-std) with the clamp's mask applied, and the statistics.
//   ent_coef_step_kernel    the mean of logp + target_entropy and one Adam step on the scalar log_ent_coef.
// The three kernels with sums are ONE group of kSacHeadThreads lanes each and need no workspace: a SAC minibatch is a few hundred
// to a few thousand rows, the kernels are bound by the latency of one launch and of one dependent load, and a second launch for
// the groups' partial sums would double the first.  The sums run in the optimiser's order (dockauv_optim.hip): lane t takes the
// rows t, t + 1 024, .., in float64; the lanes of a wave are added by a fixed shuffle tree, the sixteen waves in order.  No
// floating-point atomics: every bit is a function of the inputs, a row's position in the minibatch, n_rows and n_u.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dockauv.h"
#include "dockauv_device.h"
#include "dockauv_policy_tile.h"

namespace dockauv {
namespace {

// lane 0 gets the sum over the 64 lanes, added in the order of this tree (dockauv_head.hip)
__device__ __forceinline__ double wave_sum_(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// sum k of the group, k < K, the same bits in every thread: the lanes of a wave by the tree, the waves in order
template <int K>
__device__ __forceinline__ void group_sums_(double (&acc)[K], double (*red)[K]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double w = wave_sum_(acc[k]);
        if (lane == 0) red[wave][k] = w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kSacHeadThreads / 64; ++w) s += red[w][k];
        acc[k] = s;
    }
}

// One action of the squashed-Gaussian actor's sample from its two heads: a = tanh(x), s = 1 - tanh(x)^2, sz = std z, and the two
// terms of the log-probability, g (Gaussian) and c (squashing correction).  The float32 expressions are sac_actor_tile_'s, written
// as they are written there (-ffp-contract=on fuses nothing but the fmaf in the source).
struct SacAction {
    float a, s, sz, g, c;
};
__device__ __forceinline__ SacAction sac_action_(float mu, float raw, float z) {
    SacAction o;
    const float ls = fminf(fmaxf(raw, -20.0f), 2.0f);
    const float sd = expf(ls);
    const float x = fmaf(sd, z, mu);
    o.a = tanh_(x);
    o.sz = sd * z;
    o.g = fmaf(-0.5f * z, z, -(ls + kHalfLog2Pi));
    // 1 - tanh(x)^2 = 4 e / (1 + e)^2 with e = exp(-2 |x|): no cancellation, no overflow
    const float e = expf(-2.0f * fabsf(x)), d = 1.0f + e;
    o.s = 4.0f * e / (d * d);
    o.c = logf(o.s + 1e-6f);
    return o;
}

// The log-probability's four sums, from 0.0f in the order of j: lo over j = 0..3, hi over 4..7 -- what the two lane halves of the
// tile kernel hold -- and logp = (G_lo - C_lo) + (G_hi - C_hi)
struct SacLogp {
    float gauss_lo = 0.0f, corr_lo = 0.0f, gauss_hi = 0.0f, corr_hi = 0.0f;
    __device__ __forceinline__ void add(int j, const SacAction& o) {
        if (j < 4) {
            gauss_lo += o.g;
            corr_lo += o.c;
        } else {
            gauss_hi += o.g;
            corr_hi += o.c;
        }
    }
    __device__ __forceinline__ float total() const {
        const float lp_lo = gauss_lo - corr_lo, lp_hi = gauss_hi - corr_hi;
        return lp_lo + lp_hi;
    }
};

__global__ __launch_bounds__(kSacSampleThreads) void sac_sample_kernel(const SacSampleLaunch a) {
    const long i = (long)blockIdx.x * kSacSampleThreads + threadIdx.x;
    if (i >= a.n) return;
    const int n_u = a.n_u;
    const float* h = a.heads + i * (2 * n_u);
    float* dst = a.a + i * n_u;
    SacLogp lp;
#pragma unroll
    for (int j = 0; j < DOCKAUV_MAX_U; ++j) {
        if (j < n_u) {
            const float z = policy_normal_(a.seed, a.row_off_lo + (uint32_t)i, a.t_lo, (uint32_t)j, 5u);
            const SacAction o = sac_action_(h[j], h[n_u + j], z);
            dst[j] = o.a;
            lp.add(j, o);
        }
    }
    a.logp[i] = lp.total();
}

__global__ __launch_bounds__(kSacHeadThreads) void sac_critic_head_kernel(const SacCriticHeadLaunch a) {
    __shared__ double red[kSacHeadThreads / 64][5];
    const float nf = (float)a.n;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long i = threadIdx.x; i < a.n; i += kSacHeadThreads) {
        const float q1 = a.q1[i], q2 = a.q2[i], y = a.y[i];
        const float d1 = q1 - y, d2 = q2 - y;
        a.grad_q1[i] = d1 / nf;
        a.grad_q2[i] = d2 / nf;
        acc[0] += (double)(d1 * d1);
        acc[1] += (double)(d2 * d2);
        acc[2] += (double)q1;
        acc[3] += (double)q2;
        acc[4] += (double)y;
    }
    group_sums_<5>(acc, red);
    if (threadIdx.x == 0) {
        const double n = (double)a.n;
        const float mse1 = (float)(acc[0] / n), mse2 = (float)(acc[1] / n);
        a.stats[0] = 0.5f * (mse1 + mse2);
        a.stats[1] = mse1;
        a.stats[2] = mse2;
        a.stats[3] = (float)(acc[2] / n);
        a.stats[4] = (float)(acc[3] / n);
        a.stats[5] = (float)(acc[4] / n);
    }
}

__global__ __launch_bounds__(kSacHeadThreads) void sac_actor_head_kernel(const SacActorHeadLaunch a) {
    __shared__ double red[kSacHeadThreads / 64][3];
    const int n_u = a.n_u;
    const float nf = (float)a.n;
    const float alpha = a.log_ent_coef ? expf(*a.log_ent_coef) : a.ent_coef;
    const float alpha_n = alpha / nf;
    double acc[3] = {0.0, 0.0, 0.0};
    for (long i = threadIdx.x; i < a.n; i += kSacHeadThreads) {
        const float* h = a.heads + i * (2 * n_u);
        const float q1 = a.q1_pi[i], q2 = a.q2_pi[i];
        const float* dq = (q1 <= q2 ? a.dq1 : a.dq2) + i * n_u;   // torch.min's gradient; a tie goes to critic 1
        float* g = a.grad_out + i * (2 * n_u);
        SacLogp sums;
#pragma unroll 1
        for (int j = 0; j < n_u; ++j) {
            const float raw = h[n_u + j];
            const float z = policy_normal_(a.seed, a.row_off_lo + (uint32_t)i, a.t_lo, (uint32_t)j, 5u);
            const SacAction o = sac_action_(h[j], raw, z);
            sums.add(j, o);
            // include/dockauv.h (dockauv_sac_actor_head) states this order
            const float w = (2.0f * o.a) * (o.s / (o.s + 1e-6f));
            const float sel = dq[j];
            const float gx = fmaf(alpha, w, -(sel * o.s)) / nf;
            const bool inside = raw >= -20.0f && raw <= 2.0f;   // torch.clamp's backward: both edges included
            g[j] = gx;
            g[n_u + j] = inside ? fmaf(gx, o.sz, -alpha_n) : 0.0f;
        }
        const float lp = sums.total();
        const float mq = fminf(q1, q2);
        acc[0] += (double)fmaf(alpha, lp, -mq);
        acc[1] += (double)lp;
        acc[2] += (double)mq;
    }
    group_sums_<3>(acc, red);
    if (threadIdx.x == 0) {
        const double n = (double)a.n;
        a.stats[0] = (float)(acc[0] / n);
        a.stats[1] = (float)(acc[1] / n);
        a.stats[2] = (float)(acc[2] / n);
        a.stats[3] = alpha;
    }
}

__global__ __launch_bounds__(kSacHeadThreads) void ent_coef_step_kernel(const EntCoefLaunch a) {
    __shared__ double red[kSacHeadThreads / 64][1];
    double acc[1] = {0.0};
    for (long i = threadIdx.x; i < a.n; i += kSacHeadThreads) acc[0] += (double)(a.logp[i] + a.target_entropy);
    group_sums_<1>(acc, red);
    if (threadIdx.x == 0) {
        // include/dockauv.h (dockauv_sac_ent_coef_step) states this order: dockauv_optim_step's on one element, no clipping
        const float p = a.state[0];
        float m = a.state[1], v = a.state[2];
        const float mean = (float)(acc[0] / (double)a.n);
        const float g = -mean;
        m = fmaf(a.c1, g - m, m);
        const float bv = a.b2 * v;
        v = fmaf(a.c2 * g, g, bv);
        const float denom = fmaf(sqrtf(v), a.rsq, a.eps);
        const float upd = a.step_size * (m / denom);
        const float p_new = p - upd;
        a.state[0] = p_new;
        a.state[1] = m;
        a.state[2] = v;
        if (a.before) *a.before = p;
        if (a.stats) {
            a.stats[0] = -(p * mean);
            a.stats[1] = expf(p);
            a.stats[2] = mean;
            a.stats[3] = p_new;
        }
    }
}

}  // namespace

int launch_sac_sample(const SacSampleLaunch& a, void* stream) {
    if (a.n < 1 || a.n_u < 1 || a.n_u > DOCKAUV_MAX_U) return (int)hipErrorInvalidValue;
    const long groups = (a.n + kSacSampleThreads - 1) / kSacSampleThreads;
    if (groups > 0x7fffffffL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sac_sample_kernel, dim3((unsigned)groups), dim3(kSacSampleThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_sac_critic_head(const SacCriticHeadLaunch& a, void* stream) {
    if (a.n < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sac_critic_head_kernel, dim3(1), dim3(kSacHeadThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_sac_actor_head(const SacActorHeadLaunch& a, void* stream) {
    if (a.n < 1 || a.n_u < 1 || a.n_u > DOCKAUV_MAX_U) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sac_actor_head_kernel, dim3(1), dim3(kSacHeadThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_ent_coef_step(const EntCoefLaunch& a, void* stream) {
    if (a.n < 1 || !a.state || !a.logp) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(ent_coef_step_kernel, dim3(1), dim3(kSacHeadThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace dockauv
