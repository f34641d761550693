// dockauv_sac.hip -- the gradient-free half of SAC for gfx950 (MI355X) on the tile body of dockauv_policy.hip (include/dockauv.h:
// dockauv_sac_actor_*, dockauv_q_*, dockauv_sac_target; the reference's counterpart is SB3 1.5's sac.policies.Actor /
// ContinuousCritic and the no_grad block of SAC.train, which train() runs with MODEL = SAC).
//
//   * the squashed-Gaussian actor: the output tile of 32 units carries BOTH heads -- W_mu in units 0 .. n_u - 1, W_ls in units
//     8 .. 8 + n_u - 1.  By the C/D layout of v_mfma_f32_32x32x2_f32 (unit_of_(r, half) = (r & 3) + 8 (r >> 2) + 4 half) the lane
//     that holds mu_j in register r (j = 4 half + r) holds log_std_j in register 4 + r: the second head costs no MFMA beyond the
//     output tile every actor already computes and no cross-lane traffic.  sac_actor_kernel (no log-probability: the rollout's
//     form keeps its registers, as policy_mlp_kernel does) and sac_actor_logp_kernel share sac_actor_tile_;
//   * the Q critic: the same body with a two-source layer-1 operand -- column k < n_obs from the observation row, k >= n_obs from
//     actions[k - n_obs], chosen per lane, so an odd n_obs straddles the two sources inside one k step;
//   * the TD target's last stage: one thread per row.
//   * sac_actor_heads_kernel (dockauv_sac_actor_forward_rows, the forward of the gradient half): the actor's tile body with mu and
//     the raw log_std written out, before clamp, noise and tanh.
// Rows come through an optional int64 index with a free row stride (as policy_rows_kernel takes them), so all of it runs on the
// replay ring as it stands.  Instantiated per (tiles of hidden layer 1, tiles of hidden layer 2) like the other MLP kernels.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dockauv.h"
#include "dockauv_device.h"
#include "dockauv_policy_tile.h"

namespace dockauv {
namespace {

struct SacArgs {
    PolicyShape S;                     // n_out: n_u (actor), 1 (Q)
    const float* packed;
    const float* rows;                 // observation rows, row_stride floats apart
    const long long* row_index;        // nullable [n]: slot i reads row row_index[i]
    const float* act_in;               // Q only: action rows, act_in_stride floats apart
    const long long* act_index;        // Q only, nullable [n]
    float* out;                        // actor: actions [n][out_stride]; Q: q [n]
    float* log_prob;                   // actor, logp form: [n]
    long n;
    int row_stride, out_stride, act_in_stride, n_obs, stochastic;
    unsigned int t_lo, row_off_lo, slot;   // the normal's counter: (row_off_lo + i, t_lo, j, slot)
    unsigned long long seed;
};

// one tile of 32 rows of the squashed-Gaussian actor (tile * 32 < a.n); the float32 expressions are the header's
template <int MT1, int MT2, bool LOGP>
__device__ __forceinline__ void sac_actor_tile_(const SacArgs& a, const float* lds, long tile) {
    const PolicyShape& S = a.S;
    const int lane = threadIdx.x & 63, half = lane >> 5;
    const long env = tile * 32 + (lane & 31);
    const bool live = env < a.n;                        // tail: rows >= n are neither read nor written
    long src = live ? env : 0;
    if (live && a.row_index) src = (long)a.row_index[env];
    const float* row = a.rows + src * (long)a.row_stride;

    f32x16 out[1];
    mlp_tile_<MT1, MT2>(S, lds, lane, half, [&](int k) { return (live && k < S.n_in) ? row[k] : 0.0f; }, out);

    // ---- mu_j in register r, log_std_j in register 4 + r, j = 4 half + r
    float* dst = a.out + (live ? env : 0) * (long)a.out_stride;
    [[maybe_unused]] float gauss = 0.0f, corr = 0.0f;   // this lane half's two sums, in the order of r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = 4 * half + r;
        if (j < S.n_out) {
            const float mu = out[0][r];
            const float ls = fminf(fmaxf(out[0][4 + r], -20.0f), 2.0f);
            float z = 0.0f, x = mu;
            if (a.stochastic) {
                z = policy_normal_(a.seed, a.row_off_lo + (uint32_t)env, a.t_lo, (uint32_t)j, a.slot);
                x = fmaf(expf(ls), z, mu);
            }
            const float v = tanh_(x);
            if (live) dst[j] = v;
            if constexpr (LOGP) {
                gauss += fmaf(-0.5f * z, z, -(ls + kHalfLog2Pi));
                // 1 - tanh(x)^2 = 4 e / (1 + e)^2 with e = exp(-2 |x|): no cancellation, no overflow
                const float e = expf(-2.0f * fabsf(x)), d = 1.0f + e;
                corr += logf(4.0f * e / (d * d) + 1e-6f);
            }
        }
    }
    if constexpr (LOGP) {
        // lanes l and l ^ 32 hold the two halves of one row (dockauv_policy.hip: policy_tile_)
        const float lp = gauss - corr;
        const unsigned int bits = __float_as_uint(lp);
        const auto sw = __builtin_amdgcn_permlane32_swap(bits, bits, false, false);
        const float total = lp + __uint_as_float(sw[1]);
        if (live && half == 0) a.log_prob[env] = total;
    }
}

template <int MT1, int MT2>
__global__ __launch_bounds__(kPolThreads) void sac_actor_kernel(const SacArgs a) {
    extern __shared__ float lds[];
    stage_weights_(a.packed, a.S.total, lds);
    const long tile = (long)blockIdx.x * (kPolThreads / 64) + (threadIdx.x >> 6);
    if (tile * 32 >= a.n) return;                       // (no barrier below)
    sac_actor_tile_<MT1, MT2, false>(a, lds, tile);
}

template <int MT1, int MT2>
__global__ __launch_bounds__(kPolThreads) void sac_actor_logp_kernel(const SacArgs a) {
    extern __shared__ float lds[];
    stage_weights_(a.packed, a.S.total, lds);
    const long tile = (long)blockIdx.x * (kPolThreads / 64) + (threadIdx.x >> 6);
    if (tile * 32 >= a.n) return;                       // (no barrier below)
    sac_actor_tile_<MT1, MT2, true>(a, lds, tile);
}

// both heads before the clamp, without noise and tanh (dockauv_sac_actor_forward_rows): the tile body above with another
// epilogue -- registers r (mu_j) and 4 + r (the raw log_std_j), j = 4 half + r, written out as out[row][j] and out[row][n_u + j]
template <int MT1, int MT2>
__global__ __launch_bounds__(kPolThreads) void sac_actor_heads_kernel(const SacArgs a) {
    extern __shared__ float lds[];
    stage_weights_(a.packed, a.S.total, lds);
    const long tile = (long)blockIdx.x * (kPolThreads / 64) + (threadIdx.x >> 6);
    if (tile * 32 >= a.n) return;                       // (no barrier below)
    const PolicyShape& S = a.S;
    const int lane = threadIdx.x & 63, half = lane >> 5;
    const long env = tile * 32 + (lane & 31);
    const bool live = env < a.n;                        // tail: rows >= n are neither read nor written
    long src = live ? env : 0;
    if (live && a.row_index) src = (long)a.row_index[env];
    const float* row = a.rows + src * (long)a.row_stride;
    f32x16 out[1];
    mlp_tile_<MT1, MT2>(S, lds, lane, half, [&](int k) { return (live && k < S.n_in) ? row[k] : 0.0f; }, out);
    float* dst = a.out + (live ? env : 0) * (long)a.out_stride;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = 4 * half + r;
        if (live && j < S.n_out) {
            dst[j] = out[0][r];
            dst[S.n_out + j] = out[0][4 + r];
        }
    }
}

// Q(obs, action) of any rows: layer-1 column k from the observation row (k < n_obs) or the action row (n_obs <= k < n_in)
template <int MT1, int MT2>
__global__ __launch_bounds__(kPolThreads) void q_kernel(const SacArgs a) {
    extern __shared__ float lds[];
    stage_weights_(a.packed, a.S.total, lds);
    const long tile = (long)blockIdx.x * (kPolThreads / 64) + (threadIdx.x >> 6);
    if (tile * 32 >= a.n) return;                       // (no barrier below)
    const PolicyShape& S = a.S;
    const int lane = threadIdx.x & 63, half = lane >> 5;
    const long env = tile * 32 + (lane & 31);
    const bool live = env < a.n;
    long src = live ? env : 0, asrc = src;
    if (live && a.row_index) src = (long)a.row_index[env];
    if (live && a.act_index) asrc = (long)a.act_index[env];
    const float* row = a.rows + src * (long)a.row_stride;
    const float* act = a.act_in + asrc * (long)a.act_in_stride - a.n_obs;   // (indexed with k >= n_obs only)
    f32x16 out[1];
    mlp_tile_<MT1, MT2>(S, lds, lane, half, [&](int k) { return (live && k < S.n_in) ? (k < a.n_obs ? row[k] : act[k]) : 0.0f; }, out);
    if (live && half == 0) a.out[env] = out[0][0];      // unit 0: register 0 of the lower lane half
}

struct TargetArgs {
    const float *rewards, *dones, *timeouts;   // timeouts nullable
    const long long* row_index;                // nullable
    const float *logp2, *q1, *q2;
    const float* log_ent_coef;                 // nullable device scalar
    float* y;
    long n;
    int column_stride;
    float gamma, ent_coef;
};

__global__ void sac_target_kernel(const TargetArgs a) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const long src = (a.row_index ? (long)a.row_index[i] : i) * (long)a.column_stride;
    const float alpha = a.log_ent_coef ? expf(*a.log_ent_coef) : a.ent_coef;
    const float r = a.rewards[src];
    float d = a.dones[src];
    if (a.timeouts) d = d * (1.0f - a.timeouts[src]);
    const float v = fmaf(-alpha, a.logp2[i], fminf(a.q1[i], a.q2[i]));
    a.y[i] = fmaf(a.gamma * (1.0f - d), v, r);
}

enum SacKernel { SAC_ACTOR, SAC_ACTOR_LOGP, SAC_Q, SAC_HEADS };

template <int MT1, int MT2>
int launch_sac_(const SacArgs& a, int which, size_t lds, hipStream_t stream) {
    const long tiles = ((long)a.n + 31) / 32;
    const long groups = (tiles + kPolThreads / 64 - 1) / (kPolThreads / 64);
    void (*kernel)(const SacArgs) = which == SAC_Q ? q_kernel<MT1, MT2>
                                    : (which == SAC_HEADS ? sac_actor_heads_kernel<MT1, MT2>
                                       : (which == SAC_ACTOR_LOGP ? sac_actor_logp_kernel<MT1, MT2> : sac_actor_kernel<MT1, MT2>));
    if (groups > 0x7fffffffL) return (int)hipErrorInvalidValue;
    if (lds > 64 * 1024) {
        // more than 64 KiB of LDS per group must be requested explicitly, per (device, function): on the launch path
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(kPolThreads), lds, stream, a);
    return (int)hipGetLastError();
}

template <int MT1>
int launch_sac_mt1_(const SacArgs& a, int which, size_t lds, hipStream_t stream) {
    switch (a.S.mt2) {
        case 0: return launch_sac_<MT1, 0>(a, which, lds, stream);
        case 1: return launch_sac_<MT1, 1>(a, which, lds, stream);
        case 2: return launch_sac_<MT1, 2>(a, which, lds, stream);
        case 3: return launch_sac_<MT1, 3>(a, which, lds, stream);
        case 4: return launch_sac_<MT1, 4>(a, which, lds, stream);
    }
    return (int)hipErrorInvalidValue;
}

int launch_sac_any_(const SacArgs& a, int which, hipStream_t stream) {
    const size_t lds = policy_lds_bytes(a.S);
    if (a.n <= 0 || lds > kPolMaxLds) return (int)hipErrorInvalidValue;
    switch (a.S.mt1) {
        case 1: return launch_sac_mt1_<1>(a, which, lds, stream);
        case 2: return launch_sac_mt1_<2>(a, which, lds, stream);
        case 3: return launch_sac_mt1_<3>(a, which, lds, stream);
        case 4: return launch_sac_mt1_<4>(a, which, lds, stream);
    }
    return (int)hipErrorInvalidValue;
}

}  // namespace

int launch_sac_actor(const PolicyShape& s, const float* packed, const SacActorLaunch& l, void* stream) {
    SacArgs a{};
    a.S = s;
    a.packed = packed;
    a.rows = l.rows;
    a.row_index = l.row_index;
    a.out = l.actions;
    a.log_prob = l.log_prob;
    a.n = l.n;
    a.row_stride = l.row_stride;
    a.out_stride = l.act_stride;
    a.stochastic = l.stochastic ? 1 : 0;
    a.t_lo = (unsigned int)(l.t & 0xffffffffull);
    a.row_off_lo = (unsigned int)(l.row_offset & 0xffffffffull);
    a.slot = l.slot;
    a.seed = l.seed;
    return launch_sac_any_(a, l.log_prob ? SAC_ACTOR_LOGP : SAC_ACTOR, (hipStream_t)stream);
}

int launch_sac_actor_heads(const PolicyShape& s, const float* packed, const float* rows, const long long* row_index, long n,
                           int row_stride, float* out, void* stream) {
    SacArgs a{};
    a.S = s;
    a.packed = packed;
    a.rows = rows;
    a.row_index = row_index;
    a.out = out;
    a.n = n;
    a.row_stride = row_stride;
    a.out_stride = 2 * s.n_out;
    return launch_sac_any_(a, SAC_HEADS, (hipStream_t)stream);
}

int launch_q_forward(const PolicyShape& s, const float* packed, const QLaunch& l, void* stream) {
    SacArgs a{};
    a.S = s;
    a.packed = packed;
    a.rows = l.obs;
    a.row_index = l.obs_index;
    a.act_in = l.actions;
    a.act_index = l.act_index;
    a.out = l.q;
    a.n = l.n;
    a.row_stride = l.obs_stride;
    a.act_in_stride = l.act_stride;
    a.n_obs = l.n_obs;
    if (l.n_obs < 1 || l.n_obs >= s.n_in) return (int)hipErrorInvalidValue;
    return launch_sac_any_(a, SAC_Q, (hipStream_t)stream);
}

int launch_sac_target_rows(const SacTargetLaunch& l, void* stream) {
    if (l.n <= 0) return (int)hipErrorInvalidValue;
    TargetArgs a{l.rewards, l.dones, l.timeouts, l.row_index, l.logp2, l.q1, l.q2, l.log_ent_coef, l.y, l.n, l.column_stride, l.gamma, l.ent_coef};
    const long groups = (l.n + 255) / 256;
    if (groups > 0x7fffffffL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sac_target_kernel, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace dockauv
