// dockauv_policy_tile.h -- the __device__ pieces the MLP kernels share (dockauv_policy.hip: the plain actor and the critic;
// dockauv_sac.hip: the squashed-Gaussian actor and the Q critics): activations, the exploration normal, and one tile of 32
// rows through all layers on v_mfma_f32_32x32x2_f32 (dockauv_device.h: PolicyShape states the packed layout).  Internal to
// libdockauv.so; device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dockauv_device.h"

namespace dockauv {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// tanh(x) = 1 - 2 / (exp(2 x) + 1): v_exp_f32 and v_rcp_f32 are good to 1 ulp, the form has no cancellation beyond the final
// subtraction, so the absolute error stays below ~3e-7 everywhere (+-1 at the ends, exactly 0 at 0: padded units stay 0).
__device__ __forceinline__ float tanh_(float x) {
    const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);   // exp(2 x)
    return fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
}

__device__ __forceinline__ float act_(float x, int kind) {
    if (kind == DOCKAUV_ACT_TANH) return tanh_(x);
    if (kind == DOCKAUV_ACT_RELU) return fmaxf(x, 0.0f);
    return x;
}

// standard normal of Philox counter (env, t, j, slot): Box-Muller cos branch on the first two words, u1 / u2 as the current
// noise of the step kernel draws them (oracle/philox_ref.py: philox_normal).  u1 is formed in float32: the + 0.5 is held while
// c[0] >> 8 < 2^23 and rounded to even above, so u1 lies in (0, 1] -- the log is finite, and the top value gives z = 0.
// slot: 2 for the per-env actors, 5 for the rows form of the squashed-Gaussian actor (dockauv_device.h lists the slots).
__device__ __forceinline__ float policy_normal_(unsigned long long seed, uint32_t env, uint32_t t, uint32_t j, uint32_t slot = 2u) {
    uint32_t c[4] = {env, t, j, slot};
    philox4x32_10_(c, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
    const float u1 = ((float)(c[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = (float)(c[1] >> 8) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);                   // cos(2 pi u2), argument reduction exact
}

template <int MT>
__device__ __forceinline__ void load_bias_(f32x16 (&acc)[MT], const float* lds_b, int half) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = lds_b[(m * 16 + r) * 2 + half];
}

template <int MT>
__device__ __forceinline__ void activate_(f32x16 (&acc)[MT], int kind) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = act_(acc[m][r], kind);
}

// out[mo] += W[.. , k] h[k] over the units the accumulators `in` hold: k step (mi, r) takes register r of tile mi as it stands
template <int MI, int MO>
__device__ __forceinline__ void dense_(f32x16 (&out)[MO], const f32x16 (&in)[MI], const float* lds_w, int lane) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int mo = 0; mo < MO; ++mo)
                out[mo] = __builtin_amdgcn_mfma_f32_32x32x2f32(lds_w[((mi * 16 + r) * MO + mo) * 64 + lane], in[mi][r], out[mo], 0, 0, 0);
}

constexpr float kHalfLog2Pi = 0.91893853320467274f;   // log(2 pi) / 2
constexpr int kChunk = 16;   // layer-1 k steps whose row words are requested together

// the packed weights -> LDS, all threads of the group; the barrier behind it is the kernel's only one
__device__ __forceinline__ void stage_weights_(const float* packed, int total, float* lds) {
    const float4* src = reinterpret_cast<const float4*>(packed);
    float4* dst = reinterpret_cast<float4*>(lds);
    for (int i = threadIdx.x; i < total / 4; i += kPolThreads) dst[i] = src[i];
    __syncthreads();
}

// unit of accumulator register r in lane half `half` of a tile (C/D layout of v_mfma_f32_32x32x2_f32)
__device__ __forceinline__ int unit_of_(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// one tile of 32 rows through all layers, by one wave: out[0] <- the output tile before any output activation.  x(k) is the
// layer-1 input column k of this lane's row (0 for k >= n_in and for rows past the end); every pre-activation is one
// accumulator chain from the bias whose k order the shape alone fixes
template <int MT1, int MT2, class X>
__device__ __forceinline__ void mlp_tile_(const PolicyShape& S, const float* lds, int lane, int half, X x_of, f32x16 (&out)[1]) {
    // ---- layer 1
    f32x16 h1[MT1];
    load_bias_<MT1>(h1, lds + S.off_b1, half);
    for (int s0 = 0; s0 < S.ks1; s0 += kChunk) {
        float x[kChunk];
#pragma unroll
        for (int j = 0; j < kChunk; ++j) x[j] = x_of(2 * (s0 + j) + half);
#pragma unroll
        for (int j = 0; j < kChunk; ++j) {
            if (s0 + j < S.ks1) {
#pragma unroll
                for (int m = 0; m < MT1; ++m)
                    h1[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(lds[S.off_w1 + ((s0 + j) * MT1 + m) * 64 + lane], x[j], h1[m], 0, 0, 0);
            }
        }
    }
    activate_<MT1>(h1, S.hidden_act);

    // ---- hidden layer 2 (if any) and the output layer
    load_bias_<1>(out, lds + S.off_b3, half);
    if constexpr (MT2 > 0) {
        f32x16 h2[MT2];
        load_bias_<MT2>(h2, lds + S.off_b2, half);
        dense_<MT1, MT2>(h2, h1, lds + S.off_w2, lane);
        activate_<MT2>(h2, S.hidden_act);
        dense_<MT2, 1>(out, h2, lds + S.off_w3, lane);
    } else {
        dense_<MT1, 1>(out, h1, lds + S.off_w3, lane);
    }
}

}  // namespace dockauv
