// dockauv_policy.hip -- the library's own MLP actor for gfx950 (MI355X): the policy of a closed loop evaluated on the packed
// rows the step kernel writes (include/dockauv.h: dockauv_policy_*, dockauv_rollout; the reference's counterpart is SB3's
// MlpPolicy, train.py:64, queried per step in train.py:64-71, 86-119).
//
// One launch = a[i] = out_act(W3 act(W2 act(W1 obs[i] + b1) + b2) + b3) for every env row i, exact float32.
//
// Work decomposition: the TRANSPOSED product on v_mfma_f32_32x32x2_f32 -- units on the M side, envs on the N side.  A wave
// owns 32 consecutive envs (column = lane & 31) and walks them through all layers; a workgroup is four such waves and stages
// the packed weights (dockauv_device.h: PolicyShape) into LDS once.
//   * layer 1: the B operand of k step s is obs[env][2 s + (lane >> 5)], read straight from the row (only columns < n_in
//     are ever touched: the reward / done columns never enter a product, and rows >= n are never read); the A operand is
//     one LDS word per lane;
//   * the C/D layout of the instruction holds unit 32 m + (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the wave's env column in
//     register r of tile m: after the activation that register IS the B operand of one k step of the next layer, whose
//     weight columns were permuted to match when they were packed -- no transpose, no LDS traffic for activations;
//   * every pre-activation is one accumulator chain that starts from the bias and takes its k steps in an order fixed by
//     the shape alone: an env's action depends on its row and the weights, not on n, its position or the grid;
//   * the actions (<= 8) of an env sit in registers 0..3 of the two lane halves; exploration noise, output activation and
//     the store happen there; so does the log-probability of the drawn actions (launch_policy_forward: log_prob), summed per
//     lane half and exchanged once between the halves.
// policy_mlp_kernel and policy_logp_kernel (the same with the log-probability epilogue) share the tile body.  The value launch
// (dockauv_value_forward, any number of rows) is policy_mlp_kernel with one output unit.  A resident grid whose waves loop over
// the tiles -- the weights staged once per resident group, not once per 128 rows -- was built and measured for it: not reliably
// faster (profiles/collect/tile_loop_experiment.txt), so it is not here.
// Instantiated per (tiles of hidden layer 1, tiles of hidden layer 2) so that every accumulator index is a constant.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dockauv.h"
#include "dockauv_device.h"
#include "dockauv_policy_tile.h"

namespace dockauv {
namespace {

struct PolicyArgs {
    PolicyShape S;
    const float* packed;
    const float* rows;
    const long long* row_index;        // ROWS kernels only, nullable [n]: env slot i reads row row_index[i]
    float* actions;
    float* log_prob;                   // nullable [n]: sum_j (-z_ij^2 / 2 - log_std[j] - log(2 pi) / 2)
    const float* log_std;              // [n_out] raw log_std (read with log_prob only; the LDS image keeps exp(log_std))
    long n;
    int row_stride, act_stride, stochastic;
    unsigned int t_lo;                 // t mod 2^32
    unsigned int env_off_lo;           // env_id_offset mod 2^32 (the counter word is 32 bits wide)
    unsigned long long seed;
};

// one tile of 32 envs through all layers, by one wave (tile * 32 < a.n); LOGP: also a.log_prob; ROWS: the row of slot i is
// a.row_index[i] when an index is given (dockauv_policy_forward_rows) -- the arithmetic is the same instruction sequence
template <int MT1, int MT2, bool LOGP, bool ROWS = false>
__device__ __forceinline__ void policy_tile_(const PolicyArgs& a, const float* lds, long tile) {
    const PolicyShape& S = a.S;
    const int lane = threadIdx.x & 63, half = lane >> 5;
    const long env = tile * 32 + (lane & 31);
    const bool live = env < a.n;                        // tail: rows >= n are neither read nor written
    long src = live ? env : 0;
    if constexpr (ROWS) {
        if (live && a.row_index) src = (long)a.row_index[env];
    }
    const float* row = a.rows + src * (long)a.row_stride;

    // ---- layer 1
    f32x16 h1[MT1];
    load_bias_<MT1>(h1, lds + S.off_b1, half);
    for (int s0 = 0; s0 < S.ks1; s0 += kChunk) {
        float x[kChunk];
#pragma unroll
        for (int j = 0; j < kChunk; ++j) {
            const int k = 2 * (s0 + j) + half;
            x[j] = (live && k < S.n_in) ? row[k] : 0.0f;
        }
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
    f32x16 out[1];
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

    // ---- actions: unit j = 4 half + r sits in register r < 4
    float* dst = a.actions + (live ? env : 0) * (long)a.act_stride;
    [[maybe_unused]] float lp = 0.0f;                   // this lane half's part of the log-probability, in the order of r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = 4 * half + r;
        if (j < S.n_out) {
            float v = out[0][r];
            float z = 0.0f;
            if (a.stochastic) {
                z = policy_normal_(a.seed, a.env_off_lo + (uint32_t)env, a.t_lo, (uint32_t)j);
                v = fmaf(lds[S.off_std + j], z, v);
            }
            v = act_(v, S.out_act);
            if (live) dst[j] = v;
            if constexpr (LOGP) lp += fmaf(-0.5f * z, z, -(a.log_std[j] + kHalfLog2Pi));
        }
    }
    if constexpr (LOGP) {
        // lanes l and l ^ 32 hold the two halves of one env: v_permlane32_swap hands lanes 0..31 (second result) what lanes
        // 32..63 hold; the lower lane adds (actions 0..3) + (actions 4..7) and stores
        const unsigned int bits = __float_as_uint(lp);
        const auto sw = __builtin_amdgcn_permlane32_swap(bits, bits, false, false);
        const float total = lp + __uint_as_float(sw[1]);
        if (live && half == 0) a.log_prob[env] = total;
    }
}

template <int MT1, int MT2>
__global__ __launch_bounds__(kPolThreads) void policy_mlp_kernel(const PolicyArgs a) {
    extern __shared__ float lds[];
    stage_weights_(a.packed, a.S.total, lds);
    const long tile = (long)blockIdx.x * (kPolThreads / 64) + (threadIdx.x >> 6);
    if (tile * 32 >= a.n) return;                       // (no barrier below)
    policy_tile_<MT1, MT2, false>(a, lds, tile);
}

// the same with the log-probability epilogue (dockauv_policy_forward_logp): a kernel of its own, so that the plain actor
// keeps its registers (the epilogue costs <3, 3> its fourth wave per SIMD)
template <int MT1, int MT2>
__global__ __launch_bounds__(kPolThreads) void policy_logp_kernel(const PolicyArgs a) {
    extern __shared__ float lds[];
    stage_weights_(a.packed, a.S.total, lds);
    const long tile = (long)blockIdx.x * (kPolThreads / 64) + (threadIdx.x >> 6);
    if (tile * 32 >= a.n) return;                       // (no barrier below)
    policy_tile_<MT1, MT2, true>(a, lds, tile);
}

// the pre-activation output of any rows, dense or through an index (dockauv_policy_forward_rows)
template <int MT1, int MT2>
__global__ __launch_bounds__(kPolThreads) void policy_rows_kernel(const PolicyArgs a) {
    extern __shared__ float lds[];
    stage_weights_(a.packed, a.S.total, lds);
    const long tile = (long)blockIdx.x * (kPolThreads / 64) + (threadIdx.x >> 6);
    if (tile * 32 >= a.n) return;                       // (no barrier below)
    policy_tile_<MT1, MT2, false, true>(a, lds, tile);
}

struct PackArgs {
    PolicyShape S;
    PolicyRaw raw;
    float* packed;
};

__global__ void policy_pack_kernel(const PackArgs a) {
    const PolicyShape& S = a.S;
    const int n_last = S.n_h2 ? S.n_h2 : S.n_h1;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < S.total; idx += gridDim.x * blockDim.x) {
        float v = 0.0f;
        if (idx < S.off_w2) {
            const int loc = idx - S.off_w1, l = loc & 63, t = loc >> 6;
            const int m = t % S.mt1, s = t / S.mt1;
            const int unit = 32 * m + (l & 31), k = 2 * s + (l >> 5);
            if (unit < S.n_h1 && k < S.n_in) v = a.raw.W1[(long)unit * S.n_in + k];
        } else if (idx < S.off_w3) {
            const int loc = idx - S.off_w2, l = loc & 63, t = loc >> 6;
            const int m = t % S.mt2, sr = t / S.mt2;
            const int unit = 32 * m + (l & 31), k = 32 * (sr >> 4) + unit_of_(sr & 15, l >> 5);
            if (unit < S.n_h2 && k < S.n_h1) v = a.raw.W2[(long)unit * S.n_h1 + k];
        } else if (idx < S.off_b1) {
            const int loc = idx - S.off_w3, l = loc & 63, sr = loc >> 6;
            const int unit = l & 31, k = 32 * (sr >> 4) + unit_of_(sr & 15, l >> 5);
            if (unit < S.n_out && k < n_last) v = a.raw.W3[(long)unit * n_last + k];
        } else if (idx < S.off_std) {
            const float* b = idx < S.off_b2 ? a.raw.b1 : (idx < S.off_b3 ? a.raw.b2 : a.raw.b3);
            const int n_units = idx < S.off_b2 ? S.n_h1 : (idx < S.off_b3 ? S.n_h2 : S.n_out);
            const int loc = idx - (idx < S.off_b2 ? S.off_b1 : (idx < S.off_b3 ? S.off_b2 : S.off_b3));
            const int unit = 32 * (loc >> 5) + unit_of_((loc >> 1) & 15, loc & 1);
            if (unit < n_units) v = b[unit];
        } else {
            const int j = idx - S.off_std;
            if (a.raw.log_std && j < S.n_out) v = expf(a.raw.log_std[j]);
        }
        a.packed[idx] = v;
    }
}

template <int MT1, int MT2, bool ROWS>
int launch_forward_(const PolicyArgs& a, size_t lds, hipStream_t stream) {
    const long tiles = ((long)a.n + 31) / 32;
    const long groups = (tiles + kPolThreads / 64 - 1) / (kPolThreads / 64);
    void (*kernel)(const PolicyArgs) = ROWS ? policy_rows_kernel<MT1, MT2> : (a.log_prob ? policy_logp_kernel<MT1, MT2> : policy_mlp_kernel<MT1, MT2>);
    if (groups > 0x7fffffffL) return (int)hipErrorInvalidValue;
    if (lds > 64 * 1024) {
        // more than 64 KiB of LDS per group must be requested explicitly; the attribute belongs to the (device, function)
        // pair: set on the launch path, as the step kernels do
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(kPolThreads), lds, stream, a);
    return (int)hipGetLastError();
}

template <int MT1, bool ROWS>
int launch_forward_mt1_(const PolicyArgs& a, size_t lds, hipStream_t stream) {
    switch (a.S.mt2) {
        case 0: return launch_forward_<MT1, 0, ROWS>(a, lds, stream);
        case 1: return launch_forward_<MT1, 1, ROWS>(a, lds, stream);
        case 2: return launch_forward_<MT1, 2, ROWS>(a, lds, stream);
        case 3: return launch_forward_<MT1, 3, ROWS>(a, lds, stream);
        case 4: return launch_forward_<MT1, 4, ROWS>(a, lds, stream);
    }
    return (int)hipErrorInvalidValue;
}

template <bool ROWS>
int launch_forward_any_(const PolicyArgs& a, size_t lds, hipStream_t stream) {
    switch (a.S.mt1) {
        case 1: return launch_forward_mt1_<1, ROWS>(a, lds, stream);
        case 2: return launch_forward_mt1_<2, ROWS>(a, lds, stream);
        case 3: return launch_forward_mt1_<3, ROWS>(a, lds, stream);
        case 4: return launch_forward_mt1_<4, ROWS>(a, lds, stream);
    }
    return (int)hipErrorInvalidValue;
}

}  // namespace

int launch_policy_pack(const PolicyShape& s, const PolicyRaw& raw, float* packed, void* stream) {
    PackArgs a{s, raw, packed};
    hipLaunchKernelGGL(policy_pack_kernel, dim3((unsigned)((s.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_policy_forward(const PolicyShape& s, const float* packed, const float* rows, float* actions, long n, int row_stride,
                          int act_stride, unsigned long long t, int stochastic, unsigned long long seed,
                          unsigned long long env_id_offset, void* stream, float* log_prob, const float* log_std) {
    PolicyArgs a;
    a.S = s;
    a.packed = packed;
    a.rows = rows;
    a.row_index = nullptr;
    a.actions = actions;
    a.log_prob = log_prob;
    a.log_std = log_std;
    a.n = n;
    a.row_stride = row_stride;
    a.act_stride = act_stride;
    a.stochastic = stochastic ? 1 : 0;
    a.t_lo = (unsigned int)(t & 0xffffffffull);
    a.env_off_lo = (unsigned int)(env_id_offset & 0xffffffffull);
    a.seed = seed;
    const size_t lds = policy_lds_bytes(s);
    if (n <= 0 || lds > kPolMaxLds || (log_prob && !log_std)) return (int)hipErrorInvalidValue;
    return launch_forward_any_<false>(a, lds, (hipStream_t)stream);
}

int launch_policy_forward_rows(const PolicyShape& s, const float* packed, const float* rows, const long long* row_index, long n,
                               int row_stride, float* out, void* stream) {
    PolicyArgs a{};
    a.S = s;
    a.S.out_act = DOCKAUV_ACT_NONE;                     // the output before out_act
    a.packed = packed;
    a.rows = rows;
    a.row_index = row_index;
    a.actions = out;
    a.n = n;
    a.row_stride = row_stride;
    a.act_stride = s.n_out;
    const size_t lds = policy_lds_bytes(s);
    if (n <= 0 || lds > kPolMaxLds) return (int)hipErrorInvalidValue;
    return launch_forward_any_<true>(a, lds, (hipStream_t)stream);
}

}  // namespace dockauv
