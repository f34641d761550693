// dockauv_backward.hip -- the backward pass of the library's MLP for gfx950 (MI355X): the gradients of all weights and biases for
// upstream gradients on the network's raw output (include/dockauv.h: dockauv_policy_backward; the reference's counterpart is
// what torch autograd does for SB3's MlpPolicy inside PPO.train, train.py:64-71).  The upstream gradients are the PPO head's
// (dockauv_head.hip) or the learner's own; the optimiser stays in torch.
//
// Two launches.  policy_backward_kernel<MT1, MT2>: a bounded grid of groups of four waves; a group walks the passes
// b = blockIdx.x, blockIdx.x + gridDim.x, ... of 32 rt rows each and keeps its sums over all of them.  Everything of a pass lies
// in LDS as a row-major matrix with an odd stride (dockauv_device.h: BackwardLayout), so that each matrix serves as the A operand
// (lane = its row) and as the B operand (lane = its column) of v_mfma_f32_32x32x2_f32 without a bank conflict; the three kinds
// of product are the same instruction with the operands read along another axis:
//   forward    H = act(W X + b)        A = W [unit][k]        B = X [k][row]        k over the inputs, two per step
//   delta      D' = (W^T D) . act'     A = W [k][unit] (the same image, read down a column)   B = D [k][row]
//   gradient   dW += D H^T             A = D [unit][row]      B = H [unit'][row]    k over the rows of the pass
// Passes: stage X and G (rows >= n: zeros, which makes every one of their deltas an exact zero) | H1 | H2 | dW3, db3 and the
// delta of the last hidden layer | dW2, db2 and delta 1 | dW1, db1; a barrier between two of them.  The 32 x 32 tiles of a layer
// (activations, deltas) and of a gradient are dealt to the four waves round robin; a gradient tile is 16 accumulator registers
// that its wave keeps over all passes (dW2 of 128 x 128: four tiles per wave).  A bias gradient is the row sum of the staged
// delta, one unit per thread, rows in order.  Padded units have zero weights and biases: h = act(0) = 0 and delta = 0 exactly.
// At the end every group writes its sums as one partial in torch.nn.Linear layout; policy_backward_reduce_kernel adds the
// partials in group order.  No atomics: the bits depend on the shapes, n and a row's position in the minibatch only.
// SAC's networks (dockauv_sac_actor_backward, dockauv_q_backward) run the same passes in kernels of their own, below.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dockauv.h"
#include "dockauv_device.h"

namespace dockauv {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct BwdArgs {
    PolicyShape S;
    BackwardLayout L;
    const float* packed;
    const float* rows;
    const long long* row_index;        // nullable [n]
    const float* grad_out;             // [n][n_out]
    float* partial;                    // [gridDim.x][L.n_params]
    long n;
    int row_stride;
};

__device__ __forceinline__ int unit_of_(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

__device__ __forceinline__ float tanh_(float x) {      // dockauv_policy.hip: tanh_
    const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);
    return fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
}

__device__ __forceinline__ float act_(float x, int kind) { return kind == DOCKAUV_ACT_TANH ? tanh_(x) : fmaxf(x, 0.0f); }

// act'(pre-activation) from h = act(pre-activation): tanh' = 1 - h^2; relu' = 1 where the pre-activation is > 0, i.e. h > 0
__device__ __forceinline__ float dact_(float h, int kind) {
    return kind == DOCKAUV_ACT_TANH ? fmaf(-h, h, 1.0f) : (h > 0.0f ? 1.0f : 0.0f);
}

// the packed weights (PolicyShape) -> the row-major images, by all threads of the group; padding stays zero
__device__ void stage_weights_(const BwdArgs& a, float* lds) {
    const PolicyShape& S = a.S;
    const BackwardLayout& L = a.L;
    for (int i = threadIdx.x; i < L.off_x; i += kPolThreads) lds[i] = 0.0f;
    for (int i = threadIdx.x; i < L.acc_slots * 4 * 1024; i += kPolThreads) lds[L.off_acc + i] = 0.0f;
    __syncthreads();
    for (int idx = threadIdx.x; idx < S.off_std; idx += kPolThreads) {
        const float v = a.packed[idx];
        if (idx < S.off_w2) {
            const int loc = idx - S.off_w1, l = loc & 63, t = loc >> 6;
            const int m = t % S.mt1, s = t / S.mt1;
            lds[L.off_w1 + (32 * m + (l & 31)) * L.ws1 + 2 * s + (l >> 5)] = v;
        } else if (idx < S.off_w3) {
            const int loc = idx - S.off_w2, l = loc & 63, t = loc >> 6;
            const int m = t % S.mt2, sr = t / S.mt2;
            lds[L.off_w2 + (32 * m + (l & 31)) * L.ws2 + 32 * (sr >> 4) + unit_of_(sr & 15, l >> 5)] = v;
        } else if (idx < S.off_b1) {
            const int loc = idx - S.off_w3, l = loc & 63, sr = loc >> 6;
            if ((l & 31) < 8) lds[L.off_w3 + (l & 31) * L.ws3 + 32 * (sr >> 4) + unit_of_(sr & 15, l >> 5)] = v;
        } else if (idx < S.off_b3) {
            const bool first = idx < S.off_b2;
            const int loc = idx - (first ? S.off_b1 : S.off_b2);
            lds[(first ? L.off_b1 : L.off_b2) + 32 * (loc >> 5) + unit_of_((loc >> 1) & 15, loc & 1)] = v;
        }
    }
    __syncthreads();
}

// one 32 x 32 tile of H = act(W X + b) for row tile rt: units 32 m .. of `w` ([.][ws]), ks steps of two inputs of `x` ([.][rs])
__device__ __forceinline__ void forward_tile_(const float* w, int ws, const float* bias, const float* x, float* h, int rs, int ks,
                                              int m, int rt, int kind, int lane) {
    const int half = lane >> 5, col = lane & 31;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = bias[32 * m + unit_of_(r, half)];
    const float* wa = w + (32 * m + col) * ws + half;
    const float* xb = x + half * rs + 32 * rt + col;
    for (int s = 0; s < ks; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[2 * s], xb[2 * s * rs], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) h[(32 * m + unit_of_(r, half)) * rs + 32 * rt + col] = act_(acc[r], kind);
}

// one 32 x 32 tile of D' = (W^T D) . act'(H) for row tile rt: units 32 m .. of the layer below, ks steps of two units of D
__device__ __forceinline__ void delta_tile_(const float* w, int ws, const float* d, const float* h, float* out, int rs, int ks, int m,
                                            int rt, int kind, int lane) {
    const int half = lane >> 5, col = lane & 31;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const float* wa = w + half * ws + 32 * m + col;
    const float* db = d + half * rs + 32 * rt + col;
#pragma unroll 4
    for (int s = 0; s < ks; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[2 * s * ws], db[2 * s * rs], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int at = (32 * m + unit_of_(r, half)) * rs + 32 * rt + col;
        out[at] = acc[r] * dact_(h[at], kind);
    }
}

// acc += D H^T over the rows of the pass: rows 32 mo .. of `d` (d_rows of them exist) x rows 32 mi .. of `h` (h_rows exist)
__device__ __forceinline__ void grad_tile_(f32x16& acc, const float* d, int d_rows, const float* h, int h_rows, int rs, int ks,
                                           int mo, int mi, int lane) {
    const int half = lane >> 5, col = lane & 31;
    const bool a_on = 32 * mo + col < d_rows, b_on = 32 * mi + col < h_rows;
    const float* da = d + (a_on ? 32 * mo + col : 0) * rs + half;
    const float* hb = h + (b_on ? 32 * mi + col : 0) * rs + half;
#pragma unroll 4
    for (int s = 0; s < ks; ++s) {
        const float av = da[2 * s], bv = hb[2 * s];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_on ? av : 0.0f, b_on ? bv : 0.0f, acc, 0, 0, 0);
    }
}

// a gradient tile -> the group's partial, Linear layout [n_o][n_i]: register r of lane l is [32 mo + unit(r, half)][32 mi + col]
__device__ __forceinline__ void store_tile_(const f32x16& acc, float* dst, int n_o, int n_i, int mo, int mi, int lane) {
    const int half = lane >> 5, i = 32 * mi + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = 32 * mo + unit_of_(r, half);
        if (o < n_o && i < n_i) dst[o * n_i + i] = acc[r];
    }
}

// sum over the rows of the pass of row t of `d`, in row order
__device__ __forceinline__ float row_sum_(const float* d, int rs, int rows, int t) {
    float s = 0.0f;
    for (int j = 0; j < rows; ++j) s += d[t * rs + j];
    return s;
}

template <int MT1, int MT2>
__global__ __launch_bounds__(kPolThreads) void policy_backward_kernel(const BwdArgs a) {
    extern __shared__ float lds[];
    const PolicyShape& S = a.S;
    const BackwardLayout& L = a.L;
    constexpr int MTL = MT2 ? MT2 : MT1;
    constexpr int P2 = (MT1 * MT2 + 3) / 4;             // dW2 tiles of one wave
    // what backward_layout derives from the tiles alone, as constants: row tiles of a pass, row stride, strides of W2 and W3
    constexpr int MTMAX = MT1 > MT2 ? MT1 : MT2;
    constexpr int RT = MTMAX >= 3 ? 1 : (MTMAX == 2 ? 2 : 4), rs = 32 * RT + 1, R = 32 * RT;
    constexpr int WS2 = 32 * MT1 + 1, WS3 = 32 * MTL + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kind = S.hidden_act;
    float* W1 = lds + L.off_w1;
    float* W2 = lds + L.off_w2;
    float* W3 = lds + L.off_w3;
    float* X = lds + L.off_x;
    float* G = lds + L.off_g;
    float* H1 = lds + L.off_h1;
    float* H2 = lds + L.off_h2;
    float* D = lds + L.off_d;
    float* HL = MT2 ? H2 : H1;
    float* ACC = lds + L.off_acc;

    stage_weights_(a, lds);

    f32x16 g3, g2[P2 ? P2 : 1], g1[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        g3[r] = 0.0f;
        g1[0][r] = g1[1][r] = 0.0f;
#pragma unroll
        for (int j = 0; j < (P2 ? P2 : 1); ++j) g2[j][r] = 0.0f;
    }
    float s3 = 0.0f, s2 = 0.0f, s1 = 0.0f;              // bias gradients: unit tid of db3 / db2 / db1
    const int n_t1 = MT1 * L.kt1;                       // dW1 tiles: (mo, mi) = (p / kt1, p % kt1)

    const long passes = (a.n + R - 1) / R;
    for (long b = blockIdx.x; b < passes; b += gridDim.x) {
        // ---- stage the observations and the upstream gradients of the pass, [column][row]
        const int kx = 2 * S.ks1;
        for (int i = tid; i < R * kx; i += kPolThreads) {
            const int row = i / kx, k = i - row * kx;
            const long at = b * R + row;
            float v = 0.0f;
            if (at < a.n && k < S.n_in) {
                const long src = a.row_index ? (long)a.row_index[at] : at;
                v = a.rows[src * (long)a.row_stride + k];
            }
            X[k * rs + row] = v;
        }
        for (int i = tid; i < R * 8; i += kPolThreads) {
            const int row = i >> 3, o = i & 7;
            const long at = b * R + row;
            G[o * rs + row] = (at < a.n && o < S.n_out) ? a.grad_out[at * S.n_out + o] : 0.0f;
        }
        __syncthreads();

        // ---- recompute the activations
        for (int it = wave; it < MT1 * RT; it += 4)
            forward_tile_(W1, L.ws1, lds + L.off_b1, X, H1, rs, S.ks1, it / RT, it % RT, kind, lane);
        __syncthreads();
        if constexpr (MT2 > 0) {
            for (int it = wave; it < MT2 * RT; it += 4)
                forward_tile_(W2, WS2, lds + L.off_b2, H1, H2, rs, 16 * MT1, it / RT, it % RT, kind, lane);
            __syncthreads();
        }

        // ---- output layer: dW3 += G HL^T, db3, and the delta of the last hidden layer D = (W3^T G) . act'(HL)
        if (wave < MTL) grad_tile_(g3, G, 8, HL, 32 * MTL, rs, 16 * RT, 0, wave, lane);
        if (tid < 8) s3 += row_sum_(G, rs, R, tid);
        for (int it = wave; it < MTL * RT; it += 4)
            delta_tile_(W3, WS3, G, HL, D, rs, 4, it / RT, it % RT, kind, lane);
        __syncthreads();

        if constexpr (MT2 > 0) {
            // ---- dW2 += D H1^T, db2, and delta 1 = (W2^T D) . act'(H1) into the buffer of H2 (read for the last time above)
#pragma unroll
            for (int j = 0; j < P2; ++j) {
                const int p = wave + 4 * j;
                if (p < MT1 * MT2) grad_tile_(g2[j], D, 32 * MT2, H1, 32 * MT1, rs, 16 * RT, p / MT1, p % MT1, lane);
            }
            if (tid < 32 * MT2) s2 += row_sum_(D, rs, R, tid);
            for (int it = wave; it < MT1 * RT; it += 4)
                delta_tile_(W2, WS2, D, H1, H2, rs, 16 * MT2, it / RT, it % RT, kind, lane);
            __syncthreads();
        }

        // ---- dW1 += delta1 X^T, db1: a wave's first two tiles in registers, further ones (wide observations) in LDS
        const float* D1 = MT2 ? H2 : D;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int p = wave + 4 * j;
            if (p < n_t1) grad_tile_(g1[j], D1, 32 * MT1, X, S.n_in, rs, 16 * RT, p / L.kt1, p % L.kt1, lane);
        }
        for (int j = 2; wave + 4 * j < n_t1; ++j) {
            const int p = wave + 4 * j;
            float* slot = ACC + ((j - 2) * 4 + wave) * 1024 + lane;
            f32x16 t;
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = slot[64 * r];
            grad_tile_(t, D1, 32 * MT1, X, S.n_in, rs, 16 * RT, p / L.kt1, p % L.kt1, lane);
#pragma unroll
            for (int r = 0; r < 16; ++r) slot[64 * r] = t[r];
        }
        if (tid < 32 * MT1) s1 += row_sum_(D1, rs, R, tid);
        __syncthreads();
    }

    // ---- the group's partial, Linear layout
    float* out = a.partial + (long)blockIdx.x * L.n_params;
    const int n_last = S.n_h2 ? S.n_h2 : S.n_h1;
    if (wave < MTL) store_tile_(g3, out + L.p_w3, S.n_out, n_last, 0, wave, lane);
    if (tid < S.n_out) out[L.p_b3 + tid] = s3;
    if constexpr (MT2 > 0) {
#pragma unroll
        for (int j = 0; j < P2; ++j) {
            const int p = wave + 4 * j;
            if (p < MT1 * MT2) store_tile_(g2[j], out + L.p_w2, S.n_h2, S.n_h1, p / MT1, p % MT1, lane);
        }
        if (tid < S.n_h2) out[L.p_b2 + tid] = s2;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = wave + 4 * j;
        if (p < n_t1) store_tile_(g1[j], out + L.p_w1, S.n_h1, S.n_in, p / L.kt1, p % L.kt1, lane);
    }
    for (int j = 2; wave + 4 * j < n_t1; ++j) {
        const int p = wave + 4 * j;
        const float* slot = ACC + ((j - 2) * 4 + wave) * 1024 + lane;
        f32x16 t;
#pragma unroll
        for (int r = 0; r < 16; ++r) t[r] = slot[64 * r];
        store_tile_(t, out + L.p_w1, S.n_h1, S.n_in, p / L.kt1, p % L.kt1, lane);
    }
    if (tid < S.n_h1) out[L.p_b1 + tid] = s1;
}

struct ReduceArgs {
    BackwardLayout L;
    const float* partial;
    PolicyGrads g;
    int groups;
};

// gradient i = partial[0][i] + partial[1][i] + ... in group order
__global__ void policy_backward_reduce_kernel(const ReduceArgs a) {
    const BackwardLayout& L = a.L;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.n_params) return;
    float s = 0.0f;
    for (int g = 0; g < a.groups; ++g) s += a.partial[(long)g * L.n_params + i];
    if (i < L.p_b1) a.g.dW1[i - L.p_w1] = s;
    else if (i < L.p_w2) a.g.db1[i - L.p_b1] = s;
    else if (i < L.p_b2) a.g.dW2[i - L.p_w2] = s;
    else if (i < L.p_w3) a.g.db2[i - L.p_b2] = s;
    else if (i < L.p_b3) a.g.dW3[i - L.p_w3] = s;
    else a.g.db3[i - L.p_b3] = s;
}

template <int MT1, int MT2>
int launch_backward_(const BwdArgs& a, int groups, size_t lds, hipStream_t stream) {
    void (*kernel)(const BwdArgs) = policy_backward_kernel<MT1, MT2>;
    if (lds > 64 * 1024) {   // (more than 64 KiB of LDS per group is requested explicitly, dockauv_policy.hip: launch_forward_)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(kPolThreads), lds, stream, a);
    return (int)hipGetLastError();
}

template <int MT1>
int launch_backward_mt1_(const BwdArgs& a, int groups, size_t lds, hipStream_t stream) {
    switch (a.S.mt2) {
        case 0: return launch_backward_<MT1, 0>(a, groups, lds, stream);
        case 1: return launch_backward_<MT1, 1>(a, groups, lds, stream);
        case 2: return launch_backward_<MT1, 2>(a, groups, lds, stream);
        case 3: return launch_backward_<MT1, 3>(a, groups, lds, stream);
        case 4: return launch_backward_<MT1, 4>(a, groups, lds, stream);
    }
    return (int)hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------------------ SAC's networks
// dockauv_sac_actor_backward and dockauv_q_backward: the pass structure above with three extensions, as kernels of their own
// beside policy_backward_kernel, whose text and registers stay:
//   * X from two sources -- column k < n_obs from the observation row, k >= n_obs from the action row (an actor: n_obs = n_in);
//   * 16 rows of G and W3 for the squashed-Gaussian actor, whose output tile carries W_mu in units 0 .. n_u - 1 and W_ls in units
//     8 .. 8 + n_u - 1; the group's partial holds the two heads as [2 n_u][n_last], mu first, and the reduction splits them;
//   * dX on the action columns of a Q critic, grad_actions = W1[:, n_obs ..]^T delta1: one more product of the delta kind behind
//     delta 1, a 32 x 32 tile per row tile, stored straight to memory where the row and the column exist.
// Forms: BWD_ACTOR and BWD_Q (parameters) and BWD_Q_DX (dX alone: no gradient tiles, no bias sums, no partial, no reduction).  A
// call that asks for both outputs of a critic is BWD_Q and then BWD_Q_DX: SAC asks for one at a time (parameters on the replayed
// actions, dX on the actor's), and dX behind a run-time branch of BWD_Q cost that form 12 to 21 spilled SGPRs.
enum SacBwdForm { BWD_ACTOR = 0, BWD_Q = 1, BWD_Q_DX = 2 };

struct SacBwdArgs {
    PolicyShape S;                     // n_out: n_u (actor), 1 (Q)
    BackwardLayout L;                  // backward_layout with 16 output rows for the actor, whose n_params counts both heads
    const float* packed;
    const float* rows;                 // observation rows, row_stride floats apart
    const float* act_in;               // Q: action rows, act_stride floats apart
    const long long* row_index;        // nullable [n], shared by both sources
    const float* grad_out;             // actor: [n][2 n_u] (mu | raw log_std); Q: [n]
    float* partial;                    // [gridDim.x][L.n_params]; unused by BWD_Q_DX
    float* grad_actions;               // BWD_Q_DX: [n][n_u]
    long n;
    int row_stride, act_stride, n_obs, n_u;
};

// BackwardLayout's LDS offsets as the kernel forms them: from the tiles (compile time) and ks1 alone, so that they are two bases
// and immediates where eleven kernarg words would each hold an SGPR over all passes.  The launcher checks them against
// backward_layout before every launch.
struct LdsOffsets {
    int ws1, w2, w3, b1, b2, x, g, h1, h2, d, acc;
};
template <int MT1, int MT2, int GR>
__host__ __device__ __forceinline__ LdsOffsets lds_offsets_(int ks1) {
    constexpr int MTL = MT2 ? MT2 : MT1, MTMAX = MT1 > MT2 ? MT1 : MT2;
    constexpr int RT = MTMAX >= 3 ? 1 : (MTMAX == 2 ? 2 : 4), rs = 32 * RT + 1;
    LdsOffsets o;
    o.ws1 = 2 * ks1 + 1;
    o.w2 = 32 * MT1 * o.ws1;
    o.w3 = o.w2 + 32 * MT2 * (32 * MT1 + 1);
    o.b1 = o.w3 + GR * (32 * MTL + 1);
    o.b2 = o.b1 + 32 * MT1;
    o.x = o.b2 + 32 * MT2;
    o.g = o.x + 2 * ks1 * rs;
    o.h1 = o.g + GR * rs;
    o.h2 = o.h1 + 32 * MT1 * rs;
    o.d = o.h2 + (MT2 ? 32 * MTMAX : 0) * rs;
    o.acc = o.d + 32 * MTL * rs;
    return o;
}

// stage_weights_ with the output units below ROWS kept (8, or 16 for the actor's two heads)
template <int ROWS>
__device__ void stage_weights_rows_(const PolicyShape& S, const BackwardLayout& L, const float* packed, float* lds) {
    for (int i = threadIdx.x; i < L.off_x; i += kPolThreads) lds[i] = 0.0f;
    for (int i = threadIdx.x; i < L.acc_slots * 4 * 1024; i += kPolThreads) lds[L.off_acc + i] = 0.0f;
    __syncthreads();
    for (int idx = threadIdx.x; idx < S.off_std; idx += kPolThreads) {
        const float v = packed[idx];
        if (idx < S.off_w2) {
            const int loc = idx - S.off_w1, l = loc & 63, t = loc >> 6;
            const int m = t % S.mt1, s = t / S.mt1;
            lds[L.off_w1 + (32 * m + (l & 31)) * L.ws1 + 2 * s + (l >> 5)] = v;
        } else if (idx < S.off_w3) {
            const int loc = idx - S.off_w2, l = loc & 63, t = loc >> 6;
            const int m = t % S.mt2, sr = t / S.mt2;
            lds[L.off_w2 + (32 * m + (l & 31)) * L.ws2 + 32 * (sr >> 4) + unit_of_(sr & 15, l >> 5)] = v;
        } else if (idx < S.off_b1) {
            const int loc = idx - S.off_w3, l = loc & 63, sr = loc >> 6;
            if ((l & 31) < ROWS) lds[L.off_w3 + (l & 31) * L.ws3 + 32 * (sr >> 4) + unit_of_(sr & 15, l >> 5)] = v;
        } else if (idx < S.off_b3) {
            const bool first = idx < S.off_b2;
            const int loc = idx - (first ? S.off_b1 : S.off_b2);
            lds[(first ? L.off_b1 : L.off_b2) + 32 * (loc >> 5) + unit_of_((loc >> 1) & 15, loc & 1)] = v;
        }
    }
    __syncthreads();
}

// one 32 x 32 tile of dX = W1[:, n_obs ..]^T delta1 for row tile rt: A is W1 read down its columns n_obs + j (lane j < n_u, the
// other lanes zero), B is delta 1, ks steps of two hidden units, no activation factor.  Register r < 4 of lane (half, col) is
// column j = 4 half + r of row `first` + 32 rt + col: stored where the row and the column exist
__device__ __forceinline__ void dx_tile_(const float* w1, int ws, int n_obs, int n_u, const float* d, int rs, int ks, int rt, float* dst,
                                         long first, long n, int lane) {
    const int half = lane >> 5, col = lane & 31;
    const bool a_on = col < n_u;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const float* wa = w1 + half * ws + n_obs + (a_on ? col : 0);
    const float* db = d + half * rs + 32 * rt + col;
#pragma unroll 4
    for (int s = 0; s < ks; ++s) {
        const float av = wa[2 * s * ws];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_on ? av : 0.0f, db[2 * s * rs], acc, 0, 0, 0);
    }
    const long at = first + 32 * rt + col;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = 4 * half + r;
        if (at < n && j < n_u) dst[at * n_u + j] = acc[r];
    }
}

// the actor's output-layer tile -> the group's partial [2 n_u][n_i]: unit o < 8 is row o of W_mu, unit 8 + j row n_u + j (W_ls)
__device__ __forceinline__ void store_heads_tile_(const f32x16& acc, float* dst, int n_u, int n_i, int mi, int lane) {
    const int half = lane >> 5, i = 32 * mi + (lane & 31);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int o = unit_of_(r, half), j = o & 7;
        if (j < n_u && i < n_i) dst[((o >> 3) * n_u + j) * n_i + i] = acc[r];
    }
}

// the kernel's argument block again, through a pointer the optimiser cannot trace back to it (the block is the first object of the
// kernarg segment): what is read through it is loaded where it is read
#if defined(__HIP_DEVICE_COMPILE__)
typedef const SacBwdArgs __attribute__((address_space(4)))* LateArgs;
__device__ __forceinline__ LateArgs late_args_(const SacBwdArgs&) {
    LateArgs p = (LateArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
#else
typedef const SacBwdArgs* LateArgs;
__device__ inline LateArgs late_args_(const SacBwdArgs& a) { return &a; }
#endif

template <int MT1, int MT2, int FORM>
__device__ __forceinline__ void sac_backward_body_(const SacBwdArgs& a, float* lds) {
    constexpr bool ACTOR = FORM == BWD_ACTOR, PARAMS = FORM != BWD_Q_DX;
    constexpr int GR = ACTOR ? 16 : 8;                  // rows of G and W3
    const PolicyShape& S = a.S;
    const BackwardLayout& L = a.L;
    constexpr int MTL = MT2 ? MT2 : MT1;
    constexpr int P2 = (MT1 * MT2 + 3) / 4;
    constexpr int MTMAX = MT1 > MT2 ? MT1 : MT2;
    constexpr int RT = MTMAX >= 3 ? 1 : (MTMAX == 2 ? 2 : 4), rs = 32 * RT + 1, R = 32 * RT;
    constexpr int WS2 = 32 * MT1 + 1, WS3 = 32 * MTL + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kind = S.hidden_act;
    const LdsOffsets O = lds_offsets_<MT1, MT2, GR>(S.ks1);
    const int kt1 = (S.n_in + 31) >> 5;                 // (BackwardLayout::kt1)
    float* W1 = lds;
    float* W2 = lds + O.w2;
    float* W3 = lds + O.w3;
    float* X = lds + O.x;
    float* G = lds + O.g;
    float* H1 = lds + O.h1;
    float* H2 = lds + O.h2;
    float* D = lds + O.d;
    float* HL = MT2 ? H2 : H1;
    [[maybe_unused]] float* ACC = lds + O.acc;

    stage_weights_rows_<GR>(S, L, a.packed, lds);

    [[maybe_unused]] f32x16 g3, g2[P2 ? P2 : 1], g1[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        g3[r] = 0.0f;
        g1[0][r] = g1[1][r] = 0.0f;
#pragma unroll
        for (int j = 0; j < (P2 ? P2 : 1); ++j) g2[j][r] = 0.0f;
    }
    [[maybe_unused]] float s3 = 0.0f, s2 = 0.0f, s1 = 0.0f;
    [[maybe_unused]] const int n_t1 = MT1 * kt1;

    const long passes = (a.n + R - 1) / R;
    for (long b = blockIdx.x; b < passes; b += gridDim.x) {
        // ---- stage [obs row | action row] and the upstream gradients of the pass, [column][row]
        const int kx = 2 * S.ks1;
        for (int i = tid; i < R * kx; i += kPolThreads) {
            const int row = i / kx, k = i - row * kx;
            const long at = b * R + row;
            float v = 0.0f;
            if (at < a.n && k < S.n_in) {
                const long src = a.row_index ? (long)a.row_index[at] : at;
                if constexpr (ACTOR) v = a.rows[src * (long)a.row_stride + k];
                else v = k < a.n_obs ? a.rows[src * (long)a.row_stride + k] : a.act_in[src * (long)a.act_stride + (k - a.n_obs)];
            }
            X[k * rs + row] = v;
        }
        for (int i = tid; i < R * GR; i += kPolThreads) {
            const int row = i / GR, o = i - row * GR;
            const long at = b * R + row;
            float v = 0.0f;
            if constexpr (ACTOR) {
                const int j = o & 7;                    // unit o: column j of head o >> 3
                if (at < a.n && j < S.n_out) v = a.grad_out[at * (2 * S.n_out) + (o >> 3) * S.n_out + j];
            } else {
                if (at < a.n && o == 0) v = a.grad_out[at];     // (a critic has one output)
            }
            G[o * rs + row] = v;
        }
        __syncthreads();

        // ---- recompute the activations
        for (int it = wave; it < MT1 * RT; it += 4)
            forward_tile_(W1, O.ws1, lds + O.b1, X, H1, rs, S.ks1, it / RT, it % RT, kind, lane);
        __syncthreads();
        if constexpr (MT2 > 0) {
            for (int it = wave; it < MT2 * RT; it += 4)
                forward_tile_(W2, WS2, lds + O.b2, H1, H2, rs, 16 * MT1, it / RT, it % RT, kind, lane);
            __syncthreads();
        }

        // ---- output layer: dW3 += G HL^T, db3, and the delta of the last hidden layer
        if constexpr (PARAMS) {
            if (wave < MTL) grad_tile_(g3, G, GR, HL, 32 * MTL, rs, 16 * RT, 0, wave, lane);
            if (tid < GR) s3 += row_sum_(G, rs, R, tid);
        }
        for (int it = wave; it < MTL * RT; it += 4)
            delta_tile_(W3, WS3, G, HL, D, rs, GR / 2, it / RT, it % RT, kind, lane);
        __syncthreads();

        if constexpr (MT2 > 0) {
            // ---- dW2 += D H1^T, db2, and delta 1 into the buffer of H2
            if constexpr (PARAMS) {
#pragma unroll
                for (int j = 0; j < P2; ++j) {
                    const int p = wave + 4 * j;
                    if (p < MT1 * MT2) grad_tile_(g2[j], D, 32 * MT2, H1, 32 * MT1, rs, 16 * RT, p / MT1, p % MT1, lane);
                }
                if (tid < 32 * MT2) s2 += row_sum_(D, rs, R, tid);
            }
            for (int it = wave; it < MT1 * RT; it += 4)
                delta_tile_(W2, WS2, D, H1, H2, rs, 16 * MT2, it / RT, it % RT, kind, lane);
            __syncthreads();
        }

        // ---- dW1 += delta1 X^T, db1, and dX on the action columns
        const float* D1 = MT2 ? H2 : D;
        if constexpr (PARAMS) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int p = wave + 4 * j;
                if (p < n_t1) grad_tile_(g1[j], D1, 32 * MT1, X, S.n_in, rs, 16 * RT, p / kt1, p % kt1, lane);
            }
            for (int j = 2; wave + 4 * j < n_t1; ++j) {
                const int p = wave + 4 * j;
                float* slot = ACC + ((j - 2) * 4 + wave) * 1024 + lane;
                f32x16 t;
#pragma unroll
                for (int r = 0; r < 16; ++r) t[r] = slot[64 * r];
                grad_tile_(t, D1, 32 * MT1, X, S.n_in, rs, 16 * RT, p / kt1, p % kt1, lane);
#pragma unroll
                for (int r = 0; r < 16; ++r) slot[64 * r] = t[r];
            }
            if (tid < 32 * MT1) s1 += row_sum_(D1, rs, R, tid);
        }
        if constexpr (FORM == BWD_Q_DX) {
            for (int it = wave; it < RT; it += 4)
                dx_tile_(W1, O.ws1, a.n_obs, S.n_in - a.n_obs, D1, rs, 16 * MT1, it, a.grad_actions, b * R, a.n, lane);
        }
        __syncthreads();
    }

    if constexpr (PARAMS) {
        // ---- the group's partial, Linear layout (the actor's two heads as one [2 n_u][n_last] block, mu first).  What this phase
        // alone reads -- the partial's pointer and offsets, the layer widths -- comes from the kernarg block again, through a
        // pointer the optimiser cannot trace back to it: loaded here, behind the passes, it holds no SGPR across them (with those
        // values live over the loop the two-source and 16-row forms spilled 12 to 21 SGPRs into VGPR lanes)
        const LateArgs late = late_args_(a);
        struct { int n_in, n_h1, n_h2, n_out; } S{late->S.n_in, late->S.n_h1, late->S.n_h2, late->S.n_out};
        struct { int kt1, p_w1, p_b1, p_w2, p_b2, p_w3, p_b3, n_params; } L{late->L.kt1, late->L.p_w1, late->L.p_b1, late->L.p_w2, late->L.p_b2,
                                                                            late->L.p_w3, late->L.p_b3, late->L.n_params};
        const int n_t1 = MT1 * L.kt1;
        float* out = late->partial + (long)blockIdx.x * L.n_params;
        const int n_last = S.n_h2 ? S.n_h2 : S.n_h1;
        if constexpr (ACTOR) {
            if (wave < MTL) store_heads_tile_(g3, out + L.p_w3, S.n_out, n_last, wave, lane);
            if (tid < 16 && (tid & 7) < S.n_out) out[L.p_b3 + (tid >> 3) * S.n_out + (tid & 7)] = s3;
        } else {
            if (wave < MTL) store_tile_(g3, out + L.p_w3, 1, n_last, 0, wave, lane);
            if (tid == 0) out[L.p_b3] = s3;
        }
        if constexpr (MT2 > 0) {
#pragma unroll
            for (int j = 0; j < P2; ++j) {
                const int p = wave + 4 * j;
                if (p < MT1 * MT2) store_tile_(g2[j], out + L.p_w2, S.n_h2, S.n_h1, p / MT1, p % MT1, lane);
            }
            if (tid < S.n_h2) out[L.p_b2 + tid] = s2;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int p = wave + 4 * j;
            if (p < n_t1) store_tile_(g1[j], out + L.p_w1, S.n_h1, S.n_in, p / L.kt1, p % L.kt1, lane);
        }
        for (int j = 2; wave + 4 * j < n_t1; ++j) {
            const int p = wave + 4 * j;
            const float* slot = ACC + ((j - 2) * 4 + wave) * 1024 + lane;
            f32x16 t;
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = slot[64 * r];
            store_tile_(t, out + L.p_w1, S.n_h1, S.n_in, p / L.kt1, p % L.kt1, lane);
        }
        if (tid < S.n_h1) out[L.p_b1 + tid] = s1;
    }
}

template <int MT1, int MT2>
__global__ __launch_bounds__(kPolThreads) void sac_actor_backward_kernel(const SacBwdArgs a) {
    extern __shared__ float lds[];
    sac_backward_body_<MT1, MT2, BWD_ACTOR>(a, lds);
}

template <int MT1, int MT2>
__global__ __launch_bounds__(kPolThreads) void q_backward_kernel(const SacBwdArgs a) {
    extern __shared__ float lds[];
    sac_backward_body_<MT1, MT2, BWD_Q>(a, lds);
}

template <int MT1, int MT2>
__global__ __launch_bounds__(kPolThreads) void q_backward_dx_kernel(const SacBwdArgs a) {
    extern __shared__ float lds[];
    sac_backward_body_<MT1, MT2, BWD_Q_DX>(a, lds);
}

struct SacReduceArgs {
    BackwardLayout L;
    const float* partial;
    SacActorGrads g;
    int groups, n_head;                // n_head: n_u n_last, the floats of one head's weights
    int n_u;
};

// policy_backward_reduce_kernel for the actor: the [2 n_u][n_last] block and its bias go to the four head arrays
__global__ void sac_actor_backward_reduce_kernel(const SacReduceArgs a) {
    const BackwardLayout& L = a.L;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.n_params) return;
    float s = 0.0f;
    for (int g = 0; g < a.groups; ++g) s += a.partial[(long)g * L.n_params + i];
    if (i < L.p_b1) a.g.dW1[i - L.p_w1] = s;
    else if (i < L.p_w2) a.g.db1[i - L.p_b1] = s;
    else if (i < L.p_b2) a.g.dW2[i - L.p_w2] = s;
    else if (i < L.p_w3) a.g.db2[i - L.p_b2] = s;
    else if (i < L.p_w3 + a.n_head) a.g.dW_mu[i - L.p_w3] = s;
    else if (i < L.p_b3) a.g.dW_ls[i - L.p_w3 - a.n_head] = s;
    else if (i < L.p_b3 + a.n_u) a.g.db_mu[i - L.p_b3] = s;
    else a.g.db_ls[i - L.p_b3 - a.n_u] = s;
}

template <int MT1, int MT2, int GR>
bool offsets_agree_(const PolicyShape& S, const BackwardLayout& L) {
    const LdsOffsets o = lds_offsets_<MT1, MT2, GR>(S.ks1);
    return L.off_w1 == 0 && o.ws1 == L.ws1 && o.w2 == L.off_w2 && o.w3 == L.off_w3 && o.b1 == L.off_b1 && o.b2 == L.off_b2 &&
           o.x == L.off_x && o.g == L.off_g && o.h1 == L.off_h1 && o.h2 == L.off_h2 && o.d == L.off_d && o.acc == L.off_acc &&
           (S.n_in + 31) / 32 == L.kt1;
}

template <int MT1, int MT2>
int launch_sac_backward_(const SacBwdArgs& a, int form, int groups, size_t lds, hipStream_t stream) {
    if (!(form == BWD_ACTOR ? offsets_agree_<MT1, MT2, 16>(a.S, a.L) : offsets_agree_<MT1, MT2, 8>(a.S, a.L))) return (int)hipErrorInvalidValue;
    void (*kernel)(const SacBwdArgs) = form == BWD_ACTOR ? sac_actor_backward_kernel<MT1, MT2>
                                       : (form == BWD_Q ? q_backward_kernel<MT1, MT2> : q_backward_dx_kernel<MT1, MT2>);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(kPolThreads), lds, stream, a);
    return (int)hipGetLastError();
}

template <int MT1>
int launch_sac_backward_mt1_(const SacBwdArgs& a, int form, int groups, size_t lds, hipStream_t stream) {
    switch (a.S.mt2) {
        case 0: return launch_sac_backward_<MT1, 0>(a, form, groups, lds, stream);
        case 1: return launch_sac_backward_<MT1, 1>(a, form, groups, lds, stream);
        case 2: return launch_sac_backward_<MT1, 2>(a, form, groups, lds, stream);
        case 3: return launch_sac_backward_<MT1, 3>(a, form, groups, lds, stream);
        case 4: return launch_sac_backward_<MT1, 4>(a, form, groups, lds, stream);
    }
    return (int)hipErrorInvalidValue;
}

// the kernel of `form` on the bounded grid; *groups_out: the partials it leaves
int launch_sac_backward_any_(SacBwdArgs& a, int form, int* groups_out, hipStream_t stream) {
    const size_t lds = backward_lds_bytes(a.L);
    if (a.n <= 0 || lds > kPolMaxLds) return (int)hipErrorInvalidValue;
    const long passes = (a.n + 32 * a.L.rt - 1) / (32 * a.L.rt);
    const int groups = (int)(passes < kBwdMaxGroups ? passes : kBwdMaxGroups);
    *groups_out = groups;
    switch (a.S.mt1) {
        case 1: return launch_sac_backward_mt1_<1>(a, form, groups, lds, stream);
        case 2: return launch_sac_backward_mt1_<2>(a, form, groups, lds, stream);
        case 3: return launch_sac_backward_mt1_<3>(a, form, groups, lds, stream);
        case 4: return launch_sac_backward_mt1_<4>(a, form, groups, lds, stream);
    }
    return (int)hipErrorInvalidValue;
}

}  // namespace

int launch_sac_actor_backward(const PolicyShape& s, const float* packed, const SacBackwardLaunch& l, float* partial,
                              const SacActorGrads& grads, void* stream) {
    SacBwdArgs a{};
    a.S = s;
    sac_actor_backward_layout(s, a.L);
    a.packed = packed;
    a.rows = l.rows;
    a.row_index = l.row_index;
    a.grad_out = l.grad_out;
    a.partial = partial;
    a.n = l.n;
    a.row_stride = l.row_stride;
    a.n_obs = s.n_in;                                   // (every column comes from the observation row)
    a.n_u = s.n_out;
    if (!partial || (s.n_h2 && (!grads.dW2 || !grads.db2))) return (int)hipErrorInvalidValue;
    int groups = 0;
    const int rc = launch_sac_backward_any_(a, BWD_ACTOR, &groups, (hipStream_t)stream);
    if (rc != 0) return rc;
    SacReduceArgs r{a.L, partial, grads, groups, s.n_out * (s.n_h2 ? s.n_h2 : s.n_h1), s.n_out};
    hipLaunchKernelGGL(sac_actor_backward_reduce_kernel, dim3((unsigned)((a.L.n_params + 255) / 256)), dim3(256), 0, (hipStream_t)stream, r);
    return (int)hipGetLastError();
}

int launch_q_backward(const PolicyShape& s, const float* packed, const SacBackwardLaunch& l, float* partial, const PolicyGrads* grads,
                      void* stream) {
    SacBwdArgs a{};
    a.S = s;
    backward_layout(s, a.L);
    a.packed = packed;
    a.rows = l.rows;
    a.act_in = l.actions;
    a.row_index = l.row_index;
    a.grad_out = l.grad_out;
    a.partial = partial;
    a.grad_actions = l.grad_actions;
    a.n = l.n;
    a.row_stride = l.row_stride;
    a.act_stride = l.act_stride;
    a.n_obs = l.n_obs;
    a.n_u = s.n_in - l.n_obs;
    if (l.n_obs < 1 || a.n_u < 1 || a.n_u > kMaxU || (!grads && !l.grad_actions)) return (int)hipErrorInvalidValue;
    if (grads && (!partial || (s.n_h2 && (!grads->dW2 || !grads->db2)))) return (int)hipErrorInvalidValue;
    int groups = 0;
    if (grads) {
        const int rc = launch_sac_backward_any_(a, BWD_Q, &groups, (hipStream_t)stream);
        if (rc != 0) return rc;
        ReduceArgs r{a.L, partial, *grads, groups};
        hipLaunchKernelGGL(policy_backward_reduce_kernel, dim3((unsigned)((a.L.n_params + 255) / 256)), dim3(256), 0, (hipStream_t)stream, r);
        const int rr = (int)hipGetLastError();
        if (rr != 0 || !l.grad_actions) return rr;
    }
    return launch_sac_backward_any_(a, BWD_Q_DX, &groups, (hipStream_t)stream);
}

int launch_policy_backward(const PolicyShape& s, const float* packed, const float* rows, const long long* row_index, long n,
                           int row_stride, const float* grad_out, float* partial, const PolicyGrads& grads, void* stream) {
    BwdArgs a;
    a.S = s;
    backward_layout(s, a.L);
    a.packed = packed;
    a.rows = rows;
    a.row_index = row_index;
    a.grad_out = grad_out;
    a.partial = partial;
    a.n = n;
    a.row_stride = row_stride;
    const size_t lds = backward_lds_bytes(a.L);
    if (n <= 0 || lds > kPolMaxLds || (s.n_h2 && (!grads.dW2 || !grads.db2))) return (int)hipErrorInvalidValue;
    const long passes = (n + 32 * a.L.rt - 1) / (32 * a.L.rt);
    const int groups = (int)(passes < kBwdMaxGroups ? passes : kBwdMaxGroups);
    int rc = (int)hipErrorInvalidValue;
    switch (s.mt1) {
        case 1: rc = launch_backward_mt1_<1>(a, groups, lds, (hipStream_t)stream); break;
        case 2: rc = launch_backward_mt1_<2>(a, groups, lds, (hipStream_t)stream); break;
        case 3: rc = launch_backward_mt1_<3>(a, groups, lds, (hipStream_t)stream); break;
        case 4: rc = launch_backward_mt1_<4>(a, groups, lds, (hipStream_t)stream); break;
    }
    if (rc != 0) return rc;
    ReduceArgs r{a.L, partial, grads, groups};
    hipLaunchKernelGGL(policy_backward_reduce_kernel, dim3((unsigned)((a.L.n_params + 255) / 256)), dim3(256), 0, (hipStream_t)stream, r);
    return (int)hipGetLastError();
}

}  // namespace dockauv
