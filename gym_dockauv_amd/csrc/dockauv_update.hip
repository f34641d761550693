// dockauv_update.hip -- what dockauv_ppo_update adds to the kernels of its pieces, for gfx950 (MI355X): the minibatch
// permutation of an epoch and the start of a call on the optimiser's control block (include/dockauv.h: dockauv_permutation
// states every integer expression, dockauv_ppo_update the control block; the reference's counterpart is the
// np.random.permutation of SB3's RolloutBuffer.get inside PPO.train, train.py:64-71).
//
// The permutation is the bijective shuffle of Mitchell, Stokes, Frank and Holmes, "Bandwidth-optimal random shuffling for GPUs"
// (2022): a keyed bijection of [0, 2^b) -- an eight-round Feistel network on unequal halves -- restricted to [0, n) by
// cycle-walking.  One lane per output, no sort, no workspace, integer arithmetic only: out[i] is a function of (seed, epoch, n, i).
// The round keys are two Philox blocks of wave-uniform inputs (kernel arguments), so every lane of the launch holds the same
// eight words.  The walk of lane i follows the cycle of the bijection that contains i and stops at the first point below n;
// that cycle contains i < n itself, so the loop ends without a bound.  Lanes of a wave walk different lengths (fewer than two
// applications on average, since 2^b < 2 n for n > 2): they diverge there, and that is accepted.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dockauv_device.h"

namespace dockauv {
namespace {

// one application of the network to x < 2^(wl + wr): the left half is the high wl bits
__device__ __forceinline__ uint32_t feistel_(uint32_t x, const uint32_t (&key)[8], int wl, int wr) {
    uint32_t L = x >> wr, R = x & ((1u << wr) - 1u);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int w = (r & 1) ? wr : wl;        // the width of the current left half: the two widths swap every round
        const uint64_t t = (uint64_t)(R + key[r]) * 0xD2511F53u;
        uint32_t f = (uint32_t)(t >> 32) ^ (uint32_t)t;
        f = (f ^ (f >> 15)) & ((1u << w) - 1u);
        const uint32_t nl = R;
        R = L ^ f;
        L = nl;
    }
    return (L << wr) | R;                       // (eight rounds: the widths are the first ones again)
}

__global__ __launch_bounds__(kPermThreads) void permutation_kernel(unsigned long long seed, uint32_t epoch, long long n, int wl, int wr,
                                                                   long long* __restrict__ out) {
    uint32_t key[8];
#pragma unroll
    for (uint32_t q = 0; q < 2; ++q) {
        uint32_t c[4] = {q, epoch, 0u, kPermStream};
        philox4x32_10_(c, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
#pragma unroll
        for (int k = 0; k < 4; ++k) key[4 * q + k] = c[k];
    }
    const long long i = (long long)blockIdx.x * kPermThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t x = (uint32_t)i;
    do x = feistel_(x, key, wl, wr);
    while ((long long)x >= n);
    out[i] = (long long)x;
}

__global__ __launch_bounds__(64) void update_begin_kernel(OptimCtl* ctl, long long t0) {
    if (threadIdx.x == 0) {
        ctl->t = t0;
        ctl->stop = 0;
        ctl->reserved = 0;
        ctl->step_size = 0.0f;
        ctl->rsq = 0.0f;
    }
}

}  // namespace

int launch_permutation(unsigned long long seed, unsigned long long epoch, long long n, long long* out, void* stream) {
    if (n < 1 || n > (1ll << 31) || !out) return (int)hipErrorInvalidValue;
    int b = 0;
    while ((1ll << b) < n) ++b;                 // bit_length(n - 1)
    if (b < 2) b = 2;
    const int wl = b / 2, wr = b - wl;
    const unsigned groups = (unsigned)((n + kPermThreads - 1) / kPermThreads);
    hipLaunchKernelGGL(permutation_kernel, dim3(groups), dim3(kPermThreads), 0, (hipStream_t)stream, seed, (uint32_t)(epoch & 0xffffffffull),
                       n, wl, wr, out);
    return (int)hipGetLastError();
}

int launch_update_begin(OptimCtl* ctl, long long t0, void* stream) {
    if (!ctl) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(update_begin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ctl, t0);
    return (int)hipGetLastError();
}

}  // namespace dockauv
