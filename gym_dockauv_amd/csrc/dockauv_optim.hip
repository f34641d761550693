// dockauv_optim.hip -- gradient-norm clipping and one Adam step over all parameters of an actor, its log_std and a critic for
// gfx950 (MI355X), in ONE launch (include/dockauv.h: dockauv_optim_step states every float32 expression; the reference's
// counterpart is the tail of SB3's PPO.train, train.py:64-71: clip_grad_norm_ and Adam.step).
//
// The index space is kOptSegments arrays back to back -- actor W1 b1 W2 b2 W3 b3, log_std, critic W1 b1 W2 b2 W3 b3, torch.nn.Linear
// layout, any of them empty -- at most a few ten thousand floats: the step is bound by the latency of dependent launches and of
// dependent loads, not by traffic.  So there is no pass between groups: a grid of ceil(total / kOptThreads) groups of sixteen
// waves, thread i of the grid owning element i of the index space, and EVERY group forms the whole gradient norm itself:
//   - a thread first issues the loads of its own element (parameter, gradient, both moments), which are then in flight behind
//     the norm;
//   - segment by segment, lane t of the group adds (double)g * (double)g of the elements t, t + 1024, t + 2048, .. of the segment
//     (kOptChunk loads in flight; the gradients are a few hundred KiB and come from L2 for every group but the first to ask);
//   - the lanes of a wave are added by a fixed shuffle tree, the sixteen waves in order from LDS by every thread (broadcast
//     reads): the same float64 sum, hence the same float32 norm and the same coef, bit for bit, in every thread of every group;
//   - the thread updates its element and stores p, m and v; thread 0 of group 0 writes stats.
// No floating-point atomics: the bits depend on the gradients, the state and the segment lengths only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dockauv_device.h"

namespace dockauv {
namespace {

// lane 0 gets the sum over the 64 lanes, added in the order of this tree (dockauv_head.hip)
__device__ __forceinline__ double wave_sum_(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// A: AdamArgs (dockauv_optim_step), or AdamArgsCtl (dockauv_ppo_update): the step's two bias corrections come from the
// optimiser's control block, and a launch that finds its stop flag set changes nothing
template <class A>
__global__ __launch_bounds__(kOptThreads) void adam_step_kernel(const A a) {
    __shared__ double red[kOptThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    [[maybe_unused]] float ctl_step_size = 0.0f, ctl_rsq = 0.0f;
    if constexpr (A::kCtl) {
        if (a.ctl->stop != 0) return;       // (the same in every thread of the grid)
        ctl_step_size = a.ctl->step_size;
        ctl_rsq = a.ctl->rsq;
    }

    // the thread's own element: segment s, offset k in it (at most one segment holds i)
    const int i = (int)blockIdx.x * kOptThreads + tid;
    const bool own = i < a.total;
    float* pp = nullptr;
    const float* gp = nullptr;
    int first = 0;
#pragma unroll
    for (int s = 0; s < kOptSegments; ++s) {
        const int k = i - first;
        if (k >= 0 && k < a.len[s]) {
            pp = a.p[s] + k;
            gp = a.g[s] + k;
        }
        first += a.len[s];
    }
    float p = 0.0f, grad = 0.0f, m = 0.0f, v = 0.0f;
    if (own) {
        p = *pp;
        grad = *gp;
        m = a.m[i];
        v = a.v[i];
    }

    // the whole norm, in every group
    double acc = 0.0;
#pragma unroll
    for (int s = 0; s < kOptSegments; ++s) {
        const float* g = a.g[s];
        const int n = a.len[s];
        for (int k0 = tid; k0 < n; k0 += kOptChunk * kOptThreads) {
            float x[kOptChunk];
#pragma unroll
            for (int c = 0; c < kOptChunk; ++c) {
                const int k = k0 + c * kOptThreads;
                x[c] = k < n ? g[k] : 0.0f;
            }
#pragma unroll
            for (int c = 0; c < kOptChunk; ++c) acc += (double)x[c] * (double)x[c];
        }
    }
    const double w = wave_sum_(acc);
    if (lane == 0) red[wave] = w;
    __syncthreads();
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < kOptThreads / 64; ++k) sum += red[k];
    const float norm = (float)sqrt(sum);
    const float coef = a.max_grad_norm > 0.0f ? fminf(1.0f, a.max_grad_norm / (norm + 1e-6f)) : 1.0f;
    if (a.stats && blockIdx.x == 0 && tid == 0) {
        a.stats[0] = norm;
        a.stats[1] = coef;
    }

    if (own) {
        // include/dockauv.h (dockauv_optim_step) states this order; -ffp-contract=on fuses nothing but the fmaf written here
        const float g = grad * coef;
        m = fmaf(a.c1, g - m, m);
        const float bv = a.b2 * v;
        v = fmaf(a.c2 * g, g, bv);
        const float denom = fmaf(sqrtf(v), A::kCtl ? ctl_rsq : a.rsq, a.eps);
        const float upd = (A::kCtl ? ctl_step_size : a.step_size) * (m / denom);
        *pp = p - upd;
        a.m[i] = m;
        a.v[i] = v;
    }
}

}  // namespace

namespace {

// groups of the launch, 0: the arguments do not describe one index space
unsigned adam_groups(const AdamArgs& a) {
    long total = 0;
    for (int s = 0; s < kOptSegments; ++s) {
        if (a.len[s] < 0 || (a.len[s] > 0 && (!a.p[s] || !a.g[s]))) return 0;
        total += a.len[s];
    }
    if (total < 1 || total != (long)a.total || !a.m || !a.v) return 0;
    return (unsigned)((total + kOptThreads - 1) / kOptThreads);
}

}  // namespace

int launch_adam_step(const AdamArgs& a, void* stream) {
    const unsigned groups = adam_groups(a);
    if (!groups) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(adam_step_kernel<AdamArgs>, dim3(groups), dim3(kOptThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_adam_step_ctl(const AdamArgs& a, const OptimCtl* ctl, void* stream) {
    const unsigned groups = adam_groups(a);
    if (!groups || !ctl) return (int)hipErrorInvalidValue;
    AdamArgsCtl x;
    static_cast<AdamArgs&>(x) = a;
    x.ctl = ctl;
    hipLaunchKernelGGL(adam_step_kernel<AdamArgsCtl>, dim3(groups), dim3(kOptThreads), 0, (hipStream_t)stream, x);
    return (int)hipGetLastError();
}

}  // namespace dockauv
