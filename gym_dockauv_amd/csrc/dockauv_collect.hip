// dockauv_collect.hip -- generalised advantage estimation on the packed rows of a rollout, for gfx950 (MI355X)
// (include/dockauv.h: dockauv_gae, dockauv_collect; the reference's counterpart is SB3's RolloutBuffer.
// compute_returns_and_advantage, which train.py:64-71 runs after every collect_rollouts).
//
// One lane per env walks its K steps backwards.  The recurrence gae <- fma(c, gae, delta) is a serial chain, the loads it
// consumes are not: the reward / done words and the values of kGaeChunk steps are requested together, so that a wave waits
// for memory once per chunk and not once per step (a dependent global load costs the better part of a microsecond; the chain
// itself is four VALU instructions per step).  The loads of a chunk are unconditional -- a chunk that reaches below step 0
// reads step 0 again and drops the result -- because a load inside a branch of its own is waited for at the end of that
// branch.  Reward and done are neighbours in a row; the source reads them as two floats and the compiler makes one 8-byte
// load of them for every n_obs (global loads need no 8-byte alignment on gfx950).  The observation columns are never touched;
// lanes >= N neither read nor write; every offset is 64-bit ([K][N][row] passes 2^32 bytes at the workload's sizes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dockauv_device.h"

namespace dockauv {
namespace {

constexpr int kGaeThreads = 64;   // one wave per group: 65 536 envs are 1 024 groups, spread over every CU
constexpr int kGaeChunk = 8;      // steps whose loads are in flight together

struct GaeArgs {
    const float* rows;            // [K][N][row_stride]
    const float* values;          // [K + 1][N]
    float* advantages;            // [K][N]
    float* returns;               // [K][N]
    int n_steps, n_envs, n_obs, row_stride;
    float gamma, gae_lambda;
};

__global__ __launch_bounds__(kGaeThreads) void gae_kernel(const GaeArgs a) {
    const int env = blockIdx.x * kGaeThreads + threadIdx.x;
    if (env >= a.n_envs) return;
    const size_t N = (size_t)a.n_envs, stride = (size_t)a.row_stride;
    const float* rd = a.rows + (size_t)env * stride + (size_t)a.n_obs;   // reward word of (step 0, env); step k: + k N stride
    const float gl = a.gamma * a.gae_lambda;
    float v_next = a.values[(size_t)a.n_steps * N + (size_t)env];
    float gae = 0.0f;
    for (int k0 = a.n_steps - 1; k0 >= 0; k0 -= kGaeChunk) {
        float r[kGaeChunk], d[kGaeChunk], v[kGaeChunk];
#pragma unroll
        for (int j = 0; j < kGaeChunk; ++j) {
            const int k = k0 - j > 0 ? k0 - j : 0;      // (below step 0: step 0 again, dropped by the loop below)
            const float* p = rd + (size_t)k * N * stride;
            r[j] = p[0];
            d[j] = p[1];
            v[j] = a.values[(size_t)k * N + (size_t)env];
        }
#pragma unroll
        for (int j = 0; j < kGaeChunk; ++j) {
            const int k = k0 - j;
            if (k >= 0) {
                // include/dockauv.h (dockauv_gae) states this order; -ffp-contract=on fuses nothing but the fmaf written here
                const float nt = d[j] > 0.5f ? 0.0f : 1.0f;
                const float gnt = a.gamma * nt;
                const float delta = fmaf(gnt, v_next, r[j]) - v[j];
                gae = fmaf(gl * nt, gae, delta);
                const size_t o = (size_t)k * N + (size_t)env;
                a.advantages[o] = gae;
                a.returns[o] = gae + v[j];
                v_next = v[j];
            }
        }
    }
}

}  // namespace

int launch_gae(const float* rows, const float* values, float* advantages, float* returns, int n_steps, int n_envs, int n_obs,
               float gamma, float gae_lambda, void* stream) {
    if (n_steps < 1 || n_envs < 1 || n_obs < 1) return (int)hipErrorInvalidValue;
    GaeArgs a{rows, values, advantages, returns, n_steps, n_envs, n_obs, n_obs + 2, gamma, gae_lambda};
    const unsigned groups = (unsigned)((n_envs + kGaeThreads - 1) / kGaeThreads);
    hipLaunchKernelGGL(gae_kernel, dim3(groups), dim3(kGaeThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace dockauv
