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
//
// The truncation bootstrap (include/dockauv.h: dockauv_truncation_scan, dockauv_gae_truncated; SB3's collect_rollouts adds
// gamma V(terminal_observation) to the reward of a step that ended on the time limit) is two kernels of the same shape: a forward
// scan that leaves every env's truncated steps in per-env slots, and the GAE kernel instantiated on those slots.  Between the two
// the critic's indexed rows kernel (dockauv_policy.hip) evaluates the slots' terminal observations.
//
// GAE on normalised rewards (include/dockauv.h: dockauv_gae_normalized): the same kernel instantiated twice more, with and without
// the slots, on argument blocks whose reward is a [K][N] column (Args::kColumn: one coalesced load a step in place of the rows'
// reward word).  A trait, not a run-time branch: the two instantiations on the rows are the code they were.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dockauv_device.h"

namespace dockauv {
namespace {

constexpr int kGaeThreads = 64;   // one wave per group: 65 536 envs are 1 024 groups, spread over every CU
constexpr int kGaeChunk = 8;      // steps whose loads are in flight together
constexpr int kGaePairs = kGaeChunk / 2;   // truncated steps a chunk can hold: a truncated episode has max_timesteps + 1 >= 2 steps

struct GaeArgs {
    static constexpr bool kTrunc = false;   // (what the kernel is instantiated on: dockauv_gae's own)
    static constexpr bool kColumn = false;
    const float* rows;            // [K][N][row_stride]
    const float* values;          // [K + 1][N]
    float* advantages;            // [K][N]
    float* returns;               // [K][N]
    int n_steps, n_envs, n_obs, row_stride;
    float gamma, gae_lambda;
};
struct GaeArgsTrunc : GaeArgs {   // dockauv_gae_truncated: the scan's slot table and the values of its rows
    static constexpr bool kTrunc = true;
    const int32_t* trunc_step;    // [n_slots][N], ascending per env, -1 in unused slots
    const float* v_terminal;      // [n_slots][N]
    int n_slots;
};
// dockauv_gae_normalized: the reward of step k comes from reward_col [K][N] (dockauv_rewnorm_scan's reward_norm), not from the
// rows' reward word; the done word still comes from the rows
struct GaeArgsCol : GaeArgs {
    static constexpr bool kColumn = true;
    const float* reward_col;
};
struct GaeArgsTruncCol : GaeArgsTrunc {
    static constexpr bool kColumn = true;
    const float* reward_col;
};

// Args::kTrunc: the lane's slots are counted once (n_slots coalesced loads in front of the first chunk); `pend` is the slot of
// the latest truncated step not yet passed.  The kGaePairs slots from `pend` downwards are requested with the chunk's other
// loads, unconditionally (below slot 0: slot 0 again, marked unused) and at addresses that depend on `pend` alone, so the chain
// never waits for a lookup; a step is truncated iff one of them names it.
template <class Args>
__global__ __launch_bounds__(kGaeThreads) void gae_kernel(const Args a) {
    const int env = blockIdx.x * kGaeThreads + threadIdx.x;
    if (env >= a.n_envs) return;
    const size_t N = (size_t)a.n_envs, stride = (size_t)a.row_stride;
    const float* rd = a.rows + (size_t)env * stride + (size_t)a.n_obs;   // reward word of (step 0, env); step k: + k N stride
    const float gl = a.gamma * a.gae_lambda;
    float v_next = a.values[(size_t)a.n_steps * N + (size_t)env];
    float gae = 0.0f;
    [[maybe_unused]] int pend = -1;
    if constexpr (Args::kTrunc) {
        for (int s = 0; s < a.n_slots; ++s) pend += a.trunc_step[(size_t)s * N + (size_t)env] >= 0 ? 1 : 0;
    }
    for (int k0 = a.n_steps - 1; k0 >= 0; k0 -= kGaeChunk) {
        float r[kGaeChunk], d[kGaeChunk], v[kGaeChunk];
        [[maybe_unused]] int tk[kGaePairs];
        [[maybe_unused]] float tv[kGaePairs];
#pragma unroll
        for (int j = 0; j < kGaeChunk; ++j) {
            const int k = k0 - j > 0 ? k0 - j : 0;      // (below step 0: step 0 again, dropped by the loop below)
            const float* p = rd + (size_t)k * N * stride;
            if constexpr (Args::kColumn) r[j] = a.reward_col[(size_t)k * N + (size_t)env];
            else r[j] = p[0];
            d[j] = p[1];
            v[j] = a.values[(size_t)k * N + (size_t)env];
        }
        if constexpr (Args::kTrunc) {
#pragma unroll
            for (int i = 0; i < kGaePairs; ++i) {
                const int s = pend - i;
                const size_t o = (size_t)(s > 0 ? s : 0) * N + (size_t)env;
                const int t = a.trunc_step[o];
                tv[i] = a.v_terminal[o];
                tk[i] = s >= 0 ? t : -1;
            }
            // the slots are ascending and all pending ones lie at or below k0: those inside the chunk are passed by its end
#pragma unroll
            for (int i = 0; i < kGaePairs; ++i) pend -= (tk[i] >= 0 && tk[i] > k0 - kGaeChunk) ? 1 : 0;
        }
#pragma unroll
        for (int j = 0; j < kGaeChunk; ++j) {
            const int k = k0 - j;
            if (k >= 0) {
                // include/dockauv.h (dockauv_gae, dockauv_gae_truncated) states this order; -ffp-contract=on fuses nothing but
                // the fmaf written here
                const float nt = d[j] > 0.5f ? 0.0f : 1.0f;
                const float gnt = a.gamma * nt;
                float rb = r[j];
                if constexpr (Args::kTrunc) {
#pragma unroll
                    for (int i = 0; i < kGaePairs; ++i) rb = tk[i] == k ? fmaf(a.gamma, tv[i], r[j]) : rb;
                }
                const float delta = fmaf(gnt, v_next, rb) - v[j];
                gae = fmaf(gl * nt, gae, delta);
                const size_t o = (size_t)k * N + (size_t)env;
                a.advantages[o] = gae;
                a.returns[o] = gae + v[j];
                v_next = v[j];
            }
        }
    }
}

// One lane per env walks its K steps forwards, the load shape monitor_scan_kernel's (dockauv_monitor.hip): the done words of a
// chunk requested together and unconditionally -- a chunk that reaches past step K - 1 reads step K - 1 again and drops the
// result --, 64-bit offsets, lanes >= N neither read nor write.  The rule is the monitor's outcome 3 with the same comparisons;
// its length test comes first, so that only a done at the time limit loads the three words of its terminal observation.  A slot
// index is checked against n_slots before every store (a carry above max_timesteps could otherwise pass the bound).
__global__ __launch_bounds__(kGaeThreads) void truncation_scan_kernel(const TruncArgs a) {
    const int env = blockIdx.x * kGaeThreads + threadIdx.x;
    if (env >= a.n_envs) return;
    const size_t N = (size_t)a.n_envs, stride = (size_t)a.row_stride;
    const float* dn = a.rows + (size_t)env * stride + (size_t)a.n_obs + 1;   // done word of (step 0, env); step k: + k N stride
    int c_len = a.carry_len[env];
    int slot = 0;
    for (int k0 = 0; k0 < a.n_steps; k0 += kGaeChunk) {
        float d[kGaeChunk];
#pragma unroll
        for (int j = 0; j < kGaeChunk; ++j) {
            const int k = k0 + j < a.n_steps ? k0 + j : a.n_steps - 1;   // (past the last step: that step again, dropped below)
            d[j] = dn[(size_t)k * N * stride];
        }
#pragma unroll
        for (int j = 0; j < kGaeChunk; ++j) {
            const int k = k0 + j;
            if (k < a.n_steps) {
                const int len = c_len + 1;
                if (d[j] > 0.5f) {
                    if (len > a.max_timesteps) {
                        const size_t o = (size_t)k * N + (size_t)env;
                        const float* to = a.terminal_obs + o * (size_t)a.n_obs;
                        const float t0 = to[0], t6 = to[6], t7 = to[7];
                        const bool lower = t0 == 0.0f || t0 == 1.0f || fabsf(t6) == 1.0f || fabsf(t7) == 1.0f;
                        if (!lower && slot < a.n_slots) {
                            const size_t w = (size_t)slot * N + (size_t)env;
                            a.trunc_step[w] = k;
                            a.trunc_row[w] = (long long)o;
                            slot += 1;
                        }
                    }
                    c_len = 0;
                } else {
                    c_len = len;
                }
            }
        }
    }
    for (; slot < a.n_slots; ++slot) {
        const size_t w = (size_t)slot * N + (size_t)env;
        a.trunc_step[w] = -1;
        a.trunc_row[w] = (long long)env;   // (step 0's row: valid to read, its value is never used)
    }
    a.carry_len[env] = c_len;
}

}  // namespace

namespace {

template <class Args>
int launch_gae_on(const Args& a, void* stream) {
    const unsigned groups = (unsigned)((a.n_envs + kGaeThreads - 1) / kGaeThreads);
    hipLaunchKernelGGL(gae_kernel<Args>, dim3(groups), dim3(kGaeThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace

int launch_gae(const GaeLaunch& g, void* stream) {
    if (g.n_steps < 1 || g.n_envs < 1 || g.n_obs < 1 || (g.trunc_step && g.n_slots < 1)) return (int)hipErrorInvalidValue;
    const GaeArgs rows{g.rows, g.values, g.advantages, g.returns, g.n_steps, g.n_envs, g.n_obs, g.n_obs + 2, g.gamma, g.gae_lambda};
    const GaeArgsTrunc slots{rows, g.trunc_step, g.v_terminal, g.n_slots};
    if (!g.reward_col) return !g.trunc_step ? launch_gae_on(rows, stream) : launch_gae_on(slots, stream);
    return g.trunc_step ? launch_gae_on(GaeArgsTruncCol{slots, g.reward_col}, stream) : launch_gae_on(GaeArgsCol{rows, g.reward_col}, stream);
}

int launch_truncation_scan(const TruncArgs& a, void* stream) {
    if (a.n_steps < 1 || a.n_envs < 1 || a.n_obs < 8 || a.n_slots < 1 || a.max_timesteps < 1) return (int)hipErrorInvalidValue;
    const unsigned groups = (unsigned)((a.n_envs + kGaeThreads - 1) / kGaeThreads);
    hipLaunchKernelGGL(truncation_scan_kernel, dim3(groups), dim3(kGaeThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace dockauv
