// dockauv_replay.hip -- the replay buffer's kernels for gfx950 (MI355X): the push that scatters K x N transitions into the ring
// and the sample that gathers G x B of them through indices it derives from Philox (include/dockauv.h: dockauv_replay_*; the
// reference's counterparts are SB3 1.5's ReplayBuffer.add / .sample behind train.py with MODEL = SAC).
//
// Shape, both kernels: a team of kReplayTeam = 16 lanes per record, four records per wave, sixteen per group of 256.  A record
// is 52 .. 84 floats (208 .. 336 bytes) at the shipped configs and starts on a 16-byte boundary, so the record side moves as
// 16-byte words, lane l of the team the words l and l + 16: a team's access is one contiguous run of up to 256 bytes, a wave's
// four such runs.  The other side -- the packed rows of a rollout (88 or 152 bytes apart: 8-byte aligned at best), the terminal
// observations, the actions, the sample's outputs -- moves as 4-byte words: which source serves a word depends on the word's
// place in the record, not on the lane, and consecutive lanes touch consecutive words of the same row, so the accesses coalesce
// as they stand.  Every word is moved as a uint32: a copy, whatever its bits (NaN payloads, -0.0f).
// Nothing here waits on another lane, there is no LDS, no atomic: a record is written by one team and read by one team.
// The push writes the carry buffer it does NOT read (dockauv_capi_replay.hip alternates the two), so the launch has no lane
// that reads what another writes.  All offsets into the ring are 64-bit (dockauv_replay.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dockauv_device.h"
#include "dockauv_replay.h"

namespace dockauv {
namespace {

constexpr int kTeams = kReplayThreads / kReplayTeam;

__global__ __launch_bounds__(kReplayThreads) void replay_sync_kernel(const uint32_t* __restrict__ rows, uint32_t* __restrict__ carry,
                                                                      int n_envs, int n_obs) {
    const long long i = (long long)blockIdx.x * kReplayThreads + threadIdx.x;
    if (i >= (long long)n_envs * n_obs) return;
    const long long env = i / n_obs;
    const int j = (int)(i - env * n_obs);
    carry[i] = rows[(size_t)env * (size_t)(n_obs + 2) + j];
}

__global__ __launch_bounds__(kReplayThreads) void replay_push_kernel(const ReplayPushArgs a) {
    const long long rec = (long long)blockIdx.x * kTeams + (threadIdx.x / kReplayTeam);   // k * N + env
    const int lane = threadIdx.x % kReplayTeam;
    if (rec >= (long long)a.n_steps * a.n_envs) return;
    const int k = (int)(rec / a.n_envs), env = (int)(rec - (long long)k * a.n_envs);
    const int n_obs = a.n_obs, stride = n_obs + 2;
    const float* rowf = a.rows_out + (size_t)rec * (size_t)stride;
    const uint32_t* row = (const uint32_t*)rowf;
    const bool done = rowf[n_obs + 1] > 0.5f;
    // what the step read: the row before, or for step 0 rows_in / the carry
    const uint32_t* obs = k == 0 ? (const uint32_t*)a.obs0 + (size_t)env * (size_t)a.obs0_stride : row - (size_t)a.n_envs * (size_t)stride;
    // terminal_obs and ep_outcome are read only where done: elsewhere they hold whatever they held before
    const uint32_t* nxt = done ? (const uint32_t*)a.terminal_obs + (size_t)rec * (size_t)n_obs : row;
    const uint32_t* act = (const uint32_t*)a.actions + (size_t)rec * (size_t)a.n_u;
    bool timeout = false;
    if (done && a.ep_outcome) timeout = a.ep_outcome[rec] == 3;
    long long slot = a.pos + k;   // pos < capacity_steps and k < K <= capacity_steps: one wrap at most
    if (slot >= a.capacity_steps) slot -= a.capacity_steps;
    uint4* dst = (uint4*)(a.storage + replay_record_offset(replay_record_index(slot, a.n_envs, env), a.record_floats));
    const int o1 = n_obs, o2 = 2 * n_obs, o3 = o2 + a.n_u;
    const uint32_t one = __float_as_uint(1.0f);
    for (int c = lane; c < a.record_floats / 4; c += kReplayTeam) {
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = 4 * c + j;
            uint32_t w = 0u;   // (the padding)
            if (p < o1) w = obs[p];
            else if (p < o2) w = nxt[p - o1];
            else if (p < o3) w = act[p - o2];
            else if (p == o3) w = row[n_obs];
            else if (p == o3 + 1) w = done ? one : 0u;
            else if (p == o3 + 2) w = timeout ? one : 0u;
            v[j] = w;
        }
        dst[c] = make_uint4(v[0], v[1], v[2], v[3]);
    }
    if (k == a.n_steps - 1) {
        uint32_t* carry = (uint32_t*)a.carry_out + (size_t)env * (size_t)n_obs;
        for (int j = lane; j < n_obs; j += kReplayTeam) carry[j] = row[j];
    }
}

__global__ __launch_bounds__(kReplayThreads) void replay_sample_kernel(const ReplaySampleArgs a) {
    const long long rec = (long long)blockIdx.x * kTeams + (threadIdx.x / kReplayTeam);   // g * B + b
    const int lane = threadIdx.x % kReplayTeam;
    if (rec >= (long long)a.n_batches * a.batch_size) return;
    const long long g = rec / a.batch_size, b = rec - g * a.batch_size;
    // every lane of the team derives the index itself: ten rounds of integer work against a shuffle and a dependency on lane 0
    const uint64_t d = a.draws + (uint64_t)g;
    uint32_t c[4] = {(uint32_t)b, (uint32_t)d, (uint32_t)(d >> 32), kReplayStream};
    philox4x32_10_(c, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
    const uint32_t step = replay_mulshift(c[0], a.size), env = replay_mulshift(c[1], (uint32_t)a.n_envs);
    const unsigned long long record = replay_record_index((long long)step, a.n_envs, (int)env);
    const uint32_t* src1 = (const uint32_t*)a.storage + replay_record_offset(record, a.record_floats);
    const uint4* src = (const uint4*)src1;
    const int n_obs = a.n_obs, n_u = a.n_u;
    const int o1 = n_obs, o2 = 2 * n_obs, o3 = o2 + n_u;
    uint32_t* obs = (uint32_t*)a.obs + (size_t)rec * (size_t)n_obs;
    uint32_t* nxt = (uint32_t*)a.next_obs + (size_t)rec * (size_t)n_obs;
    uint32_t* act = (uint32_t*)a.actions + (size_t)rec * (size_t)n_u;
    for (int q = lane; q < a.record_floats / 4; q += kReplayTeam) {
        const uint4 v4 = src[q];
        const uint32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = 4 * q + j;
            if (p < o1) obs[p] = v[j];
            else if (p < o2) nxt[p - o1] = v[j];
            else if (p < o3) act[p - o2] = v[j];
            else if (p == o3) ((uint32_t*)a.rewards)[rec] = v[j];
            else if (p == o3 + 1) {
                // done * (1 - timeout), both exactly 0.0f or 1.0f; the timeout word may sit in the next 16-byte word
                const float t = __uint_as_float(src1[o3 + 2]);
                a.dones[rec] = __uint_as_float(v[j]) * (1.0f - t);
            }
        }
    }
    if (lane == 0 && a.index) a.index[rec] = (long long)record;
}

}  // namespace

int launch_replay_sync(const float* rows, float* carry, int n_envs, int n_obs, void* stream) {
    if (n_envs < 1 || n_obs < 1) return (int)hipErrorInvalidValue;
    const long long n = (long long)n_envs * n_obs;
    const long long groups = (n + kReplayThreads - 1) / kReplayThreads;
    if (groups > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(replay_sync_kernel, dim3((unsigned)groups), dim3(kReplayThreads), 0, (hipStream_t)stream,
                       (const uint32_t*)rows, (uint32_t*)carry, n_envs, n_obs);
    return (int)hipGetLastError();
}

int launch_replay_push(const ReplayPushArgs& a, void* stream) {
    if (a.n_steps < 1 || a.n_envs < 1 || a.n_obs < 1 || a.n_u < 1 || a.record_floats != replay_record_floats(a.n_obs, a.n_u) ||
        a.n_steps > a.capacity_steps || a.pos < 0 || a.pos >= a.capacity_steps)
        return (int)hipErrorInvalidValue;
    const long long groups = ((long long)a.n_steps * a.n_envs + kTeams - 1) / kTeams;
    if (groups > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(replay_push_kernel, dim3((unsigned)groups), dim3(kReplayThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_replay_sample(const ReplaySampleArgs& a, void* stream) {
    if (a.n_batches < 1 || a.batch_size < 1 || a.size < 1 || a.n_envs < 1 || a.record_floats != replay_record_floats(a.n_obs, a.n_u))
        return (int)hipErrorInvalidValue;
    const long long groups = ((long long)a.n_batches * a.batch_size + kTeams - 1) / kTeams;
    if (groups > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(replay_sample_kernel, dim3((unsigned)groups), dim3(kReplayThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace dockauv
