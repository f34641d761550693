// dockauv_replay.h -- what the replay buffer's kernels (dockauv_replay.hip) and its entry points (dockauv_capi_replay.hip) share:
// the record layout of include/dockauv.h (dockauv_replay_*) and the launchers.  Plain C++: a host compiler can include it
// (tests/replay_offset_host.cpp pins the 64-bit offsets on a CPU).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DOCKAUV_REPLAY_HD __host__ __device__
#else
#define DOCKAUV_REPLAY_HD
#endif

namespace dockauv {

constexpr uint32_t kReplayStream = 4u;   // Philox counter word 3 of the sample indices (0 .. 3: dockauv_device.h)
constexpr int kReplayTeam = 16;          // lanes per record: four records per wave
constexpr int kReplayThreads = 256;      // sixteen records per group

// floats of one record: [obs | next_obs | action | reward | done | timeout | 0 ..], a multiple of 4
DOCKAUV_REPLAY_HD inline int replay_record_floats(int n_obs, int n_u) { return (2 * n_obs + n_u + 3 + 3) & ~3; }

// the record of (step slot s, env i) is record number s * n_envs + i; where it starts, in floats and in bytes.  The ring may
// exceed 4 GiB (config 3's 65 536 envs x 128 steps x 84 floats are 2.8 GB, 256 steps 5.6 GB): 64-bit, every factor widened first
DOCKAUV_REPLAY_HD inline unsigned long long replay_record_index(long long step_slot, int n_envs, int env) {
    return (unsigned long long)step_slot * (unsigned long long)n_envs + (unsigned long long)env;
}
DOCKAUV_REPLAY_HD inline unsigned long long replay_record_offset(unsigned long long record, int record_floats) {
    return record * (unsigned long long)record_floats;
}
DOCKAUV_REPLAY_HD inline unsigned long long replay_record_byte_offset(unsigned long long record, int record_floats) {
    return replay_record_offset(record, record_floats) * 4ull;
}

// (x * n) >> 32: a word of Philox to [0, n), n < 2^32
DOCKAUV_REPLAY_HD inline uint32_t replay_mulshift(uint32_t x, uint32_t n) { return (uint32_t)(((uint64_t)x * (uint64_t)n) >> 32); }

struct ReplayPushArgs {
    float* storage;                 // the ring
    const float* obs0;              // what step 0 read: rows_in (stride n_obs + 2) or the carry (stride n_obs)
    int obs0_stride;
    const float* rows_out;          // [K][N][n_obs + 2]
    const float* actions;           // [K][N][n_u]
    const float* terminal_obs;      // [K][N][n_obs]
    const uint8_t* ep_outcome;      // nullable [K][N]
    float* carry_out;               // [N][n_obs]: the other carry buffer
    int n_steps, n_envs, n_obs, n_u, record_floats;
    long long pos, capacity_steps;
};

struct ReplaySampleArgs {
    const float* storage;
    float *obs, *actions, *next_obs, *rewards, *dones;
    long long* index;               // nullable
    long long batch_size;
    int n_batches, n_envs, n_obs, n_u, record_floats;
    uint32_t size;                  // step slots filled, >= 1
    uint64_t seed, draws;
};

// dockauv_replay.hip; each returns a hipError_t as int
int launch_replay_sync(const float* rows, float* carry, int n_envs, int n_obs, void* stream);
int launch_replay_push(const ReplayPushArgs& a, void* stream);
int launch_replay_sample(const ReplaySampleArgs& a, void* stream);

}  // namespace dockauv
