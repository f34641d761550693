// Host build of the replay ring's record arithmetic (gym_dockauv_amd/csrc/dockauv_replay.h), for tests/test_replay_host.py: the
// functions the push and sample kernels call to find a record, compiled by a host compiler and asked for offsets beyond 2^32.
// Arguments: record record_floats  -> "<offset in floats> <offset in bytes>";  slot n_envs env -> "<record>" with "index" first;
// "floats" n_obs n_u -> record_floats;  "mulshift" x n -> (x * n) >> 32.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dockauv_replay.h"

int main(int argc, char** argv) {
    using namespace dockauv;
    if (argc == 4 && !std::strcmp(argv[1], "floats")) {
        std::printf("%d\n", replay_record_floats(std::atoi(argv[2]), std::atoi(argv[3])));
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "mulshift")) {
        std::printf("%u\n", replay_mulshift((uint32_t)std::strtoull(argv[2], nullptr, 10), (uint32_t)std::strtoull(argv[3], nullptr, 10)));
        return 0;
    }
    if (argc == 5 && !std::strcmp(argv[1], "index")) {
        std::printf("%llu\n", replay_record_index(std::atoll(argv[2]), std::atoi(argv[3]), std::atoi(argv[4])));
        return 0;
    }
    if (argc == 3) {
        const unsigned long long record = std::strtoull(argv[1], nullptr, 10);
        const int rf = std::atoi(argv[2]);
        std::printf("%llu %llu\n", replay_record_offset(record, rf), replay_record_byte_offset(record, rf));
        return 0;
    }
    return 2;
}
