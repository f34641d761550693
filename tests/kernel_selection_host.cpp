// Prints the kernel-selection table of gym_dockauv_amd/csrc/dockauv_device.h (select_step, select_sequence,
// choose_threads) over a fixed grid: host code only, built and compared with tests/golden/kernel_selection.txt by
// tests/test_kernel_selection_host.py.  With the argument "full": one line per grid point instead of the folded table.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dockauv_device.h"

using namespace dockauv;

namespace {

const char* const kKinds[] = {"plain", "output", "trace", "noise", "pool", "reward2", "term-packed", "term", "ride", "ride-term"};
const char* const kVk[] = {"joy", "denseb", "lauv", "mixed"};
const int kThreads[] = {64, 128, 256, 512}, kEnvs[] = {262144, 262208}, kPads[] = {4, 5, 6};

// request kind k of kKinds: packed float32 rows unless the kind says otherwise
void set_kind(StepRequest& r, int k) {
    r.reset_mode = k == 4 ? 1 : 2;   // DOCKAUV_RESET_POOL : DOCKAUV_RESET_DEVICE
    r.reward_set = k == 5 ? 2 : 1;
    r.extras = k >= 1 && k <= 3;
    r.terminal_obs = k == 6 || k == 7 || k == 9;
    r.pack = k == 7 ? 0 : 1;
    r.ride = k >= 8;
}

// step "NT" + L(OG) T(ERM) W(rite-back) R(ide kernel) X(not supported), "/", sequence "NT" + W or "-" (step by step)
std::string cell(const StepRequest& r) {
    const StepVariant s = select_step(r), q = select_sequence(r);
    std::string c = std::to_string(s.NT);
    if (s.LOG) c += 'L';
    if (s.TERM) c += 'T';
    if (s.WB) c += 'W';
    if (s.ride) c += 'R';
    if (s.unsupported) c += 'X';
    c += '/';
    if (q.unsupported) return c + '-';
    return c + std::to_string(q.NT) + (q.WB ? "W" : "");
}

}  // namespace

int main(int argc, char** argv) {
    const bool full = argc > 1 && !strcmp(argv[1], "full");
    printf("# precision kinetics vehicle obstacles request pads | step/sequence at (envs, threads) =");
    for (int n : kEnvs)
        for (int t : kThreads) printf(" (%d, %d)", n, t);
    printf("\n");
    for (int f64 = 0; f64 < 2; ++f64)
        for (int sym = 1; sym >= 0; --sym)
            for (int vk = 0; vk < 4; ++vk)
                for (int rays = 0; rays < 2; ++rays)
                    for (int k = 0; k < 10; ++k) {
                        char key[96];
                        snprintf(key, sizeof key, "%s %s %s %s %s", f64 ? "f64" : "f32", sym ? "sym" : "general", kVk[vk], rays ? "rays" : "none", kKinds[k]);
                        std::vector<std::string> rows, pads;   // the pads that share a row are listed together
                        for (int pad : kPads) {
                            std::string row;
                            for (int n : kEnvs)
                                for (int t : kThreads) {
                                    StepRequest r{};
                                    r.f64 = f64, r.sym = sym, r.vk = vk, r.has_rays = rays, r.threads = t, r.n_envs = n, r.ray_pad_log2 = pad;
                                    set_kind(r, k);
                                    if (full) printf("%s pad%d %d %d %s\n", key, pad, n, t, cell(r).c_str());
                                    row += " " + cell(r);
                                }
                            size_t g = 0;
                            while (g < rows.size() && rows[g] != row) ++g;
                            if (g == rows.size()) rows.push_back(row), pads.push_back("pad");
                            pads[g] += (pads[g].size() > 3 ? "," : "") + std::to_string(pad);
                        }
                        for (size_t g = 0; g < rows.size() && !full; ++g) printf("%s %s |%s\n", key, pads[g].c_str(), rows[g].c_str());
                    }
    // choose_threads: every batch-size boundary and the value just above it
    const int bounds[] = {32768, 65536, 131072, 163840, 196608, 393216, 786432};
    const struct { const char* name; int n_rays, caps, sph; } loads[] = {
        {"none", 63, 0, 0}, {"light", 16, 0, 8}, {"heavy-regrec", 63, 5, 0}, {"heavy", 63, 6, 0}, {"heavy-spheres", 63, 5, 1}};
    printf("# threads: precision workload vehicles threads_per_group | at envs =");
    for (int b : bounds) printf(" %d %d", b, b + 1);
    printf("\n");
    for (int f64 = 0; f64 < 2; ++f64)
        for (const auto& w : loads)
            for (int nv = 1; nv <= 2; ++nv)
                for (int tpg : {0, 128}) {
                    printf("threads %s %s %d %d |", f64 ? "f64" : "f32", w.name, nv, tpg);
                    for (int b : bounds)
                        for (int n : {b, b + 1}) printf(" %d", choose_threads(f64, n, w.n_rays, w.caps, w.sph, nv, tpg));
                    printf("\n");
                }
    // the group shapes tests/test_gpu_fullsize.py::test_group_shape_the_library_picks expects of BASELINE's configs
    // (config 2: no obstacles; 3: 16 beams x 8 spheres; 4: 63 rays x 5 capsules; 5: the same, two vehicles)
    const struct { int cfg, envs; } shapes[] = {{2, 4096}, {2, 131072}, {2, 262144}, {3, 65536}, {3, 262144}, {4, 32768},
                                                {4, 65536}, {4, 196608}, {4, 262144}, {5, 65536}, {5, 262144}, {5, 524288}};
    const auto config_threads = [](bool f64, int cfg, int envs) {
        return choose_threads(f64, envs, cfg == 3 ? 16 : 63, cfg >= 4 ? 5 : 0, cfg == 3 ? 8 : 0, cfg == 5 ? 2 : 1, 0);
    };
    for (const auto& s : shapes) printf("config %d f32 %d -> %d\n", s.cfg, s.envs, config_threads(false, s.cfg, s.envs));
    printf("config 4 f64 262144 -> %d\n", config_threads(true, 4, 262144));
    return 0;
}
