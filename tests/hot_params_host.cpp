// CPU check of the packed hot block (gym_dockauv_amd/csrc/dockauv_device.h: HotP, pack_hot): every EnvP / VehicleP field
// element gets a value of its own, the block is packed, and every slot must hold the bits of its source.  Prints one line
// per failure and "ok <checked slots>" at the end; tests/test_hot_params_host.py compiles and runs it.
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "dockauv_device.h"

using namespace dockauv;

static int failures = 0;

template <typename T>
static bool same_bits(const T& a, const T& b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

template <typename T>
static void expect(const char* what, int i, const T& got, const T& want, int& checked) {
    ++checked;
    if (!same_bits(got, want)) {
        std::printf("FAIL %s[%d]: %.9g != %.9g\n", what, i, (double)got, (double)want);
        ++failures;
    }
}

// every T-sized word of a parameter struct gets its own value (integers included: they are overwritten where it matters)
template <typename T, typename S>
static void fill_distinct(S& s, double first) {
    T words[sizeof(S) / sizeof(T)];
    for (size_t i = 0; i < sizeof(S) / sizeof(T); ++i) words[i] = (T)(first + 0.37 * (double)i);
    std::memset(&s, 0, sizeof(S));
    std::memcpy(&s, words, sizeof(words));
}

template <typename T>
static int check_vehicle(const char* name, int n_u, bool diagonal_b) {
    ParamBlock<T, 2> P;
    fill_distinct<T>(P.E, 1000.0);
    for (int v = 0; v < 2; ++v) {
        fill_distinct<T>(P.V[v], 3000.0 + 1000.0 * v);
        P.V[v].n_u = n_u;
        if (diagonal_b)
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < kMaxU; ++j)
                    if (i != j) P.V[v].B[i * kMaxU + j] = (T)0;
        std::memset(&P.H[v], 0xff, sizeof(P.H[v]));
        pack_hot(P.H[v], P.E, P.V[v]);
    }
    int checked = 0;
    for (int v = 0; v < 2; ++v) {
        const HotP<T>& H = P.H[v];
        const VehicleP<T>& V = P.V[v];
        expect("lp_alpha", v, H.lp_alpha, P.E.lp_alpha, checked);
        expect("mu", v, H.mu, P.E.mu, checked);
        expect("h", v, H.h, P.E.h, checked);
        for (int i = 0; i < kMaxU; ++i) {
            expect("w_act", i, H.w_act[i], P.E.w_act[i], checked);
            expect("ulo", i, H.ulo[i], V.ulo[i], checked);
            expect("uhalf", i, H.uhalf[i], V.uhalf[i], checked);
        }
        for (int i = 0; i < 6; ++i) {
            expect("bdiag", i, H.bdiag[i], V.B[i * kMaxU + i], checked);
            expect("dl", i, H.dl[i], V.dl[i], checked);
            expect("dq", i, H.dq[i], V.dq[i], checked);
        }
        const int minv[10] = {0, 4, 7, 9, 14, 19, 21, 24, 28, 35};   // the entries kinetics_ reads (SYM)
        for (int i = 0; i < 10; ++i) {
            expect("kc", i, H.kc[i], V.kc[i], checked);
            expect("minv", i, H.minv[i], V.Minv[minv[i]], checked);
            if (minv_sym(i) != minv[i]) { std::printf("FAIL minv_sym(%d)\n", i); ++failures; }
        }
        expect("gWB", v, H.gWB, V.gWB, checked);
        expect("gz", v, H.gz, V.gz, checked);
        for (int i = 0; i < L_COUNT; ++i) expect("lauv", i, H.lauv[i], V.lauv[i], checked);
    }
    // all slots of the block are accounted for: nothing but padding is left
    const size_t slots = 3 + 3 * kMaxU + 3 * 6 + 2 * 10 + 2 + L_COUNT;
    if ((size_t)checked != 2 * slots || slots * sizeof(T) > sizeof(HotP<T>) || sizeof(HotP<T>) - slots * sizeof(T) >= 64) {
        std::printf("FAIL %s: %d slots checked, %zu expected, block of %zu bytes\n", name, checked, 2 * slots, sizeof(HotP<T>));
        ++failures;
    }
    // layout: whole 64-byte lines at 64-byte offsets of the parameter block
    typedef ParamBlock<T, 2> PB;
    const size_t off = offsetof(PB, H);
    if (sizeof(HotP<T>) % 64 || alignof(HotP<T>) != 64 || off % 64 || sizeof(PB) % 64 || off < sizeof(EnvP<T>) + 2 * sizeof(VehicleP<T>)) {
        std::printf("FAIL %s: sizeof(HotP) %zu, alignof %zu, offset %zu, sizeof(ParamBlock) %zu\n", name, sizeof(HotP<T>),
                    alignof(HotP<T>), off, sizeof(PB));
        ++failures;
    }
    std::printf("%s: %d slots, HotP %zu bytes at offset %zu of %zu\n", name, checked, sizeof(HotP<T>), off, sizeof(PB));
    return checked;
}

int main() {
    int n = 0;
    n += check_vehicle<float>("f32 six inputs, diagonal B", 6, true);
    n += check_vehicle<float>("f32 LAUV", 3, false);
    n += check_vehicle<double>("f64 six inputs, diagonal B", 6, true);
    n += check_vehicle<double>("f64 LAUV", 3, false);
    if (failures) return 1;
    std::printf("ok %d\n", n);
    return 0;
}
