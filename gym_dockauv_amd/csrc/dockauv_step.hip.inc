// dockauv_step.hip.inc -- the fused docking3d step kernel for gfx950 (MI355X); included by dockauv_kernels_f32.hip
// (product) and dockauv_kernels_f64.hip (validation instantiation of the same source).
//
// One launch = BaseDocking3d.step (reference envs/docking3d.py:346-402) for every env of the handle:
//   current speed + body-frame current -> un-normalise + low-pass -> RKF45(4) step of the Fossen 6-DOF model
//   -> angle wrap -> ray fan vs capsules/spheres -> body collision -> navigation errors -> observation
//   -> done conditions -> 13-term reward -> (optional) in-kernel episode reset.
//
// Work decomposition (no MFMA: there is no dense contraction on this path).  A workgroup owns EPG = 64 consecutive
// envs and has NT / 64 waves (DESIGN.md section 3):
//   * wave 0, lane = env, integrates ("env phase"; mixed batches of >= 4 waves: wave 0 the vehicle-0 lanes, wave 1
//     the vehicle-1 lanes): every per-env array is struct-of-arrays in HBM, so lane-consecutive = address-consecutive
//     (256 B / wave instruction; scalar array base + a 32-bit lane offset that carries the row offset, ldgx_); vehicle / reward parameters live in a
//     persistent device block read with scalar loads, prefetched into the scalar cache by the group's idle wave;
//   * the helper waves prefetch the raw obstacle rows into LDS meanwhile, zero the observation tile, and one of them
//     (the resetter) draws the next episode's random numbers;
//   * once the integrating waves have published the new pose, all waves complete the obstacle records in the BODY
//     frame and decide which obstacles any ray of the fan can reach (per-env bit masks);
//   * ray stage: envs whose fan reaches no obstacle get their constants from one lane = env sweep; the others are
//     compacted into a list and take lane = ray passes (an env, or four, per wave pass; compile-time forms for the
//     16- and 64-lane fans), dealt to the waves so that the integrating wave is served last; fans wider than 64
//     rays: lane = env / wave = block-max cell;
//   * tail in up to four roles side by side (navigation-dependent observations + state write-back | the other
//     observations | reset | conditions + reward), observation rows into an LDS tile [EPG][n_obs (+2)]; in the product
//     kernels with four or more waves the roles run in FRONT of the barrier behind the ray stage (EARLY): only the
//     obstacle-avoidance term and a finished env's ray cells wait for the rays; there the integrating wave alone works
//     out navigation errors and done conditions and shares them through LDS (SHARE_NAV);
//   * the whole group streams the tile out row-major (what the learner wants) with 16-B coalesced stores.
// Two instantiations per shape: the PRODUCT kernels (LOG = false) serve the mandatory outputs only; optional inputs /
// outputs, logging, pool resets, reward set 2 and other fan widths run on the full instantiation (dockauv_device.h: select_step).
// Numerics: T = float is the product path; T = double instantiates the same code for validation.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include <stdint.h>

#include "dockauv_device.h"
#include "dockauv_ride.h"

namespace dockauv {

// ------------------------------------------------------------------------------------------ math wrappers
// float: v_sin_f32 / v_cos_f32 (arguments in revolutions; every angle on this path is bounded by a few pi; measured on
// gfx950 over [-4.5, 4.5]: 3.9e-7 / 4.2e-7 max abs error, scripts/micro/trig_acc.hip) -- three issue slots per
// sincos; the post-step rotation uses a bounded-range software sincos (sincos_accurate_: Cody-Waite pi/2 reduction in
// three FMA steps + minimax polynomials; 7e-8 abs, ~25 instructions).  The generic ocml sincosf would inline its
// Payne-Hanek path (64-bit integer multiplies) at each of the 21 call sites.  v_rcp / v_sqrt / v_rsq (1 ulp) stand
// in for the IEEE division / sqrt expansions (~10 instructions each).  double: libm-exact calls.
// bounded-range software sincos: Cody-Waite pi/2 reduction in three FMA steps + minimax polynomials (7e-8 abs)
__device__ __forceinline__ void sincos_accurate_(float a, float& sn, float& cs) {
    const float j = fmaf(a, 0.636619747f, 12582912.f) - 12582912.f;
    a = fmaf(j, -1.57079601e+00f, a);
    a = fmaf(j, -3.13916473e-07f, a);
    a = fmaf(j, -5.39030253e-15f, a);
    const int i = (int)j;
    const float s = a * a;
    float r = 2.86567956e-6f;
    r = fmaf(r, s, -1.98559923e-4f);
    r = fmaf(r, s, 8.33338592e-3f);
    r = fmaf(r, s, -1.66666672e-1f);
    const float si = fmaf(r, a * s, a);
    float c = 2.44677067e-5f;
    c = fmaf(c, s, -1.38877297e-3f);
    c = fmaf(c, s, 4.16666567e-2f);
    c = fmaf(c, s, -5.00000000e-1f);
    c = fmaf(c, s, 1.0f);
    float so = (i & 1) ? c : si;
    float co = (i & 1) ? si : c;
    sn = (i & 2) ? -so : so;
    cs = ((i + 1) & 2) ? -co : co;
}
__device__ __forceinline__ void sincos_accurate_(double x, double& s, double& c) { sincos(x, &s, &c); }
__device__ __forceinline__ void sincos_(float a, float& sn, float& cs) {
    const float r = a * 0.15915494309189535f;
    sn = __builtin_amdgcn_sinf(r);
    cs = __builtin_amdgcn_cosf(r);
}
__device__ __forceinline__ void sincos_(double x, double& s, double& c) { sincos(x, &s, &c); }
__device__ __forceinline__ float rcp_(float x) { return __builtin_amdgcn_rcpf(x); }
// float64: IEEE division.  (Round 1 replaced it by a Newton iteration on v_rcp_f64 and blamed v_div_fmas_f64 / VCC for
// wrong quotients in the register-starved general-path kernels; the cause was the SGPR-spill strategy of that
// translation unit, csrc/build.py: PER_SOURCE_FLAGS, and the expansion is innocent.)
__device__ __forceinline__ double rcp_(double x) { return 1.0 / x; }
__device__ __forceinline__ float div_(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
__device__ __forceinline__ double div_(double a, double b) { return a / b; }
__device__ __forceinline__ float sqrt_(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ double sqrt_(double x) { return sqrt(x); }
__device__ __forceinline__ float rsqrt_(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ double rsqrt_(double x) { return rcp_(sqrt(x)); }
__device__ __forceinline__ float log_(float x) { return __builtin_amdgcn_logf(x) * 0.6931471805599453f; }   // v_log_f32 (log2), 1.7e-7 rel. measured
__device__ __forceinline__ double log_(double x) { return log(x); }
// atan2 for finite arguments: octant reduction + degree-7 minimax polynomial in t^2 for atan(t), t in [0, 1]
// (1.2e-7 max abs error evaluated in float32; ocml's atan2f costs about twice the instructions).  atan2(+-0, +-0)
// follows numpy (0 / pi with the sign of y).
__device__ __forceinline__ float atan2_(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    float t = mn * __builtin_amdgcn_rcpf(mx);
    t = (mx == 0.0f) ? 0.0f : t;
    const float s = t * t;
    float p = -0.004054433666169643f;
    p = fmaf(p, s, 0.021862447261810303f);
    p = fmaf(p, s, -0.05591154843568802f);
    p = fmaf(p, s, 0.09642137587070465f);
    p = fmaf(p, s, -0.139086052775383f);
    p = fmaf(p, s, 0.19946560263633728f);
    p = fmaf(p, s, -0.33329859375953674f);
    p = fmaf(p, s, 0.9999993443489075f);
    float a = p * t;
    a = (ay > ax) ? (1.57079632679489662f - a) : a;
    a = (x < 0.0f || (x == 0.0f && __builtin_signbitf(x))) ? (3.14159265358979324f - a) : a;
    return __builtin_copysignf(a, y);
}
__device__ __forceinline__ double atan2_(double y, double x) { return atan2(y, x); }
__device__ __forceinline__ float floor_(float x) { return floorf(x); }
__device__ __forceinline__ double floor_(double x) { return floor(x); }
__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float abs_(float x) { return fabsf(x); }
__device__ __forceinline__ double abs_(double x) { return fabs(x); }
__device__ __forceinline__ bool isnan_(float x) { return x != x; }
__device__ __forceinline__ bool isnan_(double x) { return x != x; }


// Global-memory access as `global_load/store v, v_off, s[base:base+1]`: the wave-uniform part of the address (array
// base + SoA row offset + the group's first env) is pinned to an SGPR pair with readfirstlane (free on an already
// uniform value, but it stops the optimiser from folding the row offset into the per-lane index, which produces a
// 64-bit per-lane address per access: ~60 VGPRs held from the loads to the stores and ~150 v_lshl_add_u64); the
// per-lane part is the 32-bit element index `lane`.
template <typename P>
__device__ __forceinline__ __attribute__((address_space(1))) P* uniform_(P* p) {
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (__attribute__((address_space(1))) P*)(((uint64_t)hi << 32) | lo);
}
// byte offset of SoA row k: 32-bit arithmetic (one s_mul_i32 or shift + add/addc; the 64-bit product k * S cost five to
// six scalar instructions per row: 77 -> 65 instructions in front of the kernel's first load, ~80 fewer in all; the
// step time did not move measurably, same-box A/B).  dockauv_create guarantees that no row offset of a handle
// reaches 2^32 bytes.
template <typename P>
__device__ __forceinline__ unsigned row_off_(long k, long S) { return (unsigned)k * (unsigned)S * (unsigned)sizeof(P); }
// element `lane` of SoA row k (base already points at the group's first env)
// VOFF: the row offset rides in the per-lane 32-bit offset register (base pair = the array, shared by all its rows;
// rows of equal index share their offset register across arrays) instead of in a per-row SGPR base pair (three scalar
// instructions per row: the integrating wave's ~40 row loads and ~25 row stores spent ~180 instructions on them).
// Same-box A/B: config 3 10.2 -> 9.85 us, config 4 -1 %, config 2 unchanged; the mixed kernel since it stopped spilling
// (round 3, 113 VGPRs) -1.7 %.  Every instantiation uses it.
// AF = access flags of a kernel instantiation: bit 0 (kAfVoff) row offset in the lane offset register, bit 1 (kAfWriteBack)
// plain write-back stores instead of write-through ones (see store_global_)
constexpr int kAfVoff = 1, kAfWriteBack = 2;
template <int AF, typename P>
__device__ __forceinline__ P ldgx_(const P* base, long k, long S, unsigned lane) {
    typedef __attribute__((address_space(1))) const char* gcp;
    constexpr bool VOFF = (AF & kAfVoff) != 0;
    if (VOFF)
        return *reinterpret_cast<__attribute__((address_space(1))) const P*>(
            reinterpret_cast<gcp>(uniform_(reinterpret_cast<const char*>(base))) + (unsigned)(lane * (unsigned)sizeof(P) + row_off_<P>(k, S)));
    return *reinterpret_cast<__attribute__((address_space(1))) const P*>(
        reinterpret_cast<gcp>(uniform_(reinterpret_cast<const char*>(base) + row_off_<P>(k, S))) + lane * (unsigned)sizeof(P));
}
// WRITE-THROUGH stores (round 3).  MI355X has one L2 per XCD, and a kernel's release at its end has to write the dirty
// lines of all eight back before the next kernel of the stream may start: with plain stores a launch that writes 15 MB
// (config 3) spends ~2.5 us there, AFTER its last wave has ended -- a quarter of the event-timed duration
// (scripts/micro/writeback_cost.hip, profiles/r3/writeback_cost.txt; the `nt` hint changes nothing).  Stores at agent
// scope (`sc1`) go through to memory while the kernel is still computing and leave nothing to flush: 0.65 us behind the
// last wave whatever was written.  Every global store of the step kernel's state / outputs is of that kind.  A single
// launch reads nothing of what it has written; the resident sequence kernel does, in its next step, and orders the two itself
// (step_seq_kernel: the inter-step fence, barrier and L1 invalidation).
#ifndef DOCKAUV_WT_STORES
#define DOCKAUV_WT_STORES 1
#endif
// WHEN write-through pays: while every group of the launch is resident at once (BASELINE's batch sizes).  Once a launch runs
// in several rounds of groups (>= 262 144 envs) a wave that ends has to wait for its write-through stores to be acknowledged
// by memory instead of by L2, the groups live longer and the next round starts later: config 3 at 1 048 576 envs 168 -> 191 us.
// The instantiations that only serve such batches (kAfWriteBack) keep plain write-back stores.
template <int AF = 0, typename P>
__device__ __forceinline__ void store_global_(__attribute__((address_space(1))) P* p, P v) {
    if (DOCKAUV_WT_STORES && !(AF & kAfWriteBack))
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        *p = v;
}
template <int AF, typename P, typename V>
__device__ __forceinline__ void stgx_(P* base, long k, long S, unsigned lane, V v) {
    typedef __attribute__((address_space(1))) char* gcp;
    constexpr bool VOFF = (AF & kAfVoff) != 0;
    if (VOFF)
        store_global_<AF>(reinterpret_cast<__attribute__((address_space(1))) P*>(
            reinterpret_cast<gcp>(uniform_(reinterpret_cast<char*>(base))) + (unsigned)(lane * (unsigned)sizeof(P) + row_off_<P>(k, S))), (P)v);
    else
        store_global_<AF>(reinterpret_cast<__attribute__((address_space(1))) P*>(
            reinterpret_cast<gcp>(uniform_(reinterpret_cast<char*>(base) + row_off_<P>(k, S))) + lane * (unsigned)sizeof(P)), (P)v);
}
// 16 bytes of the observation tile: global_store_dwordx4 v_off, v[0:3], s[base] (sc1 = write-through)
typedef float tile_f32x4 __attribute__((ext_vector_type(4)));
template <int AF = 0>
__device__ __forceinline__ void store_tile16_(float* base, unsigned byte_off, const float4& v) {
    const tile_f32x4 r = {v.x, v.y, v.z, v.w};
    if (DOCKAUV_WT_STORES && !(AF & kAfWriteBack))
        asm volatile("global_store_dwordx4 %0, %1, %2 sc1" ::"v"(byte_off), "v"(r), "s"(base) : "memory");
    else
        asm volatile("global_store_dwordx4 %0, %1, %2" ::"v"(byte_off), "v"(r), "s"(base) : "memory");
}
template <typename P>
__device__ __forceinline__ P ldg_(const P* base, long k, long S, unsigned lane) { return ldgx_<0>(base, k, S, lane); }
template <typename P, typename V>
__device__ __forceinline__ void stg_(P* base, long k, long S, unsigned lane, V v) { stgx_<0>(base, k, S, lane, v); }

template <typename T> __device__ __forceinline__ T pi_() { return T(3.14159265358979323846); }
template <typename T> __device__ __forceinline__ T inf_() { return T(INFINITY); }

// np.clip(x, lo, hi): NaN propagates
template <typename T> __device__ __forceinline__ T clip_(T x, T lo, T hi) { return x < lo ? lo : (x > hi ? hi : x); }
// max that propagates NaN like np.max
template <typename T> __device__ __forceinline__ T nanmax_(T a, T b) { return (isnan_(a) || a > b) ? a : b; }

// ssa: ((a + pi) mod 2 pi) - pi in [-pi, pi), Python floor-mod.  utils/geomutils.py:4-11
// An angle already inside [-pi, pi) is returned UNTOUCHED: in float32 the round trip (a + pi) - pi costs up to 2.4e-7 rad
// per call (a + pi lies in [2, 8): ulp 2.4e-7 .. 4.8e-7), and the heading -- which nothing damps -- random-walks by that much
// every step: ~3e-6 rad after 260 steps, which the position then integrates (round 3: this, not "float32 itself", was
// most of the free-running drift against the float64 reference, where the same round trip costs 4e-16;
// oracle/ulp_perturb_reference.py shows what float32 storage alone costs: <= 3e-6 on the observations).
template <typename T>
__device__ __forceinline__ T ssa_(T a) {
    const T two_pi = T(2) * pi_<T>();
    T t = a + pi_<T>();
    T k = floor_(t * (T(1) / two_pi));
    T r = t - k * two_pi;
    r = (r < T(0)) ? r + two_pi : r;
    r = (r >= two_pi) ? r - two_pi : r;
    // (a select, not a branch: an early return here split the integrator's tail into basic blocks and cost the float
    // kernels ~25 VGPRs and their first spills)
    return (a >= -pi_<T>() && a < pi_<T>()) ? a : r - pi_<T>();
}

template <typename T>
struct Trig {
    T sf, cf, st, ct, sp, cp;
};

// post-step attitude: its rotation matrix takes obstacle vectors of up to |p| ~ 25 m into the body frame, where the
// ray tests rely on |d'| = 1 and p' _|_ d' (cancelling terms ~|p|^2): 4e-7 of v_sin/v_cos would show up as ~1e-4 m
template <typename T>
__device__ __forceinline__ Trig<T> trig_accurate_(T phi, T th, T psi) {
    Trig<T> g;
    sincos_accurate_(phi, g.sf, g.cf);
    sincos_accurate_(th, g.st, g.ct);
    sincos_accurate_(psi, g.sp, g.cp);
    return g;
}

template <typename T>
__device__ __forceinline__ Trig<T> trig_(T phi, T th, T psi) {
    Trig<T> g;
    sincos_(phi, g.sf, g.cf);
    sincos_(th, g.st, g.ct);
    sincos_(psi, g.sp, g.cp);
    return g;
}

// R_b^n(Theta), utils/geomutils.py:14-43
template <typename T>
__device__ __forceinline__ void rotmat_(const Trig<T>& g, T R[9]) {
    R[0] = g.cp * g.ct;
    R[1] = -g.sp * g.cf + g.cp * g.st * g.sf;
    R[2] = g.sp * g.sf + g.cp * g.cf * g.st;
    R[3] = g.sp * g.ct;
    R[4] = g.cp * g.cf + g.sf * g.st * g.sp;
    R[5] = -g.cp * g.sf + g.st * g.sp * g.cf;
    R[6] = -g.st;
    R[7] = g.ct * g.sf;
    R[8] = g.ct * g.cf;
}

// v_n = R_b^n(Theta) v_b and v_b = R_b^n(Theta)^T v_n as chains of planar rotations (same value as rotmat_ up to rounding)
template <typename T>
__device__ __forceinline__ void rot_body_to_ned_(const Trig<T>& g, T x, T y, T z, T out[3]) {
    const T y1 = g.cf * y - g.sf * z, z1 = g.sf * y + g.cf * z;            // R_x(phi)
    const T x2 = g.ct * x + g.st * z1, z2 = g.ct * z1 - g.st * x;          // R_y(theta)
    out[0] = g.cp * x2 - g.sp * y1;                                        // R_z(psi)
    out[1] = g.sp * x2 + g.cp * y1;
    out[2] = z2;
}
template <typename T>
__device__ __forceinline__ void rot_ned_to_body_(const Trig<T>& g, T x, T y, T z, T out[3]) {
    const T x1 = g.cp * x + g.sp * y, y1 = g.cp * y - g.sp * x;            // R_z(psi)^T
    const T x2 = g.ct * x1 - g.st * z, z2 = g.st * x1 + g.ct * z;          // R_y(theta)^T
    out[0] = x2;
    out[1] = g.cf * y1 + g.sf * z2;                                        // R_x(phi)^T
    out[2] = g.cf * z2 - g.sf * y1;
}

// ------------------------------------------------------------------------------------------ diagnostic stamps
// -DDOCKAUV_STAMPS builds a diagnostic library (never the product): lane 0 of the first 64 groups records the shader
// clock (s_memtime) at up to 32 points of the kernel into a buffer of its own that no other code reads; the host side
// fetches it with dockauv_debug_read_stamps (only exported by that build).  scripts/stamps.py prints the deltas.
#ifdef DOCKAUV_STAMPS
__device__ unsigned long long g_stamps[64 * 32];
// start / end of EVERY group (first 16 384) on both clocks: s_memrealtime (100 MHz, shared by the XCDs: when does a group
// start and end within the launch) and s_memtime (its life in shader ticks); scripts/span.py
__device__ unsigned long long g_span[16384 * 6];   // per group: (realtime, memtime) at entry, after the first kernarg / parameter words, at the end
#define DOCKAUV_SPAN(i)                                                                                    \
    do {                                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        if ((i) == 2) __builtin_amdgcn_s_waitcnt(0);   /* the group's end: its stores have left */         \
        if (threadIdx.x == 0 && blockIdx.x < 16384) {                                                      \
            g_span[blockIdx.x * 6 + 2 * (i)] = __builtin_amdgcn_s_memrealtime();                           \
            g_span[blockIdx.x * 6 + 2 * (i) + 1] = __builtin_amdgcn_s_memtime();                           \
        }                                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
    } while (0)
// which groups are sampled: every (1 << DOCKAUV_STAMP_SHIFT)-th, the first 64 of those (shift 4 with 1 024 groups: half
// of the groups of XCD 0, whose stamps share one clock -- start and end spread of a launch)
#ifndef DOCKAUV_STAMP_SHIFT
#define DOCKAUV_STAMP_SHIFT 0
#endif
#define DOCKAUV_STAMP_SEL ((blockIdx.x & ((1u << DOCKAUV_STAMP_SHIFT) - 1u)) == 0 && (blockIdx.x >> DOCKAUV_STAMP_SHIFT) < 64)
#define DOCKAUV_STAMP_ROW ((blockIdx.x >> DOCKAUV_STAMP_SHIFT) * 32)
// (sched_barrier: the scheduler must not move the clock read, or the arithmetic it brackets, across the stamp)
#define DOCKAUV_STAMP(i)                                                                                   \
    do {                                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        if (threadIdx.x == 0 && DOCKAUV_STAMP_SEL) g_stamps[DOCKAUV_STAMP_ROW + (i)] = __builtin_amdgcn_s_memtime(); \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
    } while (0)
// the same from lane 0 of the group's SECOND wave (a pure ray-stage wave)
#define DOCKAUV_STAMP_W1(i)                                                                                \
    do {                                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        if (threadIdx.x == 64 && DOCKAUV_STAMP_SEL) g_stamps[DOCKAUV_STAMP_ROW + (i)] = __builtin_amdgcn_s_memtime(); \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
    } while (0)
// every wave of the group stamps slot base + its physical wave index (lane 0 of each wave)
#define DOCKAUV_STAMP_WAVES(base)                                                                          \
    do {                                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        if ((threadIdx.x & 63) == 0 && DOCKAUV_STAMP_SEL) g_stamps[DOCKAUV_STAMP_ROW + (base) + (threadIdx.x >> 6)] = __builtin_amdgcn_s_memtime(); \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
    } while (0)
// stamp once the n values of `arr` exist: the empty asm makes each value opaque at this point, so neither IR-level
// sinking nor the scheduler can move the arithmetic that produces them behind the clock read
#define DOCKAUV_STAMP_PIN(i, arr, n)                                        \
    do {                                                                    \
        _Pragma("unroll") for (int k_ = 0; k_ < (n); ++k_) asm volatile("" : "+v"((arr)[k_])); \
        DOCKAUV_STAMP(i);                                                   \
    } while (0)
#else
#define DOCKAUV_SPAN(i) do { } while (0)
#define DOCKAUV_STAMP(i) do { } while (0)
#define DOCKAUV_STAMP_W1(i) do { } while (0)
#define DOCKAUV_STAMP_WAVES(base) do { } while (0)
#define DOCKAUV_STAMP_PIN(i, arr, n) do { } while (0)
#endif

// ------------------------------------------------------------------------------------------ Fossen RHS
// nu_dot = M^-1 (B(nu) u - D(nu) nu - C(nu) nu - g(eta)),  objects/auvsim.py:152-158, statespace.py:199-397
// SYM = the structure both shipped vehicles have, verified on the host before it is selected (dockauv_capi.hip):
// x_G = y_G = x_B = y_B = 0, diagonal I_b, and hence M^-1 = diagonal + the (u,q) and (v,p) couplings only.  It is
// the same arithmetic with the terms that multiply an exact zero dropped (the parameters are run-time scalars, so
// the compiler cannot drop them itself).  SYM = false evaluates the general expressions.
// VP / EP = VehicleP<T> / EnvP<T> as seen through the constant address space (scalar loads)
// damping force D(nu) nu and control force tau for one vehicle kind:  acc = tau - D(nu) nu
// LAUV: fin force / moment coefficients times the (filtered, per step constant) fin inputs; the stages multiply by u^2
template <typename T, typename VP>
__device__ __forceinline__ void lauv_fin_terms_(const VP& V, const T* u, T tau_c[6]) {
    tau_c[1] = V.lauv[L_Y_uudr] * u[1];
    tau_c[2] = V.lauv[L_Z_uuds] * u[2];
    tau_c[4] = V.lauv[L_M_uuds] * u[2];
    tau_c[5] = V.lauv[L_N_uudr] * u[1];
}
template <typename T, int VK, typename VP>
__device__ __forceinline__ void tau_minus_damping_(const VP& V, const T nu[6], const T tau_c[6], const T* u, T acc[6]) {
    const T u_ = nu[0], v_ = nu[1], w_ = nu[2], p_ = nu[3], q_ = nu[4], r_ = nu[5];
    const T au = abs_(u_), av = abs_(v_), aw = abs_(w_), ap = abs_(p_), aq = abs_(q_), ar = abs_(r_);
    // statespace.py:288-350: D = -(D_L + D_NL |nu|) (diagonal) => -D(nu) nu = +(dl + dq |nu|) nu
    if (VK == VK_LAUV) {
        const auto* L = V.lauv;
        const T uu = u_ * u_;   // LAUV.py:60: fins scale with u**2
        // LAUV.py:69-101: cross terms and lift ~ |u|.  The fin terms coefficient * input are the same in every stage of the
        // step (the filtered input is frozen): tau_c[1], [2], [4], [5] = Y_uudr dr, Z_uuds ds, M_uuds ds, N_uudr dr, combined
        // once by the caller (lauv_fin_terms_)
        acc[0] = u[0] + (V.dl[0] + V.dq[0] * au) * u_;
        acc[1] = tau_c[1] * uu + (V.dl[1] + V.dq[1] * av + L[L_Y_uv] * au) * v_ + (L[L_Y_r] + L[L_Y_rr] * ar + L[L_Y_urf] * au) * r_;
        acc[2] = tau_c[2] * uu + (V.dl[2] + V.dq[2] * aw + L[L_Z_uw] * au) * w_ + (L[L_Z_q] + L[L_Z_qq] * aq + L[L_Z_uqf] * au) * q_;
        acc[3] = (V.dl[3] + V.dq[3] * ap) * p_;
        acc[4] = tau_c[4] * uu + (V.dl[4] + V.dq[4] * aq + L[L_M_uqf] * au) * q_ + (L[L_M_w] + L[L_M_ww] * aw + L[L_M_uw] * au) * w_;
        acc[5] = tau_c[5] * uu + (V.dl[5] + V.dq[5] * ar + L[L_N_urf] * au) * r_ + (L[L_N_v] + L[L_N_vv] * av + L[L_N_uv] * au) * v_;
    } else {
        acc[0] = tau_c[0] + (V.dl[0] + V.dq[0] * au) * u_;
        acc[1] = tau_c[1] + (V.dl[1] + V.dq[1] * av) * v_;
        acc[2] = tau_c[2] + (V.dl[2] + V.dq[2] * aw) * w_;
        acc[3] = tau_c[3] + (V.dl[3] + V.dq[3] * ap) * p_;
        acc[4] = tau_c[4] + (V.dl[4] + V.dq[4] * aq) * q_;
        acc[5] = tau_c[5] + (V.dl[5] + V.dq[5] * ar) * r_;
    }
}

template <typename T, int VK, bool SYM, typename VP>
__device__ __forceinline__ void kinetics_(const VP& V, const T nu[6], const Trig<T>& g, const T tau_c[6],
                                          const T* u, T nud[6]) {
    const T u_ = nu[0], v_ = nu[1], w_ = nu[2], p_ = nu[3], q_ = nu[4], r_ = nu[5];
    T rhs[6];
    tau_minus_damping_<T, VK>(V, nu, tau_c, u, rhs);
    const T ctsf = g.ct * g.sf, ctcf = g.ct * g.cf;
    if (SYM) {
        // C(nu) nu = C_RB nu + C_A nu (statespace.py:199-286) multiplied out for r_G = (0, 0, z_G), diagonal I_b and
        // diagonal M_A: every component is a 2-3 term polynomial in products of two velocities; the coefficients
        // (VehicleP::kc) are combined on the host in float64.  Same value as the general branch below.
        const auto* K = V.kc;
        const T qw = q_ * w_, rv = r_ * v_, ru = r_ * u_, pw = p_ * w_, pr = p_ * r_, qr = q_ * r_;
        rhs[0] -= K[2] * qw - K[1] * rv + K[3] * pr;
        rhs[1] -= K[0] * ru - K[2] * pw + K[3] * qr;
        rhs[2] -= K[1] * (p_ * v_) - K[0] * (q_ * u_) - K[3] * (p_ * p_ + q_ * q_);
        rhs[3] -= -K[3] * (ru - pw) - K[4] * qr - K[5] * (v_ * w_);
        rhs[4] -= K[3] * (qw - rv) - K[6] * pr - K[7] * (u_ * w_);
        rhs[5] -= -K[8] * (p_ * q_) - K[9] * (u_ * v_);
        // restoring forces g(eta), statespace.py:353-397 with x_G = y_G = x_B = y_B = 0
        rhs[0] -= V.gWB * g.st;
        rhs[1] += V.gWB * ctsf;
        rhs[2] += V.gWB * ctcf;
        rhs[3] -= V.gz * ctsf;
        rhs[4] -= V.gz * g.st;
        nud[0] = V.Minv[0] * rhs[0] + V.Minv[4] * rhs[4];
        nud[1] = V.Minv[7] * rhs[1] + V.Minv[9] * rhs[3];
        nud[2] = V.Minv[14] * rhs[2];
        nud[3] = V.Minv[19] * rhs[1] + V.Minv[21] * rhs[3];
        nud[4] = V.Minv[24] * rhs[0] + V.Minv[28] * rhs[4];
        nud[5] = V.Minv[35] * rhs[5];
    } else {
        // --- Coriolis as cross products.  C_RB = [[m S(v2), -m S(v2) S(rG)], [m S(rG) S(v2), -S(I_b v2)]]
        const T c1x = q_ * w_ - r_ * v_, c1y = r_ * u_ - p_ * w_, c1z = p_ * v_ - q_ * u_;              // v2 x v1
        const T t1x = V.rg[1] * r_ - V.rg[2] * q_, t1y = V.rg[2] * p_ - V.rg[0] * r_, t1z = V.rg[0] * q_ - V.rg[1] * p_;
        const T c2x = q_ * t1z - r_ * t1y, c2y = r_ * t1x - p_ * t1z, c2z = p_ * t1y - q_ * t1x;        // v2 x (rG x v2)
        const T c3x = V.rg[1] * c1z - V.rg[2] * c1y, c3y = V.rg[2] * c1x - V.rg[0] * c1z, c3z = V.rg[0] * c1y - V.rg[1] * c1x;
        const T ivx = V.Ib[0] * p_ + V.Ib[1] * q_ + V.Ib[2] * r_;
        const T ivy = V.Ib[3] * p_ + V.Ib[4] * q_ + V.Ib[5] * r_;
        const T ivz = V.Ib[6] * p_ + V.Ib[7] * q_ + V.Ib[8] * r_;
        const T c4x = ivy * r_ - ivz * q_, c4y = ivz * p_ - ivx * r_, c4z = ivx * q_ - ivy * p_;         // (I_b v2) x v2
        // C_A = [[0, -S(a1)], [-S(a1), -S(a2)]],  a = M_A nu (diagonal M_A)
        const T a1x = V.ma[0] * u_, a1y = V.ma[1] * v_, a1z = V.ma[2] * w_;
        const T a2x = V.ma[3] * p_, a2y = V.ma[4] * q_, a2z = V.ma[5] * r_;
        rhs[0] -= V.m * (c1x - c2x) - (a1y * r_ - a1z * q_);
        rhs[1] -= V.m * (c1y - c2y) - (a1z * p_ - a1x * r_);
        rhs[2] -= V.m * (c1z - c2z) - (a1x * q_ - a1y * p_);
        rhs[3] -= V.m * c3x - c4x - (a1y * w_ - a1z * v_) - (a2y * r_ - a2z * q_);
        rhs[4] -= V.m * c3y - c4y - (a1z * u_ - a1x * w_) - (a2z * p_ - a2x * r_);
        rhs[5] -= V.m * c3z - c4z - (a1x * v_ - a1y * u_) - (a2x * q_ - a2y * p_);
        rhs[0] -= V.gWB * g.st;
        rhs[1] += V.gWB * ctsf;
        rhs[2] += V.gWB * ctcf;
        rhs[3] -= -V.gy * ctcf + V.gz * ctsf;
        rhs[4] -= V.gz * g.st + V.gx * ctcf;
        rhs[5] -= -V.gx * ctsf - V.gy * g.st;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            T acc = T(0);
#pragma unroll
            for (int j = 0; j < 6; ++j) acc += V.Minv[i * 6 + j] * rhs[j];
            nud[i] = acc;
        }
    }
}

// one RHS evaluation: derivative of (pos, att, nu) at stage values (att, nu).  The RHS does not depend on position.
template <typename T, int VK, bool SYM, bool WANT_POS, typename VP>
__device__ __forceinline__ void rhs_(const VP& V, const T att[3], const T nu[6], const T nuc[3],
                                     const T tau_c[6], const T* u, T pd[3], T ad[3], T nd[6]) {
    const Trig<T> g = trig_(att[0], att[1], att[2]);
    if (WANT_POS) {
        // p_dot = R_z(psi) R_y(theta) R_x(phi) v (geomutils.py:14-43: Rzyx is that product): three planar rotations, twelve
        // multiply-adds, instead of nine matrix entries (sixteen products) and nine more for R v
        const T vx = nu[0] + nuc[0], vy = nu[1] + nuc[1], vz = nu[2] + nuc[2];
        rot_body_to_ned_(g, vx, vy, vz, pd);
    }
    // T_Theta, utils/geomutils.py:46-75
    const T inv_ct = rcp_(g.ct);
    const T sq_cr = (g.sf * nu[4] + g.cf * nu[5]) * inv_ct;
    ad[0] = nu[3] + sq_cr * g.st;
    ad[1] = g.cf * nu[4] - g.sf * nu[5];
    ad[2] = sq_cr;
    kinetics_<T, VK, SYM>(V, nu, g, tau_c, u, nd);
}
// rhs_ with position of stage 1 in a kernel with a hot block: before_kinetics() stands between the kinematics, which need no
// parameter, and the kinetics (vehicle_step_ pins its second batch there).  Same expressions as rhs_.
struct NoFetch { __device__ __forceinline__ void operator()() const {} };
template <typename T, int VK, bool SYM, typename VP, typename PIN>
__device__ __forceinline__ void rhs_pinned_(const VP& V, const T att[3], const T nu[6], const T nuc[3], const T tau_c[6],
                                            const T* u, T pd[3], T ad[3], T nd[6], const PIN& before_kinetics) {
    const Trig<T> g = trig_(att[0], att[1], att[2]);
    const T vx = nu[0] + nuc[0], vy = nu[1] + nuc[1], vz = nu[2] + nuc[2];
    rot_body_to_ned_(g, vx, vy, vz, pd);
    const T inv_ct = rcp_(g.ct);
    const T sq_cr = (g.sf * nu[4] + g.cf * nu[5]) * inv_ct;
    ad[0] = nu[3] + sq_cr * g.st;
    ad[1] = g.cf * nu[4] - g.sf * nu[5];
    ad[2] = sq_cr;
    before_kinetics();
    kinetics_<T, VK, SYM>(V, nu, g, tau_c, u, nd);
}

// AUVSim.step: un-normalise, low-pass, Fehlberg 4th-order step, wrap.  objects/auvsim.py:77-108,
// utils/odesolver45.py:18-27 (stage 6 and the 5th-order result are dead in the reference and not computed).
// psi_lo (float path): low-order word of the heading, see the end of the function
// HOTV: V and E are the register copy of the wave's hot block (HotRegs, fetch_hot_input_: the input stage's part is there);
// all filtered inputs are computed first and stored then (a store between two inputs kept the parameter reads of the next
// one from moving above it, which nothing needs once they are in registers), and behind the constant part of the control
// force request_kinetics() asks for the second batch (request_hot_kinetics_), into the registers the input stage has given
// back; pin_kinetics() awaits it behind the kinematics of stage 1 (some 30 vector instructions), which cover the round trip.
// request_tail() stands behind the last right-hand side, where the kinetics' registers are free again: the wave asks there for
// what it reads behind the integrator (request_tail_), and the final sums and the post-step trigonometry cover the round trip.
template <typename T, int VK, bool SYM, int VOFF, bool HOTV = false, typename VP, typename EP, typename REQ = NoFetch, typename PIN = NoFetch,
          typename REQT = NoFetch>
__device__ __forceinline__ void vehicle_step_(const VP& V, const EP& E, T y[9], T dpos[3], T u[kMaxU],
                                              const T act[kMaxU], const T nuc[3], T* g_u, long S, unsigned ul, T& psi_lo,
                                              const REQ& request_kinetics = REQ(), const PIN& pin_kinetics = PIN(),
                                              const REQT& request_tail = REQT()) {
    const int n_u = (VK == VK_LAUV) ? 3 : (VK == VK_JOY ? 6 : V.n_u);
    const T one_m_alpha = T(1) - E.lp_alpha;
#pragma unroll
    for (int i = 0; i < kMaxU; ++i) {
        if (i < n_u) {
            const T a = clip_(act[i], T(-1), T(1));
            const T x = V.ulo[i] + V.uhalf[i] * ((a + T(1)) * T(0.5));
            u[i] = E.lp_alpha * x + one_m_alpha * u[i];
            // the filtered input is final: it goes back to HBM before the stages (a reset at the end of the step
            // overwrites it with zeros), so that for constant-B vehicles only tau_c stays live through them
            if (!HOTV) stgx_<VOFF>(g_u, i, S, ul, u[i]);
        }
    }
    if (HOTV) {
#pragma unroll
        for (int i = 0; i < kMaxU; ++i)
            if (i < n_u) stgx_<VOFF>(g_u, i, S, ul, u[i]);
    }
    T tau_c[6] = {0, 0, 0, 0, 0, 0};
    if (VK == VK_JOY) {
#pragma unroll
        for (int i = 0; i < 6; ++i) tau_c[i] = V.B[i * kMaxU + i] * u[i];
    } else if (VK == VK_DENSEB) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            T acc = T(0);
#pragma unroll
            for (int j = 0; j < kMaxU; ++j)
                if (j < n_u) acc += V.B[i * kMaxU + j] * u[j];
            tau_c[i] = acc;
        }
    } else if (VK == VK_LAUV) {
        lauv_fin_terms_<T>(V, u, tau_c);
    }
    if (HOTV) request_kinetics();
    // Fehlberg tableau times h: wave-uniform scalars
    const T h = E.h;
    const T a21 = h * T(1.0 / 4.0);
    const T a31 = h * T(3.0 / 32.0), a32 = h * T(9.0 / 32.0);
    const T a41 = h * T(1932.0 / 2197.0), a42 = h * T(-7200.0 / 2197.0), a43 = h * T(7296.0 / 2197.0);
    const T a51 = h * T(439.0 / 216.0), a52 = h * T(-8.0), a53 = h * T(3680.0 / 513.0), a54 = h * T(-845.0 / 4104.0);
    const T b1 = h * T(25.0 / 216.0), b3 = h * T(1408.0 / 2565.0), b4 = h * T(2197.0 / 4104.0), b5 = h * T(-1.0 / 5.0);
    // Register discipline (occupancy): the RHS does not depend on position, so the position increment is summed on
    // the fly (dpos) and the position itself is only loaded after the stages; k1, k3, k4 are folded into the final
    // sum as soon as the stage-5 input exists.  y = (att[3], nu[6]).
    T k1[9], k2[9], k3[9], k4[9], pd[3], ys[9];
    DOCKAUV_STAMP_PIN(16, tau_c, 6);   // inputs filtered
    if (HOTV) rhs_pinned_<T, VK, SYM>(V, y, y + 3, nuc, tau_c, u, pd, k1, k1 + 3, pin_kinetics);
    else rhs_<T, VK, SYM, true>(V, y, y + 3, nuc, tau_c, u, pd, k1, k1 + 3);
    DOCKAUV_STAMP_PIN(17, k1, 9);
#pragma unroll
    for (int i = 0; i < 3; ++i) dpos[i] = b1 * pd[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) ys[i] = y[i] + a21 * k1[i];
    rhs_<T, VK, SYM, false>(V, ys, ys + 3, nuc, tau_c, u, nullptr, k2, k2 + 3);
    DOCKAUV_STAMP_PIN(18, k2, 9);
#pragma unroll
    for (int i = 0; i < 9; ++i) ys[i] = y[i] + a31 * k1[i] + a32 * k2[i];
    rhs_<T, VK, SYM, true>(V, ys, ys + 3, nuc, tau_c, u, pd, k3, k3 + 3);
    DOCKAUV_STAMP_PIN(19, k3, 9);
#pragma unroll
    for (int i = 0; i < 3; ++i) dpos[i] += b3 * pd[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) ys[i] = y[i] + a41 * k1[i] + a42 * k2[i] + a43 * k3[i];
    rhs_<T, VK, SYM, true>(V, ys, ys + 3, nuc, tau_c, u, pd, k4, k4 + 3);
    DOCKAUV_STAMP_PIN(20, k4, 9);
#pragma unroll
    for (int i = 0; i < 3; ++i) dpos[i] += b4 * pd[i];
    constexpr bool PSI2 = sizeof(T) == 4;   // heading in two floats
    T psi_inc = T(0);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        ys[i] = y[i] + a51 * k1[i] + a52 * k2[i] + a53 * k3[i] + a54 * k4[i];
        const T inc = b1 * k1[i] + b3 * k3[i] + b4 * k4[i];      // k1..k4 are dead after this loop
        if (PSI2 && i == 2) psi_inc = inc; else y[i] = y[i] + inc;
    }
    rhs_<T, VK, SYM, true>(V, ys, ys + 3, nuc, tau_c, u, pd, k1, k1 + 3);   // k5 reuses k1's registers
    DOCKAUV_STAMP_PIN(21, k1, 9);
    if (HOTV) request_tail();
#pragma unroll
    for (int i = 0; i < 3; ++i) dpos[i] += b5 * pd[i];
#pragma unroll
    for (int i = 0; i < 9; ++i)
        if (!(PSI2 && i == 2)) y[i] += b5 * k1[i];
    y[0] = ssa_(y[0]);
    y[1] = ssa_(y[1]);
    if (PSI2) {
        // The heading is the second state nothing damps (after the position): psi += dpsi once per step, ~0.03 rad onto
        // up to pi, each sum dropping up to half an ulp (1.2e-7 rad) for good; the position then integrates v * dpsi.
        // Two-float accumulation as for the position (Knuth two-sum, exact), and a wrap that loses nothing: for
        // |s| in [pi, 2 pi) the subtraction s -+ fl(2 pi) is exact (Sterbenz), and what fl(2 pi) = 6.2831855 misses of
        // 2 pi (-1.7484555e-7) goes into the low word.  An angle inside [-pi, pi) is left alone (see ssa_).
        const T b = (psi_inc + b5 * k1[2]) + psi_lo;
        const T s_ = y[2] + b;
        const T bb = s_ - y[2];
        T lo = (y[2] - (s_ - bb)) + (b - bb);
        const T kk = s_ >= pi_<T>() ? T(1) : (s_ < -pi_<T>() ? T(-1) : T(0));
        y[2] = s_ - kk * T(6.2831855f);
        lo -= kk * T(-1.7484555e-7f);
        y[2] = ssa_(y[2]);   // (more than one turn per step: never in a valid episode; the generic wrap)
        psi_lo = lo;
    } else {
        y[2] = ssa_(y[2]);
    }
}

// ------------------------------------------------------------------------------------------ LDS layout
// (field counts and lds_bytes live in dockauv_device.h, shared with the host side)

// ------------------------------------------------------------------------------------------ ray kernels
// All rays of an env share the origin, and a ray enters the intersection tests only through dot products with
// per-(env, obstacle) vectors.  The env phase therefore rotates those vectors into the BODY frame once
// (d' = R^T d, ...), and the ray stage dots them with the constant body-frame ray table: a wave shares one ray, so the
// ray components are scalar (SGPR) operands and no ray is ever rotated or normalised per lane (Radar.update,
// objects/sensor.py:97-102, normalises R(Theta) rd_b, a unit vector already).
//
// One ray vs one capsule: same case structure and results as the vectorised reference routine
// (objects/shape.py:327-390) in a form that is well conditioned in float32.  The reference works with the
// un-normalised axis ba and the products baba*oaoa - baoa^2, b^2 - a*c: for a vehicle 20 m from a 1 m pillar both
// terms are ~400 and their difference ~1, i.e. float32 inputs alone put ~1e-4 m into the hit distance.  Here the
// offset is split into oa_par (along the unit axis d) and oa_perp, the ray into bard d + q, and the quadratic is
// solved around the point of closest approach in the plane perpendicular to d:
//   t0 = -(q.oa_perp)/|q|^2,  e = oa_perp + t0 q,  t = t0 - sqrt((r^2 - |e|^2)/|q|^2),  y/|ba| = oa_par + t bard
// (identical to t = (-b - sqrt(b^2 - a c))/a of the reference, all terms O(r)).  A cap sphere sits at
// oc = oa_perp + s d (s = oa_par at the bottom, oa_par - |ba| at the top) and is tested the same way.
// The shaft test is straight-line code; the cap test runs only in waves where some lane hit the infinite cylinder
// outside the segment (rare for the 40 m pillars).
// LDS record (kCapFields): d'(3) oa_perp'(3) oa_par len r^2 oa_top
template <typename T>
struct CapRec {
    T dx, dy, dz, px, py, pz, oa_par, len, r2, oa_top;
};

template <typename T>
__device__ __forceinline__ CapRec<T> load_cap_(const T* cp, int stride) {
    CapRec<T> c;
    c.dx = cp[0 * stride]; c.dy = cp[1 * stride]; c.dz = cp[2 * stride];
    c.px = cp[3 * stride]; c.py = cp[4 * stride]; c.pz = cp[5 * stride];
    c.oa_par = cp[6 * stride]; c.len = cp[7 * stride]; c.r2 = cp[8 * stride]; c.oa_top = cp[9 * stride];
    return c;
}

// (bx, by, bz): body-frame unit ray (wave-uniform)
template <typename T>
__device__ __forceinline__ T ray_capsule_(const CapRec<T>& c, T bx, T by, T bz) {
    const T bard = bx * c.dx + by * c.dy + bz * c.dz;
    const T qx = bx - bard * c.dx, qy = by - bard * c.dy, qz = bz - bard * c.dz;   // ray component _|_ axis
    const T a = qx * qx + qy * qy + qz * qz;
    const T b = bx * c.px + by * c.py + bz * c.pz;
    const T ra = rcp_(a);
    const T t0 = -b * ra;
    const T ex = c.px + t0 * qx, ey = c.py + t0 * qy, ez = c.pz + t0 * qz;
    const T h = c.r2 - (ex * ex + ey * ey + ez * ez);
    const bool hit = h > T(0);   // h <= 0 (tangent included) and NaN -> -inf  (shape.py:389)
    const T t = t0 - sqrt_(abs_(h) * ra);
    const T y = c.oa_par + t * bard;
    const bool shaft = (y > T(0)) && (y < c.len);
    T res = t;
    if (__any(hit && !shaft)) {
        // cap sphere: top cap wins at y == 0 (second assignment, shape.py:378-379)
        const T s = (y >= T(0)) ? c.oa_top : c.oa_par;
        const T ocx = c.px + s * c.dx, ocy = c.py + s * c.dy, ocz = c.pz + s * c.dz;
        const T b2 = bx * ocx + by * ocy + bz * ocz;
        const T fx = ocx - b2 * bx, fy = ocy - b2 * by, fz = ocz - b2 * bz;
        const T h2 = c.r2 - (fx * fx + fy * fy + fz * fz);
        const T cap = (h2 > T(0)) ? (-b2 - sqrt_(abs_(h2))) : T(0);
        res = shaft ? t : cap;
        // y NaN (ray parallel to the axis, a == 0): the reference tests the cap sphere with oc = 0 and gets -r
        // (shape.py:377); any negative number gives the same clamped distance.  The reference's a = |ba|^2 - (ba.rd)^2
        // cancels to exactly 0 for every ray within ~1e-8 rad of the axis (sin^2 < 2^-53), not only for bard == 1: |q|^2
        // here keeps 1e-32 for the central ray (1, 1.1e-16, 1.1e-16) of the shipped fans along an x-aligned axis and used
        // to answer the cap hit where the reference answers a miss (tests/golden/g4_rays.npz: edge cases 3 and 4)
        res = (isnan_(y) || a < T(1.1102230246251565e-16)) ? T(-1) : res;
    }
    // an exact zero -> -inf  (shape.py:386-388)
    return (hit && res != T(0)) ? res : -inf_<T>();
}

// one ray vs one sphere (intersec_dist_lines_spheres_vectorized, objects/shape.py:235-264); (ox, oy, oz) = body-frame
// origin - centre.  h = b^2 - (|oc|^2 - r^2) is evaluated as r^2 - |oc - b rd|^2 (no cancellation far away).
template <typename T>
__device__ __forceinline__ T ray_sphere_(T ox, T oy, T oz, T r2, T bx, T by, T bz) {
    const T b = ox * bx + oy * by + oz * bz;
    const T ex = ox - b * bx, ey = oy - b * by, ez = oz - b * bz;
    const T hh = r2 - (ex * ex + ey * ey + ez * ez);
    return (hh < T(0)) ? -inf_<T>() : (-b - sqrt_(abs_(hh)));
}

template <int N> struct IntC { static constexpr int value = N; };

// Sum of x over the 64 lanes of the wave, result in lane 63 (only): four DPP row rotations give every lane its row's
// sum, row_bcast:15 adds row 0's into row 1 and row 2's into row 3, row_bcast:31 adds rows 0 + 1 into rows 2 and 3.
// No LDS crossbar round trip (the two __shfl_xor doublings of group_sum_ cost ~250 cycles of latency each on a
// lone wave).  Fixed order: deterministic.
__device__ __forceinline__ float wave_sum_to_last_(float x) {
#define DOCKAUV_DPP_ADD(v, ctrl, rmask) ((v) + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, rmask, 0xf, false)))
    x = DOCKAUV_DPP_ADD(x, 0x128, 0xf);   // row_ror:8
    x = DOCKAUV_DPP_ADD(x, 0x124, 0xf);   // row_ror:4
    x = DOCKAUV_DPP_ADD(x, 0x122, 0xf);   // row_ror:2
    x = DOCKAUV_DPP_ADD(x, 0x121, 0xf);   // row_ror:1
    x = DOCKAUV_DPP_ADD(x, 0x142, 0xa);   // row_bcast:15 into rows 1 and 3
    x = DOCKAUV_DPP_ADD(x, 0x143, 0xc);   // row_bcast:31 into rows 2 and 3
#undef DOCKAUV_DPP_ADD
    return x;
}
__device__ __forceinline__ double wave_sum_to_last_(double x) { return x; }   // (never called: float kernels only)

// Sum of x over aligned groups of `width` lanes (power of two <= 64), result in every lane of the group.  float: four
// DPP row rotations cover 16 lanes (no LDS crossbar round trips: a chain of six ds_bpermute costs ~700 cycles of latency
// on a lone wave), the remaining one or two doublings go through __shfl_xor.  Fixed order: deterministic.
__device__ __forceinline__ float group_sum_(float x, int width) {
    if (width >= 16) {
#define DOCKAUV_ROW_ROR(v, ctrl) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xf, 0xf, false))
        x += DOCKAUV_ROW_ROR(x, 0x128);   // row_ror:8
        x += DOCKAUV_ROW_ROR(x, 0x124);   // row_ror:4
        x += DOCKAUV_ROW_ROR(x, 0x122);   // row_ror:2
        x += DOCKAUV_ROW_ROR(x, 0x121);   // row_ror:1
#undef DOCKAUV_ROW_ROR
        for (int m = 16; m < width; m <<= 1) x += __shfl_xor(x, m, 64);
        return x;
    }
    for (int m = 1; m < width; m <<= 1) x += __shfl_xor(x, m, 64);
    return x;
}
__device__ __forceinline__ double group_sum_(double x, int width) {
    for (int m = 1; m < width; m <<= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// ------------------------------------------------------------------------------------------ obstacle culling
// Can any ray of the fan reach this obstacle within ray_max?  Conservative (never says no for an obstacle a ray hits
// in range), evaluated once per (env, obstacle) in the body frame, where the fan lies inside the circular cone of
// half-angle theta_f around +x (EnvP::fan_cos / fan_sin).  A ray in the cone that touches the surface at S is within
// asin(r / |A|) <= asin(r / d_min) =: rho of the axis point A nearest to S, so some axis point lies within
// theta_f + rho of +x.  Skipping an obstacle cannot change a clamped distance: whatever it would have contributed
// (a miss, a negative value, a hit beyond ray_max) ends as ray_max (docking3d.py:436-439, sensor.py:117).
template <typename T>
__device__ __forceinline__ bool cone_reaches_(T cos_axis_angle, T dmin, T rad, T ray_max, T fan_cos, T fan_sin) {
    if (!(dmin > rad)) return true;                    // origin inside or touching (also NaN): keep
    if (dmin - rad > ray_max) return false;            // out of range
    const T srho = rad * rcp_(dmin);
    const T crho = sqrt_(T(1) - srho * srho);
    const T thr = fan_cos * crho - fan_sin * srho;     // cos(theta_f + rho)
    return !(cos_axis_angle < thr - T(1e-3));
}

// capsule: axis points X(tau) = -oa_perp + tau d, tau in [-oa_par, |ba| - oa_par] (oa_perp _|_ d).  The derivative of
// (X.x)/|X| has the sign of d.x |oa_perp|^2 + tau oa_perp.x, so the maximum sits at an end of the segment or at
// tau* = -d.x |oa_perp|^2 / oa_perp.x (a maximum when oa_perp.x < 0; evaluating it in the other case is harmless:
// clamped to the segment it is an axis point like any other)
template <typename T>
__device__ __forceinline__ bool capsule_may_be_hit_(T dx, T px, T pp, T oa_par, T len, T rad, T ray_max, T fan_cos, T fan_sin) {
    const T lo = -oa_par, hi = len - oa_par;
    const T tc = lo > T(0) ? lo : (hi < T(0) ? hi : T(0));          // nearest axis point
    const T dmin = sqrt_(pp + tc * tc);
    auto cosang = [&](T tau) { return (tau * dx - px) * rsqrt_(pp + tau * tau); };
    T cmax = cosang(lo);
    const T chi = cosang(hi);
    cmax = chi > cmax ? chi : cmax;
    if (px != T(0)) {
        T ts = -dx * pp * rcp_(px);
        ts = ts < lo ? lo : (ts > hi ? hi : ts);
        const T cs = cosang(ts);
        cmax = cs > cmax ? cs : cmax;
    }
    if (!(pp > T(0))) cmax = T(1);                                    // origin on the axis line
    return cone_reaches_(cmax, dmin, rad, ray_max, fan_cos, fan_sin);
}

// sphere: ocx = (origin - centre).x in the body frame, d2 = |origin - centre|^2
// (cone_reaches_ multiplied through by the distance: cos(angle to +x) * dist = -ocx and cos(theta_f + rho) * dist =
// fan_cos sqrt(dist^2 - r^2) - fan_sin r -- one square root instead of two reciprocals and a square root; same test)
template <typename T>
__device__ __forceinline__ bool sphere_may_be_hit_(T ocx, T d2, T dist, T rad, T ray_max, T fan_cos, T fan_sin) {
    if (!(dist > rad)) return true;                    // origin inside or touching (also NaN): keep
    if (dist - rad > ray_max) return false;            // out of range
    const T t = sqrt_(d2 - rad * rad);
    const T thr_d = fan_cos * t - fan_sin * rad;       // cos(theta_f + rho) * dist
    return !(-ocx < thr_d - T(1e-3) * dist);
}

// ------------------------------------------------------------------------------------------ device-side reset
// Philox4x32-10: philox4x32_10_ of dockauv_device.h (shared with the policy kernel).  Counter = (env, episode, block, 0),
// key = config.seed.

// Scenario generators of the reference (envs/docking3d.py:687-703, 795-988) fed with 12 uniforms U[k] = (x >> 8) 2^-24
// in the reference's draw order (same mapping as gym_dockauv_amd/scenarios.py: episodes_from_uniforms).
// Writes pose (6), goal (4), current rows (8) and the capsule slots of the env (caps_blk = capsule rows at this
// group's first env, ul = lane offset).
// the 12 (8 for SimpleDocking3d) uniforms of episode `episode` of env `env`
// NORING: the caller does not read ring_u (a kernel without capsule code, NOCAP); SphereDocking3d then reads draws 0..6 only
template <typename T, bool NORING = false, typename EP>
__device__ __forceinline__ void episode_uniforms_(const EP& E, int env, int episode, T U[12]) {
    const int scn = E.scenario;
    const unsigned long long seed = E.seed;
#pragma unroll
    for (int blk = 0; blk < 3; ++blk) {
        uint32_t c[4] = {(uint32_t)env, (uint32_t)episode, (uint32_t)blk, 0u};
        // SimpleDocking3d draws 7 uniforms: the third counter block is never looked at (32-bit integer multiplies
        // are quarter rate; a block is ~40 of them)
        if (blk < 2 || (scn != 0 && !(NORING && scn == 7))) philox4x32_10_(c, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
#pragma unroll
        for (int j = 0; j < 4; ++j) U[blk * 4 + j] = T(c[j] >> 8) * T(1.0 / 16777216.0);
    }
}

// generate_episode_ computes pose / goal / current of the next episode and the one draw the capsule rows depend on
// (ring_u: angle of the four-pillar ring); it has no side effects, so that a wave can run it ahead of time.
// store_capsules_ writes the capsule rows of an env once its episode really ends.
// (episode_uniforms_<T, NORING> relies on this: scenario 7 -- SphereDocking3d -- reads U[0..6] and nothing of U[8..11] but ring_u.
// A change that makes scenario 7 read a later draw has to take that scenario out of NORING's skip.)
template <typename T, typename EP>
__device__ __forceinline__ void generate_episode_(const EP& E, const T U[12], T pose[6], T goal[4], T cur[8], T& ring_u) {
    const int scn = E.scenario;
    const T pi = pi_<T>();
    ring_u = U[9];
    goal[0] = goal[1] = goal[2] = T(0);
    goal[3] = (U[0] - T(0.5)) * pi;                                        // docking3d.py:814
    T rx = U[1] - T(0.5), ry = U[2] - T(0.5), rz = U[3] - T(0.5);          // :694
    const T sgn = rz > T(0) ? T(1) : (rz < T(0) ? T(-1) : T(0));
    rz = abs_(rx + ry) * T(1.0 / 3.0) * sgn;                               // :695
    const T sc = T(15) * rsqrt_(rx * rx + ry * ry + rz * rz);              // :696, :809
    pose[0] = rx * sc; pose[1] = ry * sc; pose[2] = rz * sc;
    pose[3] = (U[4] - T(0.5)) * T(2) * (E.max_att * T(0.7));               // :699-703
    pose[4] = (U[5] - T(0.5)) * T(2) * (E.max_att * T(0.7));
    pose[5] = (U[6] - T(0.5)) * T(2) * pi;
    T Vc = T(0), vmin = T(0), vmax = T(0), al = T(0), be = T(0);           // :820-822
    if (scn == 1) {                                                        // SimpleCurrent :844-848
        al = (U[7] - T(0.5)) * T(2) * (pi / T(2));
        be = (U[8] - T(0.5)) * T(2) * pi;
        vmin = vmax = U[9];
        Vc = T(0.5);
    }
    if (scn >= 2 && scn <= 6) {                                            // Capsule* / Obstacles* :860-886
        T sth, cth;
        sincos_(U[7] * T(2) * pi, sth, cth);   // draws 7.. : scenario 1 (which used them) is not in this branch
        goal[0] = cth * T(2);                                              // CAPSULE_RADIUS + safety radius
        goal[1] = sth * T(2);
        goal[2] = (U[8] - T(0.5)) * T(4);
        goal[3] = ssa_(atan2_(-goal[1], -goal[0]));                        // :884-886
        if (scn == 3 || scn == 6) {                                        // *Current :904-906, :984-986
            // constant indices only (a run-time index would put U into scratch memory)
            al = ((scn >= 4 ? U[10] : U[9]) - T(0.5)) * T(2) * (pi / T(2));
            be = ((scn >= 4 ? U[11] : U[10]) - T(0.5)) * T(2) * pi;
            Vc = vmin = vmax = T(0.5);
        }
    }
    T sa, ca, sb, cb;
    sincos_(al, sa, ca);
    sincos_(be, sb, cb);
    cur[0] = Vc; cur[1] = ca * cb; cur[2] = sb; cur[3] = sa * cb;         // objects/current.py:70-74
    cur[4] = vmin; cur[5] = vmax; cur[6] = al; cur[7] = be;
}

// capsule slots of the Capsule* / Obstacles* scenarios (caps_blk = capsule rows at this group's first env, ul = lane)
template <typename T, typename EP>
__device__ __forceinline__ void store_capsules_(const EP& E, T* caps_blk, long S, unsigned ul, T ring_u) {
    const int scn = E.scenario;
    if (!(scn >= 2 && scn <= 6)) return;
    const T pi = pi_<T>();
    int slot = 0;
    if (scn != 5 && slot < E.max_cap) {                                    // centre capsule (popped by NoCap, :964)
        T* cg = caps_blk + (size_t)slot * 7 * S;
        stg_(cg, 0, S, ul, T(0)); stg_(cg, 1, S, ul, T(0)); stg_(cg, 2, S, ul, T(2));
        stg_(cg, 3, S, ul, T(0)); stg_(cg, 4, S, ul, T(0)); stg_(cg, 5, S, ul, T(-2));
        stg_(cg, 6, S, ul, T(1));
        ++slot;
    }
    if (scn >= 4) {                                                        // four pillars :923-946
        T th = ring_u * T(2) * pi;
        const T half = E.dmax;                                             // 2 * max_dist_from_goal / 2
        for (int i = 0; i < 4; ++i) {
            T s_, c_;
            sincos_(th, s_, c_);
            th += pi / T(2);
            if (slot < E.max_cap) {
                T* cg = caps_blk + (size_t)slot * 7 * S;
                stg_(cg, 0, S, ul, c_ * T(6)); stg_(cg, 1, S, ul, s_ * T(6)); stg_(cg, 2, S, ul, half);
                stg_(cg, 3, S, ul, c_ * T(6)); stg_(cg, 4, S, ul, s_ * T(6)); stg_(cg, 5, S, ul, -half);
                stg_(cg, 6, S, ul, T(1));
                ++slot;
            }
        }
    }
    for (; slot < E.max_cap; ++slot) stg_(caps_blk, ((size_t)slot * 7 + 6), S, ul, T(-1));
}

// Keep a wave-uniform value in an SGPR.  Parameters come from constant memory and the compiler treats such a load as
// free to repeat: inside the ray loops it re-issued `s_load_dword; s_waitcnt lgkmcnt(0)` for the same few integers
// ~20 times per cell, one exposed scalar-cache round trip each (measured: two thirds of the ray stage was spent in
// those waits).  The empty asm makes the copy opaque, so it is loaded once.
template <typename V>
__device__ __forceinline__ V pin_sgpr_(V v) {
    asm volatile("" : "+s"(v));
    return v;
}

// The integrating wave's hot block in registers (dockauv_device.h: HotP, the rule at ParamBlock): a VehicleP of which only
// the fields HotP holds are written -- kinetics_ / tau_minus_damping_ / vehicle_step_ read it like the parameter block's, the
// rest is never read on this path and does not exist after scalar replacement -- and the input-stage scalars of EnvP.
template <typename T>
struct HotRegs {
    VehicleP<T> V;
    T lp_alpha, mu, h, w_act[kMaxU];
};
// The block arrives in TWO batches, because the wave has no SGPRs for all of it at once (61 scalars for the BlueROV2, 66
// for the LAUV, next to ~60 of addresses; all at once: 13 -> 57 SGPR spills in config 3's kernel): the input stage's part
// behind the row loads, whose latency covers it, and the kinetics' part behind the input filter, in the registers the
// first part has just given back, awaited behind the kinematics of stage 1 (pin_hot_kinetics_).  In each, every load
// comes first (adjacent words: the compiler merges them into s_load_dwordx2 .. x16), then the pins, which keep the batch
// where it is requested (pin_sgpr_).
template <typename T, int VK, bool WACT, typename HP>
__device__ __forceinline__ void fetch_hot_input_(const HP& H, HotRegs<T>& R) {
    static_assert(VK == VK_JOY || VK == VK_LAUV, "vehicle kinds with a hot block");
    constexpr int NU = VK == VK_LAUV ? 3 : 6;
    R.lp_alpha = H.lp_alpha; R.mu = H.mu; R.h = H.h;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
        if (WACT) R.w_act[i] = H.w_act[i];
        R.V.ulo[i] = H.ulo[i]; R.V.uhalf[i] = H.uhalf[i];
    }
    // what turns the filtered inputs into the constant part of the control force: dead in front of the stages as well
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (VK == VK_JOY) R.V.B[i * kMaxU + i] = H.bdiag[i];
#pragma unroll
    for (int i = L_Y_uudr; i < L_COUNT; ++i)
        if (VK == VK_LAUV) R.V.lauv[i] = H.lauv[i];
    R.lp_alpha = pin_sgpr_(R.lp_alpha); R.mu = pin_sgpr_(R.mu); R.h = pin_sgpr_(R.h);
#pragma unroll
    for (int i = 0; i < NU; ++i) {
        if (WACT) R.w_act[i] = pin_sgpr_(R.w_act[i]);
        R.V.ulo[i] = pin_sgpr_(R.V.ulo[i]); R.V.uhalf[i] = pin_sgpr_(R.V.uhalf[i]);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (VK == VK_JOY) R.V.B[i * kMaxU + i] = pin_sgpr_(R.V.B[i * kMaxU + i]);
#pragma unroll
    for (int i = L_Y_uudr; i < L_COUNT; ++i)
        if (VK == VK_LAUV) R.V.lauv[i] = pin_sgpr_(R.V.lauv[i]);
}
template <typename T, int VK, typename HP>
__device__ __forceinline__ void request_hot_kinetics_(const HP& H, HotRegs<T>& R) {
    static_assert(VK == VK_JOY || VK == VK_LAUV, "vehicle kinds with a hot block");
#pragma unroll
    for (int i = 0; i < 6; ++i) { R.V.dl[i] = H.dl[i]; R.V.dq[i] = H.dq[i]; }
#pragma unroll
    for (int i = 0; i < 10; ++i) { R.V.kc[i] = H.kc[i]; R.V.Minv[minv_sym(i)] = H.minv[i]; }
    R.V.gWB = H.gWB; R.V.gz = H.gz;
    if (VK == VK_LAUV) {
#pragma unroll
        for (int i = 0; i < L_Y_uudr; ++i) R.V.lauv[i] = H.lauv[i];
    }
    // (the loads stay in front of this point: nothing may be scheduled across it)
    __builtin_amdgcn_sched_barrier(0);
}
template <typename T, int VK>
__device__ __forceinline__ void pin_hot_kinetics_(HotRegs<T>& R) {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 6; ++i) { R.V.dl[i] = pin_sgpr_(R.V.dl[i]); R.V.dq[i] = pin_sgpr_(R.V.dq[i]); }
#pragma unroll
    for (int i = 0; i < 10; ++i) { R.V.kc[i] = pin_sgpr_(R.V.kc[i]); R.V.Minv[minv_sym(i)] = pin_sgpr_(R.V.Minv[minv_sym(i)]); }
    R.V.gWB = pin_sgpr_(R.V.gWB); R.V.gz = pin_sgpr_(R.V.gz);
    if (VK == VK_LAUV) {
#pragma unroll
        for (int i = 0; i < L_Y_uudr; ++i) R.V.lauv[i] = pin_sgpr_(R.V.lauv[i]);
    }
}

// What a wave role reads BEHIND the integrator (dockauv_device.h: TailP), as one batch per role.  G: the groups of the block
// the role needs -- they are adjacent in TailP, so a role's batch is two or three wide loads.  request_tail_ issues every load
// and nothing else (nothing may be scheduled across its end), pin_tail_ awaits them and keeps them in SGPRs (pin_sgpr_); the
// caller puts work that needs none of them in between.  Q: the tail's scalars, RC: the record completion's, RQ: the pass waves'
// (step_body).  Fields of a group the role did not ask for stay unset and are never read by it.
enum TailGroup { kTgDone = 1, kTgAll = 2, kTgRec = 4, kTgPass = 8, kTgObs = 16, kTgBk = 32 };
template <int G, typename TP, typename QT, typename RCT, typename RQT>
__device__ __forceinline__ void request_tail_(const TP& P, QT& Q, RCT& RC, RQT& RQ) {
    if (G & kTgDone) {
        Q.inv_log_tol = P.inv_log_tol; Q.dtol = P.dtol; Q.dmax = P.dmax; Q.max_att = P.max_att; Q.max_timesteps = P.max_timesteps;
    }
    if (G & kTgAll) { Q.reset_mode = P.reset_mode; Q.n_obs = P.n_obs; Q.inv_dmax = P.inv_dmax; }
    if (G & kTgRec) { RC.ray_max = P.ray_max; RC.fan_cos = P.fan_cos; RC.fan_sin = P.fan_sin; RC.safety = P.safety; }
    if (G & kTgPass) {
        RQ.ray_max = P.ray_max; RQ.max_cap = P.max_cap; RQ.max_sph = P.max_sph; RQ.pad = P.ray_pad; RQ.pad_log2 = P.ray_pad_log2;
        RQ.n_rays = P.n_rays; RQ.n_red = P.n_red; RQ.inv_ray_max = P.inv_ray_max; RQ.sum_beta = P.sum_beta;
    }
    if (G & kTgObs) {
#pragma unroll
        for (int k = 0; k < 6; ++k) Q.inv_vel[k] = P.inv_vel[k];
        Q.inv_max_att = P.inv_max_att;
    }
    if (G & kTgBk) {
        Q.inv_log_tol_eps = P.inv_log_tol_eps;
        Q.w_d = P.w_d; Q.w_dth = P.w_dth; Q.w_dpsi = P.w_dpsi; Q.w_phi = P.w_phi; Q.w_th = P.w_th; Q.w_thdot = P.w_thdot;
        Q.w_oa = P.w_oa;
#pragma unroll
        for (int k = 0; k < 5; ++k) Q.w_done[k] = P.w_done[k];
    }
    __builtin_amdgcn_sched_barrier(0);
}
template <int G, typename QT, typename RCT, typename RQT>
__device__ __forceinline__ void pin_tail_(QT& Q, RCT& RC, RQT& RQ) {
    __builtin_amdgcn_sched_barrier(0);
    if (G & kTgDone) {
        Q.inv_log_tol = pin_sgpr_(Q.inv_log_tol); Q.dtol = pin_sgpr_(Q.dtol); Q.dmax = pin_sgpr_(Q.dmax);
        Q.max_att = pin_sgpr_(Q.max_att); Q.max_timesteps = pin_sgpr_(Q.max_timesteps);
    }
    if (G & kTgAll) { Q.reset_mode = pin_sgpr_(Q.reset_mode); Q.n_obs = pin_sgpr_(Q.n_obs); Q.inv_dmax = pin_sgpr_(Q.inv_dmax); }
    if (G & kTgRec) {
        RC.ray_max = pin_sgpr_(RC.ray_max); RC.fan_cos = pin_sgpr_(RC.fan_cos); RC.fan_sin = pin_sgpr_(RC.fan_sin);
        RC.safety = pin_sgpr_(RC.safety);
    }
    if (G & kTgPass) {
        RQ.ray_max = pin_sgpr_(RQ.ray_max); RQ.max_cap = pin_sgpr_(RQ.max_cap); RQ.max_sph = pin_sgpr_(RQ.max_sph);
        RQ.pad = pin_sgpr_(RQ.pad); RQ.pad_log2 = pin_sgpr_(RQ.pad_log2); RQ.n_rays = pin_sgpr_(RQ.n_rays);
        RQ.n_red = pin_sgpr_(RQ.n_red); RQ.inv_ray_max = pin_sgpr_(RQ.inv_ray_max); RQ.sum_beta = pin_sgpr_(RQ.sum_beta);
    }
    if (G & kTgObs) {
#pragma unroll
        for (int k = 0; k < 6; ++k) Q.inv_vel[k] = pin_sgpr_(Q.inv_vel[k]);
        Q.inv_max_att = pin_sgpr_(Q.inv_max_att);
    }
    if (G & kTgBk) {
        Q.inv_log_tol_eps = pin_sgpr_(Q.inv_log_tol_eps);
        Q.w_d = pin_sgpr_(Q.w_d); Q.w_dth = pin_sgpr_(Q.w_dth); Q.w_dpsi = pin_sgpr_(Q.w_dpsi); Q.w_phi = pin_sgpr_(Q.w_phi);
        Q.w_th = pin_sgpr_(Q.w_th); Q.w_thdot = pin_sgpr_(Q.w_thdot); Q.w_oa = pin_sgpr_(Q.w_oa);
#pragma unroll
        for (int k = 0; k < 5; ++k) Q.w_done[k] = pin_sgpr_(Q.w_done[k]);
    }
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the wave's global stores
// (s_waitcnt vmcnt(0)): every hand-over in this kernel goes through LDS, and the state / input write-backs that are
// in flight at that point have no reader inside the launch.  A single-wave group needs no s_barrier at all: LDS
// operations of one wave complete in order.
template <int NT>
__device__ __forceinline__ void lds_barrier_() {
    if (NT <= 64) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    }
}

// AUVSim._state_dot = state_dot(0, state, nu_c) at the NEW state with the new filtered input (objects/auvsim.py:108,
// 145-160): what EpisodeDataStorage logs as "states_dot".  Only evaluated when a caller asks for it (dockauv_step_io::
// state_dot, dockauv_trace_*); the reward needs its Euler-rate rows alone.
template <typename T, int VK, bool SYM, typename VP>
__device__ __forceinline__ void post_step_rhs_(const VP& V, const T st[12], const Trig<T>& g, const T nuc[3], const T* u, T sd[12]) {
    const int n_u = (VK == VK_LAUV) ? 3 : (VK == VK_JOY ? 6 : V.n_u);
    T tau_c[6] = {0, 0, 0, 0, 0, 0};
    if (VK == VK_JOY) {
#pragma unroll
        for (int i = 0; i < 6; ++i) tau_c[i] = V.B[i * kMaxU + i] * u[i];
    } else if (VK == VK_DENSEB) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            T acc = T(0);
#pragma unroll
            for (int j = 0; j < kMaxU; ++j)
                if (j < n_u) acc += V.B[i * kMaxU + j] * u[j];
            tau_c[i] = acc;
        }
    } else if (VK == VK_LAUV) {
        lauv_fin_terms_<T>(V, u, tau_c);
    }
    T R[9];
    rotmat_(g, R);
    const T vx = st[6] + nuc[0], vy = st[7] + nuc[1], vz = st[8] + nuc[2];
    sd[0] = R[0] * vx + R[1] * vy + R[2] * vz;
    sd[1] = R[3] * vx + R[4] * vy + R[5] * vz;
    sd[2] = R[6] * vx + R[7] * vy + R[8] * vz;
    const T sq_cr = (g.sf * st[10] + g.cf * st[11]) * rcp_(g.ct);
    sd[3] = st[9] + sq_cr * g.st;
    sd[4] = g.cf * st[10] - g.sf * st[11];
    sd[5] = sq_cr;
    kinetics_<T, VK, SYM>(V, st + 6, g, tau_c, u, sd + 6);
}

// w = sigma * N(0, 1) of Current.sim (objects/current.py:88) drawn in the kernel (dockauv_config::device_noise):
// Philox counter (env, episode, t_steps, 1), Box-Muller on the first two words; same numbers as
// oracle/philox_ref.py: philox_normal
template <typename T>
__device__ __forceinline__ T device_normal_(unsigned long long seed, int env, int episode, int t_steps) {
    uint32_t c[4] = {(uint32_t)env, (uint32_t)episode, (uint32_t)t_steps, 1u};
    philox4x32_10_(c, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
    const T u1 = (T(c[0] >> 8) + T(0.5)) * T(1.0 / 16777216.0);   // (0, 1): log is finite
    const T u2 = T(c[1] >> 8) * T(1.0 / 16777216.0);
    T sn, cs;
    sincos_accurate_(T(2) * pi_<T>() * u2, sn, cs);
    return sqrt_(T(-2) * log_(u1)) * cs;
}

// ------------------------------------------------------------------------------------------ the step kernel
// Scheduling choices of the product kernels, each settled by same-box A/B runs (profiles/r2/, profiles/r3/ab_same_box.txt;
// the losing branches were deleted in round 4):
//  * wave roles rotate with the group index in ray groups of two or four waves (not of eight: two groups per CU, their
//    integrating waves land on different SIMDs anyway; config 4 9.95 -> 9.77 us without);
//  * integrating waves of the 256-thread ray kernels of ONE vehicle kind run at raised priority during the env phase
//    (config 3 8.57 -> 8.40 us); 512-thread groups (config 4: 2.6 % faster without) and the mixed kernel (two integrating
//    waves per group at raised priority: +5 %) do not;
//  * helper waves request their rows at once (holding them back cost 0.1-1.3 us: their own work is nearly critical);
//  * a tail role polls the hand-over flag every kNavSleep x 64 clocks;
//  * pass ranks of waves 0..3 of a mixed EARLY group: the integrating waves first (kMixedRanks).
constexpr int kNavSleep = 2;
constexpr int kPrioLevel = 3;
constexpr unsigned kMixedRanks = 0x2310u;
#ifndef DOCKAUV_FAULT_INJECT_DROP_NAV_FLAG
#define DOCKAUV_FAULT_INJECT_DROP_NAV_FLAG 0
#endif

// float kernels are held at <= 128 VGPRs (4 waves per SIMD: four 256-thread groups per CU); the float64 validation
// kernels take what they need
template <typename T, int NT> constexpr int min_waves_() { return sizeof(T) == 4 ? 4 : 1; }

// LOG = the logging instantiation: state_dot output, episode-storage trace, in-kernel current noise.  Compiled as kernels
// of their own (select_step picks them when a step asks for any of the three): with the same paths behind run-time
// branches of the product kernels every BASELINE config lost 5-12 % (same-box A/B, round 2).
// which kernels run the tail roles in front of the ray-stage barrier (EARLY) and share the integrating wave's navigation
// errors / done bits through LDS (SHARE_NAV): needed by the kernel body and by the host-side LDS sizing
template <int VK, bool RAYS, int EPG, int NT, bool LOG>
constexpr bool early_tail_() {
    return RAYS && (NT / EPG >= 4) && !LOG;
}
template <int VK, bool RAYS, int EPG, int NT, bool LOG>
constexpr bool share_nav_() {
    // (groups of four waves: the integrating wave then takes no ray pass either; groups of eight -- config 4 -- keep it in
    // the pass rotation, last: taking it out cost them 0.7-2 %, sharing alone gains 2 %)
    return early_tail_<VK, RAYS, EPG, NT, LOG>();
}

// Which kernels fetch the integrating wave's parameters in early batches (fetch_hot_input_ / request_hot_kinetics_): float
// product kernels of the structural fast path, one vehicle kind per kernel.  KIND: 0 = step_kernel, 1 = step_ride_kernel,
// 2 = step_seq_kernel.  The batches are pinned, so the register allocator can no longer re-load a parameter where it would
// otherwise spill one; the instantiations in which that raised the SGPR-spill count (the guard rails of DESIGN.md section 3,
// profiles/hot_params/kernel_usage.txt) keep the loads at the uses:
//  * mixed batches: the two integrating waves of a group hold the union of both vehicles' registers (12 -> 50 spills);
//  * the LAUV's ray kernels and its 256-thread sensor-free kernels (50 kinetics scalars live at once: +2 .. +13 spills);
//  * of the BlueROV2's: the resident ray kernels of 256 threads, the resident sensor-free kernels of 128 / 256 threads, the
//    riding one-wave ray kernel (+1 .. +2 spills each).
template <typename T, int VK, bool SYM, bool RAYS, int EPG, int NT, bool LOG, bool TERM, bool WB, int KIND>
constexpr bool hot_params_() {
    if (sizeof(T) != 4 || !SYM || LOG) return false;
    if (VK == VK_LAUV) return !RAYS && NT < 256;
    if (VK != VK_JOY) return false;
    if (KIND == 1) return !(RAYS && NT == 64);
    if (KIND == 2) return RAYS ? NT != 256 : NT == 64;
    return true;
}

// Which kernels fetch what their roles read behind the integrator in one batch per role (request_tail_ / pin_tail_, TailP):
// kernels with a hot block -- the integrating wave's request stands in the registers the kinetics batch has given back -- that
// kept the guard rails with it (DESIGN.md section 3, profiles/tail_params/kernel_usage.txt); the others, and every full (LOG)
// instantiation, keep reading EnvP at the uses.
template <typename T, int VK, bool SYM, bool RAYS, int EPG, int NT, bool LOG, bool TERM, bool WB, int KIND>
constexpr bool tail_params_() {
    if (!hot_params_<T, VK, SYM, RAYS, EPG, NT, LOG, TERM, WB, KIND>()) return false;
    // ray kernels of four waves only: a one-wave group (everything is the integrating wave's) took one more SGPR spill with its
    // batch; in the sensor-free kernels the batch removed no round trip from the straight-line path (their one batch already
    // stood behind the trigonometry; the kernarg word that used to ride in its wait got a wait of its own); in groups of eight
    // waves the integrating wave takes ray passes, whose scalars need a batch of their own in front of the hand-over barrier:
    // the plain and the riding kernel took two more SGPR spills, the other two lost no round trip behind the integrator
    if (!RAYS || NT / EPG != 4) return false;
    return true;
}

// TERM (product kernels, packed rows): the terminal observation of the envs that finish in this step is delivered as well
// (dockauv_step_io::terminal_obs; SB3's infos[i]["terminal_observation"], train.py:64-71 via DummyVecEnv) -- an
// instantiation of its own, so that the plain product kernels carry none of it: the tail roles write the TRUE observation
// of every env into the tile, and behind the tile's last barrier one wave copies the rows of the finished envs to
// terminal_obs and zeroes them (the reference's reset observation, Q8) before the tile is streamed out.
// WB: plain write-back stores (instantiations that serve launches of several rounds of groups only, see store_global_)
// NOCUR (float32 product kernels of the shapes nocur_shape names, dockauv_device.h): the handle has no water current -- V_c =
// V_min = V_max = 0 in every env for as long as select_step picks this form -- and the step carries none of it: no `cur` row is
// loaded or stored, V_c is not filtered, V_c and nu_c do not travel through lds_hx (rows 12 and 16-18 stay unused), observations
// 13-15 are written as the +0 they always were, and an episode reset leaves the current rows, which hold what it would write,
// alone.  The right-hand sides keep their three nu + nu_c additions with nu_c a literal zero: x + 0 is not x for x = -0.
// NOCAP (on top of NOCUR; the BlueROV2's ray kernel of 256 threads, nocap_shape in dockauv_device.h): the handle has no capsule slot,
// and the ray stage and the reset carry no capsule code -- no capsule masks (cm_l, wc, cmask are literal zeros, nocap a literal true:
// row 14 of lds_pose is neither zeroed nor read, row 0 is not read by the ray stage), no capsule loop in the passes, no capsule rows
// in a reset and no draw of the pillar ring's angle.  Wave 1's zero-trip capsule prefetch and the slot count it leaves in row 0 for
// the record completion stay: with `ncap` a literal zero there the plain and the riding kernel took 112 / 111 VGPRs against their
// twins' 107 (a guard rail, DESIGN.md section 3); with the row read 107 / 107 and 2 / 2 SGPR spills against 6 / 7.
// Measured and left out (profiles/sphere_only/parts.txt): the sphere prefetch spread over waves 1 and 2 with every row requested at
// once -- the pose barrier never waited for the prefetch, and 32 more row loads per group at the launch's cold start held up the
// integrating wave's own rows -- and a group-wide skip of spheres out of range in the record completion.
template <typename T, int VK, bool SYM, bool RAYS, int EPG, int NT, bool LOG = false, bool TERM = false, bool WB = false, int KIND = 0,
          bool NOCUR = false, bool NOCAP = false>
__device__ __forceinline__ void step_body(const DevArgs& A, const unsigned tix = threadIdx.x, const unsigned bix = blockIdx.x) {
    static_assert(!NOCUR || (sizeof(T) == 4 && SYM && !LOG && VK != VK_MIXED && NT / EPG >= 4), "the lean form: see nocur_shape");
    static_assert(!NOCAP || (NOCUR && RAYS && VK == VK_JOY && NT / EPG == 4), "the sphere-only form: see nocap_shape");
    DOCKAUV_SPAN(0);   // (diagnostic build: the group's very first instructions)
    extern __shared__ __align__(16) unsigned char smem_raw[];
    typedef const __attribute__((address_space(4))) ParamBlock<T, 2> CParams;
    CParams* const PB = (CParams*)(uintptr_t)A.params;
    const auto& E = PB->E;
    const Buffers& B = A.B;
    // The product instantiations (LOG = false) serve the calls that ask for the mandatory outputs only -- observation
    // rows and reward / done, separate or packed; every optional input / output of dockauv_step_io is a compile-time
    // null there (launch_vk sends any other call to the LOG instantiation).
    StepIO IO = A.io;
    if (!LOG) {
        IO.noise = nullptr; IO.reward_terms = nullptr; IO.conditions = nullptr; IO.nav = nullptr; IO.ray_dist = nullptr;
        IO.terminal_obs = nullptr; IO.state_dot = nullptr; IO.trace = nullptr; IO.device_noise = 0;
    }
    static_assert(!(TERM && LOG), "the full instantiation writes terminal_obs from its tail roles");
    float* const term_out = TERM ? A.io.terminal_obs : nullptr;   // (TERM: packed rows only, see launch_vk)
    const long S = B.stride;
    constexpr bool LATE_GOAL = VK == VK_MIXED && !LOG && RAYS;   // (see the loads of the integrating waves)
    // access flags of this instantiation (ldgx_ / stgx_): row offsets in the lane offset register, write-back stores
    constexpr int VOFF = kAfVoff | (WB ? kAfWriteBack : 0);
    // Ray kernels: wave roles rotate with the group index, so that the integrating waves of the groups that share a
    // CU sit on different SIMDs whatever starting SIMD the dispatcher picks (config 3: 15.3 -> 14.6 us, config 5:
    // 26.7 -> 26.0 us, config 4 unchanged; the sensor-free kernel is 2 % slower with it and keeps wave 0).
    // (round 3, events around the timed regions: groups of eight waves -- config 4 -- are 1.8 % FASTER without the rotation
    // (9.95 -> 9.77 us): two groups per CU, their integrating waves land on different SIMDs anyway; groups of four keep it)
#ifdef DOCKAUV_STAMPS
    constexpr bool ROTATE = false;   // (the diagnostic build's stamps are taken by fixed threads)
#else
    constexpr bool ROTATE = RAYS && NT / EPG > 1 && NT / EPG < 8;
#endif
    // (tix / bix: thread and group index; the resident sequence kernel passes them opaque per step, see step_seq_kernel)
    const int tid = ROTATE ? (int)((((tix / EPG) + bix) % (NT / EPG)) * EPG + tix % EPG) : (int)tix;
    const int env0 = bix * EPG;
    const int env = env0 + tid;
    // Mixed batches in groups of four or more waves: TWO integrating waves, wave 0 for the vehicle-0 lanes and wave 1
    // for the vehicle-1 lanes of the same 64 envs, side by side on different SIMDs.  One wave would run both vehicle
    // models back to back under complementary EXEC masks (a wave with half its lanes off issues just as many
    // instructions: config 5's env phase was the sum of the two, ~10 k cycles).  Each of the two owns its lanes for the
    // rest of the step (pose hand-over, collision, navigation-dependent observations, state write-back).
    constexpr bool MIXED2 = (VK == VK_MIXED) && (NT / EPG >= 4);
    const bool loader = (MIXED2 ? tid < 2 * EPG : tid < EPG) && (env0 + tid % EPG < A.n_envs);   // requests the env's rows
    bool owner = (tid < EPG) && (env < A.n_envs);   // integrates the env (MIXED2: narrowed to the wave's vehicle below)
    const int n_valid = min(EPG, A.n_envs - env0);
    const int row_len = E.n_obs + (IO.pack ? 2 : 0);   // observation row in the LDS tile and in the output

    DOCKAUV_SPAN(1);   // (the first kernarg and parameter-block words have arrived)
    DOCKAUV_STAMP(0);
#ifdef DOCKAUV_STAMPS
    {   // diagnostic: when has the first word of the kernarg segment arrived
        int probe = A.n_envs;
        asm volatile("" : "+s"(probe));
        DOCKAUV_STAMP(6);
    }
#endif
    // LDS carve-up (host side: dockauv_device.h, lds_bytes)
    // SOLO = a ray group of ONE wave (light fans beyond the batch sizes where every group is resident at once): what bounds
    // such launches is how many groups a CU holds, and with four waves per SIMD by registers that is decided by LDS.  The
    // wave is integrator and ray stage in one, so pose, slot counts, may-be-hit masks and the collision flag stay in the
    // lane = env registers (no pose rows, no per-wave flag row), and the observation tile -- written by the tail, when the
    // obstacle records are dead -- OVERLAYS the records; only the ray cells, which the passes accumulate, get an array of
    // their own ([EPG][n_red] floats).  Config 3: 18 944 -> 9 984 B per group, 8 -> 16 groups per CU.
    constexpr bool SOLO = RAYS && (NT / EPG == 1);
    static_assert(!(SOLO && (LOG || TERM)), "one-wave ray groups exist as plain product kernels only");
    // One-wave groups of the 63-ray fan against capsules only (solo_regrec, dockauv_device.h): a pass serves ONE env, so a
    // completed capsule record is wave-uniform there -- it stays in the lane = env registers of the wave that completed it and
    // reaches the pass through v_readlane (scalar operands of the ray test) instead of ten LDS rows per capsule.  The list of
    // active envs is the ballot itself (s_ff1), the obstacle-avoidance sum of an env goes from the pass to the env's lane through
    // a scalar.  LDS then holds the raw rows c1 | c2 - c1 | r the prefetch parked ([max_cap][7][EPG]) and, once the
    // records exist and those are dead, in the same bytes the tile (ray cells in place).  Config 4: 18 688 -> 9 728 B per
    // group, 8 -> 16 groups per CU.
    constexpr bool REGREC_OK = SOLO && sizeof(T) == 4;
    const bool regrec = REGREC_OK && solo_regrec(E.max_cap, E.max_sph, E.ray_pad_log2);
    T* lds_pose = reinterpret_cast<T*>(smem_raw);
    T* lds_cap = lds_pose + ((RAYS && !SOLO) ? kPoseFields * EPG : 0);
    T* lds_sph = lds_cap + (RAYS ? kCapFields * E.max_cap * EPG : 0);
    T* lds_oa = lds_sph + (RAYS ? kSphFields * E.max_sph * EPG : 0);   // [NT/EPG][2][EPG] obstacle-avoidance partial sums
    if (SOLO) {   // (behind the larger of records and tile)
        size_t rec_bytes = (size_t)(lds_oa - lds_pose) * sizeof(T);
        const size_t tile_bytes = (size_t)EPG * (size_t)(E.n_obs + 2) * sizeof(float);
        rec_bytes = ((rec_bytes > tile_bytes ? rec_bytes : tile_bytes) + 15) & ~(size_t)15;
        lds_oa = reinterpret_cast<T*>(smem_raw + rec_bytes);
    }
    T* lds_col = lds_oa + (RAYS ? (NT / EPG) * 2 * EPG : 0);           // [NT/EPG][EPG] per-wave body-collision flags
    T* lds_act = lds_col + ((RAYS && !SOLO) ? (NT / EPG) * EPG : 0);   // [NT/EPG][EPG] per-wave list of the envs whose fan reaches an obstacle
    T* lds_hx = lds_act + (RAYS ? (NT / EPG) * EPG : 0);               // [kHxFields][EPG] env phase -> tail waves
    T* lds_spec = lds_hx + (NT / EPG >= 2 ? kHxFields * EPG : 0);      // [kSpecFields][EPG] pre-drawn next episodes
    // [kNavFields][EPG] (SHARE_NAV): in the rows of the per-wave obstacle-avoidance sums that the lane = ray stage leaves
    // unused (it writes slot 0 only; product kernels have no other ray stage) -- config 5's group sits exactly at the
    // 40 KB that let four groups share a CU, there is no LDS to add
    T* lds_nav = lds_oa + 2 * EPG;
    static_assert(!share_nav_<VK, RAYS, EPG, NT, LOG>() || (NT / EPG) * 2 >= 2 + kNavFields, "navigation hand-over needs the spare rows of lds_oa");
    size_t t_bytes = (size_t)(lds_spec + (NT / EPG >= 2 ? kSpecFields * EPG : 0) - lds_pose) * sizeof(T);
    t_bytes = (t_bytes + 15) & ~(size_t)15;
    float* lds_obs = reinterpret_cast<float*>(SOLO ? smem_raw : smem_raw + t_bytes);
    float* const lds_cells = reinterpret_cast<float*>(smem_raw + t_bytes);   // SOLO: [EPG][n_red] ray cells (see above)
    T* const lds_raw = lds_pose;   // regrec: [max_cap][7][EPG] raw capsule rows (nothing else of the carve-up above exists then)
    // where the ray stage accumulates the cells of env e: its row of the tile, or (SOLO without regrec) of the cell array
    auto cell_row = [&](unsigned e, int n_red_) -> float* {
        return (SOLO && !regrec) ? lds_cells + (size_t)e * (unsigned)n_red_ : lds_obs + (size_t)e * row_len + 16;
    };
    T oa_den_r = T(0);   // regrec: the env's obstacle-avoidance denominator (instead of lds_oa)

    // Addressing: every SoA row base (+ this group's first env) is wave-uniform and lives in an SGPR pair; the
    // per-lane part is the 32-bit unsigned lane offset `ul`, so each access is `global_* v, v_off, s[base]` and no
    // 64-bit per-lane address is ever formed or kept alive (they used to cost ~60 VGPRs between load and store).
    const unsigned ul = (unsigned)(tid % EPG);   // lane = env within the group (integrating waves)
    T* g_state = static_cast<T*>(B.state) + env0;
    T* g_plo = static_cast<T*>(B.pos_lo) + env0;
    T* g_u = static_cast<T*>(B.u) + env0;
    T* g_goal = static_cast<T*>(B.goal) + env0;
    T* g_cur = static_cast<T*>(B.cur) + env0;
    T* g_cum = static_cast<T*>(B.cum_reward) + env0;
    T* g_caps = static_cast<T*>(B.caps) + env0;
    T* g_sph = static_cast<T*>(B.sph) + env0;
    int32_t* g_tsteps = B.t_steps + env0;
    int32_t* g_episode = B.episode + env0;
    // compile-time input count where the vehicle kind fixes it (the host sets n_u_max accordingly, dockauv_capi.hip)
    constexpr int NU_CT = (VK == VK_LAUV) ? 3 : ((VK == VK_DENSEB) ? 0 : 6);
    const int n_u_max = NU_CT ? NU_CT : E.n_u_max;

    // Wave roles.  Wave 0 integrates (env phase) and builds the observation; when the group has more waves, one of
    // the otherwise idle ones -- the "bookkeeper" -- takes the other half of the tail: done conditions, reward,
    // episode reset, state write-back, and draws the next episode's random numbers while wave 0 integrates.  For a
    // small batch the step is the latency of ONE wave's instruction stream (~12 k cycles); the split takes ~1/3 off.
    // With a single wave per group the same code runs back to back in wave 0 (the compiler merges the shared parts).
    constexpr int W = NT / EPG;
    constexpr bool DUAL = W >= 2;
    constexpr int BK = DUAL ? (W >= 4 ? 3 : 1) : 0;   // waves 1 and 2 prefetch obstacles when there are four or more
    // With four or more waves the tail is cut in four: wave 0 keeps the navigation-dependent observations and the
    // state write-back, wave OB builds the other thirteen observations, wave RS resets finished envs (and draws
    // their next episode while wave 0 integrates), the bookkeeper is left with conditions + reward.  Each of them
    // recomputes the navigation errors it needs (~100 instructions, side by side on different SIMDs).
    constexpr bool QUAD = W >= 4;
    constexpr int OB = QUAD ? (MIXED2 ? 2 : 1) : 0;   // (MIXED2: wave 1 integrates; the resetter builds the observations too)
    // (EARLY, defined with the tail below; groups of exactly four waves: the resetter shares the observation wave, so
    // that one wave has no tail role and takes the group's first ray pass)
    constexpr bool EARLY_ = early_tail_<VK, RAYS, EPG, NT, LOG>();
    constexpr bool FREE_WAVE = EARLY_ && !MIXED2 && W == 4;
    constexpr int RS = QUAD ? (FREE_WAVE ? OB : 2) : BK;
    // SHARE_NAV (EARLY kernels): the integrating wave alone works out the navigation errors and the done conditions and
    // hands them to the other roles through LDS (they wait for its flag): one decision, ~175 instructions and 14 row loads
    // less per group than three more copies of it; the integrating wave takes no ray pass then.
    constexpr bool SHARE_NAV = share_nav_<VK, RAYS, EPG, NT, LOG>();
    const int wv = __builtin_amdgcn_readfirstlane(tid / EPG);
    const unsigned ule = (unsigned)(tid % EPG);       // lane's env within the group, for any wave
    const bool lane_ok = env0 + (int)ule < A.n_envs;
    const bool bk_lane = (wv == BK) && lane_ok;
    const bool rs_lane = (wv == RS) && lane_ok;
    const bool ob_lane = (wv == OB) && lane_ok;

    // registers that live across the ray stage (env phase lanes only)
    T st[12], nuc[3], goal[4];
    T plo[3] = {T(0), T(0), T(0)};   // float path: low-order words of the position
    T psi_lo = T(0);                 // ... and of the heading (row 3 of the same buffer)
    T Vc = T(0), edot_norm2 = T(0), act_pen = T(0);
    int t_steps = 0;
    // bookkeeper / resetter inputs
    T goal_b[4] = {T(0), T(0), T(0), T(0)}, cum_in = T(0);
    int t_steps_b = 0, episode_in = 0;
    T goal_o[4] = {T(0), T(0), T(0), T(0)};
    int t_steps_o = 0;
    Trig<T> g1{};
    bool collision = false;
    int n_u_env = E.n_u_max;

    T u[kMaxU], act[kMaxU];
    T cdx = T(0), cdy = T(0), cdz = T(0), vmin = T(0), vmax = T(0), w_noise = T(0);
    int vid_l = 0;
    constexpr bool HOT = hot_params_<T, VK, SYM, RAYS, EPG, NT, LOG, TERM, WB, KIND>();
    // NOCUR: nu_c is a literal zero in the right-hand sides -- except in the BlueROV2's ray kernels, where the zero stands in three
    // registers that stay live up to the hand-over, as nu_c's do in the general kernel (no instruction, same sums).  With the
    // literal those kernels took 13 / 18 / 13 SGPR spills (plain / TERM / riding) against their general twins' 10 / 14 / 12; with
    // the registers 6 / 10 / 7.  The other lean kernels stay within their twins' registers and spills either way.
    constexpr bool NUC_REGS = NOCUR && RAYS && VK == VK_JOY;
    // (ray kernels: the action weights stay with EnvP, one round trip of their own -- six more SGPRs across the row loads
    // cost config 3's kernel four more spills)
    constexpr bool HOT_WACT = !RAYS;
    HotRegs<T> HR;   // (HOT: the integrating wave's parameters, see fetch_hot_input_)
    // TAIL: one batch per role for what is read behind the integrator (request_tail_).  The integrating wave asks behind its
    // last right-hand side and awaits behind the post-step trigonometry -- G0: what IT reads there; in groups of four waves it
    // takes no ray pass (NO_PASS) and asks neither for the pass scalars nor for the lane table --, the other waves ask where
    // they idle in front of the hand-over barrier (GH).
    constexpr bool TAIL = tail_params_<T, VK, SYM, RAYS, EPG, NT, LOG, TERM, WB, KIND>();
    constexpr bool NO_PASS = SHARE_NAV && NT / EPG == 4 && !MIXED2;
    constexpr int G0 = kTgDone | kTgAll | (RAYS ? kTgRec : 0) | ((RAYS && !DUAL) ? kTgPass : 0) | (QUAD ? 0 : kTgObs) | (DUAL ? 0 : kTgBk);
    constexpr int GH = kTgAll | (SHARE_NAV ? 0 : kTgDone) | (RAYS ? (kTgRec | kTgPass) : 0) | kTgObs | kTgBk;
    // the tail's parameters (filled below: one batch of scalar loads, pinned -- see pin_sgpr_), the pass waves' and the record
    // completion's
    struct {
        T inv_dmax, inv_log_tol, inv_log_tol_eps, inv_max_att, inv_vel[6], dtol, dmax, max_att;
        T w_d, w_dth, w_dpsi, w_phi, w_th, w_thdot, w_oa, w_done[5];
        int max_timesteps, reward_set, n_obs, reset_mode;
    } Q;
    struct {
        int pad, pad_log2, n_rays, n_red, max_cap, max_sph;
        T ray_max, inv_ray_max, sum_beta;
    } RQ;
    if (!TAIL) {   // (TAIL: no value but the role's own batch -- a zero would make a per-lane merge of it)
        __builtin_memset(&RQ, 0, sizeof(RQ));
    }
    struct { T ray_max, fan_cos, fan_sin, safety; } RC;
    // (the record completion reads a TAIL kernel's pinned copy or, in the kernels that keep their loads at the uses, EnvP)
    auto rc_ray_max = [&]() -> T { if constexpr (TAIL) return RC.ray_max; else return E.ray_max; };
    auto rc_fan_cos = [&]() -> T { if constexpr (TAIL) return RC.fan_cos; else return E.fan_cos; };
    auto rc_fan_sin = [&]() -> T { if constexpr (TAIL) return RC.fan_sin; else return E.fan_sin; };
    auto rc_safety = [&]() -> T { if constexpr (TAIL) return RC.safety; else return E.safety; };
    // What WHOLE waves read behind the integrator -- the terminal copy and the bfloat16 tile store run on every lane of a wave,
    // the lanes of a partial group's missing envs included -- has a source of its own.  The integrating wave's batch is requested
    // and pinned under its lane mask (owner), so Q holds nothing on its other lanes: every thread requests these two words
    // itself, outside every mask, in front of the hand-over barrier, and pins them behind it (TAIL; the others: Q's, below).
    struct { int n_obs, reset_mode; } WQ;
    // episode-storage trace of selected envs (include/dockauv.h: dockauv_trace_*) and its row in the ring for this step
    typedef const __attribute__((address_space(1))) TraceDev GTrace;
    GTrace* const TR = LOG ? (GTrace*)(uintptr_t)IO.trace : nullptr;
    int trace_slot = -1;
    T sigma_l = T(0);
    int episode_l = 0;
    // The integrating waves are the critical path of the step; the helper waves that share their SIMDs (obstacle
    // prefetch, the resetter's Philox draws: quarter-rate integer multiplies) run in its shadow.  VALU issue is
    // arbitrated by priority, then age: the integrators take priority until the env phase is over.
    constexpr bool RAISE_PRIO = NT == 256 && RAYS && VK != VK_MIXED && !LOG;
    if (RAISE_PRIO && wv == 0) __builtin_amdgcn_s_setprio(kPrioLevel);
    if (loader) {
        // ---------------- load (coalesced SoA): everything the step needs is requested up front ----------------
        if (VK == VK_MIXED) vid_l = ldgx_<VOFF>(B.veh_id + env0, 0, S, ul);
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (!(LATE_GOAL && k < 3)) st[k] = ldgx_<VOFF>(g_state, k, S, ul);   // (LATE_GOAL: the position comes behind the stages)
        if (sizeof(T) == 4 && !LATE_GOAL) {
#pragma unroll
            for (int k = 0; k < 3; ++k) plo[k] = ldgx_<VOFF>(g_plo, k, S, ul);
        }
        if (sizeof(T) == 4) psi_lo = ldgx_<VOFF>(g_plo, 3, S, ul);   // (needed at the end of the stages: not a late load)
        const T* actp = static_cast<const T*>(IO.actions) + (size_t)env0 * n_u_max;
#pragma unroll
        for (int k = 0; k < kMaxU; ++k) {
            if (k < n_u_max) {
                u[k] = ldgx_<VOFF>(g_u, k, S, ul);
                act[k] = actp[ul * (unsigned)n_u_max + k];
            } else {
                u[k] = T(0);
                act[k] = T(0);
            }
        }
        if (!NOCUR) {
            Vc = ldgx_<VOFF>(g_cur, 0, S, ul);
            cdx = ldgx_<VOFF>(g_cur, 1, S, ul); cdy = ldgx_<VOFF>(g_cur, 2, S, ul); cdz = ldgx_<VOFF>(g_cur, 3, S, ul);
            vmin = ldgx_<VOFF>(g_cur, 4, S, ul); vmax = ldgx_<VOFF>(g_cur, 5, S, ul);
        }
        // everything the tail of the step needs is requested now as well: a lone wave per SIMD (small batches) has
        // nothing to hide a late load behind.  (Mixed product kernels, at the 128-VGPR limit: held through the stages
        // these five values were spilled to scratch and reloaded; they are requested behind the stages instead.)
        if (!LATE_GOAL) {
#pragma unroll
            for (int k = 0; k < 4; ++k) goal[k] = ldgx_<VOFF>(g_goal, k, S, ul);
            t_steps = ldgx_<VOFF>(g_tsteps, 0, S, ul);
        }
        w_noise = IO.noise ? ldgx_<VOFF>(static_cast<const T*>(IO.noise) + env0, 0, S, ul) : T(0);
        if (LOG && IO.device_noise) {
            sigma_l = ldgx_<VOFF>(static_cast<const T*>(B.cur_sigma) + env0, 0, S, ul);
            episode_l = ldgx_<VOFF>(g_episode, 0, S, ul);
        }
        if (TR) trace_slot = TR->slot_of_env[env0 + (int)ul];
        DOCKAUV_STAMP(1);   // loads issued
        // the integrating wave's input-stage parameters: one batch behind the row loads, whose latency (800-1 900 ticks)
        // covers it
        if constexpr (HOT) fetch_hot_input_<T, VK, HOT_WACT>(PB->H[0], HR);
    }
    // The first touch of a 64-byte line of the parameter block in a launch goes to L2 (~200 cycles on gfx950,
    // scripts/micro/issue_rate.hip; 56 from the scalar cache, which the waves of a CU share), and a lone wave pays each of
    // them in full.  The group's last wave (idle until the hand-over) requests one word of every line the launch reads at
    // once -- with a hot block: its lines first, then EnvP's for the batches of the other roles; nobody reads VehicleP then
    // -- so that they sit in the scalar cache when a role's batch asks for them.
    if (wv == W - 1) {
        typedef const __attribute__((address_space(4))) unsigned CW;
        CW* const pw = (CW*)(uintptr_t)A.params;
        unsigned param_touch = 0;
        typedef ParamBlock<T, 2> PBlock;
        if (HOT) {
            constexpr int h0 = (int)(__builtin_offsetof(PBlock, H) / 4), hw = (int)(sizeof(HotP<T>) / 4);
#pragma unroll
            for (int off = h0; off < h0 + hw; off += 16) param_touch ^= pw[off];
            if (TAIL) {   // (the roles' batches behind the integrator)
                constexpr int q0 = (int)(__builtin_offsetof(PBlock, Q) / 4), qw = (int)(sizeof(TailP<T>) / 4);
#pragma unroll
                for (int off = q0; off < q0 + qw; off += 16) param_touch ^= pw[off];
            }
#pragma unroll
            for (int off = 0; off < (int)(sizeof(EnvP<T>) / 4); off += 16) param_touch ^= pw[off];
        } else {
#pragma unroll
            for (int off = 0; off < (int)(__builtin_offsetof(PBlock, H) / 4); off += 16) param_touch ^= pw[off];
        }
        asm volatile("" ::"s"(param_touch));
    }
    // (after wave 0's loads in program order: wave 0 is the critical path)
    if (bk_lane || rs_lane) {
        if (!SHARE_NAV) {   // (SHARE_NAV: goal and step counter are the integrating wave's business alone)
#pragma unroll
            for (int k = 0; k < 4; ++k) goal_b[k] = ldgx_<VOFF>(g_goal, k, S, ule);
        }
        t_steps_b = ldgx_<VOFF>(g_tsteps, 0, S, ule);
        cum_in = ldgx_<VOFF>(g_cum, 0, S, ule);
        episode_in = ldgx_<VOFF>(g_episode, 0, S, ule);
    }
    if (QUAD && ob_lane && !SHARE_NAV) {
#pragma unroll
        for (int k = 0; k < 4; ++k) goal_o[k] = ldgx_<VOFF>(g_goal, k, S, ule);
        t_steps_o = ldgx_<VOFF>(g_tsteps, 0, S, ule);
    }

    if (RAYS && (!LOG || E.n_rays <= 64)) {
        // lane-per-ray stage: block maxima are accumulated in the observation tile with LDS atomics and only wave
        // slot 0 of the partial sums is written per env -> both start from zero (ordered by the barriers below)
        // (lane = env, cells strided over the helper waves: no integer division by the run-time cell count, and nothing
        // of it in the integrating waves, whose instruction stream is the step's critical path -- this block used to cost
        // wave 0 ~100 instructions in front of the env phase)
        constexpr int W_ = NT / EPG;
        constexpr int NI = W_ == 1 ? 0 : (MIXED2 ? 2 : 1);          // integrating waves
        constexpr int NH = W_ - NI;                                  // helper waves (W_ = 1: wave 0 does it itself)
        const int hw = wv - NI;
        if ((W_ == 1 && !regrec) || hw >= 0) {   // (regrec: behind the record completion, these bytes hold raw rows until then)
            const int step = W_ == 1 ? 1 : NH, first = W_ == 1 ? 0 : hw;
            const int n_red_z = E.n_red;
            float* orow = cell_row(ule, n_red_z);
            for (int k = first; k < n_red_z; k += step) orow[k] = 0.0f;
            for (int k = first; k < W_ * 2; k += step) lds_oa[k * EPG + ule] = T(0);
            if (first == 0 && !SOLO) {
                if (!NOCAP) lds_pose[14 * EPG + ule] = T(0);   // may-be-hit masks (bit patterns: all zero)
                lds_pose[15 * EPG + ule] = T(0);
                if (SHARE_NAV && ule < 2) lds_nav[4 * EPG + ule] = T(0);   // "navigation errors published" flags
            }
        }
    }
    // SOLO: slot counts and may-be-hit masks of the lane's env (registers instead of pose rows)
    int ncap_r = 0, nsph_r = 0;
    unsigned cmask_r = 0u, smask_r = 0u;
    T rr[REGREC_OK ? kRegCaps : 1][kCapFields] = {};   // regrec: the completed capsule records of the lane's env
    if (RAYS) {
        // ---------------- obstacle prefetch ----------------
        // The raw obstacle rows go from HBM to LDS while the vehicle is being integrated: by the group's second /
        // third wave (idle until the ray stage) when there is one, else by this wave right behind its state loads.
        // Only the pose-independent part is done here (unit axis, length); the env phase completes the records
        // from LDS once the new pose exists.  (Loading them after the integration, one capsule at a time, cost the
        // env phase a memory round trip per capsule: ~7 000 cycles for 5 capsules.)
        // raw capsule record, in the slots of the final one: c1(3) d(3) |ba| r ; raw sphere record: c(3) r
        constexpr int W = NT / EPG;
        const int pw = tid / EPG, pe = tid % EPG;
        const bool pvalid = env0 + pe < A.n_envs;
        if (pvalid && pw == (MIXED2 ? 2 : (W > 1 ? 1 : 0))) {
            int ncap = 0;
            bool open = true;
            for (int c = 0; c < E.max_cap; ++c) {
                const T* cg = g_caps + (size_t)c * 7 * S;
                const unsigned pl = (unsigned)pe;
                const T c1x = ldgx_<VOFF>(cg, 0, S, pl), c1y = ldgx_<VOFF>(cg, 1, S, pl), c1z = ldgx_<VOFF>(cg, 2, S, pl);
                const T bax = ldgx_<VOFF>(cg, 3, S, pl) - c1x, bay = ldgx_<VOFF>(cg, 4, S, pl) - c1y, baz = ldgx_<VOFF>(cg, 5, S, pl) - c1z;
                const T rad = ldgx_<VOFF>(cg, 6, S, pl);
                if (SOLO && regrec) {   // (unit axis and length: with the record, same expressions)
                    T* rp = lds_raw + (size_t)c * 7 * EPG + pe;
                    rp[0 * EPG] = c1x; rp[1 * EPG] = c1y; rp[2 * EPG] = c1z;
                    rp[3 * EPG] = bax; rp[4 * EPG] = bay; rp[5 * EPG] = baz;
                    rp[6 * EPG] = rad;
                    open = open && (rad > T(0));
                    ncap = open ? c + 1 : ncap;
                    continue;
                }
                const T len = sqrt_(bax * bax + bay * bay + baz * baz);
                const T inv_len = rcp_(len);
                T* cp = lds_cap + (size_t)c * kCapFields * EPG + pe;
                cp[0 * EPG] = c1x; cp[1 * EPG] = c1y; cp[2 * EPG] = c1z;
                cp[3 * EPG] = bax * inv_len; cp[4 * EPG] = bay * inv_len; cp[5 * EPG] = baz * inv_len;
                cp[6 * EPG] = len;
                cp[7 * EPG] = rad;
                open = open && (rad > T(0));
                ncap = open ? c + 1 : ncap;
            }
            if (SOLO) ncap_r = ncap; else lds_pose[0 * EPG + pe] = T(ncap);
        }
        if (pvalid && pw == (MIXED2 ? 3 : (W > 2 ? 2 : 0))) {
            int nsph = 0;
            bool open = true;
            for (int s_i = 0; s_i < E.max_sph; ++s_i) {
                T rad = T(0);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    rad = ldgx_<VOFF>(g_sph, s_i * 4 + k, S, (unsigned)pe);
                    lds_sph[(size_t)(s_i * kSphFields + k) * EPG + pe] = rad;
                }
                open = open && (rad > T(0));
                nsph = open ? s_i + 1 : nsph;
            }
            if (SOLO) nsph_r = nsph; else lds_pose[1 * EPG + pe] = T(nsph);
            if (W == 4 && !MIXED2) DOCKAUV_STAMP_WAVES(28);   // (diagnostic build) slot 30: the sphere rows are in LDS
        }
    }

    if (DUAL && rs_lane && E.reset_mode == 2) {
        // next episode: uniforms and scenario mapping, done while wave 0 integrates.  Only lanes whose episode ends in
        // this step will use it, so it is parked in LDS (read back by the same lane) rather than held in 19 registers
        // through the ray stage.
        T Ub[12], pose_s[6], goal_s[4], cur_s[8], ring_s;
        episode_uniforms_<T, NOCAP>(E, env0 + (int)ule, episode_in + 1, Ub);
        generate_episode_<T>(E, Ub, pose_s, goal_s, cur_s, ring_s);
#pragma unroll
        for (int k = 0; k < 6; ++k) lds_spec[k * EPG + ule] = pose_s[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) lds_spec[(6 + k) * EPG + ule] = goal_s[k];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (!NOCUR) lds_spec[(10 + k) * EPG + ule] = cur_s[k];   // (NOCUR: the resetter writes no current row)
        if (!NOCAP) lds_spec[18 * EPG + ule] = ring_s;   // (NOCAP: no capsule rows, nobody reads the ring's angle)
    }

    if (MIXED2) owner = loader && (vid_l == wv);
    if (owner) {
        size_t trace_row = 0;
        if (TR && trace_slot >= 0) {
            trace_row = (size_t)(IO.trace_step % TR->capacity) * (size_t)TR->n_rows + (size_t)trace_slot;
            T* sp = static_cast<T*>(TR->state_pre) + trace_row * 12;
#pragma unroll
            for (int k = 0; k < 12; ++k) sp[k] = st[k];
        }
        // ---------------- 1. Current.sim (objects/current.py:78-96) ----------------
        if (LOG && IO.device_noise && __any(sigma_l != T(0)))
            w_noise = sigma_l * device_normal_<T>(E.seed, env0 + (int)ul, episode_l, t_steps);
        if constexpr (!NOCUR) {   // (NOCUR: V_c = 0 stays 0 under the filter and the clip to [0, 0])
            if constexpr (HOT) Vc += (-HR.mu * Vc + w_noise) * HR.h; else Vc += (-E.mu * Vc + w_noise) * E.h;
            Vc = clip_(Vc, vmin, vmax);
        }
        // ---------------- 2. nu_c = R(Theta_pre)^T v_c^n (objects/current.py:33-53) ----------------
        nuc[0] = nuc[1] = nuc[2] = T(0);
        if (NUC_REGS) {
#pragma unroll
            for (int k = 0; k < 3; ++k) asm volatile("" : "+v"(nuc[k]));
        }
        if (!NOCUR && __any(Vc != T(0))) {   // scenarios without current: V_c = 0 in every lane, nu_c = R^T 0 = 0
            const Trig<T> g0 = trig_(st[3], st[4], st[5]);
            rot_ned_to_body_(g0, Vc * cdx, Vc * cdy, Vc * cdz, nuc);
        }
        DOCKAUV_STAMP_PIN(2, nuc, 3);   // loads landed, nu_c done
        // ---------------- 3. vehicle ----------------
        T dpos[3];
        int vid = 0;
        if (VK == VK_MIXED) {
            vid = vid_l;
            n_u_env = vid == 0 ? 6 : 3;
        } else {
            n_u_env = (VK == VK_LAUV) ? 3 : (VK == VK_JOY ? 6 : PB->V[0].n_u);
        }
        {
            // the raw action is reduced to the one number the reward needs (docking3d.py:584-585) before the
            // integrator runs: nothing of it stays live through the stages
            const T inv_nu = n_u_env == 6 ? T(1.0 / 6.0) : (n_u_env == 3 ? T(1.0 / 3.0) : rcp_(T(n_u_env)));
#pragma unroll
            for (int k = 0; k < kMaxU; ++k) {
                if (k < n_u_env) {
                    const T a = abs_(act[k]) * inv_nu;   // raw, un-clipped action
                    if constexpr (HOT && HOT_WACT) act_pen += a * a * HR.w_act[k]; else act_pen += a * a * E.w_act[k];
                }
            }
        }
        if constexpr (HOT) {
            vehicle_step_<T, VK, SYM, VOFF, true>(HR.V, HR, st + 3, dpos, u, act, nuc, g_u, S, ul, psi_lo,
                                                  [&]() { request_hot_kinetics_<T, VK>(PB->H[0], HR); },
                                                  [&]() { pin_hot_kinetics_<T, VK>(HR); },
                                                  [&]() { if constexpr (TAIL) request_tail_<G0>(PB->Q, Q, RC, RQ); });
        } else if (VK == VK_MIXED) {
            if (vid == 0) {
                vehicle_step_<T, VK_JOY, SYM, VOFF>(PB->V[0], E, st + 3, dpos, u, act, nuc, g_u, S, ul, psi_lo);
            } else {
                vehicle_step_<T, VK_LAUV, SYM, VOFF>(PB->V[1], E, st + 3, dpos, u, act, nuc, g_u, S, ul, psi_lo);
            }
        } else {
            vehicle_step_<T, VK, SYM, VOFF>(PB->V[0], E, st + 3, dpos, u, act, nuc, g_u, S, ul, psi_lo);
        }
        // The position is the one state the dynamics do not damp: x += dx once per step, ~0.05 m onto up to 20 m.  In
        // float32 every such sum drops up to half an ulp of x (1e-6 m) for good, and over an episode the losses add up to
        // 2-3e-5 m -- which near the goal, where the observations divide by the distance, is the whole 1e-5 budget
        // (profiles/r1_parity_drift_f32.txt).  Two-float accumulation: the rounding error of each sum (Knuth's two-sum:
        // exact) is carried in pos_lo and fed into the next step's increment; state[0:3] stays the correctly rounded
        // position.  float64 needs none of it.
        auto update_position = [&]() {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (sizeof(T) == 4) {
                    const T b = dpos[k] + plo[k];
                    const T s_ = st[k] + b;
                    const T bb = s_ - st[k];
                    plo[k] = (st[k] - (s_ - bb)) + (b - bb);
                    st[k] = s_;
                } else {
                    st[k] += dpos[k];
                }
            }
        };
        if (!LATE_GOAL) update_position();
        DOCKAUV_STAMP_PIN(3, st + 3, 9);   // RK step done
        if (LATE_GOAL) {
            // what the stages did not need: position (the right-hand side does not depend on it), its low-order words,
            // goal and step counter -- requested here, in flight behind the post-step trigonometry
#pragma unroll
            for (int k = 0; k < 3; ++k) st[k] = ldgx_<VOFF>(g_state, k, S, ul);
            if (sizeof(T) == 4) {
#pragma unroll
                for (int k = 0; k < 3; ++k) plo[k] = ldgx_<VOFF>(g_plo, k, S, ul);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) goal[k] = ldgx_<VOFF>(g_goal, k, S, ul);
            t_steps = ldgx_<VOFF>(g_tsteps, 0, S, ul);
        }
        // post-step trig of the wrapped attitude: euler_dot (Q4, auvsim.py:108), ray rotation, obs[8:10]
        g1 = RAYS ? trig_accurate_(st[3], st[4], st[5]) : trig_(st[3], st[4], st[5]);
        {
            const T sq_cr = (g1.sf * st[10] + g1.cf * st[11]) * rcp_(g1.ct);
            const T e0 = st[9] + sq_cr * g1.st, e1 = g1.cf * st[10] - g1.sf * st[11], e2 = sq_cr;
            edot_norm2 = e0 * e0 + e1 * e1 + e2 * e2;
        }
        if (LATE_GOAL) update_position();
        if (LOG && (IO.state_dot || (TR && trace_slot >= 0))) {
            // logging only: the full right-hand side at the new state (u[] holds the filtered input since vehicle_step_)
            T uu[kMaxU], sd[12];
#pragma unroll
            for (int k = 0; k < kMaxU; ++k) uu[k] = (k < n_u_env) ? u[k] : T(0);
            if (VK == VK_MIXED) {
                if (vid == 0) post_step_rhs_<T, VK_JOY, SYM>(PB->V[0], st, g1, nuc, uu, sd);
                else post_step_rhs_<T, VK_LAUV, SYM>(PB->V[1], st, g1, nuc, uu, sd);
            } else {
                post_step_rhs_<T, VK, SYM>(PB->V[0], st, g1, nuc, uu, sd);
            }
            if (IO.state_dot) {
                T* o = static_cast<T*>(IO.state_dot) + ((size_t)env0 + ul) * 12;
#pragma unroll
                for (int k = 0; k < 12; ++k) o[k] = sd[k];
            }
            if (TR && trace_slot >= 0) {
                T* o1 = static_cast<T*>(TR->state) + trace_row * 12;
                T* o2 = static_cast<T*>(TR->state_dot) + trace_row * 12;
                T* o3 = static_cast<T*>(TR->u) + trace_row * kMaxU;
                T* o4 = static_cast<T*>(TR->nu_c) + trace_row * 3;
#pragma unroll
                for (int k = 0; k < 12; ++k) { o1[k] = st[k]; o2[k] = sd[k]; }
#pragma unroll
                for (int k = 0; k < kMaxU; ++k) o3[k] = uu[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) o4[k] = nuc[k];
            }
        }
        // (TAIL: the integrating wave's batch, requested behind the last right-hand side, has landed behind the trigonometry.
        // Request and pin stand under the wave's lane mask: on this wave only the lanes that integrate an env hold them, and only
        // those lanes read them -- every later use on this wave is the role's own, under the same mask (record completion,
        // w0_tail); what a whole wave reads comes from WQ.)
        if constexpr (TAIL) pin_tail_<G0>(Q, RC, RQ);
    }

    if (RAISE_PRIO && wv == 0) __builtin_amdgcn_s_setprio(0);
    // TAIL: the other waves' batch, where they idle in front of the hand-over barrier
    if constexpr (TAIL && DUAL) {
        static_assert(NO_PASS, "an integrating wave that takes ray passes would need their scalars here");
        if (wv != 0) {
            request_tail_<GH>(PB->Q, Q, RC, RQ);
            pin_tail_<GH>(Q, RC, RQ);
        }
    }
    // (every thread, outside every mask: the line is in the scalar cache by now, and the wait of the pose's LDS writes in front
    // of the barrier covers the trip)
    if constexpr (TAIL) { WQ.n_obs = PB->Q.n_obs; WQ.reset_mode = PB->Q.reset_mode; }
    // what the bookkeeper needs from the env phase: new state (12), V_c, action penalty, |euler_dot|^2, collision
    // (SHARE_NAV kernels: the integrating wave alone needs position and heading -- navigation errors -- and writes the
    // state of the envs that go on itself; V_c only travels with a reset, whose resetter takes the new one; the collision
    // flag comes from the records: six rows nobody reads are not written)
    constexpr bool LEAN_HX = share_nav_<VK, RAYS, EPG, NT, LOG>();
    auto publish_hx = [&]() {
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (!(LEAN_HX && (k < 3 || k == 5))) lds_hx[k * EPG + ul] = st[k];
        if (!LEAN_HX && !NOCUR) lds_hx[12 * EPG + ul] = Vc;
        lds_hx[13 * EPG + ul] = act_pen;
        lds_hx[14 * EPG + ul] = edot_norm2;
        if (!LEAN_HX) lds_hx[15 * EPG + ul] = collision ? T(1) : T(0);
        if (QUAD) {
            if (!NOCUR) {
#pragma unroll
                for (int k = 0; k < 3; ++k) lds_hx[(16 + k) * EPG + ul] = nuc[k];
            } else if (NUC_REGS) {
#pragma unroll
                for (int k = 0; k < 3; ++k) asm volatile("" ::"v"(nuc[k]));
            }
            lds_hx[19 * EPG + ul] = g1.sp;
            lds_hx[20 * EPG + ul] = g1.cp;
        }
    };
    if (DUAL && !RAYS) {
        if (owner) publish_hx();
        // the bookkeeper may overwrite the filtered-input rows (reset): wave 0's stores to them, issued before the
        // integrator, must have left the wave (they have; the wait is free)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        lds_barrier_<NT>();
    }

    // Ray stage of fans of <= 64 rays (lane = ray): what a lane needs to know about its ray comes from a host-built
    // table (lane -> ray of its env slot: body-frame direction, obstacle-avoidance weight, block-max cell), and the
    // stage's parameters are fetched as ONE batch of scalar loads; both are requested here, before the record
    // completion, so that they have landed when the stage starts (they used to be fetched one by one at its start:
    // a dozen exposed scalar-cache round trips, four integer divisions and a global load in front of the first pass)
    // (TAIL: the scalars came with the role's batch; an integrating wave that takes no pass needs no ray either)
    T lr_bx = T(0), lr_by = T(0), lr_bz = T(0), lr_beta = T(0);
    int lr_cell = 0;
    if (RAYS && (!LOG || E.n_rays <= 64)) {
        if (!TAIL) {
            RQ.pad = E.ray_pad; RQ.pad_log2 = E.ray_pad_log2; RQ.n_rays = E.n_rays; RQ.n_red = E.n_red;
            RQ.max_cap = E.max_cap; RQ.max_sph = E.max_sph;
            RQ.ray_max = E.ray_max; RQ.inv_ray_max = E.inv_ray_max; RQ.sum_beta = E.sum_beta;
        }
        if (!(TAIL && NO_PASS && wv == 0)) {
            typedef const __attribute__((address_space(1))) T GT;
            typedef const __attribute__((address_space(1))) int GI;
            GT* const lt = (GT*)(uintptr_t)B.lane_tab + (unsigned)(tid % 64) * 4u;
            lr_bx = lt[0]; lr_by = lt[1]; lr_bz = lt[2]; lr_beta = lt[3];
            lr_cell = ((GI*)(uintptr_t)B.lane_cell)[tid % 64];
        }
    }

    // ------------------------------------------------------------------------------------------ tail (definitions)
    // The tail of the step in roles: wave 0 (navigation-dependent observations), OB (the other thirteen), BK
    // (conditions, reward, counters), RS (state write-back, episode reset).  Nothing of it needs the ray stage except
    // the reward's obstacle-avoidance term and the zeroing of a finished env's ray cells, so in the product kernels
    // with four or more waves (EARLY) every role runs BEFORE the barrier behind the ray stage -- wave 0 right after the
    // record completion, the others behind their ray passes -- and only those two leftovers behind it.  With the
    // roles behind that barrier (as the full instantiation still has them) the group spent ~2 000 cycles at 4 waves per
    // SIMD there while most of its waves had idled through the ray stage (config 3: ~1 env in 100 takes a pass).
    constexpr bool EARLY = EARLY_;
    // the tail's parameters, fetched as one batch of scalar loads and pinned (see pin_sgpr_) -- TAIL: per role, above
    if constexpr (!TAIL) {
        Q.inv_dmax = E.inv_dmax; Q.inv_log_tol = E.inv_log_tol; Q.inv_log_tol_eps = E.inv_log_tol_eps;
        Q.inv_max_att = E.inv_max_att; Q.dtol = E.dtol; Q.dmax = E.dmax; Q.max_att = E.max_att;
        Q.w_d = E.w_d; Q.w_dth = E.w_dth; Q.w_dpsi = E.w_dpsi; Q.w_phi = E.w_phi; Q.w_th = E.w_th;
        Q.w_thdot = E.w_thdot; Q.w_oa = E.w_oa;
        Q.max_timesteps = E.max_timesteps; Q.reward_set = E.reward_set; Q.n_obs = E.n_obs; Q.reset_mode = E.reset_mode;
#pragma unroll
        for (int k = 0; k < 6; ++k) Q.inv_vel[k] = E.inv_vel[k];
#pragma unroll
        for (int k = 0; k < 5; ++k) Q.w_done[k] = E.w_done[k];
        Q.inv_dmax = pin_sgpr_(Q.inv_dmax); Q.inv_log_tol = pin_sgpr_(Q.inv_log_tol);
        Q.inv_log_tol_eps = pin_sgpr_(Q.inv_log_tol_eps); Q.inv_max_att = pin_sgpr_(Q.inv_max_att);
        Q.dtol = pin_sgpr_(Q.dtol); Q.dmax = pin_sgpr_(Q.dmax); Q.max_att = pin_sgpr_(Q.max_att);
        Q.w_d = pin_sgpr_(Q.w_d); Q.w_dth = pin_sgpr_(Q.w_dth); Q.w_dpsi = pin_sgpr_(Q.w_dpsi);
        Q.w_phi = pin_sgpr_(Q.w_phi); Q.w_th = pin_sgpr_(Q.w_th); Q.w_thdot = pin_sgpr_(Q.w_thdot);
        Q.w_oa = pin_sgpr_(Q.w_oa);
        Q.max_timesteps = pin_sgpr_(Q.max_timesteps); Q.reward_set = pin_sgpr_(Q.reward_set); Q.n_obs = pin_sgpr_(Q.n_obs);
        Q.reset_mode = pin_sgpr_(Q.reset_mode);
#pragma unroll
        for (int k = 0; k < 6; ++k) Q.inv_vel[k] = pin_sgpr_(Q.inv_vel[k]);
#pragma unroll
        for (int k = 0; k < 5; ++k) Q.w_done[k] = pin_sgpr_(Q.w_done[k]);
        WQ.n_obs = Q.n_obs; WQ.reset_mode = Q.reset_mode;
    }

    // 9. navigation errors (envs/docking3d.py:404-413) -- both halves of the tail need them
    // (the squared distance is formed by explicit fused multiply-adds in ONE order wherever it is needed: the roles
    // that decide `done` side by side -- observation rows zeroed, reward flag, reset -- must get the same bits)
    auto dist2_xy = [](T dx, T dy) { return fma_(dy, dy, dx * dx); };
    auto dist2_xyz = [&](T dx, T dy, T dz) { return fma_(dz, dz, dist2_xy(dx, dy)); };
    auto nav_errors = [&](const T* s_, const T* g_, T& dd, T& dth, T& dpsi) {
        const T dx = g_[0] - s_[0], dy = g_[1] - s_[1], dz = g_[2] - s_[2];
        dd = sqrt_(dist2_xyz(dx, dy, dz));
        const T dxy = sqrt_(dist2_xy(dx, dy));
        dth = s_[4] + atan2_(dz, dxy);   // ssa(atan2(dz, |dxy|)) is the identity: the angle lies in [-pi/2, pi/2]
        dpsi = ssa_(atan2_(dy, dx) - s_[5]);
    };
    // distance to the goal alone: all the done conditions need of the navigation errors
    auto goal_dist = [&](const T* s_, const T* g_) {
        const T dx = g_[0] - s_[0], dy = g_[1] - s_[1], dz = g_[2] - s_[2];
        return sqrt_(dist2_xyz(dx, dy, dz));
    };
    // 11. done conditions (envs/docking3d.py:597-631) as bits 0..4
    auto conditions = [&](T dd, const T* s_, int tsteps, bool col) -> int {
        const bool c0 = dd < Q.dtol;
        const bool c1 = dd > Q.dmax;
        const bool c2 = (abs_(s_[3]) > Q.max_att) || (abs_(s_[4]) > Q.max_att);
        const bool c3 = tsteps >= Q.max_timesteps;
        return (c0 ? 1 : 0) | (c1 ? 2 : 0) | (c2 ? 4 : 0) | (c3 ? 8 : 0) | (col ? 16 : 0);
    };

    // ---------------- observation: the thirteen entries that do not depend on the navigation errors, ray cells ----------------
    // (wave 0 itself below unless the group has four waves: then wave OB, from the hand-over)
    // row of lane's env in the trace ring for this step, or null
    auto trace_obs_row = [&](unsigned lane) -> float* {
        if (!TR) return nullptr;
        const int slot = TR->slot_of_env[env0 + (int)lane];
        if (slot < 0) return nullptr;
        return TR->obs + ((size_t)(IO.trace_step % TR->capacity) * (size_t)TR->n_rows + (size_t)slot) * (size_t)Q.n_obs;
    };
    // SHARE_NAV: the roles' view of the integrating wave's decision.  The flag is raised by wave 0 right behind its own
    // tail, which nothing of this group can hold up (it waits for no other wave between the barrier in front of the ray
    // stage and that point): the wait ends.
    // Ordering by the memory model, not by what the hardware happens to do: the integrating wave publishes its rows,
    // RELEASES them (workgroup scope, LDS) and raises an atomic flag (raise_nav_flag_); a waiting role polls the flag with
    // atomic loads and ACQUIRES behind the loop, so neither a row store can sink below the flag store nor a row load
    // rise above the loop.  The wait is bounded: a role that never sees the flag (an integrating wave that left early
    // would be a bug of this kernel) gives up after ~30 ms, sets bit 0 of the handle's sticky status word -- the host
    // reports it at its next synchronisation (DOCKAUV_E_KERNEL) -- and the grid drains instead of hanging the chip.
    int* const nav_flags = reinterpret_cast<int*>(lds_nav + 4 * EPG);   // (mixed groups: one flag per integrating wave, a T apart)
    auto raise_nav_flag_ = [&](int which) {
        // (fault injection, test library only -- csrc/build.py: libdockauv_faultinject.so: group 0 never raises its flag, so
        // that tests/test_gpu_status.py can watch the bounded wait give up and the status word reach the host)
        if (DOCKAUV_FAULT_INJECT_DROP_NAV_FLAG && bix == 0) return;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __hip_atomic_store(reinterpret_cast<int*>(lds_nav + 4 * EPG + which), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    auto wait_nav_ = [&]() {
        unsigned spins = 0;
        for (;;) {
            int f = __hip_atomic_load(nav_flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (MIXED2) f &= __hip_atomic_load(reinterpret_cast<int*>(lds_nav + 4 * EPG + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (__builtin_amdgcn_readfirstlane(f) != 0) break;
            if (++spins > (1u << 18)) {
                const int me = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                if (me == __builtin_amdgcn_readfirstlane(me))   // (the wave's first active lane; the word is host memory: system scope)
                    __hip_atomic_fetch_or(B.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                break;
            }
            __builtin_amdgcn_s_sleep(kNavSleep);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    };
    auto wait_nav = wait_nav_;
    bool ob_zero_row = false;
    // ray cells of a finished env's row (after the ray stage): copies for terminal_obs / the trace, then zeros
    auto obs_ray_cells = [&](bool zero_row, unsigned lane) {
        if (TERM) return;   // (nothing to copy or zero here: see the terminal copy in front of the tile store)
        float* ot = lds_obs + (size_t)lane * row_len;
        if (SOLO && regrec) {   // (the cells are in place)
            if (zero_row)
                for (int k = 16; k < Q.n_obs; ++k) ot[k] = 0.0f;
            return;
        }
        if (SOLO) {   // the cells move from their own array into the tile, which only now may overwrite the obstacle records
            const float* cr = lds_cells + (size_t)lane * (unsigned)(Q.n_obs - 16);
            for (int k = 16; k < Q.n_obs; ++k) ot[k] = zero_row ? 0.0f : cr[k - 16];
            return;
        }
        if (zero_row && IO.terminal_obs) {
            float* to = IO.terminal_obs + (size_t)env0 * Q.n_obs + lane * (unsigned)Q.n_obs;
            for (int k = 16; k < Q.n_obs; ++k) to[k] = ot[k];
        }
        if (float* tro = trace_obs_row(lane))   // episode storage: the observation before any auto-reset zeroing
            for (int k = 16; k < Q.n_obs; ++k) tro[k] = ot[k];
        if (zero_row)
            for (int k = 16; k < Q.n_obs; ++k) ot[k] = 0.0f;
    };
    // (lazy_done: SHARE_NAV's observation wave learns `done` from the integrating wave -- it asks once its own thirteen
    // values exist, right in front of the first use)
    auto obs_rest = [&](const T* s_, const T* nuc_, T sp_, T cp_, bool zero_row, unsigned lane, bool lazy_done = false) {
        float* ot = lds_obs + (size_t)lane * row_len;
        T o[16];
        o[3] = clip_(s_[6] * Q.inv_vel[0], T(-1), T(1));
        o[4] = clip_(s_[7] * Q.inv_vel[1], T(-1), T(1));
        o[5] = clip_(s_[8] * Q.inv_vel[2], T(-1), T(1));
        o[6] = clip_(s_[3] * Q.inv_max_att, T(-1), T(1));
        o[7] = clip_(s_[4] * Q.inv_max_att, T(-1), T(1));
        o[8] = clip_(sp_, T(-1), T(1));
        o[9] = clip_(cp_, T(-1), T(1));
        o[10] = clip_(s_[9] * Q.inv_vel[3], T(-1), T(1));
        o[11] = clip_(s_[10] * Q.inv_vel[4], T(-1), T(1));
        o[12] = clip_(s_[11] * Q.inv_vel[5], T(-1), T(1));
        if constexpr (NOCUR) {   // (clip(+0 * 0.5, -1, 1))
            o[13] = o[14] = o[15] = T(0);
        } else {
            o[13] = clip_(nuc_[0] * T(0.5), T(-1), T(1));
            o[14] = clip_(nuc_[1] * T(0.5), T(-1), T(1));
            o[15] = clip_(nuc_[2] * T(0.5), T(-1), T(1));
        }
        if (SHARE_NAV && lazy_done && !TERM) {   // (TERM: this role never zeroes: it does not need to know)
#pragma unroll
            for (int k = 3; k < 16; ++k) asm volatile("" : "+v"(o[k]));   // (the values exist before the wait starts)
            wait_nav_();
            zero_row = (lds_nav[3 * EPG + lane] != T(0)) && Q.reset_mode != 0;
            ob_zero_row = zero_row;
        }
        // VecEnv auto-reset: the row of a finished env is the reference's reset observation = all zeros
        // (Q8, docking3d.py:269,322); the terminal one goes to terminal_obs
        if (TERM) zero_row = false;   // (the tile keeps the true row until the terminal copy behind its last barrier)
        if (zero_row && IO.terminal_obs) {
            float* to = IO.terminal_obs + (size_t)env0 * Q.n_obs + lane * (unsigned)Q.n_obs;
#pragma unroll
            for (int k = 3; k < 16; ++k) to[k] = (float)o[k];
            if (!RAYS)
                for (int k = 16; k < Q.n_obs; ++k) to[k] = 1.0f;
        }
        if (float* tro = trace_obs_row(lane)) {   // episode storage: the observation before any auto-reset zeroing
#pragma unroll
            for (int k = 3; k < 16; ++k) tro[k] = (float)o[k];
            if (!RAYS)
                for (int k = 16; k < Q.n_obs; ++k) tro[k] = 1.0f;
        }
#pragma unroll
        for (int k = 3; k < 16; ++k) ot[k] = zero_row ? 0.0f : (float)o[k];
        if (!RAYS) {
            const float fill = zero_row ? 0.0f : 1.0f;     // every ray reports max_dist
            int k = 16;
            if ((row_len & 1) == 0)                         // rows start 8-B aligned: two cells per LDS write
                for (; k + 2 <= Q.n_obs; k += 2) *reinterpret_cast<float2*>(ot + k) = make_float2(fill, fill);
            for (; k < Q.n_obs; ++k) ot[k] = fill;
            if (IO.ray_dist)
                for (int r = 0; r < E.n_rays; ++r) (static_cast<T*>(IO.ray_dist) + (size_t)env0 * E.n_rays)[lane * (unsigned)E.n_rays + r] = E.ray_max;
        }
    };

    // body collision of the lane's env, for the roles that run before wave 0 could hand it over: the OR of the
    // waves' flags of the record completion (complete behind the barrier in front of the ray stage)
    auto col_from_records = [&](unsigned lane) -> bool {
        bool c = false;
#pragma unroll
        for (int w = 0; w < W; ++w) c = c || (lds_col[w * EPG + lane] != T(0));
        return c;
    };

    // ---------------- wave 0: navigation-dependent observations, low-order position words ----------------
    auto w0_tail = [&]() {
        DOCKAUV_STAMP(4);   // ray stage done
        T dd, dth, dpsi;
        nav_errors(st, goal, dd, dth, dpsi);
        // 10. observation (envs/docking3d.py:462-488); divisions by configuration constants are multiplications by
        // reciprocals prepared on the host (EnvP)
        float* ot = lds_obs + (size_t)ul * row_len;
        const T o0 = clip_(T(1) - log_(dd * Q.inv_dmax) * Q.inv_log_tol, T(0), T(1));
        const T o1 = clip_(dth * (T(2) / pi_<T>()), T(-1), T(1));
        const T o2 = clip_(dpsi * (T(1) / pi_<T>()), T(-1), T(1));
        const int cbits0 = conditions(dd, st, t_steps, collision);
        const bool done = cbits0 != 0;
        const bool zero_row = done && Q.reset_mode != 0;
        if (SHARE_NAV) {
            // what the other roles need of this: they wait for the flag (release / acquire pair, see wait_nav_)
            lds_nav[0 * EPG + ul] = dd;
            lds_nav[1 * EPG + ul] = dth;
            lds_nav[2 * EPG + ul] = dpsi;
            lds_nav[3 * EPG + ul] = T(cbits0);
            raise_nav_flag_(MIXED2 ? wv : 0);
        }
        if (zero_row && IO.terminal_obs) {
            float* to = IO.terminal_obs + (size_t)env0 * Q.n_obs + ul * (unsigned)Q.n_obs;
            to[0] = (float)o0; to[1] = (float)o1; to[2] = (float)o2;
        }
        if (float* tro = trace_obs_row(ul)) {
            tro[0] = (float)o0; tro[1] = (float)o1; tro[2] = (float)o2;
        }
        const bool zero_tile = zero_row && !TERM;
        ot[0] = zero_tile ? 0.0f : (float)o0;
        ot[1] = zero_tile ? 0.0f : (float)o1;
        ot[2] = zero_tile ? 0.0f : (float)o2;
        if (!QUAD) {
            obs_rest(st, nuc, g1.sp, g1.cp, zero_row, ul);
            if (RAYS) obs_ray_cells(zero_row, ul);
        }
        if (DUAL && !zero_row) {
            // this wave still holds the new state: it writes the state of the envs that go on, the resetter the others
#pragma unroll
            for (int k = 0; k < 12; ++k) stgx_<VOFF>(g_state, k, S, ul, st[k]);
            if (!NOCUR) stgx_<VOFF>(g_cur, 0, S, ul, Vc);
        }
        if (sizeof(T) == 4) {   // (a new episode starts with exact coordinates)
#pragma unroll
            for (int k = 0; k < 3; ++k) stgx_<VOFF>(g_plo, k, S, ul, zero_row ? T(0) : plo[k]);
            stgx_<VOFF>(g_plo, 3, S, ul, zero_row ? T(0) : psi_lo);
        }
        DOCKAUV_STAMP(5);   // nav + obs done
    };

    // ---------------- wave OB (groups of four or more waves): the thirteen observations that need no navigation error ----
    auto ob_tail_pre = [&]() {
        if (QUAD && ob_lane) {
            T so[12], nuco[3];
#pragma unroll
            for (int k = 0; k < 12; ++k) so[k] = lds_hx[k * EPG + ule];
#pragma unroll
            for (int k = 0; k < 3; ++k) nuco[k] = NOCUR ? T(0) : lds_hx[(16 + k) * EPG + ule];
            if (SHARE_NAV) {
                obs_rest(so, nuco, lds_hx[19 * EPG + ule], lds_hx[20 * EPG + ule], false, ule, true);   // (sets ob_zero_row)
            } else {
                const bool col = EARLY ? col_from_records(ule) : (lds_hx[15 * EPG + ule] != T(0));
                const bool done = conditions(goal_dist(so, goal_o), so, t_steps_o, col) != 0;
                ob_zero_row = done && Q.reset_mode != 0;
                obs_rest(so, nuco, lds_hx[19 * EPG + ule], lds_hx[20 * EPG + ule], ob_zero_row, ule);
            }
        }
    };
    auto ob_tail_post = [&]() {   // behind the ray stage
        if (QUAD && RAYS && ob_lane) obs_ray_cells(ob_zero_row, ule);
    };

    // ---------------- bookkeeper (conditions, reward, counters) and resetter (state write-back, episode reset) -------
    // one wave each when the group has four, the same wave when it has two, wave 0 itself when it has one
    T bk_rw[kNRew], bk_part = T(0);
    int bk_cbits = 0;
    // state, V_c, action penalty, |euler_dot|^2, collision of the lane's env as a tail role sees them
    auto role_inputs = [&](T* sb, T& Vc_b, T& act_pen_b, T& edot_b, bool& col_b) {
        if (DUAL) {
#pragma unroll
            for (int k = 0; k < 12; ++k) sb[k] = lds_hx[k * EPG + ule];
            Vc_b = NOCUR ? T(0) : lds_hx[12 * EPG + ule];
            act_pen_b = lds_hx[13 * EPG + ule];
            edot_b = lds_hx[14 * EPG + ule];
            col_b = EARLY ? col_from_records(ule) : (lds_hx[15 * EPG + ule] != T(0));
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) sb[k] = st[k];
            Vc_b = Vc; act_pen_b = act_pen; edot_b = edot_norm2; col_b = collision;
        }
    };
    T bk_dd = T(0), bk_dth = T(0), bk_dpsi = T(0), bk_psi = T(0);
    auto bk_tail_pre = [&]() {
        if (!bk_lane) return;
        T sb[12], Vc_b, act_pen_b, edot_b;
        bool col_b;
        role_inputs(sb, Vc_b, act_pen_b, edot_b, col_b);
        T* rw = bk_rw;
        // (the terms that need no navigation error first: with SHARE_NAV this wave then waits for the integrating wave's)
        {
            const T a = sb[3] * (T(2) / pi_<T>()), b = sb[4] * (T(2) / pi_<T>());
            rw[3] = -Q.w_phi * (a * a);
            rw[4] = -Q.w_th * (b * b);
            const T e = sqrt_(edot_b) * Q.inv_vel[3];
            rw[5] = -Q.w_thdot * (e * e);
        }
        rw[6] = T(0);
        rw[7] = -act_pen_b;
        T dd, dth, dpsi;
        int cbits;
        if (SHARE_NAV) {
            wait_nav();
            dd = lds_nav[0 * EPG + ule]; dth = lds_nav[1 * EPG + ule]; dpsi = lds_nav[2 * EPG + ule];
            cbits = (int)lds_nav[3 * EPG + ule];
        } else {
            nav_errors(sb, goal_b, dd, dth, dpsi);
            cbits = conditions(dd, sb, t_steps_b, col_b);
        }
        bk_dd = dd; bk_dth = dth; bk_dpsi = dpsi; bk_psi = sb[5];
        bk_cbits = cbits;
        // ---------------- 12. reward (envs/docking3d.py:490-595, 706-792): every term but the obstacle avoidance ----
        const T eps = T(0.001);
        // log_precision (docking3d.py:711-723): log(max(x, eps) / x_max)
        const T log_dd_e = log_((dd > eps ? dd : eps) * Q.inv_dmax);
        const T lp_d = T(1) - clip_(log_dd_e * Q.inv_log_tol_eps, T(0), T(1));
        bk_part = lp_d;
        rw[0] = -Q.w_d * lp_d;
        const T half_pi = pi_<T>() / T(2);
        if (LOG && Q.reward_set == 2) {   // (product kernels: reward set 1, see launch_vk)
            // cont_goal_constraints with x_des = 0 -> max(x_goal, eps) = eps; exponents 4 (docking3d.py:523-548)
            const T ath = abs_(dth), aps = abs_(dpsi);
            const T l_th = T(1) - clip_(div_(log_((ath > eps ? ath : eps) / half_pi), log_(eps / half_pi)), T(0), T(1));
            const T l_ps = T(1) - clip_(div_(log_((aps > eps ? aps : eps) / pi_<T>()), log_(eps / pi_<T>())), T(0), T(1));
            const T ld2 = lp_d * lp_d, ld4 = ld2 * ld2;
            const T t2 = l_th * l_th, p2 = l_ps * l_ps;
            rw[1] = -Q.w_dth * (t2 * t2) * ld4;
            rw[2] = -Q.w_dpsi * (p2 * p2) * ld4;
        } else {
            const T a = dth * (T(2) / pi_<T>()), b = dpsi * (T(1) / pi_<T>());
            rw[1] = -Q.w_dth * (a * a);
            rw[2] = -Q.w_dpsi * (b * b);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) rw[8 + k] = (cbits >> k & 1) ? Q.w_done[k] : T(0);
    };
    auto bk_tail_post = [&]() {   // behind the ray stage: obstacle-avoidance term, the sum, outputs, counters
        if (!bk_lane) return;
        T* rw = bk_rw;
        const int cbits = bk_cbits;
        const bool done = cbits != 0;
        const bool reset_now = done && Q.reset_mode != 0;
        // Reward.obstacle_avoidance (docking3d.py:766-784) from the ray stage's partial sums
        T oa = T(0);
        if (RAYS) {
            T sum_beta = T(0), denom = T(0);
#pragma unroll
            for (int w = 0; w < (LOG ? NT / EPG : 1); ++w) {   // (lane = ray stage: slot 0 only; the other rows may hold lds_nav)
                if (REGREC_OK && regrec) {
                    sum_beta += E.sum_beta;
                    denom += oa_den_r;
                    continue;
                }
                sum_beta += lds_oa[(w * 2 + 0) * EPG + ule];
                denom += lds_oa[(w * 2 + 1) * EPG + ule];
            }
            oa = div_(sum_beta, denom) - T(1);
        }
        if (LOG && Q.reward_set == 2) {
            const T eps = T(0.001);
            const T aoa = abs_(oa);
            const T l_oa = T(1) - clip_(div_(log_(aoa > eps ? aoa : eps), log_(eps)), T(0), T(1));
            const T ld2 = bk_part * bk_part, ld4 = ld2 * ld2;
            const T o2 = l_oa * l_oa;
            rw[6] = -Q.w_oa * (o2 * o2) * ld4;
        } else {
            rw[6] = -Q.w_oa * oa;
        }
        T reward = T(0);
#pragma unroll
        for (int k = 0; k < kNRew; ++k) reward += rw[k];

        if (!RAYS && DUAL) DOCKAUV_STAMP_W1(11);   // bookkeeper: reward done
        // ---------------- outputs, counters ----------------
        if (IO.reward) stgx_<VOFF>(static_cast<T*>(IO.reward) + env0, 0, S, ule, reward);
        if (IO.done) stgx_<VOFF>(IO.done + env0, 0, S, ule, (uint8_t)(done ? 1 : 0));
        if (IO.pack) {
            float* ot = lds_obs + (size_t)ule * row_len;
            ot[Q.n_obs] = (float)reward;
            ot[Q.n_obs + 1] = done ? 1.0f : 0.0f;
        }
        if (IO.conditions) stgx_<VOFF>(IO.conditions + env0, 0, S, ule, (uint8_t)cbits);
        if (IO.reward_terms) {
            T* rt = static_cast<T*>(IO.reward_terms) + (size_t)env0 * kNRew + ule * (unsigned)kNRew;
#pragma unroll
            for (int k = 0; k < kNRew; ++k) rt[k] = rw[k];
        }
        if (TR) {
            const int slot = TR->slot_of_env[env0 + (int)ule];
            if (slot >= 0) {
                const size_t row = (size_t)(IO.trace_step % TR->capacity) * (size_t)TR->n_rows + (size_t)slot;
                T* rt = static_cast<T*>(TR->reward_terms) + row * kNRew;
#pragma unroll
                for (int k = 0; k < kNRew; ++k) rt[k] = rw[k];
                TR->cond[row] = (uint8_t)cbits;
            }
        }
        if (IO.nav) {
            T* nv = static_cast<T*>(IO.nav) + (size_t)env0 * 4 + ule * 4u;
            nv[0] = bk_dd; nv[1] = bk_dth; nv[2] = bk_dpsi; nv[3] = ssa_(goal_b[3] - bk_psi);   // delta_psi_goal: unused downstream
        }
        stgx_<VOFF>(g_cum, 0, S, ule, reset_now ? T(0) : cum_in + reward);
        stgx_<VOFF>(g_tsteps, 0, S, ule, reset_now ? 0 : t_steps_b + 1);
    };
    auto rs_tail = [&]() {
        if (!rs_lane) return;
        DOCKAUV_STAMP(7);
        T sb[12], Vc_b, act_pen_b, edot_b;
        bool col_b;
        role_inputs(sb, Vc_b, act_pen_b, edot_b, col_b);
        // (the resetter only needs the distance of the navigation errors; sharing a wave with the bookkeeper, its bits)
        bool done;
        if (SHARE_NAV) {
            wait_nav();
            done = lds_nav[3 * EPG + ule] != T(0);
        } else {
            done = (QUAD ? conditions(goal_dist(sb, goal_b), sb, t_steps_b, col_b) : bk_cbits) != 0;
        }
        const bool reset_now = done && Q.reset_mode != 0;
        // ---------------- in-kernel episode reset; state write-back of the envs this wave is responsible for ----------------
        if (reset_now) {
            const int ep_next = episode_in + 1;
            T curv[8];
            if (LOG && Q.reset_mode == 1) {   // from the host-staged pool (product kernels: none / in-kernel generation)
                const T* pp = static_cast<const T*>(B.p_pose);
                const T* pg = static_cast<const T*>(B.p_goal);
                const T* pc = static_cast<const T*>(B.p_cur);
#pragma unroll
                for (int k = 0; k < 6; ++k) sb[k] = ldgx_<VOFF>(pp + env0, k, S, ule);
#pragma unroll
                for (int k = 0; k < 4; ++k) goal_b[k] = ldgx_<VOFF>(pg + env0, k, S, ule);
#pragma unroll
                for (int k = 0; k < 8; ++k) curv[k] = ldgx_<VOFF>(pc + env0, k, S, ule);
                const T* pcap = static_cast<const T*>(B.p_caps);
                for (int k = 0; k < E.max_cap * 7; ++k) stgx_<VOFF>(g_caps, (size_t)k, S, ule, ldgx_<VOFF>(pcap + env0, (size_t)k, S, ule));
                const T* psp = static_cast<const T*>(B.p_sph);
                for (int k = 0; k < E.max_sph * 4; ++k) stgx_<VOFF>(g_sph, (size_t)k, S, ule, ldgx_<VOFF>(psp + env0, (size_t)k, S, ule));
            } else {                   // generated in-kernel (sphere fields are static per env and stay)
                T ring_s;
                if (DUAL) {
#pragma unroll
                    for (int k = 0; k < 6; ++k) sb[k] = lds_spec[k * EPG + ule];
#pragma unroll
                    for (int k = 0; k < 4; ++k) goal_b[k] = lds_spec[(6 + k) * EPG + ule];
#pragma unroll
                    for (int k = 0; k < 8; ++k) curv[k] = NOCUR ? T(0) : lds_spec[(10 + k) * EPG + ule];
                    ring_s = NOCAP ? T(0) : lds_spec[18 * EPG + ule];
                } else {
                    T Ub[12];
                    episode_uniforms_<T>(E, env0 + (int)ule, ep_next, Ub);
                    generate_episode_<T>(E, Ub, sb, goal_b, curv, ring_s);
                }
                if (!NOCAP) store_capsules_<T>(E, g_caps, S, ule, ring_s);   // (NOCAP: the handle has no capsule slot)
            }
#pragma unroll
            for (int k = 6; k < 12; ++k) sb[k] = T(0);
#pragma unroll
            for (int k = 0; k < kMaxU; ++k)
                if (k < n_u_max) stgx_<VOFF>(g_u, k, S, ule, T(0));
#pragma unroll
            for (int k = 0; k < 4; ++k) stgx_<VOFF>(g_goal, k, S, ule, goal_b[k]);
            if (!NOCUR) {   // (NOCUR: the rows hold the generator's zeros already)
#pragma unroll
                for (int k = 1; k < 8; ++k) stgx_<VOFF>(g_cur, k, S, ule, curv[k]);
            }
            Vc_b = curv[0];
            stgx_<VOFF>(g_episode, 0, S, ule, ep_next);
        }
        if (!DUAL || reset_now) {
#pragma unroll
            for (int k = 0; k < 12; ++k) stgx_<VOFF>(g_state, k, S, ule, sb[k]);
            if (!NOCUR) stgx_<VOFF>(g_cur, 0, S, ule, Vc_b);
        }
    };

    if (RAYS) {
        DOCKAUV_STAMP(14);   // env phase part 1 done
        // ---------------- complete the obstacle records for the new pose; body collision ----------------
        // wave 0 publishes the pose (position + body -> NED rotation); every wave of the group then completes the
        // records of the obstacles c = wave, wave + W, ... for all 64 envs (on wave 0 alone this took 3.4 k cycles
        // for 5 capsules and 6.3 k for 8 spheres)
        // (SOLO: the one wave completes the records of its own lanes' envs from its registers; the raw records it reads are
        // its own writes: LDS operations of a wave complete in order)
        if (owner && !SOLO) {
            T R1[9];
            rotmat_(g1, R1);
            lds_pose[2 * EPG + ul] = st[0];
            lds_pose[3 * EPG + ul] = st[1];
            lds_pose[4 * EPG + ul] = st[2];
#pragma unroll
            for (int k = 0; k < 9; ++k) lds_pose[(5 + k) * EPG + ul] = R1[k];
        }
        if (!SOLO) lds_barrier_<NT>();   // raw obstacle records, slot counts and the pose are in LDS
        if constexpr (TAIL) { WQ.n_obs = pin_sgpr_(WQ.n_obs); WQ.reset_mode = pin_sgpr_(WQ.reset_mode); }
        if (env0 + (int)ule < A.n_envs) {
            const T* P = lds_pose + ule;
            const int ncap = SOLO ? ncap_r : (int)P[0 * EPG], nsph = SOLO ? nsph_r : (int)P[1 * EPG];
            const T px0 = SOLO ? st[0] : P[2 * EPG], py0 = SOLO ? st[1] : P[3 * EPG], pz0 = SOLO ? st[2] : P[4 * EPG];
            T R1[9];   // body -> NED; its transpose takes vectors into the body frame
            if (SOLO) {
                rotmat_(g1, R1);
            } else {
#pragma unroll
                for (int k = 0; k < 9; ++k) R1[k] = P[(5 + k) * EPG];
            }
            bool col = false;
            // one capsule (regrec): the record for the new pose out of (c1, unit axis, |ba|, r); true = the fan may reach it
            auto complete_capsule = [&](T c1x, T c1y, T c1z, T dx, T dy, T dz, T len, T rad, T* o, bool& hits_body) -> bool {
                const T oax = px0 - c1x, oay = py0 - c1y, oaz = pz0 - c1z;
                const T oa_par = oax * dx + oay * dy + oaz * dz;
                const T px = oax - oa_par * dx, py = oay - oa_par * dy, pz = oaz - oa_par * dz;
                o[0] = R1[0] * dx + R1[3] * dy + R1[6] * dz;
                o[1] = R1[1] * dx + R1[4] * dy + R1[7] * dz;
                o[2] = R1[2] * dx + R1[5] * dy + R1[8] * dz;
                o[3] = R1[0] * px + R1[3] * py + R1[6] * pz;
                o[4] = R1[1] * px + R1[4] * py + R1[7] * pz;
                o[5] = R1[2] * px + R1[5] * py + R1[8] * pz;
                o[6] = oa_par;
                o[7] = len;
                o[8] = rad * rad;
                o[9] = oa_par - len;
                const bool may = capsule_may_be_hit_<T>(o[0], o[3], px * px + py * py + pz * pz, oa_par, len, rad, rc_ray_max(),
                                                        rc_fan_cos(), rc_fan_sin());
                // collision_capsule_sphere / dist_line_point (objects/shape.py:195-210, 393-417):
                // hypot(max(s, t, 0), |(p - l1) x d|) with s = (l1 - p).d = -oa_par, t = (p - l2).d = oa_par - |ba|
                // and |(p - l1) x d| = |oa_perp| for the unit axis d
                const T s_ = -oa_par, t_ = oa_par - len;
                T hh = s_ > t_ ? s_ : t_;
                hh = hh > T(0) ? hh : T(0);
                const T dist = sqrt_(hh * hh + (px * px + py * py + pz * pz));   // np.hypot
                hits_body = dist <= rad + rc_safety();
                return may;
            };
            if (REGREC_OK && regrec) {
#pragma unroll
                for (int c = 0; c < kRegCaps; ++c) {
                    if (c < E.max_cap) {   // (scalar; a lane's unused slots are computed and masked: no divergence)
                        const T* rp = lds_raw + (size_t)c * 7 * EPG + ule;
                        const T bax = rp[3 * EPG], bay = rp[4 * EPG], baz = rp[5 * EPG];
                        const T len = sqrt_(bax * bax + bay * bay + baz * baz);
                        const T inv_len = rcp_(len);
                        bool hb;
                        const bool may = complete_capsule(rp[0 * EPG], rp[1 * EPG], rp[2 * EPG], bax * inv_len, bay * inv_len, baz * inv_len,
                                                          len, rp[6 * EPG], rr[c], hb);
                        if (c < ncap && may) cmask_r |= 1u << c;
                        col = col || (c < ncap && hb);
                    }
                }
            }
            // (the records in LDS: the same arithmetic written out, in the order this loop has always had)
            for (int c = wv; c < ((REGREC_OK && regrec) ? 0 : ncap); c += W) {
                T* cp = lds_cap + (size_t)c * kCapFields * EPG + ule;
                const T c1x = cp[0 * EPG], c1y = cp[1 * EPG], c1z = cp[2 * EPG];
                const T dx = cp[3 * EPG], dy = cp[4 * EPG], dz = cp[5 * EPG];
                const T len = cp[6 * EPG], rad = cp[7 * EPG];
                const T oax = px0 - c1x, oay = py0 - c1y, oaz = pz0 - c1z;
                const T oa_par = oax * dx + oay * dy + oaz * dz;
                const T px = oax - oa_par * dx, py = oay - oa_par * dy, pz = oaz - oa_par * dz;
                cp[0 * EPG] = R1[0] * dx + R1[3] * dy + R1[6] * dz;
                cp[1 * EPG] = R1[1] * dx + R1[4] * dy + R1[7] * dz;
                cp[2 * EPG] = R1[2] * dx + R1[5] * dy + R1[8] * dz;
                cp[3 * EPG] = R1[0] * px + R1[3] * py + R1[6] * pz;
                cp[4 * EPG] = R1[1] * px + R1[4] * py + R1[7] * pz;
                cp[5 * EPG] = R1[2] * px + R1[5] * py + R1[8] * pz;
                cp[6 * EPG] = oa_par;
                cp[7 * EPG] = len;
                cp[8 * EPG] = rad * rad;
                cp[9 * EPG] = oa_par - len;
                if (capsule_may_be_hit_<T>(cp[0 * EPG], cp[3 * EPG], px * px + py * py + pz * pz, oa_par, len, rad, rc_ray_max(),
                                           rc_fan_cos(), rc_fan_sin())) {
                    if (SOLO) cmask_r |= 1u << c;
                    else atomicOr(reinterpret_cast<unsigned int*>(lds_pose + 14 * EPG + ule), 1u << c);
                }
                const T s_ = -oa_par, t_ = oa_par - len;
                T hh = s_ > t_ ? s_ : t_;
                hh = hh > T(0) ? hh : T(0);
                const T dist = sqrt_(hh * hh + (px * px + py * py + pz * pz));   // np.hypot
                col = col || (dist <= rad + rc_safety());
            }
            for (int s_i = wv; s_i < nsph; s_i += W) {
                T* sp = lds_sph + (size_t)s_i * kSphFields * EPG + ule;
                const T cx = sp[0 * EPG], cy = sp[1 * EPG], cz = sp[2 * EPG], rad = sp[3 * EPG];
                const T ocx = px0 - cx, ocy = py0 - cy, ocz = pz0 - cz;
                const T d2 = ocx * ocx + ocy * ocy + ocz * ocz;
                sp[0 * EPG] = R1[0] * ocx + R1[3] * ocy + R1[6] * ocz;
                sp[1 * EPG] = R1[1] * ocx + R1[4] * ocy + R1[7] * ocz;
                sp[2 * EPG] = R1[2] * ocx + R1[5] * ocy + R1[8] * ocz;
                sp[3 * EPG] = rad * rad;
                const T dist = sqrt_(d2);
                if (sphere_may_be_hit_<T>(sp[0 * EPG], d2, dist, rad, rc_ray_max(), rc_fan_cos(), rc_fan_sin())) {
                    if (SOLO) smask_r |= 1u << s_i;
                    else atomicOr(reinterpret_cast<unsigned int*>(lds_pose + 15 * EPG + ule), 1u << s_i);
                }
                // collision_sphere_spheres (objects/shape.py:182-192)
                col = col || (dist <= rc_safety() + rad);
            }
            if (SOLO) collision = col; else lds_col[wv * EPG + ule] = col ? T(1) : T(0);
            DOCKAUV_STAMP(15);   // obstacle records complete
        }
        if (REGREC_OK && regrec) {
            // the raw rows are dead (every lane of this one wave has read its own: LDS operations of a wave complete in order):
            // their bytes become the tile, whose ray cells start from zero
            const int n_red_z = E.n_red;
            float* orow = cell_row(ule, n_red_z);
            for (int k = 0; k < n_red_z; ++k) orow[k] = 0.0f;
        }
        if (EARLY && owner) {
            // the hand-over to the tail roles, in front of the barrier they start behind (its collision entry is not
            // known yet: the roles take that from the waves' flags, col_from_records)
            publish_hx();
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        }
    }

    if (RAYS) {
        lds_barrier_<NT>();
        if (owner) {
            if (!SOLO) {
#pragma unroll
                for (int w = 0; w < W; ++w) collision = collision || (lds_col[w * EPG + ul] != T(0));
            }
            if (DUAL && !EARLY) {
                publish_hx();
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            }
            if (EARLY) w0_tail();   // nothing of it waits for the rays
        }
        // (mixed groups: an integrating wave may own no lane at all -- a group of one vehicle kind -- and then never runs
        // its tail: its flag is raised here, by the wave, whatever its lanes did)
        if (SHARE_NAV && MIXED2 && wv < 2) raise_nav_flag_(wv);
        // ---------------- 4-6. ray stage: thread -> env e = tid % EPG, wave w -> reduced cells w, w + NT/EPG, ... ----
        // A wave shares the body-frame ray (scalar table loads); every lane owns one env, so the block-max of a cell
        // (sensor.py:131-137) and the obstacle-avoidance sums (docking3d.py:782-784) are taken on the fly and no
        // [rays][envs] distance matrix has to be staged.
        // the ray table is read with wave-uniform indices through the constant address space: scalar loads
        typedef const __attribute__((address_space(4))) T CT;
        CT* const rays = (CT*)(uintptr_t)B.rays;
        DOCKAUV_STAMP_W1(10);   // ray stage entered
        static_assert(EPG % 64 == 0, "a wave must not straddle two ray indices");
        if (SHARE_NAV && NT / EPG == 4 && !MIXED2 && wv == 0) {
            // (the integrating wave takes no ray pass and writes no constants here: it has done its tail above, the other
            // roles are waiting for what it published)
        } else if (!LOG || E.n_rays <= 64) {   // (product kernels: fans of 9..16 / 33..64 rays only, see launch_vk)
            // ---- lane = ray.  A wave takes 64 / ray_pad envs at a time (one for the default 63-ray fan): the body-frame
            // ray of a lane is a constant, obstacle records are read from LDS with the lane's env index (a broadcast
            // when the whole wave works on one env), and an obstacle whose may-be-hit flag is clear for every env
            // of the pass is skipped by the whole wave -- with lane = env that never happens, some env of 64 always
            // needs it.  Block maxima go to the observation tile through LDS atomics (values in [0, 1]: their bit
            // patterns order like the numbers, NaN on top, as np.max wants), the weighted sum over the rays of an env
            // is a butterfly over its lanes (fixed order: deterministic).
            const int pad = pin_sgpr_(RQ.pad), pad_log2 = pin_sgpr_(RQ.pad_log2), n_rays = pin_sgpr_(RQ.n_rays);
            const int n_red = pin_sgpr_(RQ.n_red), max_cap = pin_sgpr_(RQ.max_cap), max_sph = pin_sgpr_(RQ.max_sph);
            const T ray_max = pin_sgpr_(RQ.ray_max), inv_ray_max = pin_sgpr_(RQ.inv_ray_max), sum_beta_all = pin_sgpr_(RQ.sum_beta);
            const int lane = tid % 64;
            const int r = lane & (pad - 1), sub = lane >> pad_log2;
            const bool ray_ok = r < n_rays;
            const T bx = lr_bx, by = lr_by, bz = lr_bz, beta = lr_beta;
            const int cell = lr_cell;
            T* const ray_dist = IO.ray_dist ? static_cast<T*>(IO.ray_dist) + (size_t)env0 * n_rays : nullptr;
            const int epp = 64 >> pad_log2;                            // envs per pass
            const int wq = __builtin_amdgcn_readfirstlane(tid / 64);   // this wave's index (EPG = 64: same as tid / EPG)
            // what a ray contributes once its clamped distance is known (docking3d.py:436-439, 782-792); one function
            // for the general path and for the constants of an obstacle-free pass, so that both round alike
            auto ray_terms = [&](T d, T& pen_out, float& v01_out) {
                // Reward.c_oa = clip(1 - d / d_max, 0, 1) and the penalty (gamma_c (1 - c_oa))^2 with gamma_c = 1
                // (docking3d.py:786-792): 1 - clip(1 - x, 0, 1) IS clip(x, 0, 1) -- the observation cell's value -- for every x
                // incl. NaN; evaluated once (six instructions less per pass; the two roundings of 1 - (1 - x) are gone with it)
                const T x01 = clip_(d * inv_ray_max, T(0), T(1));
                const T pen = x01 * x01;
                pen_out = (pen > T(0.001) || isnan_(pen)) ? pen : T(0.001);   // np.maximum(.., epsilon_c)
                v01_out = (float)x01;
            };
            // An env none of whose obstacles is within reach of the fan: every ray reads ray_max, i.e. constants.  Such
            // envs (the large majority wherever vehicles roam a 20 m ball: 99 % in BASELINE config 3, ~85 % in configs
            // 4 / 5, scripts/active_fraction.py) take no ray pass at all: lane = env writes their constants, and the
            // passes run over the others only.  Every wave works that out for itself from the may-be-hit masks (lane =
            // env: a ballot), no barrier.
            // (every ray at ray_max: c_oa = 0, penalty 1, so both sums of Reward.obstacle_avoidance are the sum of the
            // weights and the term is exactly 0, docking3d.py:782-784; the cell value is clip(ray_max / ray_max) = 1)
            const float v01_free = (float)clip_(ray_max * inv_ray_max, T(0), T(1));
            const bool env_ok = env0 + lane < A.n_envs;
            // lane = env view of the group: may-be-hit masks and "has no capsule" (then the sphere group is group 0 of
            // update_radar_collision, docking3d.py:431-439)
            // (NOCAP: no capsule mask, and every env "has no capsule" -- rows 14 and 0 are not read)
            const unsigned cm_l = (NOCAP || !env_ok) ? 0u : (SOLO ? cmask_r : *reinterpret_cast<const unsigned int*>(lds_pose + 14 * EPG + lane));
            const unsigned sm_l = !env_ok ? 0u : (SOLO ? smask_r : *reinterpret_cast<const unsigned int*>(lds_pose + 15 * EPG + lane));
            const int nocap_l = NOCAP ? 1 : (((SOLO ? ncap_r : (int)lds_pose[0 * EPG + lane]) == 0) ? 1 : 0);
            const bool act = (cm_l | sm_l) != 0u;
            const unsigned long long ball = __ballot(act);
            const int n_act = __builtin_amdgcn_readfirstlane(__popcll(ball));
            // who writes those constants: every wave a share of the cells -- EARLY: the waves with the lightest tail
            // roles only (groups of four: OB and RS, or the two helpers of a mixed batch; of eight: the four role-less
            // waves), never the integrating waves
            constexpr int W_ = NT / 64;
            constexpr int NCW = EARLY ? (W_ >= 8 ? W_ - 4 : 2) : W_;
            const int cwi = !EARLY ? wq : (W_ >= 8 ? wq - 4 : ((MIXED2 || FREE_WAVE) ? wq - 2 : (wq == 1 ? 0 : (wq == 3 ? 1 : -1))));
            if (env_ok && !act && cwi >= 0) {
                float* orow = cell_row((unsigned)lane, n_red);
                for (int k = cwi; k < n_red; k += NCW) orow[k] = v01_free;
                if (REGREC_OK && regrec) {
                    oa_den_r = sum_beta_all;
                } else if (cwi == 0) {
                    lds_oa[(0 * 2 + 0) * EPG + lane] = sum_beta_all;
                    lds_oa[(0 * 2 + 1) * EPG + lane] = sum_beta_all;
                }
                if (ray_dist)
                    for (int k = cwi; k < n_rays; k += NCW) ray_dist[(unsigned)lane * (unsigned)n_rays + k] = ray_max;
            }
            DOCKAUV_STAMP_W1(22);   // constants of the obstacle-free envs written
            // The passes, specialised at compile time for the two fan widths of the BASELINE configs (PL = log2 of the
            // lanes per env: 6 = one env per pass, the default 63-ray fan; 4 = four envs per pass, the 16-beam fan) and
            // generic otherwise (PL = 0: lanes per env known at run time only).  In the specialised forms the envs of
            // a pass are scalars taken from the ballot (s_ff1), their masks come out of the lane = env registers by
            // v_readlane, and the sum over an env's rays is all DPP: no LDS round trip in front of the first record.
            auto run_passes = [&](auto PLc) {
                constexpr int PL = decltype(PLc)::value;
                constexpr int EPP = PL ? (64 >> PL) : 0;                 // envs per pass (compile time) or 0
                const int epp_rt = PL ? EPP : epp;
                // Pass p belongs to the wave of rank p % W.  Ranks: the waves without a tail role first (groups of eight),
                // then OB, RS, BK -- lightest role first --, the integrating waves last: with a handful of active envs per
                // group (config 3: one at most, as a rule) those get no pass at all.  (Not EARLY: W - 1 - wave.)
                const int wr = (EARLY && wq < 4) ? (NT / 64 - 4) + (int)(((MIXED2 ? kMixedRanks : (FREE_WAVE ? 0x1023u : 0x2013u)) >> (4 * wq)) & 3u)
                                                 : NT / 64 - 1 - wq;
                int* const act_list = reinterpret_cast<int*>(lds_act + (size_t)wq * EPG);
                unsigned long long rem = ball;   // regrec: the list is the ballot itself
                if (wr * epp_rt < n_act && !(REGREC_OK && regrec)) {   // (a wave without a pass needs no list)
                    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ball >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ball, 0u));
                    if (act) act_list[rank] = lane;   // (own writes: LDS operations of a wave complete in order)
                }
                for (int p0 = wr * epp_rt; p0 < n_act; p0 += (NT / 64 - ((SHARE_NAV && NT / EPG == 4 && !MIXED2) ? 1 : 0)) * epp_rt) {
                    // ---- the envs of this pass: e (per lane), their masks, the union of the masks over the pass
                    int e;
                    bool live;
                    unsigned cmask, smask, wc, ws;
                    bool nocap;
                    if constexpr (PL == 6) {
                        int e0;
                        if (REGREC_OK && regrec) {
                            e0 = __builtin_ctzll(rem);
                            rem &= rem - 1;
                        } else {
                            e0 = __builtin_amdgcn_readfirstlane(act_list[p0]);   // one env per pass: a scalar
                        }
                        e = e0;
                        live = ray_ok;
                        wc = NOCAP ? 0u : (unsigned)__builtin_amdgcn_readlane((int)cm_l, e0);
                        ws = (unsigned)__builtin_amdgcn_readlane((int)sm_l, e0);
                        nocap = NOCAP || __builtin_amdgcn_readlane(nocap_l, e0) != 0;
                        cmask = wc;
                        smask = ws;
                    } else if constexpr (PL == 4) {
                        // four envs per pass: the env of a lane's 16-lane row comes from the wave's list, its masks from
                        // the lane = env registers through the LDS crossbar (ds_bpermute: no memory access), the union
                        // from the first lane of each row -- straight-line code (a scalar walk over the ballot compiled
                        // to a tree of exec-mask branches per selected value here)
                        const bool slot = p0 + sub < n_act;
                        e = act_list[slot ? p0 + sub : n_act - 1];
                        live = ray_ok && slot;
                        // (all 64 lanes take part in the three exchanges: a lane's source lane may sit in a row whose
                        // own slot is empty)
                        const unsigned cm_e = NOCAP ? 0u : (unsigned)__shfl((int)cm_l, e, 64), sm_e = (unsigned)__shfl((int)sm_l, e, 64);
                        nocap = NOCAP || __shfl(nocap_l, e, 64) != 0;
                        cmask = live ? cm_e : 0u;
                        smask = live ? sm_e : 0u;
                        wc = NOCAP ? 0u
                                   : ((unsigned)__builtin_amdgcn_readlane((int)cmask, 0) | (unsigned)__builtin_amdgcn_readlane((int)cmask, 16) |
                                      (unsigned)__builtin_amdgcn_readlane((int)cmask, 32) | (unsigned)__builtin_amdgcn_readlane((int)cmask, 48));
                        ws = (unsigned)__builtin_amdgcn_readlane((int)smask, 0) | (unsigned)__builtin_amdgcn_readlane((int)smask, 16) |
                             (unsigned)__builtin_amdgcn_readlane((int)smask, 32) | (unsigned)__builtin_amdgcn_readlane((int)smask, 48);
                    } else {
                        const bool slot = p0 + sub < n_act;
                        e = act_list[slot ? p0 + sub : n_act - 1];
                        live = ray_ok && slot;
                        cmask = (live && !NOCAP) ? *reinterpret_cast<const unsigned int*>(lds_pose + 14 * EPG + e) : 0u;
                        smask = live ? *reinterpret_cast<const unsigned int*>(lds_pose + 15 * EPG + e) : 0u;
                        nocap = NOCAP || (int)lds_pose[0 * EPG + e] == 0;
                        wc = 0;
                        ws = 0;
                        if (epp <= 8) {   // a few envs per wave: the first lane of each carries its masks
                            for (int k = 0; k < epp; ++k) {
                                wc |= (unsigned)__builtin_amdgcn_readlane((int)cmask, k * pad);
                                ws |= (unsigned)__builtin_amdgcn_readlane((int)smask, k * pad);
                            }
                        } else {
                            for (int c = 0; c < max_cap; ++c) wc |= __any((cmask >> c) & 1u) ? (1u << c) : 0u;
                            for (int c = 0; c < max_sph; ++c) ws |= __any((smask >> c) & 1u) ? (1u << c) : 0u;
                        }
                    }
                    const int ec = e;
                    // ---- update_radar_collision (docking3d.py:415-442): per ray the smallest positive distance over
                    // the obstacle groups (each capsule, then all spheres), else the value of group 0
                    T best = inf_<T>(), first = -inf_<T>();   // a skipped group 0 counts as a miss
                    // (one record at a time: requesting the next record ahead of the test -- round 2 -- made the compiler keep two
                    // register sets and copy one into the other, 20 v_mov per capsule in a loop that runs at the SIMD's issue
                    // limit when the fan is busy; other waves hide the LDS round trip.  Same-box A/B, round 4: config 4
                    // 9.54 -> 9.20 us, config 5 15.71 -> 15.38, ray-dense config 4 17.75 -> 16.3)
                    if constexpr (REGREC_OK && PL == 6) {
                        if (regrec) {
                            const int e0 = __builtin_amdgcn_readfirstlane(ec);
                            auto rl = [&](T x) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, (float)x), e0)); };
#pragma unroll
                            for (int c = 0; c < kRegCaps; ++c) {
                                if ((wc >> c) & 1u) {
                                    CapRec<T> rec;
                                    rec.dx = rl(rr[c][0]); rec.dy = rl(rr[c][1]); rec.dz = rl(rr[c][2]);
                                    rec.px = rl(rr[c][3]); rec.py = rl(rr[c][4]); rec.pz = rl(rr[c][5]);
                                    rec.oa_par = rl(rr[c][6]); rec.len = rl(rr[c][7]); rec.r2 = rl(rr[c][8]); rec.oa_top = rl(rr[c][9]);
                                    const T v = ray_capsule_<T>(rec, bx, by, bz);
                                    first = (c == 0) ? v : first;
                                    best = (v > T(0) && v < best) ? v : best;
                                }
                            }
                            wc = 0;
                        }
                    }
                    while (wc) {
                        const int cc = __builtin_ctz(wc);
                        wc &= wc - 1;
                        const CapRec<T> rec = load_cap_<T>(lds_cap + (size_t)cc * kCapFields * EPG + ec, EPG);
                        const T v = ray_capsule_<T>(rec, bx, by, bz);
                        if (PL == 6 || ((cmask >> cc) & 1u)) {
                            first = (cc == 0) ? v : first;
                            best = (v > T(0) && v < best) ? v : best;
                        }
                    }
                    if (ws) {
                        T sbest = inf_<T>(), sfirst = -inf_<T>();
                        while (ws) {
                            const int s_i = __builtin_ctz(ws);
                            ws &= ws - 1;
                            const T* sp = lds_sph + (size_t)s_i * kSphFields * EPG + ec;
                            const T v = ray_sphere_<T>(sp[0 * EPG], sp[1 * EPG], sp[2 * EPG], sp[3 * EPG], bx, by, bz);
                            if (PL == 6 || ((smask >> s_i) & 1u)) {
                                sfirst = (s_i == 0) ? v : sfirst;
                                sbest = (v > T(0) && v < sbest) ? v : sbest;
                            }
                        }
                        const T v = (sbest < inf_<T>()) ? sbest : sfirst;
                        if (smask != 0u) {   // (an env of the pass without a sphere in reach: its sphere group is a miss)
                            first = nocap ? v : first;
                            best = (v > T(0) && v < best) ? v : best;
                        }
                    }
                    T d = (best < inf_<T>()) ? best : first;
                    d = (d < T(0) || d > ray_max) ? ray_max : d;        // sensor.py:117 (NaN survives)
                    T pen;
                    float v01;
                    ray_terms(d, pen, v01);
                    // sum over the env's lanes (fixed order: deterministic)
                    T part = live ? pen * beta : T(0);
                    bool writer;
                    if constexpr (PL == 6 && sizeof(T) == 4) {
                        part = wave_sum_to_last_(part);
                        writer = lane == 63;
                    } else {
                        part = group_sum_(part, PL ? (1 << PL) : pad);
                        writer = r == 0;
                    }
                    if (live) {
                        atomicMax(reinterpret_cast<unsigned int*>(cell_row((unsigned)e, n_red) + cell), __float_as_uint(v01));
                        if (ray_dist) ray_dist[(unsigned)e * (unsigned)n_rays + r] = d;
                    }
                    if constexpr (REGREC_OK && PL == 6) {
                        if (regrec) {   // lane 63 has the sum: to the env's lane
                            const int e0 = __builtin_amdgcn_readfirstlane(ec);
                            const int ps = __builtin_amdgcn_readlane(__builtin_bit_cast(int, (float)part), 63);
                            oa_den_r = (lane == e0) ? (T)__builtin_bit_cast(float, ps) : oa_den_r;
                            writer = false;
                        }
                    }
                    if (writer && (PL == 6 || live)) {
                        lds_oa[(0 * 2 + 0) * EPG + e] = sum_beta_all;
                        lds_oa[(0 * 2 + 1) * EPG + e] = part;
                    }

                }
            };
            if (pad_log2 == 6) run_passes(IntC<6>{});
            else if (!LOG || pad_log2 == 4) run_passes(IntC<4>{});
            else run_passes(IntC<0>{});
            DOCKAUV_STAMP_W1(23);   // passes done
        } else {
            static_assert(EPG % 64 == 0, "a wave must not straddle two ray indices");
            const int e = tid % EPG;
            const int w = __builtin_amdgcn_readfirstlane(tid / EPG);   // wave-uniform: cells, rays and their validity are scalar
            const int env_e = env0 + e;
            T sum_beta = T(0), denom = T(0);
            if (env_e < A.n_envs) {
                const int ncap = (int)lds_pose[0 * EPG + e], nsph = (int)lds_pose[1 * EPG + e];
                const bool any_obstacle = (ncap + nsph) > 0;
                float* ot_e = lds_obs + (size_t)e * row_len;
                // loop-invariant scalars, pinned (see pin_sgpr_)
                const int blk = pin_sgpr_(E.blk), n_v = pin_sgpr_(E.n_v), n_h = pin_sgpr_(E.n_h), n_hr = pin_sgpr_(E.n_hr);
                const int n_red = pin_sgpr_(E.n_red), n_rays = pin_sgpr_(E.n_rays);
                const T ray_max = pin_sgpr_(E.ray_max), inv_ray_max = pin_sgpr_(E.inv_ray_max);
                T* const ray_dist = IO.ray_dist ? static_cast<T*>(IO.ray_dist) + (size_t)env0 * n_rays : nullptr;
                const int blk2 = blk * blk;
                constexpr int RC = sizeof(T) == 8 ? 1 : 4;   // rays tested per obstacle record (f64: register budget)
                for (int cell = w; cell < n_red; cell += NT / EPG) {
                    const int cv = cell / n_hr, ch = cell - cv * n_hr;
                    T cellmax = T(0);   // zero padding (skimage block_reduce cval = 0)
                    for (int q0 = 0; q0 < blk2; q0 += RC) {
                        // ---- up to RC rays of this cell; everything about them is wave-uniform
                        T bx[RC], by[RC], bz[RC], beta[RC];
                        bool valid[RC];
                        int rid[RC];
    #pragma unroll
                        for (int k = 0; k < RC; ++k) {
                            const int q = q0 + k;
                            const int dv = q / blk, dh = q - dv * blk;
                            const int iv = cv * blk + dv, ih = ch * blk + dh;
                            valid[k] = (q < blk2) && (iv < n_v) && (ih < n_h);
                            rid[k] = valid[k] ? (iv * n_h + ih) : 0;
                            bx[k] = rays[rid[k] * 4 + 0]; by[k] = rays[rid[k] * 4 + 1]; bz[k] = rays[rid[k] * 4 + 2];
                            beta[k] = rays[rid[k] * 4 + 3];
                        }
                        // ---- update_radar_collision, envs/docking3d.py:415-442: per ray the smallest positive distance
                        // over the obstacle groups (each capsule, then all spheres), else the value of group 0
                        T best[RC], first[RC];
    #pragma unroll
                        for (int k = 0; k < RC; ++k) { best[k] = inf_<T>(); first[k] = T(0); }
                        for (int c = 0; c < ncap; ++c) {
                            const CapRec<T> rec = load_cap_<T>(lds_cap + (size_t)c * kCapFields * EPG + e, EPG);
    #pragma unroll
                            for (int k = 0; k < RC; ++k) {
                                if (valid[k]) {   // wave-uniform
                                    const T v = ray_capsule_<T>(rec, bx[k], by[k], bz[k]);
                                    first[k] = (c == 0) ? v : first[k];
                                    best[k] = (v > T(0) && v < best[k]) ? v : best[k];
                                }
                            }
                        }
                        if (nsph > 0) {
                            T sbest[RC], sfirst[RC];
    #pragma unroll
                            for (int k = 0; k < RC; ++k) { sbest[k] = inf_<T>(); sfirst[k] = T(0); }
                            for (int sidx = 0; sidx < nsph; ++sidx) {
                                const T* sp = lds_sph + (size_t)sidx * kSphFields * EPG + e;
                                const T ox = sp[0 * EPG], oy = sp[1 * EPG], oz = sp[2 * EPG], r2 = sp[3 * EPG];
    #pragma unroll
                                for (int k = 0; k < RC; ++k) {
                                    if (valid[k]) {
                                        const T v = ray_sphere_<T>(ox, oy, oz, r2, bx[k], by[k], bz[k]);
                                        sfirst[k] = (sidx == 0) ? v : sfirst[k];
                                        sbest[k] = (v > T(0) && v < sbest[k]) ? v : sbest[k];
                                    }
                                }
                            }
    #pragma unroll
                            for (int k = 0; k < RC; ++k) {
                                const T v = (sbest[k] < inf_<T>()) ? sbest[k] : sfirst[k];
                                first[k] = (ncap == 0) ? v : first[k];
                                best[k] = (v > T(0) && v < best[k]) ? v : best[k];
                            }
                        }
    #pragma unroll
                        for (int k = 0; k < RC; ++k) {
                            if (valid[k]) {
                                T d = (best[k] < inf_<T>()) ? best[k] : first[k];
                                d = (d < T(0) || d > ray_max) ? ray_max : d;       // sensor.py:117 (NaN survives)
                                d = any_obstacle ? d : ray_max;                      // no obstacle at all (sensor.py:110-111)
                                cellmax = nanmax_(d, cellmax);
                                const T cc = clip_(T(1) - d * inv_ray_max, T(0), T(1));   // Reward.c_oa, docking3d.py:790-792
                                const T one_c = T(1) - cc;                                   // gamma_c = 1
                                T pen = one_c * one_c;
                                pen = (pen > T(0.001) || isnan_(pen)) ? pen : T(0.001);      // np.maximum(.., epsilon_c)
                                sum_beta += beta[k];
                                denom += pen * beta[k];
                                if (ray_dist) ray_dist[(unsigned)e * (unsigned)n_rays + rid[k]] = d;
                            }
                        }
                    }
                    ot_e[16 + cell] = (float)clip_(cellmax * inv_ray_max, T(0), T(1));
                    if (cell == w) DOCKAUV_STAMP_W1(11);   // first cell done
                }
                DOCKAUV_STAMP_W1(12);   // all cells done
            }
            lds_oa[(w * 2 + 0) * EPG + e] = sum_beta;
            lds_oa[(w * 2 + 1) * EPG + e] = denom;

        }
        if (EARLY) {   // the tail roles, behind each wave's own passes
            ob_tail_pre();
            bk_tail_pre();
            rs_tail();
        }
        DOCKAUV_STAMP_WAVES(24);   // each wave: arrival at the barrier behind the ray stage
        lds_barrier_<NT>();
        DOCKAUV_STAMP_W1(13);   // second barrier passed
    }

    if (!EARLY) {
        if (owner) w0_tail();
        ob_tail_pre();
        ob_tail_post();
        if (!RAYS && DUAL) DOCKAUV_STAMP_W1(10);   // hand-over received
        bk_tail_pre();
        bk_tail_post();
        rs_tail();
        if (!RAYS && DUAL) DOCKAUV_STAMP_W1(12);   // tail waves done
    } else {
        // what is left of the tail behind the ray stage: a finished env's ray cells, the obstacle-avoidance term
        ob_tail_post();
        bk_tail_post();
    }

    DOCKAUV_STAMP(8);   // reset + write-back issued
    // ---------------- coalesced row-major observation store ----------------
    lds_barrier_<NT>();
    if (TERM) {
        // terminal observations: the finished envs are read off the packed `done` column of the tile (lane = env), their
        // rows go to terminal_obs [n_envs][n_obs] (written only where done) and are zeroed in the tile; one wave, a few
        // rows per step
        if (tid < 64) {
            const int n_obs_ = WQ.n_obs;   // (whole wave: see WQ)
            const bool dn = (tid < n_valid) && (lds_obs[(size_t)tid * row_len + n_obs_ + 1] != 0.0f) && WQ.reset_mode != 0;
            unsigned long long m = __ballot(dn);
            float* const to0 = term_out + (size_t)env0 * n_obs_;
            while (m) {
                const int e = __builtin_ctzll(m);
                m &= m - 1;
                for (int k = tid; k < n_obs_; k += 64) {
                    float* cell = lds_obs + (size_t)e * row_len + k;
                    store_global_<VOFF>((__attribute__((address_space(1))) float*)(to0 + (size_t)e * n_obs_ + k), *cell);
                    *cell = 0.0f;
                }
            }
        }
        lds_barrier_<NT>();
    }
    if (IO.pack == 2) {
        // packed rows for a half-precision gather (one learner over several GPUs: the rows cross xGMI every step and the
        // links, not the kernels, set the pace -- DESIGN.md section 7): observation columns as bfloat16, round to nearest
        // even, two per word; reward and done stay float32.  Word idx of the group's rows -> (row, word) by mul_hi.
        const int n_obs_ = WQ.n_obs, npair = (n_obs_ + 1) >> 1, wpr = pin_sgpr_(E.bf16_wpr);
        const unsigned magic = pin_sgpr_(E.bf16_magic);
        const int totalw = n_valid * wpr;
        unsigned* const dstw = reinterpret_cast<unsigned*>(IO.obs) + (size_t)env0 * wpr;
        auto bf16_rne = [](float x) -> unsigned {
            const unsigned u = __float_as_uint(x);
            const unsigned r = (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
            return (x != x) ? ((u >> 16) | 0x40u) : r;   // (NaN stays a quiet NaN)
        };
        for (int idx = tid; idx < totalw; idx += NT) {
            const int e = (int)__umulhi((unsigned)idx, magic);
            const int w = idx - e * wpr;
            const float* row = lds_obs + (size_t)e * row_len;
            unsigned word;
            if (w < npair) {
                const unsigned lo = bf16_rne(row[2 * w]);
                const unsigned hi = (2 * w + 1 < n_obs_) ? bf16_rne(row[2 * w + 1]) : 0u;
                word = lo | (hi << 16);
            } else {
                word = __float_as_uint(row[n_obs_ + (w - npair)]);
            }
            store_global_<VOFF>((__attribute__((address_space(1))) unsigned*)(dstw + idx), word);
        }
    } else {
        const int total = n_valid * row_len;
        float* dst = IO.obs + (size_t)env0 * row_len;
        // EPG * row_len * 4 B is a multiple of 16 B and the tile starts 16-B aligned in LDS, so the bulk goes out
        // as 16-B stores when the destination is 16-B aligned too (it is for the buffers a learner allocates)
        if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
            const int total4 = total >> 2;
            const float4* src4 = reinterpret_cast<const float4*>(lds_obs);
            // (wave-uniform base in an SGPR pair; uniform_ widens the two halves as UNSIGNED words -- readfirstlane returns an
            // int, and a low word with bit 31 set must not sign-extend into the high word)
            float* const dstu = (float*)uniform_(dst);
            // whole sweeps of NT float4 need no per-lane predicate; four of them are in flight at a time
            const int nfull = total4 / NT;
            int j = 0;
            for (; j + 4 <= nfull; j += 4) {
                const float4 a = src4[(j + 0) * NT + tid], b = src4[(j + 1) * NT + tid];
                const float4 c = src4[(j + 2) * NT + tid], d = src4[(j + 3) * NT + tid];
                store_tile16_<VOFF>(dstu, (unsigned)((j + 0) * NT + tid) * 16u, a);
                store_tile16_<VOFF>(dstu, (unsigned)((j + 1) * NT + tid) * 16u, b);
                store_tile16_<VOFF>(dstu, (unsigned)((j + 2) * NT + tid) * 16u, c);
                store_tile16_<VOFF>(dstu, (unsigned)((j + 3) * NT + tid) * 16u, d);
            }
            {
                // what is left -- up to three whole sweeps and the partial one: all reads first, then the stores (one LDS
                // round trip instead of one per sweep; groups of 256 threads have 2-3 sweeps in all)
                const int rem = nfull - j;   // wave-uniform
                const bool tailp = nfull * NT + tid < total4;
                float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0, r3 = r0;
                if (rem > 0) r0 = src4[(j + 0) * NT + tid];
                if (rem > 1) r1 = src4[(j + 1) * NT + tid];
                if (rem > 2) r2 = src4[(j + 2) * NT + tid];
                if (tailp) r3 = src4[nfull * NT + tid];
                if (rem > 0) store_tile16_<VOFF>(dstu, (unsigned)((j + 0) * NT + tid) * 16u, r0);
                if (rem > 1) store_tile16_<VOFF>(dstu, (unsigned)((j + 1) * NT + tid) * 16u, r1);
                if (rem > 2) store_tile16_<VOFF>(dstu, (unsigned)((j + 2) * NT + tid) * 16u, r2);
                if (tailp) store_tile16_<VOFF>(dstu, (unsigned)(nfull * NT + tid) * 16u, r3);
            }
            for (int idx = (total4 << 2) + tid; idx < total; idx += NT)
                store_global_<VOFF>((__attribute__((address_space(1))) float*)(dst + idx), lds_obs[idx]);
        } else {
            for (int idx = tid; idx < total; idx += NT)
                store_global_<VOFF>((__attribute__((address_space(1))) float*)(dst + idx), lds_obs[idx]);
        }
    }
    DOCKAUV_STAMP(9);
    DOCKAUV_SPAN(2);
}

template <typename T, int VK, bool SYM, bool RAYS, int EPG, int NT, bool LOG = false, bool TERM = false, bool WB = false>
__global__ __launch_bounds__(NT, (min_waves_<T, NT>())) void step_kernel(const DevArgs A) {
    step_body<T, VK, SYM, RAYS, EPG, NT, LOG, TERM, WB>(A);
}

// The lean twins for handles without a water current (NOCUR, see step_body; select_step picks them): the plain kernel and its
// TERM form.  Kernels of their own names, so that every other instantiation keeps its symbol and its code.
template <typename T, int VK, bool SYM, bool RAYS, int EPG, int NT, bool TERM = false>
__global__ __launch_bounds__(NT, (min_waves_<T, NT>())) void step_nocur_kernel(const DevArgs A) {
    step_body<T, VK, SYM, RAYS, EPG, NT, false, TERM, false, 0, true>(A);
}

// The sphere-only twins of the lean ray kernel (NOCAP on top of NOCUR, see step_body): plain and TERM.
template <typename T, int VK, bool SYM, bool RAYS, int EPG, int NT, bool TERM = false>
__global__ __launch_bounds__(NT, (min_waves_<T, NT>())) void step_nocap_kernel(const DevArgs A) {
    step_body<T, VK, SYM, RAYS, EPG, NT, false, TERM, false, 0, true, true>(A);
}

// The step kernel with copy groups behind the step groups (dockauv_ride.h): the previous step's rows travel to the
// peers while this step is integrated.
template <typename T, int VK, bool SYM, bool RAYS, int EPG, int NT>
__global__ __launch_bounds__(NT, (min_waves_<T, NT>())) void step_ride_kernel(const DevArgs A, const RideArgs R) {
    const unsigned groups = (unsigned)((A.n_envs + EPG - 1) / EPG);
    if (blockIdx.x >= groups) {
        extern __shared__ __align__(16) unsigned char smem_raw[];
        ride_body<NT>(R, blockIdx.x - groups, gridDim.x - groups, reinterpret_cast<uint32_t*>(smem_raw));
        return;
    }
    step_body<T, VK, SYM, RAYS, EPG, NT, false, false, false, 1>(A);
}
// (its lean twin)
template <typename T, int VK, bool SYM, bool RAYS, int EPG, int NT>
__global__ __launch_bounds__(NT, (min_waves_<T, NT>())) void step_ride_nocur_kernel(const DevArgs A, const RideArgs R) {
    const unsigned groups = (unsigned)((A.n_envs + EPG - 1) / EPG);
    if (blockIdx.x >= groups) {
        extern __shared__ __align__(16) unsigned char smem_raw[];
        ride_body<NT>(R, blockIdx.x - groups, gridDim.x - groups, reinterpret_cast<uint32_t*>(smem_raw));
        return;
    }
    step_body<T, VK, SYM, RAYS, EPG, NT, false, false, false, 1, true>(A);
}
// (its sphere-only twin)
template <typename T, int VK, bool SYM, bool RAYS, int EPG, int NT>
__global__ __launch_bounds__(NT, (min_waves_<T, NT>())) void step_ride_nocap_kernel(const DevArgs A, const RideArgs R) {
    const unsigned groups = (unsigned)((A.n_envs + EPG - 1) / EPG);
    if (blockIdx.x >= groups) {
        extern __shared__ __align__(16) unsigned char smem_raw[];
        ride_body<NT>(R, blockIdx.x - groups, gridDim.x - groups, reinterpret_cast<uint32_t*>(smem_raw));
        return;
    }
    step_body<T, VK, SYM, RAYS, EPG, NT, false, false, false, 1, true, true>(A);
}

// The RESIDENT step sequence (round 4; dockauv_step_sequence's fast path for open-loop action sequences: the scripted /
// manual loops of train.py:108-117, 238, frame skip, replay).  Envs are independent, so a group can walk ITS 64 envs
// through all n steps of the call without ever meeting another group: no launch boundary between the steps -- no dispatch
// ramp, no late XCD, no end-of-kernel write-back wait (1.3-1.9 us of every 8-16 us launch, DESIGN.md section 3; config 2 at
// 4 096 envs sits on the floor of an empty dispatch).  Step k reads its actions from Q.actions[k] and writes its rows to
// Q.obs[k], exactly the bytes n single launches would have written: the body IS the single launch's body.  The env state
// goes through memory between the steps as it does between launches; what orders it is the group itself: every wave's
// stores have been performed (they are written through to L2; vmcnt(0)), the group meets at a barrier, and the vector L1 is
// invalidated before the next step's loads.
// One copy of the body inside a loop: left to itself the optimiser hoists everything that does not change from step to step
// out of the loop -- kernarg and parameter-block loads, ~40 per-lane row offsets, address arithmetic -- and keeps it alive
// through the whole body: 128 VGPRs plus 140-300 bytes of scratch per lane where the single launch needs 104-127 and none.
// The kernarg pointer and the thread / group indices are therefore made opaque at the top of every step (empty asm), so
// that each step is compiled like a launch of its own: same loads, same live ranges, same registers.
template <typename T, int VK, bool SYM, bool RAYS, int EPG, int NT, bool WB>
__global__ __launch_bounds__(NT, (min_waves_<T, NT>())) void step_seq_kernel(const DevArgs, const SeqArgs) {
    struct KernArgs { DevArgs A; SeqArgs Q; };   // (the kernarg segment: both arguments by value, 8-byte aligned)
    static_assert(alignof(DevArgs) == 8 && alignof(SeqArgs) == 8 && sizeof(DevArgs) % 8 == 0, "kernarg layout");
    typedef const __attribute__((address_space(4))) KernArgs CKA;
    CKA* ka = (CKA*)__builtin_amdgcn_kernarg_segment_ptr();
    unsigned tix = threadIdx.x, bix = blockIdx.x;
    const int n = ka->Q.n;
    for (int k = 0; k < n; ++k) {
        asm volatile("" : "+s"(ka));
        asm volatile("" : "+v"(tix));
        asm volatile("" : "+s"(bix));
        // (word by word through the constant address space: scalar loads, like the arguments of a launch of its own)
        union { DevArgs a; unsigned long long w[sizeof(DevArgs) / 8]; } Ak;
        typedef const __attribute__((address_space(4))) unsigned long long CW8;
        CW8* const src = (CW8*)ka;
#pragma unroll
        for (unsigned i = 0; i < sizeof(DevArgs) / 8; ++i) Ak.w[i] = src[i];
        Ak.a.io.actions = ka->Q.actions[k];
        Ak.a.io.obs = ka->Q.obs[k];
        step_body<T, VK, SYM, RAYS, EPG, NT, false, false, WB, 2>(Ak.a, tix, bix);
        if (k + 1 < n) {
            // What orders step k + 1 behind step k is the group itself (memory model: workgroup scope; all its waves share one
            // CU and one vector L1): every wave's stores have been performed, the group meets, and the L1 -- only the L1:
            // `buffer_inv sc0`; an agent-scope acquire (`sc1`) also invalidates L2 lines on this multi-XCD part and cost
            // 20+ us per step, measured -- drops whatever it may still hold of the rows the group has just rewritten.
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (NT > 64) __builtin_amdgcn_s_barrier();
            asm volatile("buffer_inv sc0" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
    }
}
// Its lean twin for handles without a water current (NOCUR, see step_body; select_sequence picks it): the same loop around the
// lean body -- a copy, not a shared function, so that step_seq_kernel keeps the code it has.
template <typename T, int VK, bool SYM, bool RAYS, int EPG, int NT, bool WB>
__global__ __launch_bounds__(NT, (min_waves_<T, NT>())) void step_seq_nocur_kernel(const DevArgs, const SeqArgs) {
    struct KernArgs { DevArgs A; SeqArgs Q; };   // (the kernarg segment: both arguments by value, 8-byte aligned)
    static_assert(alignof(DevArgs) == 8 && alignof(SeqArgs) == 8 && sizeof(DevArgs) % 8 == 0, "kernarg layout");
    typedef const __attribute__((address_space(4))) KernArgs CKA;
    CKA* ka = (CKA*)__builtin_amdgcn_kernarg_segment_ptr();
    unsigned tix = threadIdx.x, bix = blockIdx.x;
    const int n = ka->Q.n;
    for (int k = 0; k < n; ++k) {
        asm volatile("" : "+s"(ka));
        asm volatile("" : "+v"(tix));
        asm volatile("" : "+s"(bix));
        union { DevArgs a; unsigned long long w[sizeof(DevArgs) / 8]; } Ak;
        typedef const __attribute__((address_space(4))) unsigned long long CW8;
        CW8* const src = (CW8*)ka;
#pragma unroll
        for (unsigned i = 0; i < sizeof(DevArgs) / 8; ++i) Ak.w[i] = src[i];
        Ak.a.io.actions = ka->Q.actions[k];
        Ak.a.io.obs = ka->Q.obs[k];
        step_body<T, VK, SYM, RAYS, EPG, NT, false, false, WB, 2, true>(Ak.a, tix, bix);
        if (k + 1 < n) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (NT > 64) __builtin_amdgcn_s_barrier();
            asm volatile("buffer_inv sc0" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
    }
}

// (and the sphere-only twin of that: NOCAP on top of NOCUR -- a copy for the reason given at step_seq_nocur_kernel)
template <typename T, int VK, bool SYM, bool RAYS, int EPG, int NT, bool WB>
__global__ __launch_bounds__(NT, (min_waves_<T, NT>())) void step_seq_nocap_kernel(const DevArgs, const SeqArgs) {
    struct KernArgs { DevArgs A; SeqArgs Q; };   // (the kernarg segment: both arguments by value, 8-byte aligned)
    static_assert(alignof(DevArgs) == 8 && alignof(SeqArgs) == 8 && sizeof(DevArgs) % 8 == 0, "kernarg layout");
    typedef const __attribute__((address_space(4))) KernArgs CKA;
    CKA* ka = (CKA*)__builtin_amdgcn_kernarg_segment_ptr();
    unsigned tix = threadIdx.x, bix = blockIdx.x;
    const int n = ka->Q.n;
    for (int k = 0; k < n; ++k) {
        asm volatile("" : "+s"(ka));
        asm volatile("" : "+v"(tix));
        asm volatile("" : "+s"(bix));
        union { DevArgs a; unsigned long long w[sizeof(DevArgs) / 8]; } Ak;
        typedef const __attribute__((address_space(4))) unsigned long long CW8;
        CW8* const src = (CW8*)ka;
#pragma unroll
        for (unsigned i = 0; i < sizeof(DevArgs) / 8; ++i) Ak.w[i] = src[i];
        Ak.a.io.actions = ka->Q.actions[k];
        Ak.a.io.obs = ka->Q.obs[k];
        step_body<T, VK, SYM, RAYS, EPG, NT, false, false, WB, 2, true, true>(Ak.a, tix, bix);
        if (k + 1 < n) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (NT > 64) __builtin_amdgcn_s_barrier();
            asm volatile("buffer_inv sc0" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
    }
}

template <typename T, int VK, bool SYM, bool RAYS, int EPG, int NT, bool WB = false, bool NOCUR = false, bool NOCAP = false>
static int launch_seq_one(const KernelArgs<T, 2>& a, const SeqArgs& seq, void* stream) {
    const EnvP<T>& E = a.P.E;
    const int groups = (E.n_envs + EPG - 1) / EPG;
    const size_t lds = lds_bytes<T>(EPG, NT, E.max_cap, E.max_sph, E.n_obs, RAYS, E.ray_pad_log2);
    DevArgs d;
    d.params = a.params_dev;
    d.B = a.B;
    d.io = a.io;
    d.n_envs = E.n_envs;
    void (*kernel)(const DevArgs, const SeqArgs);
    static_assert(!NOCAP || NOCUR, "the sphere-only twins stand on the lean ones");
    if constexpr (NOCAP) kernel = &step_seq_nocap_kernel<T, VK, SYM, RAYS, EPG, NT, WB>;
    else if constexpr (NOCUR) kernel = &step_seq_nocur_kernel<T, VK, SYM, RAYS, EPG, NT, WB>;
    else kernel = &step_seq_kernel<T, VK, SYM, RAYS, EPG, NT, WB>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kernel, dim3(groups), dim3(NT), lds, (hipStream_t)stream, d, seq);
    return (int)hipGetLastError();
}

// the resident instantiations that exist for <float, VK> (select_sequence picks; the mixed kernel's write-back twin of 256
// threads is compiled and never picked, see there)
template <typename T, int VK>
static int launch_seq_vk(const KernelArgs<T, 2>& a, const StepRequest& r, const SeqArgs& seq, void* stream) {
    const StepVariant v = select_sequence(r);
    if (v.unsupported) return (int)hipErrorNotSupported;
    const auto is = [&](bool rays, int nt, bool wb) { return r.has_rays == rays && v.NT == nt && v.WB == wb; };
    if (v.NOCUR) {   // (the lean twins: nocur_shape)
        if constexpr (VK == VK_JOY) {
            if (is(false, 256, true)) return launch_seq_one<T, VK, true, false, 64, 256, true, true>(a, seq, stream);
            if (v.NOCAP && is(true, 256, false)) return launch_seq_one<T, VK, true, true, 64, 256, false, true, true>(a, seq, stream);
            if (is(true, 256, false)) return launch_seq_one<T, VK, true, true, 64, 256, false, true>(a, seq, stream);
        }
        if constexpr (VK == VK_LAUV) {
            if (is(true, 512, true)) return launch_seq_one<T, VK, true, true, 64, 512, true, true>(a, seq, stream);
        }
        return (int)hipErrorNotSupported;
    }
    if (is(false, 256, true)) return launch_seq_one<T, VK, true, false, 64, 256, true>(a, seq, stream);
    if (is(false, 128, true)) return launch_seq_one<T, VK, true, false, 64, 128, true>(a, seq, stream);
    if (is(false, 64, true)) return launch_seq_one<T, VK, true, false, 64, 64, true>(a, seq, stream);
    if (is(true, 512, true)) return launch_seq_one<T, VK, true, true, 64, 512, true>(a, seq, stream);
    if (is(true, 256, true)) return launch_seq_one<T, VK, true, true, 64, 256, true>(a, seq, stream);
    if (is(true, 256, false)) return launch_seq_one<T, VK, true, true, 64, 256>(a, seq, stream);
    if (is(true, 64, false)) return launch_seq_one<T, VK, true, true, 64, 64>(a, seq, stream);
    return (int)hipErrorNotSupported;
}

// ------------------------------------------------------------------------------------------ launchers
// NOCUR: the lean twin of a plain or TERM product kernel (step_nocur_kernel / step_ride_nocur_kernel)
// NOCAP: the sphere-only twin of that (step_nocap_kernel / step_ride_nocap_kernel)
template <typename T, int VK, bool SYM, bool RAYS, int EPG, int NT, bool LOG = false, bool TERM = false, bool WB = false, bool NOCUR = false,
          bool NOCAP = false>
static int launch_one(const KernelArgs<T, 2>& a, void* stream, void* ev0, void* ev1) {
    static_assert(!NOCUR || (!LOG && !WB), "the lean twins: plain and TERM product kernels");
    static_assert(!NOCAP || NOCUR, "the sphere-only twins stand on the lean ones");
    void (*kernel)(const DevArgs);
    if constexpr (NOCAP) kernel = &step_nocap_kernel<T, VK, SYM, RAYS, EPG, NT, TERM>;
    else if constexpr (NOCUR) kernel = &step_nocur_kernel<T, VK, SYM, RAYS, EPG, NT, TERM>;
    else kernel = &step_kernel<T, VK, SYM, RAYS, EPG, NT, LOG, TERM, WB>;
    const EnvP<T>& E = a.P.E;
    const int groups = (E.n_envs + EPG - 1) / EPG;
    const size_t lds = lds_bytes<T>(EPG, NT, E.max_cap, E.max_sph, E.n_obs, RAYS, E.ray_pad_log2);
    DevArgs d;
    d.params = a.params_dev;
    d.B = a.B;
    d.io = a.io;
    d.n_envs = E.n_envs;
    if (lds > 64 * 1024) {
        // gfx950 has 160 KiB of LDS per CU; more than 64 KiB per group must be requested explicitly.  The attribute
        // belongs to the (device, function) pair, and handles on several devices may share this process: it is set on
        // the launch path (wide fans / many obstacles only; a host-side call of a few microseconds), not cached
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    if (a.ride.plan) {
        if (LOG || TERM || WB) return (int)hipErrorNotSupported;   // (the riding gather is a throughput feature)
        // float kernels of the structural fast path only (both shipped vehicles); the caller falls back to a
        // separate gather kernel otherwise
        if constexpr (sizeof(T) == 4 && SYM) {
            void (*ride_kernel)(const DevArgs, const RideArgs);
            if constexpr (NOCAP) ride_kernel = &step_ride_nocap_kernel<T, VK, SYM, RAYS, EPG, NT>;
            else if constexpr (NOCUR) ride_kernel = &step_ride_nocur_kernel<T, VK, SYM, RAYS, EPG, NT>;
            else ride_kernel = &step_ride_kernel<T, VK, SYM, RAYS, EPG, NT>;
            if (lds > 64 * 1024) {
                hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ride_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (e != hipSuccess) return (int)e;
            }
            RideArgs r;
            r.plan = static_cast<const dockauv_p2p_plan*>(a.ride.plan);
            r.src = a.ride.src;
            r.stamp = a.ride.stamp;
            r.wait_stamp = a.ride.wait_stamp;
            hipLaunchKernelGGL(ride_kernel, dim3(groups + a.ride.groups), dim3(NT), lds < 16 ? (size_t)16 : lds, (hipStream_t)stream, d, r);
            return (int)hipGetLastError();
        } else {
            return (int)hipErrorNotSupported;
        }
    }
    if (ev0 || ev1) {
        // start/stop events attached to THIS dispatch: the elapsed time is the kernel's own duration
        hipExtLaunchKernelGGL(kernel, dim3(groups), dim3(NT), lds, (hipStream_t)stream, (hipEvent_t)ev0, (hipEvent_t)ev1, 0, d);
    } else {
        hipLaunchKernelGGL(kernel, dim3(groups), dim3(NT), lds, (hipStream_t)stream, d);
    }
    return (int)hipGetLastError();
}

// the instantiations that exist for <T, VK, SYM> (select_step picks; launch_one takes the ride branch of a plain one)
template <typename T, int VK, bool SYM>
static int launch_vk(const KernelArgs<T, 2>& a, const StepRequest& r, void* stream, void* ev0, void* ev1) {
    const StepVariant v = select_step(r);
    if (v.unsupported) return (int)hipErrorNotSupported;
    const auto is = [&](bool rays, int nt, bool log = false, bool term = false, bool wb = false) {
        return r.has_rays == rays && v.NT == nt && v.LOG == log && v.TERM == term && v.WB == wb;
    };
    constexpr bool TERM_OK = sizeof(T) == 4 && SYM && VK != VK_DENSEB;
    if (v.NOCUR) {   // (the lean twins: nocur_shape; launch_one takes the ride branch of a plain one)
        if constexpr (sizeof(T) == 4 && SYM && VK == VK_JOY) {
            if (v.NOCAP) {   // (the sphere-only twins: nocap_shape)
                if (is(true, 256)) return launch_one<T, VK, SYM, true, 64, 256, false, false, false, true, true>(a, stream, ev0, ev1);
                if (is(true, 256, false, true)) return launch_one<T, VK, SYM, true, 64, 256, false, true, false, true, true>(a, stream, ev0, ev1);
                return (int)hipErrorNotSupported;
            }
            if (is(false, 256)) return launch_one<T, VK, SYM, false, 64, 256, false, false, false, true>(a, stream, ev0, ev1);
            if (is(true, 256)) return launch_one<T, VK, SYM, true, 64, 256, false, false, false, true>(a, stream, ev0, ev1);
            if (is(false, 256, false, true)) return launch_one<T, VK, SYM, false, 64, 256, false, true, false, true>(a, stream, ev0, ev1);
            if (is(true, 256, false, true)) return launch_one<T, VK, SYM, true, 64, 256, false, true, false, true>(a, stream, ev0, ev1);
        }
        if constexpr (sizeof(T) == 4 && SYM && VK == VK_LAUV) {
            if (is(true, 512)) return launch_one<T, VK, SYM, true, 64, 512, false, false, false, true>(a, stream, ev0, ev1);
            if (is(true, 512, false, true)) return launch_one<T, VK, SYM, true, 64, 512, false, true, false, true>(a, stream, ev0, ev1);
        }
        return (int)hipErrorNotSupported;
    }
    if (is(true, 256, true)) return launch_one<T, VK, SYM, true, 64, 256, true>(a, stream, ev0, ev1);
    if (is(false, 256, true)) return launch_one<T, VK, SYM, false, 64, 256, true>(a, stream, ev0, ev1);
    if constexpr (TERM_OK) {
        if (is(false, 256, false, true)) return launch_one<T, VK, SYM, false, 64, 256, false, true>(a, stream, ev0, ev1);
        if (is(true, 512, false, true)) return launch_one<T, VK, SYM, true, 64, 512, false, true>(a, stream, ev0, ev1);
        if (is(true, 256, false, true)) return launch_one<T, VK, SYM, true, 64, 256, false, true>(a, stream, ev0, ev1);
        if (is(true, 256, false, false, true)) return launch_one<T, VK, SYM, true, 64, 256, false, false, true>(a, stream, ev0, ev1);
    }
    if (is(false, 256)) return launch_one<T, VK, SYM, false, 64, 256>(a, stream, ev0, ev1);
    if constexpr (sizeof(T) == 4 && SYM) {
        if (is(false, 128)) return launch_one<T, VK, SYM, false, 64, 128>(a, stream, ev0, ev1);
        if (is(false, 64)) return launch_one<T, VK, SYM, false, 64, 64>(a, stream, ev0, ev1);
    }
    if (is(false, 128, false, false, true)) return launch_one<T, VK, SYM, false, 64, 128, false, false, true>(a, stream, ev0, ev1);
    if (is(false, 64, false, false, true)) return launch_one<T, VK, SYM, false, 64, 64, false, false, true>(a, stream, ev0, ev1);
    if (is(true, 512)) return launch_one<T, VK, SYM, true, 64, 512>(a, stream, ev0, ev1);
    if (is(true, 256)) return launch_one<T, VK, SYM, true, 64, 256>(a, stream, ev0, ev1);
    if (is(true, 64)) return launch_one<T, VK, SYM, true, 64, 64>(a, stream, ev0, ev1);
    return (int)hipErrorNotSupported;
}

template <typename T, bool SYM>
static int launch_sym(const KernelArgs<T, 2>& a, const StepRequest& r, void* stream, void* ev0, void* ev1) {
    switch (r.vk) {
        case VK_JOY: return launch_vk<T, VK_JOY, SYM>(a, r, stream, ev0, ev1);
        case VK_DENSEB: return launch_vk<T, VK_DENSEB, SYM>(a, r, stream, ev0, ev1);
        case VK_LAUV: return launch_vk<T, VK_LAUV, SYM>(a, r, stream, ev0, ev1);
        case VK_MIXED: return launch_vk<T, VK_MIXED, SYM>(a, r, stream, ev0, ev1);
    }
    return (int)hipErrorInvalidValue;
}

template <typename T>
static int launch_t(const KernelArgs<T, 2>& a, const StepRequest& r, void* stream, void* ev0, void* ev1) {
    return r.sym ? launch_sym<T, true>(a, r, stream, ev0, ev1) : launch_sym<T, false>(a, r, stream, ev0, ev1);
}

#if defined(DOCKAUV_STAMPS) && defined(DOCKAUV_INSTANTIATE_F32)
int read_stamps(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 64 * 32);
}
int read_span(unsigned long long* out, int groups) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_span), sizeof(unsigned long long) * 6 * (size_t)(groups > 16384 ? 16384 : groups));
}
#endif
#ifdef DOCKAUV_INSTANTIATE_F32
int launch_step_f32(const KernelArgs<float, 2>& a, const StepRequest& r, void* stream, void* ev0, void* ev1) {
    return launch_t<float>(a, r, stream, ev0, ev1);
}
#endif
#ifdef DOCKAUV_INSTANTIATE_SEQ
int launch_sequence_f32(const KernelArgs<float, 2>& a, const StepRequest& r, const SeqArgs& seq, void* stream) {
    if (seq.n < 1 || seq.n > kSeqMax) return (int)hipErrorNotSupported;
    switch (r.vk) {
        case VK_JOY: return launch_seq_vk<float, VK_JOY>(a, r, seq, stream);
        case VK_LAUV: return launch_seq_vk<float, VK_LAUV>(a, r, seq, stream);
        case VK_MIXED: return launch_seq_vk<float, VK_MIXED>(a, r, seq, stream);
    }
    return (int)hipErrorNotSupported;
}
#endif
#ifdef DOCKAUV_INSTANTIATE_F64
int launch_step_f64(const KernelArgs<double, 2>& a, const StepRequest& r, void* stream, void* ev0, void* ev1) {
    return launch_t<double>(a, r, stream, ev0, ev1);
}
#endif

}  // namespace dockauv
