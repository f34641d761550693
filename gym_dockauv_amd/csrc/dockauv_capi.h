// dockauv_capi.h -- what the translation units of the C ABI share (dockauv_capi.hip, dockauv_capi_policy.hip, dockauv_capi_collect.hip,
// dockauv_capi_optim.hip, dockauv_capi_sac.hip, dockauv_capi_eval.hip, dockauv_capi_replay.hip, dockauv_p2p.hip): the env handle, error
// reporting, the step launch, and the pieces every entry point checks alike.  Internal to libdockauv.so.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/dockauv.h"
#include "dockauv_device.h"

// host-pointer step staging (dockauv_step_host): one slot per array of dockauv_step_io, in its order
enum StageSlot {
    ST_ACTIONS, ST_NOISE, ST_OBS, ST_REWARD, ST_DONE, ST_TERMS, ST_COND, ST_NAV, ST_RAYDIST, ST_TERMOBS, ST_STATEDOT, ST_COUNT
};

struct dockauv_env_s {
    dockauv_config cfg;
    int device = 0;
    bool f64 = false;
    size_t tsz = 4;
    long S = 0;   // SoA row stride (envs rounded up to 64)
    int n_rays = 0, n_red = 0, n_obs = 0, n_u_max = 0;
    double fan_cos = -1.0, fan_sin = 0.0, sum_beta = 0.0;   // cone around the ray fan, sum of the ray weights
    int vk = dockauv::VK_JOY;
    bool has_rays = false;
    bool sym = false;
    int threads = 64;
    bool no_current = false;   // no water current in any env (dockauv_device.h: no_current_after_write); cleared by dockauv_set_field
    dockauv::Buffers B{};
    std::vector<void*> allocs;
    dockauv::KernelArgs<float, 2> a32{};
    dockauv::KernelArgs<double, 2> a64{};
    std::string err;
    bool seq_resident = true;   // dockauv_set_option(DOCKAUV_OPT_SEQUENCE_RESIDENT)
    volatile unsigned int* status_host = nullptr;   // the kernels' sticky status word: pinned, host-coherent, mapped into the device
    hipStream_t last_stream = nullptr;
    // host-pointer step staging: device buffer and its pinned host mirror (the mirrors are allocated on first use)
    struct Stage { size_t bytes = 0; void* dev = nullptr; void* pin = nullptr; } stage[ST_COUNT];
    bool pinned_ready = false;
    std::vector<void*> pinned_allocs;
    hipStream_t host_stream = nullptr;
    void* ride_plans_dev = nullptr;                 // device copies of the caller's gather plans (lag-1 sequences)
    std::vector<unsigned char> ride_plans_host;
    hipEvent_t ev_step[2] = {nullptr, nullptr};     // dockauv_step_gather_sequence: step kernel / gather of row buffer k
    hipEvent_t ev_gather[2] = {nullptr, nullptr};
    // episode-storage trace (dockauv_trace_*): ring buffers + their device-side description
    dockauv::TraceDev trace{};
    void* trace_dev = nullptr;                      // device copy of `trace`
    std::vector<void*> trace_allocs;
    long long trace_step = 0;
};

namespace dockauv {

extern thread_local std::string g_create_error;   // dockauv_last_error(NULL)

// the message goes to the handle, or without one to g_create_error; returns `code`
int fail(dockauv_handle h, int code, const char* fmt, ...);

#define HIP_TRY(h, expr)                                                                                   \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) return fail(h, DOCKAUV_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

int check_status(dockauv_handle h);   // the sticky status word: DOCKAUV_E_KERNEL once a kernel gave up a wait
int sync_last(dockauv_handle h);      // wait for the stream of the handle's last launch (none yet: for the device)
// one step on `stream`, with copy groups when h->a32.ride names a plan
int launch(dockauv_handle h, const dockauv_step_io* io, hipStream_t stream, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// dockauv_p2p.hip; returns a DOCKAUV_* code, message in g_create_error
int launch_gather(const dockauv_p2p_plan* pl, const void* src, uint32_t stamp, uint32_t wait_stamp, hipStream_t stream);

// ---- what the entry points check alike.  An entry point calls these top to bottom: the order of the calls is the order of refusal.

// a block's struct_size against the library's; `name`: the struct's
template <class T>
int check_size(dockauv_handle h, const T* b, const char* name) {
    if (b->struct_size != sizeof(T)) return fail(h, DOCKAUV_E_INVALID, "%s.struct_size: got %u, library has %zu", name, b->struct_size, sizeof(T));
    return 0;
}

// an io or desc block of `fn`: not NULL (`arg`: what the message calls it -- "io", "cio", "the dockauv_rewnorm_io"), then its size
template <class T>
int check_block(dockauv_handle h, const T* b, const char* fn, const char* arg, const char* name) {
    if (!b) return fail(h, DOCKAUV_E_INVALID, "%s: %s is NULL", fn, arg);
    return check_size(h, b, name);
}

// the pointers of block `name` that must not be NULL, refused in the list's order
struct Required {
    const char* field;
    const void* p;
};
inline int require(dockauv_handle h, const char* name, std::initializer_list<Required> fields) {
    for (const Required& r : fields)
        if (!r.p) return fail(h, DOCKAUV_E_INVALID, "%s.%s is NULL", name, r.field);
    return 0;
}

// the end of a launch: rc is the launcher's hipError_t (0: queued on `stream`, which becomes the handle's last)
inline int launch_failed(dockauv_handle h, const char* what, int rc) {
    return fail(h, DOCKAUV_E_HIP, "%s launch failed: %s", what, hipGetErrorString((hipError_t)rc));
}
inline int launched(dockauv_handle h, const char* what, int rc, void* stream) {
    if (rc != 0) return launch_failed(h, what, rc);
    h->last_stream = (hipStream_t)stream;
    return 0;
}

// what reads the packed float32 rows does not take a float64 handle
inline int refuse_f64_rows(dockauv_handle h, const char* fn) {
    if (h->f64) return fail(h, DOCKAUV_E_INVALID, "%s: the packed rows are float32; the handle's precision is DOCKAUV_F64", fn);
    return 0;
}

// what follows episodes through the rows needs envs that restart
inline int refuse_reset_none(dockauv_handle h, const char* fn) {
    if (h->cfg.reset_mode == DOCKAUV_RESET_NONE)
        return fail(h, DOCKAUV_E_INVALID, "%s: the handle's reset_mode is DOCKAUV_RESET_NONE: an episode does not restart at the row "
                    "after a done", fn);
    return 0;
}

}  // namespace dockauv
