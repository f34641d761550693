// dockauv_capi_eval.hip -- C ABI of libdockauv.so (include/dockauv.h), third part: policy evaluation with an episode quota per
// env.  The kernels are in dockauv_eval.hip.
#include "dockauv_capi.h"

using namespace dockauv;

struct dockauv_eval_s {
    dockauv_handle h = nullptr;
    int n_slots = 0;              // S = max_episodes_per_env
    float* carry_ret = nullptr;   // [n_envs]: the running return of every env's episode
    int32_t* carry_len = nullptr; // [n_envs]: its length so far
    int32_t* count = nullptr;     // [n_envs]: episodes recorded since the begin
    int32_t* target = nullptr;    // [n_envs]: the quota, in [0, S]
    float* ep_return = nullptr;   // [S][n_envs]
    int32_t* ep_length = nullptr; // [S][n_envs]
    uint8_t* ep_outcome = nullptr;// [S][n_envs]
    double* ws = nullptr;         // eval_workspace_doubles(n_envs): the scan's partials
};

namespace {

// the carries <- the handle's own cumulative reward / step counters, then the begin launch, ordered on `stream`
int eval_begin(dockauv_eval e, const int32_t* targets, int uniform_target, hipStream_t stream) {
    dockauv_handle h = e->h;
    const size_t N = (size_t)h->cfg.n_envs;
    HIP_TRY(h, hipMemcpyAsync(e->carry_ret, h->B.cum_reward, N * sizeof(float), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(h, hipMemcpyAsync(e->carry_len, h->B.t_steps, N * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
    const int rc = launch_eval_begin(targets, uniform_target, e->count, e->target, e->ep_return, e->ep_length, e->ep_outcome,
                                     h->cfg.n_envs, e->n_slots, stream);
    return launched(h, "evaluation begin", rc, stream);
}

}  // namespace

extern "C" {

int dockauv_eval_create(dockauv_handle h, int max_episodes_per_env, dockauv_eval* out) {
    if (!out) return fail(h, DOCKAUV_E_INVALID, "dockauv_eval_create: out is NULL");
    *out = nullptr;
    if (max_episodes_per_env < 1)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_eval_create: max_episodes_per_env %d must be >= 1", max_episodes_per_env);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_eval_create: null handle");
    if ((long long)max_episodes_per_env * (long long)h->cfg.n_envs >= (1LL << 31))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_eval_create: max_episodes_per_env %d x n_envs %d: the slot arrays would reach 2^31 elements",
                    max_episodes_per_env, h->cfg.n_envs);
    if (int rc = refuse_f64_rows(h, "dockauv_eval_create")) return rc;
    if (int rc = refuse_reset_none(h, "dockauv_eval_create")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    dockauv_eval e = new dockauv_eval_s();
    e->h = h;
    e->n_slots = max_episodes_per_env;
    const size_t N = (size_t)h->cfg.n_envs, SN = (size_t)max_episodes_per_env * N;
    hipError_t err = hipMalloc((void**)&e->carry_ret, N * sizeof(float));
    if (err == hipSuccess) err = hipMalloc((void**)&e->carry_len, N * sizeof(int32_t));
    if (err == hipSuccess) err = hipMalloc((void**)&e->count, N * sizeof(int32_t));
    if (err == hipSuccess) err = hipMalloc((void**)&e->target, N * sizeof(int32_t));
    if (err == hipSuccess) err = hipMalloc((void**)&e->ep_return, SN * sizeof(float));
    if (err == hipSuccess) err = hipMalloc((void**)&e->ep_length, SN * sizeof(int32_t));
    if (err == hipSuccess) err = hipMalloc((void**)&e->ep_outcome, SN * sizeof(uint8_t));
    if (err == hipSuccess) err = hipMalloc((void**)&e->ws, eval_workspace_doubles(h->cfg.n_envs) * sizeof(double));
    if (err != hipSuccess) {
        dockauv_eval_destroy(e);
        return fail(h, DOCKAUV_E_HIP, "evaluation buffers: %s", hipGetErrorString(err));
    }
    // a begin with target 0, so that a scan before the caller's begin records nothing and reads no uninitialised count: what
    // the handle has queued comes first (the copies run on the default stream), and the object is usable on any stream on return
    int rc = sync_last(h);
    if (rc == 0) rc = eval_begin(e, nullptr, 0, nullptr);
    if (rc == 0 && (err = hipStreamSynchronize(nullptr)) != hipSuccess) rc = fail(h, DOCKAUV_E_HIP, "evaluation begin: %s", hipGetErrorString(err));
    if (rc != 0) {
        dockauv_eval_destroy(e);
        return rc;
    }
    *out = e;
    return 0;
}

int dockauv_eval_destroy(dockauv_eval e) {
    if (!e) return 0;
    if (e->h) (void)hipSetDevice(e->h->device);
    (void)hipDeviceSynchronize();
    void* bufs[] = {e->carry_ret, e->carry_len, e->count, e->target, e->ep_return, e->ep_length, e->ep_outcome, e->ws};
    for (void* p : bufs)
        if (p) (void)hipFree(p);
    delete e;
    return 0;
}

int dockauv_eval_begin(dockauv_eval e, const int32_t* targets, int uniform_target, void* hip_stream) {
    if (!e) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_eval_begin: null evaluator");
    if (!targets && (uniform_target < 0 || uniform_target > e->n_slots))
        return fail(e->h, DOCKAUV_E_INVALID, "dockauv_eval_begin: uniform_target %d outside [0, %d] (max_episodes_per_env)", uniform_target,
                    e->n_slots);
    HIP_TRY(e->h, hipSetDevice(e->h->device));
    return eval_begin(e, targets, uniform_target, (hipStream_t)hip_stream);
}

int dockauv_eval_scan(dockauv_handle h, dockauv_eval e, const dockauv_eval_io* io, void* hip_stream) {
    if (int rc = check_block(h, io, "dockauv_eval_scan", "io", "dockauv_eval_io")) return rc;
    if (io->n_steps < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_eval_io.n_steps: %d must be >= 1", io->n_steps);
    if (int rc = require(h, "dockauv_eval_io", {{"rows_out", io->rows_out}, {"stats", io->stats}})) return rc;
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_eval_scan: null handle");
    if (!e) return fail(h, DOCKAUV_E_INVALID, "dockauv_eval_scan: null evaluator");
    if (int rc = refuse_f64_rows(h, "dockauv_eval_scan")) return rc;
    if (int rc = refuse_reset_none(h, "dockauv_eval_scan")) return rc;
    if (e->h != h) return fail(h, DOCKAUV_E_INVALID, "dockauv_eval_scan: the evaluator was created for another handle");
    HIP_TRY(h, hipSetDevice(h->device));
    EvalArgs a{};
    a.rows = io->rows_out;
    a.terminal_obs = io->terminal_obs;
    a.carry_ret = e->carry_ret;
    a.carry_len = e->carry_len;
    a.count = e->count;
    a.target = e->target;
    a.ep_return = e->ep_return;
    a.ep_length = e->ep_length;
    a.ep_outcome = e->ep_outcome;
    a.partial = e->ws;
    a.stats = io->stats;
    a.n_steps = io->n_steps;
    a.n_envs = h->cfg.n_envs;
    a.n_obs = h->n_obs;
    a.row_stride = h->n_obs + 2;
    a.max_timesteps = h->cfg.max_timesteps;
    a.n_slots = e->n_slots;
    return launched(h, "evaluation", launch_eval_scan(a, hip_stream), hip_stream);
}

int dockauv_eval_state(dockauv_eval e, int32_t** count, int32_t** target, float** ep_return, int32_t** ep_length, uint8_t** ep_outcome,
                       float** carry_return, int32_t** carry_length) {
    if (!e) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_eval_state: null evaluator");
    if (count) *count = e->count;
    if (target) *target = e->target;
    if (ep_return) *ep_return = e->ep_return;
    if (ep_length) *ep_length = e->ep_length;
    if (ep_outcome) *ep_outcome = e->ep_outcome;
    if (carry_return) *carry_return = e->carry_ret;
    if (carry_length) *carry_length = e->carry_len;
    return 0;
}

}  // extern "C"
