// dockauv_capi_replay.hip -- C ABI of libdockauv.so (include/dockauv.h), fourth part: the replay buffer.  The kernels are in
// dockauv_replay.hip, the record layout in dockauv_replay.h.
#include "dockauv_capi.h"
#include "dockauv_replay.h"

using namespace dockauv;

struct dockauv_replay_s {
    dockauv_handle h = nullptr;
    uint64_t seed = 0;
    long long capacity_steps = 0;
    int record_floats = 0;
    float* storage = nullptr;                 // [capacity_steps][n_envs][record_floats]
    float* carry[2] = {nullptr, nullptr};     // [n_envs][n_obs] each: a push reads carry[cur] and writes the other
    int cur = 0;
    // host-side counts, read when a call is made and updated by it
    long long pos = 0, size = 0;
    uint64_t draws = 0;
};

namespace {

// the checks push, sample and sync share; `what` names the entry point
int check_pair(dockauv_handle h, dockauv_replay rb, const char* what) {
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", what);
    if (!rb) return fail(h, DOCKAUV_E_INVALID, "%s: null replay buffer", what);
    if (rb->h != h) return fail(h, DOCKAUV_E_INVALID, "%s: the replay buffer was created for another handle", what);
    return 0;
}

}  // namespace

extern "C" {

int dockauv_replay_create(dockauv_handle h, long long buffer_size, uint64_t seed, dockauv_replay* out) {
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_replay_create: null handle");
    if (!out) return fail(h, DOCKAUV_E_INVALID, "dockauv_replay_create: out is NULL");
    *out = nullptr;
    if (buffer_size < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_replay_create: buffer_size %lld must be >= 1", buffer_size);
    if (int rc = refuse_f64_rows(h, "dockauv_replay_create")) return rc;
    if (int rc = refuse_reset_none(h, "dockauv_replay_create")) return rc;
    const long long N = h->cfg.n_envs;
    const long long cap = buffer_size / N > 1 ? buffer_size / N : 1;   // SB3: max(buffer_size // n_envs, 1)
    if (cap >= (1LL << 31))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_replay_create: buffer_size %lld / n_envs %lld: capacity_steps would reach 2^31", buffer_size, N);
    HIP_TRY(h, hipSetDevice(h->device));
    dockauv_replay rb = new dockauv_replay_s();
    rb->h = h;
    rb->seed = seed;
    rb->capacity_steps = cap;
    rb->record_floats = replay_record_floats(h->n_obs, h->n_u_max);
    const size_t ring = (size_t)replay_record_byte_offset((unsigned long long)cap * (unsigned long long)N, rb->record_floats);
    const size_t carry = (size_t)N * (size_t)h->n_obs * sizeof(float);
    hipError_t e = hipMalloc((void**)&rb->storage, ring);
    if (e == hipSuccess) e = hipMalloc((void**)&rb->carry[0], carry);
    if (e == hipSuccess) e = hipMalloc((void**)&rb->carry[1], carry);
    if (e == hipSuccess) e = hipMemset(rb->storage, 0, ring);
    if (e == hipSuccess) e = hipMemset(rb->carry[0], 0, carry);
    if (e == hipSuccess) e = hipMemset(rb->carry[1], 0, carry);
    if (e == hipSuccess) e = hipDeviceSynchronize();   // the object is usable on any stream on return
    if (e != hipSuccess) {
        dockauv_replay_destroy(rb);
        return fail(h, DOCKAUV_E_HIP, "replay buffers (%zu bytes): %s", ring + 2 * carry, hipGetErrorString(e));
    }
    *out = rb;
    return 0;
}

int dockauv_replay_destroy(dockauv_replay rb) {
    if (!rb) return 0;
    if (rb->h) (void)hipSetDevice(rb->h->device);
    (void)hipDeviceSynchronize();
    void* bufs[] = {rb->storage, rb->carry[0], rb->carry[1]};
    for (void* p : bufs)
        if (p) (void)hipFree(p);
    delete rb;
    return 0;
}

int dockauv_replay_sync(dockauv_handle h, dockauv_replay rb, const float* rows, void* hip_stream) {
    if (const int rc = check_pair(h, rb, "dockauv_replay_sync")) return rc;
    if (!rows) return fail(h, DOCKAUV_E_INVALID, "dockauv_replay_sync: rows is NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    return launched(h, "replay sync", launch_replay_sync(rows, rb->carry[rb->cur], h->cfg.n_envs, h->n_obs, hip_stream), hip_stream);
}

int dockauv_replay_push(dockauv_handle h, dockauv_replay rb, const dockauv_replay_push_io* io, void* hip_stream) {
    if (const int rc = check_pair(h, rb, "dockauv_replay_push")) return rc;
    if (int rc = check_block(h, io, "dockauv_replay_push", "io", "dockauv_replay_push_io")) return rc;
    if (io->n_steps < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_replay_push_io.n_steps: %d must be >= 1", io->n_steps);
    if ((long long)io->n_steps > rb->capacity_steps)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_replay_push_io.n_steps: %d exceeds capacity_steps %lld", io->n_steps, rb->capacity_steps);
    if ((long long)io->n_steps * (long long)h->cfg.n_envs >= (1LL << 31))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_replay_push_io.n_steps: %d x n_envs %d reaches 2^31 records in one push", io->n_steps,
                    h->cfg.n_envs);
    if (int rc = require(h, "dockauv_replay_push_io", {{"rows_out", io->rows_out}, {"actions", io->actions}})) return rc;
    if (!io->terminal_obs) return fail(h, DOCKAUV_E_INVALID, "dockauv_replay_push_io.terminal_obs is NULL (next_obs where done)");
    HIP_TRY(h, hipSetDevice(h->device));
    ReplayPushArgs a{};
    a.storage = rb->storage;
    a.obs0 = io->rows_in ? io->rows_in : rb->carry[rb->cur];
    a.obs0_stride = io->rows_in ? h->n_obs + 2 : h->n_obs;
    a.rows_out = io->rows_out;
    a.actions = io->actions;
    a.terminal_obs = io->terminal_obs;
    a.ep_outcome = io->ep_outcome;
    a.carry_out = rb->carry[rb->cur ^ 1];
    a.n_steps = io->n_steps;
    a.n_envs = h->cfg.n_envs;
    a.n_obs = h->n_obs;
    a.n_u = h->n_u_max;
    a.record_floats = rb->record_floats;
    a.pos = rb->pos;
    a.capacity_steps = rb->capacity_steps;
    const int rc = launch_replay_push(a, hip_stream);
    if (rc != 0) return launch_failed(h, "replay push", rc);
    rb->cur ^= 1;
    rb->pos = (rb->pos + io->n_steps) % rb->capacity_steps;
    rb->size = rb->size + io->n_steps < rb->capacity_steps ? rb->size + io->n_steps : rb->capacity_steps;
    h->last_stream = (hipStream_t)hip_stream;
    return 0;
}

int dockauv_replay_sample(dockauv_handle h, dockauv_replay rb, const dockauv_replay_sample_io* io, void* hip_stream) {
    if (const int rc = check_pair(h, rb, "dockauv_replay_sample")) return rc;
    if (int rc = check_block(h, io, "dockauv_replay_sample", "io", "dockauv_replay_sample_io")) return rc;
    if (io->batch_size < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_replay_sample_io.batch_size: %lld must be >= 1", io->batch_size);
    if (io->n_batches < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_replay_sample_io.n_batches: %d must be >= 1", io->n_batches);
    if (io->batch_size >= (1LL << 31) || io->batch_size * (long long)io->n_batches >= (1LL << 31))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_replay_sample_io.batch_size: %lld x n_batches %d reaches 2^31 transitions in one call",
                    io->batch_size, io->n_batches);
    if (int rc = require(h, "dockauv_replay_sample_io", {{"obs", io->obs}, {"actions", io->actions}, {"next_obs", io->next_obs},
                                                         {"rewards", io->rewards}, {"dones", io->dones}}))
        return rc;
    if (rb->size < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_replay_sample: size is 0: nothing has been pushed");
    HIP_TRY(h, hipSetDevice(h->device));
    ReplaySampleArgs a{};
    a.storage = rb->storage;
    a.obs = io->obs;
    a.actions = io->actions;
    a.next_obs = io->next_obs;
    a.rewards = io->rewards;
    a.dones = io->dones;
    a.index = io->index;
    a.batch_size = io->batch_size;
    a.n_batches = io->n_batches;
    a.n_envs = h->cfg.n_envs;
    a.n_obs = h->n_obs;
    a.n_u = h->n_u_max;
    a.record_floats = rb->record_floats;
    a.size = (uint32_t)rb->size;
    a.seed = rb->seed;
    a.draws = rb->draws;
    const int rc = launch_replay_sample(a, hip_stream);
    if (rc != 0) return launch_failed(h, "replay sample", rc);
    rb->draws += (uint64_t)io->n_batches;
    h->last_stream = (hipStream_t)hip_stream;
    return 0;
}

int dockauv_replay_counts(dockauv_replay rb, long long* pos, long long* size, uint64_t* draws) {
    if (!rb) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_replay_counts: null replay buffer");
    if (pos) *pos = rb->pos;
    if (size) *size = rb->size;
    if (draws) *draws = rb->draws;
    return 0;
}

int dockauv_replay_set_counts(dockauv_replay rb, long long pos, long long size, uint64_t draws) {
    if (!rb) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_replay_set_counts: null replay buffer");
    if (pos < 0 || pos >= rb->capacity_steps)
        return fail(rb->h, DOCKAUV_E_INVALID, "dockauv_replay_set_counts: pos %lld outside [0, %lld) (capacity_steps)", pos, rb->capacity_steps);
    if (size < 0 || size > rb->capacity_steps)
        return fail(rb->h, DOCKAUV_E_INVALID, "dockauv_replay_set_counts: size %lld outside [0, %lld] (capacity_steps)", size, rb->capacity_steps);
    rb->pos = pos;
    rb->size = size;
    rb->draws = draws;
    return 0;
}

int dockauv_replay_state(dockauv_replay rb, float** storage, float** carry, long long* capacity_steps, int* record_floats) {
    if (!rb) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_replay_state: null replay buffer");
    if (storage) *storage = rb->storage;
    if (carry) *carry = rb->carry[rb->cur];
    if (capacity_steps) *capacity_steps = rb->capacity_steps;
    if (record_floats) *record_floats = rb->record_floats;
    return 0;
}

}  // extern "C"
