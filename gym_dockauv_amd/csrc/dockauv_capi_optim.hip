// dockauv_capi_optim.hip -- C ABI of libdockauv.so (include/dockauv.h), PPO's update part: the optimiser object (Adam with
// gradient-norm clipping), dockauv_permutation and the whole update in one call, dockauv_ppo_update.
// The kernels are in dockauv_optim / _update / _head.hip.
#include "dockauv_capi_policy.h"

using namespace dockauv;

struct dockauv_optim_s {
    dockauv_handle h = nullptr;
    dockauv_policy actor = nullptr, critic = nullptr;   // critic: nullable
    double beta1 = 0.9, beta2 = 0.999, eps = 1e-5;
    float max_grad_norm = 0.0f;
    long long t = 0;              // steps taken
    int len[kOptSegments] = {};   // the index space: actor W1 b1 W2 b2 W3 b3, log_std, critic W1 b1 W2 b2 W3 b3
    int total = 0;
    float *m = nullptr, *v = nullptr;   // [total] each, one allocation (m first)
    // dockauv_ppo_update: allocated by its first call, grown when a later call needs more
    OptimCtl* ctl = nullptr;      // the control block
    long long* index = nullptr;   // [index_rows]: an epoch's permutation
    long long index_rows = 0;
    float* scratch = nullptr;     // one minibatch of scratch_rows rows: mean and grad_mean [rows][n_out], v and grad_v [rows]
    long long scratch_rows = 0;
    bool pending = false;         // t is behind the control block's count (an update with target_kl > 0 is queued)
    hipStream_t pending_stream = nullptr;
};

namespace {

// one network's six parameter / gradient pointers against its segment lengths; `who`: "actor" / "critic"
int check_optim_arrays(dockauv_handle h, const char* who, const int* len, float* const* params, const float* const* grads) {
    static const char* const names[6] = {"W1", "b1", "W2", "b2", "W3", "b3"};
    for (int i = 0; i < 6; ++i) {
        if (len[i] > 0 && !params[i]) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_io.%s_params[%d] (%s) is NULL", who, i, names[i]);
        if (len[i] > 0 && !grads[i]) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_io.%s_grads[%d] (%s) is NULL", who, i, names[i]);
        if (len[i] == 0 && params[i])
            return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_io.%s_params[%d] (%s) must be NULL: the optimiser's shapes have no such array", who, i, names[i]);
        if (len[i] == 0 && grads[i])
            return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_io.%s_grads[%d] (%s) must be NULL: the optimiser's shapes have no such array", who, i, names[i]);
        if (len[i] > 0 && (const float*)params[i] == grads[i])
            return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_io.%s_grads[%d] (%s) is the params pointer: gradients are read only, parameters written", who, i, names[i]);
    }
    return 0;
}

// the policy's weights from the six device arrays (and log_std), packed on `stream`: dockauv_policy_load with device pointers,
// keeping the policy's seed and env id offset
int repack_policy(dockauv_policy p, float* const* params, const float* log_std, hipStream_t stream) {
    dockauv_policy_desc d{};
    d.struct_size = sizeof(dockauv_policy_desc);
    d.pointers_on_device = 1;
    d.W1 = params[0]; d.b1 = params[1]; d.W2 = params[2]; d.b2 = params[3]; d.W3 = params[4]; d.b3 = params[5];
    d.log_std = log_std;
    d.seed = p->seed;
    d.env_id_offset = p->env_id_offset;
    return upload_policy(p, &d, stream);
}

// a dockauv_optim_io against the optimiser (dockauv_optim_step, and the `opt` of dockauv_ppo_update)
int check_optim_io(dockauv_handle h, dockauv_optim o, const dockauv_optim_io* io) {
    if (!(io->lr >= 0.0) || !std::isfinite(io->lr)) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_io.lr: %g must be >= 0 and finite", io->lr);
    if (int rc = check_optim_arrays(h, "actor", o->len, io->actor_params, io->actor_grads)) return rc;
    if (int rc = require(h, "dockauv_optim_io", {{"log_std", io->log_std}, {"grad_log_std", io->grad_log_std}})) return rc;
    if ((const float*)io->log_std == io->grad_log_std)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_io.grad_log_std is the log_std pointer: gradients are read only, parameters written");
    return check_optim_arrays(h, "critic", o->len + 7, io->critic_params, io->critic_grads);
}

// the optimiser launch's arguments but the step's two bias corrections
void adam_args(dockauv_optim o, const dockauv_optim_io* io, float* stats, AdamArgs& a) {
    for (int i = 0; i < 6; ++i) {
        a.p[i] = io->actor_params[i];
        a.g[i] = io->actor_grads[i];
        a.p[7 + i] = io->critic_params[i];
        a.g[7 + i] = io->critic_grads[i];
    }
    a.p[6] = io->log_std;
    a.g[6] = io->grad_log_std;
    for (int s = 0; s < kOptSegments; ++s) a.len[s] = o->len[s];
    a.m = o->m;
    a.v = o->v;
    a.stats = stats;
    a.total = o->total;
    a.max_grad_norm = o->max_grad_norm;
    a.c1 = (float)(1.0 - o->beta1);
    a.c2 = (float)(1.0 - o->beta2);
    a.b2 = (float)o->beta2;
    a.eps = (float)o->eps;
}

// o->t <- the control block's count when an update with target_kl > 0 left it pending: waits for that update's stream
int reconcile_steps(dockauv_optim o) {
    if (!o->pending) return 0;
    dockauv_handle h = o->h;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(o->pending_stream));
    long long t = 0;
    HIP_TRY(h, hipMemcpy(&t, &o->ctl->t, sizeof(t), hipMemcpyDeviceToHost));
    o->t = t;
    o->pending = false;
    return 0;
}

}  // namespace

extern "C" {

int dockauv_optim_create(dockauv_handle h, dockauv_policy actor, dockauv_policy critic, const dockauv_optim_desc* d, dockauv_optim* out) {
    const char* fn = "dockauv_optim_create";
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (!out) return fail(h, DOCKAUV_E_INVALID, "%s: out is NULL", fn);
    *out = nullptr;
    if (!actor) return fail(h, DOCKAUV_E_INVALID, "%s: null actor", fn);
    if (int rc = check_block(h, d, fn, "desc", "dockauv_optim_desc")) return rc;
    if (actor->h != h) return fail(h, DOCKAUV_E_INVALID, "%s: the actor was created for another handle", fn);
    if (actor->role == Role::Value) return fail(h, DOCKAUV_E_INVALID, "%s: the actor argument is %s", fn, phrase(actor->role).ppo);
    if (int rc = refuse_sac(h, actor, fn)) return rc;
    if (!actor->has_log_std) return fail(h, DOCKAUV_E_INVALID, "%s: the actor has no log_std (its gradient is part of the index space)", fn);
    if (critic)
        if (int rc = check_critic(h, critic, fn)) return rc;
    if (!(d->beta1 >= 0.0 && d->beta1 < 1.0)) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_desc.beta1: %g outside [0, 1)", d->beta1);
    if (!(d->beta2 >= 0.0 && d->beta2 < 1.0)) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_desc.beta2: %g outside [0, 1)", d->beta2);
    if (!(d->eps > 0.0) || !std::isfinite(d->eps)) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_desc.eps: %g must be > 0", d->eps);
    if (std::isnan(d->max_grad_norm)) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_desc.max_grad_norm is NaN");
    HIP_TRY(h, hipSetDevice(h->device));
    dockauv_optim o = new dockauv_optim_s();
    o->h = h;
    o->actor = actor;
    o->critic = critic;
    o->beta1 = d->beta1;
    o->beta2 = d->beta2;
    o->eps = d->eps;
    o->max_grad_norm = d->max_grad_norm;
    layer_lengths(actor->S, o->len);
    o->len[6] = actor->S.n_out;
    if (critic) layer_lengths(critic->S, o->len + 7);
    for (int s = 0; s < kOptSegments; ++s) o->total += o->len[s];
    hipError_t e = hipMalloc((void**)&o->m, 2 * (size_t)o->total * sizeof(float));
    if (e == hipSuccess) e = hipMemset(o->m, 0, 2 * (size_t)o->total * sizeof(float));
    if (e != hipSuccess) {
        dockauv_optim_destroy(o);
        return fail(h, DOCKAUV_E_HIP, "optimiser state: %s", hipGetErrorString(e));
    }
    o->v = o->m + o->total;
    *out = o;
    return 0;
}

int dockauv_optim_destroy(dockauv_optim o) {
    if (!o) return 0;
    if (o->h) (void)hipSetDevice(o->h->device);
    (void)hipDeviceSynchronize();
    if (o->m) (void)hipFree(o->m);
    if (o->ctl) (void)hipFree(o->ctl);
    if (o->index) (void)hipFree(o->index);
    if (o->scratch) (void)hipFree(o->scratch);
    delete o;
    return 0;
}

int dockauv_optim_state(dockauv_optim o, float** m, float** v, long long* n_elements, long long* steps) {
    if (!o) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_optim_state: null optimiser");
    if (int rc = reconcile_steps(o)) return rc;
    if (m) *m = o->m;
    if (v) *v = o->v;
    if (n_elements) *n_elements = o->total;
    if (steps) *steps = o->t;
    return 0;
}

int dockauv_optim_step(dockauv_handle h, dockauv_optim o, const dockauv_optim_io* io, void* hip_stream) {
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_optim_step: null handle");
    if (!o) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_step: null optimiser");
    if (int rc = check_block(h, io, "dockauv_optim_step", "io", "dockauv_optim_io")) return rc;
    if (o->h != h) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_step: the optimiser was created for another handle");
    if (int rc = check_optim_io(h, o, io)) return rc;
    if (int rc = reconcile_steps(o)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    const long long t = ++o->t;
    AdamArgs a{};
    adam_args(o, io, io->stats, a);
    bias_corrections(o->beta1, o->beta2, io->lr, t, a.step_size, a.rsq);
    if (int rc = launched(h, "optimiser", launch_adam_step(a, stream), stream)) return rc;
    if (int rc = repack_policy(o->actor, io->actor_params, io->log_std, stream)) return rc;
    if (o->critic)
        if (int rc = repack_policy(o->critic, io->critic_params, nullptr, stream)) return rc;
    return 0;
}

int dockauv_permutation(dockauv_handle h, uint64_t seed, uint64_t epoch, long long n, int64_t* out, void* hip_stream) {
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_permutation: null handle");
    if (!out) return fail(h, DOCKAUV_E_INVALID, "dockauv_permutation: out is NULL");
    if (n < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_permutation: n %lld must be >= 1", n);
    if (n > (1ll << 31)) return fail(h, DOCKAUV_E_INVALID, "dockauv_permutation: n %lld must be <= 2^31 (the network works on 32-bit words)", n);
    HIP_TRY(h, hipSetDevice(h->device));
    return launched(h, "permutation", launch_permutation(seed, epoch, n, (long long*)out, hip_stream), hip_stream);
}

int dockauv_ppo_update(dockauv_handle h, dockauv_optim o, const dockauv_ppo_update_io* io, void* hip_stream) {
    const char* io_name = "dockauv_ppo_update_io";
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_ppo_update: null handle");
    if (!o) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update: null optimiser");
    if (int rc = check_block(h, io, "dockauv_ppo_update", "io", io_name)) return rc;
    if (o->h != h) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update: the optimiser was created for another handle");
    dockauv_policy actor = o->actor, critic = o->critic;
    if (int rc = check_actor(h, actor, "dockauv_ppo_update", true)) return rc;
    const long long M = io->n_rows, B = io->batch_size;
    if (M < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.n_rows: %lld must be >= 1", M);
    if (M > (1ll << 31)) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.n_rows: %lld must be <= 2^31 (dockauv_permutation)", M);
    if (B < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.batch_size: %lld must be >= 1", B);
    if (io->n_epochs < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.n_epochs: %d must be >= 1", io->n_epochs);
    const long long J = (M + B - 1) / B, last = M - (J - 1) * B;
    if (io->normalize_advantage && last < 2)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.batch_size: the last minibatch of %lld rows in batches of %lld has one row, "
                    "normalize_advantage needs two (the unbiased deviation)", M, B);
    if (!(io->clip_range > 0.0f)) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.clip_range: %g must be > 0", (double)io->clip_range);
    if (!(io->clip_range_vf >= 0.0f)) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.clip_range_vf: %g must be >= 0 (0 = off)", (double)io->clip_range_vf);
    if (!(io->target_kl >= 0.0f)) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.target_kl: %g must be >= 0 (0 = off)", (double)io->target_kl);
    if (int rc = require(h, io_name, {{"rows", io->rows}, {"actions", io->actions}, {"log_prob_old", io->log_prob_old},
                                      {"advantages", io->advantages}}))
        return rc;
    if (critic && !io->returns) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.returns is NULL (the optimiser has a critic)");
    if (io->clip_range_vf > 0.0f && !critic)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.clip_range_vf: %g, but the optimiser has no critic", (double)io->clip_range_vf);
    if (io->clip_range_vf > 0.0f && !io->values_old)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.values_old is NULL (clip_range_vf is %g)", (double)io->clip_range_vf);
    if (int rc = require(h, io_name, {{"stats", io->stats}})) return rc;
    if (int rc = check_size(h, &io->opt, "dockauv_optim_io")) return rc;
    if (int rc = check_optim_io(h, o, &io->opt)) return rc;
    if (io->opt.stats)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.opt.stats must be NULL: the norm and coef go to columns 8, 9 of dockauv_ppo_update_io.stats");
    for (dockauv_policy p : {actor, critic}) {
        if (!p) continue;
        BackwardLayout L;
        backward_layout(p->S, L);
        if (backward_lds_bytes(L) > kPolMaxLds)
            return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update: the backward kernel needs %zu B of LDS for n_in %d, n_hidden %d / %d, more than "
                        "the 160 KiB of a group (dockauv_policy_backward)", backward_lds_bytes(L), p->S.n_in, p->S.n_h1, p->S.n_h2);
    }
    if (int rc = reconcile_steps(o)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t stream = (hipStream_t)hip_stream;

    // the optimiser's buffers: allocated here the first time, grown when this call needs more (hipFree waits for the device)
    const int n_u = actor->S.n_out;
    const long long rows_mb = B < M ? B : M;
    if (!o->ctl) HIP_TRY(h, hipMalloc((void**)&o->ctl, sizeof(OptimCtl)));
    if (o->index_rows < M) {
        if (o->index) HIP_TRY(h, hipFree(o->index));
        o->index = nullptr;
        o->index_rows = 0;
        HIP_TRY(h, hipMalloc((void**)&o->index, (size_t)M * sizeof(long long)));
        o->index_rows = M;
    }
    if (o->scratch_rows < rows_mb) {
        if (o->scratch) HIP_TRY(h, hipFree(o->scratch));
        o->scratch = nullptr;
        o->scratch_rows = 0;
        HIP_TRY(h, hipMalloc((void**)&o->scratch, (size_t)rows_mb * (2 * (size_t)n_u + 2) * sizeof(float)));
        o->scratch_rows = rows_mb;
    }
    if (!actor->head_ws) HIP_TRY(h, hipMalloc((void**)&actor->head_ws, kHeadWorkspaceBytes));
    float* mean = o->scratch;
    float* grad_mean = mean + (size_t)rows_mb * n_u;
    float* v = grad_mean + (size_t)rows_mb * n_u;
    float* grad_v = v + rows_mb;

    const long long t0 = o->t;
    int rc = launch_update_begin(o->ctl, t0, stream);
    if (rc != 0) return launch_failed(h, "update control", rc);
    dockauv_policy_grads ag{}, cg{};
    ag.struct_size = cg.struct_size = sizeof(dockauv_policy_grads);
    float* const* agp = (float* const*)io->opt.actor_grads;     // (the caller's gradient buffers: read by the optimiser, written here)
    float* const* cgp = (float* const*)io->opt.critic_grads;
    ag.dW1 = agp[0]; ag.db1 = agp[1]; ag.dW2 = agp[2]; ag.db2 = agp[3]; ag.dW3 = agp[4]; ag.db3 = agp[5];
    cg.dW1 = cgp[0]; cg.db1 = cgp[1]; cg.dW2 = cgp[2]; cg.db2 = cgp[3]; cg.dW3 = cgp[4]; cg.db3 = cgp[5];
    long long k = 0;      // minibatches queued by this call
    for (int e = 0; e < io->n_epochs; ++e) {
        rc = launch_permutation(io->seed, io->first_epoch + (uint64_t)e, M, o->index, stream);
        if (rc != 0) return launch_failed(h, "permutation", rc);
        for (long long j = 0; j < J; ++j, ++k) {
            const long long n = j + 1 < J ? B : last;
            const int64_t* idx = (const int64_t*)(o->index + j * B);
            float* st = io->stats + (size_t)k * 12;
            if ((rc = dockauv_policy_forward_rows(h, actor, io->rows, idx, n, mean, stream)) != 0) return rc;
            if (critic && (rc = dockauv_policy_forward_rows(h, critic, io->rows, idx, n, v, stream)) != 0) return rc;
            dockauv_ppo_head_io hio{};
            hio.normalize_advantage = io->normalize_advantage;
            hio.mean = mean;
            hio.v = critic ? v : nullptr;
            hio.actions = io->actions;
            hio.log_prob_old = io->log_prob_old;
            hio.advantages = io->advantages;
            hio.returns = critic ? io->returns : nullptr;
            hio.row_index = idx;
            hio.n_rows = n;
            hio.clip_range = io->clip_range;
            hio.vf_coef = io->vf_coef;
            hio.ent_coef = io->ent_coef;
            hio.grad_mean = grad_mean;
            hio.grad_v = critic ? grad_v : nullptr;
            hio.grad_log_std = (float*)io->opt.grad_log_std;
            hio.stats = st;
            HeadArgs ha{};
            head_args(actor, &hio, ha);
            HeadUpdate hu{};
            hu.v_old = io->clip_range_vf > 0.0f ? io->values_old : nullptr;
            hu.clip_vf = io->clip_range_vf;
            hu.ctl = o->ctl;
            hu.target_kl = io->target_kl;
            bias_corrections(o->beta1, o->beta2, io->opt.lr, t0 + 1 + k, hu.step_size, hu.rsq);
            rc = launch_ppo_head_update(ha, hu, stream);
            if (rc != 0) return launch_failed(h, "PPO head", rc);
            if ((rc = dockauv_policy_backward(h, actor, io->rows, idx, n, grad_mean, &ag, stream)) != 0) return rc;
            if (critic && (rc = dockauv_policy_backward(h, critic, io->rows, idx, n, grad_v, &cg, stream)) != 0) return rc;
            AdamArgs aa{};
            adam_args(o, &io->opt, st + 8, aa);
            rc = launch_adam_step_ctl(aa, o->ctl, stream);
            if (rc != 0) return launch_failed(h, "optimiser", rc);
            if ((rc = repack_policy(actor, io->opt.actor_params, io->opt.log_std, stream)) != 0) return rc;
            if (critic && (rc = repack_policy(critic, io->opt.critic_params, nullptr, stream)) != 0) return rc;
        }
    }
    h->last_stream = stream;
    if (io->target_kl > 0.0f) {
        o->pending = true;
        o->pending_stream = stream;
    } else {
        o->t = t0 + k;
    }
    return 0;
}

}  // extern "C"
