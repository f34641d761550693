// dockauv_capi_sac.hip -- C ABI of libdockauv.so (include/dockauv.h), SAC's part: the squashed-Gaussian actor object, the Q critics'
// forward and the TD target; the two networks' gradients; the loss head and the learned entropy coefficient.  (dockauv_q_create is
// with the other dockauv_policy_desc objects in dockauv_capi_policy.hip.)
// The kernels are in dockauv_sac / _backward / _sac_head.hip.
#include "dockauv_capi_policy.h"

using namespace dockauv;

namespace {

const char* const kDesc = "dockauv_sac_actor_desc";

int validate_sac_desc(dockauv_handle h, const dockauv_sac_actor_desc* d, const PolicyShape* like) {
    if (int rc = validate_trunk_numbers(h, d, kDesc)) return rc;
    if (int rc = validate_trunk_arrays(h, d, kDesc)) return rc;
    if (int rc = require(h, kDesc, {{"W_mu", d->W_mu}, {"b_mu", d->b_mu}, {"W_ls", d->W_ls}, {"b_ls", d->b_ls}})) return rc;
    if (like && !trunk_matches(d, *like))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_load: n_in / n_hidden / n_out / hidden_act differ from the actor's (%d-%d-%d-%d)",
                    like->n_in, like->n_h1, like->n_h2, like->n_out);
    return 0;
}

// p->raw of a squashed-Gaussian actor: W1 b1 W2 b2, then the head array [16][n_last] and its bias [16] (rows 0 .. n_u - 1: mu,
// rows 8 .. 8 + n_u - 1: log_std, the rest zero since create).  Both heads are always copied there, host or device arrays.
int upload_sac_actor(dockauv_policy p, const dockauv_sac_actor_desc* d, hipStream_t stream) {
    dockauv_handle h = p->h;
    const PolicyShape& S = p->S;
    int len[6];
    const int n_last = layer_lengths(S, len);
    const hipMemcpyKind kind = d->pointers_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const float* src[4] = {d->W1, d->b1, d->W2, d->b2};
    const float* dev[4];
    size_t off = 0;
    for (int i = 0; i < 4; ++i) {
        dev[i] = len[i] ? (d->pointers_on_device ? src[i] : p->raw + off) : nullptr;
        if (len[i] && !d->pointers_on_device) HIP_TRY(h, hipMemcpyAsync(p->raw + off, src[i], (size_t)len[i] * sizeof(float), kind, stream));
        off += (size_t)len[i];
    }
    float* heads = p->raw + off;
    float* head_b = heads + (size_t)kSacHeadRows * n_last;
    HIP_TRY(h, hipMemcpyAsync(heads, d->W_mu, (size_t)len[4] * sizeof(float), kind, stream));
    HIP_TRY(h, hipMemcpyAsync(heads + (size_t)8 * n_last, d->W_ls, (size_t)len[4] * sizeof(float), kind, stream));
    HIP_TRY(h, hipMemcpyAsync(head_b, d->b_mu, (size_t)len[5] * sizeof(float), kind, stream));
    HIP_TRY(h, hipMemcpyAsync(head_b + 8, d->b_ls, (size_t)len[5] * sizeof(float), kind, stream));
    if (!d->pointers_on_device) HIP_TRY(h, hipStreamSynchronize(stream));   // the caller's host arrays are free on return
    PolicyShape both = S;
    both.n_out = 8 + S.n_out;              // (the layout does not depend on n_out: the pack kernel's bound on the output units)
    const PolicyRaw raw{dev[0], dev[1], dev[2], dev[3], heads, head_b, nullptr};
    const int rc = launch_policy_pack(both, raw, p->packed, stream);
    if (rc != 0) return launch_failed(h, "policy weight packing", rc);
    p->has_log_std = true;
    p->seed = d->seed;
    p->env_id_offset = d->env_id_offset;
    return 0;
}

// do the float arrays [a, a + na) and [b, b + nb) share a byte?
bool floats_overlap(const float* a, long long na, const float* b, long long nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb * sizeof(float) && b0 < a0 + (uintptr_t)na * sizeof(float);
}

struct FloatSpan {
    const char* name;
    const float* p;
    long long n;
};

// every output against every input and against the outputs behind it; the first pair that overlaps is named
int refuse_overlap(dockauv_handle h, const char* io_name, const FloatSpan* out, int n_out, const FloatSpan* in, int n_in) {
    for (int i = 0; i < n_out; ++i) {
        for (int k = 0; k < n_in; ++k)
            if (in[k].p && floats_overlap(out[i].p, out[i].n, in[k].p, in[k].n))
                return fail(h, DOCKAUV_E_INVALID, "%s.%s overlaps %s: outputs must not alias inputs", io_name, out[i].name, in[k].name);
        for (int k = i + 1; k < n_out; ++k)
            if (floats_overlap(out[i].p, out[i].n, out[k].p, out[k].n))
                return fail(h, DOCKAUV_E_INVALID, "%s.%s overlaps %s: outputs must not alias one another", io_name, out[i].name, out[k].name);
    }
    return 0;
}

// the actor head's arrays for n_u actions a row (n_u = 1 before the handle is known: every array is at least that long)
int refuse_actor_head_overlap(dockauv_handle h, const dockauv_sac_actor_head_io* io, int n_u) {
    const long long B = io->n_rows;
    const FloatSpan out[2] = {{"grad_out", io->grad_out, 2 * B * n_u}, {"stats", io->stats, 4}};
    const FloatSpan in[6] = {{"heads", io->heads, 2 * B * n_u}, {"q1_pi", io->q1_pi, B}, {"q2_pi", io->q2_pi, B}, {"dq1", io->dq1, B * n_u},
                             {"dq2", io->dq2, B * n_u}, {"log_ent_coef", io->log_ent_coef, 1}};
    return refuse_overlap(h, "dockauv_sac_actor_head_io", out, 2, in, 6);
}

// what every io block of SAC's calls starts with: the block, its size, n_rows
template <class T>
int check_rows_io(dockauv_handle h, const T* io, const char* fn, const char* io_name) {
    if (int rc = check_block(h, io, fn, "io", io_name)) return rc;
    if (io->n_rows < 1) return fail(h, DOCKAUV_E_INVALID, "%s.n_rows: %lld must be >= 1", io_name, io->n_rows);
    return 0;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------------------ the forward half (dockauv_sac.hip)

int dockauv_sac_actor_create(dockauv_handle h, const dockauv_sac_actor_desc* d, dockauv_policy* out) {
    const char* fn = "dockauv_sac_actor_create";
    if (!d || !out) return fail(h, DOCKAUV_E_INVALID, "%s: null argument", fn);
    *out = nullptr;
    if (int rc = validate_sac_desc(h, d, nullptr)) return rc;
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (h->f64) return fail(h, DOCKAUV_E_INVALID, "%s: the policy kernel is float32; the handle's precision is DOCKAUV_F64", fn);
    if (d->n_in != h->n_obs) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc.n_in: %d, the handle's n_obs is %d", d->n_in, h->n_obs);
    if (d->n_out != h->n_u_max) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc.n_out: %d, the handle's n_u is %d", d->n_out, h->n_u_max);
    PolicyShape S{};
    S.n_in = d->n_in;
    S.n_h1 = d->n_hidden[0];
    S.n_h2 = d->n_hidden[1];
    S.n_out = d->n_out;
    S.hidden_act = d->hidden_act;
    S.out_act = DOCKAUV_ACT_TANH;
    dockauv_policy p = nullptr;
    if (int rc = new_policy(h, Role::SacActor, S, kDesc, &p)) return rc;
    if (int rc = upload_sac_actor(p, d, nullptr)) {
        dockauv_policy_destroy(p);
        return rc;
    }
    *out = p;
    return 0;
}

int dockauv_sac_actor_load(dockauv_policy p, const dockauv_sac_actor_desc* d, void* hip_stream) {
    if (!p) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_sac_actor_load: null policy");
    if (!d) return fail(p->h, DOCKAUV_E_INVALID, "dockauv_sac_actor_load: null descriptor");
    if (p->role != Role::SacActor)
        return fail(p->h, DOCKAUV_E_INVALID, "dockauv_sac_actor_load: the policy is not %s", phrase(Role::SacActor).named);
    if (int rc = validate_sac_desc(p->h, d, &p->S)) return rc;
    HIP_TRY(p->h, hipSetDevice(p->h->device));
    return upload_sac_actor(p, d, (hipStream_t)hip_stream);
}

int dockauv_q_forward(dockauv_handle h, dockauv_policy critic, const dockauv_q_io* io, void* hip_stream) {
    const char* fn = "dockauv_q_forward";
    const char* io_name = "dockauv_q_io";
    if (int rc = check_rows_io(h, io, fn, io_name)) return rc;
    if (int rc = require(h, io_name, {{"obs", io->obs}, {"actions", io->actions}, {"q", io->q}})) return rc;
    if (!critic) return fail(h, DOCKAUV_E_INVALID, "%s: null critic", fn);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (int rc = check_is(h, critic, fn, "the critic", Role::Q)) return rc;
    if (io->obs_stride < h->n_obs) return fail(h, DOCKAUV_E_INVALID, "dockauv_q_io.obs_stride: %d is below the handle's n_obs %d", io->obs_stride, h->n_obs);
    if (io->act_stride < h->n_u_max) return fail(h, DOCKAUV_E_INVALID, "dockauv_q_io.act_stride: %d is below the handle's n_u %d", io->act_stride, h->n_u_max);
    HIP_TRY(h, hipSetDevice(h->device));
    const QLaunch l{io->obs, io->actions, (const long long*)io->row_index, (const long long*)io->row_index, io->q, (long)io->n_rows,
                    io->obs_stride, io->act_stride, h->n_obs};
    return launched(h, "Q kernel", launch_q_forward(critic->S, critic->packed, l, hip_stream), hip_stream);
}

int dockauv_sac_target(dockauv_handle h, dockauv_policy actor, dockauv_policy q1_target, dockauv_policy q2_target,
                       const dockauv_sac_target_io* io, void* hip_stream) {
    const char* fn = "dockauv_sac_target";
    const char* io_name = "dockauv_sac_target_io";
    if (int rc = check_rows_io(h, io, fn, io_name)) return rc;
    if (!(io->gamma >= 0.0f && io->gamma <= 1.0f)) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_target_io.gamma: %g outside [0, 1]", (double)io->gamma);
    if (!io->log_ent_coef && std::isnan(io->ent_coef)) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_target_io.ent_coef is NaN (and log_ent_coef is NULL)");
    if (int rc = require(h, io_name, {{"next_obs", io->next_obs}, {"rewards", io->rewards}, {"dones", io->dones}, {"a2", io->a2},
                                      {"logp2", io->logp2}, {"q1", io->q1}, {"q2", io->q2}, {"y", io->y}}))
        return rc;
    if (io->column_stride < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_target_io.column_stride: %d must be >= 1", io->column_stride);
    if (!actor) return fail(h, DOCKAUV_E_INVALID, "%s: null actor", fn);
    if (!q1_target || !q2_target) return fail(h, DOCKAUV_E_INVALID, "%s: null critic", fn);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (int rc = check_is(h, actor, fn, "the actor", Role::SacActor)) return rc;
    if (int rc = check_is(h, q1_target, fn, "q1_target", Role::Q)) return rc;
    if (int rc = check_is(h, q2_target, fn, "q2_target", Role::Q)) return rc;
    if (io->next_obs_stride < h->n_obs)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_target_io.next_obs_stride: %d is below the handle's n_obs %d", io->next_obs_stride, h->n_obs);
    HIP_TRY(h, hipSetDevice(h->device));
    const long n = (long)io->n_rows;
    const long long* index = (const long long*)io->row_index;
    const int n_u = h->n_u_max;
    const SacActorLaunch al{io->next_obs, index, io->a2, io->logp2, n, io->next_obs_stride, n_u, 1, io->t, io->row_offset, actor->seed, 5u};
    int rc = launch_sac_actor(actor->S, actor->packed, al, hip_stream);
    if (rc != 0) return launch_failed(h, "SAC actor kernel", rc);
    float* q_out[2] = {io->q1, io->q2};
    dockauv_policy qs[2] = {q1_target, q2_target};
    for (int i = 0; i < 2; ++i) {
        const QLaunch ql{io->next_obs, io->a2, index, nullptr, q_out[i], n, io->next_obs_stride, n_u, h->n_obs};
        if ((rc = launch_q_forward(qs[i]->S, qs[i]->packed, ql, hip_stream)) != 0) return launch_failed(h, "Q kernel", rc);
    }
    const SacTargetLaunch tl{io->rewards, io->dones, io->timeouts, index, io->logp2, io->q1, io->q2, io->log_ent_coef, io->y, n,
                             io->column_stride, io->gamma, io->ent_coef};
    return launched(h, "SAC target kernel", launch_sac_target_rows(tl, hip_stream), hip_stream);
}

// ------------------------------------------------------------------------------------------ the networks' gradients (dockauv_backward.hip)

int dockauv_sac_actor_forward_rows(dockauv_handle h, dockauv_policy actor, const dockauv_sac_rows_io* io, void* hip_stream) {
    const char* fn = "dockauv_sac_actor_forward_rows";
    const char* io_name = "dockauv_sac_rows_io";
    if (int rc = check_rows_io(h, io, fn, io_name)) return rc;
    if (io->row_stride < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_rows_io.row_stride: %d is below every row width", io->row_stride);
    if (int rc = require(h, io_name, {{"rows", io->rows}, {"out", io->out}})) return rc;
    if (!actor) return fail(h, DOCKAUV_E_INVALID, "%s: null actor", fn);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (int rc = check_role(h, actor, fn, Role::SacActor)) return rc;
    if (io->row_stride < h->n_obs) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_rows_io.row_stride: %d is below the handle's n_obs %d", io->row_stride, h->n_obs);
    HIP_TRY(h, hipSetDevice(h->device));
    const int rc = launch_sac_actor_heads(actor->S, actor->packed, io->rows, (const long long*)io->row_index, (long)io->n_rows, io->row_stride,
                                          io->out, hip_stream);
    return launched(h, "SAC actor heads kernel", rc, hip_stream);
}

int dockauv_sac_actor_backward(dockauv_handle h, dockauv_policy actor, const dockauv_sac_actor_backward_io* io, void* hip_stream) {
    const char* fn = "dockauv_sac_actor_backward";
    const char* io_name = "dockauv_sac_actor_backward_io";
    if (int rc = check_rows_io(h, io, fn, io_name)) return rc;
    if (io->row_stride < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_backward_io.row_stride: %d is below every row width", io->row_stride);
    if (int rc = require(h, io_name, {{"rows", io->rows}, {"grad_out", io->grad_out}, {"dW1", io->dW1}, {"db1", io->db1}, {"dW_mu", io->dW_mu},
                                      {"db_mu", io->db_mu}, {"dW_ls", io->dW_ls}, {"db_ls", io->db_ls}}))
        return rc;
    if (!actor) return fail(h, DOCKAUV_E_INVALID, "%s: null actor", fn);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (int rc = check_role(h, actor, fn, Role::SacActor)) return rc;
    if (io->row_stride < h->n_obs)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_backward_io.row_stride: %d is below the handle's n_obs %d", io->row_stride, h->n_obs);
    if (actor->S.n_h2 > 0 && !io->dW2) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_backward_io.dW2 is NULL, the actor has two hidden layers");
    if (actor->S.n_h2 > 0 && !io->db2) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_backward_io.db2 is NULL, the actor has two hidden layers");
    BackwardLayout L;
    sac_actor_backward_layout(actor->S, L);
    if (int rc = check_backward_lds(h, actor, L, fn)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (!actor->bwd_partial) HIP_TRY(h, hipMalloc((void**)&actor->bwd_partial, (size_t)kBwdMaxGroups * L.n_params * sizeof(float)));
    const bool two = actor->S.n_h2 > 0;
    const SacActorGrads g{io->dW1, io->db1, two ? io->dW2 : nullptr, two ? io->db2 : nullptr, io->dW_mu, io->db_mu, io->dW_ls, io->db_ls};
    const SacBackwardLaunch l{io->rows, nullptr, (const long long*)io->row_index, io->grad_out, nullptr, (long)io->n_rows, io->row_stride, 0,
                              actor->S.n_in};
    return launched(h, "SAC actor backward", launch_sac_actor_backward(actor->S, actor->packed, l, actor->bwd_partial, g, hip_stream), hip_stream);
}

int dockauv_q_backward(dockauv_handle h, dockauv_policy critic, const dockauv_q_backward_io* io, void* hip_stream) {
    const char* fn = "dockauv_q_backward";
    const char* io_name = "dockauv_q_backward_io";
    if (int rc = check_rows_io(h, io, fn, io_name)) return rc;
    if (io->obs_stride < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_q_backward_io.obs_stride: %d is below every row width", io->obs_stride);
    if (io->act_stride < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_q_backward_io.act_stride: %d is below every row width", io->act_stride);
    if (int rc = require(h, io_name, {{"obs", io->obs}, {"actions", io->actions}, {"grad_q", io->grad_q}})) return rc;
    if (!io->grads && !io->grad_actions)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_q_backward_io: grads and grad_actions are both NULL, at least one output is required");
    const dockauv_policy_grads* gr = io->grads;
    if (gr)
        if (int rc = check_size(h, gr, "dockauv_policy_grads")) return rc;
    if (gr && (!gr->dW1 || !gr->db1 || !gr->dW3 || !gr->db3))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_grads: dW1/db1/dW3/db3 must not be NULL");
    if (!critic) return fail(h, DOCKAUV_E_INVALID, "%s: null critic", fn);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (int rc = check_role(h, critic, fn, Role::Q)) return rc;
    if (io->obs_stride < h->n_obs) return fail(h, DOCKAUV_E_INVALID, "dockauv_q_backward_io.obs_stride: %d is below the handle's n_obs %d", io->obs_stride, h->n_obs);
    if (io->act_stride < h->n_u_max) return fail(h, DOCKAUV_E_INVALID, "dockauv_q_backward_io.act_stride: %d is below the handle's n_u %d", io->act_stride, h->n_u_max);
    if (gr && critic->S.n_h2 > 0 && (!gr->dW2 || !gr->db2))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_grads: dW2/db2 are NULL, the critic has two hidden layers");
    BackwardLayout L;
    backward_layout(critic->S, L);
    if (int rc = check_backward_lds(h, critic, L, fn)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (gr && !critic->bwd_partial) HIP_TRY(h, hipMalloc((void**)&critic->bwd_partial, (size_t)kBwdMaxGroups * L.n_params * sizeof(float)));
    const bool two = critic->S.n_h2 > 0;
    PolicyGrads g{};
    if (gr) g = PolicyGrads{gr->dW1, gr->db1, two ? gr->dW2 : nullptr, two ? gr->db2 : nullptr, gr->dW3, gr->db3};
    const SacBackwardLaunch l{io->obs, io->actions, (const long long*)io->row_index, io->grad_q, io->grad_actions, (long)io->n_rows,
                              io->obs_stride, io->act_stride, h->n_obs};
    const int rc = launch_q_backward(critic->S, critic->packed, l, gr ? critic->bwd_partial : nullptr, gr ? &g : nullptr, hip_stream);
    return launched(h, "Q backward", rc, hip_stream);
}

// ------------------------------------------------------------------------------------------ the loss head (dockauv_sac_head.hip)

int dockauv_sac_sample(dockauv_handle h, dockauv_policy actor, const dockauv_sac_sample_io* io, void* hip_stream) {
    const char* fn = "dockauv_sac_sample";
    const char* io_name = "dockauv_sac_sample_io";
    if (int rc = check_rows_io(h, io, fn, io_name)) return rc;
    if (int rc = require(h, io_name, {{"heads", io->heads}, {"a", io->a}, {"logp", io->logp}})) return rc;
    if (!actor) return fail(h, DOCKAUV_E_INVALID, "%s: null actor", fn);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (int rc = check_role(h, actor, fn, Role::SacActor)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const SacSampleLaunch l{io->heads, io->a, io->logp, (long)io->n_rows, actor->S.n_out, (unsigned int)(io->t & 0xffffffffull),
                            (unsigned int)(io->row_offset & 0xffffffffull), actor->seed};
    return launched(h, "SAC sample kernel", launch_sac_sample(l, hip_stream), hip_stream);
}

int dockauv_sac_critic_head(dockauv_handle h, dockauv_policy q1_critic, const dockauv_sac_critic_head_io* io, void* hip_stream) {
    const char* fn = "dockauv_sac_critic_head";
    const char* io_name = "dockauv_sac_critic_head_io";
    if (int rc = check_rows_io(h, io, fn, io_name)) return rc;
    if (int rc = require(h, io_name, {{"q1", io->q1}, {"q2", io->q2}, {"y", io->y}, {"grad_q1", io->grad_q1}, {"grad_q2", io->grad_q2},
                                      {"stats", io->stats}}))
        return rc;
    const long long B = io->n_rows;
    const FloatSpan out[3] = {{"grad_q1", io->grad_q1, B}, {"grad_q2", io->grad_q2, B}, {"stats", io->stats, 6}};
    const FloatSpan in[3] = {{"q1", io->q1, B}, {"q2", io->q2, B}, {"y", io->y, B}};
    if (int rc = refuse_overlap(h, io_name, out, 3, in, 3)) return rc;
    if (!q1_critic) return fail(h, DOCKAUV_E_INVALID, "%s: null critic", fn);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (int rc = check_role(h, q1_critic, fn, Role::Q)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const SacCriticHeadLaunch l{io->q1, io->q2, io->y, io->grad_q1, io->grad_q2, io->stats, (long)B};
    return launched(h, "SAC critic head kernel", launch_sac_critic_head(l, hip_stream), hip_stream);
}

int dockauv_sac_actor_head(dockauv_handle h, dockauv_policy actor, const dockauv_sac_actor_head_io* io, void* hip_stream) {
    const char* fn = "dockauv_sac_actor_head";
    const char* io_name = "dockauv_sac_actor_head_io";
    if (int rc = check_rows_io(h, io, fn, io_name)) return rc;
    if (!io->log_ent_coef && std::isnan(io->ent_coef))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_head_io.ent_coef is NaN (and log_ent_coef is NULL)");
    if (int rc = require(h, io_name, {{"heads", io->heads}, {"q1_pi", io->q1_pi}, {"q2_pi", io->q2_pi}, {"dq1", io->dq1}, {"dq2", io->dq2},
                                      {"grad_out", io->grad_out}, {"stats", io->stats}}))
        return rc;
    if (int rc = refuse_actor_head_overlap(h, io, 1)) return rc;
    if (!actor) return fail(h, DOCKAUV_E_INVALID, "%s: null actor", fn);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (int rc = check_role(h, actor, fn, Role::SacActor)) return rc;
    if (int rc = refuse_actor_head_overlap(h, io, actor->S.n_out)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const SacActorHeadLaunch l{io->heads, io->q1_pi, io->q2_pi, io->dq1, io->dq2, io->log_ent_coef, io->grad_out, io->stats, (long)io->n_rows,
                               actor->S.n_out, (unsigned int)(io->t & 0xffffffffull), (unsigned int)(io->row_offset & 0xffffffffull),
                               actor->seed, io->ent_coef};
    return launched(h, "SAC actor head kernel", launch_sac_actor_head(l, hip_stream), hip_stream);
}

int dockauv_sac_ent_coef_step(dockauv_handle h, const dockauv_sac_ent_coef_io* io, void* hip_stream) {
    const char* fn = "dockauv_sac_ent_coef_step";
    const char* io_name = "dockauv_sac_ent_coef_io";
    if (int rc = check_rows_io(h, io, fn, io_name)) return rc;
    if (io->step < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_ent_coef_io.step: %lld must be >= 1 (the caller's count of this step)", io->step);
    if (!(io->lr >= 0.0) || !std::isfinite(io->lr)) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_ent_coef_io.lr: %g must be finite and >= 0", io->lr);
    if (!(io->beta1 >= 0.0 && io->beta1 < 1.0)) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_ent_coef_io.beta1: %g outside [0, 1)", io->beta1);
    if (!(io->beta2 >= 0.0 && io->beta2 < 1.0)) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_ent_coef_io.beta2: %g outside [0, 1)", io->beta2);
    if (!(io->eps > 0.0)) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_ent_coef_io.eps: %g must be > 0", io->eps);
    if (int rc = require(h, io_name, {{"state", io->state}, {"logp", io->logp}})) return rc;
    if (io->before && floats_overlap(io->before, 1, io->state, 3))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_ent_coef_io.before overlaps state: it receives the value from before the step");
    if (io->stats && floats_overlap(io->stats, 4, io->state, 3)) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_ent_coef_io.stats overlaps state");
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    HIP_TRY(h, hipSetDevice(h->device));
    EntCoefLaunch l{io->state, io->logp, io->before, io->stats, (long)io->n_rows, io->target_entropy};
    l.c1 = (float)(1.0 - io->beta1);
    l.c2 = (float)(1.0 - io->beta2);
    l.b2 = (float)io->beta2;
    bias_corrections(io->beta1, io->beta2, io->lr, io->step, l.step_size, l.rsq);
    l.eps = (float)io->eps;
    return launched(h, "ent_coef step kernel", launch_ent_coef_step(l, hip_stream), hip_stream);
}

}  // extern "C"
