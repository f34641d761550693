// dockauv_capi_policy.hip -- C ABI of libdockauv.so (include/dockauv.h), the networks' part: the policy object (actor, value critic),
// its forward, rows, backward and rollout calls, and the PPO head.  The collector is in dockauv_capi_collect.hip, the optimiser in
// dockauv_capi_optim.hip, SAC in dockauv_capi_sac.hip; dockauv_capi_policy.h is what the four share.
// The kernels are in dockauv_policy / _backward / _head / _sac.hip.
#include "dockauv_capi_policy.h"

using namespace dockauv;

namespace dockauv {

int new_policy(dockauv_handle h, Role role, PolicyShape S, const char* desc_name, dockauv_policy* out) {
    policy_layout(S);
    if (policy_lds_bytes(S) > kPolMaxLds)
        return fail(h, DOCKAUV_E_INVALID, "%s: the padded weights (%zu B for n_in %d, n_hidden %d / %d) exceed "
                    "the 160 KiB of LDS the policy kernel keeps them in: narrower layers", desc_name, policy_lds_bytes(S), S.n_in, S.n_h1, S.n_h2);
    HIP_TRY(h, hipSetDevice(h->device));
    dockauv_policy p = new dockauv_policy_s();
    p->h = h;
    p->S = S;
    p->role = role;
    int len[6];
    const int n_last = layer_lengths(S, len);
    const size_t trunk = (size_t)len[0] + len[1] + len[2] + len[3];
    const bool sac = role == Role::SacActor;   // (the head array [kSacHeadRows][n_last] and its bias in place of W3 b3 log_std)
    const size_t raw_floats = trunk + (sac ? (size_t)kSacHeadRows * (n_last + 1) : (size_t)len[4] + 2 * (size_t)len[5]);
    hipError_t e = hipMalloc((void**)&p->packed, (size_t)S.total * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&p->raw, raw_floats * sizeof(float));
    if (e == hipSuccess && sac) e = hipMemset(p->raw, 0, raw_floats * sizeof(float));
    if (e == hipSuccess && !sac) e = hipMalloc((void**)&p->log_std, DOCKAUV_MAX_U * sizeof(float));
    if (e == hipSuccess && !sac) e = hipMemset(p->log_std, 0, DOCKAUV_MAX_U * sizeof(float));
    if (e != hipSuccess) {
        dockauv_policy_destroy(p);
        return fail(h, DOCKAUV_E_HIP, "policy buffers: %s", hipGetErrorString(e));
    }
    *out = p;
    return 0;
}

int upload_policy(dockauv_policy p, const dockauv_policy_desc* d, hipStream_t stream) {
    dockauv_handle h = p->h;
    const PolicyShape& S = p->S;
    int len[6];
    layer_lengths(S, len);
    const float* src[7] = {d->W1, d->b1, d->W2, d->b2, d->W3, d->b3, d->log_std};
    const size_t cnt[7] = {(size_t)len[0], (size_t)len[1], (size_t)len[2], (size_t)len[3], (size_t)len[4], (size_t)len[5], (size_t)S.n_out};
    const float* dev[7];
    if (d->pointers_on_device) {
        for (int i = 0; i < 7; ++i) dev[i] = src[i];
    } else {
        size_t off = 0;
        for (int i = 0; i < 7; ++i) {
            dev[i] = (src[i] && cnt[i] && !(i == 6 && is_critic(p->role))) ? p->raw + off : nullptr;
            if (dev[i]) HIP_TRY(h, hipMemcpyAsync(p->raw + off, src[i], cnt[i] * sizeof(float), hipMemcpyHostToDevice, stream));
            off += cnt[i];
        }
        HIP_TRY(h, hipStreamSynchronize(stream));   // the caller's host arrays are free on return
    }
    if (!S.n_h2) dev[2] = dev[3] = nullptr;
    if (is_critic(p->role)) dev[6] = nullptr;   // (a critic has no exploration noise)
    if (dev[6]) HIP_TRY(h, hipMemcpyAsync(p->log_std, dev[6], cnt[6] * sizeof(float), hipMemcpyDeviceToDevice, stream));
    const PolicyRaw raw{dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6]};
    const int rc = launch_policy_pack(S, raw, p->packed, stream);
    if (rc != 0) return launch_failed(h, "policy weight packing", rc);
    p->has_log_std = dev[6] != nullptr;
    p->seed = d->seed;
    p->env_id_offset = d->env_id_offset;
    return 0;
}

int policy_forward(dockauv_handle h, dockauv_policy p, const float* rows, float* actions, uint64_t t, int stochastic, hipStream_t stream,
                   float* log_prob) {
    if (p->role == Role::SacActor) {
        // the per-env form of the squashed-Gaussian actor: the plain actor's rows, counter and noise stream
        SacActorLaunch l{rows, nullptr, actions, log_prob, (long)h->cfg.n_envs, h->n_obs + 2, h->n_u_max, stochastic ? 1 : 0,
                         t, p->env_id_offset, p->seed, 2u};
        return launched(h, "SAC actor kernel", launch_sac_actor(p->S, p->packed, l, stream), stream);
    }
    const int rc = launch_policy_forward(p->S, p->packed, rows, actions, h->cfg.n_envs, h->n_obs + 2, h->n_u_max, t,
                                         (stochastic && p->has_log_std) ? 1 : 0, p->seed, p->env_id_offset, stream, log_prob,
                                         log_prob ? p->log_std : nullptr);
    return launched(h, "policy kernel", rc, stream);
}

// (the critic's kernel with one output unit and an action stride of 1)
int value_forward(dockauv_handle h, dockauv_policy c, const float* rows, long long n_rows, float* values, hipStream_t stream) {
    return launched(h, "value kernel", launch_policy_forward(c->S, c->packed, rows, values, (long)n_rows, h->n_obs + 2, 1, 0, 0, 0, 0, stream), stream);
}

int queue_rollout(dockauv_handle h, dockauv_policy p, const float* rows_in, float* rows_out, float* actions_out, float* terminal_obs,
                  float* log_prob, int n_steps, uint64_t t0, int stochastic, hipStream_t stream) {
    const size_t N = (size_t)h->cfg.n_envs, row = (size_t)h->n_obs + 2;
    for (int k = 0; k < n_steps; ++k) {
        const float* rows = k == 0 ? rows_in : rows_out + (size_t)(k - 1) * N * row;
        float* act = actions_out + (size_t)k * N * h->n_u_max;
        int rc = policy_forward(h, p, rows, act, t0 + (uint64_t)k, stochastic, stream, log_prob ? log_prob + (size_t)k * N : nullptr);
        if (rc) return rc;
        dockauv_step_io io{};
        io.actions = act;
        io.obs = rows_out + (size_t)k * N * row;
        io.terminal_obs = terminal_obs ? terminal_obs + (size_t)k * N * h->n_obs : nullptr;
        io.pack_reward_done = 1;
        if ((rc = launch(h, &io, stream)) != 0) return rc;
    }
    return 0;
}

void head_args(dockauv_policy actor, const dockauv_ppo_head_io* io, HeadArgs& a) {
    a.mean = io->mean;
    a.v = io->v;
    a.actions = io->actions;
    a.log_prob_old = io->log_prob_old;
    a.advantages = io->advantages;
    a.returns = io->returns;
    a.row_index = (const long long*)io->row_index;
    a.log_std = actor->log_std;
    a.grad_mean = io->grad_mean;
    a.grad_v = io->grad_v;
    a.grad_log_std = io->grad_log_std;
    a.stats = io->stats;
    a.moments = actor->head_ws;
    a.partial = actor->head_ws + (size_t)kBwdMaxGroups * kHeadMoments;
    a.n = (long)io->n_rows;
    a.n_out = actor->S.n_out;
    a.normalize = io->normalize_advantage ? 1 : 0;
    a.clip = io->clip_range;
    a.vf_coef = io->vf_coef;
    a.ent_coef = io->ent_coef;
}

}  // namespace dockauv

namespace {

const char* const kDesc = "dockauv_policy_desc";

// the descriptor's own fields; `like` != nullptr: a reload, shapes and activations must be those of the policy
int validate_policy_desc(dockauv_handle h, const dockauv_policy_desc* d, const PolicyShape* like) {
    if (int rc = validate_trunk_numbers(h, d, kDesc)) return rc;
    if (d->out_act != DOCKAUV_ACT_NONE && d->out_act != DOCKAUV_ACT_TANH)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.out_act: %d is neither DOCKAUV_ACT_NONE nor DOCKAUV_ACT_TANH", d->out_act);
    if (int rc = validate_trunk_arrays(h, d, kDesc)) return rc;
    if (int rc = require(h, kDesc, {{"W3", d->W3}, {"b3", d->b3}})) return rc;
    if (like && !(trunk_matches(d, *like) && d->out_act == like->out_act))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_load: n_in / n_hidden / n_out / activations differ from the policy's (%d-%d-%d-%d)",
                    like->n_in, like->n_h1, like->n_h2, like->n_out);
    return 0;
}

// actor (dockauv_policy_create), value critic (dockauv_value_create) or Q critic (dockauv_q_create): `fn` names the entry point
int create_policy(dockauv_handle h, const dockauv_policy_desc* d, dockauv_policy* out, Role role, const char* fn) {
    if (!d || !out) return fail(h, DOCKAUV_E_INVALID, "%s: null argument", fn);
    *out = nullptr;
    int rc = validate_policy_desc(h, d, nullptr);
    if (rc) return rc;
    if (is_critic(role) && d->n_out != 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.n_out: %d, a critic has one output", d->n_out);
    if (is_critic(role) && d->out_act != DOCKAUV_ACT_NONE)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.out_act: %d, a critic's output is raw (DOCKAUV_ACT_NONE)", d->out_act);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (h->f64) return fail(h, DOCKAUV_E_INVALID, "%s: the policy kernel is float32; the handle's precision is DOCKAUV_F64", fn);
    if (role == Role::Q && d->n_in != h->n_obs + h->n_u_max)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.n_in: %d, a Q critic reads [obs | action]: the handle's n_obs + n_u is %d + %d", d->n_in,
                    h->n_obs, h->n_u_max);
    if (role != Role::Q && d->n_in != h->n_obs) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.n_in: %d, the handle's n_obs is %d", d->n_in, h->n_obs);
    if (!is_critic(role) && d->n_out != h->n_u_max)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.n_out: %d, the handle's n_u is %d", d->n_out, h->n_u_max);
    PolicyShape S{};
    S.n_in = d->n_in;
    S.n_h1 = d->n_hidden[0];
    S.n_h2 = d->n_hidden[1];
    S.n_out = d->n_out;
    S.hidden_act = d->hidden_act;
    S.out_act = d->out_act;
    dockauv_policy p = nullptr;
    if ((rc = new_policy(h, role, S, kDesc, &p)) != 0) return rc;
    if ((rc = upload_policy(p, d, nullptr)) != 0) {
        dockauv_policy_destroy(p);
        return rc;
    }
    *out = p;
    return 0;
}

}  // namespace

extern "C" {

int dockauv_policy_create(dockauv_handle h, const dockauv_policy_desc* d, dockauv_policy* out) {
    return create_policy(h, d, out, Role::Actor, "dockauv_policy_create");
}

int dockauv_value_create(dockauv_handle h, const dockauv_policy_desc* d, dockauv_policy* out) {
    return create_policy(h, d, out, Role::Value, "dockauv_value_create");
}

int dockauv_q_create(dockauv_handle h, const dockauv_policy_desc* d, dockauv_policy* out) {
    return create_policy(h, d, out, Role::Q, "dockauv_q_create");
}

int dockauv_policy_load(dockauv_policy p, const dockauv_policy_desc* d, void* hip_stream) {
    if (!p) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_policy_load: null policy");
    if (!d) return fail(p->h, DOCKAUV_E_INVALID, "dockauv_policy_load: null descriptor");
    if (p->role == Role::SacActor)
        return fail(p->h, DOCKAUV_E_INVALID, "dockauv_policy_load: the policy is %s: its weights come through dockauv_sac_actor_load",
                    phrase(p->role).named);
    int rc = validate_policy_desc(p->h, d, &p->S);
    if (rc) return rc;
    HIP_TRY(p->h, hipSetDevice(p->h->device));
    return upload_policy(p, d, (hipStream_t)hip_stream);
}

int dockauv_policy_destroy(dockauv_policy p) {
    if (!p) return 0;
    if (p->h) (void)hipSetDevice(p->h->device);
    (void)hipDeviceSynchronize();
    if (p->packed) (void)hipFree(p->packed);
    if (p->raw) (void)hipFree(p->raw);
    if (p->log_std) (void)hipFree(p->log_std);
    if (p->bwd_partial) (void)hipFree(p->bwd_partial);
    if (p->head_ws) (void)hipFree(p->head_ws);
    delete p;
    return 0;
}

int dockauv_policy_forward(dockauv_handle h, dockauv_policy p, const float* rows, float* actions, uint64_t t, int stochastic,
                           void* hip_stream) {
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_policy_forward: null handle");
    if (!p) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_forward: null policy");
    if (int rc = check_actor(h, p, "dockauv_policy_forward", false, false)) return rc;
    if (!rows || !actions) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_forward: rows/actions must not be NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    return policy_forward(h, p, rows, actions, t, stochastic, (hipStream_t)hip_stream);
}

int dockauv_policy_forward_logp(dockauv_handle h, dockauv_policy p, const float* rows, float* actions, float* log_prob, uint64_t t,
                                int stochastic, void* hip_stream) {
    if (!rows || !actions || !log_prob) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_forward_logp: rows/actions/log_prob must not be NULL");
    if (!p) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_forward_logp: null policy");
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_policy_forward_logp: null handle");
    if (int rc = check_actor(h, p, "dockauv_policy_forward_logp", true, false)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return policy_forward(h, p, rows, actions, t, stochastic, (hipStream_t)hip_stream, log_prob);
}

int dockauv_value_forward(dockauv_handle h, dockauv_policy critic, const float* rows, long long n_rows, float* values, void* hip_stream) {
    if (!rows || !values) return fail(h, DOCKAUV_E_INVALID, "dockauv_value_forward: rows/values must not be NULL");
    if (n_rows < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_value_forward: n_rows %lld must be >= 1", n_rows);
    if (!critic) return fail(h, DOCKAUV_E_INVALID, "dockauv_value_forward: null critic");
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_value_forward: null handle");
    if (int rc = check_critic(h, critic, "dockauv_value_forward")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return value_forward(h, critic, rows, n_rows, values, (hipStream_t)hip_stream);
}

int dockauv_policy_forward_rows(dockauv_handle h, dockauv_policy p, const float* rows, const int64_t* row_index, long long n_rows,
                                float* out, void* hip_stream) {
    if (!rows || !out) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_forward_rows: rows/out must not be NULL");
    if (n_rows < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_forward_rows: n_rows %lld must be >= 1", n_rows);
    if (!p) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_forward_rows: null policy");
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_policy_forward_rows: null handle");
    if (p->h != h) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_forward_rows: the policy was created for another handle");
    if (int rc = refuse_sac(h, p, "dockauv_policy_forward_rows")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const int rc = launch_policy_forward_rows(p->S, p->packed, rows, (const long long*)row_index, (long)n_rows, h->n_obs + 2, out,
                                              (hipStream_t)hip_stream);
    return launched(h, "policy rows kernel", rc, hip_stream);
}

int dockauv_policy_backward(dockauv_handle h, dockauv_policy p, const float* rows, const int64_t* row_index, long long n_rows,
                            const float* grad_out, const dockauv_policy_grads* grads, void* hip_stream) {
    const char* fn = "dockauv_policy_backward";
    if (!rows || !grad_out || !grads) return fail(h, DOCKAUV_E_INVALID, "%s: rows/grad_out/grads must not be NULL", fn);
    if (int rc = check_size(h, grads, "dockauv_policy_grads")) return rc;
    if (!grads->dW1 || !grads->db1 || !grads->dW3 || !grads->db3)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_grads: dW1/db1/dW3/db3 must not be NULL");
    if (n_rows < 1) return fail(h, DOCKAUV_E_INVALID, "%s: n_rows %lld must be >= 1", fn, n_rows);
    if (!p) return fail(h, DOCKAUV_E_INVALID, "%s: null policy", fn);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (p->h != h) return fail(h, DOCKAUV_E_INVALID, "%s: the policy was created for another handle", fn);
    if (int rc = refuse_sac(h, p, fn)) return rc;
    if (p->S.n_h2 > 0 && (!grads->dW2 || !grads->db2))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_grads: dW2/db2 are NULL, the policy has two hidden layers");
    BackwardLayout L;
    backward_layout(p->S, L);
    if (int rc = check_backward_lds(h, p, L, fn)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (!p->bwd_partial) HIP_TRY(h, hipMalloc((void**)&p->bwd_partial, (size_t)kBwdMaxGroups * L.n_params * sizeof(float)));
    const PolicyGrads g{grads->dW1, grads->db1, p->S.n_h2 ? grads->dW2 : nullptr, p->S.n_h2 ? grads->db2 : nullptr, grads->dW3, grads->db3};
    const int rc = launch_policy_backward(p->S, p->packed, rows, (const long long*)row_index, (long)n_rows, h->n_obs + 2, grad_out,
                                          p->bwd_partial, g, (hipStream_t)hip_stream);
    return launched(h, "policy backward", rc, hip_stream);
}

int dockauv_policy_backward_workspace(dockauv_policy p, float** partial, long long* n_floats) {
    if (!p) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_policy_backward_workspace: null policy");
    BackwardLayout L;                                   // (the role fixes the partial's size)
    if (p->role == Role::SacActor) sac_actor_backward_layout(p->S, L);
    else backward_layout(p->S, L);
    if (partial) *partial = p->bwd_partial;
    if (n_floats) *n_floats = p->bwd_partial ? (long long)kBwdMaxGroups * L.n_params : 0;
    return 0;
}

int dockauv_ppo_head(dockauv_handle h, dockauv_policy actor, const dockauv_ppo_head_io* io, void* hip_stream) {
    const char* io_name = "dockauv_ppo_head_io";
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_ppo_head: null handle");
    if (!actor) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head: null actor");
    if (int rc = check_block(h, io, "dockauv_ppo_head", "io", io_name)) return rc;
    if (int rc = check_actor(h, actor, "dockauv_ppo_head", true)) return rc;
    if (io->n_rows < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head_io.n_rows: %lld must be >= 1", io->n_rows);
    if (io->normalize_advantage && io->n_rows < 2)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head_io.n_rows: %lld must be >= 2 with normalize_advantage (the unbiased deviation)", io->n_rows);
    if (!(io->clip_range > 0.0f)) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head_io.clip_range: %g must be > 0", (double)io->clip_range);
    if (int rc = require(h, io_name, {{"mean", io->mean}, {"actions", io->actions}, {"log_prob_old", io->log_prob_old},
                                      {"advantages", io->advantages}, {"grad_mean", io->grad_mean}, {"grad_log_std", io->grad_log_std},
                                      {"stats", io->stats}}))
        return rc;
    if ((io->v == nullptr) != (io->grad_v == nullptr))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head_io.v / grad_v: both or neither must be NULL (NULL: no critic)");
    if (io->v && !io->returns) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head_io.returns is NULL (v is given)");
    HIP_TRY(h, hipSetDevice(h->device));
    if (!actor->head_ws) HIP_TRY(h, hipMalloc((void**)&actor->head_ws, kHeadWorkspaceBytes));
    HeadArgs a{};
    head_args(actor, io, a);
    return launched(h, "PPO head", launch_ppo_head(a, hip_stream), hip_stream);
}

int dockauv_rollout(dockauv_handle h, dockauv_policy p, const float* rows_in, float* rows_out, float* actions_out,
                    float* terminal_obs, int n_steps, uint64_t t0, int stochastic, void* hip_stream) {
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_rollout: null handle");
    if (!p) return fail(h, DOCKAUV_E_INVALID, "dockauv_rollout: null policy");
    if (int rc = check_actor(h, p, "dockauv_rollout", false, false)) return rc;
    if (n_steps < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_rollout: n_steps %d must be >= 1", n_steps);
    if (!rows_in || !rows_out || !actions_out) return fail(h, DOCKAUV_E_INVALID, "dockauv_rollout: rows_in/rows_out/actions_out must not be NULL");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = queue_rollout(h, p, rows_in, rows_out, actions_out, terminal_obs, nullptr, n_steps, t0, stochastic, (hipStream_t)hip_stream))
        return rc;
    return check_status(h);   // (what dockauv_poll_status looks at: no synchronisation)
}

}  // extern "C"
