// dockauv_capi_policy.hip -- C ABI of libdockauv.so (include/dockauv.h), second part: MLP policy and critic, closed-loop
// rollout, PPO collector, backward, head, optimiser, episode monitor and reward normaliser, and (at the end) SAC's forward half, its networks' gradients and its loss head.
// The kernels are in dockauv_policy / _collect / _backward / _head / _optim / _monitor / _update / _rewnorm / _sac / _sac_head.hip.
#include <cmath>
#include <cstring>

#include "dockauv_capi.h"

using namespace dockauv;

struct dockauv_policy_s {
    dockauv_handle h = nullptr;
    PolicyShape S{};
    float* packed = nullptr;      // the weights as the kernel reads them (dockauv_device.h: PolicyShape)
    float* raw = nullptr;         // device staging of host arrays: W1 b1 W2 b2 W3 b3 log_std back to back
    float* log_std = nullptr;     // the raw log_std [DOCKAUV_MAX_U] (the packed image keeps exp(log_std)): read by the log-prob epilogue
    bool has_log_std = false;
    bool value_role = false;      // a critic (dockauv_value_create): n_out == 1, raw output
    bool sac_role = false;        // a squashed-Gaussian actor (dockauv_sac_actor_create): both heads in the output tile, out_act TANH
    bool q_role = false;          // a Q critic (dockauv_q_create): n_in == n_obs + n_u, n_out == 1, raw output
    uint64_t seed = 0, env_id_offset = 0;
    float* bwd_partial = nullptr; // dockauv_policy_backward's per-group partial sums, allocated by the first backward
    double* head_ws = nullptr;    // dockauv_ppo_head's moment and row-sum partials (kHeadWorkspaceBytes), allocated by the first head call
};

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

struct dockauv_monitor_s {
    dockauv_handle h = nullptr;
    float* carry_ret = nullptr;   // [n_envs]: the running return of every env's episode
    int32_t* carry_len = nullptr; // [n_envs]: its length so far
    double* ws = nullptr;         // monitor_workspace_doubles(n_envs): the scan's partials, then the explained variance's
};

struct dockauv_rewnorm_s {
    dockauv_handle h = nullptr;
    float gamma = 0.0f, clip_reward = 0.0f;
    double epsilon = 0.0;
    float* carry = nullptr;       // [n_envs]: the discounted return of every env
    double* state = nullptr;      // [4]: running mean, var, count, reserved
};

namespace {

// the carries <- the handle's own cumulative reward / step counters (float32 handle), ordered on `stream`
int monitor_sync(dockauv_monitor m, hipStream_t stream) {
    dockauv_handle h = m->h;
    const size_t N = (size_t)h->cfg.n_envs;
    HIP_TRY(h, hipMemcpyAsync(m->carry_ret, h->B.cum_reward, N * sizeof(float), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(h, hipMemcpyAsync(m->carry_len, h->B.t_steps, N * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
    h->last_stream = stream;
    return 0;
}

// the descriptor's own fields; `like` != nullptr: a reload, shapes and activations must be those of the policy
int validate_policy_desc(dockauv_handle h, const dockauv_policy_desc* d, const PolicyShape* like) {
    if (d->struct_size != sizeof(dockauv_policy_desc))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.struct_size: got %u, library has %zu", d->struct_size, sizeof(dockauv_policy_desc));
    if (d->precision != DOCKAUV_F32) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.precision: %d, only DOCKAUV_F32 is implemented", d->precision);
    if (d->n_in < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.n_in: %d must be >= 1", d->n_in);
    if (d->n_hidden[0] < 1 || d->n_hidden[0] > DOCKAUV_POLICY_MAX_WIDTH)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.n_hidden[0]: %d outside 1..%d", d->n_hidden[0], DOCKAUV_POLICY_MAX_WIDTH);
    if (d->n_hidden[1] < 0 || d->n_hidden[1] > DOCKAUV_POLICY_MAX_WIDTH)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.n_hidden[1]: %d outside 0..%d (0 = one hidden layer)", d->n_hidden[1], DOCKAUV_POLICY_MAX_WIDTH);
    if (d->n_out < 1 || d->n_out > DOCKAUV_MAX_U) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.n_out: %d outside 1..%d", d->n_out, DOCKAUV_MAX_U);
    if (d->hidden_act != DOCKAUV_ACT_TANH && d->hidden_act != DOCKAUV_ACT_RELU)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.hidden_act: %d is neither DOCKAUV_ACT_TANH nor DOCKAUV_ACT_RELU", d->hidden_act);
    if (d->out_act != DOCKAUV_ACT_NONE && d->out_act != DOCKAUV_ACT_TANH)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.out_act: %d is neither DOCKAUV_ACT_NONE nor DOCKAUV_ACT_TANH", d->out_act);
    if (d->pointers_on_device != 0 && d->pointers_on_device != 1)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.pointers_on_device: %d must be 0 or 1", d->pointers_on_device);
    if (!d->W1) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.W1 is NULL");
    if (!d->b1) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.b1 is NULL");
    if (d->n_hidden[1] > 0 && !d->W2) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.W2 is NULL (n_hidden[1] > 0)");
    if (d->n_hidden[1] > 0 && !d->b2) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.b2 is NULL (n_hidden[1] > 0)");
    if (!d->W3) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.W3 is NULL");
    if (!d->b3) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.b3 is NULL");
    if (like && (d->n_in != like->n_in || d->n_hidden[0] != like->n_h1 || d->n_hidden[1] != like->n_h2 || d->n_out != like->n_out ||
                 d->hidden_act != like->hidden_act || d->out_act != like->out_act))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_load: n_in / n_hidden / n_out / activations differ from the policy's (%d-%d-%d-%d)",
                    like->n_in, like->n_h1, like->n_h2, like->n_out);
    return 0;
}

// weights of `d` -> p->packed, ordered on `stream`; host arrays go through p->raw and the call waits for the copies
int upload_policy(dockauv_policy p, const dockauv_policy_desc* d, hipStream_t stream) {
    dockauv_handle h = p->h;
    const PolicyShape& S = p->S;
    const int n_last = S.n_h2 ? S.n_h2 : S.n_h1;
    const float* src[7] = {d->W1, d->b1, d->W2, d->b2, d->W3, d->b3, d->log_std};
    const size_t cnt[7] = {(size_t)S.n_h1 * S.n_in, (size_t)S.n_h1, (size_t)S.n_h2 * S.n_h1, (size_t)S.n_h2,
                           (size_t)S.n_out * n_last, (size_t)S.n_out, (size_t)S.n_out};
    const float* dev[7];
    if (d->pointers_on_device) {
        for (int i = 0; i < 7; ++i) dev[i] = src[i];
    } else {
        size_t off = 0;
        for (int i = 0; i < 7; ++i) {
            dev[i] = (src[i] && cnt[i] && !(i == 6 && (p->value_role || p->q_role))) ? p->raw + off : nullptr;
            if (dev[i]) HIP_TRY(h, hipMemcpyAsync(p->raw + off, src[i], cnt[i] * sizeof(float), hipMemcpyHostToDevice, stream));
            off += cnt[i];
        }
        HIP_TRY(h, hipStreamSynchronize(stream));   // the caller's host arrays are free on return
    }
    if (!S.n_h2) dev[2] = dev[3] = nullptr;
    if (p->value_role || p->q_role) dev[6] = nullptr;   // (a critic has no exploration noise)
    if (dev[6]) HIP_TRY(h, hipMemcpyAsync(p->log_std, dev[6], cnt[6] * sizeof(float), hipMemcpyDeviceToDevice, stream));
    const PolicyRaw raw{dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], dev[6]};
    const int rc = launch_policy_pack(S, raw, p->packed, stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "policy weight packing launch failed: %s", hipGetErrorString((hipError_t)rc));
    p->has_log_std = dev[6] != nullptr;
    p->seed = d->seed;
    p->env_id_offset = d->env_id_offset;
    return 0;
}

int policy_forward(dockauv_handle h, dockauv_policy p, const float* rows, float* actions, uint64_t t, int stochastic, hipStream_t stream,
                   float* log_prob = nullptr) {
    if (p->sac_role) {
        // the per-env form of the squashed-Gaussian actor: the plain actor's rows, counter and noise stream
        SacActorLaunch l{rows, nullptr, actions, log_prob, (long)h->cfg.n_envs, h->n_obs + 2, h->n_u_max, stochastic ? 1 : 0,
                         t, p->env_id_offset, p->seed, 2u};
        const int rc = launch_sac_actor(p->S, p->packed, l, stream);
        if (rc != 0) return fail(h, DOCKAUV_E_HIP, "SAC actor kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
        h->last_stream = stream;
        return 0;
    }
    const int rc = launch_policy_forward(p->S, p->packed, rows, actions, h->cfg.n_envs, h->n_obs + 2, h->n_u_max, t,
                                         (stochastic && p->has_log_std) ? 1 : 0, p->seed, p->env_id_offset, stream, log_prob,
                                         log_prob ? p->log_std : nullptr);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "policy kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = stream;
    return 0;
}

// V(rows[r]) for n_rows packed rows -> values[r]: the critic's kernel with one output unit and an action stride of 1
int value_forward(dockauv_handle h, dockauv_policy c, const float* rows, long long n_rows, float* values, hipStream_t stream) {
    const int rc = launch_policy_forward(c->S, c->packed, rows, values, (long)n_rows, h->n_obs + 2, 1, 0, 0, 0, 0, stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "value kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = stream;
    return 0;
}

// what the actor argument of `fn` must be: of this handle, not a critic; with want_logp also a log_std and a raw output.
// ppo (everything but forward / forward_logp / rollout): a squashed-Gaussian actor is refused by name
int check_actor(dockauv_handle h, dockauv_policy p, const char* fn, bool want_logp, bool ppo = true) {
    if (p->h != h) return fail(h, DOCKAUV_E_INVALID, "%s: the policy was created for another handle", fn);
    if (p->value_role) return fail(h, DOCKAUV_E_INVALID, "%s: the policy is a critic (dockauv_value_create), an actor is needed", fn);
    if (p->q_role) return fail(h, DOCKAUV_E_INVALID, "%s: the policy is a Q critic (dockauv_q_create), an actor is needed", fn);
    if (p->sac_role && ppo)
        return fail(h, DOCKAUV_E_INVALID, "%s: the policy is a squashed-Gaussian actor (dockauv_sac_actor_create); this call is PPO's and "
                    "takes a plain actor (dockauv_policy_create)", fn);
    if (p->sac_role) return 0;   // (its log-probability carries the squashing correction)
    if (want_logp && !p->has_log_std) return fail(h, DOCKAUV_E_INVALID, "%s: log_prob needs a policy with a log_std", fn);
    if (want_logp && p->S.out_act == DOCKAUV_ACT_TANH)
        return fail(h, DOCKAUV_E_INVALID, "%s: log_prob of a policy with out_act DOCKAUV_ACT_TANH needs the squashing correction, "
                    "which stays with the learner", fn);
    return 0;
}

// the SAC roles by name, for the calls whose arithmetic is the plain MLP's or PPO's
int refuse_sac_roles(dockauv_handle h, dockauv_policy p, const char* fn) {
    if (p->sac_role)
        return fail(h, DOCKAUV_E_INVALID, "%s: the policy is a squashed-Gaussian actor (dockauv_sac_actor_create), which this call does not take", fn);
    if (p->q_role) return fail(h, DOCKAUV_E_INVALID, "%s: the policy is a Q critic (dockauv_q_create), which this call does not take", fn);
    return 0;
}

int check_critic(dockauv_handle h, dockauv_policy c, const char* fn) {
    if (c->h != h) return fail(h, DOCKAUV_E_INVALID, "%s: the critic was created for another handle", fn);
    if (c->q_role) return fail(h, DOCKAUV_E_INVALID, "%s: the critic argument is a Q critic (dockauv_q_create), a value critic is needed", fn);
    if (c->sac_role)
        return fail(h, DOCKAUV_E_INVALID, "%s: the critic argument is a squashed-Gaussian actor (dockauv_sac_actor_create), not a critic", fn);
    if (!c->value_role) return fail(h, DOCKAUV_E_INVALID, "%s: the critic argument is an actor (dockauv_policy_create), not a critic", fn);
    return 0;
}

int check_gae_factors(dockauv_handle h, const char* fn, float gamma, float gae_lambda) {
    if (!(gamma >= 0.0f && gamma <= 1.0f)) return fail(h, DOCKAUV_E_INVALID, "%s: gamma %g outside [0, 1]", fn, (double)gamma);
    if (!(gae_lambda >= 0.0f && gae_lambda <= 1.0f)) return fail(h, DOCKAUV_E_INVALID, "%s: gae_lambda %g outside [0, 1]", fn, (double)gae_lambda);
    return 0;
}

// the launches of dockauv_rollout; log_prob (nullable, [n_steps][n_envs]): the actor in its log-prob form
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

// a dockauv_truncation_io against the handle, before any device call; `full`: also what the value launch and GAE touch
int check_truncation(dockauv_handle h, const dockauv_truncation_io* io, const char* fn, bool full) {
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (!io) return fail(h, DOCKAUV_E_INVALID, "%s: io is NULL", fn);
    if (io->struct_size != sizeof(dockauv_truncation_io))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.struct_size: got %u, library has %zu", io->struct_size, sizeof(dockauv_truncation_io));
    if (io->n_steps < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.n_steps: %d must be >= 1", io->n_steps);
    if (h->cfg.max_timesteps < 1) return fail(h, DOCKAUV_E_INVALID, "%s: the handle's max_timesteps %d must be >= 1", fn, h->cfg.max_timesteps);
    const int need = truncation_slots(io->n_steps, h->cfg.max_timesteps);
    if (io->n_slots < need)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.n_slots: %d, dockauv_truncation_slots gives %d for %d steps", io->n_slots, need, io->n_steps);
    if (!io->rows_out) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.rows_out is NULL");
    if (!io->terminal_obs) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.terminal_obs is NULL");
    if (!io->length_carry) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.length_carry is NULL");
    if (!io->trunc_step) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.trunc_step is NULL");
    if (!io->trunc_row) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.trunc_row is NULL");
    if (full) {
        if (!io->values) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.values is NULL");
        if (!io->v_terminal) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.v_terminal is NULL");
        if (!io->advantages) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.advantages is NULL");
        if (!io->returns) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.returns is NULL");
        if (int rc = check_gae_factors(h, "dockauv_truncation_io", io->gamma, io->gae_lambda)) return rc;
    }
    if (h->f64) return fail(h, DOCKAUV_E_INVALID, "%s: the packed rows are float32; the handle's precision is DOCKAUV_F64", fn);
    if (h->cfg.reset_mode == DOCKAUV_RESET_NONE)
        return fail(h, DOCKAUV_E_INVALID, "%s: the handle's reset_mode is DOCKAUV_RESET_NONE: an episode does not restart at the row "
                    "after a done", fn);
    return 0;
}

int truncation_scan(dockauv_handle h, const dockauv_truncation_io* io, hipStream_t stream) {
    TruncArgs a{};
    a.rows = io->rows_out;
    a.terminal_obs = io->terminal_obs;
    a.carry_len = io->length_carry;
    a.trunc_step = io->trunc_step;
    a.trunc_row = (long long*)io->trunc_row;
    a.n_steps = io->n_steps;
    a.n_envs = h->cfg.n_envs;
    a.n_obs = h->n_obs;
    a.row_stride = h->n_obs + 2;
    a.max_timesteps = h->cfg.max_timesteps;
    a.n_slots = io->n_slots;
    const int rc = launch_truncation_scan(a, stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "truncation scan launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = stream;
    return 0;
}

// the GAE stage of every entry point: g carries the caller's buffers and factors (reward_col: the reward column of
// dockauv_gae_normalized).  With tio the three launches of dockauv_gae_truncated: the scan, V of the slots' terminal observations,
// and the GAE launch on the slots
int queue_gae(dockauv_handle h, dockauv_policy critic, const dockauv_truncation_io* tio, GaeLaunch g, hipStream_t stream) {
    g.n_envs = h->cfg.n_envs;
    g.n_obs = h->n_obs;
    if (tio) {
        if (int rc = truncation_scan(h, tio, stream)) return rc;
        const long n = (long)tio->n_slots * (long)h->cfg.n_envs;
        const int rc = launch_policy_forward_rows(critic->S, critic->packed, tio->terminal_obs, (const long long*)tio->trunc_row, n, h->n_obs,
                                                  tio->v_terminal, stream);
        if (rc != 0) return fail(h, DOCKAUV_E_HIP, "value kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
        g.trunc_step = tio->trunc_step;
        g.v_terminal = tio->v_terminal;
        g.n_slots = tio->n_slots;
    }
    const int rc = launch_gae(g, stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "GAE kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = stream;
    return 0;
}

// a dockauv_rewnorm_io on its own, before any device call and before the handle is looked at
int check_rewnorm_io(dockauv_handle h, const dockauv_rewnorm_io* io, const char* fn) {
    if (!io) return fail(h, DOCKAUV_E_INVALID, "%s: the dockauv_rewnorm_io is NULL", fn);
    if (io->struct_size != sizeof(dockauv_rewnorm_io))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_io.struct_size: got %u, library has %zu", io->struct_size, sizeof(dockauv_rewnorm_io));
    if (io->n_steps < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_io.n_steps: %d must be >= 1", io->n_steps);
    if (!io->rows_out) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_io.rows_out is NULL");
    if (!io->reward_norm) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_io.reward_norm is NULL");
    if (io->training && !io->discounted) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_io.discounted is NULL (required when training)");
    if (io->training && !io->step_stats) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_io.step_stats is NULL (required when training)");
    return 0;
}

// handle and normaliser of `fn`, after the argument blocks
int check_rewnorm(dockauv_handle h, dockauv_rewnorm rn, const char* fn) {
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (!rn) return fail(h, DOCKAUV_E_INVALID, "%s: null normaliser", fn);
    if (h->f64) return fail(h, DOCKAUV_E_INVALID, "%s: the packed rows are float32; the handle's precision is DOCKAUV_F64", fn);
    if (rn->h != h) return fail(h, DOCKAUV_E_INVALID, "%s: the normaliser was created for another handle", fn);
    return 0;
}

int rewnorm_scan(dockauv_handle h, dockauv_rewnorm rn, const dockauv_rewnorm_io* io, hipStream_t stream) {
    RewnormArgs a{};
    a.rows = io->rows_out;
    a.carry = rn->carry;
    a.state = rn->state;
    a.discounted = io->discounted;
    a.reward_norm = io->reward_norm;
    a.step_stats = io->step_stats;
    a.n_steps = io->n_steps;
    a.n_envs = h->cfg.n_envs;
    a.n_obs = h->n_obs;
    a.row_stride = h->n_obs + 2;
    a.training = io->training ? 1 : 0;
    a.gamma = rn->gamma;
    a.clip_reward = rn->clip_reward;
    a.epsilon = rn->epsilon;
    const int rc = launch_rewnorm_scan(a, stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "reward normalisation launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = stream;
    return 0;
}

// what a truncation block must share with the GAE arguments `g` of the call it belongs to; `whose`: the block
// (dockauv_collect_io, whose terminal_obs must be the truncation block's too) or the function (dockauv_gae_normalized) they come from
int check_truncation_matches(dockauv_handle h, const dockauv_truncation_io* tio, const GaeLaunch& g, const float* terminal_obs, const char* whose) {
    if (tio->n_steps != g.n_steps) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.n_steps: %d, %s's is %d", tio->n_steps, whose, g.n_steps);
    if (tio->rows_out != g.rows) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.rows_out is not %s's", whose);
    if (terminal_obs && tio->terminal_obs != terminal_obs) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.terminal_obs is not %s's", whose);
    if (tio->values != g.values) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.values is not %s's", whose);
    if (tio->advantages != g.advantages) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.advantages is not %s's", whose);
    if (tio->returns != g.returns) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.returns is not %s's", whose);
    if (tio->gamma != g.gamma) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.gamma: %g, %s's is %g", (double)tio->gamma, whose, (double)g.gamma);
    if (tio->gae_lambda != g.gae_lambda)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.gae_lambda: %g, %s's is %g", (double)tio->gae_lambda, whose, (double)g.gae_lambda);
    return 0;
}

// what the three collect calls check alike on their dockauv_collect_io, `arg` in the words of `fn`
int check_collect_io(dockauv_handle h, const dockauv_collect_io* io, const char* fn, const char* arg) {
    if (!io) return fail(h, DOCKAUV_E_INVALID, "%s: %s is NULL", fn, arg);
    if (io->struct_size != sizeof(dockauv_collect_io))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_collect_io.struct_size: got %u, library has %zu", io->struct_size, sizeof(dockauv_collect_io));
    if (io->n_steps < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_collect_io.n_steps: %d must be >= 1", io->n_steps);
    if (!io->rows_in || !io->rows_out || !io->actions_out)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_collect_io: rows_in/rows_out/actions_out must not be NULL");
    return 0;
}

// the GAE arguments of a collect block
GaeLaunch gae_of(const dockauv_collect_io* cio, const float* reward_col = nullptr) {
    return {cio->rows_out, cio->values, cio->advantages, cio->returns, cio->n_steps, cio->gamma, cio->gae_lambda, reward_col};
}

// One collection, validated by its entry point: with tio, length_carry <- the steps of every env's episode before step 0 (the
// handle's own counters at this point of the stream: monitor_sync); the rollout; with a critic V of the K + 1 observation sets,
// with rn the normaliser's scan, and the GAE stage
int queue_collect(dockauv_handle h, dockauv_policy actor, dockauv_policy critic, const dockauv_collect_io* cio,
                  const dockauv_truncation_io* tio, dockauv_rewnorm rn, const dockauv_rewnorm_io* nio, hipStream_t stream) {
    HIP_TRY(h, hipSetDevice(h->device));
    const int K = cio->n_steps;
    const size_t N = (size_t)h->cfg.n_envs;
    if (tio) {
        HIP_TRY(h, hipMemcpyAsync(tio->length_carry, h->B.t_steps, N * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
        h->last_stream = stream;
    }
    int rc = queue_rollout(h, actor, cio->rows_in, cio->rows_out, cio->actions_out, cio->terminal_obs, cio->log_prob, K, cio->t0,
                           cio->stochastic, stream);
    if (rc) return rc;
    if (critic) {
        if ((rc = value_forward(h, critic, cio->rows_in, (long long)N, cio->values, stream)) != 0) return rc;
        if ((rc = value_forward(h, critic, cio->rows_out, (long long)K * (long long)N, cio->values + N, stream)) != 0) return rc;
        if (rn && (rc = rewnorm_scan(h, rn, nio, stream)) != 0) return rc;
        if ((rc = queue_gae(h, critic, tio, gae_of(cio, rn ? nio->reward_norm : nullptr), stream)) != 0) return rc;
    }
    return check_status(h);   // (what dockauv_poll_status looks at: no synchronisation)
}

// actor (dockauv_policy_create) or critic (dockauv_value_create): `fn` names the entry point in the messages
int create_policy(dockauv_handle h, const dockauv_policy_desc* d, dockauv_policy* out, bool value_role, const char* fn, bool q_role = false) {
    if (!d || !out) return fail(h, DOCKAUV_E_INVALID, "%s: null argument", fn);
    *out = nullptr;
    int rc = validate_policy_desc(h, d, nullptr);
    if (rc) return rc;
    if ((value_role || q_role) && d->n_out != 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.n_out: %d, a critic has one output", d->n_out);
    if ((value_role || q_role) && d->out_act != DOCKAUV_ACT_NONE)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.out_act: %d, a critic's output is raw (DOCKAUV_ACT_NONE)", d->out_act);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (h->f64) return fail(h, DOCKAUV_E_INVALID, "%s: the policy kernel is float32; the handle's precision is DOCKAUV_F64", fn);
    if (q_role && d->n_in != h->n_obs + h->n_u_max)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.n_in: %d, a Q critic reads [obs | action]: the handle's n_obs + n_u is %d + %d", d->n_in,
                    h->n_obs, h->n_u_max);
    if (!q_role && d->n_in != h->n_obs) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.n_in: %d, the handle's n_obs is %d", d->n_in, h->n_obs);
    if (!value_role && !q_role && d->n_out != h->n_u_max)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc.n_out: %d, the handle's n_u is %d", d->n_out, h->n_u_max);
    PolicyShape S{};
    S.n_in = d->n_in;
    S.n_h1 = d->n_hidden[0];
    S.n_h2 = d->n_hidden[1];
    S.n_out = d->n_out;
    S.hidden_act = d->hidden_act;
    S.out_act = d->out_act;
    policy_layout(S);
    if (policy_lds_bytes(S) > kPolMaxLds)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_desc: the padded weights (%zu B for n_in %d, n_hidden %d / %d) exceed "
                    "the 160 KiB of LDS the policy kernel keeps them in: narrower layers", policy_lds_bytes(S), S.n_in, S.n_h1, S.n_h2);
    HIP_TRY(h, hipSetDevice(h->device));
    dockauv_policy p = new dockauv_policy_s();
    p->h = h;
    p->S = S;
    p->value_role = value_role;
    p->q_role = q_role;
    const int n_last = S.n_h2 ? S.n_h2 : S.n_h1;
    const size_t raw_floats = (size_t)S.n_h1 * S.n_in + S.n_h1 + (size_t)S.n_h2 * S.n_h1 + S.n_h2 + (size_t)S.n_out * n_last + 2 * (size_t)S.n_out;
    hipError_t e = hipMalloc((void**)&p->packed, (size_t)S.total * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&p->raw, raw_floats * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&p->log_std, DOCKAUV_MAX_U * sizeof(float));
    if (e == hipSuccess) e = hipMemset(p->log_std, 0, DOCKAUV_MAX_U * sizeof(float));
    if (e != hipSuccess) {
        dockauv_policy_destroy(p);
        return fail(h, DOCKAUV_E_HIP, "policy buffers: %s", hipGetErrorString(e));
    }
    if ((rc = upload_policy(p, d, nullptr)) != 0) {
        dockauv_policy_destroy(p);
        return rc;
    }
    *out = p;
    return 0;
}

// lengths of W1 b1 W2 b2 W3 b3 of a policy, torch.nn.Linear layout
void layer_lengths(const PolicyShape& S, int* len) {
    const int n_last = S.n_h2 ? S.n_h2 : S.n_h1;
    len[0] = S.n_h1 * S.n_in;
    len[1] = S.n_h1;
    len[2] = S.n_h2 * S.n_h1;
    len[3] = S.n_h2;
    len[4] = S.n_out * n_last;
    len[5] = S.n_out;
}

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

// the head launches' arguments from the io block; the workspace is the actor's
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

// a dockauv_optim_io against the optimiser (dockauv_optim_step, and the `opt` of dockauv_ppo_update)
int check_optim_io(dockauv_handle h, dockauv_optim o, const dockauv_optim_io* io) {
    if (!(io->lr >= 0.0) || !std::isfinite(io->lr)) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_io.lr: %g must be >= 0 and finite", io->lr);
    if (int rc = check_optim_arrays(h, "actor", o->len, io->actor_params, io->actor_grads)) return rc;
    if (!io->log_std) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_io.log_std is NULL");
    if (!io->grad_log_std) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_io.grad_log_std is NULL");
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

// step t's bias corrections, in double, rounded once (include/dockauv.h: dockauv_optim_step)
void bias_corrections(dockauv_optim o, double lr, long long t, float& step_size, float& rsq) {
    step_size = (float)(lr / (1.0 - std::pow(o->beta1, (double)t)));
    rsq = (float)(1.0 / std::sqrt(1.0 - std::pow(o->beta2, (double)t)));
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

int dockauv_policy_create(dockauv_handle h, const dockauv_policy_desc* d, dockauv_policy* out) {
    return create_policy(h, d, out, false, "dockauv_policy_create");
}

int dockauv_value_create(dockauv_handle h, const dockauv_policy_desc* d, dockauv_policy* out) {
    return create_policy(h, d, out, true, "dockauv_value_create");
}

int dockauv_policy_load(dockauv_policy p, const dockauv_policy_desc* d, void* hip_stream) {
    if (!p) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_policy_load: null policy");
    if (!d) return fail(p->h, DOCKAUV_E_INVALID, "dockauv_policy_load: null descriptor");
    if (p->sac_role)
        return fail(p->h, DOCKAUV_E_INVALID, "dockauv_policy_load: the policy is a squashed-Gaussian actor (dockauv_sac_actor_create): "
                    "its weights come through dockauv_sac_actor_load");
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
    if (int rc = refuse_sac_roles(h, p, "dockauv_policy_forward_rows")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const int rc = launch_policy_forward_rows(p->S, p->packed, rows, (const long long*)row_index, (long)n_rows, h->n_obs + 2, out,
                                              (hipStream_t)hip_stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "policy rows kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = (hipStream_t)hip_stream;
    return 0;
}

int dockauv_policy_backward(dockauv_handle h, dockauv_policy p, const float* rows, const int64_t* row_index, long long n_rows,
                            const float* grad_out, const dockauv_policy_grads* grads, void* hip_stream) {
    if (!rows || !grad_out || !grads) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_backward: rows/grad_out/grads must not be NULL");
    if (grads->struct_size != sizeof(dockauv_policy_grads))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_grads.struct_size: got %u, library has %zu", grads->struct_size, sizeof(dockauv_policy_grads));
    if (!grads->dW1 || !grads->db1 || !grads->dW3 || !grads->db3)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_grads: dW1/db1/dW3/db3 must not be NULL");
    if (n_rows < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_backward: n_rows %lld must be >= 1", n_rows);
    if (!p) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_backward: null policy");
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_policy_backward: null handle");
    if (p->h != h) return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_backward: the policy was created for another handle");
    if (int rc = refuse_sac_roles(h, p, "dockauv_policy_backward")) return rc;
    if (p->S.n_h2 > 0 && (!grads->dW2 || !grads->db2))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_grads: dW2/db2 are NULL, the policy has two hidden layers");
    BackwardLayout L;
    backward_layout(p->S, L);
    if (backward_lds_bytes(L) > kPolMaxLds)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_backward: the kernel needs %zu B of LDS for n_in %d, n_hidden %d / %d (weights, one "
                    "pass's rows, activations and deltas), more than the 160 KiB of a group: narrower layers or observations",
                    backward_lds_bytes(L), p->S.n_in, p->S.n_h1, p->S.n_h2);
    HIP_TRY(h, hipSetDevice(h->device));
    if (!p->bwd_partial) HIP_TRY(h, hipMalloc((void**)&p->bwd_partial, (size_t)kBwdMaxGroups * L.n_params * sizeof(float)));
    const PolicyGrads g{grads->dW1, grads->db1, p->S.n_h2 ? grads->dW2 : nullptr, p->S.n_h2 ? grads->db2 : nullptr, grads->dW3, grads->db3};
    const int rc = launch_policy_backward(p->S, p->packed, rows, (const long long*)row_index, (long)n_rows, h->n_obs + 2, grad_out,
                                          p->bwd_partial, g, (hipStream_t)hip_stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "policy backward launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = (hipStream_t)hip_stream;
    return 0;
}

int dockauv_ppo_head(dockauv_handle h, dockauv_policy actor, const dockauv_ppo_head_io* io, void* hip_stream) {
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_ppo_head: null handle");
    if (!actor) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head: null actor");
    if (!io) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head: io is NULL");
    if (io->struct_size != sizeof(dockauv_ppo_head_io))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head_io.struct_size: got %u, library has %zu", io->struct_size, sizeof(dockauv_ppo_head_io));
    if (int rc = check_actor(h, actor, "dockauv_ppo_head", true)) return rc;
    if (io->n_rows < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head_io.n_rows: %lld must be >= 1", io->n_rows);
    if (io->normalize_advantage && io->n_rows < 2)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head_io.n_rows: %lld must be >= 2 with normalize_advantage (the unbiased deviation)", io->n_rows);
    if (!(io->clip_range > 0.0f)) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head_io.clip_range: %g must be > 0", (double)io->clip_range);
    if (!io->mean) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head_io.mean is NULL");
    if (!io->actions) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head_io.actions is NULL");
    if (!io->log_prob_old) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head_io.log_prob_old is NULL");
    if (!io->advantages) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head_io.advantages is NULL");
    if (!io->grad_mean) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head_io.grad_mean is NULL");
    if (!io->grad_log_std) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head_io.grad_log_std is NULL");
    if (!io->stats) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head_io.stats is NULL");
    if ((io->v == nullptr) != (io->grad_v == nullptr))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head_io.v / grad_v: both or neither must be NULL (NULL: no critic)");
    if (io->v && !io->returns) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_head_io.returns is NULL (v is given)");
    HIP_TRY(h, hipSetDevice(h->device));
    if (!actor->head_ws) HIP_TRY(h, hipMalloc((void**)&actor->head_ws, kHeadWorkspaceBytes));
    HeadArgs a{};
    head_args(actor, io, a);
    const int rc = launch_ppo_head(a, hip_stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "PPO head launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = (hipStream_t)hip_stream;
    return 0;
}

int dockauv_gae(dockauv_handle h, const float* rows_out, const float* values, int n_steps, float gamma, float gae_lambda,
                float* advantages, float* returns, void* hip_stream) {
    if (!rows_out || !values || !advantages || !returns)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_gae: rows_out/values/advantages/returns must not be NULL");
    if (n_steps < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_gae: n_steps %d must be >= 1", n_steps);
    if (int rc = check_gae_factors(h, "dockauv_gae", gamma, gae_lambda)) return rc;
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_gae: null handle");
    if (h->f64) return fail(h, DOCKAUV_E_INVALID, "dockauv_gae: the packed rows are float32; the handle's precision is DOCKAUV_F64");
    HIP_TRY(h, hipSetDevice(h->device));
    return queue_gae(h, nullptr, nullptr, {rows_out, values, advantages, returns, n_steps, gamma, gae_lambda}, (hipStream_t)hip_stream);
}

int dockauv_collect(dockauv_handle h, dockauv_policy actor, dockauv_policy critic, const dockauv_collect_io* io, void* hip_stream) {
    if (int rc = check_collect_io(h, io, "dockauv_collect", "io")) return rc;
    if (critic && (!io->values || !io->advantages || !io->returns))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_collect_io: values/advantages/returns must not be NULL with a critic");
    if (!critic && (io->values || io->advantages || io->returns))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_collect_io: values/advantages/returns must be NULL without a critic");
    if (critic)
        if (int rc = check_gae_factors(h, "dockauv_collect_io", io->gamma, io->gae_lambda)) return rc;
    if (!actor) return fail(h, DOCKAUV_E_INVALID, "dockauv_collect: null actor");
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_collect: null handle");
    if (int rc = check_actor(h, actor, "dockauv_collect", io->log_prob != nullptr)) return rc;
    if (critic)
        if (int rc = check_critic(h, critic, "dockauv_collect")) return rc;
    return queue_collect(h, actor, critic, io, nullptr, nullptr, nullptr, (hipStream_t)hip_stream);
}

int dockauv_truncation_slots(dockauv_handle h, int n_steps) {
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_truncation_slots: null handle");
    if (n_steps < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_slots: n_steps %d must be >= 1", n_steps);
    if (h->cfg.max_timesteps < 1)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_slots: the handle's max_timesteps %d must be >= 1", h->cfg.max_timesteps);
    return truncation_slots(n_steps, h->cfg.max_timesteps);
}

int dockauv_truncation_scan(dockauv_handle h, const dockauv_truncation_io* io, void* hip_stream) {
    if (int rc = check_truncation(h, io, "dockauv_truncation_scan", false)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return truncation_scan(h, io, (hipStream_t)hip_stream);
}

int dockauv_gae_truncated(dockauv_handle h, dockauv_policy critic, const dockauv_truncation_io* io, void* hip_stream) {
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_gae_truncated: null handle");
    if (!critic) return fail(h, DOCKAUV_E_INVALID, "dockauv_gae_truncated: null critic");
    if (int rc = check_truncation(h, io, "dockauv_gae_truncated", true)) return rc;
    if (int rc = check_critic(h, critic, "dockauv_gae_truncated")) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return queue_gae(h, critic, io, {io->rows_out, io->values, io->advantages, io->returns, io->n_steps, io->gamma, io->gae_lambda},
                     (hipStream_t)hip_stream);
}

int dockauv_collect_truncated(dockauv_handle h, dockauv_policy actor, dockauv_policy critic, const dockauv_collect_io* cio,
                              const dockauv_truncation_io* tio, void* hip_stream) {
    const char* fn = "dockauv_collect_truncated";
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (!actor) return fail(h, DOCKAUV_E_INVALID, "%s: null actor", fn);
    if (!critic) return fail(h, DOCKAUV_E_INVALID, "%s: null critic (the bootstrap is the critic's value)", fn);
    if (int rc = check_collect_io(h, cio, fn, "cio")) return rc;
    if (!cio->terminal_obs) return fail(h, DOCKAUV_E_INVALID, "dockauv_collect_io.terminal_obs is NULL (%s reads it)", fn);
    if (!cio->values || !cio->advantages || !cio->returns)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_collect_io: values/advantages/returns must not be NULL with a critic");
    if (int rc = check_truncation(h, tio, fn, true)) return rc;
    if (int rc = check_truncation_matches(h, tio, gae_of(cio), cio->terminal_obs, "dockauv_collect_io")) return rc;
    if (int rc = check_actor(h, actor, fn, cio->log_prob != nullptr)) return rc;
    if (int rc = check_critic(h, critic, fn)) return rc;
    return queue_collect(h, actor, critic, cio, tio, nullptr, nullptr, (hipStream_t)hip_stream);
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

int dockauv_optim_create(dockauv_handle h, dockauv_policy actor, dockauv_policy critic, const dockauv_optim_desc* d, dockauv_optim* out) {
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_optim_create: null handle");
    if (!out) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_create: out is NULL");
    *out = nullptr;
    if (!actor) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_create: null actor");
    if (!d) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_create: desc is NULL");
    if (d->struct_size != sizeof(dockauv_optim_desc))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_desc.struct_size: got %u, library has %zu", d->struct_size, sizeof(dockauv_optim_desc));
    if (actor->h != h) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_create: the actor was created for another handle");
    if (actor->value_role) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_create: the actor argument is a critic (dockauv_value_create)");
    if (int rc = refuse_sac_roles(h, actor, "dockauv_optim_create")) return rc;
    if (!actor->has_log_std) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_create: the actor has no log_std (its gradient is part of the index space)");
    if (critic)
        if (int rc = check_critic(h, critic, "dockauv_optim_create")) return rc;
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
    if (!io) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_step: io is NULL");
    if (io->struct_size != sizeof(dockauv_optim_io))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_io.struct_size: got %u, library has %zu", io->struct_size, sizeof(dockauv_optim_io));
    if (o->h != h) return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_step: the optimiser was created for another handle");
    if (int rc = check_optim_io(h, o, io)) return rc;
    if (int rc = reconcile_steps(o)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    const long long t = ++o->t;
    AdamArgs a{};
    adam_args(o, io, io->stats, a);
    bias_corrections(o, io->lr, t, a.step_size, a.rsq);
    const int rc = launch_adam_step(a, stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "optimiser launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = stream;
    if (int rc2 = repack_policy(o->actor, io->actor_params, io->log_std, stream)) return rc2;
    if (o->critic)
        if (int rc2 = repack_policy(o->critic, io->critic_params, nullptr, stream)) return rc2;
    return 0;
}

int dockauv_permutation(dockauv_handle h, uint64_t seed, uint64_t epoch, long long n, int64_t* out, void* hip_stream) {
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_permutation: null handle");
    if (!out) return fail(h, DOCKAUV_E_INVALID, "dockauv_permutation: out is NULL");
    if (n < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_permutation: n %lld must be >= 1", n);
    if (n > (1ll << 31)) return fail(h, DOCKAUV_E_INVALID, "dockauv_permutation: n %lld must be <= 2^31 (the network works on 32-bit words)", n);
    HIP_TRY(h, hipSetDevice(h->device));
    const int rc = launch_permutation(seed, epoch, n, (long long*)out, hip_stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "permutation launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = (hipStream_t)hip_stream;
    return 0;
}

int dockauv_ppo_update(dockauv_handle h, dockauv_optim o, const dockauv_ppo_update_io* io, void* hip_stream) {
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_ppo_update: null handle");
    if (!o) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update: null optimiser");
    if (!io) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update: io is NULL");
    if (io->struct_size != sizeof(dockauv_ppo_update_io))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.struct_size: got %u, library has %zu", io->struct_size, sizeof(dockauv_ppo_update_io));
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
    if (!io->rows) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.rows is NULL");
    if (!io->actions) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.actions is NULL");
    if (!io->log_prob_old) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.log_prob_old is NULL");
    if (!io->advantages) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.advantages is NULL");
    if (critic && !io->returns) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.returns is NULL (the optimiser has a critic)");
    if (io->clip_range_vf > 0.0f && !critic)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.clip_range_vf: %g, but the optimiser has no critic", (double)io->clip_range_vf);
    if (io->clip_range_vf > 0.0f && !io->values_old)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.values_old is NULL (clip_range_vf is %g)", (double)io->clip_range_vf);
    if (!io->stats) return fail(h, DOCKAUV_E_INVALID, "dockauv_ppo_update_io.stats is NULL");
    if (io->opt.struct_size != sizeof(dockauv_optim_io))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_optim_io.struct_size: got %u, library has %zu", io->opt.struct_size, sizeof(dockauv_optim_io));
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
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "update control launch failed: %s", hipGetErrorString((hipError_t)rc));
    dockauv_policy_grads ag{}, cg{};
    ag.struct_size = cg.struct_size = sizeof(dockauv_policy_grads);
    float* const* agp = (float* const*)io->opt.actor_grads;     // (the caller's gradient buffers: read by the optimiser, written here)
    float* const* cgp = (float* const*)io->opt.critic_grads;
    ag.dW1 = agp[0]; ag.db1 = agp[1]; ag.dW2 = agp[2]; ag.db2 = agp[3]; ag.dW3 = agp[4]; ag.db3 = agp[5];
    cg.dW1 = cgp[0]; cg.db1 = cgp[1]; cg.dW2 = cgp[2]; cg.db2 = cgp[3]; cg.dW3 = cgp[4]; cg.db3 = cgp[5];
    long long k = 0;      // minibatches queued by this call
    for (int e = 0; e < io->n_epochs; ++e) {
        rc = launch_permutation(io->seed, io->first_epoch + (uint64_t)e, M, o->index, stream);
        if (rc != 0) return fail(h, DOCKAUV_E_HIP, "permutation launch failed: %s", hipGetErrorString((hipError_t)rc));
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
            bias_corrections(o, io->opt.lr, t0 + 1 + k, hu.step_size, hu.rsq);
            rc = launch_ppo_head_update(ha, hu, stream);
            if (rc != 0) return fail(h, DOCKAUV_E_HIP, "PPO head launch failed: %s", hipGetErrorString((hipError_t)rc));
            if ((rc = dockauv_policy_backward(h, actor, io->rows, idx, n, grad_mean, &ag, stream)) != 0) return rc;
            if (critic && (rc = dockauv_policy_backward(h, critic, io->rows, idx, n, grad_v, &cg, stream)) != 0) return rc;
            AdamArgs aa{};
            adam_args(o, &io->opt, st + 8, aa);
            rc = launch_adam_step_ctl(aa, o->ctl, stream);
            if (rc != 0) return fail(h, DOCKAUV_E_HIP, "optimiser launch failed: %s", hipGetErrorString((hipError_t)rc));
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

int dockauv_monitor_create(dockauv_handle h, dockauv_monitor* out) {
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_monitor_create: null handle");
    if (!out) return fail(h, DOCKAUV_E_INVALID, "dockauv_monitor_create: out is NULL");
    *out = nullptr;
    if (h->f64) return fail(h, DOCKAUV_E_INVALID, "dockauv_monitor_create: the packed rows are float32; the handle's precision is DOCKAUV_F64");
    if (h->cfg.reset_mode == DOCKAUV_RESET_NONE)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_monitor_create: the handle's reset_mode is DOCKAUV_RESET_NONE: an episode does not "
                    "restart at the row after a done");
    HIP_TRY(h, hipSetDevice(h->device));
    dockauv_monitor m = new dockauv_monitor_s();
    m->h = h;
    const size_t N = (size_t)h->cfg.n_envs;
    hipError_t e = hipMalloc((void**)&m->carry_ret, N * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&m->carry_len, N * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&m->ws, monitor_workspace_doubles(h->cfg.n_envs) * sizeof(double));
    if (e != hipSuccess) {
        dockauv_monitor_destroy(m);
        return fail(h, DOCKAUV_E_HIP, "monitor buffers: %s", hipGetErrorString(e));
    }
    if (int rc = sync_last(h)) {   // (what the handle has queued comes first: the copies below run on the default stream)
        dockauv_monitor_destroy(m);
        return rc;
    }
    if (int rc = monitor_sync(m, nullptr)) {
        dockauv_monitor_destroy(m);
        return rc;
    }
    *out = m;
    return 0;
}

int dockauv_monitor_destroy(dockauv_monitor m) {
    if (!m) return 0;
    if (m->h) (void)hipSetDevice(m->h->device);
    (void)hipDeviceSynchronize();
    if (m->carry_ret) (void)hipFree(m->carry_ret);
    if (m->carry_len) (void)hipFree(m->carry_len);
    if (m->ws) (void)hipFree(m->ws);
    delete m;
    return 0;
}

int dockauv_monitor_sync(dockauv_monitor m, void* hip_stream) {
    if (!m) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_monitor_sync: null monitor");
    HIP_TRY(m->h, hipSetDevice(m->h->device));
    return monitor_sync(m, (hipStream_t)hip_stream);
}

int dockauv_monitor_carry(dockauv_monitor m, float** carry_return, int32_t** carry_length) {
    if (!m) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_monitor_carry: null monitor");
    if (carry_return) *carry_return = m->carry_ret;
    if (carry_length) *carry_length = m->carry_len;
    return 0;
}

int dockauv_monitor_scan(dockauv_handle h, dockauv_monitor m, const dockauv_monitor_io* io, void* hip_stream) {
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_monitor_scan: null handle");
    if (!m) return fail(h, DOCKAUV_E_INVALID, "dockauv_monitor_scan: null monitor");
    if (!io) return fail(h, DOCKAUV_E_INVALID, "dockauv_monitor_scan: io is NULL");
    if (io->struct_size != sizeof(dockauv_monitor_io))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_monitor_io.struct_size: got %u, library has %zu", io->struct_size, sizeof(dockauv_monitor_io));
    if (io->n_steps < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_monitor_io.n_steps: %d must be >= 1", io->n_steps);
    if (!io->rows_out) return fail(h, DOCKAUV_E_INVALID, "dockauv_monitor_io.rows_out is NULL");
    if (!io->stats) return fail(h, DOCKAUV_E_INVALID, "dockauv_monitor_io.stats is NULL");
    if (io->ep_outcome && !io->terminal_obs)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_monitor_io.ep_outcome needs terminal_obs (the outcome is read off the terminal observation)");
    if ((io->values == nullptr) != (io->returns == nullptr))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_monitor_io.values / returns: both or neither must be NULL (NULL: no explained variance)");
    if (h->f64) return fail(h, DOCKAUV_E_INVALID, "dockauv_monitor_scan: the packed rows are float32; the handle's precision is DOCKAUV_F64");
    if (h->cfg.reset_mode == DOCKAUV_RESET_NONE)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_monitor_scan: the handle's reset_mode is DOCKAUV_RESET_NONE: an episode does not "
                    "restart at the row after a done");
    if (m->h != h) return fail(h, DOCKAUV_E_INVALID, "dockauv_monitor_scan: the monitor was created for another handle");
    HIP_TRY(h, hipSetDevice(h->device));
    MonitorArgs a{};
    a.rows = io->rows_out;
    a.terminal_obs = io->terminal_obs;
    a.values = io->values;
    a.returns = io->returns;
    a.carry_ret = m->carry_ret;
    a.carry_len = m->carry_len;
    a.ep_return = io->ep_return;
    a.ep_length = io->ep_length;
    a.ep_outcome = io->ep_outcome;
    a.partial = m->ws;
    a.ev_partial = m->ws + (size_t)kMonWords * (size_t)monitor_groups(h->cfg.n_envs);
    a.stats = io->stats;
    a.n_steps = io->n_steps;
    a.n_envs = h->cfg.n_envs;
    a.n_obs = h->n_obs;
    a.row_stride = h->n_obs + 2;
    a.max_timesteps = h->cfg.max_timesteps;
    const int rc = launch_monitor_scan(a, hip_stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "monitor launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = (hipStream_t)hip_stream;
    return 0;
}

int dockauv_rewnorm_create(dockauv_handle h, float gamma, float clip_reward, double epsilon, dockauv_rewnorm* out) {
    if (!out) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_create: out is NULL");
    *out = nullptr;
    if (!(gamma >= 0.0f && gamma <= 1.0f)) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_create: gamma %g outside [0, 1]", (double)gamma);
    if (!(clip_reward > 0.0f)) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_create: clip_reward %g must be > 0", (double)clip_reward);
    if (!(epsilon >= 0.0)) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_create: epsilon %g must be >= 0", epsilon);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_rewnorm_create: null handle");
    if (h->f64) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_create: the packed rows are float32; the handle's precision is DOCKAUV_F64");
    HIP_TRY(h, hipSetDevice(h->device));
    dockauv_rewnorm rn = new dockauv_rewnorm_s();
    rn->h = h;
    rn->gamma = gamma;
    rn->clip_reward = clip_reward;
    rn->epsilon = epsilon;
    hipError_t e = hipMalloc((void**)&rn->carry, (size_t)h->cfg.n_envs * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&rn->state, 4 * sizeof(double));
    if (e != hipSuccess) {
        dockauv_rewnorm_destroy(rn);
        return fail(h, DOCKAUV_E_HIP, "reward normaliser buffers: %s", hipGetErrorString(e));
    }
    const int rc = launch_rewnorm_reset(rn->carry, rn->state, h->cfg.n_envs, nullptr);
    if (rc != 0) {
        dockauv_rewnorm_destroy(rn);
        return fail(h, DOCKAUV_E_HIP, "reward normaliser reset launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
    e = hipStreamSynchronize(nullptr);   // (the object is usable on any stream on return)
    if (e != hipSuccess) {
        dockauv_rewnorm_destroy(rn);
        return fail(h, DOCKAUV_E_HIP, "reward normaliser reset: %s", hipGetErrorString(e));
    }
    *out = rn;
    return 0;
}

int dockauv_rewnorm_destroy(dockauv_rewnorm rn) {
    if (!rn) return 0;
    if (rn->h) (void)hipSetDevice(rn->h->device);
    (void)hipDeviceSynchronize();
    if (rn->carry) (void)hipFree(rn->carry);
    if (rn->state) (void)hipFree(rn->state);
    delete rn;
    return 0;
}

int dockauv_rewnorm_state(dockauv_rewnorm rn, double** state, float** carry) {
    if (!rn) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_rewnorm_state: null normaliser");
    if (state) *state = rn->state;
    if (carry) *carry = rn->carry;
    return 0;
}

int dockauv_rewnorm_reset(dockauv_rewnorm rn, void* hip_stream) {
    if (!rn) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_rewnorm_reset: null normaliser");
    dockauv_handle h = rn->h;
    HIP_TRY(h, hipSetDevice(h->device));
    const int rc = launch_rewnorm_reset(rn->carry, rn->state, h->cfg.n_envs, hip_stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "reward normaliser reset launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = (hipStream_t)hip_stream;
    return 0;
}

int dockauv_rewnorm_scan(dockauv_handle h, dockauv_rewnorm rn, const dockauv_rewnorm_io* io, void* hip_stream) {
    const char* fn = "dockauv_rewnorm_scan";
    if (int rc = check_rewnorm_io(h, io, fn)) return rc;
    if (int rc = check_rewnorm(h, rn, fn)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return rewnorm_scan(h, rn, io, (hipStream_t)hip_stream);
}

int dockauv_gae_normalized(dockauv_handle h, dockauv_policy critic, const float* reward_norm, const dockauv_truncation_io* tio,
                           const float* rows_out, const float* values, int n_steps, float gamma, float gae_lambda,
                           float* advantages, float* returns, void* hip_stream) {
    const char* fn = "dockauv_gae_normalized";
    const GaeLaunch g{rows_out, values, advantages, returns, n_steps, gamma, gae_lambda, reward_norm};
    if (!reward_norm) return fail(h, DOCKAUV_E_INVALID, "%s: reward_norm is NULL", fn);
    if (!rows_out || !values || !advantages || !returns)
        return fail(h, DOCKAUV_E_INVALID, "%s: rows_out/values/advantages/returns must not be NULL", fn);
    if (n_steps < 1) return fail(h, DOCKAUV_E_INVALID, "%s: n_steps %d must be >= 1", fn, n_steps);
    if (int rc = check_gae_factors(h, fn, gamma, gae_lambda)) return rc;
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (h->f64) return fail(h, DOCKAUV_E_INVALID, "%s: the packed rows are float32; the handle's precision is DOCKAUV_F64", fn);
    if (tio) {
        if (!critic) return fail(h, DOCKAUV_E_INVALID, "%s: null critic (the bootstrap is the critic's value)", fn);
        if (int rc = check_truncation(h, tio, fn, true)) return rc;
        if (int rc = check_truncation_matches(h, tio, g, nullptr, fn)) return rc;
        if (int rc = check_critic(h, critic, fn)) return rc;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    return queue_gae(h, critic, tio, g, (hipStream_t)hip_stream);
}

int dockauv_collect_normalized(dockauv_handle h, dockauv_policy actor, dockauv_policy critic, const dockauv_collect_io* cio,
                               const dockauv_truncation_io* tio, dockauv_rewnorm rn, const dockauv_rewnorm_io* nio,
                               void* hip_stream) {
    const char* fn = "dockauv_collect_normalized";
    if (int rc = check_collect_io(h, cio, fn, "cio")) return rc;
    if (!cio->values || !cio->advantages || !cio->returns)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_collect_io: values/advantages/returns must not be NULL (%s needs a critic)", fn);
    if (tio && !cio->terminal_obs) return fail(h, DOCKAUV_E_INVALID, "dockauv_collect_io.terminal_obs is NULL (the truncation block reads it)");
    if (int rc = check_gae_factors(h, "dockauv_collect_io", cio->gamma, cio->gae_lambda)) return rc;
    if (int rc = check_rewnorm_io(h, nio, fn)) return rc;
    if (nio->n_steps != cio->n_steps) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_io.n_steps: %d, dockauv_collect_io's is %d", nio->n_steps, cio->n_steps);
    if (nio->rows_out != cio->rows_out) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_io.rows_out is not dockauv_collect_io's");
    if (int rc = check_rewnorm(h, rn, fn)) return rc;
    if (rn->gamma != cio->gamma)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_collect_io.gamma: %g, the normaliser's is %g", (double)cio->gamma, (double)rn->gamma);
    if (!actor) return fail(h, DOCKAUV_E_INVALID, "%s: null actor", fn);
    if (!critic) return fail(h, DOCKAUV_E_INVALID, "%s: null critic (advantages of normalised rewards need values)", fn);
    if (tio) {
        if (int rc = check_truncation(h, tio, fn, true)) return rc;
        if (int rc = check_truncation_matches(h, tio, gae_of(cio), cio->terminal_obs, "dockauv_collect_io")) return rc;
    }
    if (int rc = check_actor(h, actor, fn, cio->log_prob != nullptr)) return rc;
    if (int rc = check_critic(h, critic, fn)) return rc;
    return queue_collect(h, actor, critic, cio, tio, rn, nio, (hipStream_t)hip_stream);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ SAC: the forward half (dockauv_sac.hip)
namespace {

constexpr int kSacHeadRows = 16;   // the [8 + n_u][n_last] array both heads are packed from, padded to the two register groups

int validate_sac_desc(dockauv_handle h, const dockauv_sac_actor_desc* d, const PolicyShape* like) {
    if (d->struct_size != sizeof(dockauv_sac_actor_desc))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc.struct_size: got %u, library has %zu", d->struct_size, sizeof(dockauv_sac_actor_desc));
    if (d->precision != DOCKAUV_F32) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc.precision: %d, only DOCKAUV_F32 is implemented", d->precision);
    if (d->n_in < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc.n_in: %d must be >= 1", d->n_in);
    if (d->n_hidden[0] < 1 || d->n_hidden[0] > DOCKAUV_POLICY_MAX_WIDTH)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc.n_hidden[0]: %d outside 1..%d", d->n_hidden[0], DOCKAUV_POLICY_MAX_WIDTH);
    if (d->n_hidden[1] < 0 || d->n_hidden[1] > DOCKAUV_POLICY_MAX_WIDTH)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc.n_hidden[1]: %d outside 0..%d (0 = one hidden layer)", d->n_hidden[1], DOCKAUV_POLICY_MAX_WIDTH);
    if (d->n_out < 1 || d->n_out > DOCKAUV_MAX_U) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc.n_out: %d outside 1..%d", d->n_out, DOCKAUV_MAX_U);
    if (d->hidden_act != DOCKAUV_ACT_TANH && d->hidden_act != DOCKAUV_ACT_RELU)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc.hidden_act: %d is neither DOCKAUV_ACT_TANH nor DOCKAUV_ACT_RELU", d->hidden_act);
    if (d->pointers_on_device != 0 && d->pointers_on_device != 1)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc.pointers_on_device: %d must be 0 or 1", d->pointers_on_device);
    if (!d->W1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc.W1 is NULL");
    if (!d->b1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc.b1 is NULL");
    if (d->n_hidden[1] > 0 && !d->W2) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc.W2 is NULL (n_hidden[1] > 0)");
    if (d->n_hidden[1] > 0 && !d->b2) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc.b2 is NULL (n_hidden[1] > 0)");
    if (!d->W_mu) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc.W_mu is NULL");
    if (!d->b_mu) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc.b_mu is NULL");
    if (!d->W_ls) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc.W_ls is NULL");
    if (!d->b_ls) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc.b_ls is NULL");
    if (like && (d->n_in != like->n_in || d->n_hidden[0] != like->n_h1 || d->n_hidden[1] != like->n_h2 || d->n_out != like->n_out ||
                 d->hidden_act != like->hidden_act))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_load: n_in / n_hidden / n_out / hidden_act differ from the actor's (%d-%d-%d-%d)",
                    like->n_in, like->n_h1, like->n_h2, like->n_out);
    return 0;
}

// p->raw of a squashed-Gaussian actor: W1 b1 W2 b2, then the head array [16][n_last] and its bias [16] (rows 0 .. n_u - 1: mu,
// rows 8 .. 8 + n_u - 1: log_std, the rest zero since create).  Both heads are always copied there, host or device arrays.
int upload_sac_actor(dockauv_policy p, const dockauv_sac_actor_desc* d, hipStream_t stream) {
    dockauv_handle h = p->h;
    const PolicyShape& S = p->S;
    const int n_last = S.n_h2 ? S.n_h2 : S.n_h1;
    const hipMemcpyKind kind = d->pointers_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const float* src[4] = {d->W1, d->b1, d->W2, d->b2};
    const size_t cnt[4] = {(size_t)S.n_h1 * S.n_in, (size_t)S.n_h1, (size_t)S.n_h2 * S.n_h1, (size_t)S.n_h2};
    const float* dev[4];
    size_t off = 0;
    for (int i = 0; i < 4; ++i) {
        dev[i] = cnt[i] ? (d->pointers_on_device ? src[i] : p->raw + off) : nullptr;
        if (cnt[i] && !d->pointers_on_device) HIP_TRY(h, hipMemcpyAsync(p->raw + off, src[i], cnt[i] * sizeof(float), kind, stream));
        off += cnt[i];
    }
    float* heads = p->raw + off;
    float* head_b = heads + (size_t)kSacHeadRows * n_last;
    HIP_TRY(h, hipMemcpyAsync(heads, d->W_mu, (size_t)S.n_out * n_last * sizeof(float), kind, stream));
    HIP_TRY(h, hipMemcpyAsync(heads + (size_t)8 * n_last, d->W_ls, (size_t)S.n_out * n_last * sizeof(float), kind, stream));
    HIP_TRY(h, hipMemcpyAsync(head_b, d->b_mu, (size_t)S.n_out * sizeof(float), kind, stream));
    HIP_TRY(h, hipMemcpyAsync(head_b + 8, d->b_ls, (size_t)S.n_out * sizeof(float), kind, stream));
    if (!d->pointers_on_device) HIP_TRY(h, hipStreamSynchronize(stream));   // the caller's host arrays are free on return
    PolicyShape both = S;
    both.n_out = 8 + S.n_out;              // (the layout does not depend on n_out: the pack kernel's bound on the output units)
    const PolicyRaw raw{dev[0], dev[1], dev[2], dev[3], heads, head_b, nullptr};
    const int rc = launch_policy_pack(both, raw, p->packed, stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "policy weight packing launch failed: %s", hipGetErrorString((hipError_t)rc));
    p->has_log_std = true;
    p->seed = d->seed;
    p->env_id_offset = d->env_id_offset;
    return 0;
}

int check_q(dockauv_handle h, dockauv_policy c, const char* fn, const char* arg) {
    if (c->h != h) return fail(h, DOCKAUV_E_INVALID, "%s: %s was created for another handle", fn, arg);
    if (!c->q_role) return fail(h, DOCKAUV_E_INVALID, "%s: %s is not a Q critic (dockauv_q_create)", fn, arg);
    return 0;
}

}  // namespace

extern "C" {

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
    policy_layout(S);
    if (policy_lds_bytes(S) > kPolMaxLds)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_desc: the padded weights (%zu B for n_in %d, n_hidden %d / %d) exceed "
                    "the 160 KiB of LDS the policy kernel keeps them in: narrower layers", policy_lds_bytes(S), S.n_in, S.n_h1, S.n_h2);
    HIP_TRY(h, hipSetDevice(h->device));
    dockauv_policy p = new dockauv_policy_s();
    p->h = h;
    p->S = S;
    p->sac_role = true;
    const int n_last = S.n_h2 ? S.n_h2 : S.n_h1;
    const size_t raw_floats = (size_t)S.n_h1 * S.n_in + S.n_h1 + (size_t)S.n_h2 * S.n_h1 + S.n_h2 + (size_t)kSacHeadRows * (n_last + 1);
    hipError_t e = hipMalloc((void**)&p->packed, (size_t)S.total * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&p->raw, raw_floats * sizeof(float));
    if (e == hipSuccess) e = hipMemset(p->raw, 0, raw_floats * sizeof(float));
    if (e != hipSuccess) {
        dockauv_policy_destroy(p);
        return fail(h, DOCKAUV_E_HIP, "policy buffers: %s", hipGetErrorString(e));
    }
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
    if (!p->sac_role) return fail(p->h, DOCKAUV_E_INVALID, "dockauv_sac_actor_load: the policy is not a squashed-Gaussian actor (dockauv_sac_actor_create)");
    if (int rc = validate_sac_desc(p->h, d, &p->S)) return rc;
    HIP_TRY(p->h, hipSetDevice(p->h->device));
    return upload_sac_actor(p, d, (hipStream_t)hip_stream);
}

int dockauv_q_create(dockauv_handle h, const dockauv_policy_desc* d, dockauv_policy* out) {
    return create_policy(h, d, out, false, "dockauv_q_create", true);
}

int dockauv_q_forward(dockauv_handle h, dockauv_policy critic, const dockauv_q_io* io, void* hip_stream) {
    const char* fn = "dockauv_q_forward";
    if (!io) return fail(h, DOCKAUV_E_INVALID, "%s: io is NULL", fn);
    if (io->struct_size != sizeof(dockauv_q_io))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_q_io.struct_size: got %u, library has %zu", io->struct_size, sizeof(dockauv_q_io));
    if (io->n_rows < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_q_io.n_rows: %lld must be >= 1", io->n_rows);
    if (!io->obs) return fail(h, DOCKAUV_E_INVALID, "dockauv_q_io.obs is NULL");
    if (!io->actions) return fail(h, DOCKAUV_E_INVALID, "dockauv_q_io.actions is NULL");
    if (!io->q) return fail(h, DOCKAUV_E_INVALID, "dockauv_q_io.q is NULL");
    if (!critic) return fail(h, DOCKAUV_E_INVALID, "%s: null critic", fn);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (int rc = check_q(h, critic, fn, "the critic")) return rc;
    if (io->obs_stride < h->n_obs) return fail(h, DOCKAUV_E_INVALID, "dockauv_q_io.obs_stride: %d is below the handle's n_obs %d", io->obs_stride, h->n_obs);
    if (io->act_stride < h->n_u_max) return fail(h, DOCKAUV_E_INVALID, "dockauv_q_io.act_stride: %d is below the handle's n_u %d", io->act_stride, h->n_u_max);
    HIP_TRY(h, hipSetDevice(h->device));
    const QLaunch l{io->obs, io->actions, (const long long*)io->row_index, (const long long*)io->row_index, io->q, (long)io->n_rows,
                    io->obs_stride, io->act_stride, h->n_obs};
    const int rc = launch_q_forward(critic->S, critic->packed, l, hip_stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "Q kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = (hipStream_t)hip_stream;
    return 0;
}

int dockauv_sac_target(dockauv_handle h, dockauv_policy actor, dockauv_policy q1_target, dockauv_policy q2_target,
                       const dockauv_sac_target_io* io, void* hip_stream) {
    const char* fn = "dockauv_sac_target";
    if (!io) return fail(h, DOCKAUV_E_INVALID, "%s: io is NULL", fn);
    if (io->struct_size != sizeof(dockauv_sac_target_io))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_target_io.struct_size: got %u, library has %zu", io->struct_size, sizeof(dockauv_sac_target_io));
    if (io->n_rows < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_target_io.n_rows: %lld must be >= 1", io->n_rows);
    if (!(io->gamma >= 0.0f && io->gamma <= 1.0f)) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_target_io.gamma: %g outside [0, 1]", (double)io->gamma);
    if (!io->log_ent_coef && std::isnan(io->ent_coef)) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_target_io.ent_coef is NaN (and log_ent_coef is NULL)");
    if (!io->next_obs) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_target_io.next_obs is NULL");
    if (!io->rewards) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_target_io.rewards is NULL");
    if (!io->dones) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_target_io.dones is NULL");
    if (!io->a2) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_target_io.a2 is NULL");
    if (!io->logp2) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_target_io.logp2 is NULL");
    if (!io->q1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_target_io.q1 is NULL");
    if (!io->q2) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_target_io.q2 is NULL");
    if (!io->y) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_target_io.y is NULL");
    if (io->column_stride < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_target_io.column_stride: %d must be >= 1", io->column_stride);
    if (!actor) return fail(h, DOCKAUV_E_INVALID, "%s: null actor", fn);
    if (!q1_target || !q2_target) return fail(h, DOCKAUV_E_INVALID, "%s: null critic", fn);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (actor->h != h) return fail(h, DOCKAUV_E_INVALID, "%s: the actor was created for another handle", fn);
    if (!actor->sac_role) return fail(h, DOCKAUV_E_INVALID, "%s: the actor is not a squashed-Gaussian actor (dockauv_sac_actor_create)", fn);
    if (int rc = check_q(h, q1_target, fn, "q1_target")) return rc;
    if (int rc = check_q(h, q2_target, fn, "q2_target")) return rc;
    if (io->next_obs_stride < h->n_obs)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_target_io.next_obs_stride: %d is below the handle's n_obs %d", io->next_obs_stride, h->n_obs);
    HIP_TRY(h, hipSetDevice(h->device));
    const long n = (long)io->n_rows;
    const long long* index = (const long long*)io->row_index;
    const int n_u = h->n_u_max;
    const SacActorLaunch al{io->next_obs, index, io->a2, io->logp2, n, io->next_obs_stride, n_u, 1, io->t, io->row_offset, actor->seed, 5u};
    int rc = launch_sac_actor(actor->S, actor->packed, al, hip_stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "SAC actor kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    float* q_out[2] = {io->q1, io->q2};
    dockauv_policy qs[2] = {q1_target, q2_target};
    for (int i = 0; i < 2; ++i) {
        const QLaunch ql{io->next_obs, io->a2, index, nullptr, q_out[i], n, io->next_obs_stride, n_u, h->n_obs};
        if ((rc = launch_q_forward(qs[i]->S, qs[i]->packed, ql, hip_stream)) != 0)
            return fail(h, DOCKAUV_E_HIP, "Q kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    }
    const SacTargetLaunch tl{io->rewards, io->dones, io->timeouts, index, io->logp2, io->q1, io->q2, io->log_ent_coef, io->y, n,
                             io->column_stride, io->gamma, io->ent_coef};
    if ((rc = launch_sac_target_rows(tl, hip_stream)) != 0)
        return fail(h, DOCKAUV_E_HIP, "SAC target kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = (hipStream_t)hip_stream;
    return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ SAC: the networks' gradients (dockauv_backward.hip)
namespace {

// `p` must be this handle's squashed-Gaussian actor (sac) or Q critic (!sac): the three other roles by name
int check_sac_role(dockauv_handle h, dockauv_policy p, const char* fn, bool sac) {
    if (p->h != h) return fail(h, DOCKAUV_E_INVALID, "%s: the policy was created for another handle", fn);
    const char* want = sac ? "a squashed-Gaussian actor (dockauv_sac_actor_create)" : "a Q critic (dockauv_q_create)";
    if (p->value_role) return fail(h, DOCKAUV_E_INVALID, "%s: the policy is a value critic (dockauv_value_create), %s is needed", fn, want);
    if (p->sac_role && !sac) return fail(h, DOCKAUV_E_INVALID, "%s: the policy is a squashed-Gaussian actor (dockauv_sac_actor_create), %s is needed", fn, want);
    if (p->q_role && sac) return fail(h, DOCKAUV_E_INVALID, "%s: the policy is a Q critic (dockauv_q_create), %s is needed", fn, want);
    if (!p->sac_role && !p->q_role) return fail(h, DOCKAUV_E_INVALID, "%s: the policy is a plain actor (dockauv_policy_create), %s is needed", fn, want);
    return 0;
}

// the LDS need of the backward of `p` against the 160 KiB of a group
int check_backward_lds(dockauv_handle h, dockauv_policy p, const BackwardLayout& L, const char* fn) {
    if (backward_lds_bytes(L) > kPolMaxLds)
        return fail(h, DOCKAUV_E_INVALID, "%s: the kernel needs %zu B of LDS for n_in %d, n_hidden %d / %d (weights, one pass's rows, "
                    "activations and deltas), more than the 160 KiB of a group: narrower layers or observations",
                    fn, backward_lds_bytes(L), p->S.n_in, p->S.n_h1, p->S.n_h2);
    return 0;
}

}  // namespace

extern "C" {

int dockauv_sac_actor_forward_rows(dockauv_handle h, dockauv_policy actor, const dockauv_sac_rows_io* io, void* hip_stream) {
    const char* fn = "dockauv_sac_actor_forward_rows";
    if (!io) return fail(h, DOCKAUV_E_INVALID, "%s: io is NULL", fn);
    if (io->struct_size != sizeof(dockauv_sac_rows_io))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_rows_io.struct_size: got %u, library has %zu", io->struct_size, sizeof(dockauv_sac_rows_io));
    if (io->n_rows < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_rows_io.n_rows: %lld must be >= 1", io->n_rows);
    if (io->row_stride < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_rows_io.row_stride: %d is below every row width", io->row_stride);
    if (!io->rows) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_rows_io.rows is NULL");
    if (!io->out) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_rows_io.out is NULL");
    if (!actor) return fail(h, DOCKAUV_E_INVALID, "%s: null actor", fn);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (int rc = check_sac_role(h, actor, fn, true)) return rc;
    if (io->row_stride < h->n_obs) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_rows_io.row_stride: %d is below the handle's n_obs %d", io->row_stride, h->n_obs);
    HIP_TRY(h, hipSetDevice(h->device));
    const int rc = launch_sac_actor_heads(actor->S, actor->packed, io->rows, (const long long*)io->row_index, (long)io->n_rows, io->row_stride,
                                          io->out, hip_stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "SAC actor heads kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = (hipStream_t)hip_stream;
    return 0;
}

int dockauv_sac_actor_backward(dockauv_handle h, dockauv_policy actor, const dockauv_sac_actor_backward_io* io, void* hip_stream) {
    const char* fn = "dockauv_sac_actor_backward";
    if (!io) return fail(h, DOCKAUV_E_INVALID, "%s: io is NULL", fn);
    if (io->struct_size != sizeof(dockauv_sac_actor_backward_io))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_backward_io.struct_size: got %u, library has %zu", io->struct_size,
                    sizeof(dockauv_sac_actor_backward_io));
    if (io->n_rows < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_backward_io.n_rows: %lld must be >= 1", io->n_rows);
    if (io->row_stride < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_backward_io.row_stride: %d is below every row width", io->row_stride);
    if (!io->rows) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_backward_io.rows is NULL");
    if (!io->grad_out) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_backward_io.grad_out is NULL");
    if (!io->dW1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_backward_io.dW1 is NULL");
    if (!io->db1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_backward_io.db1 is NULL");
    if (!io->dW_mu) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_backward_io.dW_mu is NULL");
    if (!io->db_mu) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_backward_io.db_mu is NULL");
    if (!io->dW_ls) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_backward_io.dW_ls is NULL");
    if (!io->db_ls) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_backward_io.db_ls is NULL");
    if (!actor) return fail(h, DOCKAUV_E_INVALID, "%s: null actor", fn);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (int rc = check_sac_role(h, actor, fn, true)) return rc;
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
    const int rc = launch_sac_actor_backward(actor->S, actor->packed, l, actor->bwd_partial, g, hip_stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "SAC actor backward launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = (hipStream_t)hip_stream;
    return 0;
}

int dockauv_q_backward(dockauv_handle h, dockauv_policy critic, const dockauv_q_backward_io* io, void* hip_stream) {
    const char* fn = "dockauv_q_backward";
    if (!io) return fail(h, DOCKAUV_E_INVALID, "%s: io is NULL", fn);
    if (io->struct_size != sizeof(dockauv_q_backward_io))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_q_backward_io.struct_size: got %u, library has %zu", io->struct_size, sizeof(dockauv_q_backward_io));
    if (io->n_rows < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_q_backward_io.n_rows: %lld must be >= 1", io->n_rows);
    if (io->obs_stride < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_q_backward_io.obs_stride: %d is below every row width", io->obs_stride);
    if (io->act_stride < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_q_backward_io.act_stride: %d is below every row width", io->act_stride);
    if (!io->obs) return fail(h, DOCKAUV_E_INVALID, "dockauv_q_backward_io.obs is NULL");
    if (!io->actions) return fail(h, DOCKAUV_E_INVALID, "dockauv_q_backward_io.actions is NULL");
    if (!io->grad_q) return fail(h, DOCKAUV_E_INVALID, "dockauv_q_backward_io.grad_q is NULL");
    if (!io->grads && !io->grad_actions)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_q_backward_io: grads and grad_actions are both NULL, at least one output is required");
    const dockauv_policy_grads* gr = io->grads;
    if (gr && gr->struct_size != sizeof(dockauv_policy_grads))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_grads.struct_size: got %u, library has %zu", gr->struct_size, sizeof(dockauv_policy_grads));
    if (gr && (!gr->dW1 || !gr->db1 || !gr->dW3 || !gr->db3))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_policy_grads: dW1/db1/dW3/db3 must not be NULL");
    if (!critic) return fail(h, DOCKAUV_E_INVALID, "%s: null critic", fn);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (int rc = check_sac_role(h, critic, fn, false)) return rc;
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
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "Q backward launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = (hipStream_t)hip_stream;
    return 0;
}

int dockauv_policy_backward_workspace(dockauv_policy p, float** partial, long long* n_floats) {
    if (!p) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_policy_backward_workspace: null policy");
    BackwardLayout L;                                   // (the role fixes the partial's size)
    if (p->sac_role) sac_actor_backward_layout(p->S, L);
    else backward_layout(p->S, L);
    if (partial) *partial = p->bwd_partial;
    if (n_floats) *n_floats = p->bwd_partial ? (long long)kBwdMaxGroups * L.n_params : 0;
    return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ SAC: the loss head (dockauv_sac_head.hip)
namespace {

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

}  // namespace

extern "C" {

int dockauv_sac_sample(dockauv_handle h, dockauv_policy actor, const dockauv_sac_sample_io* io, void* hip_stream) {
    const char* fn = "dockauv_sac_sample";
    if (!io) return fail(h, DOCKAUV_E_INVALID, "%s: io is NULL", fn);
    if (io->struct_size != sizeof(dockauv_sac_sample_io))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_sample_io.struct_size: got %u, library has %zu", io->struct_size, sizeof(dockauv_sac_sample_io));
    if (io->n_rows < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_sample_io.n_rows: %lld must be >= 1", io->n_rows);
    if (!io->heads) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_sample_io.heads is NULL");
    if (!io->a) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_sample_io.a is NULL");
    if (!io->logp) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_sample_io.logp is NULL");
    if (!actor) return fail(h, DOCKAUV_E_INVALID, "%s: null actor", fn);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (int rc = check_sac_role(h, actor, fn, true)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const SacSampleLaunch l{io->heads, io->a, io->logp, (long)io->n_rows, actor->S.n_out, (unsigned int)(io->t & 0xffffffffull),
                            (unsigned int)(io->row_offset & 0xffffffffull), actor->seed};
    const int rc = launch_sac_sample(l, hip_stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "SAC sample kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = (hipStream_t)hip_stream;
    return 0;
}

int dockauv_sac_critic_head(dockauv_handle h, dockauv_policy q1_critic, const dockauv_sac_critic_head_io* io, void* hip_stream) {
    const char* fn = "dockauv_sac_critic_head";
    if (!io) return fail(h, DOCKAUV_E_INVALID, "%s: io is NULL", fn);
    if (io->struct_size != sizeof(dockauv_sac_critic_head_io))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_critic_head_io.struct_size: got %u, library has %zu", io->struct_size,
                    sizeof(dockauv_sac_critic_head_io));
    if (io->n_rows < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_critic_head_io.n_rows: %lld must be >= 1", io->n_rows);
    if (!io->q1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_critic_head_io.q1 is NULL");
    if (!io->q2) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_critic_head_io.q2 is NULL");
    if (!io->y) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_critic_head_io.y is NULL");
    if (!io->grad_q1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_critic_head_io.grad_q1 is NULL");
    if (!io->grad_q2) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_critic_head_io.grad_q2 is NULL");
    if (!io->stats) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_critic_head_io.stats is NULL");
    const long long B = io->n_rows;
    const FloatSpan out[3] = {{"grad_q1", io->grad_q1, B}, {"grad_q2", io->grad_q2, B}, {"stats", io->stats, 6}};
    const FloatSpan in[3] = {{"q1", io->q1, B}, {"q2", io->q2, B}, {"y", io->y, B}};
    if (int rc = refuse_overlap(h, "dockauv_sac_critic_head_io", out, 3, in, 3)) return rc;
    if (!q1_critic) return fail(h, DOCKAUV_E_INVALID, "%s: null critic", fn);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (int rc = check_sac_role(h, q1_critic, fn, false)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const SacCriticHeadLaunch l{io->q1, io->q2, io->y, io->grad_q1, io->grad_q2, io->stats, (long)B};
    const int rc = launch_sac_critic_head(l, hip_stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "SAC critic head kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = (hipStream_t)hip_stream;
    return 0;
}

int dockauv_sac_actor_head(dockauv_handle h, dockauv_policy actor, const dockauv_sac_actor_head_io* io, void* hip_stream) {
    const char* fn = "dockauv_sac_actor_head";
    if (!io) return fail(h, DOCKAUV_E_INVALID, "%s: io is NULL", fn);
    if (io->struct_size != sizeof(dockauv_sac_actor_head_io))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_head_io.struct_size: got %u, library has %zu", io->struct_size,
                    sizeof(dockauv_sac_actor_head_io));
    if (io->n_rows < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_head_io.n_rows: %lld must be >= 1", io->n_rows);
    if (!io->log_ent_coef && std::isnan(io->ent_coef))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_head_io.ent_coef is NaN (and log_ent_coef is NULL)");
    if (!io->heads) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_head_io.heads is NULL");
    if (!io->q1_pi) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_head_io.q1_pi is NULL");
    if (!io->q2_pi) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_head_io.q2_pi is NULL");
    if (!io->dq1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_head_io.dq1 is NULL");
    if (!io->dq2) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_head_io.dq2 is NULL");
    if (!io->grad_out) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_head_io.grad_out is NULL");
    if (!io->stats) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_actor_head_io.stats is NULL");
    if (int rc = refuse_actor_head_overlap(h, io, 1)) return rc;
    if (!actor) return fail(h, DOCKAUV_E_INVALID, "%s: null actor", fn);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (int rc = check_sac_role(h, actor, fn, true)) return rc;
    if (int rc = refuse_actor_head_overlap(h, io, actor->S.n_out)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const SacActorHeadLaunch l{io->heads, io->q1_pi, io->q2_pi, io->dq1, io->dq2, io->log_ent_coef, io->grad_out, io->stats, (long)io->n_rows,
                               actor->S.n_out, (unsigned int)(io->t & 0xffffffffull), (unsigned int)(io->row_offset & 0xffffffffull),
                               actor->seed, io->ent_coef};
    const int rc = launch_sac_actor_head(l, hip_stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "SAC actor head kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = (hipStream_t)hip_stream;
    return 0;
}

int dockauv_sac_ent_coef_step(dockauv_handle h, const dockauv_sac_ent_coef_io* io, void* hip_stream) {
    const char* fn = "dockauv_sac_ent_coef_step";
    if (!io) return fail(h, DOCKAUV_E_INVALID, "%s: io is NULL", fn);
    if (io->struct_size != sizeof(dockauv_sac_ent_coef_io))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_ent_coef_io.struct_size: got %u, library has %zu", io->struct_size,
                    sizeof(dockauv_sac_ent_coef_io));
    if (io->n_rows < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_ent_coef_io.n_rows: %lld must be >= 1", io->n_rows);
    if (io->step < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_ent_coef_io.step: %lld must be >= 1 (the caller's count of this step)", io->step);
    if (!(io->lr >= 0.0) || !std::isfinite(io->lr)) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_ent_coef_io.lr: %g must be finite and >= 0", io->lr);
    if (!(io->beta1 >= 0.0 && io->beta1 < 1.0)) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_ent_coef_io.beta1: %g outside [0, 1)", io->beta1);
    if (!(io->beta2 >= 0.0 && io->beta2 < 1.0)) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_ent_coef_io.beta2: %g outside [0, 1)", io->beta2);
    if (!(io->eps > 0.0)) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_ent_coef_io.eps: %g must be > 0", io->eps);
    if (!io->state) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_ent_coef_io.state is NULL");
    if (!io->logp) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_ent_coef_io.logp is NULL");
    if (io->before && floats_overlap(io->before, 1, io->state, 3))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_ent_coef_io.before overlaps state: it receives the value from before the step");
    if (io->stats && floats_overlap(io->stats, 4, io->state, 3)) return fail(h, DOCKAUV_E_INVALID, "dockauv_sac_ent_coef_io.stats overlaps state");
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    HIP_TRY(h, hipSetDevice(h->device));
    // step's scalars in double, rounded once (include/dockauv.h: dockauv_optim_step)
    EntCoefLaunch l{io->state, io->logp, io->before, io->stats, (long)io->n_rows, io->target_entropy};
    l.c1 = (float)(1.0 - io->beta1);
    l.c2 = (float)(1.0 - io->beta2);
    l.b2 = (float)io->beta2;
    l.step_size = (float)(io->lr / (1.0 - std::pow(io->beta1, (double)io->step)));
    l.rsq = (float)(1.0 / std::sqrt(1.0 - std::pow(io->beta2, (double)io->step)));
    l.eps = (float)io->eps;
    const int rc = launch_ent_coef_step(l, hip_stream);
    if (rc != 0) return fail(h, DOCKAUV_E_HIP, "ent_coef step kernel launch failed: %s", hipGetErrorString((hipError_t)rc));
    h->last_stream = (hipStream_t)hip_stream;
    return 0;
}

}  // extern "C"
