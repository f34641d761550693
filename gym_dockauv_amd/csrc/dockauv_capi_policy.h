// dockauv_capi_policy.h -- what the C ABI's network files share (dockauv_capi_policy.hip, dockauv_capi_collect.hip,
// dockauv_capi_optim.hip, dockauv_capi_sac.hip): the policy object and its role, the role checks, the descriptor trunk, construction and
// the forward launches.  Internal to libdockauv.so.
#pragma once
#include <cmath>

#include "dockauv_capi.h"

namespace dockauv {

// what a dockauv_policy is; the creating call fixes it
enum class Role { Actor, Value, SacActor, Q };

// each role in the messages' words: `named` tells the four apart, `ppo` is the wording of the calls that predate SAC
struct RolePhrase {
    const char* named;
    const char* ppo;
};
constexpr RolePhrase kRolePhrase[4] = {
    {"a plain actor (dockauv_policy_create)", "an actor (dockauv_policy_create)"},
    {"a value critic (dockauv_value_create)", "a critic (dockauv_value_create)"},
    {"a squashed-Gaussian actor (dockauv_sac_actor_create)", "a squashed-Gaussian actor (dockauv_sac_actor_create)"},
    {"a Q critic (dockauv_q_create)", "a Q critic (dockauv_q_create)"},
};
inline const RolePhrase& phrase(Role r) { return kRolePhrase[(int)r]; }
inline bool is_critic(Role r) { return r == Role::Value || r == Role::Q; }   // n_out == 1, raw output, no exploration noise

constexpr int kSacHeadRows = 16;   // the [8 + n_u][n_last] array both heads are packed from, padded to the two register groups

}  // namespace dockauv

struct dockauv_policy_s {
    dockauv_handle h = nullptr;
    dockauv::PolicyShape S{};
    float* packed = nullptr;      // the weights as the kernel reads them (dockauv_device.h: PolicyShape)
    float* raw = nullptr;         // device staging of host arrays: W1 b1 W2 b2 W3 b3 log_std back to back
    float* log_std = nullptr;     // the raw log_std [DOCKAUV_MAX_U] (the packed image keeps exp(log_std)): read by the log-prob epilogue
    bool has_log_std = false;
    // Actor: dockauv_policy_create.  Value: dockauv_value_create, n_out == 1, raw output.  SacActor: dockauv_sac_actor_create, both heads
    // in the output tile, out_act TANH.  Q: dockauv_q_create, n_in == n_obs + n_u, n_out == 1, raw output
    dockauv::Role role = dockauv::Role::Actor;
    uint64_t seed = 0, env_id_offset = 0;
    float* bwd_partial = nullptr; // dockauv_policy_backward's per-group partial sums, allocated by the first backward
    double* head_ws = nullptr;    // dockauv_ppo_head's moment and row-sum partials (kHeadWorkspaceBytes), allocated by the first head call
};

namespace dockauv {

// ---- the role checks.  Every one starts with the handle the object was created for.

// what the actor argument of `fn` must be: of this handle, not a critic; with want_logp also a log_std and a raw output.
// ppo (everything but forward / forward_logp / rollout): a squashed-Gaussian actor is refused by name
inline int check_actor(dockauv_handle h, dockauv_policy p, const char* fn, bool want_logp, bool ppo = true) {
    if (p->h != h) return fail(h, DOCKAUV_E_INVALID, "%s: the policy was created for another handle", fn);
    if (is_critic(p->role)) return fail(h, DOCKAUV_E_INVALID, "%s: the policy is %s, an actor is needed", fn, phrase(p->role).ppo);
    if (p->role == Role::SacActor && ppo)
        return fail(h, DOCKAUV_E_INVALID, "%s: the policy is %s; this call is PPO's and takes %s", fn, phrase(p->role).named,
                    phrase(Role::Actor).named);
    if (p->role == Role::SacActor) return 0;   // (its log-probability carries the squashing correction)
    if (want_logp && !p->has_log_std) return fail(h, DOCKAUV_E_INVALID, "%s: log_prob needs a policy with a log_std", fn);
    if (want_logp && p->S.out_act == DOCKAUV_ACT_TANH)
        return fail(h, DOCKAUV_E_INVALID, "%s: log_prob of a policy with out_act DOCKAUV_ACT_TANH needs the squashing correction, "
                    "which stays with the learner", fn);
    return 0;
}

// the SAC roles by name, for the calls whose arithmetic is the plain MLP's or PPO's
inline int refuse_sac(dockauv_handle h, dockauv_policy p, const char* fn) {
    if (p->role == Role::SacActor || p->role == Role::Q)
        return fail(h, DOCKAUV_E_INVALID, "%s: the policy is %s, which this call does not take", fn, phrase(p->role).named);
    return 0;
}

inline int check_critic(dockauv_handle h, dockauv_policy c, const char* fn) {
    if (c->h != h) return fail(h, DOCKAUV_E_INVALID, "%s: the critic was created for another handle", fn);
    if (c->role == Role::Q) return fail(h, DOCKAUV_E_INVALID, "%s: the critic argument is %s, a value critic is needed", fn, phrase(c->role).named);
    if (c->role != Role::Value) return fail(h, DOCKAUV_E_INVALID, "%s: the critic argument is %s, not a critic", fn, phrase(c->role).ppo);
    return 0;
}

// `p` must be this handle's `want`: any other role is named.  The sentence of SAC's calls with one network (forward_rows, the two
// backwards, sample, the two heads): "the policy is X, Y is needed"
inline int check_role(dockauv_handle h, dockauv_policy p, const char* fn, Role want) {
    if (p->h != h) return fail(h, DOCKAUV_E_INVALID, "%s: the policy was created for another handle", fn);
    if (p->role != want) return fail(h, DOCKAUV_E_INVALID, "%s: the policy is %s, %s is needed", fn, phrase(p->role).named, phrase(want).named);
    return 0;
}

// the same in the sentence of dockauv_q_forward and dockauv_sac_target, which say which argument: "<arg> is not Y"; `arg`: what the
// message calls this one ("the critic", "the actor", "q1_target")
inline int check_is(dockauv_handle h, dockauv_policy p, const char* fn, const char* arg, Role want) {
    if (p->h != h) return fail(h, DOCKAUV_E_INVALID, "%s: %s was created for another handle", fn, arg);
    if (p->role != want) return fail(h, DOCKAUV_E_INVALID, "%s: %s is not %s", fn, arg, phrase(want).named);
    return 0;
}

// the LDS need of the backward of `p` against the 160 KiB of a group
inline int check_backward_lds(dockauv_handle h, dockauv_policy p, const BackwardLayout& L, const char* fn) {
    if (backward_lds_bytes(L) > kPolMaxLds)
        return fail(h, DOCKAUV_E_INVALID, "%s: the kernel needs %zu B of LDS for n_in %d, n_hidden %d / %d (weights, one pass's rows, "
                    "activations and deltas), more than the 160 KiB of a group: narrower layers or observations",
                    fn, backward_lds_bytes(L), p->S.n_in, p->S.n_h1, p->S.n_h2);
    return 0;
}

// ---- the trunk dockauv_policy_desc and dockauv_sac_actor_desc share, `name`: the struct's.  Two parts, since dockauv_policy_desc checks
// its out_act between them

template <class D>
int validate_trunk_numbers(dockauv_handle h, const D* d, const char* name) {
    if (int rc = check_size(h, d, name)) return rc;
    if (d->precision != DOCKAUV_F32) return fail(h, DOCKAUV_E_INVALID, "%s.precision: %d, only DOCKAUV_F32 is implemented", name, d->precision);
    if (d->n_in < 1) return fail(h, DOCKAUV_E_INVALID, "%s.n_in: %d must be >= 1", name, d->n_in);
    if (d->n_hidden[0] < 1 || d->n_hidden[0] > DOCKAUV_POLICY_MAX_WIDTH)
        return fail(h, DOCKAUV_E_INVALID, "%s.n_hidden[0]: %d outside 1..%d", name, d->n_hidden[0], DOCKAUV_POLICY_MAX_WIDTH);
    if (d->n_hidden[1] < 0 || d->n_hidden[1] > DOCKAUV_POLICY_MAX_WIDTH)
        return fail(h, DOCKAUV_E_INVALID, "%s.n_hidden[1]: %d outside 0..%d (0 = one hidden layer)", name, d->n_hidden[1], DOCKAUV_POLICY_MAX_WIDTH);
    if (d->n_out < 1 || d->n_out > DOCKAUV_MAX_U) return fail(h, DOCKAUV_E_INVALID, "%s.n_out: %d outside 1..%d", name, d->n_out, DOCKAUV_MAX_U);
    if (d->hidden_act != DOCKAUV_ACT_TANH && d->hidden_act != DOCKAUV_ACT_RELU)
        return fail(h, DOCKAUV_E_INVALID, "%s.hidden_act: %d is neither DOCKAUV_ACT_TANH nor DOCKAUV_ACT_RELU", name, d->hidden_act);
    return 0;
}

template <class D>
int validate_trunk_arrays(dockauv_handle h, const D* d, const char* name) {
    if (d->pointers_on_device != 0 && d->pointers_on_device != 1)
        return fail(h, DOCKAUV_E_INVALID, "%s.pointers_on_device: %d must be 0 or 1", name, d->pointers_on_device);
    if (int rc = require(h, name, {{"W1", d->W1}, {"b1", d->b1}})) return rc;
    if (d->n_hidden[1] > 0 && !d->W2) return fail(h, DOCKAUV_E_INVALID, "%s.W2 is NULL (n_hidden[1] > 0)", name);
    if (d->n_hidden[1] > 0 && !d->b2) return fail(h, DOCKAUV_E_INVALID, "%s.b2 is NULL (n_hidden[1] > 0)", name);
    return 0;
}

// does the trunk of `d` have the shape of `like` (a reload)?  The output activation is the caller's to compare
template <class D>
bool trunk_matches(const D* d, const PolicyShape& like) {
    return d->n_in == like.n_in && d->n_hidden[0] == like.n_h1 && d->n_hidden[1] == like.n_h2 && d->n_out == like.n_out &&
           d->hidden_act == like.hidden_act;
}

// lengths of W1 b1 W2 b2 W3 b3 of a network, torch.nn.Linear layout; returns the width its output layer reads
inline int layer_lengths(const PolicyShape& S, int* len) {
    const int n_last = S.n_h2 ? S.n_h2 : S.n_h1;
    len[0] = S.n_h1 * S.n_in;
    len[1] = S.n_h1;
    len[2] = S.n_h2 * S.n_h1;
    len[3] = S.n_h2;
    len[4] = S.n_out * n_last;
    len[5] = S.n_out;
    return n_last;
}

// step t's two Adam bias corrections, in double, rounded once (include/dockauv.h: dockauv_optim_step)
inline void bias_corrections(double beta1, double beta2, double lr, long long t, float& step_size, float& rsq) {
    step_size = (float)(lr / (1.0 - std::pow(beta1, (double)t)));
    rsq = (float)(1.0 / std::sqrt(1.0 - std::pow(beta2, (double)t)));
}

// ---- dockauv_capi_policy.hip

// A new object of `role` for the numbers of a validated descriptor `desc_name` (n_in, n_h1, n_h2, n_out and the activations of S):
// the layout, the refusal on LDS size, packed and raw (a squashed-Gaussian actor's raw zeroed, every other role with a zeroed
// log_std).  Nothing is left behind on failure
int new_policy(dockauv_handle h, Role role, PolicyShape S, const char* desc_name, dockauv_policy* out);
// weights of `d` -> p->packed, ordered on `stream`; host arrays go through p->raw and the call waits for the copies
int upload_policy(dockauv_policy p, const dockauv_policy_desc* d, hipStream_t stream);
// the actor's step of a rollout; log_prob (nullable, [n_envs]): the actor in its log-prob form
int policy_forward(dockauv_handle h, dockauv_policy p, const float* rows, float* actions, uint64_t t, int stochastic, hipStream_t stream,
                   float* log_prob = nullptr);
// V(rows[r]) for n_rows packed rows -> values[r]
int value_forward(dockauv_handle h, dockauv_policy c, const float* rows, long long n_rows, float* values, hipStream_t stream);
// the launches of dockauv_rollout; log_prob (nullable, [n_steps][n_envs]): the actor in its log-prob form
int queue_rollout(dockauv_handle h, dockauv_policy p, const float* rows_in, float* rows_out, float* actions_out, float* terminal_obs,
                  float* log_prob, int n_steps, uint64_t t0, int stochastic, hipStream_t stream);
// the head launches' arguments from the io block; the workspace is the actor's
void head_args(dockauv_policy actor, const dockauv_ppo_head_io* io, HeadArgs& a);

}  // namespace dockauv
