// dockauv_capi_collect.hip -- C ABI of libdockauv.so (include/dockauv.h), the PPO collector's part: GAE, time-limit truncation, the
// three collect calls, the episode monitor and the reward normaliser.
// The kernels are in dockauv_collect / _monitor / _rewnorm.hip.
#include "dockauv_capi_policy.h"

using namespace dockauv;

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

int check_gae_factors(dockauv_handle h, const char* fn, float gamma, float gae_lambda) {
    if (!(gamma >= 0.0f && gamma <= 1.0f)) return fail(h, DOCKAUV_E_INVALID, "%s: gamma %g outside [0, 1]", fn, (double)gamma);
    if (!(gae_lambda >= 0.0f && gae_lambda <= 1.0f)) return fail(h, DOCKAUV_E_INVALID, "%s: gae_lambda %g outside [0, 1]", fn, (double)gae_lambda);
    return 0;
}

// a dockauv_truncation_io against the handle, before any device call; `full`: also what the value launch and GAE touch
int check_truncation(dockauv_handle h, const dockauv_truncation_io* io, const char* fn, bool full) {
    const char* io_name = "dockauv_truncation_io";
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (int rc = check_block(h, io, fn, "io", io_name)) return rc;
    if (io->n_steps < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.n_steps: %d must be >= 1", io->n_steps);
    if (h->cfg.max_timesteps < 1) return fail(h, DOCKAUV_E_INVALID, "%s: the handle's max_timesteps %d must be >= 1", fn, h->cfg.max_timesteps);
    const int need = truncation_slots(io->n_steps, h->cfg.max_timesteps);
    if (io->n_slots < need)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_truncation_io.n_slots: %d, dockauv_truncation_slots gives %d for %d steps", io->n_slots, need, io->n_steps);
    if (int rc = require(h, io_name, {{"rows_out", io->rows_out}, {"terminal_obs", io->terminal_obs}, {"length_carry", io->length_carry},
                                      {"trunc_step", io->trunc_step}, {"trunc_row", io->trunc_row}}))
        return rc;
    if (full) {
        if (int rc = require(h, io_name, {{"values", io->values}, {"v_terminal", io->v_terminal}, {"advantages", io->advantages},
                                          {"returns", io->returns}}))
            return rc;
        if (int rc = check_gae_factors(h, io_name, io->gamma, io->gae_lambda)) return rc;
    }
    if (int rc = refuse_f64_rows(h, fn)) return rc;
    return refuse_reset_none(h, fn);
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
    return launched(h, "truncation scan", launch_truncation_scan(a, stream), stream);
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
        if (rc != 0) return launch_failed(h, "value kernel", rc);
        g.trunc_step = tio->trunc_step;
        g.v_terminal = tio->v_terminal;
        g.n_slots = tio->n_slots;
    }
    return launched(h, "GAE kernel", launch_gae(g, stream), stream);
}

// a dockauv_rewnorm_io on its own, before any device call and before the handle is looked at
int check_rewnorm_io(dockauv_handle h, const dockauv_rewnorm_io* io, const char* fn) {
    const char* io_name = "dockauv_rewnorm_io";
    if (int rc = check_block(h, io, fn, "the dockauv_rewnorm_io", io_name)) return rc;
    if (io->n_steps < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_io.n_steps: %d must be >= 1", io->n_steps);
    if (int rc = require(h, io_name, {{"rows_out", io->rows_out}, {"reward_norm", io->reward_norm}})) return rc;
    if (io->training && !io->discounted) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_io.discounted is NULL (required when training)");
    if (io->training && !io->step_stats) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_io.step_stats is NULL (required when training)");
    return 0;
}

// handle and normaliser of `fn`, after the argument blocks
int check_rewnorm(dockauv_handle h, dockauv_rewnorm rn, const char* fn) {
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (!rn) return fail(h, DOCKAUV_E_INVALID, "%s: null normaliser", fn);
    if (int rc = refuse_f64_rows(h, fn)) return rc;
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
    return launched(h, "reward normalisation", launch_rewnorm_scan(a, stream), stream);
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
    if (int rc = check_block(h, io, fn, arg, "dockauv_collect_io")) return rc;
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

}  // namespace

extern "C" {

int dockauv_gae(dockauv_handle h, const float* rows_out, const float* values, int n_steps, float gamma, float gae_lambda,
                float* advantages, float* returns, void* hip_stream) {
    if (!rows_out || !values || !advantages || !returns)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_gae: rows_out/values/advantages/returns must not be NULL");
    if (n_steps < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_gae: n_steps %d must be >= 1", n_steps);
    if (int rc = check_gae_factors(h, "dockauv_gae", gamma, gae_lambda)) return rc;
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_gae: null handle");
    if (int rc = refuse_f64_rows(h, "dockauv_gae")) return rc;
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

int dockauv_monitor_create(dockauv_handle h, dockauv_monitor* out) {
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_monitor_create: null handle");
    if (!out) return fail(h, DOCKAUV_E_INVALID, "dockauv_monitor_create: out is NULL");
    *out = nullptr;
    if (int rc = refuse_f64_rows(h, "dockauv_monitor_create")) return rc;
    if (int rc = refuse_reset_none(h, "dockauv_monitor_create")) return rc;
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
    const char* fn = "dockauv_monitor_scan";
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "%s: null handle", fn);
    if (!m) return fail(h, DOCKAUV_E_INVALID, "%s: null monitor", fn);
    if (int rc = check_block(h, io, fn, "io", "dockauv_monitor_io")) return rc;
    if (io->n_steps < 1) return fail(h, DOCKAUV_E_INVALID, "dockauv_monitor_io.n_steps: %d must be >= 1", io->n_steps);
    if (int rc = require(h, "dockauv_monitor_io", {{"rows_out", io->rows_out}, {"stats", io->stats}})) return rc;
    if (io->ep_outcome && !io->terminal_obs)
        return fail(h, DOCKAUV_E_INVALID, "dockauv_monitor_io.ep_outcome needs terminal_obs (the outcome is read off the terminal observation)");
    if ((io->values == nullptr) != (io->returns == nullptr))
        return fail(h, DOCKAUV_E_INVALID, "dockauv_monitor_io.values / returns: both or neither must be NULL (NULL: no explained variance)");
    if (int rc = refuse_f64_rows(h, fn)) return rc;
    if (int rc = refuse_reset_none(h, fn)) return rc;
    if (m->h != h) return fail(h, DOCKAUV_E_INVALID, "%s: the monitor was created for another handle", fn);
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
    return launched(h, "monitor", launch_monitor_scan(a, hip_stream), hip_stream);
}

int dockauv_rewnorm_create(dockauv_handle h, float gamma, float clip_reward, double epsilon, dockauv_rewnorm* out) {
    if (!out) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_create: out is NULL");
    *out = nullptr;
    if (!(gamma >= 0.0f && gamma <= 1.0f)) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_create: gamma %g outside [0, 1]", (double)gamma);
    if (!(clip_reward > 0.0f)) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_create: clip_reward %g must be > 0", (double)clip_reward);
    if (!(epsilon >= 0.0)) return fail(h, DOCKAUV_E_INVALID, "dockauv_rewnorm_create: epsilon %g must be >= 0", epsilon);
    if (!h) return fail(nullptr, DOCKAUV_E_INVALID, "dockauv_rewnorm_create: null handle");
    if (int rc = refuse_f64_rows(h, "dockauv_rewnorm_create")) return rc;
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
        return launch_failed(h, "reward normaliser reset", rc);
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
    return launched(h, "reward normaliser reset", launch_rewnorm_reset(rn->carry, rn->state, h->cfg.n_envs, hip_stream), hip_stream);
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
    if (int rc = refuse_f64_rows(h, fn)) return rc;
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
