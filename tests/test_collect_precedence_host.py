"""
Which refusal wins, host side (no GPU): the six collector entry points -- dockauv_gae, dockauv_gae_truncated, dockauv_gae_normalized,
dockauv_collect, dockauv_collect_truncated, dockauv_collect_normalized -- validate their arguments in different orders, and callers
see that order through the message of a call that is wrong twice.  Every row below is such a call: a NULL handle plus fake pointers
that are never dereferenced, two defects drawn from what is checked before the handle is looked into, and the message that must be
reported -- that of the defect checked first.  The rows cover every adjacent pair of each function's order of checks.  The checks
behind the handle (a foreign actor, n_slots, a truncation block that does not match, the normaliser's gamma) are pinned the same way
by the test_refusals_on_a_live_handle of tests/test_gpu_collect.py, test_gpu_truncation.py and test_gpu_rewnorm.py.
"""
import ctypes as C

import pytest

FAKE = 8          # an actor, critic or normaliser: never dereferenced, the calls are refused first
K = 4


@pytest.fixture(scope="module")
def lib():
    from gym_dockauv_amd.csrc import build
    build.build()
    from gym_dockauv_amd import _capi
    return _capi.load_library()


def blocks(cio=None, tio=None, nio=None):
    """a dockauv_collect_io, dockauv_truncation_io and dockauv_rewnorm_io that agree, every pointer a small fake address; the
    dicts overwrite fields (None: a NULL pointer)"""
    from gym_dockauv_amd import _capi
    fake = lambda i: 64 * (i + 1)
    c = _capi.CollectIO()
    c.struct_size, c.n_steps = C.sizeof(_capi.CollectIO), K
    c.rows_in, c.rows_out, c.actions_out, c.terminal_obs = fake(0), fake(1), fake(2), fake(3)
    c.values, c.advantages, c.returns = fake(4), fake(5), fake(6)
    c.gamma, c.gae_lambda = 0.99, 0.95
    t = _capi.TruncationIO()
    t.struct_size, t.n_steps, t.n_slots = C.sizeof(_capi.TruncationIO), K, 1
    t.gamma, t.gae_lambda = 0.99, 0.95
    t.rows_out, t.terminal_obs, t.values, t.advantages, t.returns = fake(1), fake(3), fake(4), fake(5), fake(6)
    t.length_carry, t.trunc_step, t.trunc_row, t.v_terminal = fake(7), fake(8), fake(9), fake(13)
    n = _capi.RewnormIO()
    n.struct_size, n.n_steps, n.training = C.sizeof(_capi.RewnormIO), K, 1
    n.rows_out, n.reward_norm, n.discounted, n.step_stats = fake(1), fake(10), fake(11), fake(12)
    for block, over in ((c, cio), (t, tio), (n, nio)):
        for name, value in (over or {}).items():
            setattr(block, name, value)
    return c, t, n


ref = lambda block, given: C.byref(block) if given else None
ptr = lambda x: C.c_void_p(x or None)


# ------------------------------------------------------------------------------------------------------- the three GAE calls
def call_gae(lib, rows=128, val=256, n_steps=K, gamma=0.99, lam=0.95, adv=320, ret=384):
    return lib.dockauv_gae(None, ptr(rows), ptr(val), n_steps, gamma, lam, ptr(adv), ptr(ret), None)


def call_gae_truncated(lib, critic=FAKE, io=True, tio=None):
    return lib.dockauv_gae_truncated(None, ptr(critic), ref(blocks(tio=tio)[1], io), None)


def call_gae_normalized(lib, critic=FAKE, rn=64, rows=128, val=256, n_steps=K, gamma=0.99, lam=0.95, adv=320, ret=384, with_tio=False,
                        tio=None):
    return lib.dockauv_gae_normalized(None, ptr(critic), ptr(rn), ref(blocks(tio=tio)[1], with_tio), ptr(rows), ptr(val), n_steps, gamma,
                                      lam, ptr(adv), ptr(ret), None)


# ------------------------------------------------------------------------------------------------------- the three collect calls
def call_collect(lib, actor=FAKE, critic=FAKE, io=True, cio=None):
    return lib.dockauv_collect(None, ptr(actor), ptr(critic), ref(blocks(cio=cio)[0], io), None)


def call_collect_truncated(lib, actor=FAKE, critic=FAKE, with_cio=True, with_tio=True, cio=None, tio=None):
    c, t, _ = blocks(cio=cio, tio=tio)
    return lib.dockauv_collect_truncated(None, ptr(actor), ptr(critic), ref(c, with_cio), ref(t, with_tio), None)


def call_collect_normalized(lib, actor=FAKE, critic=FAKE, rn=FAKE, with_cio=True, with_tio=False, with_nio=True, cio=None, tio=None,
                            nio=None):
    c, t, n = blocks(cio=cio, tio=tio, nio=nio)
    return lib.dockauv_collect_normalized(None, ptr(actor), ptr(critic), ref(c, with_cio), ref(t, with_tio), ptr(rn), ref(n, with_nio),
                                          None)


NO_CRITIC = dict(values=None, advantages=None, returns=None)   # a dockauv_collect_io as dockauv_collect wants it without a critic

# (call, its arguments: the two defects, the message of the one that is checked first).  The NULL handle is a defect of every row:
# where the message is "null handle", the other defect is one that is checked behind it.
TABLE = [
    # dockauv_gae: the buffers, n_steps, gamma, gae_lambda, the handle
    (call_gae, dict(val=None, n_steps=0), b"dockauv_gae: rows_out/values/advantages/returns must not be NULL"),
    (call_gae, dict(ret=None, gamma=1.5), b"dockauv_gae: rows_out/values/advantages/returns must not be NULL"),
    (call_gae, dict(n_steps=0, gamma=1.5), b"dockauv_gae: n_steps 0 must be >= 1"),
    (call_gae, dict(gamma=1.5, lam=-0.5), b"dockauv_gae: gamma 1.5 outside [0, 1]"),
    (call_gae, dict(lam=-0.5), b"dockauv_gae: gae_lambda -0.5 outside [0, 1]"),
    (call_gae, dict(), b"dockauv_gae: null handle"),

    # dockauv_gae_truncated: the handle is first, everything else is behind it
    (call_gae_truncated, dict(critic=None), b"dockauv_gae_truncated: null handle"),
    (call_gae_truncated, dict(io=False), b"dockauv_gae_truncated: null handle"),
    (call_gae_truncated, dict(tio=dict(struct_size=8)), b"dockauv_gae_truncated: null handle"),
    (call_gae_truncated, dict(tio=dict(gamma=1.5)), b"dockauv_gae_truncated: null handle"),

    # dockauv_gae_normalized: the column, the buffers, n_steps, gamma, gae_lambda, the handle; the truncation block is behind it
    (call_gae_normalized, dict(rn=None, rows=None), b"dockauv_gae_normalized: reward_norm is NULL"),
    (call_gae_normalized, dict(adv=None, n_steps=0), b"dockauv_gae_normalized: rows_out/values/advantages/returns must not be NULL"),
    (call_gae_normalized, dict(n_steps=0, gamma=-0.1), b"dockauv_gae_normalized: n_steps 0 must be >= 1"),
    (call_gae_normalized, dict(gamma=-0.1, lam=1.5), b"dockauv_gae_normalized: gamma -0.1 outside [0, 1]"),
    (call_gae_normalized, dict(lam=1.5), b"dockauv_gae_normalized: gae_lambda 1.5 outside [0, 1]"),
    (call_gae_normalized, dict(lam=1.5, with_tio=True, critic=None), b"dockauv_gae_normalized: gae_lambda 1.5 outside [0, 1]"),
    (call_gae_normalized, dict(with_tio=True, critic=None), b"dockauv_gae_normalized: null handle"),
    (call_gae_normalized, dict(with_tio=True, tio=dict(struct_size=8)), b"dockauv_gae_normalized: null handle"),
    (call_gae_normalized, dict(with_tio=True, tio=dict(n_steps=K + 1)), b"dockauv_gae_normalized: null handle"),

    # dockauv_collect: the block (NULL, struct_size, n_steps, the rollout's buffers, the critic's buffers, with a critic gamma and
    # gae_lambda), the actor, the handle
    (call_collect, dict(io=False, actor=None), b"dockauv_collect: io is NULL"),
    (call_collect, dict(cio=dict(struct_size=8, n_steps=0)), b"dockauv_collect_io.struct_size: got 8"),
    (call_collect, dict(cio=dict(n_steps=0, rows_in=None)), b"dockauv_collect_io.n_steps: 0 must be >= 1"),
    (call_collect, dict(cio=dict(actions_out=None, values=None)), b"dockauv_collect_io: rows_in/rows_out/actions_out must not be NULL"),
    (call_collect, dict(cio=dict(rows_out=None), critic=None), b"dockauv_collect_io: rows_in/rows_out/actions_out must not be NULL"),
    (call_collect, dict(cio=dict(returns=None, gamma=1.5)), b"dockauv_collect_io: values/advantages/returns must not be NULL with a critic"),
    (call_collect, dict(critic=None, actor=None), b"dockauv_collect_io: values/advantages/returns must be NULL without a critic"),
    (call_collect, dict(cio=dict(gamma=1.5, gae_lambda=-0.5)), b"dockauv_collect_io: gamma 1.5 outside [0, 1]"),
    (call_collect, dict(cio=dict(gae_lambda=-0.5), actor=None), b"dockauv_collect_io: gae_lambda -0.5 outside [0, 1]"),
    (call_collect, dict(cio=dict(gamma=1.5, **NO_CRITIC), critic=None, actor=None), b"dockauv_collect: null actor"),   # (no critic: no GAE)
    (call_collect, dict(actor=None), b"dockauv_collect: null actor"),
    (call_collect, dict(), b"dockauv_collect: null handle"),
    (call_collect, dict(cio=NO_CRITIC, critic=None), b"dockauv_collect: null handle"),

    # dockauv_collect_truncated: the handle is first, everything else is behind it
    (call_collect_truncated, dict(actor=None), b"dockauv_collect_truncated: null handle"),
    (call_collect_truncated, dict(critic=None), b"dockauv_collect_truncated: null handle"),
    (call_collect_truncated, dict(with_cio=False), b"dockauv_collect_truncated: null handle"),
    (call_collect_truncated, dict(cio=dict(struct_size=8)), b"dockauv_collect_truncated: null handle"),
    (call_collect_truncated, dict(cio=dict(terminal_obs=None)), b"dockauv_collect_truncated: null handle"),
    (call_collect_truncated, dict(with_tio=False), b"dockauv_collect_truncated: null handle"),
    (call_collect_truncated, dict(tio=dict(n_steps=K + 1)), b"dockauv_collect_truncated: null handle"),

    # dockauv_collect_normalized: the collect block (NULL, struct_size, n_steps, the rollout's buffers, the critic's buffers,
    # terminal_obs with a truncation block, gamma, gae_lambda), the normaliser's block (NULL, struct_size, n_steps, rows_out,
    # reward_norm, when training discounted and step_stats), what the two share (n_steps, rows_out), the handle; the normaliser,
    # the actor, the critic and the truncation block are behind it
    (call_collect_normalized, dict(with_cio=False, with_nio=False), b"dockauv_collect_normalized: cio is NULL"),
    (call_collect_normalized, dict(cio=dict(struct_size=8, n_steps=0)), b"dockauv_collect_io.struct_size: got 8"),
    (call_collect_normalized, dict(cio=dict(n_steps=0, rows_out=None)), b"dockauv_collect_io.n_steps: 0 must be >= 1"),
    (call_collect_normalized, dict(cio=dict(rows_in=None, advantages=None)), b"dockauv_collect_io: rows_in/rows_out/actions_out must not be NULL"),
    (call_collect_normalized, dict(cio=dict(values=None, terminal_obs=None), with_tio=True),
     b"dockauv_collect_io: values/advantages/returns must not be NULL (dockauv_collect_normalized needs a critic)"),
    (call_collect_normalized, dict(cio=dict(terminal_obs=None, gamma=1.5), with_tio=True),
     b"dockauv_collect_io.terminal_obs is NULL (the truncation block reads it)"),
    (call_collect_normalized, dict(cio=dict(terminal_obs=None, gamma=1.5)), b"dockauv_collect_io: gamma 1.5 outside [0, 1]"),   # (no block: optional)
    (call_collect_normalized, dict(cio=dict(gamma=1.5, gae_lambda=-0.5)), b"dockauv_collect_io: gamma 1.5 outside [0, 1]"),
    (call_collect_normalized, dict(cio=dict(gae_lambda=-0.5), with_nio=False), b"dockauv_collect_io: gae_lambda -0.5 outside [0, 1]"),
    (call_collect_normalized, dict(with_nio=False, rn=None), b"dockauv_collect_normalized: the dockauv_rewnorm_io is NULL"),
    (call_collect_normalized, dict(nio=dict(struct_size=8, n_steps=0)), b"dockauv_rewnorm_io.struct_size: got 8"),
    (call_collect_normalized, dict(nio=dict(n_steps=0, rows_out=None)), b"dockauv_rewnorm_io.n_steps: 0 must be >= 1"),
    (call_collect_normalized, dict(nio=dict(rows_out=None, reward_norm=None)), b"dockauv_rewnorm_io.rows_out is NULL"),
    (call_collect_normalized, dict(nio=dict(reward_norm=None, discounted=None)), b"dockauv_rewnorm_io.reward_norm is NULL"),
    (call_collect_normalized, dict(nio=dict(discounted=None, step_stats=None)), b"dockauv_rewnorm_io.discounted is NULL (required when training)"),
    (call_collect_normalized, dict(nio=dict(step_stats=None, n_steps=K + 1)), b"dockauv_rewnorm_io.step_stats is NULL (required when training)"),
    (call_collect_normalized, dict(nio=dict(n_steps=K + 1, rows_out=4096)), b"dockauv_rewnorm_io.n_steps: 5, dockauv_collect_io's is 4"),
    (call_collect_normalized, dict(nio=dict(rows_out=4096)), b"dockauv_rewnorm_io.rows_out is not dockauv_collect_io's"),
    (call_collect_normalized, dict(nio=dict(rows_out=4096), rn=None), b"dockauv_rewnorm_io.rows_out is not dockauv_collect_io's"),
    (call_collect_normalized, dict(rn=None), b"dockauv_collect_normalized: null handle"),
    (call_collect_normalized, dict(actor=None), b"dockauv_collect_normalized: null handle"),
    (call_collect_normalized, dict(critic=None), b"dockauv_collect_normalized: null handle"),
    (call_collect_normalized, dict(with_tio=True, tio=dict(struct_size=8)), b"dockauv_collect_normalized: null handle"),
    (call_collect_normalized, dict(with_tio=True, tio=dict(gamma=0.5)), b"dockauv_collect_normalized: null handle"),
    (call_collect_normalized, dict(nio=dict(training=0, discounted=None, step_stats=None)), b"dockauv_collect_normalized: null handle"),
]


@pytest.mark.parametrize("row", range(len(TABLE)), ids=lambda i: f"{TABLE[i][0].__name__[5:]}-{i}")
def test_the_first_defect_in_the_order_of_checks_is_reported(lib, row):
    call, kwargs, message = TABLE[row]
    assert call(lib, **kwargs) == -1, (call.__name__, kwargs)
    got = lib.dockauv_last_error(None)
    assert message in got, (call.__name__, kwargs, got)


def test_the_table_covers_the_six_entry_points():
    assert {call.__name__ for call, _, _ in TABLE} == {"call_gae", "call_gae_truncated", "call_gae_normalized", "call_collect",
                                                       "call_collect_truncated", "call_collect_normalized"}
