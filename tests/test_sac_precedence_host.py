"""
Which refusal wins, host side (no GPU), for SAC's entry points: dockauv_sac_actor_create, dockauv_sac_actor_load, dockauv_q_create,
dockauv_q_forward, dockauv_sac_target, dockauv_sac_actor_forward_rows, dockauv_sac_actor_backward, dockauv_q_backward,
dockauv_sac_sample, dockauv_sac_critic_head, dockauv_sac_actor_head and dockauv_sac_ent_coef_step.  As in
tests/test_collect_precedence_host.py every call has a NULL handle and small fake addresses that are never dereferenced, and is
wrong twice; the message reported must be that of the defect checked first.

ORDER lists, per entry point, the defects that are checked before the handle is looked into, in the order of the checks, each with
its message.  The rows are built from it: every adjacent pair of an order becomes one call with both defects, which must report the
first one's message; the last defect of an order stands alone (its partner is the NULL handle, or it is the NULL handle).  The
overlap refusals of the two loss heads are part of the orders: an array is moved onto the output it must not alias.  The checks
behind the handle (roles, strides against n_obs, two-layer gradients, the LDS bound) are pinned by the role-refusal loops and
test_refusals_on_a_live_handle of tests/test_gpu_sac*.py.
"""
import ctypes as C

import pytest

FAKE = 8          # an actor or critic: never dereferenced, the calls are refused first
B = 4             # n_rows of every block: 16-byte arrays at addresses 4096 apart do not overlap unless a row moves one
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from gym_dockauv_amd.csrc import build
    build.build()
    from gym_dockauv_amd import _capi
    return _capi.load_library()


def block(cls, **scalars):
    """a block of type `cls`: struct_size right, every pointer field a fake address of its own (4096 x its position), `scalars` set"""
    b = cls()
    for k, (name, ctype) in enumerate(cls._fields_):
        if ctype is C.c_void_p:
            setattr(b, name, 4096 * (k + 1))
    b.struct_size = C.sizeof(cls)
    for name, value in scalars.items():
        setattr(b, name, value)
    return b


def apply(b, over):
    """the defects of a row on a block; `@name` is the address the block holds in `name`, n_hidden0 / n_hidden1 index the array"""
    values = {name: (getattr(b, value[1:]) if isinstance(value, str) else value) for name, value in over.items()}
    for name, value in values.items():
        if name in ("n_hidden0", "n_hidden1"):
            b.n_hidden[int(name[-1])] = value
        else:
            setattr(b, name, value)
    return b


ptr = lambda x: C.c_void_p(x or None)
ref = lambda b, given: C.byref(b) if given else None


def split(kw):
    """a row's defects: those of the call's arguments (`_name`), of the gradient block of dockauv_q_backward (`grads.name`), of the block"""
    args = {k[1:]: v for k, v in kw.items() if k.startswith("_")}
    grads = {k[6:]: v for k, v in kw.items() if k.startswith("grads.")}
    return args, grads, {k: v for k, v in kw.items() if not k.startswith("_") and not k.startswith("grads.")}


def sac_desc():
    from gym_dockauv_amd import _capi
    return block(_capi.SacActorDesc, precision=_capi.F32, n_in=4, n_hidden=(C.c_int32 * 2)(8, 8), n_out=2, hidden_act=_capi.ACT_TANH)


def q_desc():
    from gym_dockauv_amd import _capi
    return block(_capi.PolicyDesc, precision=_capi.F32, n_in=6, n_hidden=(C.c_int32 * 2)(8, 8), n_out=1, hidden_act=_capi.ACT_TANH,
                 out_act=_capi.ACT_NONE)


def create(name, make_desc):
    def call(lib, **kw):
        args, _, over = split(kw)
        out = C.c_void_p()
        return getattr(lib, name)(None, ref(apply(make_desc(), over), args.get("d", True)), C.byref(out) if args.get("out", True) else None)
    call.__name__ = name
    return call


def with_io(name, io_class, n_objects=1, **scalars):
    """h, n_objects actors / critics (`_obj0`, `_obj1`, ...: None for NULL), the io block (`_io=False`: NULL), the stream"""
    def call(lib, **kw):
        from gym_dockauv_amd import _capi
        args, grads, over = split(kw)
        b = block(getattr(_capi, io_class), n_rows=B, **scalars)
        keep = None
        if io_class == "QBackwardIO":
            keep = apply(block(_capi.PolicyGrads), grads)
            b.grads = C.pointer(keep) if args.get("grads", True) else None
        objects = [ptr(args.get(f"obj{i}", FAKE)) for i in range(n_objects)]
        return getattr(lib, name)(None, *objects, ref(apply(b, over), args.get("io", True)), None)
    call.__name__ = name
    return call


def call_sac_actor_load(lib, **kw):
    return lib.dockauv_sac_actor_load(None, None, None)


CALLS = {
    "dockauv_sac_actor_create": create("dockauv_sac_actor_create", sac_desc),
    "dockauv_sac_actor_load": call_sac_actor_load,
    "dockauv_q_create": create("dockauv_q_create", q_desc),
    "dockauv_q_forward": with_io("dockauv_q_forward", "QIO", obs_stride=8, act_stride=2),
    "dockauv_sac_target": with_io("dockauv_sac_target", "SacTargetIO", 3, next_obs_stride=8, column_stride=1, gamma=0.99, ent_coef=0.2),
    "dockauv_sac_actor_forward_rows": with_io("dockauv_sac_actor_forward_rows", "SacRowsIO", row_stride=8),
    "dockauv_sac_actor_backward": with_io("dockauv_sac_actor_backward", "SacActorBackwardIO", row_stride=8),
    "dockauv_q_backward": with_io("dockauv_q_backward", "QBackwardIO", obs_stride=8, act_stride=2),
    "dockauv_sac_sample": with_io("dockauv_sac_sample", "SacSampleIO"),
    "dockauv_sac_critic_head": with_io("dockauv_sac_critic_head", "SacCriticHeadIO"),
    "dockauv_sac_actor_head": with_io("dockauv_sac_actor_head", "SacActorHeadIO", ent_coef=0.2),
    "dockauv_sac_ent_coef_step": with_io("dockauv_sac_ent_coef_step", "SacEntCoefIO", 0, target_entropy=-2.0, step=1, lr=3e-4, beta1=0.9,
                                         beta2=0.999, eps=1e-8),
}


def trunk(fn, name):
    """the fields dockauv_policy_desc and dockauv_sac_actor_desc share, in the order of their checks, but pointers_on_device and
    the four trunk arrays, which come behind out_act in dockauv_policy_desc"""
    s = name.encode()
    return [
        (dict(_d=False), fn.encode() + b": null argument"),
        (dict(struct_size=8), s + b".struct_size: got 8, library has "),
        (dict(precision=1), s + b".precision: 1, only DOCKAUV_F32 is implemented"),
        (dict(n_in=0), s + b".n_in: 0 must be >= 1"),
        (dict(n_hidden0=0), s + b".n_hidden[0]: 0 outside 1..128"),
        (dict(n_hidden1=129), s + b".n_hidden[1]: 129 outside 0..128 (0 = one hidden layer)"),
        (dict(n_out=0), s + b".n_out: 0 outside 1..8"),
        (dict(hidden_act=0), s + b".hidden_act: 0 is neither DOCKAUV_ACT_TANH nor DOCKAUV_ACT_RELU"),
    ]


def arrays(name):
    s = name.encode()
    return [
        (dict(pointers_on_device=2), s + b".pointers_on_device: 2 must be 0 or 1"),
        (dict(W1=None), s + b".W1 is NULL"),
        (dict(b1=None), s + b".b1 is NULL"),
        (dict(W2=None), s + b".W2 is NULL (n_hidden[1] > 0)"),
        (dict(b2=None), s + b".b2 is NULL (n_hidden[1] > 0)"),
    ]


def nulls(io_name, *fields):
    return [({f: None}, f"{io_name}.{f} is NULL".encode()) for f in fields]


def io_head(fn, io_name):
    return [
        (dict(_io=False), f"{fn}: io is NULL".encode()),
        (dict(struct_size=8), f"{io_name}.struct_size: got 8, library has ".encode()),
        (dict(n_rows=0), f"{io_name}.n_rows: 0 must be >= 1".encode()),
    ]


def overlaps(io_name, outputs, inputs):
    """refuse_overlap's order: every output against every input, then against the outputs behind it.  The defect moves the other
    array onto the output"""
    rows = []
    for i, out in enumerate(outputs):
        for name in inputs:
            rows.append(({name: "@" + out}, f"{io_name}.{out} overlaps {name}: outputs must not alias inputs".encode()))
        for name in outputs[i + 1:]:
            rows.append(({name: "@" + out}, f"{io_name}.{out} overlaps {name}: outputs must not alias one another".encode()))
    return rows


ORDER = {
    "dockauv_sac_actor_create": trunk("dockauv_sac_actor_create", "dockauv_sac_actor_desc") + arrays("dockauv_sac_actor_desc")
    + nulls("dockauv_sac_actor_desc", "W_mu", "b_mu", "W_ls", "b_ls")
    + [(dict(), b"dockauv_sac_actor_create: null handle")],

    # (behind the policy, the descriptor is read through it: nothing else is reachable without one)
    "dockauv_sac_actor_load": [(dict(), b"dockauv_sac_actor_load: null policy")],

    "dockauv_q_create": trunk("dockauv_q_create", "dockauv_policy_desc")
    + [(dict(out_act=2), b"dockauv_policy_desc.out_act: 2 is neither DOCKAUV_ACT_NONE nor DOCKAUV_ACT_TANH")]
    + arrays("dockauv_policy_desc") + nulls("dockauv_policy_desc", "W3", "b3")
    + [(dict(n_out=2), b"dockauv_policy_desc.n_out: 2, a critic has one output"),
       (dict(out_act=1), b"dockauv_policy_desc.out_act: 1, a critic's output is raw (DOCKAUV_ACT_NONE)"),
       (dict(), b"dockauv_q_create: null handle")],

    "dockauv_q_forward": io_head("dockauv_q_forward", "dockauv_q_io") + nulls("dockauv_q_io", "obs", "actions", "q")
    + [(dict(_obj0=None), b"dockauv_q_forward: null critic"),
       (dict(), b"dockauv_q_forward: null handle")],

    "dockauv_sac_target": io_head("dockauv_sac_target", "dockauv_sac_target_io")
    + [(dict(gamma=1.5), b"dockauv_sac_target_io.gamma: 1.5 outside [0, 1]"),
       (dict(ent_coef=NAN, log_ent_coef=None), b"dockauv_sac_target_io.ent_coef is NaN (and log_ent_coef is NULL)")]
    + nulls("dockauv_sac_target_io", "next_obs", "rewards", "dones", "a2", "logp2", "q1", "q2", "y")
    + [(dict(column_stride=0), b"dockauv_sac_target_io.column_stride: 0 must be >= 1"),
       (dict(_obj0=None), b"dockauv_sac_target: null actor"),
       # (the two target critics are one check with one message: the pair of rows has no order to pin, it is here so that a NULL
       # q1_target and a NULL q2_target are each refused before the handle)
       (dict(_obj1=None), b"dockauv_sac_target: null critic"),
       (dict(_obj2=None), b"dockauv_sac_target: null critic"),
       (dict(), b"dockauv_sac_target: null handle")],

    "dockauv_sac_actor_forward_rows": io_head("dockauv_sac_actor_forward_rows", "dockauv_sac_rows_io")
    + [(dict(row_stride=0), b"dockauv_sac_rows_io.row_stride: 0 is below every row width")]
    + nulls("dockauv_sac_rows_io", "rows", "out")
    + [(dict(_obj0=None), b"dockauv_sac_actor_forward_rows: null actor"),
       (dict(), b"dockauv_sac_actor_forward_rows: null handle")],

    "dockauv_sac_actor_backward": io_head("dockauv_sac_actor_backward", "dockauv_sac_actor_backward_io")
    + [(dict(row_stride=0), b"dockauv_sac_actor_backward_io.row_stride: 0 is below every row width")]
    + nulls("dockauv_sac_actor_backward_io", "rows", "grad_out", "dW1", "db1", "dW_mu", "db_mu", "dW_ls", "db_ls")
    + [(dict(_obj0=None), b"dockauv_sac_actor_backward: null actor"),
       (dict(dW2=None), b"dockauv_sac_actor_backward: null handle"),     # (the second layer's arrays are behind the handle)
       (dict(), b"dockauv_sac_actor_backward: null handle")],

    "dockauv_q_backward": io_head("dockauv_q_backward", "dockauv_q_backward_io")
    + [(dict(obs_stride=0), b"dockauv_q_backward_io.obs_stride: 0 is below every row width"),
       (dict(act_stride=0), b"dockauv_q_backward_io.act_stride: 0 is below every row width")]
    + nulls("dockauv_q_backward_io", "obs", "actions", "grad_q")
    + [(dict(_grads=False, grad_actions=None), b"dockauv_q_backward_io: grads and grad_actions are both NULL, at least one output is required"),
       ({"grads.struct_size": 8}, b"dockauv_policy_grads.struct_size: got 8, library has "),
       ({"grads.dW1": None}, b"dockauv_policy_grads: dW1/db1/dW3/db3 must not be NULL"),
       (dict(_obj0=None), b"dockauv_q_backward: null critic"),
       ({"grads.dW2": None}, b"dockauv_q_backward: null handle"),       # (the second layer's arrays are behind the handle)
       (dict(), b"dockauv_q_backward: null handle")],

    "dockauv_sac_sample": io_head("dockauv_sac_sample", "dockauv_sac_sample_io") + nulls("dockauv_sac_sample_io", "heads", "a", "logp")
    + [(dict(_obj0=None), b"dockauv_sac_sample: null actor"),
       (dict(), b"dockauv_sac_sample: null handle")],

    "dockauv_sac_critic_head": io_head("dockauv_sac_critic_head", "dockauv_sac_critic_head_io")
    + nulls("dockauv_sac_critic_head_io", "q1", "q2", "y", "grad_q1", "grad_q2", "stats")
    + overlaps("dockauv_sac_critic_head_io", ["grad_q1", "grad_q2", "stats"], ["q1", "q2", "y"])
    + [(dict(_obj0=None), b"dockauv_sac_critic_head: null critic"),
       (dict(), b"dockauv_sac_critic_head: null handle")],

    "dockauv_sac_actor_head": io_head("dockauv_sac_actor_head", "dockauv_sac_actor_head_io")
    + [(dict(ent_coef=NAN, log_ent_coef=None), b"dockauv_sac_actor_head_io.ent_coef is NaN (and log_ent_coef is NULL)")]
    + nulls("dockauv_sac_actor_head_io", "heads", "q1_pi", "q2_pi", "dq1", "dq2", "grad_out", "stats")
    + overlaps("dockauv_sac_actor_head_io", ["grad_out", "stats"], ["heads", "q1_pi", "q2_pi", "dq1", "dq2", "log_ent_coef"])
    + [(dict(_obj0=None), b"dockauv_sac_actor_head: null actor"),
       (dict(), b"dockauv_sac_actor_head: null handle")],

    "dockauv_sac_ent_coef_step": io_head("dockauv_sac_ent_coef_step", "dockauv_sac_ent_coef_io")
    + [(dict(step=0), b"dockauv_sac_ent_coef_io.step: 0 must be >= 1 (the caller's count of this step)"),
       (dict(lr=-1.0), b"dockauv_sac_ent_coef_io.lr: -1 must be finite and >= 0"),
       (dict(beta1=1.0), b"dockauv_sac_ent_coef_io.beta1: 1 outside [0, 1)"),
       (dict(beta2=-0.5), b"dockauv_sac_ent_coef_io.beta2: -0.5 outside [0, 1)"),
       (dict(eps=0.0), b"dockauv_sac_ent_coef_io.eps: 0 must be > 0")]
    + nulls("dockauv_sac_ent_coef_io", "state", "logp")
    + [(dict(before="@state"), b"dockauv_sac_ent_coef_io.before overlaps state: it receives the value from before the step"),
       (dict(stats="@state"), b"dockauv_sac_ent_coef_io.stats overlaps state"),
       (dict(), b"dockauv_sac_ent_coef_step: null handle")],
}


def rows():
    """(entry point, the defects of the call, the message): every adjacent pair of an order, and its last defect alone"""
    table = []
    for fn, order in ORDER.items():
        for (kw, message), (kw_next, _) in zip(order, order[1:]):
            assert not set(kw) & set(kw_next), (fn, kw, kw_next)   # the two defects are set independently
            table.append((fn, {**kw_next, **kw}, message))
        table.append((fn, order[-1][0], order[-1][1]))
    return table


TABLE = rows()


@pytest.mark.parametrize("row", range(len(TABLE)), ids=lambda i: f"{TABLE[i][0][8:]}-{i}")
def test_the_first_defect_in_the_order_of_checks_is_reported(lib, row):
    fn, kwargs, message = TABLE[row]
    assert CALLS[fn](lib, **kwargs) == -1, (fn, kwargs)
    got = lib.dockauv_last_error(None)
    assert message in got, (fn, kwargs, got)


def test_the_table_covers_the_entry_points():
    assert set(ORDER) == set(CALLS) and len(CALLS) == 12
    assert all(len(order) >= 2 for fn, order in ORDER.items() if fn != "dockauv_sac_actor_load")
