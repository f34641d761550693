"""Constructed states for the stage behind the rays -- navigation errors, done conditions, the sixteen leading observation
entries, the reward terms, the heading wrap -- and their qualification (CPU: NumPy and the oracle only).

Every env of a scene is one case: one step (two for the heading wrap) from a pre-step state, filtered input, step counter,
current row and action that the caller writes with set_field.  The generator takes the POST-step pose p+ from the oracle's
auv_step in float64, places the goal relative to p+, and where a post-step attitude, velocity or heading has to hit a value it
finds the pre-step one by a root search on auv_step (secant steps, then a bracketing search).

Classes (CLASSES), margins m in {1e-3, 1e-4} on both sides:
  goal-tol     delta_d = dist_goal_reached_tol -+ m, goal offset along +-x, +-y, +-z (1e-2 m beside the vertical; exactly
               vertical from a level vehicle at rest: float64 only) and two diagonals: bit 0, w_goal, obs[0] clipped
  goal-far     the same at max_dist_from_goal: bit 1, obs[0] clipped at the other end
  goal-close   delta_d in {1e-2, 1e-3, 5e-4, 1e-6} and the goal ON p+ (float64 only): log(0), the eps clamp of log_precision
  vertical     goal straight above / below p+: delta_theta = theta +- pi/2 (exactly: float64 only; 1e-2 m beside: float32)
  behind       atan2(dy, dx) - psi = +-(pi - m), by turning the goal around a level vehicle at heading 0 and by turning psi
               under a goal at dy == 0, dx > 0; dy = -+0.0 with dx < 0 (float64 only): obs[2] with its sign
  attitude     post-step phi or theta = +-(max_attitude -+ m): bit 2, obs[6] / obs[7] clipped
  time         step counter in {max - 2, max - 1, max, max + 1}: bit 3 on the pre-increment counter
  several      two and three conditions on one step (and, with an obstacle slot, collision with attitude): the weights add
  saturation   post-step nu_r entries at 1.25 x and 0.99 x their maxima; a current of 3 and 1.9 m/s along each body axis
               (scenes with a current); actions of +-1.5 and +-7 beside twins with the clipped action
  heading-wrap psi0 = +-(pi - delta) and a yaw rate that carries the first step, the second step or neither across +-pi
(obs[0] = clip(1 - log(d / d_max) / log(d_tol / d_max), 0, 1) is 0 inside the goal tolerance and 1 beyond the maximum.)

Yardstick groups.  A few variants make the REFERENCE's bearing ill-conditioned on float32 inputs (a goal 1e-2 m beside the
vertical, a goal within a millimetre of p+: SHIFT turns atan2(dy, dx)).  Each has a group of its own (`group`: "goal-tol/z",
"goal-close/1e-06", ...), so that its movement does not widen the bound of the rest of its class.

Qualification (qualify): the oracle is evaluated on the float64 inputs and on what a float32 handle holds -- rows rounded to
float32 (position and heading excepted: dockauv_set_field keeps their low words; the goal row is plain float32), post-step
position moved by ray_scenes.SHIFT.  A case is float32-qualified if the two evaluations agree in all five condition bits and the
reference keeps MARGIN to every threshold the case was built next to."""
import math

import numpy as np

from oracle import dockauv_oracle as orc
from tests.ray_scenes import SHIFT, vehicles_of

CLASSES = ("goal-tol", "goal-far", "goal-close", "vertical", "behind", "attitude", "time", "several", "saturation", "heading-wrap")
F64_ONLY = ("goal-tol/exact-z", "goal-far/exact-z", "goal-close/0", "vertical/exact", "behind/zero")   # groups no float32 test reads
MARGIN = 5e-5
MARGINS = (1e-3, 1e-4)
N_ENVS = 400          # six full 64-env groups and a tail of sixteen
# The velocity maxima are smaller than the defaults: the reference's explicit step cannot leave a BlueROV2 at 1.25 x the default
# p_max (its one-step map of the roll rate peaks near 1.2 rad/s) and the LAUV's pitch and yaw rates run away beyond ~0.05 rad/s.
OVERRIDES = dict(u_max=1.0, v_max=0.5, w_max=0.5, p_max=0.5, q_max=0.5, r_max=0.6)
CFG = dict(orc.default_config(), **OVERRIDES)
DTOL, DMAX, MATT, TMAX = float(CFG["dist_goal_reached_tol"]), float(CFG["max_dist_from_goal"]), float(CFG["max_attitude"]), int(CFG["max_timesteps"])
VEL_MAX = np.array([CFG[k] for k in ("u_max", "v_max", "w_max", "p_max", "q_max", "r_max")], float)
H = float(CFG["t_step_size"])
MU = 0.005            # the Gauss-Markov constant of every scenario's current
FAR = 150.0           # where the obstacles of the ray scenarios stand: out of every ray's and the body's reach


def _unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


# ------------------------------------------------------------------------------------------------ the list of cases
def specs(with_current, with_obstacle):
    """one dict per case of a scene's period.  Keys: cls, sub, group; goal (rule, see _goal); rest (level vehicle at rest at
    heading 0); target (state index, post-step value); tsteps; action ("clip:a" = the clipped twin of a); current (body axis,
    speed); near (thresholds the case is built next to); margin, side (+1 beyond the threshold); bits (requested); collide"""
    out = []

    def add(cls, sub, goal=("ahead",), group=None, **kw):
        out.append(dict(dict(cls=cls, sub=sub, group=group or cls, goal=goal, rest=False, target=None, tsteps=None, action=None, current=None,
                             near=(), margin=None, side=0, bits=None, collide=False, yaw=None, calm=False), **kw))
    dirs = {"+x": (1, 0, 0), "-x": (-1, 0, 0), "+y": (0, 1, 0), "-y": (0, -1, 0), "+z": "beside+", "-z": "beside-",
            "d1": (1, 1, 1), "d2": (-1, 1, -1)}
    for cls, thr, key, bit in (("goal-tol", DTOL, "dtol", 0), ("goal-far", DMAX, "dmax", 1)):
        for m in MARGINS:
            for side in (-1, 1):
                fired = (side < 0) if bit == 0 else (side > 0)
                kw = dict(near=(key,), margin=m, side=side, bits=(1 << bit) if fired else 0)
                for name, d in dirs.items():
                    if isinstance(d, str):
                        add(cls, f"{name}{side:+d}/{m:g}", ("beside", 1.0 if d[-1] == "+" else -1.0, thr + side * m), group=cls + "/z", **kw)
                    else:
                        add(cls, f"{name}{side:+d}/{m:g}", ("ned", d, thr + side * m), **kw)
                for sg in (1.0, -1.0):
                    add(cls, f"exact{'+' if sg > 0 else '-'}z{side:+d}/{m:g}", ("ned", (0, 0, sg), thr + side * m), group=cls + "/exact-z",
                        rest=True, **kw)
    for dd in (1e-2, 1e-3, 5e-4, 1e-6):
        for d in ((1, 0.5, 0.3), (-0.4, 1, -0.6)):
            add("goal-close", f"{dd:g}", ("ned", d, dd), group=f"goal-close/{dd:g}", bits=1)
    add("goal-close", "0", ("on",), group="goal-close/0", bits=1)
    for sg in (1.0, -1.0):
        add("vertical", f"exact{'+' if sg > 0 else '-'}", ("ned", (0, 0, sg), 5.0), group="vertical/exact", rest=True)
        for d in (5.0, 1.5):
            add("vertical", f"beside{'+' if sg > 0 else '-'}/{d:g}", ("beside", sg, d))
    for m in MARGINS:
        for sg in (1.0, -1.0):
            kw = dict(near=("dpsi",), margin=m, side=int(sg))
            add("behind", f"goal{sg:+.0f}/{m:g}", ("bearing", sg * (math.pi - m), 5.0), rest=True, **kw)
            add("behind", f"psi{sg:+.0f}/{m:g}", ("east0",), yaw=-sg * (math.pi - m), **kw)
    add("behind", "-0.0", ("west0", -0.0), group="behind/zero", rest=True)
    add("behind", "+0.0", ("west0", 0.0), group="behind/zero", rest=True)
    for m in MARGINS:
        for k, nm in ((3, "phi"), (4, "theta")):
            for sg in (1.0, -1.0):
                for side in (-1, 1):
                    add("attitude", f"{nm}{sg:+.0f}{side:+d}/{m:g}", target=(k, sg * (MATT + side * m)), near=("att",), margin=m, side=side,
                        bits=4 if side > 0 else 0)
    for t in (TMAX - 2, TMAX - 1, TMAX, TMAX + 1):
        add("time", str(t - TMAX), tsteps=t, bits=8 if t >= TMAX else 0)
    add("several", "goal+time", ("ned", (1, 1, 0), DTOL - 1e-2), tsteps=TMAX, bits=1 | 8)
    add("several", "far+attitude", ("ned", (1, -1, 0.5), DMAX + 1e-2), target=(3, MATT + 1e-2), bits=2 | 4)
    add("several", "attitude+time", target=(4, -(MATT + 1e-2)), tsteps=TMAX + 3, bits=4 | 8)
    add("several", "far+attitude+time", ("ned", (-1, 0.3, 0.2), DMAX + 1e-2), target=(4, MATT + 1e-2), tsteps=TMAX, bits=2 | 4 | 8)
    if with_obstacle:
        add("several", "collision+attitude", target=(3, -(MATT + 1e-2)), collide=True, bits=4 | 16)
        add("several", "collision+goal+time", ("ned", (1, 0, 0), DTOL - 1e-2), tsteps=TMAX, collide=True, bits=1 | 8 | 16)
    for k in range(6):
        for sg in (1.0, -1.0):
            for f in (1.25, 0.99):
                add("saturation", f"nu{k}{sg:+.0f}x{f}", target=(6 + k, sg * f * VEL_MAX[k]), near=(f"sat{(3 + k) if k < 3 else (7 + k)}",),
                    side=1 if f > 1 else -1, calm=True)
    if with_current:
        for k in range(3):
            for v in (3.0, -3.0, 1.9, -1.9):
                add("saturation", f"current{k}{v:+g}", current=(k, v), near=(f"sat{13 + k}",), side=1 if abs(v) > 2 else -1)
    for a in ("+1.5", "-1.5", "+7", "-7", "mixed"):
        add("saturation", f"action{a}", action=a)
        add("saturation", f"action{a}/clipped", action="clip:" + a)
    for sg in (1.0, -1.0):
        for nm in ("cross", "short", "second"):
            add("heading-wrap", f"{nm}{sg:+.0f}", yaw=nm, target=(11, sg), calm=True)
    return out


def _interleave(sp):
    """round robin over the classes, so that every 64-env group of a scene sees every class"""
    by = {}
    for s in sp:
        by.setdefault(s["cls"], []).append(s)
    keyed = []
    for k, c in enumerate(sorted(by, key=lambda c: -len(by[c]))):
        n = len(by[c])
        keyed += [((j + 0.5) / n + 1e-6 * k, k, j, c) for j in range(n)]
    return [by[c][j] for _, _, j, c in sorted(keyed)]


def _action(spec, n_u, rs):
    a = spec["action"]
    if a is None:
        return np.zeros(n_u) if spec["rest"] or spec["calm"] else rs.uniform(-1, 1, n_u)
    clip = a.startswith("clip:")
    a = a[5:] if clip else a
    v = np.array([1.5, -7.0, 7.0, -1.5, 1.5, -7.0][:n_u]) if a == "mixed" else np.full(n_u, float(a))
    return np.clip(v, -1.0, 1.0) if clip else v


def _current_row(spec, att):
    """host row (V_c, V_min, V_max, alpha, beta) of a current of `speed` along body axis k at the PRE-step attitude"""
    if spec["current"] is None:
        return np.zeros(5)
    k, v = spec["current"]
    d = orc.rot_zyx(*att)[:, k] * np.sign(v)
    beta = math.asin(float(np.clip(d[1], -1, 1)))
    alpha = math.atan2(d[2], d[0])
    return np.array([abs(v), abs(v), abs(v), alpha, beta])


def nu_c_of(row, att):
    cur = orc.CurrentState(MU, row[1], row[2], row[0], row[3], row[4], 0.0)
    cur.sim(H, 0.0)
    return cur.body(att)


def _lowpass(m, u_prev, action):
    a = orc.lowpass_alpha(H)
    return a * m.unnormalize(action) + (1.0 - a) * u_prev


def _goal(rule, post, rs):
    p, psi = post[0:3], post[5]
    kind = rule[0]
    if kind == "ned":
        return p + rule[2] * _unit(rule[1])
    if kind == "beside":      # rule[2] m from p+, 1e-2 m of it horizontal (ahead), the rest straight down (+) / up (-)
        return p + np.array([1e-2 * math.cos(psi + 0.3), 1e-2 * math.sin(psi + 0.3), rule[1] * math.sqrt(rule[2] ** 2 - 1e-4)])
    if kind == "bearing":
        b = psi + rule[1]
        return p + np.array([rule[2] * math.cos(b), rule[2] * math.sin(b), 0.7])
    if kind == "east0":       # dy == 0 exactly, dx > 0
        return np.array([p[0] + 5.0, p[1], p[2] - 0.5])
    if kind == "west0":       # dx < 0, dy = -+0.0: p+ sits at y == +0.0
        return np.array([p[0] - 5.0, rule[1], p[2] + 0.5])
    if kind == "on":
        return p.copy()
    b, e, d = psi + rs.uniform(-1.0, 1.0), rs.uniform(-0.5, 0.5), rs.uniform(3.0, 12.0)     # "ahead": every angle well conditioned
    return p + d * np.array([math.cos(e) * math.cos(b), math.cos(e) * math.sin(b), math.sin(e)])


def make_scene(vehicle="BlueROV2", with_current=False, max_capsules=0, max_spheres=0, seed=1, n_envs=N_ENVS, classes=CLASSES):
    """One scene: dict of state [N, 12], u [N, 8], goal [N, 4], current [N, 5], tsteps [N], action [N, 8], capsules / spheres
    (the rows of F_STATE, F_U, F_GOAL, F_CURRENT, F_TSTEPS, F_CAPSULES, F_SPHERES and the step's actions), label / sub / group [N],
    near [N] (tuples), margin / side [N], bits [N] (requested condition bits, -1: none requested), twin [N] (the env holding the
    clipped twin of an action case, else -1), vehicle [N]."""
    rs = np.random.RandomState(seed)
    sp = _interleave([s for s in specs(with_current, max_capsules + max_spheres > 0) if s["cls"] in classes])
    N = int(n_envs)
    vehicles = vehicles_of(vehicle, N)
    models = {v: orc.VehicleModel(orc.VEHICLE_KINDS[v]) for v in set(vehicles)}
    sc = dict(state=np.zeros((N, 12)), u=np.zeros((N, 8)), goal=np.zeros((N, 4)), current=np.zeros((N, 5)), tsteps=np.zeros(N, int),
              action=np.zeros((N, 8)), capsules=np.zeros((N, max_capsules, 7)), spheres=np.zeros((N, max_spheres, 4)))
    sc["capsules"][:, :, 0:6] = FAR
    sc["capsules"][:, :, 5] += 2.0
    sc["capsules"][:, :, 6] = 1.0
    sc["spheres"][:, :, 0:3] = FAR
    sc["spheres"][:, :, 3] = 1.0
    meta = []
    twin = np.full(N, -1)
    last_action_case = {}
    for i in range(N):
        s = sp[i % len(sp)]
        m = models[vehicles[i]]
        n_u = m.n_u
        clipped_twin = s["action"] is not None and s["action"].startswith("clip:")
        if clipped_twin and (s["action"][5:], vehicles[i]) in last_action_case:     # same pre-step state as the raw case
            j = last_action_case[(s["action"][5:], vehicles[i])]
            st, up = sc["state"][j].copy(), sc["u"][j, :n_u].copy()
            twin[j] = i
        elif s["rest"]:
            st, up = np.zeros(12), np.zeros(n_u)
            st[0:3] = np.round(rs.uniform(-4, 4, 3) * 4) / 4
            if s["goal"][0] == "west0":
                st[1] = 0.0
        else:
            st = np.zeros(12)
            st[0:3] = rs.uniform(-6, 6, 3)
            st[3:6] = [rs.uniform(-0.5, 0.5), rs.uniform(-0.5, 0.5), rs.uniform(-2.5, 2.5)]
            ang = 0.3 if vehicles[i] == "BlueROV2" else 0.01      # (the LAUV's explicit step runs away from larger pitch / yaw rates)
            st[6:12] = rs.uniform(-0.3, 0.3, 6) * [1, 1, 1, ang, ang, ang]
            up = 0.5 * m.unnormalize(rs.uniform(-1, 1, n_u))
            if s["calm"]:     # (the asked rate is within the explicit step's reach from a level vehicle with no other motion)
                st[3:5], st[6:12], up = 0.0, 0.0, np.zeros(n_u)
        if s["cls"] == "heading-wrap":      # yaw rate after the first step: what the vehicle's explicit step can hold for two steps
            st[5] = 0.0
            s = dict(s, target=(11, s["target"][1] * (0.1 if vehicles[i] == "BlueROV2" else 0.004)))
        act = _action(s, n_u, rs)
        if s["action"] is not None and not clipped_twin:
            last_action_case[(s["action"], vehicles[i])] = i
        fix = s["target"] if s["target"] is not None else ((5, s["yaw"]) if s["yaw"] is not None and s["cls"] != "heading-wrap" else None)

        def step_from(x):
            """(post-step state, its miss of the asked value) with the pre-step entry set to x"""
            if fix is not None:
                st[fix[0]] = x
            with np.errstate(all="ignore"):     # (the search may leave the range in which the explicit step is tame)
                post, _, _ = orc.auv_step(m, st.copy(), up, act, nu_c_of(_current_row(s, st[3:6]), st[3:6]), H)
            e = 0.0 if fix is None else post[fix[0]] - fix[1]
            return post, ((e + math.pi) % (2 * math.pi) - math.pi) if fix is not None and fix[0] == 5 else e
        # the pre-step entry whose post-step value is asked for: secant steps on auv_step (the plain fixed-point iteration
        # x -= miss diverges on the stiff angular rates, where the explicit step's gain is negative)
        x0 = fix[1] if fix is not None else 0.0
        post, e0 = step_from(x0)
        x1 = x0 - e0 if e0 != 0.0 else x0
        for it in range(60):
            if abs(e0) < 1e-13:
                break
            post, e1 = step_from(x1)
            if abs(e1) < 1e-13 or e1 == e0:
                x0, e0 = x1, e1
                break
            x0, e0, x1 = x1, e1, x1 - e1 * (x1 - x0) / (e1 - e0)
        post, e0 = step_from(x0)
        if not abs(e0) < 1e-12:
            # (the secant left the range in which the explicit step is tame: bracket the root nearest to zero on a grid, then
            # regula falsi with bisection steps inside the bracket)
            w = 3.0 * max(abs(fix[1]), 0.5)
            grid = np.linspace(fix[1] - w, fix[1] + w, 97)
            miss = np.array([step_from(x)[1] for x in grid])
            k = [j for j in range(96) if np.isfinite(miss[j:j + 2]).all() and miss[j] * miss[j + 1] <= 0]
            if not k:
                raise RuntimeError(f"no pre-step state for {s['cls']} {s['sub']} ({vehicles[i]})")
            j = min(k, key=lambda j: abs(grid[j]))
            a, b, ea, eb = grid[j], grid[j + 1], miss[j], miss[j + 1]
            for it in range(200):
                x0 = a - ea * (b - a) / (eb - ea) if it % 2 == 0 and eb != ea else 0.5 * (a + b)
                post, e0 = step_from(x0)
                if abs(e0) < 1e-13 or b - a < 1e-16:
                    break
                if e0 * ea <= 0:
                    b, eb = x0, e0
                else:
                    a, ea = x0, e0
            post, e0 = step_from(x0)
            if not abs(e0) < 1e-11:
                raise RuntimeError(f"no pre-step state for {s['cls']} {s['sub']} ({vehicles[i]}): miss {e0}")
        cur = _current_row(s, st[3:6])
        if s["cls"] == "heading-wrap":
            # the heading is cyclic in the dynamics: psi0 = +-(pi - delta) with delta chosen from the two steps' turns t1, t2
            # (from psi0 = 0): "cross" the first step crosses, "short" neither, "second" delta lies between the two (the
            # second step crosses, or -- where the yaw rate reverses -- the first crosses and the second comes back)
            t1 = post[5]
            post2, _, _ = orc.auv_step(m, post.copy(), _lowpass(m, up, act), act, np.zeros(6), H)
            t2 = math.remainder(post2[5], 2 * math.pi)
            sg = 1.0 if t1 > 0 else -1.0
            delta = {"cross": 0.4 * abs(t1), "short": 3.0 * max(abs(t1), abs(t2)) + 0.01, "second": 0.5 * (abs(t1) + sg * t2)}[s["yaw"]]
            delta = max(delta, 0.2 * abs(t1))
            st[5] = sg * (math.pi - delta)
            post[5] = orc.ssa(post[5] + st[5])
        sc["state"][i], sc["u"][i, :n_u], sc["action"][i, :n_u], sc["current"][i] = st, up, act, cur
        sc["goal"][i, 0:3] = _goal(s["goal"], post, rs)
        sc["goal"][i, 3] = rs.uniform(-1.5, 1.5)
        sc["tsteps"][i] = s["tsteps"] if s["tsteps"] is not None else rs.randint(0, TMAX - 10)
        if s["collide"]:          # an obstacle of radius 1 whose surface is safety - 1e-2 from p+, straight behind the vehicle
            back = -orc.rot_zyx(*post[3:6])[:, 0]
            c = post[0:3] + (1.0 + orc.SAFETY_RADIUS - 1e-2) * back
            if max_capsules:
                side = orc.rot_zyx(*post[3:6])[:, 1]
                sc["capsules"][i, -1] = [*(c - 0.5 * side), *(c + 0.5 * side), 1.0]
            else:
                sc["spheres"][i, -1] = [*c, 1.0]
        meta.append(s)
    sc["capsules"], sc["spheres"] = sc["capsules"].reshape(N, -1), sc["spheres"].reshape(N, -1)
    sc.update(label=np.array([s["cls"] for s in meta]), sub=np.array([s["sub"] for s in meta]), group=np.array([s["group"] for s in meta]),
              near=[s["near"] for s in meta], margin=np.array([s["margin"] or 0.0 for s in meta]), side=np.array([s["side"] for s in meta]),
              bits=np.array([-1 if s["bits"] is None else s["bits"] for s in meta]), twin=twin, vehicle=np.array(vehicles),
              with_current=with_current, max_capsules=max_capsules, max_spheres=max_spheres, seed=seed)
    return sc


# ------------------------------------------------------------------------------------------------ the oracle on a scene
def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def evaluate(scene, float32_inputs=False, reward_set=1):
    """Two oracle steps per env (the second with the same action).  float32_inputs: on what a float32 handle holds.  Returns, for
    the first step, bits [N] (condition bits 0..4), done, obs [N, 16] (the reference's float32 row), nav [N, 3] (delta_d,
    delta_theta, delta_psi), state [N, 12], u [N, 8], terms [N, 13], reward [N], ratio [N, 16] (the unclipped observation
    entries), and for the second step state2 / obs2 / bits2."""
    N = scene["state"].shape[0]
    rs = np.random.RandomState(scene["seed"] + 977)
    shifts = rs.normal(size=(N, 3))
    shifts *= SHIFT / np.linalg.norm(shifts, axis=1)[:, None]
    out = dict(bits=np.zeros(N, int), done=np.zeros(N, bool), obs=np.zeros((N, 16)), nav=np.zeros((N, 3)), state=np.zeros((N, 12)),
               u=np.zeros((N, 8)), terms=np.zeros((N, 13)), reward=np.zeros(N), ratio=np.zeros((N, 16)), state2=np.zeros((N, 12)),
               obs2=np.zeros((N, 16)), bits2=np.zeros(N, int))
    C, Sp = scene["max_capsules"], scene["max_spheres"]
    pw = 2 ** np.arange(5)
    for i in range(N):
        o = orc.OracleEnv("CapsuleDocking3d" if C + Sp else "SimpleDocking3d", dict(OVERRIDES, vehicle=str(scene["vehicle"][i]), reward_set=reward_set))
        n_u = o.model.n_u
        st, up, gl, cur, act = (scene[k][i].copy() for k in ("state", "u", "goal", "current", "action"))
        caps, sph = scene["capsules"][i].reshape(-1, 7), scene["spheres"][i].reshape(-1, 4)
        if float32_inputs:
            keep = st[[0, 1, 2, 5]].copy()      # (position and heading: the state rows plus their low words)
            st = _f32(st)
            st[[0, 1, 2, 5]] = keep
            up, gl, cur, act, caps, sph = _f32(up), _f32(gl), _f32(cur), _f32(act), _f32(caps), _f32(sph)
        ep = orc.Episode(position=st[0:3], attitude=st[3:6], goal=gl[0:3], heading_goal=float(gl[3]),
                         current=orc.CurrentState(MU, cur[1], cur[2], cur[0], cur[3], cur[4], 0.0),
                         capsules=[(c[0:3], c[3:6], c[6]) for c in caps], sphere_centers=sph[:, 0:3], sphere_radii=sph[:, 3])
        o.reset(episode=ep)
        o.state[6:12] = st[6:12]
        o.u = up[:n_u].copy()
        o.t_steps = int(scene["tsteps"][i])
        inner = o._ray_distances

        def rays(o=o, inner=inner, i=i):      # (called by step() between the vehicle's step and everything that reads the pose)
            if float32_inputs:
                o.state[0:3] += shifts[i]
            return inner()
        o._ray_distances = rays
        ob, rew, done, _ = o.step(act[:n_u], noise=0.0)
        out["bits"][i], out["done"][i], out["obs"][i], out["reward"][i] = int(np.dot(o.conditions, pw)), done, ob[:16], rew
        out["nav"][i] = o.delta_d, o.delta_theta, o.delta_psi
        out["state"][i], out["u"][i, :n_u], out["terms"][i] = o.state, o.u, o.last_reward_arr
        s = o.state
        with np.errstate(all="ignore"):
            out["ratio"][i] = np.concatenate([[1 - np.log(o.delta_d / DMAX) / np.log(DTOL / DMAX), o.delta_theta / (math.pi / 2), o.delta_psi / math.pi],
                                              s[6:9] / VEL_MAX[0:3], s[3:5] / MATT, [math.sin(s[5]), math.cos(s[5])], s[9:12] / VEL_MAX[3:6],
                                              o.nu_c[0:3] / 2])
        with np.errstate(all="ignore"):         # (the LAUV's explicit step runs away from some of these states in its second step)
            ob, _, _, _ = o.step(act[:n_u], noise=0.0)
        out["state2"][i], out["obs2"][i], out["bits2"][i] = o.state, ob[:16], int(np.dot(o.conditions, pw))
    return out


def threshold_distance(scene, ev):
    """per env: the reference's distance from the nearest threshold the case was built next to (inf: none)"""
    N = scene["state"].shape[0]
    d = np.full(N, np.inf)
    for i in range(N):
        for key in scene["near"][i]:
            if key == "dtol":
                v = abs(ev["nav"][i, 0] - DTOL)
            elif key == "dmax":
                v = abs(ev["nav"][i, 0] - DMAX)
            elif key == "att":
                v = np.abs(np.abs(ev["state"][i, 3:5]) - MATT).min()
            elif key == "dpsi":
                v = math.pi - abs(ev["nav"][i, 2])
            else:
                v = abs(abs(ev["ratio"][i, int(key[3:])]) - 1.0)
            d[i] = min(d[i], v)
    return d


def qualify(scene, ev64, ev32):
    dist = threshold_distance(scene, ev64)
    same = ev64["bits"] == ev32["bits"]
    f64_only = np.isin(scene["group"], F64_ONLY)
    return dict(qualified=same & (dist >= MARGIN) & ~f64_only, dist=dist, f64_only=f64_only)


def circle(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return np.minimum(d, np.abs(2 * np.pi - d))


def reference_movement(scene, ev64, ev32, q):
    """per yardstick group: the largest movement of a qualified case's observation entries [16], reward terms [13], total
    reward, navigation errors [3] and heading between the two evaluations -- the reference's own sensitivity to float32 inputs"""
    out = {}
    for g in np.unique(scene["group"]):
        m = (scene["group"] == g) & q["qualified"]
        if not m.any():
            continue
        out[str(g)] = dict(obs=np.abs(ev64["obs"][m] - ev32["obs"][m]).max(axis=0), terms=np.abs(ev64["terms"][m] - ev32["terms"][m]).max(axis=0),
                           reward=float(np.abs(ev64["reward"][m] - ev32["reward"][m]).max()),
                           obs2=np.abs(ev64["obs2"][m] - ev32["obs2"][m]).max(axis=0),
                           psi=float(circle(ev64["state"][m, 5], ev32["state"][m, 5]).max()),
                           psi2=float(circle(ev64["state2"][m, 5], ev32["state2"][m, 5]).max()))
    return out


# ------------------------------------------------------------------------------------------------ the bounds
# (plain NumPy: the host test holds the oracle's float32-input evaluation to them, the GPU tests the kernels)
TOL = {"f64": dict(state=1e-9, obs=3e-7, rew_rel=1e-9, rew_abs=1e-9, nav=1e-9),        # tests/helpers.py: TOL
       "f32": dict(state=3e-5, obs=1e-5, rew_rel=2e-5, rew_abs=2e-5, nav=2e-5)}
# goal ON p+: the bearing and the elevation of a zero vector.  The reference answers atan2(0, 0) = 0; a kernel whose p+ differs
# in the last bit answers +-pi/2 and any bearing.  Its distance, observation 0, reward term 0 and condition bits are held.
NO_ANGLES = ("goal-close/0",)
# float32: a goal 1e-6 m from p+ is nearer than SHIFT, the reference's own bearing and elevation turn by up to pi between its two
# evaluations and 8 e_ref would bound nothing: the angle outputs of that group are not compared in float32 either
NO_ANGLES_F32 = NO_ANGLES + ("goal-close/1e-06",)
ANGLE_OBS, ANGLE_TERMS = (1, 2), (1, 2)


def clipped(ev):
    """entries the reference clips: the unclipped value lies on or beyond +-1 (column 0: on or beyond 0 / 1).  An entry that is
    +-1 only after the cast to float32 (cos psi of a small heading) is an ordinary value."""
    with np.errstate(invalid="ignore"):
        m = np.abs(ev["ratio"]) >= 1.0
        m[:, 0] |= ev["ratio"][:, 0] <= 0.0
    return m


def _worst(err, bound, scene, idx):
    r = err / bound
    k = np.unravel_index(np.nanargmax(r), r.shape)
    i = idx[k[0]]
    return float(np.nanmax(r)), f"{r[k]:.3f} x its bound ({err[k]:.3e}) at env {i} ({scene['label'][i]} {scene['sub'][i]}), column {k[1:]}"


def check_f64(name, b, out):
    """float64: bits and done equal, the clipped entries exact, everything else within TOL["f64"] (module docstring of
    tests/test_gpu_nav_edges.py).  out: obs [N, 16], reward, done, state [N, 12], u [N, 8]; optional bits, nav [N, 3], terms"""
    sc, ev = b["scene"], b["ev64"]
    tol = TOL["f64"]
    if out.get("bits") is not None:
        diff = np.flatnonzero(out["bits"] != ev["bits"])
        assert diff.size == 0, f"{name}: condition bits differ at {[(int(i), sc['sub'][i], int(out['bits'][i]), int(ev['bits'][i])) for i in diff[:6]]}"
    diff = np.flatnonzero(out["done"] != ev["done"])
    assert diff.size == 0, f"{name}: done differs at {[(int(i), sc['sub'][i]) for i in diff[:6]]}"
    angles = ~np.isin(sc["group"], NO_ANGLES)
    cm = clipped(ev)
    cm[np.ix_(~angles, ANGLE_OBS)] = False
    bad = np.argwhere(cm & (out["obs"] != ev["obs"]))
    assert bad.size == 0, f"{name}: clipped entries differ, first {[(int(i), sc['sub'][i], int(k), out['obs'][i, k]) for i, k in bad[:6]]}"
    oerr = np.abs(out["obs"] - ev["obs"])
    oerr[np.ix_(~angles, ANGLE_OBS)] = 0.0
    assert oerr.max() <= tol["obs"], f"{name}: observation {_worst(oerr, np.full_like(oerr, tol['obs']), sc, np.arange(oerr.shape[0]))[1]}"
    serr = np.abs(out["state"] - ev["state"])
    serr[:, 5] = circle(out["state"][:, 5], ev["state"][:, 5])
    assert serr.max() <= tol["state"], f"{name}: state off by {serr.max():.3e}"
    assert (out["state"][:, 5] >= -np.pi).all() and (out["state"][:, 5] < np.pi).all(), f"{name}: heading outside [-pi, pi)"
    assert np.abs(out["u"] - ev["u"]).max() <= 1e-9 * max(1.0, np.abs(ev["u"]).max()), f"{name}: filtered input off"
    if out.get("nav") is not None:
        nerr = np.abs(out["nav"] - ev["nav"])
        nerr[~angles, 1:] = 0.0
        assert nerr.max() <= tol["nav"], f"{name}: navigation errors off by {nerr.max():.3e} at {np.unravel_index(nerr.argmax(), nerr.shape)}"
    rb = tol["rew_abs"] + tol["rew_rel"] * np.abs(ev["reward"])
    if out.get("terms") is not None:
        terr = np.abs(out["terms"] - ev["terms"])
        terr[np.ix_(~angles, ANGLE_TERMS)] = 0.0
        tb = tol["rew_abs"] + tol["rew_rel"] * np.abs(ev["terms"])
        assert (terr <= tb).all(), f"{name}: reward term {_worst(terr, tb, sc, np.arange(terr.shape[0]))[1]}"
    rerr = np.abs(out["reward"] - ev["reward"])[angles]
    assert (rerr <= rb[angles]).all(), f"{name}: reward off by {rerr.max():.3e}"
    return float(oerr.max())


def check_f32(name, b, out, rew_floor=0.0):
    """float32, on the float32-qualified cases: no bit flip, done equal, the clipped entries exact, every other obs[:16] entry
    within max(8 e_ref, TOL obs) -- obs[2] directly, not on the circle --, each reward term and the total within max(8 e_ref,
    rew_abs + rew_rel |ref|), the heading within TOL state on the circle and inside [-pi, pi).  e_ref: reference_movement of
    the case's yardstick group.  rew_floor: a packed row carries the reward as float32 (half an ulp of |ref|).  Returns
    {class: largest error / bound}."""
    sc, ev, q, move = b["scene"], b["ev64"], b["q"], b["move"]
    tol = TOL["f32"]
    ok = q["qualified"]
    ratios = {}
    for g in np.unique(sc["group"][ok]):
        idx = np.flatnonzero(ok & (sc["group"] == g))
        cls = str(sc["label"][idx[0]])
        mv = move[str(g)]
        if out.get("bits") is not None:
            flip = idx[out["bits"][idx] != ev["bits"][idx]]
            assert flip.size == 0, f"{name} {g}: bit flips at {[(int(i), sc['sub'][i], int(out['bits'][i]), int(ev['bits'][i])) for i in flip[:6]]}"
        flip = idx[out["done"][idx] != ev["done"][idx]]
        assert flip.size == 0, f"{name} {g}: done flips at {[(int(i), sc['sub'][i]) for i in flip[:6]]}"
        o, o_ref = out["obs"][idx], ev["obs"][idx]
        cm = clipped(ev)[idx]
        bad = np.argwhere(cm & (o != o_ref))
        assert bad.size == 0, f"{name} {g}: clipped entries differ, first {[(int(idx[i]), sc['sub'][idx[i]], int(k), o[i, k]) for i, k in bad[:6]]}"
        oerr = np.where(cm, 0.0, np.abs(o - o_ref))
        angles = str(g) not in NO_ANGLES_F32
        if not angles:
            oerr[:, ANGLE_OBS] = 0.0
        r_o, msg = _worst(oerr, np.broadcast_to(np.maximum(8 * mv["obs"], tol["obs"]), oerr.shape), sc, idx)
        assert r_o <= 1.0, f"{name} {g}: observation {msg}"
        perr = circle(out["state"][idx, 5], ev["state"][idx, 5])
        assert perr.max() <= tol["state"], f"{name} {g}: heading off by {perr.max():.3e} on the circle"
        assert (out["state"][idx, 5] >= -np.pi).all() and (out["state"][idx, 5] < np.pi).all(), f"{name} {g}: heading outside [-pi, pi)"
        r_t = 0.0
        if out.get("terms") is not None:
            terr = np.abs(out["terms"][idx] - ev["terms"][idx])
            if not angles:
                terr[:, ANGLE_TERMS] = 0.0
            tb = np.maximum(8 * mv["terms"][None, :], tol["rew_abs"] + tol["rew_rel"] * np.abs(ev["terms"][idx]))
            r_t, msg = _worst(terr, tb, sc, idx)
            assert r_t <= 1.0, f"{name} {g}: reward term {msg}"
        rerr = np.abs(out["reward"][idx] - ev["reward"][idx]) * (1.0 if angles else 0.0)
        rb = np.maximum(8 * mv["reward"], tol["rew_abs"] + (tol["rew_rel"] + rew_floor) * np.abs(ev["reward"][idx]))
        r_r = float((rerr / rb).max())
        assert r_r <= 1.0, f"{name} {g}: reward {r_r:.3f} x its bound at env {idx[(rerr / rb).argmax()]}"
        ratios[cls] = max(ratios.get(cls, 0.0), r_o, r_t, r_r)
    return ratios


# ------------------------------------------------------------------------------------------------ shared, computed once
_BUNDLES = {}


def bundle(vehicle="BlueROV2", with_current=False, max_capsules=0, max_spheres=0, reward_set=1, seed=1, n_envs=N_ENVS, classes=CLASSES):
    """scene + both oracle evaluations + qualification + the reference's own movement, computed once per process and left
    unchanged (the arrays are read-only).  Scenes of different reward sets share their inputs."""
    skey = (vehicle, with_current, max_capsules, max_spheres, seed, n_envs, tuple(classes))
    key = skey + (reward_set,)
    if key not in _BUNDLES:
        if ("scene",) + skey not in _BUNDLES:
            _BUNDLES[("scene",) + skey] = make_scene(vehicle, with_current, max_capsules, max_spheres, seed, n_envs, classes)
        scene = _BUNDLES[("scene",) + skey]
        ev64, ev32 = evaluate(scene, reward_set=reward_set), evaluate(scene, float32_inputs=True, reward_set=reward_set)
        q = qualify(scene, ev64, ev32)
        for d in (scene, ev64, ev32, q):
            for v in d.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _BUNDLES[key] = dict(scene=scene, ev64=ev64, ev32=ev32, q=q, move=reference_movement(scene, ev64, ev32, q))
    return _BUNDLES[key]
