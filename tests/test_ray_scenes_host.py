"""CPU: the constructed ray scenes of tests/ray_scenes.py deliver what tests/test_gpu_ray_edges.py relies on -- the
qualification caps, every class, rim / rim-miss pairs that bracket the boundary, tau* capsules whose point of closest angle is
interior, slot counts that differ inside every 64-env group -- and agree with the geometric claim behind the step kernel's
obstacle culling (dockauv_step.hip.inc, "obstacle culling"), stated here in plain NumPy from the comment: an obstacle that a ray
of the fan enters within ray_max has SOME axis point within theta_f + rho of +x (theta_f: the largest angle between a ray and
+x, rho = asin(r / d_min), d_min the origin's distance from the axis) and d_min - r <= ray_max -- or holds the origin."""
import numpy as np
import pytest

from tests import ray_scenes as S

FAN_SLOTS = [("7x9", 3, 3), ("4x4", 3, 3), ("9x13", 2, 2), ("2x2", 2, 2)]
IDS = [f"{f}-{c}+{s}" for f, c, s in FAN_SLOTS]


def _kind(sub):
    return "sphere" if sub.split("/")[0] == "sphere" else "capsule"


@pytest.mark.parametrize("fan_name,C,Sp", FAN_SLOTS, ids=IDS)
def test_scene_meets_the_caps_and_holds_every_class(fan_name, C, Sp):
    b = S.bundle(fan_name, C, Sp)
    sc, ev, q = b["scene"], b["ev64"], b["q"]
    fan = sc["fan"]
    assert set(sc["label"]) == set(S.CLASSES)
    for cls in S.CLASSES:
        m = sc["label"] == cls
        share = q["qualified"][m].mean()
        print(f"{fan_name} {cls}: {m.sum()} cases, {share:.3f} float32-qualified")
        if cls != "axis-aligned":
            assert share >= 0.9, f"{cls}: only {share:.3f} of the cases are float32-qualified"
    hit = ev["dist"] < fan.max_dist
    assert hit.mean() >= 0.3, f"{hit.mean():.3f} of the rays in range"
    corners, edges, _ = S.extreme_rays(fan)
    for k in corners + edges:
        for kind in ("sphere", "capsule"):
            alone = [i for i in np.flatnonzero((sc["label"] == "rim") & sc["lone"] & (sc["target"] == k))
                     if _kind(sc["sub"][i]) == kind and np.array_equal(np.flatnonzero(hit[i]), [k])]
            assert alone, f"no rim case in which ray {k} alone reaches a {kind}"
    # a level share, and general attitudes
    level = (sc["state"][:, 3:6] == 0).all(axis=1)
    assert 0.1 < level.mean() < 0.5 and np.abs(sc["state"][~level, 3:5]).max() <= 0.6


@pytest.mark.parametrize("fan_name,C,Sp", FAN_SLOTS, ids=IDS)
def test_rim_pairs_bracket_the_boundary(fan_name, C, Sp):
    b = S.bundle(fan_name, C, Sp)
    sc, ev = b["scene"], b["ev64"]
    R = sc["fan"].max_dist
    for i in np.flatnonzero(sc["label"] == "rim"):
        k = sc["target"][i]
        assert ev["dist"][i, k] < R - 0.04, (i, sc["sub"][i])
        if sc["lone"][i]:
            assert np.array_equal(np.flatnonzero(ev["dist"][i] < R), [k]), (i, sc["sub"][i])
    n_none = 0
    for i in np.flatnonzero(sc["label"] == "rim-miss"):
        assert ev["dist"][i, sc["target"][i]] == R, (i, sc["sub"][i])
        if not sc["sub"][i].endswith("/filled"):
            assert (ev["dist"][i] == R).all(), (i, sc["sub"][i])
            n_none += 1
    assert n_none >= 4
    # both members of a pair come from the same construction: per (ray, variant) there is a hit and a miss
    def pairs(cls):
        return {(int(sc["target"][i]), sc["sub"][i].split("/")[0]) for i in np.flatnonzero(sc["label"] == cls)}
    assert pairs("rim") == pairs("rim-miss")


@pytest.mark.parametrize("fan_name,C,Sp", FAN_SLOTS, ids=IDS)
def test_tau_capsules_have_their_closest_angle_point_inside_the_segment(fan_name, C, Sp):
    b = S.bundle(fan_name, C, Sp)
    sc, ev = b["scene"], b["ev64"]
    fan = sc["fan"]
    theta_f = np.arccos(fan.rd_b[:, 0].min())
    signs = set()
    for i in np.flatnonzero(np.char.startswith(sc["sub"], "tau")):
        a, bb, r = S.body_frame(sc, ev, i)[0][-1]
        s = np.linspace(0.0, 1.0, 4001)[:, None]
        X = a[None, :] + s * (bb - a)[None, :]
        cosang = X[:, 0] / np.linalg.norm(X, axis=1)
        j = int(cosang.argmax())
        assert 100 < j < 3900, f"env {i}: the axis point of closest angle is an end"
        for e in (a, bb):    # both ends outside the widened cone
            assert np.arccos(e[0] / np.linalg.norm(e)) > theta_f + np.arcsin(r / np.linalg.norm(e))
        d = (bb - a) / np.linalg.norm(bb - a)
        oa_perp = -a + float(a @ d) * d
        assert oa_perp[0] < 0
        signs.add(bool(-d[0] * float(oa_perp @ oa_perp) / oa_perp[0] > 0))    # tau* as the kernel's comment writes it
    assert signs == {True, False}, "tau* of both signs"


@pytest.mark.parametrize("fan_name,C,Sp", FAN_SLOTS, ids=IDS)
def test_slot_counts_differ_inside_every_group(fan_name, C, Sp):
    sc = S.bundle(fan_name, C, Sp)["scene"]
    n = sc["state"].shape[0]
    for g in range(0, n, 64):
        pairs = set(zip(sc["ncap"][g:g + 64].tolist(), sc["nsph"][g:g + 64].tolist()))
        assert len(pairs) >= 3, f"group at env {g}: slot counts {pairs}"
    subs = set(sc["sub"][sc["label"] == "slots"])
    assert {"0+0", f"{C}+{Sp}", f"0+{Sp}", f"{C}+0"} <= subs
    if C >= 3:     # a closed slot in the middle of the list, real rows behind it
        i = int(np.flatnonzero(sc["sub"] == f"{C - 2}+{Sp}/cap")[0])
        rad = sc["capsules"][i].reshape(C, 7)[:, 6]
        assert rad[C - 2] <= 0 and rad[C - 1] > 0 and sc["ncap"][i] == C - 2


@pytest.mark.parametrize("fan_name,C,Sp", FAN_SLOTS, ids=IDS)
def test_every_in_range_hit_satisfies_the_culling_claim(fan_name, C, Sp):
    from oracle import dockauv_oracle as orc
    b = S.bundle(fan_name, C, Sp)
    sc, ev = b["scene"], b["ev64"]
    fan = sc["fan"]
    R = fan.max_dist
    theta_f = np.arccos(fan.rd_b[:, 0].min())
    n_true = n_false = 0
    for i in range(sc["state"].shape[0]):
        caps, sph = S.body_frame(sc, ev, i)
        any_true = False
        for ob in [(a, bb, r) for a, bb, r in caps] + [(c, c, r) for c, r in sph]:
            a, bb, r = ob
            X = a[None, :] + np.linspace(0.0, 1.0, 2001)[:, None] * (bb - a)[None, :]
            nrm = np.linalg.norm(X, axis=1)
            d_min = nrm.min()
            if d_min <= r:
                claim = True
            else:
                angle = np.arccos(np.clip(X[:, 0] / nrm, -1, 1)).min()
                claim = bool(angle <= theta_f + np.arcsin(r / d_min) and d_min - r <= R)
            if claim:
                any_true = True
                n_true += 1
                continue
            n_false += 1
            for k in range(fan.n_rays):     # the claim says no: then no ray enters it in range
                v = (orc.ray_spheres(np.zeros(3), fan.rd_b[k], a[None, :], np.array([r])) if a is bb
                     else orc.ray_capsule(np.zeros(3), fan.rd_b[k], a, bb, r))
                assert not 0 < v <= R, f"env {i} ({sc['label'][i]} {sc['sub'][i]}): ray {k} enters at {v} an obstacle the claim excludes"
        if (ev["dist"][i] < R).any():
            assert any_true, f"env {i} ({sc['label'][i]} {sc['sub'][i]}): hits, and no obstacle satisfies the claim"
    assert n_true > 100 and n_false > 20     # (the scene puts obstacles on both sides of the claim)
