"""CPU: the constructed states of tests/nav_scenes.py deliver what tests/test_gpu_nav_edges.py relies on -- every class with both
sides of its threshold, every requested combination of condition bits in the float64 oracle evaluation, the built margins, the
float32 qualification caps -- and the oracle's own evaluation on float32 inputs stays inside the bounds the kernels are held to."""
import numpy as np
import pytest

from tests import nav_scenes as S

SCENES = [("BlueROV2", True, 1, 0), ("LAUV", True, 1, 0), ("mixed", False, 0, 0)]
IDS = [f"{v}-{'current' if c else 'still'}-{a}+{b}" for v, c, a, b in SCENES]


@pytest.mark.parametrize("vehicle,current,C,Sp", SCENES, ids=IDS)
def test_classes_sides_bits_and_margins(vehicle, current, C, Sp):
    b = S.bundle(vehicle, current, C, Sp)
    sc, ev, q = b["scene"], b["ev64"], b["q"]
    assert sc["state"].shape[0] % 64 != 0
    assert set(sc["label"]) == set(S.CLASSES)
    for cls in ("goal-tol", "goal-far", "attitude", "behind", "saturation"):
        sides = set(sc["side"][sc["label"] == cls].tolist())
        assert {-1, 1} <= sides, f"{cls}: sides {sides}"
    for cls in ("goal-tol", "goal-far", "attitude", "behind"):
        m = sc["label"] == cls
        assert set(sc["margin"][m & (sc["margin"] > 0)].tolist()) == set(S.MARGINS), cls
    # the requested bits are the oracle's, and every requested combination occurs
    want = sc["bits"] >= 0
    diff = np.flatnonzero(want & (sc["bits"] != ev["bits"]))
    assert diff.size == 0, [(sc["sub"][i], int(sc["bits"][i]), int(ev["bits"][i])) for i in diff[:8]]
    combos = {0, 1, 2, 4, 8, 1 | 8, 2 | 4, 4 | 8, 2 | 4 | 8} | ({4 | 16, 1 | 8 | 16} if C + Sp else set())
    assert combos <= set(ev["bits"].tolist()), combos - set(ev["bits"].tolist())
    assert np.array_equal(ev["done"], ev["bits"] != 0)
    # Q12: the weights of all fired conditions add in the reward
    w = np.array([400.0, -200.0, -200.0, -100.0, -300.0])
    fired = (ev["bits"][:, None] >> np.arange(5)[None, :] & 1).astype(float)
    assert np.array_equal(ev["terms"][:, 8:13], fired * w[None, :])
    # the built margins hold
    m = sc["margin"] > 0
    assert np.abs(q["dist"][m] - sc["margin"][m]).max() < 1e-9, np.abs(q["dist"][m] - sc["margin"][m]).max()
    sat = np.array([bool(n) and n[0].startswith("sat") for n in sc["near"]])
    below = q["dist"][sat & (sc["side"] < 0)]      # 0.99 x a velocity maximum, 1.9 m/s of 2
    assert (q["dist"][sat & (sc["side"] > 0)] > 0.2).all() and (below > 0.0099).all() and (below < 0.0501).all()
    # what the classes are about
    o = ev["obs"]
    assert (o[(sc["label"] == "goal-tol") & (sc["side"] < 0), 0] == 0).all() and (o[(sc["label"] == "goal-tol") & (sc["side"] > 0), 0] > 0).all()
    assert (o[(sc["label"] == "goal-far") & (sc["side"] > 0), 0] == 1).all() and (o[(sc["label"] == "goal-far") & (sc["side"] < 0), 0] < 1).all()
    att = sc["label"] == "attitude"
    assert (np.abs(o[att & (sc["side"] > 0), 6:8]).max(axis=1) == 1).all() and (np.abs(o[att & (sc["side"] < 0), 6:8]).max(axis=1) < 1).all()
    behind = (sc["label"] == "behind") & (sc["margin"] > 0)
    assert np.array_equal(np.sign(ev["nav"][behind, 2]), sc["side"][behind]) and (np.abs(ev["nav"][behind, 2]) > 3.14).all()
    zero = sc["group"] == "behind/zero"
    assert (ev["nav"][zero, 2] == -np.pi).all() and (o[zero, 2] == -1).all()
    on = sc["group"] == "goal-close/0"
    assert (ev["nav"][on, 0] == 0).all() and (o[on, 0] == 0).all() and np.isfinite(ev["reward"][on]).all()
    vert = sc["group"] == "vertical/exact"
    assert np.abs(np.abs(ev["nav"][vert, 1] - ev["state"][vert, 4]) - np.pi / 2).max() < 1e-15
    # the heading wrap: a first step across +-pi, a second step across it, and twins that stay short
    hw = sc["label"] == "heading-wrap"
    psi0, psi1, psi2 = sc["state"][hw, 5], ev["state"][hw, 5], ev["state2"][hw, 5]
    sub = np.char.partition(sc["sub"][hw], "+")[:, 0]
    sub = np.char.partition(sub, "-")[:, 0]
    assert (np.sign(psi0[sub == "cross"]) != np.sign(psi1[sub == "cross"])).all()
    assert (np.sign(psi0[sub == "short"]) == np.sign(psi1[sub == "short"])).all() and (np.sign(psi0[sub == "short"]) == np.sign(psi2[sub == "short"])).all()
    assert (np.sign(psi1[sub == "second"]) != np.sign(psi2[sub == "second"])).all()
    assert (np.abs(ev["state"][:, 5]) <= np.pi).all()
    # raw and clipped actions: the same post-step state and input, another action penalty
    raw = np.flatnonzero(sc["twin"] >= 0)
    assert raw.size >= 5
    assert np.array_equal(ev["state"][raw], ev["state"][sc["twin"][raw]]) and np.array_equal(ev["u"][raw], ev["u"][sc["twin"][raw]])
    assert (ev["terms"][raw, 7] < 2.0 * ev["terms"][sc["twin"][raw], 7]).all()
    if current:
        cur = np.array([s.startswith("current") for s in sc["sub"]])
        assert (np.abs(o[cur & (sc["side"] > 0), 13:16]).max(axis=1) == 1).all()
        assert np.abs(np.abs(o[cur & (sc["side"] < 0), 13:16]).max(axis=1) - 0.95).max() < 1e-6


@pytest.mark.parametrize("vehicle,current,C,Sp", SCENES, ids=IDS)
def test_qualification_caps_and_the_oracles_own_movement(vehicle, current, C, Sp):
    b = S.bundle(vehicle, current, C, Sp)
    sc, ev, q = b["scene"], b["ev64"], b["q"]
    assert set(sc["group"][q["f64_only"]]) == set(S.F64_ONLY)      # the float64-only cases, by name
    for cls in S.CLASSES:
        m = (sc["label"] == cls) & ~q["f64_only"]
        share = q["qualified"][m].mean()
        print(f"{vehicle} {cls}: {m.sum()} cases, {share:.3f} float32-qualified")
        assert share >= 0.9, f"{cls}: only {share:.3f} of the cases are float32-qualified"
    # the oracle on float32 inputs against the oracle on float64 inputs, by the float32 bounds of the GPU test
    ratios = S.check_f32(f"{vehicle} oracle on float32 inputs", b, b["ev32"])
    print({k: round(v, 3) for k, v in ratios.items()})
    assert set(ratios) == set(S.CLASSES) and max(ratios.values()) <= 1.0
    # ... and against itself by the float64 ones
    assert S.check_f64(f"{vehicle} oracle", b, ev) == 0.0


def test_reward_set_two_shares_the_inputs():
    b1, b2 = S.bundle("BlueROV2", True, 1, 0), S.bundle("BlueROV2", True, 1, 0, reward_set=2)
    assert b1["scene"] is b2["scene"] and np.array_equal(b1["ev64"]["obs"], b2["ev64"]["obs"])
    assert not np.array_equal(b1["ev64"]["terms"][:, 1:3], b2["ev64"]["terms"][:, 1:3])
    assert np.array_equal(b1["ev64"]["terms"][:, 8:13], b2["ev64"]["terms"][:, 8:13])
