"""The lamp sampler at its limits, without a GPU.

The census (tests/light_census.py): for hostile lamp tables the exact number of generator states that pick each lamp, taken from the
library's own header on the host (ptc_check_light_sample) and from the numpy restatement (tests/direct_ref.py), against each lamp's
share w_k / W in float64 -- and the rule the library had before, restated, against the same bounds, which it breaks.

The sample against float64 (tests/light_f64.py): per sample, over classes of far scenes, extreme sizes, points in a lamp's plane, on it
and inside it, distant lamps and edge draws."""
import numpy as np
import pytest

import direct_ref as D
import light_census as LC
import light_f64 as L64


@pytest.fixture(scope="module")
def tables(pkg):
    return LC.tables(pkg)


@pytest.mark.parametrize("name", ["one_tiny_one", "one_tinier", "sky_then_bulb", "bulb_then_sky", "one_small_one", "uniform_2_20",
                                  "uniform_2_17", "uniform_2_14", "dead_lamps", "thousand_specks", "single"])
def test_census(pkg, tables, name):
    """Every state of the generator picks a lamp; a lamp of weight 0 owns none, one of weight > 0 at least one, and each is within
    1 + m states of its share p_k N (m = the live lamps whose share is below one state: what the thresholds' construction gives, no
    measurement); v = 1 and v = 2^31 - 2 pick the first and the last live lamp; library and restatement agree on every boundary."""
    flat = LC.table_scene(pkg, tables[name]).build_scene(distinct_meshes=True)
    weights = LC.flat_weights(flat)
    recs, info, ref_weights, last = D.light_table(flat)
    assert info["lights"] == len(weights) and np.array_equal(ref_weights, weights)   # (exact by construction: table_scene)
    live = np.nonzero(weights > 0.0)[0]
    assert last == live[-1]
    states, bounds = LC.census(LC.library_sampler(pkg, flat), len(weights))
    ref_states, ref_bounds = LC.census(LC.restatement_sampler(weights, last), len(weights))
    assert np.array_equal(bounds, ref_bounds)
    share = weights / np.sum(weights) * LC.N
    print(name, "lamps", len(weights), "live", len(live), "worst |states - share|", float(np.max(np.abs(states - share))),
          "states / share over the live lamps", float(np.min(states[live] / share[live])), "..", float(np.max(states[live] / share[live])))
    assert LC.check_bounds(states, weights) == []
    ends = LC.library_sampler(pkg, flat)(np.array([1, LC.N], dtype=np.uint32))
    assert ends.tolist() == [live[0], live[-1]]
    # the thresholds are the boundaries: lamp k's T_k is the first n = v - 1 of a later lamp
    assert np.array_equal(D.thresholds(weights)[:last].astype(np.int64), bounds[:last] - 1) and np.all(bounds[last:] == LC.N + 1)


@pytest.mark.parametrize("name", LC.PARENT_FAILS)
def test_the_rule_before_breaks_these_bounds(pkg, tables, name):
    """The test's power, on record: a binary search of u0 = float(v - 1) / 2^31 in the binary32 cdf never picks the middle lamp of
    (1, 1e-8, 1), and picks the small lamp of (1, 1e-9) and the bulb beside the sky by the 62 states whose u0 rounds to 1.0f."""
    flat = LC.table_scene(pkg, tables[name]).build_scene(distinct_meshes=True)
    weights = LC.flat_weights(flat)
    last = int(np.nonzero(weights > 0.0)[0][-1])
    states, _ = LC.census(LC.parent_rule(weights, last), len(weights))
    share = weights / np.sum(weights) * LC.N
    print(name, "states", states.tolist(), "share", share.tolist())
    assert int(states.sum()) == LC.N
    assert LC.check_bounds(states, weights) != []
    want = {"one_tiny_one": (1, 0), "one_tinier": (1, 62), "sky_then_bulb": (1, 62)}
    if name in want:
        k, n = want[name]
        assert states[k] == n


def test_every_lamp_dark(pkg, orc):
    """A table of weight 0: nothing is picked, nothing sampled, by either."""
    flat = LC.all_dark_scene(pkg).build_scene(distinct_meshes=True)
    assert not LC.flat_weights(flat).any() and pkg.light_table(flat)[1]["total_weight"] == 0.0
    v = np.array([1, 2, 2 ** 30, LC.N], dtype=np.uint32)
    p, nrm = np.zeros((4, 3), dtype=np.float32), np.tile(np.float32([0, 1, 0]), (4, 1))
    got = pkg.check_light_sample(flat, p, nrm, v, np.full((4, 2), 0.5))
    assert not got["sampled"].any() and not got["contribution"].any() and not got["lamp"].any()
    assert np.array_equal(got["rays"], D.sample(orc, flat, p, nrm, 0)["rays"])


@pytest.fixture(scope="module")
def f64_classes(pkg):
    return L64.classes(pkg)


def f64_outcome(pkg, orc, cases, tol, samplers=("library", "restatement")):
    """The comparison of one class: -> (worst distances per sampler, samples, samples left out).  Asserts what holds exactly: the lamp
    picked, the `sampled` flags and the zeros of a culled sample outside near_cull, and the bytes of library against restatement."""
    worst = {who: np.zeros(3) for who in samplers}
    total = left_out = 0
    for case in cases:
        flat, p, nrm, v, u = case["flat"], case["p"], case["nrm"], case["v"], case["u"]
        ref = L64.sample64(flat, case["recs"], case["lamp"], p, nrm, u[:, 0], u[:, 1])
        keep = ~L64.near_cull(ref, tol)
        total, left_out = total + len(p), left_out + int((~keep).sum())
        got = {}
        if "library" in samplers:
            got["library"] = pkg.check_light_sample(flat, p, nrm, v, u)
        if "restatement" in samplers:
            got["restatement"] = D.light_sample(orc, flat, D.light_table(flat), p, nrm, (v, u))
        for who, g in got.items():
            assert np.array_equal(g["lamp"], case["lamp"]), who
            assert np.array_equal(g["sampled"][keep], ref["sampled"][keep]), who
            culled = keep & ~ref["sampled"]
            assert not g["rays"][culled, 4:].any() and not g["contribution"][culled].any(), who
            assert np.array_equal(g["rays"][:, :4], np.concatenate([p, np.full((len(p), 1), 1e-4, dtype=np.float32)], axis=1)), who
            worst[who] = np.maximum(worst[who], L64.distances(g, ref, keep))
        if len(got) == 2:
            for key in ("rays", "contribution", "sampled"):
                assert got["library"][key].tobytes() == got["restatement"][key].tobytes(), key
    return worst, total, left_out


@pytest.mark.parametrize("name", list(L64.TOLERANCE))
def test_sample_against_float64(pkg, orc, f64_classes, name):
    """Per sample: the library's header on the host and the restatement against float64 -- equal `sampled` flags, direction, tmax and
    contribution within TOLERANCE (four times the restatement's own measured worst, in conditioning-scaled units of 2^-24), at most
    1 % of a class left out as too close to a cull for float64 to call."""
    tol = L64.TOLERANCE[name]
    worst, total, left_out = f64_outcome(pkg, orc, f64_classes[name], tol)
    print(name, "samples", total, "left out", left_out, "worst distances (direction, tmax, contribution)",
          {who: [round(float(x), 3) for x in w] for who, w in worst.items()}, "tolerance", tol)
    assert total >= 1000 and left_out <= 0.01 * total
    for who, w in worst.items():
        assert np.all(w <= np.asarray(tol)), (who, w, tol)


def test_the_classes_are_what_they_claim(f64_classes):
    """Each class reaches the edge it is named for, by float64's own account."""
    ref = lambda c: L64.sample64(c["flat"], c["recs"], c["lamp"], c["p"], c["nrm"], c["u"][:, 0], c["u"][:, 1])
    for c in f64_classes["far"]:
        assert np.min(np.abs(c["p"])) > 900.0 and ref(c)["sampled"].mean() > 0.8
    edges = [float(np.linalg.norm(c["recs"]["e1"][0])) for c in f64_classes["sizes"]]
    assert edges[0] == np.float32(1e-4) and edges[1] == 1e4 and abs(edges[2] - 1e-4) < 1e-10 and abs(edges[3] - 1000.0) < 1e-3
    in_plane, on_vertex, close = (ref(c) for c in f64_classes["plane"])
    assert np.all(in_plane["cos_l"] == 0.0) and in_plane["sampled"].mean() > 0.95 and not in_plane["contribution"].any()
    assert np.all(on_vertex["d2"] == 0.0) and not on_vertex["sampled"].any()
    assert np.all(close["d"] < 1e-4) and np.all(close["d"] >= 1e-6) and close["sampled"].mean() > 0.9
    inside = ref(f64_classes["inside"][0])
    assert np.all(np.abs(inside["d"][:100] - 1.0) < 1e-6) and np.all(inside["d"] < 2.0)   # (the centre: d = the world radius) and 0.5 < inside["sampled"].mean() < 0.95
    normals = ref(f64_classes["normals"][0])
    assert 0.2 < np.mean(np.abs(normals["cos_r"]) < 2e-3) < 0.5 and 0.2 < np.mean(normals["cos_r"] < -0.4) < 0.5
    c = f64_classes["distant"][0]
    distant = ref(c)
    assert not distant["valid"][c["lamp"] < 2].any() and np.all(np.isfinite(distant["d2"])) and distant["sampled"][c["lamp"] == 2].mean() > 0.5
    assert len(f64_classes["edge_draws"]) == 9 and {tuple(c["u"][0]) for c in f64_classes["edge_draws"]} == {
        (a, b) for a in np.float32([0.0, 1.0, L64.BELOW_ONE]) for b in np.float32([0.0, 1.0, L64.BELOW_ONE])}


def test_refusals_of_the_host_twin(pkg):
    flat = LC.table_scene(pkg, [("mesh", 1.0, [1.0])]).build_scene(distinct_meshes=True)
    p, nrm, u = np.zeros((1, 3), dtype=np.float32), np.float32([[0, 1, 0]]), np.float32([[0.5, 0.5]])
    for bad in (0, 2 ** 31 - 1, 2 ** 32 - 1):
        with pytest.raises(pkg.PtcError) as e:
            pkg.check_light_sample(flat, p, nrm, np.array([bad], dtype=np.uint32), u)
        assert e.value.code == pkg._capi.PTC_ERR_INVALID
    squashed = D.sphere_lamp_scene(pkg, pkg.glmlite.compose([pkg.glmlite.scale((0.45, 0.3, 0.4)), pkg.glmlite.translate((0.0, 1.0, 0.0))]))
    with pytest.raises(pkg.PtcError) as e:
        pkg.check_light_sample(squashed, p, nrm, np.array([1], dtype=np.uint32), u)
    assert e.value.code == pkg._capi.PTC_ERR_INVALID and "sphere" in str(e.value)
    assert len(pkg.check_light_sample(flat, p[:0], nrm[:0], np.zeros(0, dtype=np.uint32), u[:0])["lamp"]) == 0
