"""The checkers of tests/test_gpu_materials.py, checked without a GPU, where they are about to be used: the scenes of
tests/material_cases.py (material parameters over their whole range, rays at the critical angle) through the two binary32
restatements of the material code -- oracle/oracle.c and tests/lit_ref.py, written by different routes -- which must agree
to the bit; the float64 reference of tests/material_f64.py against the oracle on the probe frames, within a tolerance that
is measured here and pinned there; and the censuses that say the scenes reach what they were built for (zero-vector
refractions, k == 0, the clamp, rejected metal directions, re-hits of the object just left).  Run with -s to see every figure."""
import numpy as np
import pytest

import lit_ref as lr
import loop_ref
import material_cases as mc
import material_f64 as f64

KEYS = ("color", "normal", "depth")
_cache = {}


def _walls(pkg):
    if "walls" not in _cache:
        _cache["walls"] = {k: (s, s.build_scene()) for k, s in mc.walls(pkg).items()}
    return _cache["walls"]


def _critical(pkg):
    if "critical" not in _cache:
        _cache["critical"] = [(name, kind, index, s, s.build_scene()) for name, kind, index, s in mc.critical_frames(pkg)]
    return _cache["critical"]


def _same(got, want, what):
    for k in KEYS:
        assert mc.mismatches(got[k], want[k]) == 0, (what, k, mc.mismatches(got[k], want[k]))
    assert got["rays"] == want["rays"], what
    if "live" in want:
        assert np.array_equal(got["live"], want["live"]), what


@pytest.mark.parametrize("name", ["wall", "wall_meshes", "wall_mesh_first", "three_balls"])
def test_the_two_restatements_agree_on_the_walls(pkg, orc, name):
    scene, flat = _walls(pkg)[name]
    w, h = scene.resolution
    sh = orc.SceneHandle(flat)
    with np.errstate(all="ignore"):   # the 1e12 albedos overflow to inf, and inf * 0 is NaN, in both restatements
        for mb in (2, 8):
            want = orc.render_streaming(flat, scene.camera, w, h, 0, mc.WALL_ITERS, mb, scene_handle=sh)
            _same(loop_ref.render_streaming(orc, flat, scene.camera, w, h, 0, mc.WALL_ITERS, mb, scene_handle=sh), want,
                  (name, mb, "streaming"))
        want = orc.render_megakernel(flat, scene.camera, w, h, 0, mc.WALL_ITERS, 8, scene_handle=sh)
        _same(loop_ref.render_megakernel(orc, flat, scene.camera, w, h, 0, mc.WALL_ITERS, 8, scene_handle=sh), want,
              (name, "megakernel"))


def test_the_two_restatements_agree_on_records_out_of_range(pkg, orc):
    """Index 0 and a NaN albedo: the oracle's walk ends (every path is cut at max_bounces, every intersection loop is over
    the scene's finite lists), both restatements put NaN in the same pixels, and it stays a part of the frame."""
    scene, flat = mc.wall_out_of_range(pkg)
    w, h = scene.resolution
    with np.errstate(all="ignore"):
        want = orc.render_streaming(flat, scene.camera, w, h, 0, mc.WALL_ITERS, 8)
        _same(loop_ref.render_streaming(orc, flat, scene.camera, w, h, 0, mc.WALL_ITERS, 8), want, "streaming")
    nan = np.isnan(want["color"]).any(axis=2)
    assert 100 < nan.sum() < 0.05 * w * h, int(nan.sum())


def test_the_two_restatements_agree_on_the_critical_frames(pkg, orc):
    w, h, n, mb = mc.CRIT_W, mc.CRIT_H, mc.CRIT_ITERS, mc.CRIT_MB
    with np.errstate(all="ignore"):   # a zero direction is normalised and intersected: 0 / 0 and 1 / 0 on purpose
        for name, kind, index, scene, flat in _critical(pkg):
            sh = orc.SceneHandle(flat)
            want = orc.render_streaming(flat, scene.camera, w, h, 0, n, mb, scene_handle=sh)
            _same(loop_ref.render_streaming(orc, flat, scene.camera, w, h, 0, n, mb, scene_handle=sh), want, (name, "streaming"))
            want = orc.render_megakernel(flat, scene.camera, w, h, 0, n, mb, scene_handle=sh)
            _same(loop_ref.render_megakernel(orc, flat, scene.camera, w, h, 0, n, mb, scene_handle=sh), want, (name, "megakernel"))


def test_branch_census_of_the_critical_frames(pkg, orc):
    """Per frame: both sides of `cannot_refract`; per index: the zero-vector refractions and k == 0 the frames exist for."""
    w, h, n = mc.CRIT_W, mc.CRIT_H, mc.CRIT_ITERS
    zero_vector, k_zero, clamped = {}, {}, 0
    with np.errstate(all="ignore"):
        for name, kind, index, scene, flat in _critical(pkg):
            c = mc.glass_census(orc, lr, flat, scene.camera, w, h, n)
            print(name, c)
            front = index < 1.0
            assert c["back"] == (0 if front or kind != "critical" else c["glass"]), (name, c)
            if kind == "critical":
                assert c["cannot"] >= 100 and c["reflected"] + c["refracted"] >= 100, (name, c)
                zero_vector[index] = zero_vector.get(index, 0) + c["zero_vector"]
                k_zero[index] = k_zero.get(index, 0) + c["k_zero"]
            elif kind == "normal":
                clamped += c["clamped"]
                assert c["refracted"] >= 100, (name, c)
            else:
                assert c["glass"] >= 100 and c["cannot"] == 0, (name, c)
            ref = orc.render_streaming(flat, scene.camera, w, h, 0, n, mc.CRIT_MB)
            nan = np.isnan(ref["color"]).any(axis=2)
            if c["zero_vector"]:
                # a zero direction misses everything and the sky normalises it: NaN, in some pixels and not in all, so
                # that the NaN-mask comparison is exercised and is not the whole test
                assert 0 < nan.sum() < w * h, (name, int(nan.sum()))
            else:
                assert not nan.any(), name
    print("zero vectors", zero_vector, "k == 0", k_zero, "clamped", clamped)
    for index in (1.5, 0.75, 0.9):
        assert zero_vector[index] >= 100, (index, zero_vector)
    for index in (2.4, 0.9):
        assert k_zero[index] >= 100, (index, k_zero)
    assert clamped >= 100


@pytest.mark.parametrize("name", ["wall", "wall_lit", "wall_meshes", "wall_mesh_first", "three_balls"])
def test_census_of_the_walls(pkg, orc, name):
    """Every material is hit at bounce 0 by at least 30 paths; on the walls at least a quarter of the hits of a metal with
    fuzz >= 1 have their direction rejected and at least 200 paths of a frame hit the object they just left again at
    t < 1e-3.  (three_balls.json has one metal sphere of fuzz exactly 1: a sixth of its directions are rejected, which is
    what a unit sphere of fuzz 1 gives, and its frame is small; for it the two counts only have to be there.)"""
    scene, flat = _walls(pkg)[name]
    w, h = scene.resolution
    with np.errstate(all="ignore"):
        frames = mc.wall_census(orc, lr, flat, scene.camera, w, h, mc.WALL_ITERS)
    for c in frames:
        print(name, "least hits", int(c["per_material"].min()), "fuzz >= 1", c["wide"], "rejected", c["rejected"],
              "hit again", c["rehit"], c["rehit_types"])
    total = sum(c["per_material"] for c in frames)
    assert total.min() >= 30, (name, total)
    for c in frames:
        if name == "three_balls":
            assert c["rejected"] > 0 and c["rehit"] > 0, c
        else:
            assert 4 * c["rejected"] >= c["wide"] > 1000, c
            assert c["rehit"] >= 200, c


def _probe_errors(pkg, orc):
    """(name, max_bounces, prediction, max |oracle - float64| over the compared paths) for every probe frame, by the
    streaming loop and by the megakernel's (other draws: other scattered directions from the same hits)."""
    if "probes" not in _cache:
        out = []
        for name, scene in mc.probe_frames(pkg):
            flat = scene.build_scene()
            for mb in (1, 2):
                p = f64.predict(orc, lr, flat, scene.camera, mc.PROBE_W, mc.PROBE_H, mb)
                frame = orc.render_streaming(flat, scene.camera, mc.PROBE_W, mc.PROBE_H, 0, 1, mb)
                out.append((name, mb, p, f64.worst_error(frame["color"], p)))
                p = f64.predict(orc, lr, flat, scene.camera, mc.PROBE_W, mc.PROBE_H, mb, megakernel=True)
                frame = orc.render_megakernel(flat, scene.camera, mc.PROBE_W, mc.PROBE_H, 0, 1, mb)
                out.append((name + " (megakernel)", mb, p, f64.worst_error(frame["color"], p)))
        _cache["probes"] = out
    return _cache["probes"]


def test_float64_reference_against_the_oracle(pkg, orc):
    for name, mb, p, err in _probe_errors(pkg, orc):
        kept = int(p["compared"].sum())
        print(f"{name} mb {mb}: hits {p['hits']} compared {kept}/{p['paths']} margin-excluded {p['margin_excluded']} "
              f"outside {p['out_of_domain']} max error {err:.3e}")
    for name, mb, p, err in _probe_errors(pkg, orc):
        kept = int(p["compared"].sum())
        assert p["hits"] >= p["paths"] // 2, (name, "the object fills less than half of the frame")
        assert p["margin_excluded"] <= f64.MAX_MARGIN_EXCLUSIONS * p["paths"], (name, mb, p["margin_excluded"])
        least = f64.MIN_DOMAIN_INSIDE if name.startswith("inside") else f64.MIN_DOMAIN
        assert kept >= least * p["paths"], (name, mb, kept)
        assert err <= f64.TOLERANCE, (name, mb, err)


def test_measured_maximum_is_the_constant(pkg, orc):
    """The tolerance of the GPU test is TOLERANCE_FACTOR x the oracle's own worst distance from the float64 reference;
    that distance is re-derived here and must not exceed the constant written down in material_f64.py."""
    worst = max(err for _, _, _, err in _probe_errors(pkg, orc))
    print(f"measured max |oracle - float64| = {worst!r}")
    assert worst <= f64.MEASURED_MAX_ORACLE_ERROR
    assert worst < 1e-4, "more than rounding"
    assert f64.TOLERANCE == f64.TOLERANCE_FACTOR * f64.MEASURED_MAX_ORACLE_ERROR and f64.TOLERANCE_FACTOR == 4.0
