"""Direct lighting in the megakernel without a GPU: the binding, and the CPU restatement
(loop_ref.render_megakernel with direct=True) against the same loop without the option for everything but the colour, on the
no-lamp and glass-fronted-lamp scenes for the emission gate, and against direct_ref's sample for the light stream at bounce 0."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import direct_loop_scenes as scenes
import direct_ref as dr
import loop_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


W, H = 16, 12
_cache = {}


def _both(orc, key, scene, mb, iters=2):
    if (key, mb) not in _cache:
        flat = scene.build_scene()
        sh = orc.SceneHandle(flat)
        record = []
        lit = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 0, iters, mb, direct=True, scene_handle=sh, record=record)
        plain = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 0, iters, mb, scene_handle=sh)
        _cache[(key, mb)] = (flat, lit, plain, record)
    return _cache[(key, mb)]


def test_binding(pkg):
    lib = pkg.lib()
    assert hasattr(lib, "ptc_get_direct_loop_stats")
    capi = pkg._capi
    assert [f[0] for f in capi.ptc_direct_loop_stats._fields_] == ["diffuse_hits", "shadow_rays", "unoccluded"]
    assert C.sizeof(capi.ptc_direct_loop_stats) == 24
    assert "ptc_get_direct_loop_stats" in capi.SIGNATURES
    assert lib.ptc_abi_version() == 3
    # the Python mirror: direct_light is the switch (assigned) and still the query (called); no context is made here (no GPU)
    assert isinstance(pkg.PathTracer.direct_light, property) and pkg.PathTracer.direct_light.fset is not None
    assert callable(pkg.PathTracer.direct_loop_stats)
    exe = os.path.join(ROOT, "cuda-path-tracer_amd", "host", "hip_pt")
    for extra in ([], ["--method", "streaming"]):
        run = subprocess.run([exe, "--direct-light", *extra, "-o", "unused.png", "scenes/cornell_lit.json"], cwd=ROOT,
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert run.returncode == 1, (extra, run.returncode, run.stderr)
        assert "--direct-light needs --method megakernel" in run.stderr, run.stderr
    usage = subprocess.run([exe, "--help"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert "--direct-light" in usage.stderr


@pytest.mark.parametrize("mb", [1, 2, 5])
def test_restatement_moves_only_the_colour(pkg, orc, mb):
    scene = pkg.scenes.cornell_lit(resolution=(W, H), with_mesh=True)
    _, lit, plain, _ = _both(orc, "cornell_lit", scene, mb)
    assert np.array_equal(lit["normal"], plain["normal"])
    assert np.array_equal(lit["depth"], plain["depth"])
    assert lit["rays"] == plain["rays"]
    assert not np.array_equal(lit["color"], plain["color"])
    assert lit["diffuse_hits"] >= lit["shadow_rays"] >= lit["unoccluded"] > 0


def test_a_scene_without_lamps_is_untouched(pkg, orc):
    scene = pkg.scenes.cornell_spheres((W, H))
    _, lit, plain, record = _both(orc, "no_lamps", scene, 5)
    for k in ("color", "normal", "depth"):
        assert np.array_equal(lit[k], plain[k]), k
    assert lit["rays"] == plain["rays"]
    assert (lit["diffuse_hits"], lit["shadow_rays"], lit["unoccluded"]) == (0, 0, 0) and not record


def test_a_lamp_behind_glass_keeps_its_emission(pkg, orc):
    """Every shadow ray is blocked by the glass, and the lamp is only ever hit after a dielectric vertex or from the camera: the
    gate must let every such hit count, so the colour is the plain render's (radiance stays 0; 0 + colour == colour)."""
    scene = scenes.glass_lamp_scene(pkg)
    _, lit, plain, _ = _both(orc, "glass_lamp", scene, 5)
    assert lit["shadow_rays"] > 0 and lit["unoccluded"] == 0
    seen = plain["color"].max(axis=-1) > 1.0
    assert seen.sum() >= 4, "the lamp is seen (directly through the glass)"
    assert np.array_equal(lit["color"][seen], plain["color"][seen])
    assert np.array_equal(lit["color"], plain["color"])


def test_bounce_0_is_the_query_sample(pkg, orc):
    """The light sample at bounce 0 of pixel i == direct_ref's sample for point index i at sample_index = iteration, on the
    restatement's own first-hit points (points without a diffuse first hit get a dummy and are left out of the comparison)."""
    scene = pkg.scenes.cornell_lit(resolution=(W, H), with_mesh=True)
    flat, _, _, record = _both(orc, "cornell_lit", scene, 2)
    table = dr.light_table(flat)
    first = [r for r in record if r["kind"] == "light" and r["bounce"] == 0]
    assert len(first) == 2
    for r in first:
        pts = np.zeros((W * H, 3), dtype=np.float32)
        nrm = np.tile(np.array([0.0, 1.0, 0.0], dtype=np.float32), (W * H, 1))
        pts[r["pixels"]], nrm[r["pixels"]] = r["points"], r["normals"]
        want = dr.sample(orc, flat, pts, nrm, r["iteration"], table=table)
        assert len(r["pixels"]) > W * H // 2
        assert np.array_equal(want["rays"][r["pixels"]], r["sample"]["rays"])
        assert np.array_equal(want["contribution"][r["pixels"]], r["sample"]["contribution"])
        assert np.array_equal(want["sampled"][r["pixels"]], r["sample"]["sampled"])
        assert r["sample"]["sampled"].any() and not r["sample"]["sampled"].all()
