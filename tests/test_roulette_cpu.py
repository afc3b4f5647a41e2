"""Russian roulette (ptc_set_param "roulette") without a GPU: the binding and hip_pt's argument handling, and the
CPU restatement (loop_ref's loops with roulette >= 1) against the same loops without the option wherever no bounce plays, and the
properties the rule promises where one does.  The bits of either are pinned by tests/test_loop_ref_golden_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

import loop_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


W, H, ITERS, MB = 16, 12, 2, 6
PLANES = ("color", "normal", "depth")
_cache = {}


def _scene(pkg, orc):
    if "scene" not in _cache:
        scene = pkg.scenes.cornell_lit(resolution=(W, H), with_mesh=True)
        flat = scene.build_scene()
        _cache["scene"] = (scene, flat, orc.SceneHandle(flat))
    return _cache["scene"]


def _streaming(pkg, orc, k, record=None):
    scene, flat, sh = _scene(pkg, orc)
    if record is not None:
        return loop_ref.render_streaming(orc, flat, scene.camera, W, H, 0, ITERS, MB, roulette=k, scene_handle=sh, record=record)
    if ("s", k) not in _cache:
        _cache[("s", k)] = loop_ref.render_streaming(orc, flat, scene.camera, W, H, 0, ITERS, MB, roulette=k, scene_handle=sh)
    return _cache[("s", k)]


def test_binding_and_hip_pt_arguments(pkg):
    lib = pkg.lib()
    assert lib.ptc_abi_version() == 3  # no struct and no entry point was added
    # the Python mirror: a property with a checked setter; no context is made here (no GPU)
    prop = pkg.PathTracer.roulette
    assert isinstance(prop, property) and prop.fset is not None
    blank = pkg.PathTracer.__new__(pkg.PathTracer)
    for k in (0, 1, 64):
        prop.fset(blank, k)
        assert prop.fget(blank) == k
    for bad in (-1, 65):
        with pytest.raises(ValueError) as e:
            prop.fset(blank, bad)
        assert "roulette must be in [0,64]" in str(e.value)
    with open(os.path.join(ROOT, "include", "ptcore.h")) as f:
        assert '"roulette"' in f.read()
    exe = os.path.join(ROOT, "cuda-path-tracer_amd", "host", "hip_pt")
    usage = subprocess.run([exe, "--help"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert usage.returncode == 0 and "--roulette K" in usage.stderr
    for bad in ("65", "-1", "x", "3x", "", "1e1", "100"):
        run = subprocess.run([exe, "--roulette", bad, "-o", "unused.png", "scenes/cornell_lit.json"], cwd=ROOT, stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True)
        assert run.returncode == 1, (bad, run.returncode, run.stderr)
        assert "--roulette" in run.stderr and "[0,64]" in run.stderr, (bad, run.stderr)
    missing = subprocess.run([exe, "--roulette"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert missing.returncode == 1 and "missing an argument" in missing.stderr
    # a value in range passes the argument parsing: the scene is read and dumped, no GPU needed
    ok = subprocess.run([exe, "--roulette", "64", "--dump-scene", os.devnull, "scenes/cornell_lit.json"], cwd=ROOT, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True)
    assert ok.returncode == 0, ok.stderr


@pytest.mark.parametrize("k", [0, MB - 1, MB, 64])
def test_no_bounce_plays_streaming(pkg, orc, k):
    scene, flat, sh = _scene(pkg, orc)
    if "plain_s" not in _cache:
        _cache["plain_s"] = loop_ref.render_streaming(orc, flat, scene.camera, W, H, 0, ITERS, MB, scene_handle=sh)
    plain, got = _cache["plain_s"], _streaming(pkg, orc, k)
    for p in PLANES:
        assert np.array_equal(got[p].view(np.uint32), plain[p].view(np.uint32)), p
    assert got["rays"] == plain["rays"] and np.array_equal(got["live"], plain["live"])
    assert got["played"].sum() == 0


@pytest.mark.parametrize("k", [0, MB - 1, 64])
@pytest.mark.parametrize("direct", [False, True])
def test_no_bounce_plays_megakernel(pkg, orc, k, direct):
    scene, flat, sh = _scene(pkg, orc)
    key = ("plain_m", direct)
    if key not in _cache:
        _cache[key] = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 0, ITERS, MB, direct=direct, scene_handle=sh)
    plain = _cache[key]
    got = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 0, ITERS, MB, direct=direct, roulette=k, scene_handle=sh)
    for p in PLANES:
        assert np.array_equal(got[p].view(np.uint32), plain[p].view(np.uint32)), p
    assert got["rays"] == plain["rays"] and got["played"].sum() == 0
    if direct:
        for c in ("diffuse_hits", "shadow_rays", "unoccluded"):
            assert got[c] == plain[c], c


def test_k_1_streaming(pkg, orc):
    """Bounce 0 never plays: normal, depth and the live counts up to bounce k are the plain render's; later counts are not larger;
    every survivor that was divided has a largest component of exactly 1."""
    k = 1
    record = []
    got = _streaming(pkg, orc, k, record=record)
    plain = _streaming(pkg, orc, 0)
    assert np.array_equal(got["normal"], plain["normal"]) and np.array_equal(got["depth"], plain["depth"])
    assert np.array_equal(got["live"][:, :k + 1], plain["live"][:, :k + 1])
    assert (got["live"][:, k + 1:] <= plain["live"][:, k + 1:]).all() and got["live"].sum() < plain["live"].sum()
    assert got["rays"] < plain["rays"] and got["rays"] == int(got["live"].sum())
    assert not np.array_equal(got["color"], plain["color"])
    assert got["played"][:, 0].sum() == 0 and got["played"][:, MB - 1].sum() == 0  # bounce 0 and the last bounce never play
    assert got["ended"].sum() > 0 and (got["played"] - got["ended"] - got["skipped"]).sum() > 0
    assert np.array_equal(got["played"][:, 1:MB - 1] - got["ended"][:, 1:MB - 1], got["live"][:, 2:MB])  # who plays and stays is live
    divided = np.concatenate([r["after"] for r in record])
    assert len(divided) > 0 and np.array_equal(divided.max(axis=1), np.ones(len(divided), dtype=np.float32))
    for r in record:
        assert 1 <= r["bounce"] < MB - 1
        assert not (r["skipped"] & r["ended"]).any()


def test_k_1_megakernel(pkg, orc):
    scene, flat, sh = _scene(pkg, orc)
    for direct in (False, True):
        plain = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 0, ITERS, MB, direct=direct, scene_handle=sh)
        record = []
        got = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 0, ITERS, MB, direct=direct, roulette=1, scene_handle=sh, record=record)
        record = [r for r in record if r["kind"] == "roulette"]
        assert np.array_equal(got["normal"], plain["normal"]) and np.array_equal(got["depth"], plain["depth"])
        assert got["rays"] < plain["rays"] and not np.array_equal(got["color"], plain["color"])
        assert got["ended"].sum() > 0
        divided = np.concatenate([r["after"] for r in record])
        assert len(divided) > 0 and (divided.max(axis=1) == np.float32(1.0)).all()
        if direct:
            assert 0 < got["diffuse_hits"] < plain["diffuse_hits"]


def test_a_black_wall_ends_every_path_that_leaves_it(pkg, orc):
    """A floor of albedo (0, 0, 0): a path that leaves it carries throughput 0, so q == 0 and !(u < 0) at its next play."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.add_material("black", pkg.DiffuseMateral((0.0, 0.0, 0.0)))
    s.add_material("white", pkg.DiffuseMateral((0.8, 0.8, 0.8)))
    s.add_object(pkg.Sphere((0, 0, 0), 1000.0), glm.translate((0.0, -1001.0, 0.0)), "black")
    s.add_object(pkg.Sphere((0, 0, 0), 0.9), glm.translate((0.0, -0.1, -1.0)), "white")
    s.camera = pkg.scenes._camera_from_look_at((0.0, 0.6, 3.0), (0.0, -0.3, -1.0), vfov_deg=50.0)
    flat = s.build_scene()
    record = []
    got = loop_ref.render_streaming(orc, flat, s.camera, W, H, 0, ITERS, MB, roulette=1, record=record)
    zero = sum(int((r["q"] == 0).sum()) for r in record)
    assert zero > 0
    for r in record:
        assert r["ended"][r["q"] == 0].all()
    # ... so no path with throughput 0 is ever shaded twice: every path alive behind a play has a positive throughput
    plain = loop_ref.render_streaming(orc, flat, s.camera, W, H, 0, ITERS, MB)
    assert got["rays"] < plain["rays"]
    # the image is the plain one wherever no divided path arrives: a dead path deposits 0 either way (0 * sky == 0)
    assert np.isfinite(got["color"]).all()
