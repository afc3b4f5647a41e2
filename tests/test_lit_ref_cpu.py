"""tests/loop_ref.py -- the CPU restatement of the render loops, here with emissive materials (tests/lit_ref.py) --
pinned to the oracle where the oracle can speak (scenes without emitters: every bit of colour, normal, depth, live counts and ray totals, streaming, megakernel and
interleaved rows), the emissive rule's own properties where it cannot, and the "emissive" entry of the scene grammar in both
readers (json_parser.py and hip_pt --dump-scene).  Emitters are an extension: the reference has none, so what is checked
here is the rule of include/ptcore.h, not the reference."""
import json
import os
import subprocess

import numpy as np
import pytest

import lit_ref as lr
import loop_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_PT = os.path.join(ROOT, "cuda-path-tracer_amd", "host", "hip_pt")


KEYS = ("color", "normal", "depth")


def _glass_and_mirror(pkg):
    """Glass and fuzz-0 metal in front of a diffuse wall: refraction, total internal reflection, the 1e-5 t_min."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.add_material("wall", pkg.DiffuseMateral((0.7, 0.6, 0.5)))
    s.add_material("glass", pkg.DielectricMaterial(1.5))
    s.add_material("mirror", pkg.MetalMaterial((0.9, 0.9, 0.9), 0.0))
    s.add_object(pkg.Sphere((0, 0, 0), 100.0), glm.translate((0.0, 0.0, -103.0)), "wall")
    s.add_object(pkg.Sphere((0, 0, 0), 0.6), glm.translate((-0.5, 0.0, 0.0)), "glass")
    s.add_object(pkg.Sphere((0, 0, 0), 0.5), glm.translate((0.6, 0.1, -0.5)), "mirror")
    s.camera = pkg.scenes._camera_from_look_at((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), vfov_deg=50.0)
    return s


def _scenes(pkg):
    return {
        "cornell_spheres": (pkg.scenes.cornell_spheres(resolution=(40, 30)), 40, 30),
        "cornell_bunny": (pkg.scenes.cornell_bunny(resolution=(32, 24), n_lat=6, n_lon=12), 32, 24),
        "glass_and_mirror": (_glass_and_mirror(pkg), 36, 28),
    }


def _same(got, want, what):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (what, k, int(np.sum(got[k] != want[k])))
    assert got["rays"] == want["rays"], what
    if "live" in want:
        assert np.array_equal(got["live"], want["live"]), what


@pytest.mark.parametrize("name", ["cornell_spheres", "cornell_bunny", "glass_and_mirror"])
@pytest.mark.parametrize("mb", [1, 2, 6])
def test_restatement_equals_the_oracle_without_emitters(pkg, orc, name, mb):
    scene, w, h = _scenes(pkg)[name]
    flat = scene.build_scene()
    sh = orc.SceneHandle(flat)
    # streaming: three iterations, and two more folded into the first two's frame (the running mean's later steps)
    got = loop_ref.render_streaming(orc, flat, scene.camera, w, h, 0, 3, mb, scene_handle=sh)
    want = orc.render_streaming(flat, scene.camera, w, h, 0, 3, mb, scene_handle=sh)
    _same(got, want, (name, mb, "streaming"))
    got2 = loop_ref.render_streaming(orc, flat, scene.camera, w, h, 3, 2, mb, prev=got, scene_handle=sh)
    want2 = orc.render_streaming(flat, scene.camera, w, h, 3, 2, mb, prev=want, scene_handle=sh)
    _same(got2, want2, (name, mb, "streaming, iterations 3-4"))
    got = loop_ref.render_megakernel(orc, flat, scene.camera, w, h, 0, 3, mb, scene_handle=sh)
    want = orc.render_megakernel(flat, scene.camera, w, h, 0, 3, mb, scene_handle=sh)
    _same(got, want, (name, mb, "megakernel"))
    for rank, world, block in ((0, 2, 8), (1, 2, 8), (2, 3, 4)):
        pixels = lr.interleaved_pixels(w, h, rank, world, block)
        got = loop_ref.render_streaming(orc, flat, scene.camera, w, h, 0, 3, mb, pixels=pixels, slot_offset=rank * w * h, scene_handle=sh)
        want = orc.render_interleaved(flat, scene.camera, w, h, rank, world, block, rank * w * h, 0, 3, mb, scene_handle=sh)
        _same(got, want, (name, mb, "interleaved", rank, world))


def _one_ball(pkg, material, radius=0.5, at=(0.0, 0.0, 0.0), extra=()):
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.add_material("ball", material)
    s.add_object(pkg.Sphere((0, 0, 0), radius), glm.translate(at), "ball")
    for name, m, r, c in extra:
        s.add_material(name, m)
        s.add_object(pkg.Sphere((0, 0, 0), r), glm.translate(c), name)
    s.camera = pkg.scenes._camera_from_look_at((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), vfov_deg=50.0)
    return s


@pytest.mark.parametrize("mode", ["streaming", "megakernel"])
def test_an_emitter_that_fills_the_view_gives_its_emission(pkg, orc, mode):
    e = (0.25, 3.0, 7.5)
    scene = _one_ball(pkg, pkg.EmissiveMaterial(e), radius=50.0)  # the camera sits inside the lamp: every ray hits it
    flat = scene.build_scene()
    render = loop_ref.render_streaming if mode == "streaming" else loop_ref.render_megakernel
    out = render(orc, flat, scene.camera, 24, 16, 0, 3, 6)
    assert np.array_equal(out["color"], np.broadcast_to(np.array(e, dtype=np.float32), (16, 24, 3)))
    assert out["rays"] == 3 * 24 * 16  # every path ends at its first hit
    if mode == "streaming":
        assert out["live"][:, 0].tolist() == [24 * 16] * 3 and not out["live"][:, 1:].any()


def test_an_unreachable_emitter_changes_nothing(pkg, orc):
    base = pkg.scenes.cornell_spheres(resolution=(40, 30))
    lit = pkg.scenes.cornell_spheres(resolution=(40, 30))
    # inside the floor sphere, far below the box: no ray of the scene reaches it
    lit.add_material("buried", pkg.EmissiveMaterial((5.0, 5.0, 5.0)))
    lit.add_object(pkg.Sphere((0, 0, 0), 0.5), pkg.glmlite.translate((0.0, -500.0, 0.0)), "buried")
    fb, fl = base.build_scene(), lit.build_scene()
    for mb in (2, 6):
        want = orc.render_streaming(fb, base.camera, 40, 30, 0, 3, mb)
        got = loop_ref.render_streaming(orc, fl, lit.camera, 40, 30, 0, 3, mb)
        _same(got, want, ("streaming", mb))
        want = orc.render_megakernel(fb, base.camera, 40, 30, 0, 3, mb)
        got = loop_ref.render_megakernel(orc, fl, lit.camera, 40, 30, 0, 3, mb)
        _same(got, want, ("megakernel", mb))


def test_a_black_emitter_ends_the_path(pkg, orc):
    # a black lamp in front of a white wall: its pixels are 0 and their paths end there (fewer rays than a diffuse ball)
    extra = (("wall", pkg.DiffuseMateral((0.9, 0.9, 0.9)), 100.0, (0.0, 0.0, -104.0)),)
    dark = _one_ball(pkg, pkg.EmissiveMaterial((0.0, 0.0, 0.0)), radius=0.8, at=(0.0, 0.0, -2.0), extra=extra)
    grey = _one_ball(pkg, pkg.DiffuseMateral((0.5, 0.5, 0.5)), radius=0.8, at=(0.0, 0.0, -2.0), extra=extra)
    fd, fg = dark.build_scene(), grey.build_scene()
    a = loop_ref.render_streaming(orc, fd, dark.camera, 32, 24, 0, 1, 6)
    b = loop_ref.render_streaming(orc, fg, grey.camera, 32, 24, 0, 1, 6)
    assert np.array_equal(a["depth"], b["depth"])
    on_ball = a["depth"] < 3.0  # the ball's front face lies at t 1.2 ... 2, the wall at 4 and beyond
    assert on_ball.sum() > 20
    assert not a["color"][on_ball].any()
    assert b["color"][on_ball].any()
    assert a["live"][0, 1] == b["live"][0, 1] - int(on_ball.sum())
    assert a["rays"] < b["rays"]
    m = loop_ref.render_megakernel(orc, fd, dark.camera, 32, 24, 0, 1, 6)
    assert not m["color"][on_ball].any()


# ---- the scene grammar: "emissive" with "emission": [r, g, b], both readers ----
LIT_JSON = os.path.join(ROOT, "assets", "scenes", "cornell_lit.json")


def _dump(path, out):
    return subprocess.run([HIP_PT, path, "--dump-scene", out], capture_output=True, text=True)


def _read_dump(path, flat):
    """--dump-scene writes the flat arrays one after another, each as a uint64 count + its bytes (main.cpp dump_vec)."""
    data = open(path, "rb").read()
    at, out = 0, []
    for ref in (flat.objects, flat.object_material_indices, flat.spheres, flat.materials):
        n = int(np.frombuffer(data, dtype=np.uint64, count=1, offset=at)[0])
        at += 8
        size = ref.dtype.itemsize * (ref[0].size if ref.ndim > 1 else 1)
        out.append(np.frombuffer(data, dtype=ref.dtype, count=n * (ref[0].size if ref.ndim > 1 else 1), offset=at))
        at += n * size
    return out


def test_both_readers_agree_on_a_scene_with_an_emitter(pkg, tmp_path):
    scene = pkg.json_parser.scene_from_json(LIT_JSON)
    flat = scene.build_scene()
    types = flat.materials["type"].tolist()
    assert types.count(3) == 1
    lamp = flat.materials[types.index(3)]
    assert lamp["p"].tolist() == [4.0, np.float32(3.6), 3.0, 0.0]
    if not os.path.exists(HIP_PT):
        pytest.fail("hip_pt is not built (build() makes it)")
    r = _dump(LIT_JSON, str(tmp_path / "lit.bin"))
    assert r.returncode == 0, r.stderr
    objects, mat_idx, spheres, materials = _read_dump(str(tmp_path / "lit.bin"), flat)
    assert objects.tobytes() == flat.objects.tobytes()
    assert mat_idx.tobytes() == np.ascontiguousarray(flat.object_material_indices).tobytes()
    assert spheres.tobytes() == np.ascontiguousarray(flat.spheres).tobytes()
    assert materials.tobytes() == flat.materials.tobytes()


@pytest.mark.parametrize("bad", [None, [1.0, 2.0], [1.0, 2.0, 3.0, 4.0], "warm", [1.0, "x", 2.0], [1.0, -0.5, 2.0],
                                 [True, 1.0, 1.0], {"r": 1.0}])
def test_both_readers_reject_a_bad_emission(pkg, tmp_path, bad):
    j = json.load(open(LIT_JSON))
    for m in j["materials"]:
        if m["type"] == "emissive":
            if bad is None:
                del m["emission"]
            else:
                m["emission"] = bad
    path = str(tmp_path / "bad.json")
    json.dump(j, open(path, "w"))
    with pytest.raises(ValueError, match="emission"):
        pkg.json_parser.scene_from_json(path)
    r = _dump(path, str(tmp_path / "bad.bin"))
    assert r.returncode != 0 and "emission" in (r.stderr + r.stdout), (bad, r.returncode, r.stderr)


def test_the_packing_of_an_emissive_material(pkg):
    from importlib import import_module
    sd = import_module(pkg.__name__ + ".scene_description")
    rec = sd.material_record(pkg.EmissiveMaterial((0.5, 1.0, 2.0)))
    assert int(rec["type"]) == 3 and rec["p"].tolist() == [0.5, 1.0, 2.0, 0.0]
