"""Emissive materials (ptc_material type 3, an extension: the reference has no emitters) on the GPU against tests/loop_ref.py,
bit for bit: colour, first-hit normal and depth, ray totals and the live counts of the last frame.  A path whose closest hit
is an emitter ends there with colour * emission and no draw, and leaves the stable partition like a miss -- so every later
survivor's slot, and with it its random numbers, moves.  The scenes put the emitter in each place a closest hit can come
from: the sphere run that ends the object list (k_shade_fused's tail), a mesh (the traversal kernels), the sphere run in
front of the first mesh (k_spheres / "prefold") and a run between two meshes; the schedules cover every form of the kernel
that ends a bounce (fused and three-kernel, prefold, the persistent launch, the megakernel, interleaved ranks)."""
import os
import subprocess

import numpy as np
import pytest

import lit_ref as lr
import loop_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, ITERS = 64, 48, 3
KNOBS = [(("fused_shade", 0),), (("prefold", 0),), (("sphere_fold", 0),), (("sphere_lanes", 0),), (("filter_rays", 0),),
         (("beam", 0),), (("merge_instances", 0),), (("frames_in_flight", 1),), (("frames_in_flight", 4), ("batch_frames", 2)),
         (("ray_sort", 1),), (("pair_batches", 1), ("frames_in_flight", 4), ("batch_frames", 2))]


_cache = {}


def _reference(orc, key, flat, camera, mb, method="streaming"):
    k = (key, mb, method)
    if k not in _cache:
        if method == "streaming":
            _cache[k] = loop_ref.render_streaming(orc, flat, camera, W, H, 0, ITERS, mb)
        else:
            _cache[k] = loop_ref.render_megakernel(orc, flat, camera, W, H, 0, ITERS, mb)
    return _cache[k]


def _render(pkg, scene, flat, mb, params=(), method=None, interleave=None):
    with pkg.PathTracer(device=0, max_bounces=mb) as pt:
        for k, v in params:
            pt.set_param(k, v)
        if method is not None:
            pt.current_gpu_method = method
        pt.create_buffers((W, H), flat)
        if interleave is not None:
            rank, world, block = interleave
            pt.set_interleave(rank, world, block)
            pt.set_param("slot_offset", rank * W * H)
        pt.max_iterations = ITERS
        pt.reset_profile()
        for _ in range(ITERS):
            pt.path_trace(scene.camera)
        out = {k: pt.download(k) for k in ("color", "normal", "depth")}
        st = pt.stats()
        out["rays"], out["last_live"] = st["rays_total"], st["last_live"]
        out["persist_launches"] = pt.profile()["persist_launches"]
    return out


def _same(got, ref, what, live=True):
    for k in ("color", "normal", "depth"):
        want = ref[k].reshape(got[k].shape)
        assert np.array_equal(got[k], want), (what, k, int(np.sum(got[k] != want)))
    assert got["rays"] == ref["rays"], (what, got["rays"], ref["rays"])
    if live:
        want = [int(x) for x in ref["live"][-1]]
        assert got["last_live"][:len(want)] == want, (what, got["last_live"], want)


def _lit(pkg, kind):
    if kind == "sphere_light":
        return pkg.scenes.cornell_lit(resolution=(W, H))
    return pkg.scenes.cornell_lit(resolution=(W, H), with_mesh=True)


@pytest.mark.parametrize("kind", ["sphere_light", "mesh_light"])
@pytest.mark.parametrize("mb", [1, 2, 6])
def test_cornell_lit_every_schedule(pkg, orc, kind, mb):
    scene = _lit(pkg, kind)
    flat = scene.build_scene()
    ref = _reference(orc, kind, flat, scene.camera, mb)
    assert (ref["color"] > 1.0).any(), "the lamps are seen"
    _same(_render(pkg, scene, flat, mb), ref, "default")
    for params in (KNOBS if mb == 6 else KNOBS[:1]):
        _same(_render(pkg, scene, flat, mb, params=params), ref, params)
    mk = _reference(orc, kind, flat, scene.camera, mb, method="megakernel")
    _same(_render(pkg, scene, flat, mb, method=pkg.GPUMethod.megakernel), mk, "megakernel", live=False)


def _mesh_first(pkg):
    """The persistent launch's shape: one mesh object that opens the list (a lamp panel over a floor), then spheres -- a
    diffuse ball and a sphere lamp in the run that ends the list."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.add_material("panel", pkg.EmissiveMaterial((3.0, 3.0, 3.0)))
    s.add_material("floor", pkg.DiffuseMateral((0.7, 0.7, 0.7)))
    s.add_material("lamp", pkg.EmissiveMaterial((0.5, 2.0, 1.0)))
    s.add_material("mirror", pkg.MetalMaterial((0.9, 0.9, 0.9), 0.0))
    s.add_object(s.add_mesh("panel", pkg.scenes.light_panel_mesh(-1.0, 1.0, -2.0, 0.0, 1.0)), glm.identity(), "panel")
    s.add_object(pkg.Sphere((0, 0, 0), 100.0), glm.translate((0.0, -101.0, 0.0)), "floor")
    s.add_object(pkg.Sphere((0, 0, 0), 0.4), glm.translate((0.5, -0.6, -1.0)), "mirror")
    s.add_object(pkg.Sphere((0, 0, 0), 0.3), glm.translate((-0.6, -0.7, -0.8)), "lamp")
    s.camera = pkg.scenes._camera_from_look_at((0.0, 0.2, 3.0), (0.0, -0.2, -1.0), vfov_deg=55.0)
    return s


@pytest.mark.parametrize("mb", [2, 6])
def test_persistent_launch_with_emitters(pkg, orc, mb):
    scene = _mesh_first(pkg)
    flat = scene.build_scene()
    ref = _reference(orc, "mesh_first", flat, scene.camera, mb)
    on = _render(pkg, scene, flat, mb, params=(("persist", 1), ("frames_in_flight", 12), ("batch_frames", 12)))
    assert on["persist_launches"] >= 1, "the batch did not take the persistent launch"
    _same(on, ref, "persist")
    _same(_render(pkg, scene, flat, mb), ref, "default")


def test_interleaved_ranks_with_emitters(pkg, orc):
    scene = _lit(pkg, "mesh_light")
    flat = scene.build_scene()
    sh = orc.SceneHandle(flat)
    for rank in (0, 1):
        pixels = lr.interleaved_pixels(W, H, rank, 2, 8)
        ref = loop_ref.render_streaming(orc, flat, scene.camera, W, H, 0, ITERS, 6, pixels=pixels, slot_offset=rank * W * H,
                                  scene_handle=sh)
        got = _render(pkg, scene, flat, 6, interleave=(rank, 2, 8))
        _same(got, ref, ("interleaved", rank))


def _random_lit(pkg, seed):
    """An object list drawn at random (the shape of test_gpu_random_scenes.py) with one or two emissive materials."""
    rng = np.random.default_rng(5000 + seed)
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    mats = [("white", pkg.DiffuseMateral((0.8, 0.8, 0.8))), ("steel", pkg.MetalMaterial((0.8, 0.8, 0.9), 0.2)),
            ("mirror", pkg.MetalMaterial((0.9, 0.9, 0.9), 0.0)), ("glass", pkg.DielectricMaterial(1.5)),
            ("lamp", pkg.EmissiveMaterial((4.0, 3.0, 2.0))), ("lamp2", pkg.EmissiveMaterial((0.3, 1.5, 6.0)))]
    for name, m in mats:
        s.add_material(name, m)
    meshes = [pkg.scenes.displaced_sphere_mesh(10, 20), pkg.scenes.heightfield_mesh(17, 9, 2.0, 1.0, seed=3 + seed)]
    for k, m in enumerate(meshes):
        s.add_mesh(f"m{k}", m)

    def vec(lo, hi):
        return tuple(float(v) for v in rng.uniform(lo, hi, 3).astype(np.float32))

    n = int(rng.integers(3, 8))
    kinds = []
    for i in range(n):
        mat = mats[int(rng.integers(0, len(mats)))][0]
        if rng.random() < 0.5:
            r = float(np.float32(rng.choice([0.15, 0.4, 0.8])))
            s.add_object(pkg.Sphere((0.0, 0.0, 0.0), r), glm.translate(vec(-1.2, 1.2)), mat)
            kinds.append("s")
        else:
            k = int(rng.integers(0, 2))
            s.add_object(meshes[k], glm.compose([glm.scale(float(rng.uniform(0.3, 0.9))), glm.translate(vec(-1.0, 1.0))]), mat)
            kinds.append("ab"[k])
        kinds[-1] += "*" if mat.startswith("lamp") else ""
    if seed % 3 == 0:  # a small lamp at the end of the list: the sphere run that ends it
        s.add_object(pkg.Sphere((0.0, 0.0, 0.0), 0.3), glm.translate(vec(-1.0, 1.0)), "lamp2")
        kinds.append("s*")
    eye = vec(-0.6, 0.6)
    s.camera = pkg.Camera(position=(eye[0], eye[1] + 0.3, 3.2), rotation=(1.0, 0.0, 0.0, 0.0), vfov=float(np.radians(55.0)))
    return s, " ".join(kinds)


def _where(kinds):
    """Where the scene's emitters sit in the object list: 'leading' (a sphere run in front of the first mesh), 'mesh',
    'between' (a sphere run between two meshes), 'trailing' (the run that ends the list)."""
    objs = kinds.split()
    mesh_at = [i for i, o in enumerate(objs) if o[0] in "ab"]
    out = set()
    for i, o in enumerate(objs):
        if not o.endswith("*"):
            continue
        if o[0] in "ab":
            out.add("mesh")
        elif not mesh_at or i > mesh_at[-1]:
            out.add("trailing")
        elif i < mesh_at[0]:
            out.add("leading")
        else:
            out.add("between")
    return out


SEEDS = [0, 1, 2, 3, 5, 6, 7, 9, 12, 13]


def test_random_seeds_cover_every_place_of_an_emitter(pkg):
    places = set()
    for seed in SEEDS:
        places |= _where(_random_lit(pkg, seed)[1])
    assert places == {"leading", "mesh", "between", "trailing"}, places


@pytest.mark.parametrize("seed", SEEDS)
def test_random_object_lists_with_emitters(pkg, orc, seed):
    scene, kinds = _random_lit(pkg, seed)
    flat = scene.build_scene(distinct_meshes=True)
    assert 3 in flat.materials["type"].tolist()
    ref = loop_ref.render_streaming(orc, flat, scene.camera, W, H, 0, ITERS, 6)
    for params in ((), KNOBS[seed % len(KNOBS)]):
        _same(_render(pkg, scene, flat, 6, params=params), ref, (seed, kinds, params))


@pytest.mark.parametrize("bad", [(float("nan"), 1.0, 1.0, 0.0), (1.0, float("inf"), 1.0, 0.0), (1.0, 1.0, -0.5, 0.0),
                                 (1.0, 1.0, 1.0, 0.5)])
def test_upload_rejects_a_bad_emissive_material(pkg, bad):
    scene = pkg.scenes.cornell_lit(resolution=(16, 16))
    flat = scene.build_scene()
    at = flat.materials["type"].tolist().index(3)
    flat.materials["p"][at] = bad
    with pkg.PathTracer(device=0, max_bounces=2) as pt:
        with pytest.raises(pkg.PtcError) as e:
            pt.create_buffers((16, 16), flat)
        assert f"material {at}" in str(e.value), str(e.value)


def test_upload_rejects_unknown_material_types(pkg):
    scene = pkg.scenes.cornell_lit(resolution=(16, 16))
    flat = scene.build_scene()
    for t in (4, -1):
        flat.materials["type"][0] = t
        with pkg.PathTracer(device=0, max_bounces=2) as pt:
            with pytest.raises(pkg.PtcError):
                pt.create_buffers((16, 16), flat)


def test_hip_pt_renders_the_lit_scene_file(pkg, orc, tmp_path):
    """hip_pt on assets/scenes/cornell_lit.json: its PNG is the tonemapped restatement within one step of 8 bits."""
    from PIL import Image
    path = os.path.join(ROOT, "assets", "scenes", "cornell_lit.json")
    exe = os.path.join(ROOT, "cuda-path-tracer_amd", "host", "hip_pt")
    out = str(tmp_path / "lit.png")
    r = subprocess.run([exe, path, "-o", out, "--spp", "2", "--max-bounces", "6"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.array(Image.open(out)).astype(np.int32)
    scene = pkg.json_parser.scene_from_json(path)
    w, h = scene.resolution
    ref = loop_ref.render_streaming(orc, scene.build_scene(), scene.camera, w, h, 0, 2, 6)
    want = orc.preview(ref["color"], w, h, 0).astype(np.int32)
    assert got.shape == want.shape
    assert (ref["color"] > 1.0).any()
    assert np.abs(got - want).max() <= 1
