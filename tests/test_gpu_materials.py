"""The material kernels (evaluate_material and its re-organised form shade_kinds: k_shade_fused, k_shade, k_megakernel,
k_persist) over their parameter range and at their edges, against the checkers that tests/test_material_cases_cpu.py has
checked: the oracle's bits (lit_ref's for the wall with emitters) on the walls of tests/material_cases.py -- 60 material
records in one scene, albedo 0 ... 1e12, fuzz 0 ... 4, refraction index 1e-3 ... 1e3, so that every wavefront mixes kinds and
parameters -- on the reference's three_balls scene and on frames whose rays meet glass within ulps of the critical angle
(refracted direction (0, 0, 0), k == 0, the clamp), through every way to reach the material code; and the float64 reference
of tests/material_f64.py on the probe frames, within the tolerance measured on the CPU.

NaN: the 1e12 albedos overflow to inf and a rejected metal direction then gives inf * 0; a zero direction gives 0 / 0 in the
sky.  The checker has them too; x86 and gfx950 differ in a NaN's sign bit, so where the checker has NaN the frame must have
NaN and everywhere else the same value (material_cases.mismatches)."""
import numpy as np
import pytest

import lit_ref as lr
import loop_ref
import material_cases as mc
import material_f64 as f64

pytestmark = pytest.mark.gpu

ITERS = mc.WALL_ITERS
# (label, parameters, trace variant)
SCHEDULES = [("default", (), None), ("fused_shade 0", (("fused_shade", 0),), None), ("prefold 0", (("prefold", 0),), None),
             ("sphere_lanes 0, sphere_fold 0", (("sphere_lanes", 0), ("sphere_fold", 0)), None),
             ("4 in flight, batches of 2", (("frames_in_flight", 4), ("batch_frames", 2)), None),
             ("variant 0", (), 0), ("variant 1", (), 1)]
_cache = {}


def _wall(pkg, name):
    if name not in _cache:
        scene = mc.walls(pkg)[name]
        _cache[name] = (scene, scene.build_scene())
    return _cache[name]


def _render(pkg, flat, camera, w, h, iters, mb, params=(), variant=None, method=None, interleave=None):
    with pkg.PathTracer(device=0, max_bounces=mb) as pt:
        for k, v in params:
            pt.set_param(k, v)
        if variant is not None:
            pt.set_trace_variant(variant)
        if method is not None:
            pt.current_gpu_method = method
        pt.create_buffers((w, h), flat)
        if interleave is not None:
            rank, world, block = interleave
            pt.set_interleave(rank, world, block)
            pt.set_param("slot_offset", rank * w * h)
        pt.max_iterations = iters
        pt.reset_profile()
        for _ in range(iters):
            pt.path_trace(camera)
        out = {k: pt.download(k) for k in ("color", "normal", "depth")}
        st = pt.stats()
        out["rays"], out["last_live"] = st["rays_total"], st["last_live"]
        out["persist_launches"] = pt.profile()["persist_launches"]
    return out


def _same(got, ref, what, live=True):
    for k in ("color", "normal", "depth"):
        bad = mc.mismatches(got[k], ref[k])
        assert bad == 0, (what, k, bad)
    assert got["rays"] == ref["rays"], (what, got["rays"], ref["rays"])
    if live:
        want = [int(x) for x in ref["live"][-1]]
        assert got["last_live"][:len(want)] == want, (what, got["last_live"], want)


def _huge_pixels(orc, scene, flat):
    """Pixels whose first hit (iteration 0) is an object with the 1e12 albedo."""
    w, h = scene.resolution
    mats = np.asarray(flat.materials)
    sh = orc.SceneHandle(flat)
    o, d, tmin, st, recs, hit = mc._first_hits(orc, lr, flat, scene.camera, w, h, 0, sh)
    mid = recs["material_id"].astype(np.int64) % len(mats)
    return int(np.sum(hit & (mats["type"][mid] <= 1) & (mats["p"][mid, 0] == np.float32(1e12))))


@pytest.mark.parametrize("mb", [1, 2, 8])
@pytest.mark.parametrize("name", ["wall", "wall_lit", "wall_meshes", "wall_mesh_first", "three_balls"])
def test_walls_through_every_way_to_the_material_code(pkg, orc, name, mb):
    scene, flat = _wall(pkg, name)
    w, h = scene.resolution
    sh = orc.SceneHandle(flat)
    lit = name == "wall_lit"
    with np.errstate(all="ignore"):
        if lit:   # the oracle has no emitters: tests/lit_ref.py is the checker (pinned to the oracle on the other walls)
            ref = loop_ref.render_streaming(orc, flat, scene.camera, w, h, 0, ITERS, mb, scene_handle=sh)
            mk = loop_ref.render_megakernel(orc, flat, scene.camera, w, h, 0, ITERS, mb, scene_handle=sh)
            rank = loop_ref.render_streaming(orc, flat, scene.camera, w, h, 0, ITERS, mb, scene_handle=sh,
                                       pixels=lr.interleaved_pixels(w, h, 1, 2, 8), slot_offset=w * h)
        else:
            ref = orc.render_streaming(flat, scene.camera, w, h, 0, ITERS, mb, scene_handle=sh)
            mk = orc.render_megakernel(flat, scene.camera, w, h, 0, ITERS, mb, scene_handle=sh)
            rank = orc.render_interleaved(flat, scene.camera, w, h, 1, 2, 8, w * h, 0, ITERS, mb, scene_handle=sh)
    if name != "three_balls":
        nan = int(np.isnan(ref["color"]).any(axis=2).sum())
        huge = _huge_pixels(orc, scene, flat)
        print(name, mb, "NaN pixels", nan, "pixels of the 1e12 objects", huge)
        assert huge > 1000 and nan < 0.05 * huge, (nan, huge)
    for label, params, variant in SCHEDULES:
        _same(_render(pkg, flat, scene.camera, w, h, ITERS, mb, params=params, variant=variant), ref, (name, mb, label))
    _same(_render(pkg, flat, scene.camera, w, h, ITERS, mb, method=pkg.GPUMethod.megakernel), mk, (name, mb, "megakernel"),
          live=False)
    # rank 1 of 2: its slots are numbered from slot_offset on, so a slot index that is not the pixel's own keys the draws
    _same(_render(pkg, flat, scene.camera, w, h, ITERS, mb, interleave=(1, 2, 8)), rank, (name, mb, "rank 1 of 2"))
    if name == "wall_mesh_first":
        got = _render(pkg, flat, scene.camera, w, h, ITERS, mb,
                      params=(("persist", 1), ("frames_in_flight", 12), ("batch_frames", 12)))
        if mb >= 2:   # (one bounce: there is no bounce >= 1 for the persistent launch to span)
            assert got["persist_launches"] > 0, "the batch did not take the persistent launch"
        _same(got, ref, (name, mb, "persist"))


def test_wall_with_records_out_of_range(pkg, orc):
    """Refraction index 0 and a NaN albedo (material_cases.wall_out_of_range): not refused by ptc_upload_scene; the kernels
    give NaN where the oracle does and the oracle's values everywhere else.  Nothing in the material code branches on a
    colour, and the directions these records make (the zero vector, NaN) take the degenerate-direction paths that the
    critical-angle frames below exercise."""
    scene, flat = mc.wall_out_of_range(pkg)
    w, h = scene.resolution
    ref = orc.render_streaming(flat, scene.camera, w, h, 0, ITERS, 8)
    mk = orc.render_megakernel(flat, scene.camera, w, h, 0, ITERS, 8)
    assert 100 < np.isnan(ref["color"]).any(axis=2).sum() < 0.05 * w * h
    for label, params, variant in SCHEDULES[:4]:
        _same(_render(pkg, flat, scene.camera, w, h, ITERS, 8, params=params, variant=variant), ref, label)
    _same(_render(pkg, flat, scene.camera, w, h, ITERS, 8, method=pkg.GPUMethod.megakernel), mk, "megakernel", live=False)


def test_critical_angle_frames(pkg, orc):
    """Zero-vector refractions, k == 0, grazing and normal incidence: default schedule, the plain evaluate_material of
    k_shade, and the megakernel; the census of these frames is asserted in tests/test_material_cases_cpu.py."""
    w, h, n, mb = mc.CRIT_W, mc.CRIT_H, mc.CRIT_ITERS, mc.CRIT_MB
    with_nan = 0
    for name, kind, index, scene in mc.critical_frames(pkg):
        flat = scene.build_scene()
        sh = orc.SceneHandle(flat)
        ref = orc.render_streaming(flat, scene.camera, w, h, 0, n, mb, scene_handle=sh)
        mk = orc.render_megakernel(flat, scene.camera, w, h, 0, n, mb, scene_handle=sh)
        with_nan += bool(np.isnan(ref["color"]).any())
        _same(_render(pkg, flat, scene.camera, w, h, n, mb), ref, (name, "default"))
        _same(_render(pkg, flat, scene.camera, w, h, n, mb, params=(("fused_shade", 0),)), ref, (name, "fused_shade 0"))
        _same(_render(pkg, flat, scene.camera, w, h, n, mb, method=pkg.GPUMethod.megakernel), mk, (name, "megakernel"),
              live=False)
    assert with_nan >= 20, with_nan   # the frames of index 1.5, 0.75, 0.9 and the inside-sphere ones


def test_probe_frames_against_the_float64_reference(pkg, orc):
    """The GPU's colour against the float64 prediction, within TOLERANCE (4 x the oracle's own measured distance), on the
    paths the CPU test compares: the excluded set comes from the oracle's inputs, never from the GPU's result."""
    worst = 0.0
    for name, scene in mc.probe_frames(pkg):
        flat = scene.build_scene()
        for mb in (1, 2):
            streaming = f64.predict(orc, lr, flat, scene.camera, mc.PROBE_W, mc.PROBE_H, mb)
            mega = f64.predict(orc, lr, flat, scene.camera, mc.PROBE_W, mc.PROBE_H, mb, megakernel=True)
            for label, params, method in (("default", (), None), ("fused_shade 0", (("fused_shade", 0),), None),
                                          ("megakernel", (), pkg.GPUMethod.megakernel)):
                got = _render(pkg, flat, scene.camera, mc.PROBE_W, mc.PROBE_H, 1, mb, params=params, method=method)
                p = mega if method is not None else streaming
                err = f64.worst_error(got["color"], p)
                print(f"{name} mb {mb} {label}: compared {int(p['compared'].sum())}/{p['paths']} max error {err:.3e}")
                worst = max(worst, err)
                assert err <= f64.TOLERANCE, (name, mb, label, err)
    print("worst", worst, "tolerance", f64.TOLERANCE)


def test_wall_at_full_size(pkg, orc):
    """The wall at 1920 x 1080, 8 bounces, 2 iterations (about 30 M rays), default schedule, against the oracle."""
    w, h, mb = 1920, 1080, 8
    scene = mc.wall(pkg, size=(w, h))
    flat = scene.build_scene()
    ref = orc.render_streaming(flat, scene.camera, w, h, 0, ITERS, mb)
    _same(_render(pkg, flat, scene.camera, w, h, ITERS, mb), ref, "1920 x 1080")
