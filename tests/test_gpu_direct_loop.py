"""Direct lighting in the megakernel (ptc_set_param "direct_light" 1) on the GPU against its CPU restatement
(tests/loop_ref.py, render_megakernel with direct=True), bit for bit: colour, first-hit normal and depth, ptc_stats.rays_total and the three loop counters
(diffuse hits, shadow rays traced, unoccluded).  Then what the rule promises beside the bits: normal / depth / rays_total equal to
the plain megakernel's, a lamp-less scene untouched, interleaved ranks assembling to the one-context frame, the refusals, and a
paired statistical test of the estimator (same expectation as the plain render, lower spread)."""
import math

import numpy as np
import pytest

import direct_loop_scenes as scenes
import direct_ref as D
import loop_ref

pytestmark = pytest.mark.gpu

PLANES = ("color", "normal", "depth")
COUNTERS = ("diffuse_hits", "shadow_rays", "unoccluded")


def _render(pkg, scene, flat, w, h, mb, iters, direct, iter_begin=0, interleave=None):
    with pkg.PathTracer(device=0, max_bounces=mb) as pt:
        pt.current_gpu_method = pkg.GPUMethod.megakernel
        pt.direct_light = direct
        pt.create_buffers((w, h), flat)  # (ptc_resize clears the framebuffers and the counters)
        if interleave is not None:
            pt.set_interleave(*interleave)
        pt.restart()
        if iter_begin:
            pt.set_iteration(iter_begin)
        pt.max_iterations = iter_begin + iters
        for _ in range(iters):
            pt.path_trace(scene.camera)
        out = {k: pt.download(k) for k in PLANES}
        out["rays"] = pt.stats()["rays_total"]
        out.update(pt.direct_loop_stats())
    return out


def _same(got, ref, what, planes=PLANES, counters=COUNTERS):
    for k in planes:
        a = np.ascontiguousarray(got[k]).view(np.uint32)
        b = np.ascontiguousarray(ref[k], dtype=np.float32).reshape(got[k].shape).view(np.uint32)
        assert np.array_equal(a, b), (what, k, int(np.sum(a != b)), np.argwhere(a != b)[:4].tolist())
    assert got["rays"] == ref["rays"], (what, got["rays"], ref["rays"])
    for k in counters:
        assert got[k] == ref[k], (what, k, got[k], ref[k])


def _against_restatement(pkg, orc, scene, w, h, mb, iters, what, iter_begin=0):
    flat = scene.build_scene()
    ref = loop_ref.render_megakernel(orc, flat, scene.camera, w, h, iter_begin, iters, mb, direct=True)
    got = _render(pkg, scene, flat, w, h, mb, iters, True, iter_begin)
    _same(got, ref, what)
    return flat, got, ref


@pytest.mark.parametrize("mb", [1, 2, 8])
def test_cornell_lit_against_the_restatement(pkg, orc, mb):
    """A sphere lamp and a mesh panel; bounce 1 = a light sample and then the cap.  The same run with direct_light 0: the geometry."""
    w, h = 64, 48
    scene = pkg.scenes.cornell_lit(resolution=(w, h), with_mesh=True)
    flat, got, ref = _against_restatement(pkg, orc, scene, w, h, mb, 3, ("cornell_lit", mb))
    assert ref["diffuse_hits"] > ref["shadow_rays"] > ref["unoccluded"] > 0
    plain = _render(pkg, scene, flat, w, h, mb, 3, False)
    _same(got, plain, ("against direct_light 0", mb), planes=("normal", "depth"), counters=())
    assert not np.array_equal(got["color"], plain["color"])
    assert (plain["diffuse_hits"], plain["shadow_rays"], plain["unoccluded"]) == (0, 0, 0)


def test_a_frame_that_is_no_multiple_of_a_wavefront(pkg, orc):
    scene = pkg.scenes.cornell_lit(resolution=(65, 33), with_mesh=True)
    _against_restatement(pkg, orc, scene, 65, 33, 4, 2, "65 x 33")


def test_high_sample_indices(pkg, orc):
    """Iterations 2^31 - 6 .. 2^31 - 4: the light stream's seed (and the running mean) far into a session."""
    scene = pkg.scenes.cornell_lit(resolution=(32, 24), with_mesh=True)
    _against_restatement(pkg, orc, scene, 32, 24, 4, 3, "2^31 - 6", iter_begin=2 ** 31 - 6)


def _floor_and_camera(pkg, scene, add_floor):
    if add_floor:
        scene.add_material("floor_", pkg.DiffuseMateral((0.6, 0.6, 0.6)))
        scene.add_object(pkg.Sphere((0, 0, 0), 1000.0), pkg.glmlite.translate((0.0, -1001.0, 0.0)), "floor_")
    scene.camera = pkg.scenes._camera_from_look_at((0.0, 0.3, 3.5), (0.0, 0.0, -0.5), vfov_deg=50.0)
    return scene


SCENES = {
    "two_instances": lambda pkg: D.two_instance_scene(pkg),
    "dark_lamps": lambda pkg: D.dark_lamp_scene(pkg),
    "area_0_triangles": lambda pkg: _floor_and_camera(pkg, D.degenerate_scene(pkg), True),
    "big_emitter": lambda pkg: _floor_and_camera(pkg, D.big_emitter_scene(pkg), False),  # 16,384 triangles: the cdf search runs 14 steps
    "metal_and_glass": lambda pkg: scenes.metal_glass_scene(pkg),
    "lamp_behind_glass": lambda pkg: scenes.glass_lamp_scene(pkg),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_lamp_scenes_against_the_restatement(pkg, orc, name):
    scene = SCENES[name](pkg)
    _, got, ref = _against_restatement(pkg, orc, scene, 48, 36, 5, 2, name)
    assert ref["shadow_rays"] > 0, name
    if name == "lamp_behind_glass":
        assert ref["unoccluded"] == 0
    else:
        assert ref["unoccluded"] > 0, name


def test_a_scene_without_lamps_renders_as_without_the_parameter(pkg):
    scene = pkg.scenes.cornell_spheres((64, 48))
    flat = scene.build_scene()
    on, off = (_render(pkg, scene, flat, 64, 48, 6, 3, direct) for direct in (True, False))
    _same(on, off, "no lamps")
    assert (on["diffuse_hits"], on["shadow_rays"], on["unoccluded"]) == (0, 0, 0)


def test_two_interleaved_ranks_assemble_to_the_one_context_frame(pkg):
    """The megakernel seeds by frame pixel (material stream and light stream): contexts one after another, rows dealt in blocks."""
    w, h, block = 64, 44, 8  # (the last block has 4 rows)
    scene = pkg.scenes.cornell_lit(resolution=(w, h), with_mesh=True)
    flat = scene.build_scene()
    whole = _render(pkg, scene, flat, w, h, 5, 3, True)
    parts = [_render(pkg, scene, flat, w, h, 5, 3, True, interleave=(rank, 2, block)) for rank in (0, 1)]
    for k in PLANES:
        frame = pkg.bands.assemble_interleaved([p[k] for p in parts], h, 2, block)
        assert np.array_equal(frame.view(np.uint32), whole[k].view(np.uint32)), k
    for k in ("rays",) + COUNTERS:
        assert parts[0][k] + parts[1][k] == whole[k], k


def test_refusals(pkg):
    scene = pkg.scenes.cornell_lit(resolution=(48, 32), with_mesh=True)
    flat = scene.build_scene()
    invalid = pkg._capi.PTC_ERR_INVALID
    # the streaming method: refused before anything is queued, the accumulation untouched
    with pkg.PathTracer(max_bounces=4) as pt:
        pt.create_buffers((48, 32), flat)
        pt.max_iterations = 8
        for _ in range(2):
            pt.path_trace(scene.camera)
        before = {k: pt.download(k) for k in PLANES}
        rays = pt.stats()["rays_total"]
        pt.direct_light = True
        for call in (pt.path_trace, pt.trace_begin):
            with pytest.raises(pkg.PtcError) as e:
                call(scene.camera)
            assert e.value.code == invalid and "megakernel" in str(e.value), str(e.value)
        assert pt.iteration() == 2 and pt.stats()["rays_total"] == rays
        for k in PLANES:
            assert np.array_equal(pt.download(k), before[k]), k
        with pytest.raises(pkg.PtcError) as e:
            pt.set_param("direct_light", 2)
        assert e.value.code == invalid and "direct_light must be 0 or 1" in str(e.value)
        with pytest.raises(pkg.PtcError):
            pt.set_param("direct_light", -1)
        pt.direct_light = False
        pt.path_trace(scene.camera)  # and the context goes on
        assert pt.iteration() == 3
    # a sphere lamp under a non-similarity cannot be sampled: the object is named, as by ptc_direct_light
    glm = pkg.glmlite
    bad = pkg.scenes.cornell_spheres((48, 32))
    bad.add_material("lamp", pkg.EmissiveMaterial((4.0, 3.0, 2.0)))
    bad.add_object(pkg.Sphere((0, 0, 0), 1.0), glm.compose([glm.scale((0.45, 0.3, 0.4)), glm.translate((0.3, 0.9, -0.5))]), "lamp")
    with pkg.PathTracer(max_bounces=4) as pt:
        pt.current_gpu_method = pkg.GPUMethod.megakernel
        pt.create_buffers((48, 32), bad.build_scene())
        pt.direct_light = True
        with pytest.raises(pkg.PtcError) as e:
            pt.path_trace(bad.camera)
        assert e.value.code == invalid and "object 7" in str(e.value), str(e.value)
        assert pt.iteration() == 0
        pt.direct_light = False
        pt.path_trace(bad.camera)
        assert pt.iteration() == 1


def test_denoise_and_present_after_direct_lit_iterations(pkg):
    """A smoke test: no parity claim."""
    scene = pkg.scenes.cornell_lit(resolution=(64, 48), with_mesh=True)
    with pkg.PathTracer(max_bounces=6) as pt:
        pt.current_gpu_method = pkg.GPUMethod.megakernel
        pt.direct_light = True
        pt.create_buffers((64, 48), scene.build_scene())
        pt.max_iterations = 4
        for _ in range(4):
            pt.path_trace(scene.camera)
        pt.denoise()
        rgba = pt.send_to_preview()
        assert rgba.shape == (48, 64, 4) and rgba.dtype == np.uint8 and rgba[..., :3].max() > 0
        assert np.isfinite(pt.download("final")).all() and np.isfinite(pt.download("color")).all()
        assert pt.direct_loop_stats()["unoccluded"] > 0
        # the Python field is still the query when called
        assert bool(pt.direct_light) is True
        radiance = pt.direct_light(np.array([[0.2, -1.0, 0.1]], dtype=np.float32), np.array([[0.0, 1.0, 0.0]], dtype=np.float32), 3)
        assert radiance.shape == (1, 3) and np.isfinite(radiance).all()


def stat_blocks(pkg, blocks=16, per_block=256, w=32, h=24, room=None):
    """Per mode (direct_light 0, 1) and block b the image mean per channel of iterations [per_block b, per_block (b + 1)), and
    whether normal and depth agreed.  Each block starts from framebuffers that ptc_resize has cleared, at iteration per_block * b:
    the running mean then holds (sum of the block's samples) / (per_block (b + 1)), so the block's own mean is that times (b + 1)."""
    scene = (room or scenes.small_lamp_room)(pkg)
    flat = scene.build_scene()
    means = np.zeros((2, blocks, 3))
    geometry = []
    tracers = []
    try:
        for mode in (0, 1):
            pt = pkg.PathTracer(device=0, max_bounces=scenes.STAT_BOUNCES)
            tracers.append(pt)
            pt.current_gpu_method = pkg.GPUMethod.megakernel
            pt.direct_light = bool(mode)
            pt.create_buffers((w, h), flat)
        for b in range(blocks):
            planes = []
            for mode, pt in enumerate(tracers):
                pt.resize_image((w, h))
                pt.restart()
                pt.set_iteration(per_block * b)
                pt.max_iterations = per_block * (b + 1)
                for _ in range(per_block):
                    pt.path_trace(scene.camera)
                means[mode, b] = pt.download("color").astype(np.float64).reshape(-1, 3).mean(axis=0) * (b + 1)
                planes.append((pt.download("normal"), pt.download("depth")))
            geometry.append(np.array_equal(planes[0][0], planes[1][0]) and np.array_equal(planes[0][1], planes[1][1]))
    finally:
        for pt in tracers:
            pt.close()
    return means, geometry


def test_same_expectation_lower_spread(pkg):
    """Paired over B = 16 blocks of 256 iterations (fixed seeds: deterministic).  D_b = image mean of block b with direct light
    minus without.  |mean(D)| <= 4.073 sd(D) / sqrt(16) per channel (the two-sided 0.1 % point of Student's t, 15 degrees of
    freedom), and the spread of the direct-lit block means is below the plain ones'.
    The room's walls are triangles (direct_loop_scenes.small_lamp_room says why).  The same room from the stock scenes' radius-1000 wall
    spheres MISSES the first bound -- mean(D) -1.885e-3 / -1.596e-3 / -1.173e-3 against bounds 1.844e-3 / 1.661e-3 / 1.372e-3 (r, g,
    b; image mean 0.21, variance ratios 3.1 / 2.5 / 2.9) -- because 7 % of its shadow rays, carrying 6 % of the unshadowed direct light, hit the wall they start
    on: section 5f's shadow epsilon (origin at the hit point, t_min 1e-4) is too small for a sphere of radius 1000 in binary32.  A
    finding about that epsilon, recorded in DESIGN section 5g; the estimator is tested where the epsilon holds."""
    means, geometry = stat_blocks(pkg)
    assert all(geometry), "normal and depth differ between the modes"
    d = means[1] - means[0]
    for c in range(3):
        mean_d, sd_d = d[:, c].mean(), d[:, c].std(ddof=1)
        sd0, sd1 = means[0, :, c].std(ddof=1), means[1, :, c].std(ddof=1)
        print(f"channel {c}: mean0 {means[0, :, c].mean():.6f} mean1 {means[1, :, c].mean():.6f} mean(D) {mean_d:+.3e} "
              f"bound {4.073 * sd_d / 4.0:.3e} sd0 {sd0:.3e} sd1 {sd1:.3e} variance ratio {(sd0 / sd1) ** 2:.1f}")
    for c in range(3):
        mean_d, sd_d = d[:, c].mean(), d[:, c].std(ddof=1)
        assert abs(mean_d) <= 4.073 * sd_d / math.sqrt(16.0), (c, mean_d, sd_d)
        assert means[1, :, c].std(ddof=1) < means[0, :, c].std(ddof=1), c
