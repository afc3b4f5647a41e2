"""Russian roulette (ptc_set_param "roulette") on the GPU against its CPU restatement (tests/loop_ref.py with roulette >= 1), bit
for bit: colour, first-hit normal and depth, ptc_stats.rays_total and the per-bounce live counts, under the streaming method (every
schedule that ends a bounce differently, interleaved ranks, the stepwise calls, high sample indices) and under the megakernel (plain
and with "direct_light" 1: the three loop counters too).  Then what the rule promises beside the bits: a parameter that lets no
bounce play renders as 0 does, fewer rays, and a paired statistical test of the estimator in both methods."""
import math

import numpy as np
import pytest

import direct_loop_scenes as scenes
import lit_ref as lr
import loop_ref

pytestmark = pytest.mark.gpu

PLANES = ("color", "normal", "depth")
COUNTERS = ("diffuse_hits", "shadow_rays", "unoccluded")
W, H, MB, ITERS = 65, 33, 8, 3  # 2145 slots: five 512-slot tiles, the last one partly filled
_cache = {}


def _lit(pkg):
    if "lit" not in _cache:
        scene = pkg.scenes.cornell_lit(resolution=(W, H), with_mesh=True)
        _cache["lit"] = (scene, scene.build_scene())
    return _cache["lit"]


def _ref_streaming(orc, key, flat, camera, w, h, mb, iters, k, **kw):
    key = ("s", key, w, h, mb, iters, k, tuple(sorted((a, str(b)[:40]) for a, b in kw.items() if a != "pixels")))
    if key not in _cache:
        _cache[key] = loop_ref.render_streaming(orc, flat, camera, w, h, kw.pop("iter_begin", 0), iters, mb, roulette=k, **kw)
    return _cache[key]


def _render(pkg, scene, flat, w, h, mb, iters, k, params=(), variant=None, method=None, direct=False, iter_begin=0, interleave=None,
            stepwise=False):
    lives = []
    with pkg.PathTracer(device=0, max_bounces=mb) as pt:
        for name, v in params:
            pt.set_param(name, v)
        if method is not None:
            pt.current_gpu_method = method
        pt.direct_light = direct
        pt.roulette = k
        pt.create_buffers((w, h), flat)
        if variant is not None:
            pt.set_trace_variant(variant)
        if interleave is not None:
            rank, world, block = interleave
            pt.set_interleave(rank, world, block)
            pt.set_param("slot_offset", rank * w * h)
        pt.restart()
        if iter_begin:
            pt.set_iteration(iter_begin)
        pt.max_iterations = iter_begin + iters
        pt.reset_profile()
        for _ in range(iters):
            if stepwise:
                pt.trace_begin(scene.camera)
                for b in range(mb):
                    pt.trace_bounce(b)
                lives.append([pt.read_live_count(b) for b in range(mb)])
                pt.trace_end()
            else:
                pt.path_trace(scene.camera)
        out = {p: pt.download(p) for p in PLANES}
        st = pt.stats()
        out["rays"], out["last_live"] = st["rays_total"], st["last_live"]
        out["lives"] = lives
        out["persist_launches"] = pt.profile()["persist_launches"]
        out.update(pt.direct_loop_stats())
    return out


def _same(got, ref, what, live=True, counters=()):
    for p in PLANES:
        a = np.ascontiguousarray(got[p]).view(np.uint32)
        b = np.ascontiguousarray(ref[p], dtype=np.float32).reshape(got[p].shape).view(np.uint32)
        assert np.array_equal(a, b), (what, p, int(np.sum(a != b)), np.argwhere(a != b)[:4].tolist())
    assert got["rays"] == ref["rays"], (what, got["rays"], ref["rays"])
    if live:
        want = ref["last_live"] if "last_live" in ref else [int(x) for x in ref["live"][-1]]
        assert got["last_live"][:len(want)] == want, (what, got["last_live"], want)
    for c in counters:
        assert got[c] == ref[c], (what, c, got[c], ref[c])


def _classes(ref):
    """(ended, survived with the division, skipped with q >= 1) of a restatement's run"""
    ended, skipped = int(ref["ended"].sum()), int(ref["skipped"].sum())
    return ended, int(ref["played"].sum()) - ended - skipped, skipped


@pytest.mark.parametrize("k", [1, 3])
def test_streaming_against_the_restatement_and_the_stepwise_calls(pkg, orc, k):
    """Five tiles: the look-back crosses tiles after paths have ended.  ptc_trace (batched) and the stepwise calls, whose live counts
    are read per iteration and bounce (ptc_read_live_count)."""
    scene, flat = _lit(pkg)
    ref = _ref_streaming(orc, "lit", flat, scene.camera, W, H, MB, ITERS, k)
    assert all(n > 0 for n in _classes(ref)), _classes(ref)
    got = _render(pkg, scene, flat, W, H, MB, ITERS, k)
    _same(got, ref, ("ptc_trace", k))
    step = _render(pkg, scene, flat, W, H, MB, ITERS, k, stepwise=True)
    _same(step, ref, ("stepwise", k))
    assert np.array_equal(np.array(step["lives"], dtype=np.uint32), ref["live"]), (step["lives"], ref["live"])
    _same(step, got, ("stepwise against ptc_trace", k))
    plain = _ref_streaming(orc, "lit", flat, scene.camera, W, H, MB, ITERS, 0)
    assert got["rays"] < plain["rays"]
    assert np.array_equal(got["normal"], plain["normal"].reshape(got["normal"].shape))
    assert np.array_equal(got["depth"], plain["depth"].reshape(got["depth"].shape))


SCHEDULES = {
    "variant0_fif1": dict(variant=0, params=(("frames_in_flight", 1),)),
    "variant0_fif3": dict(variant=0, params=(("frames_in_flight", 3),)),
    "variant1_fif1": dict(variant=1, params=(("frames_in_flight", 1),)),
    "variant1_fif3": dict(variant=1, params=(("frames_in_flight", 3),)),
    "variant3_fif1": dict(variant=3, params=(("frames_in_flight", 1),)),
    "variant3_fif3": dict(variant=3, params=(("frames_in_flight", 3),)),
    "ray_sort": dict(params=(("ray_sort", 1),)),
    "ray_sort_batches": dict(params=(("frames_in_flight", 6), ("batch_frames", 3), ("ray_sort", 1))),
    "three_kernels": dict(params=(("fused_shade", 0),)),
    "three_kernels_batches": dict(params=(("frames_in_flight", 6), ("batch_frames", 3), ("fused_shade", 0))),
    "no_prefold": dict(params=(("prefold", 0),)),
    "persist": dict(params=(("persist", 1),)),
    "lds_2": dict(params=(("debug_lds_entries", 2),)),
    "lds_2_batches": dict(params=(("frames_in_flight", 6), ("batch_frames", 3), ("debug_lds_entries", 2))),
}


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_every_schedule_renders_the_default_s_bits(pkg, orc, name):
    """The knobs tests/test_gpu_schedules.py flips, each against the restatement (which the default equals: the test above)."""
    scene, flat = _lit(pkg)
    for k in (1, 3):
        ref = _ref_streaming(orc, "lit", flat, scene.camera, W, H, MB, ITERS, k)
        _same(_render(pkg, scene, flat, W, H, MB, ITERS, k, **SCHEDULES[name]), ref, (name, k))


def _mesh_first(pkg):
    """The persistent launch's shape (tests/test_gpu_emissive.py): one mesh object that opens the list, then spheres."""
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


def test_a_frame_with_a_roulette_bounce_leaves_the_persistent_launch(pkg, orc):
    """k_persist is not taught roulette: "persist" 1 renders such a frame through the per-bounce launches, with the same bits; a
    parameter that lets no bounce play keeps the persistent launch."""
    scene = _mesh_first(pkg)
    flat = scene.build_scene()
    w, h, mb = 64, 48, 6
    params = (("persist", 1), ("frames_in_flight", 12), ("batch_frames", 12))
    ref = _ref_streaming(orc, "mesh_first", flat, scene.camera, w, h, mb, ITERS, 1)
    ended, divided, _ = _classes(ref)  # (no glass here: no path comes in with throughput 1 behind bounce 0)
    assert ended > 0 and divided > 0, _classes(ref)
    on = _render(pkg, scene, flat, w, h, mb, ITERS, 1, params=params)
    assert on["persist_launches"] == 0
    _same(on, ref, "persist 1, roulette 1")
    for k in (0, mb - 1):
        off = _render(pkg, scene, flat, w, h, mb, ITERS, k, params=params)
        assert off["persist_launches"] >= 1, k
        _same(off, _ref_streaming(orc, "mesh_first", flat, scene.camera, w, h, mb, ITERS, 0), ("persist 1, no play", k))


@pytest.mark.parametrize("name", ["metal_glass", "cornell_spheres"])
def test_every_class_of_path(pkg, orc, name):
    """metal_glass_scene: a mesh lamp, metal, glass (throughput 1: q >= 1).  cornell_spheres: no mesh, every hit comes from the sphere
    run that ends the object list (the kFirst instances).  The restatement must show every class, so the test cannot pass vacuously."""
    if name == "metal_glass":
        scene, w, h, iters = scenes.metal_glass_scene(pkg), 48, 32, 3
    else:
        scene, w, h, iters = pkg.scenes.cornell_spheres((96, 96)), 96, 96, 2
    flat = scene.build_scene()
    for k in (1, 2):
        ref = _ref_streaming(orc, name, flat, scene.camera, w, h, MB, iters, k)
        ended, divided, skipped = _classes(ref)
        assert ended > 0 and divided > 0 and skipped > 0, (name, k, ended, divided, skipped)
        _same(_render(pkg, scene, flat, w, h, MB, iters, k), ref, (name, k))
        _same(_render(pkg, scene, flat, w, h, MB, iters, k, params=(("fused_shade", 0),)), ref, (name, k, "three kernels"))
    mk = loop_ref.render_megakernel(orc, flat, scene.camera, w, h, 0, iters, MB, roulette=1)
    assert all(n > 0 for n in _classes(mk)), _classes(mk)
    _same(_render(pkg, scene, flat, w, h, MB, iters, 1, method=pkg.GPUMethod.megakernel), mk, (name, "megakernel"), live=False)


@pytest.mark.parametrize("k", [64, 7])
def test_a_parameter_that_lets_no_bounce_play_renders_as_0(pkg, orc, k):
    scene, flat = _lit(pkg)
    plain = _ref_streaming(orc, "lit", flat, scene.camera, W, H, MB, ITERS, 0)
    if "gpu0" not in _cache:
        _cache["gpu0"] = {m: _render(pkg, scene, flat, W, H, MB, ITERS, 0, method=m) for m in (pkg.GPUMethod.streaming, pkg.GPUMethod.megakernel)}
    zero = _cache["gpu0"]
    _same(zero[pkg.GPUMethod.streaming], plain, "roulette 0 against loop_ref")
    for m in zero:
        _same(_render(pkg, scene, flat, W, H, MB, ITERS, k, method=m), zero[m], (k, m), live=m == pkg.GPUMethod.streaming)
    direct0 = _render(pkg, scene, flat, W, H, MB, ITERS, 0, method=pkg.GPUMethod.megakernel, direct=True)
    _same(_render(pkg, scene, flat, W, H, MB, ITERS, k, method=pkg.GPUMethod.megakernel, direct=True), direct0, (k, "direct"), live=False,
          counters=COUNTERS)


def test_high_sample_indices(pkg, orc):
    """Iterations 2^31 - 6 .. 2^31 - 4: the roulette stream's seed (and the running mean) far into a session."""
    scene = pkg.scenes.cornell_lit(resolution=(32, 24), with_mesh=True)
    flat = scene.build_scene()
    begin = 2 ** 31 - 6
    ref = loop_ref.render_streaming(orc, flat, scene.camera, 32, 24, begin, 3, 6, roulette=1)
    assert all(n > 0 for n in _classes(ref))
    _same(_render(pkg, scene, flat, 32, 24, 6, 3, 1, iter_begin=begin), ref, "2^31 - 6")
    mk = loop_ref.render_megakernel(orc, flat, scene.camera, 32, 24, begin, 3, 6, direct=True, roulette=1)
    _same(_render(pkg, scene, flat, 32, 24, 6, 3, 1, iter_begin=begin, method=pkg.GPUMethod.megakernel, direct=True), mk, "2^31 - 6, direct",
          live=False, counters=COUNTERS)


def test_two_interleaved_ranks(pkg, orc):
    """Set up as tests/test_gpu_interleaved.py: rows dealt in blocks of 8, paths numbered per rank, slot_offset = rank * W * H -- the
    roulette stream is keyed on slot_offset + slot like the material stream."""
    w, h, block, mb = 64, 44, 8, 6  # (the last block has 4 rows)
    scene = pkg.scenes.cornell_lit(resolution=(w, h), with_mesh=True)
    flat = scene.build_scene()
    sh = orc.SceneHandle(flat)
    for rank in (0, 1):
        pixels = lr.interleaved_pixels(w, h, rank, 2, block)
        ref = loop_ref.render_streaming(orc, flat, scene.camera, w, h, 0, ITERS, mb, roulette=1, pixels=pixels, slot_offset=rank * w * h,
                                  scene_handle=sh)
        assert all(n > 0 for n in _classes(ref))
        _same(_render(pkg, scene, flat, w, h, mb, ITERS, 1, interleave=(rank, 2, block)), ref, ("interleaved", rank))


@pytest.mark.parametrize("mb", [2, 8])
@pytest.mark.parametrize("direct", [False, True])
def test_megakernel_against_the_restatement(pkg, orc, mb, direct):
    """Plain and with "direct_light" 1.  At 2 bounces bounce 1 is the last one: nothing plays."""
    scene, flat = _lit(pkg)
    k = 1
    ref = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 0, ITERS, mb, direct=direct, roulette=k)
    got = _render(pkg, scene, flat, W, H, mb, ITERS, k, method=pkg.GPUMethod.megakernel, direct=direct)
    _same(got, ref, ("megakernel", mb, direct), live=False, counters=COUNTERS)
    off = _render(pkg, scene, flat, W, H, mb, ITERS, 0, method=pkg.GPUMethod.megakernel, direct=direct)
    assert np.array_equal(got["normal"], off["normal"]) and np.array_equal(got["depth"], off["depth"])
    if mb == 2:
        assert ref["played"].sum() == 0
        _same(got, off, ("nothing plays", direct), live=False, counters=COUNTERS)
    else:
        assert all(n > 0 for n in _classes(ref)), _classes(ref)
        assert got["rays"] < off["rays"]
        assert not np.array_equal(got["color"], off["color"])
        if direct:
            assert 0 < got["diffuse_hits"] < off["diffuse_hits"]
        else:
            assert (got["diffuse_hits"], got["shadow_rays"], got["unoccluded"]) == (0, 0, 0)


def test_the_forms_of_the_end_of_a_bounce_agree(pkg, orc):
    """64 x 48, 6 bounces, 2 iterations, roulette 1: the fused, three-kernel and persistent forms of the end of a bounce give byte-equal
    colour (and the restatement's), and the megakernel with "direct_light" 1 -- the one loop with its direct part -- the restatement's."""
    w, h, mb, iters, k = 64, 48, 6, 2, 1
    scene = pkg.scenes.cornell_lit(resolution=(w, h), with_mesh=True)
    flat = scene.build_scene()
    ref = loop_ref.render_streaming(orc, flat, scene.camera, w, h, 0, iters, mb, roulette=k)
    assert all(n > 0 for n in _classes(ref)), _classes(ref)
    forms = {name: _render(pkg, scene, flat, w, h, mb, iters, k, params=params)
             for name, params in (("fused", ()), ("three_kernels", (("fused_shade", 0),)), ("persist", (("persist", 1),)))}
    for name, got in forms.items():
        assert got["color"].tobytes() == forms["fused"]["color"].tobytes(), name
        _same(got, ref, name)
    mk = loop_ref.render_megakernel(orc, flat, scene.camera, w, h, 0, iters, mb, direct=True, roulette=k)
    _same(_render(pkg, scene, flat, w, h, mb, iters, k, method=pkg.GPUMethod.megakernel, direct=True), mk, "megakernel, direct", live=False,
          counters=COUNTERS)


def test_the_refusals(pkg):
    scene, flat = _lit(pkg)
    invalid = pkg._capi.PTC_ERR_INVALID
    with pkg.PathTracer(max_bounces=4) as pt:
        pt.create_buffers((W, H), flat)
        for bad in (-1, 65):
            with pytest.raises(pkg.PtcError) as e:
                pt.set_param("roulette", bad)
            assert e.value.code == invalid and "roulette must be in [0,64]" in str(e.value), str(e.value)
        pt.set_param("roulette", 64)  # settable at any time, after ptc_resize too
        pt.roulette = 1
        pt.max_iterations = 2
        pt.path_trace(scene.camera)
        # direct lighting under the streaming method stays refused, roulette or not
        pt.direct_light = True
        with pytest.raises(pkg.PtcError) as e:
            pt.path_trace(scene.camera)
        assert e.value.code == invalid and "megakernel" in str(e.value)
        assert pt.iteration() == 1


STAT_K, STAT_BLOCKS, STAT_PER_BLOCK = 2, 16, 256


def stat_blocks(pkg, method, w=32, h=24):
    """Per mode (roulette 0, STAT_K) and block b the image mean per channel of iterations [256 b, 256 (b + 1)) and the rays traced.
    Each block starts from framebuffers that ptc_resize has cleared, at iteration 256 b: the running mean then holds (sum of the
    block's samples) / (256 (b + 1)), so the block's own mean is that times (b + 1)  (tests/test_gpu_direct_loop.py)."""
    scene = scenes.small_lamp_room(pkg)
    flat = scene.build_scene()
    means = np.zeros((2, STAT_BLOCKS, 3))
    rays = [0, 0]
    tracers = []
    try:
        for mode in (0, 1):
            pt = pkg.PathTracer(device=0, max_bounces=scenes.STAT_BOUNCES)
            tracers.append(pt)
            pt.current_gpu_method = method
            if method == pkg.GPUMethod.streaming:  # (few launches: 32 iterations per batch)
                pt.set_param("frames_in_flight", 64)
                pt.set_param("batch_frames", 32)
            pt.roulette = STAT_K if mode else 0
            pt.create_buffers((w, h), flat)
        for b in range(STAT_BLOCKS):
            for mode, pt in enumerate(tracers):
                pt.resize_image((w, h))
                pt.restart()
                pt.set_iteration(STAT_PER_BLOCK * b)
                pt.max_iterations = STAT_PER_BLOCK * (b + 1)
                for _ in range(STAT_PER_BLOCK):
                    pt.path_trace(scene.camera)
                means[mode, b] = pt.download("color").astype(np.float64).reshape(-1, 3).mean(axis=0) * (b + 1)
                rays[mode] += pt.stats()["rays_total"]
    finally:
        for pt in tracers:
            pt.close()
    return means, rays


@pytest.mark.parametrize("method", ["streaming", "megakernel"])
def test_same_expectation_fewer_rays(pkg, method):
    """Paired over 16 blocks of 256 iterations (fixed seeds: deterministic) in the closed 12-triangle room at 24 bounces, roulette 2
    against 0.  D_b = image mean of block b with roulette minus without.  |mean(D)| <= 4.073 sd(D) / sqrt(16) per channel (the two-sided
    0.1 % point of Student's t, 15 degrees of freedom; the constant and form of tests/test_gpu_direct_loop.py), and the roulette run
    traces fewer rays.  No assertion on the spread: roulette may raise it (the figures are printed)."""
    means, rays = stat_blocks(pkg, getattr(pkg.GPUMethod, method))
    d = means[1] - means[0]
    print(f"{method}: rays {rays[0]} -> {rays[1]} ({rays[1] / rays[0]:.3f})")
    for c in range(3):
        mean_d, sd_d = d[:, c].mean(), d[:, c].std(ddof=1)
        sd0, sd1 = means[0, :, c].std(ddof=1), means[1, :, c].std(ddof=1)
        print(f"channel {c}: mean0 {means[0, :, c].mean():.6f} mean1 {means[1, :, c].mean():.6f} mean(D) {mean_d:+.3e} "
              f"bound {4.073 * sd_d / 4.0:.3e} sd0 {sd0:.3e} sd1 {sd1:.3e} variance ratio (1 / 0) {(sd1 / sd0) ** 2:.2f}")
    for c in range(3):
        mean_d, sd_d = d[:, c].mean(), d[:, c].std(ddof=1)
        assert abs(mean_d) <= 4.073 * sd_d / math.sqrt(16.0), (method, c, mean_d, sd_d)
    assert rays[1] < rays[0], rays
