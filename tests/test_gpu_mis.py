"""Multiple importance sampling in the megakernel on the GPU (ptc_set_param "mis", ptc_environment_light_pdf): the
density kernel and the megakernel's multiple-importance instance against the numpy restatement tests/mis_ref.py, bit for bit; what the
parameter must leave alone; the cases in which it must change nothing; the estimator's expectation against the render without it."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import direct_loop_scenes
import direct_ref
import env_light_ref
import loop_ref
import mis_ref

pytestmark = pytest.mark.gpu

PLANES = ("color", "normal", "depth")
SIX = ("diffuse_hits", "shadow_rays", "unoccluded", "env_diffuse_hits", "env_shadow_rays", "env_unoccluded")
MIS = ("mis_emitter_hits", "mis_misses")
EVERYTHING = PLANES + ("rays",) + SIX + MIS
W, H, ITERS = 33, 17, 2
LENS = (0.25, 3.5)
T_BOUND = 4.073  # the two-sided 0.1 % point of Student's t, 15 degrees of freedom (test_gpu_direct_loop.test_same_expectation_lower_spread)
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sun_map(n, seed=5, sky=1.0, sun=400.0, at=None):
    """a random sky (no two texels alike) with a two-texel sun: in the upper hemisphere, or at texel `at` = (j, i) and its neighbour"""
    m = np.random.default_rng(seed).uniform(0.05, sky, (n, n, 3)).astype(np.float32)
    j, i = at or ((2 * n) // 5, n // 2)
    m[j, i] = m[j, min(i + 1, n - 1)] = (sun, 0.9 * sun, 0.8 * sun)
    return m


ENV = sun_map(7)
SIDE = sun_map(7, seed=6, at=(3, 5))  # the sun low in +x: it shines through the opening of the lit_open room


def _table(pkg, env):
    key = ("table", id(env))
    if key not in _cache:
        _cache[key] = (env_light_ref.table_of(pkg, env)[0], env)  # (env kept: its id stays its own)
    return _cache[key][0]


def _scene(pkg, name):
    """name -> (scene, flat), built once.  room: direct_loop_scenes' closed lamp-lit room.  open: a height field under the sky, no lamp.
    lit_open: cornell_lit (a sphere lamp, a mesh panel lamp, three balls) with the right wall taken out.  glass_lamp, metal_glass:
    direct_loop_scenes'.  dark_lamps: direct_ref's, with an emissive material of luminance 0."""
    if name not in _cache:
        if name == "room":
            scene = direct_loop_scenes.small_lamp_room(pkg)
        elif name == "open":
            scene = pkg.scenes.heightfield_scene(resolution=(W, H), nx=17, nz=9)
        elif name == "glass_lamp":
            scene = direct_loop_scenes.glass_lamp_scene(pkg)
        elif name == "metal_glass":
            scene = direct_loop_scenes.metal_glass_scene(pkg)
        elif name == "dark_lamps":
            scene = direct_ref.dark_lamp_scene(pkg)
        else:
            scene = pkg.scenes.cornell_lit(resolution=(W, H), with_mesh=True)
            at = scene.objects_material_mapping_.index("right")
            del scene.objects_[at], scene.objects_material_mapping_[at]
            scene.camera = pkg.scenes._camera_from_look_at((-1.2, 0.0, 4.0), (0.6, -0.1, 0.0), vfov_deg=50.0)
        _cache[name] = (scene, scene.build_scene())
    return _cache[name]


def _tracer(pkg, flat, w=W, h=H, mb=8, mega=True, mis=True, env_light=False, direct=False, roulette=0, lens=None, interleave=None):
    pt = pkg.PathTracer(device=0, max_bounces=mb)
    if mega:
        pt.current_gpu_method = pkg.GPUMethod.megakernel
    pt.mis = mis
    pt.environment_light = env_light
    pt.direct_light = direct
    pt.roulette = roulette
    if lens is not None:
        pt.lens = lens
    pt.create_buffers((w, h), flat)
    if interleave is not None:
        rank, world, block = interleave
        pt.set_interleave(rank, world, block)
    return pt


def _result(pt):
    out = {p: pt.download(p) for p in PLANES}
    out["rays"] = pt.stats()["rays_total"]
    out.update(pt.direct_loop_stats())
    out.update({"env_" + k: v for k, v in pt.environment_light_loop_stats().items()})
    st = pt.mis_loop_stats()
    out.update({"mis_emitter_hits": st["weighted_emitter_hits"], "mis_misses": st["weighted_misses"]})
    return out


def _run(pt, camera, env, iters=ITERS, iter_begin=0):
    pt.environment = env
    pt.restart()
    if iter_begin:
        pt.set_iteration(iter_begin)
    pt.max_iterations = iter_begin + iters
    rays0 = pt.stats()["rays_total"]
    for _ in range(iters):
        pt.path_trace(camera)
    out = _result(pt)
    out["rays"] -= rays0
    return out


def _same(got, ref, keys, what):
    for k in keys:
        if k in PLANES:
            a, b = _bits(got[k]), _bits(np.asarray(ref[k], dtype=np.float32).reshape(got[k].shape))
            assert np.array_equal(a, b), (what, k, int(np.sum(a != b)), np.argwhere(a != b)[:4].tolist())
        else:
            assert got[k] == ref[k], (what, k, got[k], ref[k])


def _against_the_loop(pkg, orc, scene_name, w=W, h=H, mb=8, env=None, iters=ITERS, iter_begin=0, env_light=False, direct=False, roulette=0,
                      lens=None):
    scene, flat = _scene(pkg, scene_name)
    entries = _table(pkg, env) if env is not None else None
    ref = loop_ref.render_megakernel(orc, flat, scene.camera, w, h, iter_begin, iters, mb, env=env, entries=entries, env_light=env_light,
                                    direct=direct, mis=True, roulette=roulette, lens=lens)
    with _tracer(pkg, flat, w, h, mb, env_light=env_light, direct=direct, roulette=roulette, lens=lens) as pt:
        got = _run(pt, scene.camera, env, iters, iter_begin)
    _same(got, ref, EVERYTHING, (scene_name, w, h, mb, env_light, direct, roulette, lens, iter_begin))
    return got


# ---- 1. the density ---------------------------------------------------------------------------------------------------------------------
def _directions(count, seed):
    d = np.random.default_rng(seed).standard_normal((count, 3))
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
    d[:6] = np.concatenate([np.eye(3), -np.eye(3)])
    d[6] = (0.0, 0.0, 0.0)
    d[7] = (np.nan, 0.5, 0.5)
    return d


@pytest.mark.parametrize("n_map", [2, 5, 64])
def test_density_against_the_restatement(pkg, n_map):
    """4099 directions (no multiple of 64 or 256), the axes, a zero and a NaN direction among them; host pointers and device pointers"""
    torch = pytest.importorskip("torch")
    scene, flat = _scene(pkg, "open")
    env = sun_map(n_map, seed=n_map)
    dirs = _directions(4099, 20 + n_map)
    want = mis_ref.pdf(env_light_ref.table_of(pkg, env)[0], n_map, dirs)
    with _tracer(pkg, flat, mega=False, mis=False) as pt:
        pt.environment = env
        before = (pt.stats(), pt.direct_stats(), pt.environment_light_stats())
        got = pt.environment_light_pdf(dirs)
        assert (pt.stats(), pt.direct_stats(), pt.environment_light_stats()) == before  # it moves no statistics
        d_dirs = torch.from_numpy(dirs).cuda()
        d_out = torch.full((4099,), -1.0, dtype=torch.float32, device="cuda")
        pt.environment_light_pdf_dev(d_dirs.data_ptr(), 4099, d_out.data_ptr())
        on_device = d_out.cpu().numpy()
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (n_map, int(bad.sum()), np.nonzero(bad)[0][:4].tolist())
    assert np.array_equal(_bits(on_device), _bits(want))
    assert got[6] == 0.0 and got[7] == 0.0 and (got > 0.0).sum() > 4000


def test_density_on_a_map_of_1024(pkg):
    """entry indices near the end of a 2^20-entry table: a 1024 x 1024 map whose weight sits in its last 40 rows"""
    scene, flat = _scene(pkg, "open")
    n = 1024
    env = np.full((n, n, 3), 1e-3, dtype=np.float32)
    env[n - 40:, :, :] = np.random.default_rng(3).uniform(1.0, 2.0, (40, n, 3)).astype(np.float32)
    entries = env_light_ref.table_of(pkg, env)[0]
    rng = np.random.default_rng(4)
    k = 4099  # unit directions of points in the last 40 rows of the square, and some anywhere
    sx, sz = rng.uniform(0, 1, k).astype(np.float32), rng.uniform((n - 40) / n, 1, k).astype(np.float32)
    sz[::8] = rng.uniform(0, 1, len(sz[::8])).astype(np.float32)
    dirs, _ = env_light_ref.decode(sx, sz)
    ok, qx, qz = mis_ref.project(dirs)
    assert (mis_ref.square_of(qx, qz, n) >= 2 ** 20 - 40 * 1024).sum() > 3000
    want = mis_ref.pdf(entries, n, dirs)
    with _tracer(pkg, flat, mega=False, mis=False) as pt:
        pt.environment = env
        got = pt.environment_light_pdf(dirs)
    assert np.array_equal(_bits(got), _bits(want))
    assert got.max() > 100.0 * got.min() > 0.0


def test_density_refusals_and_a_map_of_zeros(pkg):
    scene, flat = _scene(pkg, "open")
    dirs = _directions(70, 1)
    with _tracer(pkg, flat, mega=False, mis=False) as pt:
        with pytest.raises(pkg._capi.PtcError) as e:
            pt.environment_light_pdf(dirs)
        assert e.value.code == pkg._capi.PTC_ERR_INVALID and "no environment" in str(e.value)
        pt.environment = np.zeros((4, 4, 3), dtype=np.float32)
        assert not pt.environment_light_pdf(dirs).any()
        pt.environment = ENV
        assert pt.environment_light_pdf(dirs).any()
        lib, ctx = pt._lib, pt._ctx
        out = np.zeros(70, np.float32)
        assert lib.ptc_environment_light_pdf(ctx, None, 70, out.ctypes.data, 0) == pkg._capi.PTC_ERR_INVALID
        assert lib.ptc_environment_light_pdf(ctx, dirs.ctypes.data, 70, None, 0) == pkg._capi.PTC_ERR_INVALID
        assert lib.ptc_environment_light_pdf(ctx, None, 0, None, 0) == 0


# ---- 2. the megakernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(33, 17), (65, 33)])
@pytest.mark.parametrize("mb", [1, 2, 8])
def test_lamps_alone_in_the_closed_room(pkg, orc, w, h, mb):
    got = _against_the_loop(pkg, orc, "room", w, h, mb, direct=True)
    assert got["diffuse_hits"] > 0 and got["env_diffuse_hits"] == 0 and got["mis_misses"] == 0
    assert got["mis_emitter_hits"] == 0 if mb == 1 else mb < 8 or got["mis_emitter_hits"] > 0


@pytest.mark.parametrize("w,h", [(33, 17), (65, 33)])
@pytest.mark.parametrize("mb", [1, 2, 8])
def test_the_sky_alone_on_a_scene_without_lamps(pkg, orc, w, h, mb):
    got = _against_the_loop(pkg, orc, "open", w, h, mb, env=ENV, env_light=True)
    assert got["env_diffuse_hits"] > 0 and got["diffuse_hits"] == 0 and got["mis_emitter_hits"] == 0
    assert (got["mis_misses"] > 0) == (mb > 1)


@pytest.mark.parametrize("w,h", [(33, 17), (65, 33)])
@pytest.mark.parametrize("mb", [1, 2, 8])
def test_lamps_and_sky_together(pkg, orc, w, h, mb):
    got = _against_the_loop(pkg, orc, "lit_open", w, h, mb, env=SIDE, env_light=True, direct=True)
    assert got["shadow_rays"] > 0 and got["env_shadow_rays"] > got["env_unoccluded"] > 0
    assert (got["mis_misses"] > 0) == (mb > 1)


def test_roulette_under_the_lens(pkg, orc):
    got = _against_the_loop(pkg, orc, "lit_open", env=SIDE, env_light=True, direct=True, roulette=1, lens=LENS)
    assert got["mis_misses"] > 0 and got["mis_emitter_hits"] > 0


def test_lamps_sampled_under_a_sky_that_is_not(pkg, orc):
    """"direct_light" with an environment that is no light: every miss counts the sky, the lamps' gate alone works"""
    got = _against_the_loop(pkg, orc, "lit_open", env=SIDE, direct=True, roulette=2)
    assert got["env_diffuse_hits"] == 0 and got["mis_misses"] == 0 and got["mis_emitter_hits"] > 0


@pytest.mark.parametrize("name", ["glass_lamp", "metal_glass", "dark_lamps"])
def test_lamp_scenes(pkg, orc, name):
    """a lamp behind glass (every shadow ray blocked, the lamp reached through dielectric vertices: weight 1 paths), a lamp seen in
    metal, an emissive material of luminance 0 (its inv_pdf_m is 0: a hit counts fully)"""
    got = _against_the_loop(pkg, orc, name, 48, 36, 5, direct=True)
    assert got["shadow_rays"] > 0
    if name == "glass_lamp":
        assert got["unoccluded"] == 0


def test_iteration_2_31_minus_5(pkg, orc):
    _against_the_loop(pkg, orc, "lit_open", mb=4, iters=2, iter_begin=2 ** 31 - 5, env=SIDE, env_light=True, direct=True)


def test_two_interleaved_ranks_against_the_one_context_frame(pkg):
    scene, flat = _scene(pkg, "lit_open")
    with _tracer(pkg, flat, env_light=True, direct=True) as pt:
        one = _run(pt, scene.camera, SIDE)
    assert one["mis_misses"] > 0
    parts = []
    for rank in (0, 1):
        with _tracer(pkg, flat, env_light=True, direct=True, interleave=(rank, 2, 8)) as pt:
            parts.append(_run(pt, scene.camera, SIDE))
        rows = [r for first in range(rank * 8, H, 16) for r in range(first, min(first + 8, H))]
        for p in PLANES:
            assert np.array_equal(_bits(parts[-1][p].reshape(len(rows), W, -1)), _bits(one[p].reshape(H, W, -1)[rows])), (rank, p)
    for k in ("rays",) + SIX + MIS:
        assert parts[0][k] + parts[1][k] == one[k], k


def test_another_map_between_frames_and_its_removal(pkg, orc):
    """set, trace 2; another map of another size, trace 2; no map, trace 2 (the frame samples neither light: the plain instance); the
    first map again: the restatement continued with prev="""
    scene, flat = _scene(pkg, "open")
    other = sun_map(12, seed=9, sky=0.5, sun=90.0)
    ref = None
    for k, env in enumerate((ENV, other, None, ENV)):
        entries = _table(pkg, env) if env is not None else None
        ref = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 2 * k, 2, 4, env=env, entries=entries, env_light=True, mis=True, prev=ref)
    with _tracer(pkg, flat, mb=4, env_light=True) as pt:
        pt.max_iterations = 8
        for env in (ENV, other, None, ENV):
            pt.environment = env
            pt.path_trace(scene.camera)
            pt.path_trace(scene.camera)
        _same(_result(pt), ref, PLANES, "maps")


# ---- 3. only colour differs; the cases that change nothing ---------------------------------------------------------------------------------
def test_only_colour_differs(pkg):
    scene, flat = _scene(pkg, "lit_open")
    runs = []
    for on in (False, True):
        with _tracer(pkg, flat, mis=on, env_light=True, direct=True, roulette=2) as pt:
            runs.append(_run(pt, scene.camera, SIDE))
    off, on = runs
    _same(on, off, ("normal", "depth", "rays") + SIX, "only colour")
    assert not np.array_equal(off["color"], on["color"])
    assert off["mis_misses"] == 0 and off["mis_emitter_hits"] == 0 and on["mis_misses"] > 0


@pytest.mark.parametrize("case", ["neither_parameter", "zeros", "no_lamps"])
def test_the_bits_of_mis_0(pkg, case):
    """mis 1 with neither light parameter, with "environment_light" under a map of zeros, and with "direct_light" on a scene without
    lamps, gives the bits of mis 0"""
    scene, flat = _scene(pkg, "open" if case == "no_lamps" else "lit_open")
    kw = {"neither_parameter": dict(), "zeros": dict(env_light=True), "no_lamps": dict(direct=True)}[case]
    env = np.zeros((4, 4, 3), dtype=np.float32) if case == "zeros" else SIDE
    runs = []
    for on in (False, True):
        with _tracer(pkg, flat, mis=on, **kw) as pt:
            runs.append(_run(pt, scene.camera, env))
    _same(runs[1], runs[0], EVERYTHING, case)
    assert runs[1]["mis_misses"] == 0 and runs[1]["mis_emitter_hits"] == 0


def test_the_streaming_loop_refuses_and_queues_nothing(pkg):
    scene, flat = _scene(pkg, "lit_open")
    with _tracer(pkg, flat, mega=False, mis=True) as pt:
        pt.max_iterations = 4
        for _ in range(2):
            with pytest.raises(pkg._capi.PtcError) as e:
                pt.path_trace(scene.camera)
            assert e.value.code == pkg._capi.PTC_ERR_INVALID and "mis is rendered by the megakernel" in str(e.value)
        cam = pkg._capi.ptc_camera()
        assert pt._lib.ptc_trace_begin(pt._ctx, C.byref(cam)) == pkg._capi.PTC_ERR_INVALID
        assert pt.iteration() == 0 and pt.stats()["rays_total"] == 0 and pt.stats()["frames"] == 0
        pt.mis = False  # and without it the context renders as ever
        pt.path_trace(scene.camera)
        assert pt.iteration() == 1 and pt.stats()["rays_total"] > 0
    with pkg.PathTracer(device=0) as pt:
        for bad in (-1, 2):
            with pytest.raises(pkg._capi.PtcError) as e:
                pt.set_param("mis", bad)
            assert "mis must be 0 or 1" in str(e.value)


# ---- 4. the same expectation ------------------------------------------------------------------------------------------------------------
def sun_yard(pkg):
    """test_gpu_environment_light's yard: a triangle floor under the sky and a triangle panel hanging over it; albedo 0.5"""
    s = pkg.SceneDescription()

    def quad(x0, x1, z0, z1, y):
        positions = np.array([[x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]], dtype=np.float32)
        return pkg.Mesh(positions, np.array([0, 1, 2, 0, 2, 3], dtype=np.uint32))

    s.add_material("floor", pkg.DiffuseMateral((0.5, 0.5, 0.5)))
    s.add_material("panel", pkg.DiffuseMateral((0.5, 0.4, 0.3)))
    s.add_object(s.add_mesh("models/yard_floor.obj", quad(-6.0, 6.0, -6.0, 6.0, -1.0)), pkg.glmlite.identity(), "floor")
    s.add_object(s.add_mesh("models/yard_panel.obj", quad(-0.9, 0.7, -1.2, 0.4, 0.1)), pkg.glmlite.identity(), "panel")
    s.camera = pkg.scenes._camera_from_look_at((0.0, 1.6, 4.0), (0.0, -0.8, -0.4), vfov_deg=45.0)
    return s


def low_panel_scene(pkg):
    """A 12 x 12 triangle floor (albedo 0.7), a 1 x 1 emissive quad 0.03 above it, a diffuse back wall; the camera looks at the panel's
    near edge (three meshes: build_scene(distinct_meshes=True)).  Everything is triangles: no radius-1000 sphere under the shadow epsilon."""
    s = pkg.SceneDescription()

    def quad(p0, p1, p2, p3):
        return pkg.Mesh(np.array([p0, p1, p2, p3], dtype=np.float32), np.array([0, 1, 2, 0, 2, 3], dtype=np.uint32))

    s.add_material("floor", pkg.DiffuseMateral((0.7, 0.7, 0.7)))
    s.add_material("wall", pkg.DiffuseMateral((0.6, 0.3, 0.25)))
    s.add_material("panel", pkg.EmissiveMaterial((6.0, 5.5, 4.5)))
    ident = pkg.glmlite.identity()
    s.add_object(s.add_mesh("models/lp_floor.obj", quad((-6, -1, -6), (6, -1, -6), (6, -1, 6), (-6, -1, 6))), ident, "floor")
    s.add_object(s.add_mesh("models/lp_wall.obj", quad((-6, -1, -2), (6, -1, -2), (6, 3, -2), (-6, 3, -2))), ident, "wall")
    s.add_object(s.add_mesh("models/lp_panel.obj", quad((-0.5, -0.97, -1.0), (0.5, -0.97, -1.0), (0.5, -0.97, 0.0), (-0.5, -0.97, 0.0))), ident, "panel")
    s.camera = pkg.scenes._camera_from_look_at((0.0, -0.2, 2.6), (0.0, -1.0, 0.0), vfov_deg=40.0)
    return s


def stat_blocks(pkg, scene, env, direct, env_light, blocks=16, per_block=256, w=32, h=24, distinct_meshes=False):
    """Per mode (mis 0, 1; the light parameters on in both) and block b the image mean per channel of iterations [per_block b,
    per_block (b + 1)), as test_gpu_direct_loop.stat_blocks takes them, and whether normal and depth agreed"""
    flat = scene.build_scene(distinct_meshes=distinct_meshes)
    means = np.zeros((2, blocks, 3))
    geometry = []
    tracers = []
    try:
        for mode in (0, 1):
            pt = pkg.PathTracer(device=0, max_bounces=direct_loop_scenes.STAT_BOUNCES)
            tracers.append(pt)
            pt.current_gpu_method = pkg.GPUMethod.megakernel
            pt.direct_light, pt.environment_light, pt.mis = direct, env_light, bool(mode)
            pt.environment = env
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


def _paired(means, geometry, what, lower_spread=False):
    assert all(geometry), "normal and depth differ between the modes"
    d = means[1] - means[0]
    bound = T_BOUND * d.std(axis=0, ddof=1) / np.sqrt(len(d))
    spread = means.std(axis=1, ddof=1)
    print(what, "image mean", means.mean(axis=1), "mean(D)", d.mean(axis=0), "bound", bound, "spread 0 / 1", spread[0], spread[1],
          "variance ratio 0 / 1", (spread[0] / spread[1]) ** 2)
    assert (means.mean(axis=1) > 0.05).all()
    assert (np.abs(d.mean(axis=0)) <= bound).all(), (what, d.mean(axis=0), bound)
    if lower_spread:
        assert (spread[1] < spread[0]).all(), (what, spread)


def test_same_expectation_under_the_lamp(pkg):
    """Section 5g's design: paired over B = 16 blocks of 256 iterations at 32 x 24 and 24 bounces in the closed 12-triangle room with
    one sphere lamp, "direct_light" on in both modes; D_b = image mean of block b with mis minus without -- the render without it is
    the code as it stood, the reference.  Normal and depth equal per block; |mean(D)| <= 4.073 sd(D) / sqrt(16) per channel.  (The
    expectations are equal exactly: the last bounce's samples keep weight 1, section 5l item 7.)  The spreads are printed, not asserted:
    the room's lamp is small and far from every wall, the case the lamp sample alone already serves."""
    _paired(*stat_blocks(pkg, direct_loop_scenes.small_lamp_room(pkg), None, True, False), "lamp")


def test_same_expectation_under_the_sky(pkg):
    """... and on the triangle floor under a 32 x 32 sky with a bright two-texel sun, "environment_light" on in both modes"""
    _paired(*stat_blocks(pkg, sun_yard(pkg), sun_map(32, seed=21, sky=0.2, sun=2000.0), False, True), "sky")


def test_same_expectation_lower_spread_under_a_low_panel(pkg):
    """... and on low_panel_scene, an emissive quad 0.03 above the floor: the lamp sample's cos_l / d^2 explodes under the panel, the
    case the continuation ray serves.  The numpy restatement shows the ratio of the spreads of 16 block means (mis 1 / mis 0, 24 x 16,
    8 iterations a block) at 0.25 / 0.37 / 0.39 (tools/mis_ab.py --cpu), under the 0.5 that lets this test assert it: the spread of
    the block means with mis is below the spread without, at equal iteration counts (64 a block)."""
    _paired(*stat_blocks(pkg, low_panel_scene(pkg), None, True, False, per_block=64, distinct_meshes=True), "low panel", lower_spread=True)


# ---- 5. the command line ---------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_PT = os.path.join(ROOT, "cuda-path-tracer_amd", "host", "hip_pt")


def _read_raw(path):
    data = open(path, "rb").read()
    assert data[:4] == b"PTRF"
    w, h, ch = struct.unpack_from("<III", data, 4)
    assert ch == 7 and len(data) == 16 + 4 * 7 * w * h
    f = np.frombuffer(data, dtype="<f4", offset=16)
    P = w * h
    return {"color": f[:3 * P].reshape(h, w, 3), "normal": f[3 * P:6 * P].reshape(h, w, 3), "depth": f[6 * P:].reshape(h, w)}


@pytest.mark.parametrize("extra", [["--mis", "--environment-light"], ["--mis"], ["--mis", "--gpus", "2"]], ids=["flag", "scene_key", "two_ranks"])
def test_hip_pt_mis_equals_the_python_tracer(pkg, tmp_path, extra):
    """hip_pt --method megakernel --mis on the asset scene lit by a sky with a sun (its "environment" says "light": true): the float
    framebuffers are the Python PathTracer's with environment_light and mis, and not those without mis"""
    if not os.path.exists(HIP_PT):
        subprocess.run(["make"], cwd=os.path.dirname(HIP_PT), check=True, stdout=subprocess.DEVNULL)
    scene = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "spheres_sun.json"))
    w, h = scene.resolution
    flat = scene.build_scene()
    spp, mb = 2, 4
    with _tracer(pkg, flat, w, h, mb, env_light=True) as pt:
        want = _run(pt, scene.camera, scene.environment, iters=spp)
    with _tracer(pkg, flat, w, h, mb, mis=False, env_light=True) as pt:
        without = _run(pt, scene.camera, scene.environment, iters=spp)
    assert want["mis_misses"] > 0 and not np.array_equal(want["color"], without["color"])
    raw = tmp_path / "out.raw"
    cmd = [HIP_PT, "scenes/spheres_sun.json", "-o", str(tmp_path / "out.png"), "--spp", str(spp), "--max-bounces", str(mb), "--dump-raw", str(raw),
           "--method", "megakernel"] + extra
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    _same(_read_raw(raw), want, PLANES, extra)
