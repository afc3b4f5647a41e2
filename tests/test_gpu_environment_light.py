"""Environment light sampling on the GPU (ptc_environment_light, ptc_set_param "environment_light"): the query and the
megakernel's environment-light instance against the numpy restatement tests/env_light_ref.py, bit for bit; what the parameter must
leave alone; the cases in which it must change nothing; the estimator's expectation and spread against the render without it."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import direct_ref
import env_light_ref
import env_ref
import loop_ref

pytestmark = pytest.mark.gpu

PLANES = ("color", "normal", "depth")
LAMP_COUNTERS = ("diffuse_hits", "shadow_rays", "unoccluded")
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
        _cache[key] = (env_light_ref.table_of(pkg, env)[0], env_ref.apron(env), env)  # (env kept: its id stays its own)
    return _cache[key][:2]


def _scene(pkg, name):
    """name -> (scene, flat), built once.  open: a height field under the sky, no lamp.  lit_open: cornell_lit (a sphere lamp, a mesh
    panel lamp, three balls) with the right wall taken out."""
    if name not in _cache:
        if name == "open":
            scene = pkg.scenes.heightfield_scene(resolution=(W, H), nx=17, nz=9)
        else:
            scene = pkg.scenes.cornell_lit(resolution=(W, H), with_mesh=True)
            at = scene.objects_material_mapping_.index("right")
            del scene.objects_[at], scene.objects_material_mapping_[at]
            scene.camera = pkg.scenes._camera_from_look_at((-1.2, 0.0, 4.0), (0.6, -0.1, 0.0), vfov_deg=50.0)
        _cache[name] = (scene, scene.build_scene())
    return _cache[name]


def _tracer(pkg, flat, w=W, h=H, mb=8, variant=None, mega=True, env_light=True, direct=False, roulette=0, lens=None, interleave=None):
    pt = pkg.PathTracer(device=0, max_bounces=mb)
    if variant is not None:
        pt.set_trace_variant(variant)
    if mega:
        pt.current_gpu_method = pkg.GPUMethod.megakernel
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


ENV_COUNTERS = ("env_diffuse_hits", "env_shadow_rays", "env_unoccluded")
EVERYTHING = PLANES + ("rays",) + LAMP_COUNTERS + ENV_COUNTERS


def _against_the_loop(pkg, orc, scene_name, w=W, h=H, mb=8, env=ENV, iters=ITERS, iter_begin=0, direct=False, roulette=0, lens=None):
    scene, flat = _scene(pkg, scene_name)
    entries, _ = _table(pkg, env)
    ref = loop_ref.render_megakernel(orc, flat, scene.camera, w, h, iter_begin, iters, mb, env=env, entries=entries, env_light=True,
                                          direct=direct, roulette=roulette, lens=lens)
    with _tracer(pkg, flat, w, h, mb, direct=direct, roulette=roulette, lens=lens) as pt:
        got = _run(pt, scene.camera, env, iters, iter_begin)
    _same(got, ref, EVERYTHING, (scene_name, w, h, mb, direct, roulette, lens, iter_begin))
    return got


# ---- 1. the query ---------------------------------------------------------------------------------------------------------------------
def _query_case(pkg, orc, n_map, sample_index):
    key = ("query", n_map, sample_index)
    if key not in _cache:
        scene, flat = _scene(pkg, "lit_open")
        env = sun_map(n_map, seed=n_map)
        points, normals = direct_ref.room_points(4099, seed=11)
        entries, texels = env_light_ref.table_of(pkg, env)[0], env_ref.apron(env)
        _cache[key] = (flat, env, points, normals, env_light_ref.query(orc, flat, entries, texels, points, normals, sample_index))
    return _cache[key]


@pytest.mark.parametrize("sample_index", [0, 7, 2 ** 31 - 5])
@pytest.mark.parametrize("n_map", [2, 5, 64])
def test_query_against_the_restatement(pkg, orc, n_map, sample_index):
    """4099 points (no multiple of 64 or 256) on the open room with its mesh and sphere occluders, every fifth normal flipped; host
    pointers: radiance, rays, visible and the counters"""
    flat, env, points, normals, (radiance, rays, visible, sampled) = _query_case(pkg, orc, n_map, sample_index)
    with _tracer(pkg, flat, mega=False, env_light=False) as pt:
        pt.environment = env
        before = (pt.stats(), pt.direct_stats(), pt.occlusion_stats())
        got = pt.environment_light(points, normals, sample_index, want_rays=True)
        st = pt.environment_light_stats()
        assert (pt.stats(), pt.direct_stats(), pt.occlusion_stats()) == before  # it moves no other statistics
    for name, a, b in (("radiance", got[0], radiance), ("rays", got[1], rays)):
        bad = (_bits(a) != _bits(b)).any(axis=1)
        assert not bad.any(), (name, n_map, sample_index, int(bad.sum()), np.nonzero(bad)[0][:4].tolist())
    assert np.array_equal(got[2], visible)
    assert (st["points"], st["sampled"], st["unoccluded"]) == (4099, int(sampled.sum()), int(visible.sum()))
    assert 0 < visible.sum() < sampled.sum() < 4099  # culled samples, blocked rays and free ones are all there


def test_query_on_device_pointers_and_the_trace_variants(pkg, orc):
    """torch tensors for every array; trace variants 1 and 0 (the exact closest-hit kernel) agree with 3"""
    torch = pytest.importorskip("torch")
    flat, env, points, normals, (radiance, rays, visible, _) = _query_case(pkg, orc, 5, 7)
    n = len(points)
    for variant in (3, 1, 0):
        with _tracer(pkg, flat, mega=False, env_light=False, variant=variant) as pt:
            pt.environment = env
            p, nr = torch.from_numpy(points).cuda(), torch.from_numpy(normals).cuda()
            out = torch.full((n, 3), -1.0, dtype=torch.float32, device="cuda")
            out_rays = torch.full((n, 8), -1.0, dtype=torch.float32, device="cuda")
            vis = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
            pt.environment_light_dev(p.data_ptr(), nr.data_ptr(), n, 7, out.data_ptr(), out_rays.data_ptr(), vis.data_ptr())
            assert np.array_equal(_bits(out.cpu().numpy()), _bits(radiance)), variant
            assert np.array_equal(_bits(out_rays.cpu().numpy()), _bits(rays)), variant
            assert np.array_equal(vis.cpu().numpy(), visible), variant
            host = pt.environment_light(points, normals, 7)
            assert np.array_equal(_bits(host), _bits(radiance)), variant


def test_query_on_a_map_of_1024(pkg, orc):
    """entry indices above 2^16 rows of the table: a map of 1024 x 1024 whose weight sits in its last rows"""
    scene, flat = _scene(pkg, "lit_open")
    n = 1024
    env = np.full((n, n, 3), 1e-3, dtype=np.float32)
    env[n - 40:, :, :] = np.random.default_rng(3).uniform(1.0, 2.0, (40, n, 3)).astype(np.float32)
    env[n // 2 - 3, n // 2 + 5] = (900.0, 800.0, 700.0)
    points, normals = direct_ref.room_points(515, seed=12)
    entries, texels = env_light_ref.table_of(pkg, env)[0], env_ref.apron(env)
    radiance, rays, visible, sampled = env_light_ref.query(orc, flat, entries, texels, points, normals, 3)
    v, u = env_light_ref.stream(orc, np.arange(len(points)), 3, 0)
    squares = env_light_ref.sample(entries, texels, points, normals, v, u)["square"]
    assert (squares >= (1 << 16) * 8).sum() > 100
    with _tracer(pkg, flat, mega=False, env_light=False) as pt:
        pt.environment = env
        got = pt.environment_light(points, normals, 3, want_rays=True)
    assert np.array_equal(_bits(got[0]), _bits(radiance)) and np.array_equal(_bits(got[1]), _bits(rays)) and np.array_equal(got[2], visible)


def test_query_refusals_and_a_map_of_zeros(pkg):
    scene, flat = _scene(pkg, "lit_open")
    points, normals = direct_ref.room_points(70, seed=1)
    with _tracer(pkg, flat, mega=False, env_light=False) as pt:
        with pytest.raises(pkg._capi.PtcError) as e:
            pt.environment_light(points, normals)
        assert e.value.code == pkg._capi.PTC_ERR_INVALID and "no environment" in str(e.value)
        pt.environment = np.zeros((4, 4, 3), dtype=np.float32)
        radiance, rays, visible = pt.environment_light(points, normals, want_rays=True)
        assert not radiance.any() and not visible.any() and np.array_equal(rays[:, :3], points) and (rays[:, 3] == np.float32(1e-4)).all()
        assert not rays[:, 4:].any()
        st = pt.environment_light_stats()
        assert (st["points"], st["sampled"], st["launches"]) == (70, 0, 0)  # zeros, and nothing launched
        pt.environment = ENV
        lib, ctx = pt._lib, pt._ctx
        pt.environment_light(points, normals)  # (pushes the map)
        out = np.zeros((70, 3), np.float32)
        assert lib.ptc_environment_light(ctx, None, normals.ctypes.data, 70, 0, out.ctypes.data, None, None, 0) == pkg._capi.PTC_ERR_INVALID
        assert lib.ptc_environment_light(ctx, points.ctypes.data, normals.ctypes.data, 70, 0, None, None, None, 0) == pkg._capi.PTC_ERR_INVALID
        assert lib.ptc_environment_light(ctx, None, None, 0, 0, None, None, None, 0) == 0


# ---- 2. the megakernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(33, 17), (65, 33)])
@pytest.mark.parametrize("mb", [1, 2, 8])
def test_environment_light_alone_on_a_scene_without_lamps(pkg, orc, w, h, mb):
    got = _against_the_loop(pkg, orc, "open", w, h, mb)
    assert got["env_diffuse_hits"] > 0 and got["diffuse_hits"] == 0


@pytest.mark.parametrize("roulette,lens", [(0, None), (1, LENS)])
def test_with_direct_light_on_a_scene_with_lamps(pkg, orc, roulette, lens):
    """lamp sample and environment sample, two shadow rays per diffuse hit; with roulette 1 and the lens"""
    got = _against_the_loop(pkg, orc, "lit_open", env=SIDE, direct=True, roulette=roulette, lens=lens)
    assert got["shadow_rays"] > 0 and got["env_shadow_rays"] > got["env_unoccluded"] > 0
    assert got["env_diffuse_hits"] == got["diffuse_hits"]


def test_emitters_without_direct_light(pkg, orc):
    """the lamps are there but not sampled (lt.records null): every emitter hit counts, the environment's gate alone works"""
    got = _against_the_loop(pkg, orc, "lit_open", env=SIDE, direct=False, roulette=2)
    assert got["diffuse_hits"] == 0 and got["env_diffuse_hits"] > 0 and got["env_unoccluded"] > 0


def test_iteration_2_31_minus_5(pkg, orc):
    _against_the_loop(pkg, orc, "open", mb=4, iters=2, iter_begin=2 ** 31 - 5)


def test_two_interleaved_ranks_against_the_one_context_frame(pkg, orc):
    """the megakernel's streams are keyed by the pixel: two ranks' rows, dealt in blocks of 8, are the one-context frame's rows"""
    scene, flat = _scene(pkg, "lit_open")
    with _tracer(pkg, flat, direct=True) as pt:
        one = _run(pt, scene.camera, SIDE)
    assert one["env_unoccluded"] > 0
    parts = []
    for rank in (0, 1):
        with _tracer(pkg, flat, direct=True, interleave=(rank, 2, 8)) as pt:
            parts.append(_run(pt, scene.camera, SIDE))
        rows = [r for first in range(rank * 8, H, 16) for r in range(first, min(first + 8, H))]
        for p in PLANES:
            assert np.array_equal(_bits(parts[-1][p].reshape(len(rows), W, -1)), _bits(one[p].reshape(H, W, -1)[rows])), (rank, p)
    for k in ("rays",) + LAMP_COUNTERS + ENV_COUNTERS:
        assert parts[0][k] + parts[1][k] == one[k], k


def test_another_map_between_frames_and_its_removal(pkg, orc):
    """set, trace 2; another map of another size, trace 2 (the old table is gone with the old map); no map, trace 2: the restatement
    continued with prev=.  Then the first map again: a table is built anew."""
    scene, flat = _scene(pkg, "open")
    other = sun_map(12, seed=9, sky=0.5, sun=90.0)
    ref = None
    for k, env in enumerate((ENV, other, None, ENV)):
        entries = _table(pkg, env)[0] if env is not None else None
        ref = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 2 * k, 2, 4, env=env, entries=entries, env_light=True, prev=ref)
    with _tracer(pkg, flat, mb=4) as pt:
        pt.max_iterations = 8
        for env in (ENV, other, None, ENV):
            pt.environment = env
            pt.path_trace(scene.camera)
            pt.path_trace(scene.camera)
        _same(_result(pt), ref, PLANES, "maps")


# ---- 3. only colour differs; the cases that change nothing ---------------------------------------------------------------------------------
def test_only_colour_differs(pkg):
    """normal, depth, rays_total and the lamps' counters are those of the render without the parameter"""
    scene, flat = _scene(pkg, "lit_open")
    runs = []
    for on in (False, True):
        with _tracer(pkg, flat, env_light=on, direct=True, roulette=2) as pt:
            runs.append(_run(pt, scene.camera, SIDE))
    off, on = runs
    _same(on, off, ("normal", "depth", "rays") + LAMP_COUNTERS, "only colour")
    assert not np.array_equal(off["color"], on["color"])
    assert off["env_diffuse_hits"] == 0 and on["env_diffuse_hits"] > 0 and on["env_unoccluded"] > 0


@pytest.mark.parametrize("env", [None, np.zeros((4, 4, 3), dtype=np.float32)], ids=["no_map", "zeros"])
@pytest.mark.parametrize("direct", [False, True])
def test_off_equivalence(pkg, env, direct):
    """the parameter at 1 with no map, and with a map of zeros, gives the bits of 0"""
    scene, flat = _scene(pkg, "lit_open")
    runs = []
    for on in (False, True):
        with _tracer(pkg, flat, env_light=on, direct=direct) as pt:
            runs.append(_run(pt, scene.camera, env))
    _same(runs[1], runs[0], EVERYTHING, ("off", direct))
    assert runs[1]["env_diffuse_hits"] == 0


def test_the_streaming_loop_refuses_and_queues_nothing(pkg):
    scene, flat = _scene(pkg, "open")
    with _tracer(pkg, flat, mega=False, env_light=True) as pt:
        pt.environment = ENV
        pt.max_iterations = 4
        for _ in range(2):
            with pytest.raises(pkg._capi.PtcError) as e:
                pt.path_trace(scene.camera)
            assert e.value.code == pkg._capi.PTC_ERR_INVALID and "environment_light" in str(e.value)
        cam = pkg._capi.ptc_camera()
        assert pt._lib.ptc_trace_begin(pt._ctx, C.byref(cam)) == pkg._capi.PTC_ERR_INVALID
        assert pt.iteration() == 0 and pt.stats()["rays_total"] == 0 and pt.stats()["frames"] == 0
        pt.environment_light = False  # and without it the context renders as ever
        pt.path_trace(scene.camera)
        assert pt.iteration() == 1 and pt.stats()["rays_total"] > 0
    with pkg.PathTracer(device=0) as pt:
        for bad in (-1, 2):
            with pytest.raises(pkg._capi.PtcError):
                pt.set_param("environment_light", bad)


# ---- 4. the same expectation, a lower spread -------------------------------------------------------------------------------------------
STAT_BOUNCES = 12


def sun_yard(pkg):
    """A triangle floor under the sky and a triangle panel hanging over it (the blocker): no sphere of radius 1000, whose own wall blocks
    some of the shadow rays that start on it (DESIGN section 5g's finding on the shadow epsilon).  Albedo 0.5."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()

    def quad(x0, x1, z0, z1, y):
        positions = np.array([[x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]], dtype=np.float32)
        return pkg.Mesh(positions, np.array([0, 1, 2, 0, 2, 3], dtype=np.uint32))

    s.add_material("floor", pkg.DiffuseMateral((0.5, 0.5, 0.5)))
    s.add_material("panel", pkg.DiffuseMateral((0.5, 0.4, 0.3)))
    s.add_object(s.add_mesh("models/yard_floor.obj", quad(-6.0, 6.0, -6.0, 6.0, -1.0)), glm.identity(), "floor")
    s.add_object(s.add_mesh("models/yard_panel.obj", quad(-0.9, 0.7, -1.2, 0.4, 0.1)), glm.identity(), "panel")
    s.camera = pkg.scenes._camera_from_look_at((0.0, 1.6, 4.0), (0.0, -0.8, -0.4), vfov_deg=45.0)
    return s


def stat_blocks(pkg, blocks=16, per_block=256, w=32, h=24):
    """Per mode (environment_light 0, 1) and block b the image mean per channel of iterations [per_block b, per_block (b + 1)), as
    test_gpu_direct_loop.stat_blocks takes them: each block starts from cleared framebuffers at iteration per_block * b, so the
    running mean holds (sum of the block's samples) / (per_block (b + 1))."""
    scene = sun_yard(pkg)
    flat = scene.build_scene()
    env = sun_map(32, seed=21, sky=0.2, sun=2000.0)
    means = np.zeros((2, blocks, 3))
    geometry = []
    tracers = []
    try:
        for mode in (0, 1):
            pt = pkg.PathTracer(device=0, max_bounces=STAT_BOUNCES)
            tracers.append(pt)
            pt.current_gpu_method = pkg.GPUMethod.megakernel
            pt.environment_light = bool(mode)
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


def test_same_expectation_lower_spread(pkg):
    """Paired over B = 16 blocks of 256 iterations at 32 x 24 (fixed seeds: deterministic), on a triangle floor with a blocker under a
    32 x 32 sky with a bright two-texel sun.  D_b = image mean of block b with environment light minus without -- the render without
    it is the code as it stood, the reference.  |mean(D)| <= 4.073 sd(D) / sqrt(16) per channel (the two-sided 0.1 % point of Student's
    t, 15 degrees of freedom), and the spread of the block means with the parameter is below the spread without.  (A diffuse hit at the
    last of the 12 bounces still draws a sample the capped plain render has no term for: at most 0.5^12 = 2.4e-4 of a path's light, on
    the few paths that are still alive there -- far below what the test resolves.)"""
    means, geometry = stat_blocks(pkg)
    assert all(geometry)
    d = means[1] - means[0]
    bound = T_BOUND * d.std(axis=0, ddof=1) / np.sqrt(len(d))
    spread = means.std(axis=1, ddof=1)
    print("image mean", means.mean(axis=1), "mean(D)", d.mean(axis=0), "bound", bound, "spread 0 / 1", spread[0], spread[1])
    assert (means.mean(axis=1) > 0.05).all()
    assert (np.abs(d.mean(axis=0)) <= bound).all(), (d.mean(axis=0), bound)
    assert (spread[1] < spread[0]).all(), spread


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


@pytest.mark.parametrize("extra", [["--environment-light"], [], ["--environment-light", "--gpus", "2"]], ids=["flag", "scene_key", "two_ranks"])
def test_hip_pt_environment_light_equals_the_python_tracer(pkg, tmp_path, extra):
    """hip_pt --method megakernel on the asset scene lit by a sky with a sun (its "environment" says "light": true), with the flag, by
    the scene's key alone, and over two ranks: the float framebuffers are the Python PathTracer's with environment_light = True"""
    if not os.path.exists(HIP_PT):
        subprocess.run(["make"], cwd=os.path.dirname(HIP_PT), check=True, stdout=subprocess.DEVNULL)
    scene = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "spheres_sun.json"))
    assert scene.environment_source["light"] is True and scene.environment.shape == (32, 32, 3)
    w, h = scene.resolution
    flat = scene.build_scene()
    spp, mb = 2, 4
    with _tracer(pkg, flat, w, h, mb) as pt:
        want = _run(pt, scene.camera, scene.environment, iters=spp)
    assert want["env_unoccluded"] > 0
    raw = tmp_path / "out.raw"
    cmd = [HIP_PT, "scenes/spheres_sun.json", "-o", str(tmp_path / "out.png"), "--spp", str(spp), "--max-bounces", str(mb), "--dump-raw", str(raw),
           "--method", "megakernel"] + extra
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    _same(_read_raw(raw), want, PLANES, extra)
