"""Environment lighting (ptc_set_environment) on the GPU against its CPU restatement (tests/loop_ref.py's loops
with tests/env_ref.py's lookup for a sky), bit for bit.  An environment changes only colour: every render here is compared in colour with the
restatement, and in normal, depth, the last frame's live counts and rays_total with the SAME context's render without an environment.
The lookup itself through ptc_sample_environment; every schedule of the streaming loop, the megakernel, emitters, roulette, a lens,
"direct_light", interleaved ranks, a late iteration; a map of zeros; a change of map between frames; removal; the refusals; denoise
and present; hip_pt --environment against the Python PathTracer.  The open scene is heightfield_scene(nx=17, nz=9) -- a mesh that opens the object list and three spheres (diffuse, metal,
glass) that end it -- at 33 x 17 and 65 x 33; 3 accumulated iterations unless a case says otherwise."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import env_ref
import lit_ref
import loop_ref

pytestmark = pytest.mark.gpu

PLANES = ("color", "normal", "depth")
COUNTERS = ("diffuse_hits", "shadow_rays", "unoccluded")
W, H, ITERS = 33, 17, 3
LENS = (0.25, 3.5)
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _env(n=7, seed=5, top=3.0):
    """a random map: no two texels alike, so a wrong texel or weight shows"""
    return np.random.default_rng(seed).uniform(0.0, top, (n, n, 3)).astype(np.float32)


ENV = _env()


def _scene(pkg, name):
    """name -> (scene, flat), built once"""
    if name not in _cache:
        if name == "open":
            scene = pkg.scenes.heightfield_scene(resolution=(W, H), nx=17, nz=9)
        else:  # cornell_lit (a sphere lamp, a mesh panel lamp) with the right wall taken out: lamp-lit, and open to the sky
            scene = pkg.scenes.cornell_lit(resolution=(W, H), with_mesh=True)
            at = scene.objects_material_mapping_.index("right")
            del scene.objects_[at], scene.objects_material_mapping_[at]
            scene.camera = pkg.scenes._camera_from_look_at((-1.2, 0.0, 4.0), (0.6, -0.1, 0.0), vfov_deg=50.0)
        _cache[name] = (scene, scene.build_scene())
    return _cache[name]


def _tracer(pkg, flat, w=W, h=H, mb=8, params=(), variant=None, method=None, direct=False, roulette=0, lens=None, interleave=None):
    pt = pkg.PathTracer(device=0, max_bounces=mb)
    for name, v in params:
        pt.set_param(name, v)
    if variant is not None:
        pt.set_trace_variant(variant)
    if method is not None:
        pt.current_gpu_method = method
    pt.direct_light = direct
    pt.roulette = roulette
    if lens is not None:
        pt.lens = lens
    pt.create_buffers((w, h), flat)
    if interleave is not None:
        rank, world, block = interleave
        pt.set_interleave(rank, world, block)
        pt.set_param("slot_offset", rank * w * h)
    return pt


def _result(pt):
    out = {p: pt.download(p) for p in PLANES}
    st = pt.stats()
    out["rays"], out["last_live"] = st["rays_total"], st["last_live"]
    out["persist_launches"] = pt.profile()["persist_launches"]
    out.update(pt.direct_loop_stats())
    return out


def _run(pt, camera, env, iters=ITERS, iter_begin=0):
    pt.environment = env
    pt.restart()
    if iter_begin:
        pt.set_iteration(iter_begin)
    pt.max_iterations = iter_begin + iters
    pt.reset_profile()
    rays0 = pt.stats()["rays_total"]
    for _ in range(iters):
        pt.path_trace(camera)
    out = _result(pt)
    out["rays"] -= rays0
    return out


def _both(pkg, flat, camera, env=ENV, iters=ITERS, iter_begin=0, **kw):
    """the same context: without an environment, then with it -> (gradient render, environment render)"""
    with _tracer(pkg, flat, **kw) as pt:
        base = _run(pt, camera, None, iters, iter_begin)
        if iter_begin == 0:
            return base, _run(pt, camera, env, iters)
    # (a run that starts late folds into what the framebuffers hold: ptc_restart leaves them to iteration 0 to overwrite.  A context
    # of its own, then, as the restatement starts from zeros)
    with _tracer(pkg, flat, **kw) as pt:
        return base, _run(pt, camera, env, iters, iter_begin)


def _colour_is(got, ref, what):
    a, b = _bits(got["color"]), _bits(np.asarray(ref["color"], dtype=np.float32).reshape(got["color"].shape))
    assert np.array_equal(a, b), (what, int(np.sum(a != b)), np.argwhere(a != b)[:4].tolist())


def _only_colour_differs(base, got, what, counters=()):
    for p in ("normal", "depth"):
        assert np.array_equal(_bits(base[p]), _bits(got[p])), (what, p)
    assert base["rays"] == got["rays"] and base["rays"] > 0, (what, base["rays"], got["rays"])
    assert base["last_live"] == got["last_live"], (what, base["last_live"], got["last_live"])
    for c in counters:
        assert base[c] == got[c], (what, c)
    assert not np.array_equal(base["color"], got["color"]), what  # (the environment does change the frame)


def _ref_streaming(orc, flat, camera, w, h, mb, env=ENV, iters=ITERS, iter_begin=0, **kw):
    key = ("stream", id(flat), w, h, mb, id(env), iters, iter_begin, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _cache:
        _cache[key] = loop_ref.render_streaming(orc, flat, camera, w, h, iter_begin, iters, mb, env=env, **kw)
    return _cache[key]


# ---- 1. the lookup ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 5, 64])
def test_sample_environment_against_the_restatement(pkg, n):
    _, flat = _scene(pkg, "open")
    env = np.random.default_rng(300 + n).uniform(0.0, 50.0, (n, n, 3)).astype(np.float32)
    dirs = env_ref.direction_set(np.random.default_rng(n), n)
    with _tracer(pkg, flat) as pt:
        pt.environment = env
        got = pt.sample_environment(dirs)
        size = C.c_uint32(99)
        assert pt._lib.ptc_get_environment(pt._ctx, C.byref(size)) == 0 and size.value == n
        assert pt.stats()["rays_total"] == 0 and pt.iteration() == 0
    want = env_ref.lookup(env, dirs)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (n, int(bad.sum()), dirs[bad.any(axis=1)][:4].tolist())
    assert (got[-10:] == 0.0).all() and (got[:4096] > 0.0).all()


# ---- 2. every schedule of the streaming loop ------------------------------------------------------------------------------------------
SCHEDULES = {
    "default": dict(),                                                     # k_raygen_env<true, true> finishes the sky pixels, k_shade_fused_env
    "three_kernels": dict(params=(("fused_shade", 0),)),                   # k_shade_env
    "no_filter": dict(params=(("filter_rays", 0),)),                       # every miss in k_shade_fused_env
    "no_prefold": dict(params=(("prefold", 0),)),
    "no_filter_three_kernels": dict(params=(("filter_rays", 0), ("fused_shade", 0))),
    "batch_4": dict(params=(("frames_in_flight", 8), ("batch_frames", 4))),
    "unstaged": dict(params=(("frames_in_flight", 1),)),
    "variant_0": dict(variant=0),
    "variant_1": dict(variant=1),
    "persist": dict(params=(("persist", 1), ("frames_in_flight", 12), ("batch_frames", 12))),  # falls back to the per-bounce launches
}


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_streaming_schedules(pkg, orc, name):
    scene, flat = _scene(pkg, "open")
    iters = 4 if name == "batch_4" else ITERS
    base, got = _both(pkg, flat, scene.camera, iters=iters, **SCHEDULES[name])
    _colour_is(got, _ref_streaming(orc, flat, scene.camera, W, H, 8, iters=iters), name)
    _only_colour_differs(base, got, name)
    if name == "persist":  # (the gradient's batch did take the persistent launch: the fallback is the environment's doing)
        assert base["persist_launches"] >= 1 and got["persist_launches"] == 0


@pytest.mark.parametrize("w,h", [(33, 17), (65, 33)])
@pytest.mark.parametrize("mb", [1, 2, 8])
@pytest.mark.parametrize("method", ["streaming", "megakernel"])
def test_sizes_and_bounces(pkg, orc, w, h, mb, method):
    scene, flat = _scene(pkg, "open")
    mega = method == "megakernel"
    base, got = _both(pkg, flat, scene.camera, w=w, h=h, mb=mb, method=pkg.GPUMethod.megakernel if mega else None)
    if mega:
        ref = loop_ref.render_megakernel(orc, flat, scene.camera, w, h, 0, ITERS, mb, env=ENV)
    else:
        ref = _ref_streaming(orc, flat, scene.camera, w, h, mb)
    _colour_is(got, ref, (method, w, h, mb))
    _only_colour_differs(base, got, (method, w, h, mb))
    assert got["rays"] == ref["rays"]


def test_prefold_on_the_open_room(pkg, orc):
    """the open cornell_lit opens with a sphere run in front of its mesh: k_raygen_next, k_shade_fused_env<.., kNext>"""
    scene, flat = _scene(pkg, "lit_open")
    ref = _ref_streaming(orc, flat, scene.camera, W, H, 4)
    for params in ((), (("prefold", 0),), (("filter_rays", 0),)):
        base, got = _both(pkg, flat, scene.camera, mb=4, params=params)
        _colour_is(got, ref, ("lit_open", params))
        _only_colour_differs(base, got, ("lit_open", params))


# ---- 3. emitters, roulette, a lens, direct light ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["streaming", "megakernel"])
@pytest.mark.parametrize("scene_name,roulette,lens", [("lit_open", 0, None), ("lit_open", 1, None), ("open", 3, None), ("open", 0, LENS),
                                                      ("lit_open", 3, LENS)])
def test_emitters_roulette_and_lens(pkg, orc, method, scene_name, roulette, lens):
    scene, flat = _scene(pkg, scene_name)
    mega = method == "megakernel"
    render = loop_ref.render_megakernel if mega else loop_ref.render_streaming
    ref = render(orc, flat, scene.camera, W, H, 0, ITERS, 8, env=ENV, lens=lens, roulette=roulette)
    what = (method, scene_name, roulette, lens)
    schedules = ({},) if mega else ({}, {"params": (("fused_shade", 0),)})
    for kw in schedules:
        base, got = _both(pkg, flat, scene.camera, roulette=roulette, lens=lens, method=pkg.GPUMethod.megakernel if mega else None, **kw)
        _colour_is(got, ref, what)
        _only_colour_differs(base, got, what)
        assert got["rays"] == ref["rays"]
    if roulette:
        assert ref["played"].sum() > 0 and ref["ended"].sum() > 0


@pytest.mark.parametrize("roulette,lens", [(0, None), (2, LENS)])
def test_direct_light_in_the_megakernel(pkg, orc, roulette, lens):
    """the environment counts at every miss whatever the light sample before it did; it is no lamp: the three loop counters stay"""
    scene, flat = _scene(pkg, "lit_open")
    ref = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 0, ITERS, 8, env=ENV, lens=lens, direct=True, roulette=roulette)
    assert ref["shadow_rays"] > 0
    base, got = _both(pkg, flat, scene.camera, method=pkg.GPUMethod.megakernel, direct=True, roulette=roulette, lens=lens)
    _colour_is(got, ref, ("direct", roulette, lens))
    _only_colour_differs(base, got, ("direct", roulette, lens), counters=COUNTERS)
    for c in COUNTERS:
        assert got[c] == ref[c], c


# ---- 4. interleaved ranks, a late iteration -----------------------------------------------------------------------------------------
def test_two_interleaved_ranks_against_the_one_context_frame(pkg, orc):
    """rows dealt in blocks of 8, slot_offset = rank * W * H: each rank against the restatement of its rows; and the environment is
    keyed by direction alone, so a rank's sky pixels are the one-context frame's"""
    scene, flat = _scene(pkg, "open")
    sh = orc.SceneHandle(flat)
    with _tracer(pkg, flat, mb=1) as pt:
        one = _run(pt, scene.camera, ENV, iters=1)
    whole, sky = one["color"].reshape(-1, 3), one["depth"].reshape(-1) == np.float32(1e6)  # (sky: the primary ray hit nothing)
    assert 50 < sky.sum() < W * H - 50
    for rank in (0, 1):
        pixels = lit_ref.interleaved_pixels(W, H, rank, 2, 8)
        ref = loop_ref.render_streaming(orc, flat, scene.camera, W, H, 0, ITERS, 8, env=ENV, pixels=pixels, slot_offset=rank * W * H, scene_handle=sh)
        base, got = _both(pkg, flat, scene.camera, interleave=(rank, 2, 8))
        _colour_is(got, ref, ("interleaved", rank))
        _only_colour_differs(base, got, ("interleaved", rank))
        with _tracer(pkg, flat, mb=1, interleave=(rank, 2, 8)) as pt:  # (the material draws are keyed by slot: the sky pixels alone compare)
            part = _run(pt, scene.camera, ENV, iters=1)["color"].reshape(-1, 3)
        assert np.array_equal(_bits(part[sky[pixels]]), _bits(whole[pixels][sky[pixels]])), rank


@pytest.mark.parametrize("method", ["streaming", "megakernel"])
def test_iteration_2_31_minus_5(pkg, orc, method):
    scene, flat = _scene(pkg, "open")
    mega = method == "megakernel"
    first = 2 ** 31 - 5
    render = loop_ref.render_megakernel if mega else loop_ref.render_streaming
    ref = render(orc, flat, scene.camera, W, H, first, 2, 4, env=ENV)
    base, got = _both(pkg, flat, scene.camera, mb=4, iters=2, iter_begin=first, method=pkg.GPUMethod.megakernel if mega else None)
    _colour_is(got, ref, (method, first))
    _only_colour_differs(base, got, (method, first))


# ---- 5. a map of zeros, a change of map, removal ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["streaming", "megakernel"])
def test_a_map_of_zeros_on_the_open_room(pkg, orc, method):
    """A dark sky over a lamp-lit room.  One iteration: the gradient's frame and the dark frame differ exactly at the pixels whose
    path left through the opening (every other outcome -- an emitter, the cap, roulette -- deposits the same bits under both), and
    each of those deposits exactly 0."""
    scene, flat = _scene(pkg, "lit_open")
    mega = method == "megakernel"
    zeros = np.zeros((4, 4, 3), dtype=np.float32)
    render = loop_ref.render_megakernel if mega else loop_ref.render_streaming
    ref = render(orc, flat, scene.camera, W, H, 0, 1, 8, env=zeros)
    base, got = _both(pkg, flat, scene.camera, env=zeros, iters=1, method=pkg.GPUMethod.megakernel if mega else None)
    _colour_is(got, ref, method)
    _only_colour_differs(base, got, method)
    left = np.any(_bits(base["color"]) != _bits(got["color"]), axis=-1)
    assert left.sum() > 20 and (_bits(got["color"])[left] == 0).all()
    lit = np.any(got["color"] > 0.0, axis=-1)
    assert lit.sum() > 20  # (the lamps still light the room)


@pytest.mark.parametrize("method", ["streaming", "megakernel"])
def test_another_map_between_frames(pkg, orc, method):
    """set, trace 2, set another (another size), trace 2: the restatement continued with prev="""
    scene, flat = _scene(pkg, "open")
    mega = method == "megakernel"
    render = loop_ref.render_megakernel if mega else loop_ref.render_streaming
    other = _env(n=12, seed=9, top=1.0)
    ref = render(orc, flat, scene.camera, W, H, 0, 2, 4, env=ENV)
    ref = render(orc, flat, scene.camera, W, H, 2, 2, 4, env=other, prev=ref)
    with _tracer(pkg, flat, mb=4, method=pkg.GPUMethod.megakernel if mega else None) as pt:
        pt.max_iterations = 4
        for env in (ENV, other):
            pt.environment = env
            pt.path_trace(scene.camera)
            pt.path_trace(scene.camera)
        _colour_is(_result(pt), ref, method)


def test_removal_equals_a_context_that_never_had_one(pkg, orc):
    scene, flat = _scene(pkg, "open")
    with _tracer(pkg, flat) as pt:
        never = _run(pt, scene.camera, None)
    with _tracer(pkg, flat) as pt:
        _run(pt, scene.camera, ENV, iters=1)
        after = _run(pt, scene.camera, None)
        size = C.c_uint32(99)
        assert pt._lib.ptc_get_environment(pt._ctx, C.byref(size)) == 0 and size.value == 0
        assert pt._lib.ptc_sample_environment(pt._ctx, None, 0, None) == pkg._capi.PTC_ERR_INVALID
    for p in PLANES:
        assert np.array_equal(_bits(never[p]), _bits(after[p])), p
    assert never["rays"] == after["rays"] and never["last_live"] == after["last_live"]
    ref = loop_ref.render_streaming(orc, flat, scene.camera, W, H, 0, ITERS, 8)
    _colour_is(after, ref, "removed")


def test_the_map_survives_upload_and_resize(pkg, orc):
    scene, flat = _scene(pkg, "open")
    with _tracer(pkg, flat, w=16, h=12, mb=4) as pt:
        pt.environment = ENV
        pt.max_iterations = 1
        pt.path_trace(scene.camera)
        pt.create_buffers((W, H), flat)  # ptc_upload_scene + ptc_resize
        got = _run(pt, scene.camera, ENV)
    _colour_is(got, _ref_streaming(orc, flat, scene.camera, W, H, 4), "after upload and resize")


# ---- 6. the refusals --------------------------------------------------------------------------------------------------------------
def test_the_refusals_leave_the_map_in_place(pkg):
    _, flat = _scene(pkg, "open")
    invalid = pkg._capi.PTC_ERR_INVALID
    dirs = env_ref.direction_set(np.random.default_rng(1), 7, count=256)
    want = env_ref.lookup(ENV, dirs)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with _tracer(pkg, flat) as pt:
        assert pt._lib.ptc_sample_environment(pt._ctx, p(dirs), len(dirs), p(np.empty_like(dirs))) == invalid
        assert "no environment" in pt._lib.ptc_last_error(pt._ctx).decode()
        pt.environment = ENV
        assert np.array_equal(_bits(pt.sample_environment(dirs)), _bits(want))
        for n in (1, 4097):
            assert pt._lib.ptc_set_environment(pt._ctx, p(ENV), n) == invalid
            assert str(n) in pt._lib.ptc_last_error(pt._ctx).decode()
        for bad, says in ((np.nan, "nan"), (np.inf, "inf"), (-0.5, "-0.5")):
            e = _env(n=4, seed=2)
            e[2, 1, 1] = bad
            assert pt._lib.ptc_set_environment(pt._ctx, p(e), 4) == invalid
            text = pt._lib.ptc_last_error(pt._ctx).decode()
            assert "row 2" in text and "column 1" in text and "component 1" in text and says in text, text
        size = C.c_uint32(0)
        assert pt._lib.ptc_get_environment(pt._ctx, C.byref(size)) == 0 and size.value == 7
        assert np.array_equal(_bits(pt.sample_environment(dirs)), _bits(want))  # the old map, still


# ---- 7. denoise and present -----------------------------------------------------------------------------------------------------
def test_denoise_and_present_of_an_environment_frame(pkg, orc):
    """ptc_denoise and send_to_preview on a frame with an environment agree with orc_denoise / orc_preview on the same planes within
    the tolerances of tests/test_gpu_denoise.py (1e-5 relative to the map's scale of 3, 1 LSB)"""
    scene, flat = _scene(pkg, "open")
    with _tracer(pkg, flat) as pt:
        pt.environment = ENV
        pt.max_iterations = 2
        for _ in range(2):
            pt.path_trace(scene.camera)
        g = {k: pt.download(k) for k in PLANES}
        pt.denoise()
        out = pt.download("final")
        rgba = pt.send_to_preview()
    want, _ = orc.denoise(scene.camera, W, H, g["color"], g["normal"], g["depth"], 10)
    assert np.isfinite(want).all() and np.isfinite(out).all()
    assert float(np.max(np.abs(out.astype(np.float64) - want.astype(np.float64)))) <= 3e-5
    want_rgba = orc.preview(want, W, H, 0)
    assert np.all(rgba[..., 3] == 255)
    assert int(np.abs(rgba[..., :3].astype(np.int32) - want_rgba[..., :3].astype(np.int32)).max()) <= 1


# ---- 8. the command line ----------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("extra", [[], ["--method", "megakernel"], ["--gpus", "2"]])
def test_hip_pt_environment_equals_the_python_tracer(pkg, tmp_path, extra):
    """hip_pt --environment FILE --environment-scale S --environment-size N --dump-raw on a scene without the key, and the asset scene
    that has it: the float framebuffers are the Python PathTracer's with the same map"""
    if not os.path.exists(HIP_PT):
        subprocess.run(["make"], cwd=os.path.dirname(HIP_PT), check=True, stdout=subprocess.DEVNULL)
    sky = os.path.join(ROOT, "tests", "golden", "environment", "sky_dusk.hdr")
    spp, mb = 2, 4
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for scene_file, args, size, scale in (("cornell_spheres.json", ["--environment", sky, "--environment-scale", "0.5", "--environment-size", "20"], 20, 0.5),
                                          ("spheres_sky.json", [], 64, 1.0)):
        scene = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", scene_file))
        w, h = scene.resolution
        env_map = pkg.hdr.environment_from_equirect(pkg.hdr.read_hdr(sky), size, scale)
        if not args:
            assert np.array_equal(_bits(env_map), _bits(scene.environment))
        flat = scene.build_scene()
        mega = "megakernel" in extra
        want = {}
        if "--gpus" in extra:  # rows dealt in blocks of 8 over two ranks, paths numbered per rank (hip_pt's run_ranks)
            parts = {p: [] for p in PLANES}
            for rank in (0, 1):
                with _tracer(pkg, flat, w=w, h=h, mb=mb, interleave=(rank, 2, 8)) as pt:
                    pt.environment = env_map
                    pt.max_iterations = spp
                    for _ in range(spp):
                        pt.path_trace(scene.camera)
                    for p in PLANES:
                        parts[p].append(pt.download(p))
            want = {p: pkg.bands.assemble_interleaved(parts[p], h, 2, 8) for p in PLANES}
        else:
            with _tracer(pkg, flat, w=w, h=h, mb=mb, method=pkg.GPUMethod.megakernel if mega else None) as pt:
                pt.environment = env_map
                pt.max_iterations = spp
                for _ in range(spp):
                    pt.path_trace(scene.camera)
                want = {p: pt.download(p) for p in PLANES}
        raw = tmp_path / "out.raw"
        cmd = [HIP_PT, "scenes/" + scene_file, "-o", str(tmp_path / "out.png"), "--spp", str(spp), "--max-bounces", str(mb), "--dump-raw", str(raw)] + args + extra
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        got = _read_raw(raw)
        for p in PLANES:
            assert np.array_equal(_bits(got[p]), _bits(np.asarray(want[p]).reshape(got[p].shape))), (scene_file, extra, p)
