"""The denoiser's albedo factorisation on the GPU (ptc_set_param "denoise_albedo", ptc_denoise_albedo, ptc_get_denoise_albedo_stats;
k_denoise_albedo, k_remodulate).

The plane against the queries that exist already, bit for bit: the rays ptc_denoise_albedo built go to ptc_hit_surface (the albedo) and
ptc_intersect_rays (the material), and the plane must be the former where the latter says diffuse or metal, ones elsewhere.  Under
"textures" 0 the kernel gets no textures, so what ptc_hit_surface reports "there" is a context's in which none are set.  The irradiance
against tests/demodulate_ref.py, bit for bit; ptc_denoise under the parameter against the float64 restatement (demodulate,
tests/denoise_ref.py, remodulate) within 1e-5 x max(1, M), M the largest irradiance it filters; 0 against a context that never heard of
the parameter; one scene in which the factorisation has to show; the planes' lifetime; the refusals.

Frames of 65 x 33 and 101 x 67 (no multiple of the kernel's 8 x 8 tile, of the passes' 16 and 64) and 2 x 2."""
import ctypes as C
import os

import numpy as np
import pytest

import demodulate_ref as dm
import denoise_ref as dr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXTURES = os.path.join(ROOT, "tests", "golden", "textures")
SIZES = [(65, 33), (101, 67), (2, 2)]
NO_TRIANGLE = 0xFFFFFFFF
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _textured_scene(pkg):
    """the UV box twice -- diffuse under checker.png, metal under stripes.png --, a glass sphere, an emitter, a floor whose red lies
    under the albedo floor, and open sky"""
    if "textured" not in _cache:
        glm = pkg.glmlite
        s = pkg.SceneDescription()
        s.add_material("floor", pkg.DiffuseMateral((0.01, 0.4, 0.7)))
        s.add_material("box", pkg.DiffuseMateral((0.8, 0.8, 0.5), pkg.TextureSource(os.path.join(TEXTURES, "checker.png"))))
        s.add_material("box2", pkg.MetalMaterial((0.9, 0.9, 0.9), 0.1,
                                                 pkg.TextureSource(os.path.join(TEXTURES, "stripes.png"), "linear", "nearest", "clamp")))
        s.add_material("glass", pkg.DielectricMaterial(1.5))
        s.add_material("lamp", pkg.EmissiveMaterial((4.0, 4.0, 4.0)))
        path = os.path.join(ROOT, "assets", "models", "box_uv.obj")
        mesh = s.add_mesh(path, pkg.json_parser.load_obj(path))
        s.add_object(pkg.Sphere((0, 0, 0), 1000.0), glm.translate((0.0, -1001.0, 0.0)), "floor")
        s.add_object(mesh, glm.compose([glm.rotate(np.radians(30.0), (0, 1, 0)), glm.translate((0.9, -0.5, -0.4))]), "box")
        s.add_object(mesh, glm.compose([glm.scale(0.6), glm.rotate(np.radians(-25.0), (0.2, 1, 0)), glm.translate((-0.9, -0.7, 0.3))]), "box2")
        s.add_object(pkg.Sphere((0, 0, 0), 0.3), glm.translate((0.0, -0.7, 0.9)), "glass")
        s.add_object(pkg.Sphere((0, 0, 0), 0.25), glm.translate((0.0, 0.6, 0.0)), "lamp")
        s.camera = pkg.scenes._camera_from_look_at((0.0, 0.2, 4.0), (0.0, -0.4, 0.0), vfov_deg=45.0)
        _cache["textured"] = (s, s.build_scene())
    return _cache["textured"]


def _heightfield(pkg):
    if "heightfield" not in _cache:
        s = pkg.scenes.heightfield_scene((65, 33), nx=257, nz=129)
        _cache["heightfield"] = (s, s.build_scene())
    return _cache["heightfield"]


def _traced(pkg, which, w, h, textures=True, load=True):
    """a context holding a short render (4 bounces, 2 iterations) of one of the two scenes -> (pt, camera, flat)"""
    scene, flat = _textured_scene(pkg) if which == "textured" else _heightfield(pkg)
    camera = scene.camera if which == "textured" else dr.low_camera(pkg)
    pt = pkg.PathTracer(max_bounces=4)
    pt.set_param("frames_in_flight", 1)
    if which == "textured":
        pt.current_gpu_method = pkg.GPUMethod.megakernel
        pt.textures = textures
    pt.create_buffers((w, h), flat)
    if which == "textured" and load:
        pt.load_scene_textures(flat)
    _trace(pt, camera)
    return pt, camera, flat


def _trace(pt, camera, iterations=2):
    pt.restart()
    pt.max_iterations = iterations
    for _ in range(iterations):
        pt.path_trace(camera)


def _check_plane(pkg, pt, flat, w, h, surface_of=None, what=""):
    """ptc_denoise_albedo's three arrays and the stage's counters against ptc_hit_surface, ptc_hit_attributes and ptc_intersect_rays on
    the rays it returns.  surface_of: the context whose ptc_hit_surface says what the kernel's textures give (default: pt itself).
    -> the arrays"""
    out = pt.denoise_albedo()
    stats = pt.denoise_albedo_stats()
    rays = out["rays"]
    assert rays.shape == (w * h, 8) and out["albedo"].shape == (h, w, 3)
    t, _, mat, _ = pt.intersect_rays(rays)
    hs = (surface_of or pt).hit_surface(rays)
    tri = pt.hit_attributes(rays)["triangle"]
    types = np.asarray(flat.materials)["type"]
    hit = t >= 0
    surface = hit & (types[np.where(hit, mat, 0)] <= 1)
    want = np.where(surface[:, None], hs["albedo"], np.float32(1.0)).astype(np.float32)
    got = out["albedo"].reshape(-1, 3)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist(), got[bad[:4, 0]].tolist(), want[bad[:4, 0]].tolist())
    assert stats["pixels"] == w * h and stats["surface_hits"] == int(surface.sum()), (what, stats, int(surface.sum()))
    looked = np.zeros(w * h, dtype=bool)
    tex = (surface_of or pt).texture_table
    if tex is not None and (surface_of or pt).texcoords is not None:
        bound = np.asarray(tex[1])[np.where(hit, mat, 0)] >= 0
        looked = surface & (tri != NO_TRIANGLE) & bound & np.isfinite(hs["st"]).all(axis=1)
    assert stats["texel_lookups"] == int(looked.sum()), (what, stats, int(looked.sum()))
    with np.errstate(invalid="ignore"):
        assert stats["floored"] == int((~(got > dm.ALBEDO_FLOOR)).sum()), (what, stats)
    return out, dict(surface=surface, hit=hit, looked=looked, stats=stats)


# ---- 1. the plane, the rays, the irradiance ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_plane_on_the_textured_scene(pkg, orc, w, h):
    """"textures" 1: the texel where the rule applies; "textures" 0: the material's colour, as a context without textures reports it"""
    pt, camera, flat = _traced(pkg, "textured", w, h)
    plain, _, _ = _traced(pkg, "textured", w, h, textures=False, load=False)
    with pt, plain:
        out, seen = _check_plane(pkg, pt, flat, w, h, what="textures 1")
        if (w, h) != (2, 2):  # every kind of pixel is in the frame: both boxes' texels, the floor, glass, the lamp, the sky
            assert seen["looked"].sum() > 50 and (~seen["hit"]).sum() > 50 and (seen["hit"] & ~seen["surface"]).sum() > 10
            assert seen["stats"]["floored"] > 50 and (seen["surface"] & ~seen["looked"]).sum() > 50
        _check_rays(pkg, orc, out["rays"], camera, w, h)
        _check_irradiance(pt, out)
        pt.textures = False
        off, seen_off = _check_plane(pkg, pt, flat, w, h, surface_of=plain, what="textures 0")
        assert seen_off["stats"]["texel_lookups"] == 0
        if (w, h) != (2, 2):
            assert not np.array_equal(off["albedo"], out["albedo"])
        _check_irradiance(pt, off)


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_plane_on_the_heightfield(pkg, orc, w, h):
    pt, camera, flat = _traced(pkg, "heightfield", w, h)
    with pt:
        for textures in (1, 0):
            pt.set_param("textures", textures)
            out, seen = _check_plane(pkg, pt, flat, w, h, what=f"textures {textures}")
            assert seen["stats"]["texel_lookups"] == 0
        _check_rays(pkg, orc, out["rays"], camera, w, h)
        _check_irradiance(pt, out)


def _check_rays(pkg, orc, rays, camera, w, h):
    """pixel-centre view rays: directions within 1e-6 of the float64 restatement (about ten binary32 roundings on unit-size values), the
    origin the camera's position, a primary ray's t_min and no t_max"""
    matrix, vfov = dr.gpu_camera(orc, camera, w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    origin, dirs = dr.view_rays(matrix, vfov, w, h, xs + 0.5, ys + 0.5)
    err = float(np.max(np.abs(rays[:, 4:7].astype(np.float64) - dirs.reshape(-1, 3))))
    assert err <= 1e-6, err
    assert np.array_equal(rays[:, 0:3], np.broadcast_to(np.asarray(camera.position, dtype=np.float32), (w * h, 3)))
    assert np.all(rays[:, 0:3] == origin.astype(np.float32))
    assert np.all(rays[:, 3] == np.float32(1e-4)) and np.all(np.isposinf(rays[:, 7]))


def _check_irradiance(pt, out):
    colour = pt.download("color")
    want, _ = dm.demodulate(colour, out["albedo"])
    assert np.array_equal(_bits(out["irradiance"]), _bits(want))


# ---- 2. ptc_denoise under the parameter -------------------------------------------------------------------------------------------------
def _denoise(pt, fs, weights, variant):
    d = pt.atrous_denoiser
    d.filter_size = fs
    d.color_weight, d.normal_weight, d.position_weight = weights
    pt.set_param("denoise_variant", variant)
    pt.denoise()
    return pt.download("final")


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("which", ["textured", "heightfield"])
def test_denoise_end_to_end(pkg, orc, which, w, h):
    """filter sizes 1, 3, 16, 100 x the default weights and a mixed set x both variants against demodulated_denoise in float64 on the
    downloaded colour, normal, depth and the plane the tests above verify.  Tolerance 1e-5 x max(1, M): 1e-5 is what test_gpu_denoise.py
    allows on radiance of order 1, and a binary32 filter's absolute error scales with the magnitude it filters, M = the largest finite
    irradiance."""
    pt, camera, flat = _traced(pkg, which, w, h)
    with pt:
        g = {k: pt.download(k) for k in ("color", "normal", "depth")}
        albedo = pt.denoise_albedo()["albedo"]
        irr = dm.irradiance_f64(g["color"], albedo)
        M = float(np.max(irr[np.isfinite(irr)]))
        tol = 1e-5 * max(1.0, M)
        print(f"{which} {w}x{h}: M = {M:.6g}")
        pt.set_profiling(time_trace_kernel=True)
        pt.set_param("denoise_albedo", 1)
        passes = pt.profile()["denoise_passes"]
        for weights in (dr.DEFAULT_WEIGHTS, (0.2, 0.8, 0.05)):
            for fs in (1, 3, 16, 100):
                want = dm.demodulated_denoise(orc, camera, w, h, g["color"], albedo, g["normal"], g["depth"], fs, *weights)
                for variant in (0, 1):
                    what = (which, w, h, fs, weights, variant, "M", M)
                    got = _denoise(pt, fs, weights, variant)
                    now = pt.profile()["denoise_passes"]
                    assert now - passes == dr.passes_of(fs), what
                    passes = now
                    nan_got, nan_want = np.isnan(got).any(axis=-1), np.isnan(want).any(axis=-1)
                    assert np.array_equal(nan_got, nan_want), (what, int(nan_got.sum()), int(nan_want.sum()))
                    err = float(np.max(np.abs(got[~nan_want].astype(np.float64) - want[~nan_want]))) if (~nan_want).any() else 0.0
                    assert err <= tol, (what, err, tol)
        stats = pt.denoise_albedo_stats()
        assert stats["pixels"] == w * h and stats["stage_ms"] > 0.0
        pt.restart()
        assert pt.denoise_albedo_stats()["stage_ms"] == 0.0


def test_off_is_off(pkg):
    """0 is what a context that never heard of the parameter computes, before and after a 1; filter_size 0 under 1 runs no stage"""
    w, h = 65, 33
    never, _, _ = _traced(pkg, "textured", w, h)
    pt, _, _ = _traced(pkg, "textured", w, h)
    with never, pt:
        pt.set_profiling(time_trace_kernel=True)
        for variant in (0, 1):
            want = _denoise(never, 10, dr.DEFAULT_WEIGHTS, variant)
            pt.set_param("denoise_albedo", 0)
            assert np.array_equal(_denoise(pt, 10, dr.DEFAULT_WEIGHTS, variant), want)
            pt.set_param("denoise_albedo", 1)
            on = _denoise(pt, 10, dr.DEFAULT_WEIGHTS, variant)
            assert not np.array_equal(on, want)
            before, passes = pt.denoise_albedo_stats(), pt.profile()["denoise_passes"]
            assert before["pixels"] == w * h
            pt.denoise_albedo()
            assert np.array_equal(pt.download("final"), on)  # (the query leaves the final buffer alone)
            # no pass, no stage: the counters of a smaller frame's call would differ -- here the stage's time must not move
            for fs in (0, -1):
                pt.atrous_denoiser.filter_size = fs
                pt.denoise()
            after = pt.denoise_albedo_stats()
            assert after["pixels"] == before["pixels"] and pt.profile()["denoise_passes"] == passes
            pt.set_param("denoise_albedo", 0)
            assert np.array_equal(_denoise(pt, 10, dr.DEFAULT_WEIGHTS, variant), want)
        assert never.denoise_albedo_stats() == {"pixels": 0, "surface_hits": 0, "texel_lookups": 0, "floored": 0, "stage_ms": 0.0}


def test_no_stage_without_a_pass(pkg):
    """filter_size 0 under the parameter, in a context whose stage has never run: the counters stay zero"""
    pt, _, _ = _traced(pkg, "heightfield", 65, 33)
    with pt:
        pt.set_param("denoise_albedo", 1)
        pt.atrous_denoiser.filter_size = 0
        pt.denoise()
        assert pt.denoise_albedo_stats()["pixels"] == 0
        pt.atrous_denoiser.filter_size = 1
        pt.denoise()
        assert pt.denoise_albedo_stats()["pixels"] == 65 * 33


# ---- 3. what it is for -------------------------------------------------------------------------------------------------------------------
def test_a_checker_survives_the_filter(pkg):
    """One quad filling a 64 x 64 frame under checker8.png (0.2 / 0.8, nearest), lit by a constant environment L alone, max_bounces 2:
    every path is quad -> sky, so the accumulated colour of a pixel inside a texel is albedo x L.  On those pixels (at least 40 % of
    the frame) the denoised image is closer to the colour under the parameter than without it, at filter size 16."""
    w = h = 64
    L = np.array([1.0, 0.5, 0.25], dtype=np.float32)
    s = pkg.SceneDescription()
    s.add_material("wall", pkg.DiffuseMateral((1.0, 1.0, 1.0), pkg.TextureSource(os.path.join(TEXTURES, "checker8.png"), "linear", "nearest", "clamp")))
    positions = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], dtype=np.float32)
    st = np.array([[0, 0], [1, 0], [1, 1], [0, 0], [1, 1], [0, 1]], dtype=np.float32)
    mesh = s.add_mesh("quad", pkg.Mesh(positions, np.array([0, 1, 2, 0, 2, 3], dtype=np.uint32), texcoords=st))
    s.add_object(mesh, pkg.glmlite.identity(), "wall")
    camera = pkg.scenes._camera_from_look_at((0.0, 0.0, 2.0), (0.0, 0.0, 0.0), vfov_deg=45.0)  # (the frame sees |x|, |y| <= 0.83 of the quad)
    flat = s.build_scene()
    with pkg.PathTracer(max_bounces=2) as pt:
        pt.set_param("frames_in_flight", 1)
        pt.current_gpu_method = pkg.GPUMethod.megakernel
        pt.textures = True
        pt.environment = np.broadcast_to(L, (4, 4, 3))
        pt.create_buffers((w, h), flat)
        pt.load_scene_textures(flat)
        _trace(pt, camera, iterations=4)
        colour = pt.download("color")
        out = pt.denoise_albedo()
        stats = pt.denoise_albedo_stats()
        assert stats["surface_hits"] == w * h == stats["texel_lookups"] and stats["floored"] == 0
        assert set(np.unique(out["albedo"]).tolist()) == {float(np.float32(51) / np.float32(255)), float(np.float32(204) / np.float32(255))}
        inside = np.all(np.abs(colour.astype(np.float64) - out["albedo"].astype(np.float64) * L) <= 1e-6, axis=-1)
        share = float(inside.mean())
        assert share >= 0.40, share
        means = {}
        for on in (0, 1):
            pt.set_param("denoise_albedo", on)
            den = _denoise(pt, 16, dr.DEFAULT_WEIGHTS, 0)
            means[on] = float(np.mean(np.abs(den[inside].astype(np.float64) - colour[inside])))
        print(f"texel interiors {share:.3f} of the frame; mean |denoised - colour| there: {means[0]:.6f} without, {means[1]:.6f} with")
        assert means[1] < means[0], means


# ---- 4. lifetime and refusals ------------------------------------------------------------------------------------------------------------
def test_planes_follow_the_frame_and_the_scene(pkg):
    """ptc_resize, ptc_upload_scene of a scene without textures and ptc_set_textures(NULL) between two denoise calls: the plane is the
    new state's every time"""
    pt, camera, flat = _traced(pkg, "textured", 65, 33)
    _, hflat = _heightfield(pkg)
    with pt:
        pt.set_param("denoise_albedo", 1)
        _denoise(pt, 3, dr.DEFAULT_WEIGHTS, 0)
        first, _ = _check_plane(pkg, pt, flat, 65, 33, what="before")
        pt.resize_image((101, 67))
        _trace(pt, camera)
        _denoise(pt, 3, dr.DEFAULT_WEIGHTS, 0)
        assert pt.denoise_albedo_stats()["pixels"] == 101 * 67
        _, seen = _check_plane(pkg, pt, flat, 101, 67, what="resized")
        assert seen["looked"].sum() > 50
        pt.texture_table = None  # (the frame stays: no new trace)
        _denoise(pt, 3, dr.DEFAULT_WEIGHTS, 0)
        assert pt.denoise_albedo_stats()["texel_lookups"] == 0
        _, seen = _check_plane(pkg, pt, flat, 101, 67, what="textures removed")
        assert not seen["looked"].any()
        pt.current_gpu_method = pkg.GPUMethod.streaming
        pt.textures = False
        pt.create_buffers((65, 33), hflat)
        _trace(pt, dr.low_camera(pkg))
        out = _denoise(pt, 3, dr.DEFAULT_WEIGHTS, 0)
        assert np.isfinite(out).all()
        _check_plane(pkg, pt, hflat, 65, 33, what="another scene")


def test_refusals_leave_the_frame(pkg):
    w, h = 65, 33
    scene, flat = _heightfield(pkg)
    with pkg.PathTracer(max_bounces=4) as pt:
        for bad in (-1, 2):
            with pytest.raises(pkg._capi.PtcError) as e:
                pt.set_param("denoise_albedo", bad)
            assert e.value.code == pkg._capi.PTC_ERR_INVALID and "denoise_albedo must be 0 or 1" in str(e.value)
        for good in (1, 0, 1):
            pt.set_param("denoise_albedo", good)
        pt.set_param("frames_in_flight", 1)
        pt.create_buffers((w, h), flat)
        for call in (pt.denoise_albedo, pt.denoise):
            with pytest.raises(pkg._capi.PtcError) as e:  # no traced frame
                call()
            assert e.value.code == pkg._capi.PTC_ERR_INVALID and "denoise needs a traced frame" in str(e.value)
            assert "traced frame" in pt._lib.ptc_last_error(pt._ctx).decode()
        _trace(pt, dr.low_camera(pkg))
        whole = pt.download("color")
        out = pt.denoise_albedo()
        pt.set_rows(0, 16)  # a band: the context no longer owns the whole frame
        for call in (pt.denoise_albedo, pt.denoise):
            with pytest.raises(pkg._capi.PtcError) as e:
                call()
            assert e.value.code == pkg._capi.PTC_ERR_INVALID and "full frame in one context" in str(e.value)
        buf = np.full(3, 7.0, dtype=np.float32)
        assert pt._lib.ptc_denoise_albedo(pt._ctx, buf.ctypes.data_as(C.c_void_p), None, None) == pkg._capi.PTC_ERR_INVALID
        assert np.all(buf == 7.0) and "full frame" in pt._lib.ptc_last_error(pt._ctx).decode()
        pt.set_rows(0, h)
        assert np.array_equal(pt.download("color"), whole)  # the context renders the same frame
        again = pt.denoise_albedo()
        for k in out:
            assert np.array_equal(_bits(again[k]), _bits(out[k])), k
        # each output is optional
        alb = np.zeros((h, w, 3), dtype=np.float32)
        assert pt._lib.ptc_denoise_albedo(pt._ctx, alb.ctypes.data_as(C.c_void_p), None, None) == 0
        assert np.array_equal(alb, out["albedo"])
        assert pt._lib.ptc_denoise_albedo(pt._ctx, None, None, None) == 0
