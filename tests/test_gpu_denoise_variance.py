"""The variance-guided A-Trous mode on the GPU (ptc_set_param "denoise_variance", ptc_denoise_variance; k_variance_estimate,
k_variance_prefilter, k_denoise_var_lds<1..32>, k_denoise_var) against the float64 restatement
(tests/denoise_variance_ref.py) on rendered frames of the heightfield scene -- tests/test_gpu_denoise.py's recipe, whose sizes are no
multiple of the estimate's 32 x 8 tile, the passes' 64-wide LDS tile, the through-cache kernel's 16 x 16 tile or a step, exact tiles,
thinner than one step, and the smallest frame.

Tolerance: 1e-5 x max(1, M) on a colour and on a variance alike, M the largest value the filter sees (the accumulated
colour, or the irradiance under "denoise_albedo"): the project's bound for the denoiser.  The binary32 numpy restatement is measured
against the float64 one on every input and printed; where it is farther than the bound, four times its distance takes the bound's
place (denoise_variance_ref.tolerance).  Nothing here comes from the GPU's output."""
import ctypes as C

import numpy as np
import pytest

import demodulate_ref as dm
import denoise_ref as dr
import denoise_variance_ref as vr

pytestmark = pytest.mark.gpu

SIZES = [(65, 33), (101, 67), (64, 4), (130, 3), (3, 130), (2, 2)]
IDS = [f"{w}x{h}" for w, h in SIZES]


def _traced(pkg, w, h):
    """a context holding a short render (2 iterations, 4 bounces) of the heightfield scene from the low camera, and its G-buffer"""
    scene = pkg.scenes.heightfield_scene((w, h), nx=257, nz=129)
    camera = dr.low_camera(pkg)
    pt = pkg.PathTracer(max_bounces=4)
    pt.set_param("frames_in_flight", 1)
    pt.create_buffers((w, h), scene.build_scene())
    pt.max_iterations = 2
    for _ in range(2):
        pt.path_trace(camera)
    g = {k: pt.download(k) for k in ("color", "normal", "depth")}
    return pt, camera, g


def _denoise(pt, fs, n_phi, p_phi, variant, sigma=vr.DEFAULT_SIGMA, color_weight=0.45):
    d = pt.atrous_denoiser
    d.filter_size = fs
    d.color_weight, d.normal_weight, d.position_weight = color_weight, n_phi, p_phi
    pt.denoise_variance_sigma = sigma
    pt.set_param("denoise_variant", variant)
    pt.denoise()
    return pt.download("final")


def _plane(pt, g, albedo):
    """what the passes filter, in float64, its scale max(1, M), and the effective albedo the result is multiplied by (or None)"""
    if not albedo:
        plane, e = g["color"].astype(np.float64), None
    else:
        alb = pt.denoise_albedo()["albedo"]
        plane, e = dm.irradiance_f64(g["color"], alb), dm.effective_f64(alb)
    return plane, max(1.0, float(np.max(np.abs(plane[np.isfinite(plane)])))), e


@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_variance_planes(pkg, orc, w, h):
    """ptc_denoise_variance's two planes, two weight sets, on the colour and on the irradiance; each output optional"""
    pt, camera, g = _traced(pkg, w, h)
    with pt:
        for albedo in (0, 1):
            pt.set_param("denoise_albedo", albedo)
            plane, scale, _ = _plane(pt, g, albedo)
            for n_phi, p_phi in vr.WEIGHT_SETS:
                d = pt.atrous_denoiser
                d.normal_weight, d.position_weight = n_phi, p_phi
                got = pt.denoise_variance()
                f64 = vr.guided_chain(orc, camera, w, h, plane, g["normal"], g["depth"], 0, vr.DEFAULT_SIGMA, n_phi, p_phi)
                f32 = vr.guided_chain(orc, camera, w, h, plane, g["normal"], g["depth"], 0, vr.DEFAULT_SIGMA, n_phi, p_phi, dtype=np.float32)
                for k in ("variance", "prefiltered"):
                    d32 = float(np.abs(f32[k] - f64[k]).max())
                    print(f"{w}x{h} albedo {albedo} weights {n_phi},{p_phi} {k}: binary32 - float64 {d32:.2e} scale {scale:.3g}")
                    vr.assert_close(got[k], f64[k], vr.tolerance(scale, d32), (k, albedo, n_phi, p_phi))
                stats = pt.denoise_variance_stats()
                assert stats["pixels"] == w * h and 0 <= stats["floored"] <= w * h
        only = np.zeros((h, w), dtype=np.float32)
        assert pt._lib.ptc_denoise_variance(pt._ctx, None, only.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(only.view(np.uint32), got["prefiltered"].view(np.uint32))
        assert pt._lib.ptc_denoise_variance(pt._ctx, None, None) == 0


@pytest.mark.parametrize("albedo", [0, 1], ids=["colour", "irradiance"])
@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_denoise_end_to_end(pkg, orc, w, h, albedo):
    """filter sizes 1, 3, 16 and 100 (step 64: the through-cache kernel under either variant) x two weight sets x both variants
    against the restatement, the variants against each other, the pass count, the stage's counters"""
    pt, camera, g = _traced(pkg, w, h)
    with pt:
        pt.set_param("denoise_albedo", albedo)
        plane, scale, e = _plane(pt, g, albedo)
        pt.set_profiling(time_trace_kernel=True)
        pt.set_param("denoise_variance", 1)
        passes = pt.profile()["denoise_passes"]
        for n_phi, p_phi in vr.WEIGHT_SETS:
            n_pass = dr.passes_of(max(vr.FILTER_SIZES))
            f64 = vr.guided_chain(orc, camera, w, h, plane, g["normal"], g["depth"], n_pass, vr.DEFAULT_SIGMA, n_phi, p_phi)
            f32 = vr.guided_chain(orc, camera, w, h, plane, g["normal"], g["depth"], n_pass, vr.DEFAULT_SIGMA, n_phi, p_phi, dtype=np.float32)
            for fs in vr.FILTER_SIZES:
                k = dr.passes_of(fs) - 1
                want = f64["colour"][k] if e is None else f64["colour"][k] * e
                d32 = float(np.abs(f32["colour"][k] - f64["colour"][k]).max())
                tol = vr.tolerance(scale, d32)
                print(f"{w}x{h} albedo {albedo} weights {n_phi},{p_phi} filter {fs}: binary32 - float64 {d32:.2e} scale {scale:.3g} tol {tol:.2e}")
                outs = []
                for variant in (0, 1):
                    what = (fs, n_phi, p_phi, variant)
                    outs.append(_denoise(pt, fs, n_phi, p_phi, variant))
                    now = pt.profile()["denoise_passes"]
                    assert now - passes == dr.passes_of(fs), what
                    passes = now
                    vr.assert_close(outs[-1], want, tol, what)
                vr.assert_close(outs[0], outs[1], 2.0 * tol, ("variants", fs, n_phi, p_phi))
        stats = pt.denoise_variance_stats()
        assert stats["pixels"] == w * h and stats["stage_ms"] > 0.0
        pt.restart()
        assert pt.denoise_variance_stats()["stage_ms"] == 0.0


def test_sigma_and_colour_weight(pkg, orc):
    """sigma is read per call and changes the result as the restatement says; color_weight is not read"""
    w, h = 65, 33
    pt, camera, g = _traced(pkg, w, h)
    with pt:
        assert pt.denoise_variance_sigma == vr.DEFAULT_SIGMA
        pt.set_param("denoise_variance", 1)
        scale = max(1.0, float(np.abs(g["color"]).max()))
        outs = {}
        for sigma in vr.SIGMAS:
            outs[sigma] = _denoise(pt, 16, 0.30, 0.25, 0, sigma)
            assert pt.denoise_variance_sigma == sigma
            _, want = vr.guided(orc, camera, w, h, g["color"], g["normal"], g["depth"], 16, sigma)
            _, w32 = vr.guided(orc, camera, w, h, g["color"], g["normal"], g["depth"], 16, sigma, dtype=np.float32)
            vr.assert_close(outs[sigma], want, vr.tolerance(scale, float(np.abs(w32 - want).max())), sigma)
        assert not np.array_equal(outs[4.0], outs[16.0])
        for cw in (0.01, 0.0, float("nan")):
            assert np.array_equal(_denoise(pt, 16, 0.30, 0.25, 0, 16.0, color_weight=cw), outs[16.0]), cw


def test_a_frame_of_constant_colour(pkg):
    """the camera inside one emissive sphere: every pixel is the emitted radiance bit for bit, under normals and depths that vary.  The
    variance plane is all zero, every pixel's prefiltered variance is on the floor, and the result is the input bit for bit"""
    w, h = 101, 67
    le = (1.5, 0.75, 0.25)
    s = pkg.SceneDescription()
    s.add_material("lamp", pkg.EmissiveMaterial(le))
    s.add_object(pkg.Sphere((0, 0, 0), 10.0), pkg.glmlite.translate((0.0, 0.0, 0.0)), "lamp")
    camera = pkg.scenes._camera_from_look_at((2.0, 1.0, 3.0), (0.0, 0.0, -5.0), vfov_deg=60.0)
    with pkg.PathTracer(max_bounces=4) as pt:
        pt.set_param("frames_in_flight", 1)
        pt.create_buffers((w, h), s.build_scene())
        pt.max_iterations = 2
        for _ in range(2):
            pt.path_trace(camera)
        colour, depth = pt.download("color"), pt.download("depth")
        assert np.array_equal(colour.view(np.uint32), np.broadcast_to(np.array(le, dtype=np.float32), (h, w, 3)).view(np.uint32))
        assert float(depth.max() - depth.min()) > 1.0
        pt.set_param("denoise_variance", 1)
        for variant in (0, 1):
            for fs in vr.FILTER_SIZES:
                out = _denoise(pt, fs, 0.30, 0.25, variant)
                assert np.array_equal(out.view(np.uint32), colour.view(np.uint32)), (variant, fs)
                stats = pt.denoise_variance_stats()
                assert stats["pixels"] == w * h and stats["floored"] == w * h, (variant, fs, stats)
        planes = pt.denoise_variance()
        assert not planes["variance"].any() and not planes["prefiltered"].any()


def test_off_after_on_is_the_plain_denoiser(pkg):
    """0 after 1 is what a context that never heard of the parameter computes, and both modes run floor(log2 N) + 1 passes"""
    w, h = 101, 67
    never, _, _ = _traced(pkg, w, h)
    pt, _, _ = _traced(pkg, w, h)
    with never, pt:
        pt.set_profiling(time_trace_kernel=True)
        passes = pt.profile()["denoise_passes"]
        for fs in (3, 16, 100):
            for variant in (0, 1):
                want = _denoise(never, fs, 0.30, 0.25, variant)
                for mode in (1, 0):
                    pt.set_param("denoise_variance", mode)
                    got = _denoise(pt, fs, 0.30, 0.25, variant)
                    now = pt.profile()["denoise_passes"]
                    assert now - passes == dr.passes_of(fs), (fs, variant, mode)
                    passes = now
                    assert np.array_equal(got, want) == (mode == 0), (fs, variant, mode)


def test_parameters_take_effect_per_call(pkg):
    """denoising one traced frame twice with different parameters gives what a fresh context gives for the second set: nothing of the
    first call -- its step count, its weights, its sigma, a NaN result, its variance planes -- carries over"""
    w, h = 101, 67
    second = [(3, 0.8, 0.05, 4.0), (64, 0.30, 0.25, 16.0), (1, 0.01, 0.01, 8.0)]
    first = [(100, 1.0, 1.0, 16.0), (8, 0.0, 0.25, 8.0), (200, 0.30, 0.0, 4.0)]
    fresh = {}
    for fs, n_phi, p_phi, sigma in second:
        pt, _, _ = _traced(pkg, w, h)
        with pt:
            pt.set_param("denoise_variance", 1)
            for variant in (0, 1):
                fresh[fs, variant] = _denoise(pt, fs, n_phi, p_phi, variant, sigma)
    pt, _, _ = _traced(pkg, w, h)
    with pt:
        pt.set_param("denoise_variance", 1)
        for variant in (0, 1):
            for a, b in zip(first, second):
                _denoise(pt, a[0], a[1], a[2], variant, a[3])
                out = _denoise(pt, b[0], b[1], b[2], variant, b[3])
                assert np.isfinite(out).all()
                assert np.array_equal(out, fresh[b[0], variant]), (a, b, variant)


def test_refusals(pkg):
    w, h = 65, 33
    scene = pkg.scenes.heightfield_scene((w, h), nx=257, nz=129)
    with pkg.PathTracer(max_bounces=4) as pt:
        for bad in (-1, 2):
            with pytest.raises(pkg.PtcError) as e:
                pt.set_param("denoise_variance", bad)
            assert e.value.code == pkg._capi.PTC_ERR_INVALID
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(pkg.PtcError) as e:
                pt.denoise_variance_sigma = bad
            assert e.value.code == pkg._capi.PTC_ERR_INVALID and "sigma" in str(e.value)
            assert pt.denoise_variance_sigma == vr.DEFAULT_SIGMA  # the value set before stays
        pt.set_param("frames_in_flight", 1)
        pt.create_buffers((w, h), scene.build_scene())
        with pytest.raises(pkg.PtcError) as e:  # no traced frame
            pt.denoise_variance()
        assert e.value.code == pkg._capi.PTC_ERR_INVALID and "denoise needs a traced frame" in str(e.value)
        pt.max_iterations = 2
        for _ in range(2):
            pt.path_trace(dr.low_camera(pkg))
        out = pt.denoise_variance()
        pt.set_rows(0, 16)  # a band: the context no longer owns the whole frame
        buf = np.full(3, 7.0, dtype=np.float32)
        with pytest.raises(pkg.PtcError) as e:
            pt.denoise_variance()
        assert e.value.code == pkg._capi.PTC_ERR_INVALID and "full frame in one context" in str(e.value)
        assert pt._lib.ptc_denoise_variance(pt._ctx, buf.ctypes.data_as(C.c_void_p), None) == pkg._capi.PTC_ERR_INVALID
        assert np.all(buf == 7.0)
        pt.set_rows(0, h)
        again = pt.denoise_variance()
        for k in out:
            assert np.array_equal(again[k].view(np.uint32), out[k].view(np.uint32)), k
