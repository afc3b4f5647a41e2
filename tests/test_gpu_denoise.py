"""The A-Trous denoiser (k_denoise_positions, k_denoise_lds<1..32>, k_denoise; ptc_denoise's pass loop) over the whole
parameter range the reference's GUI reaches -- filter size 1-100, each weight 0-1 (interactive-app/gui.cpp:87-89) --
and one filter size past it, on every pixel.  The bottom row and the right column are compared too: the reference's
out-of-bounds taps (the inclusive clamp to [0, W] x [0, H], element W*H-1 past the end, the own view ray of a tap on
column W or row H) are a contract of this port, restated the same way by the CPU oracle and by the float64 restatement
(tests/denoise_ref.py, pinned to the oracle by tests/test_denoise_ref_cpu.py).

Per case: |GPU - oracle| <= 1e-5 and |GPU - float64| <= 1e-5 on the radiance, both kernel variants, which agree with
each other within 1e-5; NaN exactly where the oracle has it (every pixel for a zero weight: -0/0 at the centre tap);
the display of the result within 1 LSB of orc_preview with NaN shown as black; ptc_denoise running floor(log2 N) + 1
passes per call and none for filter_size < 1; parameters applied per call."""
import numpy as np
import pytest

import denoise_ref as dr

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _camera(pkg, scene, cam):
    return dr.low_camera(pkg) if cam == "low" else scene.camera


def _traced(pkg, w, h, cam):
    """a context holding a short render (2 iterations, 4 bounces) of the heightfield scene, and its G-buffer"""
    scene = pkg.scenes.heightfield_scene((w, h), nx=257, nz=129)
    camera = _camera(pkg, scene, cam)
    pt = pkg.PathTracer(max_bounces=4)
    pt.set_param("frames_in_flight", 1)
    pt.create_buffers((w, h), scene.build_scene())
    pt.max_iterations = 2
    for _ in range(2):
        pt.path_trace(camera)
    g = {k: pt.download(k) for k in ("color", "normal", "depth")}
    return pt, camera, g


def _denoise(pt, fs, weights, variant):
    d = pt.atrous_denoiser
    d.filter_size = fs
    d.color_weight, d.normal_weight, d.position_weight = weights
    pt.set_param("denoise_variant", variant)
    pt.denoise()
    return pt.download("final")


def assert_close(got, want, what):
    """every pixel: NaN in the same places, |got - want| <= TOL elsewhere"""
    nan_got, nan_want = np.isnan(got).any(axis=-1), np.isnan(want).any(axis=-1)
    assert np.array_equal(nan_got, nan_want), (what, int(nan_got.sum()), int(nan_want.sum()))
    ok = ~nan_want
    if ok.any():
        err = float(np.max(np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64))))
        assert err <= TOL, (what, err)


def assert_display(rgba, den, want_rgba, what):
    """send_to_preview (FINAL) of a denoised buffer: within 1 LSB of orc_preview on every pixel, opaque, NaN black"""
    assert np.all(rgba[..., 3] == 255), what
    diff = np.abs(rgba[..., :3].astype(np.int32) - want_rgba[..., :3].astype(np.int32))
    assert int(diff.max()) <= 1, (what, int(diff.max()))
    nan = np.isnan(den).any(axis=-1)
    assert not rgba[nan][:, :3].any(), what          # k_preview converts NaN to 0 (and so does the oracle)


# (camera, w, h).  "low": bottom rows and right column across the spheres (tests/denoise_ref.py); "own": the scene's
# camera.  257x129 / 101x67 / 65x33: no multiple of a 16x16 tile, a 64-wide LDS tile or a step; 64x4: exact tiles;
# 130x3 / 3x130: thinner than one step; 2x2: the smallest frame ptc_resize accepts.
CASES = [("low", 257, 129), ("low", 101, 67), ("own", 101, 67), ("low", 65, 33), ("own", 65, 33), ("low", 64, 4),
         ("low", 130, 3), ("low", 3, 130), ("low", 2, 2)]


@pytest.mark.parametrize("cam,w,h", CASES, ids=[f"{c}-{w}x{h}" for c, w, h in CASES])
def test_denoise_parameter_range(pkg, orc, cam, w, h):
    """every filter size x every weight set x both variants against the oracle and the float64 restatement"""
    pt, camera, g = _traced(pkg, w, h, cam)
    with pt:
        pt.set_profiling(time_trace_kernel=True)
        passes = pt.profile()["denoise_passes"]
        for weights in dr.WEIGHT_SETS:
            chain = dr.denoise_chain(orc, camera, w, h, g["color"], g["normal"], g["depth"], dr.passes_of(max(dr.FILTER_SIZES)),
                                     *weights)
            for fs in dr.FILTER_SIZES:
                want, _ = orc.denoise(camera, w, h, g["color"], g["normal"], g["depth"], fs, *weights)
                want_rgba = orc.preview(want, w, h, 0)
                if 0.0 in weights:
                    assert np.isnan(want).all(), (fs, weights)
                else:
                    assert np.isfinite(want).all(), (fs, weights)
                outs = []
                for variant in (0, 1):
                    what = (fs, weights, variant)
                    out = _denoise(pt, fs, weights, variant)
                    outs.append(out)
                    now = pt.profile()["denoise_passes"]
                    assert now - passes == dr.passes_of(fs), what
                    passes = now
                    assert_close(out, want, ("oracle",) + what)
                    assert_close(out, chain[dr.passes_of(fs) - 1], ("float64",) + what)
                    assert_display(pt.send_to_preview(), out, want_rgba, what)
                assert_close(outs[0], outs[1], ("variants", fs, weights))


@pytest.mark.parametrize("weights,fs", [(dr.DEFAULT_WEIGHTS, 10), ((0.2, 0.8, 0.05), 100)])
def test_denoise_full_hd(pkg, orc, weights, fs):
    """config 5's size on every pixel against the oracle, both variants (the float64 restatement stops at 257x129)"""
    w, h = 1920, 1080
    pt, camera, g = _traced(pkg, w, h, "low")
    with pt:
        outs = [_denoise(pt, fs, weights, variant) for variant in (0, 1)]
        rgba = pt.send_to_preview()
    want, _ = orc.denoise(camera, w, h, g["color"], g["normal"], g["depth"], fs, *weights)
    for variant, out in enumerate(outs):
        assert_close(out, want, (fs, weights, variant))
    assert_close(outs[0], outs[1], (fs, weights, "variants"))
    assert_display(rgba, outs[1], orc.preview(want, w, h, 0), (fs, weights))


def test_parameters_take_effect_per_call(pkg):
    """denoising one traced frame twice with different parameters gives what a fresh context gives for the second set
    (ptc_denoise reads the parameters of each call: nothing of the first call -- its step count, its weights, a NaN
    result -- carries over)"""
    w, h = 101, 67
    second = [(3, (0.2, 0.8, 0.05)), (64, dr.DEFAULT_WEIGHTS), (1, (0.01, 0.01, 0.01))]
    first = [(100, (1.0, 1.0, 1.0)), (8, (0.0, 0.30, 0.25)), (200, (0.45, 0.30, 0.0))]
    fresh = {}
    for fs, weights in second:
        pt, _, _ = _traced(pkg, w, h, "low")
        with pt:
            for variant in (0, 1):
                fresh[fs, variant] = _denoise(pt, fs, weights, variant)
    pt, _, _ = _traced(pkg, w, h, "low")
    with pt:
        for variant in (0, 1):
            for (fs0, w0), (fs, weights) in zip(first, second):
                _denoise(pt, fs0, w0, variant)
                out = _denoise(pt, fs, weights, variant)
                assert np.isfinite(out).all()
                assert np.array_equal(out, fresh[fs, variant]), (fs0, w0, fs, weights, variant)


def test_filter_size_below_one(pkg, orc):
    """filter_size 0 and -1: ptc_denoise returns PTC_OK and launches no pass (the reference's loop never runs; what
    `final` then shows is its unwritten front buffer, not asserted); the context stays usable"""
    w, h = 65, 33
    pt, camera, g = _traced(pkg, w, h, "low")
    with pt:
        pt.set_profiling(time_trace_kernel=True)
        before = pt.profile()["denoise_passes"]
        for fs in (0, -1):
            for variant in (0, 1):
                _denoise(pt, fs, dr.DEFAULT_WEIGHTS, variant)
                pt.send_to_preview()
        assert pt.profile()["denoise_passes"] == before
        out = _denoise(pt, 10, dr.DEFAULT_WEIGHTS, 0)
        assert pt.profile()["denoise_passes"] == before + 4
    want, _ = orc.denoise(camera, w, h, g["color"], g["normal"], g["depth"], 10)
    assert_close(out, want, "after filter_size < 1")
