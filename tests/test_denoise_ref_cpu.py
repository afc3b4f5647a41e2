"""The float64 restatement of the A-Trous denoiser (tests/denoise_ref.py) against the CPU oracle (orc_denoise), on every
pixel -- the out-of-bounds taps of the bottom row and right column included -- over the whole parameter range the
reference's GUI reaches (filter size 1-100, each weight 0-1) and one filter size past it.  Two independent statements of
the reference agreeing within 2e-6 is what lets tests/test_gpu_denoise.py hold the HIP kernels to both of them."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_ref as dr

TOL = 2e-6
# Past the GUI's filter sizes: the eighth pass (step 128) at the ill-conditioned end of the weights (all at 0.01, every
# exponent scaled by 100) carries the binary32 rounding of seven passes before it -- 2.1e-6 at one pixel of 3x130,
# against 1.9e-6 after seven passes.  That is the reference's own arithmetic, not a disagreement of substance: a
# misplaced tap or weight moves a pixel by 1e-3 and more (tests/test_gpu_denoise.py).
TOL_PAST_GUI = 3e-6

# (camera, w, h): oracle-rendered G-buffers of the heightfield scene (2 iterations, 4 bounces); "golden" is the
# 64x64 input of tests/golden/frames.npz.  2x2 is the smallest frame; 3x130 and 130x3 are thinner than one step.
CASES = [("golden", 64, 64), ("own", 101, 67), ("low", 101, 67), ("low", 65, 33), ("low", 3, 130), ("low", 130, 3),
         ("low", 2, 2)]


def _inputs(pkg, orc, golden_dir, cam, w, h):
    if cam == "golden":
        f = np.load(os.path.join(golden_dir, "frames.npz"))
        scene = pkg.scenes.heightfield_scene((64, 64), nx=33, nz=17)
        return scene.camera, f["denoise_in_color"], f["denoise_in_normal"], f["denoise_in_depth"]
    scene = pkg.scenes.heightfield_scene((w, h), nx=257, nz=129)
    camera = dr.low_camera(pkg) if cam == "low" else scene.camera
    r = orc.render_streaming(scene.build_scene(), camera, w, h, 0, 2, 4)
    return camera, r["color"], r["normal"], r["depth"]


def assert_same(got, want, tol, what):
    """every pixel: the same NaN positions, |got - want| <= tol elsewhere"""
    nan_got, nan_want = np.isnan(got).any(axis=-1), np.isnan(want).any(axis=-1)
    assert np.array_equal(nan_got, nan_want), (what, int(nan_got.sum()), int(nan_want.sum()))
    ok = ~nan_want
    if ok.any():
        err = float(np.max(np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64))))
        assert err <= tol, (what, err)


@pytest.mark.parametrize("cam,w,h", CASES, ids=[f"{c}-{w}x{h}" for c, w, h in CASES])
def test_restatement_against_oracle(pkg, orc, golden_dir, cam, w, h):
    camera, color, normal, depth = _inputs(pkg, orc, golden_dir, cam, w, h)
    assert np.isfinite(color).all() and np.isfinite(depth).all()
    for weights in dr.WEIGHT_SETS:
        chain = dr.denoise_chain(orc, camera, w, h, color, normal, depth, dr.passes_of(max(dr.FILTER_SIZES)), *weights)
        for fs in dr.FILTER_SIZES:
            want, _ = orc.denoise(camera, w, h, color, normal, depth, fs, *weights)
            got = chain[dr.passes_of(fs) - 1]
            assert_same(got, want, TOL if fs <= 100 else TOL_PAST_GUI, (fs, weights))
            if 0.0 in weights:
                assert np.isnan(want).all(), (fs, weights)     # -0/0 at the centre tap of every pixel
            else:
                assert np.isfinite(want).all(), (fs, weights)
        assert np.array_equal(dr.denoise(orc, camera, w, h, color, normal, depth, 10, *weights), chain[3], equal_nan=True)


def test_no_pass_below_filter_size_one(pkg, orc, golden_dir):
    """filter_size < 1: the loop never runs; the reference returns its front buffer unwritten (the oracle says -1)"""
    camera, color, normal, depth = _inputs(pkg, orc, golden_dir, "golden", 64, 64)
    assert dr.passes_of(0) == 0 and dr.passes_of(-1) == 0
    assert [dr.passes_of(fs) for fs in dr.FILTER_SIZES] == [1, 2, 2, 4, 5, 5, 6, 6, 7, 7, 8]
    for fs in (0, -1):
        assert dr.denoise(orc, camera, 64, 64, color, normal, depth, fs) is None
        a = np.zeros((64, 64, 3), dtype=np.float32)
        b = np.zeros((64, 64, 3), dtype=np.float32)
        c = np.ascontiguousarray(color, dtype=np.float32)
        n = np.ascontiguousarray(normal, dtype=np.float32)
        d = np.ascontiguousarray(depth, dtype=np.float32)
        which = orc.lib().orc_denoise(C.byref(orc.camera_c(camera)), 64, 64, c.ctypes.data, n.ctypes.data, d.ctypes.data,
                                      a.ctypes.data, b.ctypes.data, fs, 0.45, 0.30, 0.25, None, 0)
        assert which == -1 and not a.any() and not b.any()


def test_view_rays_against_oracle(pkg, orc):
    """the float64 generate_ray against orc_generate_ray (binary32) on the border coordinates the taps use, column W
    and row H included"""
    w, h = 37, 23
    camera = dr.low_camera(pkg)
    matrix, vfov = dr.gpu_camera(orc, camera, w, h)
    g = orc.OGPUCamera()
    orc.lib().orc_to_gpu_camera(C.byref(orc.camera_c(camera)), w, h, C.byref(g))
    pts = [(u, v) for u in (0, 1, w - 1, w) for v in (0, 1, h - 1, h)] + [(17, 11)]
    origin, dirs = dr.view_rays(matrix, vfov, w, h, np.array([p[0] + 0.5 for p in pts]), np.array([p[1] + 0.5 for p in pts]))
    for (u, v), d in zip(pts, dirs):
        ray = orc.ORay()
        orc.lib().orc_generate_ray(C.byref(g), u + 0.5, v + 0.5, C.byref(ray))
        assert np.max(np.abs(np.array(ray.origin[:]) - origin)) <= 1e-6
        assert np.max(np.abs(np.array(ray.direction[:]) - d)) <= 1e-6, (u, v)


def test_preview_of_nan_is_black(orc):
    """color_float_to_255 of NaN is 0 (the cast of a NaN to an integer is undefined in C; the GPU's conversion gives 0)"""
    buf = np.array([[[np.nan, 0.5, np.nan], [np.nan, np.nan, np.nan]], [[1.0, np.inf, -1.0], [0.0, 2.0, 0.25]]],
                   dtype=np.float32)
    rgba = orc.preview(buf, 2, 2, 0)
    assert rgba[0, 0].tolist() == [0, 186, 0, 255]            # 0.5 ** (1 / 2.2) * 255.99 = 186.3
    assert rgba[0, 1].tolist() == [0, 0, 0, 255]
    assert rgba[1, 0].tolist() == [255, 255, 0, 255]            # powf(-1, 1 / 2.2) is NaN
    assert rgba[1, 1].tolist() == [0, 255, 136, 255]            # 0.25 ** (1 / 2.2) * 255.99 = 136.3
