"""The variance-guided A-Trous mode (ptc_set_param "denoise_variance") without a GPU: ptc_check_denoise_variance --
the whole mode on the host, from the per-tap functions of pt_denoise_variance.hpp, the header the kernels compile -- against the
float64 restatement (tests/denoise_variance_ref.py) on synthetic planes, the claim the mode was built on (a low-contrast edge under
noise comes out closer to the clean image than from the plain passes), and the rule's corners.

Tolerance: the project's bound for the denoiser, 1e-5 x max(1, M) on a colour and on a variance alike, M the largest
colour the filter sees; the binary32 numpy restatement is measured against the float64 one on the same planes and, were it farther
than the bound, four times its distance would take the bound's place (it is not: at most 2e-6 on these planes, section 5s)."""
import numpy as np
import pytest

import denoise_ref as dr
import denoise_variance_ref as vr

SIZES = [(2, 2), (3, 130), (130, 3), (64, 4), (65, 33)]


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_library_matches_restatement(pkg, orc, w, h):
    """the estimate and the result of every filter size, two weight sets"""
    cam = dr.low_camera(pkg)
    colour, normal, depth = vr.synthetic_planes(w, h, seed=7)
    scale = max(1.0, float(np.abs(colour).max()))
    for n_phi, p_phi in vr.WEIGHT_SETS:
        passes = dr.passes_of(max(vr.FILTER_SIZES))
        f64 = vr.guided_chain(orc, cam, w, h, colour, normal, depth, passes, vr.DEFAULT_SIGMA, n_phi, p_phi)
        f32 = vr.guided_chain(orc, cam, w, h, colour, normal, depth, passes, vr.DEFAULT_SIGMA, n_phi, p_phi, dtype=np.float32)
        d_var = float(np.abs(f32["variance"] - f64["variance"]).max())
        for fs in vr.FILTER_SIZES:
            k = dr.passes_of(fs) - 1
            d_out = float(np.abs(f32["colour"][k] - f64["colour"][k]).max())
            print(f"{w}x{h} weights {n_phi},{p_phi} filter {fs}: binary32 - float64 variance {d_var:.2e} colour {d_out:.2e}")
            var, out = pkg.check_denoise_variance(colour, normal, depth, cam, fs, n_phi, p_phi, vr.DEFAULT_SIGMA)
            vr.assert_close(var, f64["variance"], vr.tolerance(scale, d_var), ("variance", fs, n_phi, p_phi))
            vr.assert_close(out, f64["colour"][k], vr.tolerance(scale, d_out), ("result", fs, n_phi, p_phi))
    var, out = pkg.check_denoise_variance(colour, normal, depth, cam, 0)
    assert out is None and np.isfinite(var).all()  # no pass, no result; the estimate is still there


# plain / guided RMSE of the float64 restatement at the default sigma over the three noise levels (tools/denoise_variance_sweep.py
# edge; profiles/denoise_variance.txt): whole frame 11.04, 5.12, 2.69; edge band 3.91, 2.38, 1.64.  The margin is half the smallest.
R_WHOLE, R_BAND = 2.69 / 2.0, 1.64 / 2.0


@pytest.mark.parametrize("noise", vr.EDGE_NOISES)
def test_guided_beats_plain_on_a_low_contrast_edge(pkg, orc, noise):
    """the 64 x 64 edge image, default weights, filter size 16: the library's guided result is closer to the clean image than the
    plain passes' (denoise_ref.denoise_chain, what orc_denoise is pinned to), on the whole frame and in the band around the edge"""
    cam = dr.low_camera(pkg)
    n = vr.EDGE_SIZE
    clean, noisy, normal, depth, band = vr.edge_image(noise)
    plain = dr.denoise(orc, cam, n, n, noisy, normal, depth, 16)
    _, guided = pkg.check_denoise_variance(noisy, normal, depth, cam, 16)
    for what, mask, r in (("whole", None, R_WHOLE), ("band", band, R_BAND)):
        g, p = vr.rmse(guided, clean, mask), vr.rmse(plain, clean, mask)
        print(f"noise {noise} {what}: guided {g:.4f} plain {p:.4f} ratio {p / g:.2f}")
        assert g < p, (what, g, p)
        assert g <= p / r, (what, g, p, r)


def test_constant_image_comes_back_bit_for_bit(pkg):
    """equal colours under normals and depths that vary: every difference from the centre is an exact zero, so v = 0 everywhere, the
    exponent is 0 / floor = 0, and the average of equal values is that value"""
    w, h = 65, 33
    _, normal, depth = vr.synthetic_planes(w, h, seed=3)
    colour = np.empty((h, w, 3), dtype=np.float32)
    colour[:] = np.array([0.1, 0.7, 1.3], dtype=np.float32)
    for fs in vr.FILTER_SIZES:
        var, out = pkg.check_denoise_variance(colour, normal, depth, dr.low_camera(pkg), fs)
        assert not var.any(), fs
        assert np.array_equal(out.view(np.uint32), colour.view(np.uint32)), fs


def test_outlier_in_a_zero_variance_neighbourhood_is_left_alone(pkg, orc):
    """A pixel that differs from a zero-variance neighbourhood keeps its value and leaves its neighbours theirs.  The neighbourhood has
    zero variance only where the estimate's own weights keep the outlier out of its neighbours' windows -- here a pixel 1000 units
    behind the rest, exp(-1e6 / p_phi) = 0 --; an outlier on the same surface raises the variance of the 7 x 7 pixels around it, as a
    spatial estimate must (section 5s, "what is approximate"), and is then filtered like any noise of that variance."""
    w, h = 33, 17
    colour = np.full((h, w, 3), 0.5, dtype=np.float32)
    normal = np.zeros((h, w, 3), dtype=np.float32)
    normal[..., 2] = 1.0
    depth = np.full((h, w), 2.0, dtype=np.float32)
    colour[8, 16] = (3.0, 0.25, 0.5)
    depth[8, 16] = 1002.0
    cam = dr.low_camera(pkg)
    for fs in vr.FILTER_SIZES:
        var, out = pkg.check_denoise_variance(colour, normal, depth, cam, fs)
        assert not var.any(), fs
        assert np.array_equal(out.view(np.uint32), colour.view(np.uint32)), fs
        v64, o64 = vr.guided(orc, cam, w, h, colour, normal, depth, fs)
        assert np.abs(v64).max() <= 1e-30 and np.abs(o64 - colour).max() <= 1e-15, fs


def test_outlier_on_the_same_surface_is_pulled_in(pkg, orc):
    """The firefly: an outlier at its neighbours' depth and normal raises the variance of the 49 pixels whose windows hold it, its own
    among them, and is then filtered as noise of that variance.  The library follows the restatement; the variance is positive
    exactly within 3 pixels of the outlier; the outlier moves towards its neighbours, further with every filter size (how far is the
    restatement's to say: at sigma 16 its own variance, 0.06 of its squared distance, leaves a neighbour's tap a weight of exp(-3));
    the pixels out of every tap's reach keep their value bit for bit."""
    w, h = 33, 17
    qx, qy = 16, 8
    colour = np.full((h, w, 3), 0.5, dtype=np.float32)
    normal = np.zeros((h, w, 3), dtype=np.float32)
    normal[..., 2] = 1.0
    depth = np.full((h, w), 0.01, dtype=np.float32)  # (flat positions, as the edge image's)
    colour[qy, qx] = (1.2, 1.2, 1.2)
    cam = dr.low_camera(pkg)
    ys, xs = np.mgrid[0:h, 0:w]
    cheb = np.maximum(np.abs(xs - qx), np.abs(ys - qy))
    before = 0.7
    for fs in (1, 3, 16):
        var, out = pkg.check_denoise_variance(colour, normal, depth, cam, fs)
        v64, o64 = vr.guided(orc, cam, w, h, colour, normal, depth, fs)
        vr.assert_close(var, v64, vr.BOUND * 1.2, ("variance", fs))
        vr.assert_close(out, o64, vr.BOUND * 1.2, ("result", fs))
        assert np.array_equal(var > 0.0, cheb <= 3), fs
        left = float(np.abs(out[qy, qx] - 0.5).max())
        print(f"filter {fs}: the outlier stands {left:.4f} from its neighbours (0.7 before the filter)")
        assert left < before, (fs, left, before)
        before = left
        reach = 2 * (2 ** dr.passes_of(fs) - 1)   # the taps of all passes together
        far = cheb > reach
        assert np.array_equal(out[far].view(np.uint32), colour[far].view(np.uint32)), fs


def test_nan_poisons_its_windows_and_taps_only(pkg, orc):
    """one NaN colour: after one pass the colour is NaN exactly within 4 pixels of it -- its 7 x 7 windows reach 3, the prefilter one
    more, and the taps at +-2 lie inside that; the variance plane carries it one pass ahead, so every later pass adds the prefilter's
    pixel and its own taps' reach.  The set of every filter size is the restatement's."""
    w, h = 65, 33
    colour, normal, depth = vr.synthetic_planes(w, h, seed=5)
    qx, qy = 30, 16
    colour[qy, qx, 1] = np.nan
    cam = dr.low_camera(pkg)
    ys, xs = np.mgrid[0:h, 0:w]
    cheb = np.maximum(np.abs(xs - qx), np.abs(ys - qy))
    for fs in (1, 3, 16):
        var, out = pkg.check_denoise_variance(colour, normal, depth, cam, fs)
        v64, o64 = vr.guided(orc, cam, w, h, colour, normal, depth, fs)
        assert np.array_equal(np.isnan(var), cheb <= 3), fs
        assert np.array_equal(np.isnan(var), np.isnan(v64)), fs
        assert np.array_equal(np.isnan(out), np.isnan(o64)), fs
        if fs == 1:
            assert np.array_equal(np.isnan(out).any(axis=-1), cheb <= 4)
        assert np.isfinite(out[~np.isnan(o64)]).all(), fs
        assert np.isnan(out).all() == (fs == 16), fs  # (five passes reach every pixel of a 65 x 33 frame, two do not)


@pytest.mark.parametrize("value", [np.inf, -np.inf])
def test_infinity_poisons_what_a_nan_does(pkg, orc, value):
    """an infinite colour: inf - inf in its own window and pass, 0 x inf in its neighbours' -- the non-finite pixels of the variance
    and of the result are the restatement's, which are those a NaN in its place gives, and nothing else is touched"""
    w, h = 65, 33
    colour, normal, depth = vr.synthetic_planes(w, h, seed=5)
    qx, qy = 30, 16
    colour[qy, qx, 1] = value
    as_nan = colour.copy()
    as_nan[qy, qx, 1] = np.nan
    cam = dr.low_camera(pkg)
    for fs in (1, 3):
        var, out = pkg.check_denoise_variance(colour, normal, depth, cam, fs)
        v64, o64 = vr.guided(orc, cam, w, h, colour, normal, depth, fs)
        vn, on = pkg.check_denoise_variance(as_nan, normal, depth, cam, fs)
        assert np.array_equal(~np.isfinite(var), ~np.isfinite(v64)), fs
        assert np.array_equal(~np.isfinite(out).all(axis=-1), ~np.isfinite(o64).all(axis=-1)), fs
        assert np.array_equal(~np.isfinite(var), np.isnan(vn)), fs
        assert np.array_equal(~np.isfinite(out).all(axis=-1), np.isnan(on).any(axis=-1)), fs
        ok = np.isfinite(o64).all(axis=-1)
        assert ok.any() and np.array_equal(out[ok].view(np.uint32), on[ok].view(np.uint32)), fs


@pytest.mark.parametrize("n_phi,p_phi", [(0.0, 0.25), (0.30, 0.0)])
def test_zero_weight_gives_nan_everywhere(pkg, n_phi, p_phi):
    """-0 / 0 at the centre tap of every window and of every pass, as in the plain passes"""
    w, h = 64, 4
    colour, normal, depth = vr.synthetic_planes(w, h, seed=9)
    var, out = pkg.check_denoise_variance(colour, normal, depth, dr.low_camera(pkg), 3, n_phi, p_phi)
    assert np.isnan(var).all() and np.isnan(out).all()


@pytest.mark.parametrize("sigma", [0.0, -1.0, float("nan"), float("inf"), float("-inf")])
def test_bad_sigma_is_refused(pkg, sigma):
    colour, normal, depth = vr.synthetic_planes(4, 4, seed=1)
    with pytest.raises(pkg.PtcError):
        pkg.check_denoise_variance(colour, normal, depth, dr.low_camera(pkg), 3, sigma=sigma)
