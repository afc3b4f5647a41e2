"""The denoiser's albedo rule without a GPU (pt_demodulate.hpp, ptc_check_demodulate): the host's check against the
numpy restatement tests/demodulate_ref.py bit for bit; what the factorisation is for -- demodulate, filter, remodulate is an identity
on colour = albedo x L where the plain filter blurs the albedo's edges --; the floor; the entry points' refusals without a context.
(The parameter's range and refusal text need a context, so a GPU: tests/test_gpu_denoise_albedo.py.)"""
import ctypes as C

import numpy as np

import demodulate_ref as dm
import denoise_ref as dr

W, H = 64, 48
L = np.array([1.0, 0.5, 0.25])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_rule_against_the_restatement(pkg):
    """0, -0, a subnormal, the floor and its two neighbours, 1, 4, inf, NaN x colours 0, 1e-30, 1, 1e30"""
    floor = dm.ALBEDO_FLOOR
    assert float(floor) == 1.0 / 64.0
    albedos = np.array([0.0, -0.0, 1e-40, np.nextafter(floor, np.float32(0)), floor, np.nextafter(floor, np.float32(1)), 1.0, 4.0, np.inf,
                        np.nan], dtype=np.float32)
    colours = np.array([0.0, 1e-30, 1.0, 1e30], dtype=np.float32)
    a, c = (g.reshape(-1) for g in np.meshgrid(albedos, colours, indexing="ij"))
    irr, eff = pkg.check_demodulate(c, a)
    want_irr, want_eff = dm.demodulate(c, a)
    assert np.array_equal(_bits(eff), _bits(want_eff)), (eff.tolist(), want_eff.tolist())
    assert np.array_equal(_bits(irr), _bits(want_irr)), (irr.tolist(), want_irr.tolist())
    # the rule's own anchors: nothing below the floor, the floor's upper neighbour is itself, a NaN albedo takes the floor
    assert np.all(eff >= floor) and not np.isnan(eff).any()
    assert np.all(eff[a == np.nextafter(floor, np.float32(1))] == np.nextafter(floor, np.float32(1)))
    assert np.all(eff[np.isnan(a)] == floor) and np.all(eff[a <= floor] == floor)
    assert np.all(irr[(c == 1.0) & (a == 4.0)] == 0.25) and np.all(irr[(c == 1.0) & (a == 0.0)] == 64.0)
    # the colour comes back: remodulate(demodulate(c)) within an ulp of c where nothing overflows
    back = dm.remodulate(irr, a)
    ok = np.isfinite(irr) & np.isfinite(eff) & (c > 1e-20)
    assert np.all(np.abs(back[ok] / c[ok] - 1.0) <= 2.0 ** -22)


def test_check_demodulate_refusals(pkg):
    lib = pkg.lib()
    one = np.ones(1, dtype=np.float32)
    p = one.ctypes.data_as(C.c_void_p)
    assert lib.ptc_check_demodulate(None, p, 1, p, p) == pkg._capi.PTC_ERR_INVALID
    assert lib.ptc_check_demodulate(p, p, 1, p, None) == pkg._capi.PTC_ERR_INVALID
    assert lib.ptc_check_demodulate(None, None, 0, None, None) == pkg._capi.PTC_OK
    import pytest
    with pytest.raises(ValueError):
        pkg.check_demodulate(np.ones(3), np.ones(4))


def _frame(pkg, orc, albedo):
    """colour = albedo x L on a wall that faces the camera: one normal, positions on the plane z = 0"""
    camera = pkg.scenes._camera_from_look_at((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), vfov_deg=45.0)
    matrix, vfov = dr.gpu_camera(orc, camera, W, H)
    ys, xs = np.mgrid[0:H, 0:W]
    _, dirs = dr.view_rays(matrix, vfov, W, H, xs + 0.5, ys + 0.5)
    depth = 3.0 / -dirs[..., 2]
    normal = np.broadcast_to(np.array([0.0, 0.0, 1.0]), (H, W, 3)).copy()
    alb = np.broadcast_to(np.asarray(albedo, dtype=np.float64)[..., None], (H, W, 3)).copy()
    return camera, alb * L, alb, normal, depth


def _checker():
    ys, xs = np.mgrid[0:H, 0:W]
    return np.where(((xs // 8) + (ys // 8)) % 2 == 0, 0.2, 0.8)


def test_identity_where_the_plain_filter_blurs(pkg, orc):
    """a 0.2 / 0.8 checker in 8-pixel squares under constant light: demodulated, the filter sees a constant and gives the colour back on
    every pixel; the plain filter leaks across every texel edge (the blur this removes: asserted, > 1e-3)"""
    camera, colour, alb, normal, depth = _frame(pkg, orc, _checker())
    for fs in (1, 16):
        got = dm.demodulated_denoise(orc, camera, W, H, colour, alb, normal, depth, fs)
        err = float(np.max(np.abs(got - colour)))
        assert err <= 1e-12, (fs, err)
        plain = dr.denoise(orc, camera, W, H, colour, normal, depth, fs)
        blur = float(np.max(np.abs(plain - colour)))
        print(f"filter size {fs}: plain filter's largest error {blur:.4f}, demodulated {err:.2e}")
        assert blur > 1e-3, (fs, blur)


def test_identity_on_the_floor(pkg, orc):
    """a uniformly dark frame, albedo 1/256 below the floor 1/64: divided and multiplied by the floor, it comes back unchanged"""
    camera, colour, alb, normal, depth = _frame(pkg, orc, np.full((H, W), 1.0 / 256.0))
    assert np.all(dm.effective_f64(alb) == 1.0 / 64.0)
    for fs in (1, 16):
        got = dm.demodulated_denoise(orc, camera, W, H, colour, alb, normal, depth, fs)
        err = float(np.max(np.abs(got - colour)))
        assert err <= 1e-12, (fs, err)


def test_filter_size_below_one_is_no_result(pkg, orc):
    camera, colour, alb, normal, depth = _frame(pkg, orc, _checker())
    assert dm.demodulated_denoise(orc, camera, W, H, colour, alb, normal, depth, 0) is None


def test_entry_points_without_a_context(pkg):
    lib = pkg.lib()
    assert lib.ptc_denoise_albedo(None, None, None, None) == pkg._capi.PTC_ERR_INVALID
    out = np.zeros(3, dtype=np.float32)
    assert lib.ptc_denoise_albedo(None, out.ctypes.data_as(C.c_void_p), None, None) == pkg._capi.PTC_ERR_INVALID
    assert not out.any()
    stats = pkg._capi.ptc_denoise_albedo_stats()
    assert lib.ptc_get_denoise_albedo_stats(None, C.byref(stats)) == pkg._capi.PTC_ERR_INVALID
    assert lib.ptc_set_param(None, b"denoise_albedo", 1) == pkg._capi.PTC_ERR_INVALID
    assert lib.ptc_abi_version() == 3
