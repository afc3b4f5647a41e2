"""The display transform's rule on the host: ptc_check_display_meter / ptc_check_display_map -- csrc/pt_display.hpp,
the functions the kernels call, compiled for the host -- against tests/display_ref.py bit for bit, the trimming rule against a
brute-force sort, the curves against binary64, exact scale invariance, the refusals, and hip_pt's flags.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import display_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_PT = os.path.join(ROOT, "cuda-path-tracer_amd", "host", "hip_pt")
U = 2.0 ** -24  # unit roundoff of binary32


def check_meter(pkg, params, rgb):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    info = pkg._capi.ptc_exposure_info()
    p = params.to_c()
    rc = pkg.lib().ptc_check_display_meter(C.byref(p), rgb.ctypes.data_as(C.c_void_p), rgb.shape[1], len(rgb), C.byref(info))
    assert rc == 0
    return {"pixels": info.pixels, "counted": info.counted, "below": info.below, "rejected": info.rejected, "level_bin": info.level_bin,
            "level": np.float32(info.level), "scale": np.float32(info.scale),
            "histogram": np.ctypeslib.as_array(info.histogram).astype(np.uint32)}


def check_map(pkg, params, scale, rgb):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    out = np.empty((len(rgb), 3), dtype=np.float32)
    p = params.to_c()
    rc = pkg.lib().ptc_check_display_map(C.byref(p), C.c_float(float(scale)), rgb.ctypes.data_as(C.c_void_p), rgb.shape[1], len(rgb),
                                         out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return out


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


def metered(pkg, **kw):
    return pkg.Display(metering=1, **kw)


def one_bin_image(n=4096):
    """every pixel in bin 131: luminances within [1.375, 1.5)"""
    img = np.full((n, 3), 1.4, dtype=np.float32)
    img[::2] *= np.float32(1.03)
    assert set(ref.bins_of(img)) == {131}
    return img


def mixed_sets():
    hostile = ref.hostile_pixels()
    return {"hostile": hostile, "lognormal": ref.lognormal_image(20000), "one_bin": one_bin_image(),
            "nothing": np.array([[0, 0, 0], [-1, 0, 0], [np.nan, 1, 1], [1e-6, 1e-6, 1e-6], [np.inf, 0, 0], [-0.0, -0.0, -0.0]], dtype=np.float32),
            "both": np.concatenate([hostile, ref.lognormal_image(5000, seed=9)])}


@pytest.mark.parametrize("name", ["hostile", "lognormal", "one_bin", "nothing", "both"])
@pytest.mark.parametrize("channels", [3, 4])
def test_meter_equals_restatement(pkg, name, channels):
    """Histogram, below, rejected, level_bin, level and scale, bit for bit, on both pixel layouts (the fourth channel is never read:
    it holds NaN here)."""
    rgb = mixed_sets()[name]
    src = rgb if channels == 3 else np.concatenate([rgb, np.full((len(rgb), 1), np.nan, dtype=np.float32)], axis=1)
    for params in (metered(pkg), metered(pkg, exposure=2.5, key=0.36, low_permille=0, high_permille=1000),
                   metered(pkg, curve=2, low_permille=499, high_permille=500)):
        got, want = check_meter(pkg, params, src), ref.meter(rgb, params)
        assert ref.same_info(got, want), (name, params, got, want)
        assert got["pixels"] == got["counted"] + got["below"] + got["rejected"] == len(rgb)
    if name == "nothing":
        assert got["level_bin"] == -1 and got["counted"] == 0 and got["below"] == 3 and got["rejected"] == 3
        assert same_bits(check_meter(pkg, metered(pkg, exposure=2.5), src)["scale"], np.float32(2.5))  # scale == exposure
    if name == "one_bin":
        assert got["level_bin"] == 131 and got["histogram"][131] == len(rgb)
    if name == "hostile":
        # the edges themselves: as_float(k << 20) in one channel has a luminance below the edge (the weight is < 1), so the bins are
        # read off the restatement; what is pinned here is where the three ranges begin
        assert got["below"] > 0 and got["rejected"] > 0 and got["histogram"][0] > 0 and got["histogram"][255] > 0


def test_bins_are_exponent_and_three_mantissa_bits(pkg):
    """A luminance that is exactly as_float(k << 20) lands in bin k - 888, its predecessor one bin lower: pixels (Y, Y, Y) / sum of the
    weights are not exact, so the luminance is built in the green channel alone and inverted exactly where that is possible --
    instead the test meters single pixels and compares with the bits of the luminance the restatement computes."""
    px = ref.hostile_pixels()
    bins = ref.bins_of(px)
    params = metered(pkg, low_permille=0, high_permille=1000)
    for i in range(0, len(px), 7):
        got = check_meter(pkg, params, px[i:i + 1])
        b = int(bins[i])
        if b >= 0:
            assert got["histogram"][b] == 1 and got["counted"] == 1 and got["level_bin"] == b
            assert same_bits(got["level"], ref.level_of(b))
        else:
            assert got["counted"] == 0 and (got["below"], got["rejected"]) == ((1, 0) if b == ref.BELOW else (0, 1))
    assert ref.level_of(128) == np.float32(1.0) and ref.level_of(0) == np.float32(2.0 ** -16) and ref.level_of(136) == np.float32(2.0)


@pytest.mark.parametrize("low,high", [(0, 1000), (50, 950), (0, 1), (999, 1000), (333, 667), (499, 500), (10, 990), (0, 500), (500, 1000)])
def test_trimming_against_a_sort(pkg, low, high):
    """level_bin against a brute-force sort of the per-pixel bins: drop the first floor(N low / 1000) and the last
    floor(N (1000 - high) / 1000) of the sorted bins, mean of the rest rounded to nearest (halves up).  Images whose bins are so few
    and so full that most pairs split one."""
    rng = np.random.default_rng(low * 1001 + high)
    images = [ref.lognormal_image(4001, seed=3), one_bin_image(777)]
    two = np.full((1000, 3), 0.3, dtype=np.float32)
    two[rng.random(1000) < 0.37] = 40.0
    images.append(two)                                   # two bins, far apart: every pair splits one of them
    images.append(np.exp2(rng.integers(-12, 12, size=(1237, 1))).astype(np.float32) * np.ones((1, 3), dtype=np.float32))
    for img in images:
        params = metered(pkg, low_permille=low, high_permille=high)
        got = check_meter(pkg, params, img)
        b = np.sort(ref.bins_of(img))
        b = b[b >= 0]
        n = len(b)
        kept = b[n * low // 1000: n - n * (1000 - high) // 1000]
        assert len(kept) >= 1
        want = (2 * int(kept.sum()) + len(kept)) // (2 * len(kept))
        assert got["level_bin"] == want == ref.level_bin(got["histogram"], low, high)


def curve_inputs():
    hostile = ref.hostile_pixels()
    sweep = np.exp2(np.linspace(-24, 21, 3001)).astype(np.float32)
    return np.concatenate([hostile, np.repeat(sweep[:, None], 3, axis=1)])


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_map_equals_restatement(pkg, curve):
    """The three curves on the hostile values, bit for bit, under several scales; NaN and negatives give 0, +inf the cap's image."""
    rgb = curve_inputs()
    for scale, white in ((1.0, 4.0), (0.18 / 0.75, 4.0), (1024.0, 1.0), (2.0 ** -30, 11.0)):
        params = pkg.Display(curve=curve, white=white)
        got = check_map(pkg, params, scale, rgb)
        assert same_bits(got, ref.map_channels(rgb, scale, params)), (curve, scale)
        assert np.all(np.isfinite(got)) and np.all(got >= 0)
        bad = np.isnan(rgb) | (rgb <= 0)
        assert np.all(got[bad] == 0)
    params = pkg.Display(curve=curve)
    cap = check_map(pkg, params, 1.0, np.array([[2.0 ** 20] * 3], dtype=np.float32))[0, 0]
    top = check_map(pkg, params, 1.0, np.array([[np.inf, 3e38, 2.0 ** 21]], dtype=np.float32))[0]
    assert same_bits(top, [cap] * 3)
    assert same_bits(cap, ref.map_channels(np.array([[ref.CAP] * 3]), 1.0, params)[0, 0])


def curve_f64(x, curve, w2):
    if curve == 1:
        return x * (1.0 + x / w2) / (1.0 + x)
    if curve == 2:
        k = [float(np.float32(v)) for v in (2.51, 0.03, 2.43, 0.59, 0.14)]
        return x * (k[0] * x + k[1]) / (x * (k[2] * x + k[3]) + k[4])
    return x


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_curves_against_binary64(pkg, curve):
    """The binary32 result against the same expression in binary64 on the same inputs (c, scale, white as binary32 values; ACES'
    constants as the binary32 numbers the code holds).  The bound, from the operation count -- u = 2^-24, every binary32 operation
    multiplies its exact result by (1 + d), |d| <= u, and every intermediate here is positive and normal (c * scale in
    [2^-20, 2^20), white = 4), so nothing cancels and relative errors add to first order:
      e = c * scale                one operation; the curve's logarithmic slope d ln y / d ln e lies in [0, 2] for Reinhard
                                   (1 + q / (1 + q) - x / (1 + x), q = x / w2) and in [-1, 2] for ACES (1 + a / b - x (c2 + d) / den),
                                   so this rounding reaches y as at most 2 u; for CLAMP as u
      CLAMP                        nothing else:                                                   u
      REINHARD                     w2 = white * white (it enters through q / (1 + q) <= 1): u; q, p, n, d, y: 5 u;      8 u in all
      ACES                         a, b, num, c2, d, f, den, y: 8 u;                                                   10 u in all
    second-order terms are below 100 u^2 < 2^-17 u; the bound asserted is the first-order sum times (1 + 2^-16)."""
    ops = {0: 1, 1: 8, 2: 10}[curve]
    bound = ops * U * (1.0 + 2.0 ** -16)
    c = np.exp2(np.linspace(-20, 20, 20001)[:-1]).astype(np.float32)
    params = pkg.Display(curve=curve, white=4.0)
    for scale in (np.float32(1.0), np.float32(0.24), np.float32(3.7)):
        rgb = np.repeat((c / scale).astype(np.float32)[:, None], 3, axis=1)
        e = rgb[:, 0].astype(np.float64) * float(scale)
        ok = (e >= 2.0 ** -20) & (e < 2.0 ** 20)
        got = check_map(pkg, params, scale, rgb)[:, 0].astype(np.float64)
        want = curve_f64(e, curve, 16.0)
        rel = np.abs(got[ok] - want[ok]) / want[ok]
        print(f"curve {curve} scale {scale}: max relative error {rel.max() / U:.3f} u (bound {ops} u)")
        assert ok.sum() > 19000 and rel.max() <= bound


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_curves_are_monotone(pkg, curve):
    """Each curve over a sorted sweep of e = c * scale from 2^-24 up to the cap and beyond: never decreasing.  The sweep's steps are a
    factor 2^(1/64): for CLAMP and Reinhard (white 4), whose slope stays above y / (2 x), a step raises the exact value by more than
    0.5 percent, far above the 8 u of rounding.  ACES levels off at 2.51 / 2.43: its exact value still rises along the whole sweep,
    but its slope falls as 0.238 / x^2: a step's rise, 0.238 * 0.0109 / x, drops under the 2 * 10 u * 1.033 that two roundings of
    test_curves_against_binary64's size can take away at x ~ 2^11.  So: strictly increasing up to 2^10 (a rise of 2.5e-6 against
    1.2e-6), and along the whole sweep no value more than a factor (1 - 20 u) under an earlier one (y_i >= f_i (1 - 10 u),
    y_k <= f_k (1 + 10 u) <= f_i (1 + 10 u) for k < i)."""
    x = np.exp2(np.arange(-24 * 64, 21 * 64 + 1) / 64.0).astype(np.float32)
    x = np.unique(x)
    params = pkg.Display(curve=curve, white=4.0)
    y = check_map(pkg, params, 1.0, np.repeat(x[:, None], 3, axis=1))[:, 0].astype(np.float64)
    if curve != 2:
        below_cap = x <= ref.CAP
        assert np.all(np.diff(y[below_cap]) > 0) and np.all(np.diff(y) >= 0)
        return
    low = x <= 2.0 ** 10
    assert np.all(np.diff(y[low]) > 0)
    running = np.maximum.accumulate(y)
    assert np.all(y >= running * (1.0 - 2 * 10 * U))
    assert y[-1] <= 2.51 / 2.43 * (1 + 10 * U)


def test_exact_scale_invariance(pkg):
    """An image with luminances inside [2^-10, 2^8], times 2^j for j in -4 .. 4: the metering moves by exactly 8 j bins (a power of
    two changes the exponent only: every product, sum and the bin's bits shift exactly), the scale by exactly 2^-j, and so the mapped
    floats are the same bits -- for every curve."""
    rng = np.random.default_rng(11)
    img = np.exp2(rng.uniform(-9.5, 7.5, size=(5000, 1))).astype(np.float32) * rng.uniform(0.8, 1.2, size=(5000, 3)).astype(np.float32)
    b = ref.bins_of(img)
    assert b.min() >= 8 * 6 and b.max() <= 8 * 24     # luminances inside [2^-10, 2^8]
    for curve in (0, 1, 2):
        params = metered(pkg, curve=curve)
        base = check_meter(pkg, params, img)
        mapped = check_map(pkg, params, base["scale"], img)
        for j in range(-4, 5):
            scaled = (img * np.float32(2.0 ** j)).astype(np.float32)
            got = check_meter(pkg, params, scaled)
            assert got["level_bin"] == base["level_bin"] + 8 * j
            assert np.array_equal(np.roll(base["histogram"], 8 * j), got["histogram"])
            assert same_bits(got["scale"], base["scale"] * np.float32(2.0 ** -j))
            assert same_bits(check_map(pkg, params, got["scale"], scaled), mapped), (curve, j)


REFUSALS = [({"exposure": float("nan")}, "exposure"), ({"exposure": float("inf")}, "exposure"), ({"exposure": 0.0}, "exposure"),
            ({"exposure": -1.0}, "exposure"), ({"key": 0.0}, "key"), ({"key": float("nan")}, "key"), ({"white": -4.0}, "white"),
            ({"white": float("inf")}, "white"), ({"low_permille": 950, "high_permille": 50}, "low_permille"),
            ({"low_permille": 500, "high_permille": 500}, "low_permille"), ({"high_permille": 1001}, "high_permille"),
            ({"curve": 3}, "curve"), ({"curve": -1}, "curve"), ({"metering": 2}, "metering")]


@pytest.mark.parametrize("fields,named", REFUSALS)
def test_refusals_name_the_field(pkg, fields, named):
    """ptc_set_display's decision (ptc_check_display_params: the same function, no context): PTC_ERR_INVALID, the field named; the
    host checks refuse the same parameters.  That a refused ptc_set_display leaves the context's display in place needs a context:
    tests/test_gpu_display.py."""
    lib = pkg.lib()
    why = C.create_string_buffer(256)
    good = pkg.Display().to_c()
    assert lib.ptc_check_display_params(C.byref(good), why, 256) == 0 and why.value == b""
    bad = pkg.Display().to_c()
    for k, v in fields.items():
        setattr(bad, k, v)
    assert lib.ptc_check_display_params(C.byref(bad), why, 256) == pkg._capi.PTC_ERR_INVALID
    assert why.value.decode().startswith(named), why.value
    rgb = np.ones((4, 3), dtype=np.float32)
    info = pkg._capi.ptc_exposure_info()
    assert lib.ptc_check_display_meter(C.byref(bad), rgb.ctypes.data_as(C.c_void_p), 3, 4, C.byref(info)) == pkg._capi.PTC_ERR_INVALID
    assert lib.ptc_check_display_map(C.byref(bad), C.c_float(1.0), rgb.ctypes.data_as(C.c_void_p), 3, 4,
                                     rgb.ctypes.data_as(C.c_void_p)) == pkg._capi.PTC_ERR_INVALID


def test_cli_refuses_display_flags():
    """hip_pt refuses a malformed display flag, and any of them together with --display normal | depth, before it reads the scene or
    touches a GPU; the usage text names them."""
    if not os.path.exists(HIP_PT):
        subprocess.run(["make"], cwd=os.path.dirname(HIP_PT), check=True, stdout=subprocess.DEVNULL)
    scene = "scenes/no_such_scene.json"  # never read: the refusal comes first

    def run(*flags):
        return subprocess.run([HIP_PT, scene, "-o", "x.png", *flags], cwd=ROOT, capture_output=True, text=True)

    for flags, text in ((("--tonemap", "filmic"), "unknown curve 'filmic'"), (("--exposure", "bright"), "'--exposure': 'bright'"),
                        (("--exposure", "nan"), "'--exposure'"), (("--exposure", "400"), "'--exposure'"), (("--exposure",), "missing an argument"),
                        (("--white", "0"), "'--white': '0'"), (("--white", "-2"), "'--white'"), (("--key", "inf"), "'--key'"),
                        (("--key", "0.18x"), "'--key': '0.18x'")):
        r = run(*flags)
        assert r.returncode == 1 and text in r.stderr, (flags, r.stderr)
    for flags in (("--tonemap", "aces"), ("--exposure", "1"), ("--auto-exposure",), ("--white", "2"), ("--key", "0.2")):
        for view in ("normal", "depth"):
            for order in ((*flags, "--display", view), ("--display", view, *flags)):
                r = run(*order)
                assert r.returncode == 1 and flags[0] in r.stderr and "--display normal or depth" in r.stderr, (order, r.stderr)
    r = run("--tonemap", "aces", "--exposure", "-1.5", "--auto-exposure", "--display", "color")
    assert "no_such_scene" in r.stderr or "Cannot" in r.stderr or r.returncode != 0  # accepted: it went on to the scene file
    assert "--display normal or depth" not in r.stderr and "Option" not in r.stderr
    r = subprocess.run([HIP_PT, "--help"], capture_output=True, text=True)
    for flag in ("--tonemap", "--exposure", "--auto-exposure", "--white", "--key"):
        assert flag in r.stderr
