"""Environment lighting (ptc_set_environment) without a GPU: the library's host build of csrc/pt_env.hpp
(ptc_check_environment, ptc_check_environment_apron) against the numpy restatement tests/env_ref.py -- the checker of
tests/test_gpu_environment.py -- bit for bit; the apron against the table; the properties the rule promises (index range, weights in
[0, 1), zeros for the bad directions, continuity across the fold, convergence on a smooth sky); the refusals; loop_ref's loops with env=None
are the loops without the option; the Python field's checks."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import env_ref
import lit_ref
import loop_ref

SIZES = (2, 5, 64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(pkg, env, dirs):
    env = np.ascontiguousarray(env, dtype=np.float32)
    dirs = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    out = np.full_like(dirs, -1.0)
    rc = pkg._capi.lib().ptc_check_environment(env.ctypes.data_as(C.c_void_p), env.shape[0], dirs.ctypes.data_as(C.c_void_p), len(dirs),
                                               out.ctypes.data_as(C.c_void_p))
    return rc, out


def _apron(pkg, env):
    env = np.ascontiguousarray(env, dtype=np.float32)
    n = env.shape[0]
    out = np.full((n + 2, n + 2, 4), -1.0, dtype=np.float32)
    assert pkg._capi.lib().ptc_check_environment_apron(env.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p)) == 0
    return out


def _random_map(n, seed):
    return np.random.default_rng(seed).uniform(0.0, 50.0, (n, n, 3)).astype(np.float32)


@pytest.mark.parametrize("n", SIZES)
def test_host_lookup_equals_the_restatement(pkg, n):
    """random texels in [0, 50]; 4096 random directions, the axes, +-0 components, dy = -0 and -1e-30, the fold edges, texel centres and
    edges, the bad directions of item 2"""
    env = _random_map(n, 100 + n)
    dirs = env_ref.direction_set(np.random.default_rng(n), n)
    rc, got = _check(pkg, env, dirs)
    assert rc == 0
    want = env_ref.lookup(env, dirs)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (n, int(bad.sum()), dirs[bad.any(axis=1)][:4].tolist())
    assert np.isfinite(got).all() and (got >= 0.0).all()
    assert (got[-10:] == 0.0).all()  # direction_set ends with the bad directions
    assert (got[:4096] > 0.0).all()  # (a random map has no zero texel)


@pytest.mark.parametrize("n", SIZES + (3,))
def test_apron_against_the_table(pkg, n):
    """the library's apron is env_ref's; and, independently of both, the table of section 5j entry by entry"""
    env = _random_map(n, 200 + n)
    e = _apron(pkg, env)
    assert np.array_equal(_bits(e), _bits(env_ref.apron(env)))
    assert (e[..., 3] == 0.0).all()
    c = lambda t: min(max(t, 0), n - 1)
    for J in range(n + 2):
        for I in range(n + 2):
            i, j = I - 1, J - 1
            i_out, j_out = not 0 <= i < n, not 0 <= j < n
            if not i_out and not j_out:
                want = env[j, i]
            elif i_out and not j_out:
                want = env[n - 1 - j, c(i)]
            elif j_out and not i_out:
                want = env[c(j), n - 1 - i]
            else:
                want = env[n - 1 - c(j), n - 1 - c(i)]
            assert np.array_equal(e[J, I, :3], want), (J, I)
    # the four corners of E hold the four corners of M crosswise: all of them the -y pole's neighbours
    assert np.array_equal(e[0, 0, :3], env[n - 1, n - 1]) and np.array_equal(e[n + 1, n + 1, :3], env[0, 0])
    assert np.array_equal(e[0, n + 1, :3], env[n - 1, 0]) and np.array_equal(e[n + 1, 0, :3], env[0, n - 1])


@pytest.mark.parametrize("n", SIZES)
def test_index_range_and_weights(n):
    """over the direction set, and 200 000 random directions: i0, j0 in 0 .. n exactly, t in [0, 1)"""
    rng = np.random.default_rng(7)
    named = env_ref.direction_set(rng, n)
    ok = env_ref.locate(named, n)[0]
    assert ok[:-10].all() and not ok[-10:].any()
    dirs = np.concatenate([named, rng.standard_normal((200_000, 3)).astype(np.float32)])
    ok, i0, j0, tx, tz = env_ref.locate(dirs, n)
    for idx in (i0[ok], j0[ok]):
        assert idx.min() == 0 and idx.max() == n
    for t in (tx[ok], tz[ok]):
        assert t.min() >= 0.0 and t.max() < 1.0


def test_a_map_of_zeros_is_exact_and_a_constant_map_is_close(pkg):
    """zeros come back as zeros on every direction; a constant c comes back within two roundings of each lerp (c (1 - t) + c t rounds:
    at most 3 u per lerp, two lerps deep)"""
    dirs = env_ref.direction_set(np.random.default_rng(3), 8)
    rc, got = _check(pkg, np.zeros((8, 8, 3), dtype=np.float32), dirs)
    assert rc == 0 and (_bits(got) == 0).all()
    rc, got = _check(pkg, np.full((8, 8, 3), 0.7, dtype=np.float32), dirs)
    assert rc == 0
    good = got[:-10]
    assert np.abs(good.astype(np.float64) - float(np.float32(0.7))).max() <= 0.7 * 8 * 2.0 ** -24


def _smooth(d):
    """a smooth radiance on the unit sphere, >= 0"""
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return np.stack([1.5 + np.sin(2.0 * x) * y + 0.5 * z, 1.2 + 0.8 * x * z + 0.3 * y, 2.0 + np.cos(1.5 * y) * x - 0.7 * z * y], axis=1)


def _octa_map(n, f):
    """f at the texel centres of an n-map: (u, v) = ((i + 0.5) / n, (j + 0.5) / n) -> q = 2 (u, v) - 1 -> the direction by the inverse of
    items 3 and 4 (float64)"""
    k = (np.arange(n) + 0.5) / n * 2.0 - 1.0
    qx, qz = (g.reshape(-1) for g in np.meshgrid(k, k))  # row j along z, column i along x
    y = 1.0 - np.abs(qx) - np.abs(qz)
    lower = y < 0.0
    px = np.where(lower, (1.0 - np.abs(qz)) * np.where(qx < 0, -1.0, 1.0), qx)
    pz = np.where(lower, (1.0 - np.abs(qx)) * np.where(qz < 0, -1.0, 1.0), qz)
    return f(np.stack([px, y, pz], axis=1)).reshape(n, n, 3).astype(np.float32)


def test_the_lookup_converges_on_a_smooth_sky_and_is_continuous_across_the_fold(pkg):
    """A smooth radiance sampled at the texel centres comes back with an error that falls by at least 3 x for every 4 x in n: the
    fetch is bilinear (second order) away from the creases of the octahedral chart -- the horizon and the four diagonals, where the
    chart is only continuous -- and first order (4 x per 4 x) across them.  That holds only if the apron joins the right texels: a
    wrong row of it leaves an error that does not fall at all.  And values a hair above and below the horizon agree to the map's
    resolution."""
    rng = np.random.default_rng(11)
    dirs = np.concatenate([rng.standard_normal((50_000, 3)), np.eye(3), -np.eye(3)]).astype(np.float32)
    t = np.linspace(-1.0, 1.0, 2001)
    edge = np.stack([1.0 - np.abs(t), np.zeros_like(t), t], axis=1)
    above, below = (edge + [0.0, 1e-6, 0.0]).astype(np.float32), (edge - [0.0, 1e-6, 0.0]).astype(np.float32)
    truth = _smooth(dirs.astype(np.float64))
    errs = {}
    for n in (8, 32, 128):
        env = _octa_map(n, _smooth)
        rc, got = _check(pkg, env, dirs)
        assert rc == 0
        errs[n] = float(np.abs(got - truth).max())
        _, a = _check(pkg, env, above)
        _, b = _check(pkg, env, below)
        jump = float(np.abs(a.astype(np.float64) - b).max())
        print(f"n {n}: max error {errs[n]:.3g}, largest jump across the horizon {jump:.3g}")
        assert jump <= 1e-4, (n, jump)  # (2e-6 of direction: nothing of the map's scale)
    assert errs[8] >= 3.0 * errs[32] and errs[32] >= 3.0 * errs[128], errs


def test_the_refusals(pkg):
    env = _random_map(4, 1)
    dirs = np.eye(3, dtype=np.float32)
    invalid = pkg._capi.PTC_ERR_INVALID
    lib = pkg._capi.lib()
    out = np.zeros_like(dirs)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.ptc_check_environment(None, 4, p(dirs), 3, p(out)) == invalid
    assert lib.ptc_check_environment(p(env), 4, None, 3, p(out)) == invalid
    assert lib.ptc_check_environment(p(env), 4, p(dirs), 3, None) == invalid
    assert lib.ptc_check_environment(p(env), 4, None, 0, None) == 0
    for n in (0, 1, 4097):
        big = np.zeros((max(n, 2), max(n, 2), 3), dtype=np.float32) if n < 100 else env  # (refused before anything is read)
        assert lib.ptc_check_environment(p(big), n, p(dirs), 3, p(out)) == invalid, n
    for bad in (np.nan, np.inf, -np.inf, -1e-30):
        e = env.copy()
        e[2, 1, 1] = bad
        assert lib.ptc_check_environment(p(e), 4, p(dirs), 3, p(out)) == invalid, bad
    e = env.copy()
    e[0, 0, 0] = -0.0  # (-0 is not negative)
    assert lib.ptc_check_environment(p(e), 4, p(dirs), 3, p(out)) == 0


def test_no_environment_is_lit_ref_s_own_render(pkg, orc):
    """env None given is env not given, in both loops; with a map or without, lit_ref.sky is left alone (the sky is an argument)"""
    w, h = 16, 12
    scene = pkg.scenes.cornell_spheres((w, h))
    flat = scene.build_scene()
    sky = lit_ref.sky
    for mine in (loop_ref.render_streaming, loop_ref.render_megakernel):
        a, b = mine(orc, flat, scene.camera, w, h, 0, 2, 3, env=None), mine(orc, flat, scene.camera, w, h, 0, 2, 3)
        for k in ("color", "normal", "depth"):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k
        assert a["rays"] == b["rays"]
        c = mine(orc, flat, scene.camera, w, h, 0, 2, 3, env=np.zeros((2, 2, 3), dtype=np.float32))
        assert lit_ref.sky is sky
        assert c["rays"] == b["rays"] and np.array_equal(_bits(c["depth"]), _bits(b["depth"])) and np.array_equal(_bits(c["normal"]), _bits(b["normal"]))
        assert not np.array_equal(c["color"], b["color"])


def test_the_python_field_checks_its_value(pkg):
    pt = object.__new__(pkg.PathTracer)  # (no context: the setter touches none)
    pt._environment = None
    for bad in (np.zeros((4, 4)), np.zeros((4, 5, 3)), np.zeros((1, 1, 3)), np.zeros((4, 4, 4)), np.full((2, 2, 3), np.nan), np.full((2, 2, 3), -1.0),
                np.full((2, 2, 3), np.inf)):
        with pytest.raises(ValueError):
            pt.environment = bad
    src = np.ones((3, 3, 3))
    pt.environment = src
    assert pt.environment.dtype == np.float32 and pt.environment.shape == (3, 3, 3) and pt.environment is not src
    src[:] = 5.0
    assert (pt.environment == 1.0).all()  # (copied at assignment)
    pt.environment = None
    assert pt.environment is None


# ---- the host mirrors: .hdr readers, the conversion, the scene key, hip_pt's arguments ----------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_PT = os.path.join(ROOT, "cuda-path-tracer_amd", "host", "hip_pt")
MINIMAL = {"materials": [{"name": "m", "type": "lambertian", "albedo": [0.5, 0.5, 0.5]}],
           "surfaces": [{"type": "sphere", "radius": 1.0, "material": "m", "transform": {"translate": [0, 0, 0]}}],
           "camera": {"vfov": 45, "resolution": [16, 12]}}


def _ensure_cli():
    if not os.path.exists(HIP_PT):
        subprocess.run(["make"], cwd=os.path.dirname(HIP_PT), check=True, stdout=subprocess.DEVNULL)


def _picture(h=12, w=20, seed=4):
    """RGBE bytes [h, w, 4] with runs (so the run-length form has runs and literals), exponent 0 pixels, the extreme exponents"""
    rng = np.random.default_rng(seed)
    rgbe = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    rgbe[:, :, 3] = rng.integers(120, 140, (h, w))
    rgbe[2, 3:15] = rgbe[2, 3]        # a run in every channel
    rgbe[5, :, 0] = 7                 # a whole row of one channel
    rgbe[7, 4:9, 3] = 0               # exponent 0: the value is 0 whatever the mantissas
    rgbe[8, 0] = (255, 1, 0, 255)     # the largest exponent
    rgbe[8, 1] = (255, 1, 0, 1)       # the smallest: 255 * 2^-135
    return rgbe


def _decode(rgbe):
    scale = np.ldexp(np.float32(1.0), rgbe[..., 3].astype(np.int32) - 136).astype(np.float32)
    scale[rgbe[..., 3] == 0] = 0.0
    return rgbe[..., :3].astype(np.float32) * scale[..., None]


def _scene_file(tmp_path, env=None, name="s.json"):
    scene = dict(MINIMAL)
    if env is not None:
        scene["environment"] = env
    path = tmp_path / name
    path.write_text(json.dumps(scene))
    return str(path)


def _dump_environment(tmp_path, args):
    """hip_pt ... --dump-environment -> (the decoded picture [h, w, 3], the map [n, n, 3])"""
    out = tmp_path / "env.bin"
    r = subprocess.run([HIP_PT] + args + ["--dump-environment", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    data = out.read_bytes()
    w, h = struct.unpack_from("<ii", data, 0)
    n_img = struct.unpack_from("<Q", data, 8)[0]
    img = np.frombuffer(data, dtype="<f4", count=n_img, offset=16).reshape(h, w, 3)
    off = 16 + 4 * n_img
    n_map = struct.unpack_from("<Q", data, off)[0]
    size = int(round((n_map / 3) ** 0.5))
    return img, np.frombuffer(data, dtype="<f4", count=n_map, offset=off + 8).reshape(size, size, 3)


@pytest.mark.parametrize("rle", [False, True])
def test_hdr_readers_decode_the_same_floats(pkg, tmp_path, rle):
    """a flat and a run-length-encoded file written here: Python's reader, hip_pt's reader and value = mantissa * 2^(e - 136) agree
    bit for bit"""
    _ensure_cli()
    rgbe = _picture()
    path = tmp_path / "p.hdr"
    pkg.hdr.write_hdr(str(path), rgbe, rle=rle)
    if rle:
        assert path.stat().st_size < len(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 12 +X 20\n") + rgbe.size + 4 * 12  # (runs were found)
    want = _decode(rgbe)
    got = pkg.hdr.read_hdr(str(path))
    assert got.shape == (12, 20, 3) and np.array_equal(_bits(got), _bits(want))
    assert got[8, 0, 0] == np.float32(255.0 * 2.0 ** 119) and got[8, 1, 0] == np.float32(255.0 * 2.0 ** -135) and (got[7, 4:9] == 0).all()
    img, _ = _dump_environment(tmp_path, [_scene_file(tmp_path), "--environment", str(path), "--environment-scale", "0"])
    assert np.array_equal(_bits(img), _bits(want))


def test_rgbe_round_trip_of_float_images(pkg, tmp_path):
    """write_hdr's encoder on floats: within RGBE's precision (the largest component's 8 bits, truncated)"""
    img = np.random.default_rng(2).uniform(0.0, 40.0, (9, 16, 3)).astype(np.float32)
    img[3, 3] = 0.0
    for rle in (False, True):
        pkg.hdr.write_hdr(str(tmp_path / "f.hdr"), img, rle=rle)
        back = pkg.hdr.read_hdr(str(tmp_path / "f.hdr"))
        assert (back <= img).all() and (img - back <= img.max(axis=-1, keepdims=True) / 128.0).all() and (back[3, 3] == 0).all()


def test_malformed_hdr_files_are_refused(pkg, tmp_path):
    _ensure_cli()
    good = tmp_path / "good.hdr"
    pkg.hdr.write_hdr(str(good), _picture(), rle=True)
    data = good.read_bytes()
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n"
    flat = head + b"-Y 2 +X 3\n" + bytes(24)
    cases = {"truncated_rle": data[:-5], "truncated_flat": flat[:-1], "no_signature": data[2:], "no_format": data.replace(b"FORMAT=32-bit_rle_rgbe\n", b""),
             "other_orientation": data.replace(b"-Y 12 +X 20", b"+Y 12 +X 20"), "no_resolution": head + b"\n", "zero_width": head + b"-Y 2 +X 0\n",
             "run_past_the_scanline": head + b"-Y 1 +X 8\n" + bytes([2, 2, 0, 8, 128 + 9, 1]) + bytes(64),
             "empty_literal": head + b"-Y 1 +X 8\n" + bytes([2, 2, 0, 8, 0]) + bytes(64), "empty": b""}
    scene = _scene_file(tmp_path)
    for name, blob in cases.items():
        path = tmp_path / (name + ".hdr")
        path.write_bytes(blob)
        with pytest.raises(ValueError, match="Unable to load"):
            pkg.hdr.read_hdr(str(path))
        r = subprocess.run([HIP_PT, scene, "--environment", str(path), "--dump-environment", str(tmp_path / "x.bin")], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 1 and "Unable to load" in r.stderr, (name, r.stderr)
    (tmp_path / "flat_ok.hdr").write_bytes(flat)  # (the flat file the truncated one was cut from does read)
    assert np.array_equal(pkg.hdr.read_hdr(str(tmp_path / "flat_ok.hdr")), np.zeros((2, 3, 3)))


def _equirect_f64(image, n, scale):
    """ptc_environment_from_equirect restated in float64 numpy"""
    h, w = image.shape[:2]
    k = 2.0 * ((np.arange(n) + 0.5) / n) - 1.0
    qx, qz = np.meshgrid(k, k)
    y = 1.0 - np.abs(qx) - np.abs(qz)
    lower = y < 0.0
    x = np.where(lower, (1.0 - np.abs(qz)) * np.where(qx < 0, -1.0, 1.0), qx)
    z = np.where(lower, (1.0 - np.abs(qx)) * np.where(qz < 0, -1.0, 1.0), qz)
    length = np.sqrt(x * x + y * y + z * z)
    u = np.arctan2(x / length, -z / length) / (2.0 * np.pi) + 0.5
    v = np.arccos(np.clip(y / length, -1.0, 1.0)) / np.pi
    fx, fy = u * w - 0.5, v * h - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0)[..., None], (fy - y0)[..., None]
    x0 = x0.astype(np.int64) % w
    x1 = (x0 + 1) % w
    y1 = np.clip(y0.astype(np.int64) + 1, 0, h - 1)
    y0 = np.clip(y0.astype(np.int64), 0, h - 1)
    img = image.astype(np.float64)
    top = img[y0, x0] * (1.0 - tx) + img[y0, x1] * tx
    bot = img[y1, x0] * (1.0 - tx) + img[y1, x1] * tx
    return (top * (1.0 - ty) + bot * ty) * float(np.float32(scale)), np.stack([x, y, z], axis=-1) / length[..., None]


def test_the_conversion_against_float64(pkg):
    """C against the float64 restatement to 1e-6 relative, component by component (a bilinear fetch is a convex combination of values
    >= 0: nothing cancels, and the rounding to binary32 alone is 6e-8), on a random picture -- every texel pair matters --, n odd and
    even, smaller and larger than the picture"""
    image = np.random.default_rng(6).uniform(0.0, 10.0, (16, 33, 3)).astype(np.float32)
    for n, scale in ((2, 1.0), (7, 0.5), (16, 2.0), (40, 1.0)):
        got = pkg.hdr.environment_from_equirect(image, n, scale)
        want, _ = _equirect_f64(image, n, scale)
        assert got.shape == (n, n, 3) and got.dtype == np.float32
        rel = np.abs(got - want) / want
        print(f"n {n}, scale {scale}: largest relative error {rel.max():.3g}")
        assert (want > 0.0).all() and (np.abs(got - want) <= 1e-6 * want).all(), (n, scale, float(rel.max()))
    assert pkg.hdr.environment_from_equirect(image).shape == (16, 16, 3)  # (the picture's height by default)
    for bad in (dict(size=1), dict(size=4097), dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf"))):
        with pytest.raises(ValueError):
            pkg.hdr.environment_from_equirect(image, **bad)


def test_the_conversion_converges_on_a_smooth_sky(pkg):
    """An analytic smooth sky rendered as an equirectangular picture, converted, and looked up: against the sky itself the error falls
    by at least 3 x each time n, width and height double (two bilinear resamplings of a smooth function: second order away from the
    chart's creases, first order -- 2 x -- only on them, and there the octahedral texels straddle the crease symmetrically).  No
    absolute bound."""
    rng = np.random.default_rng(12)
    dirs = rng.standard_normal((20_000, 3)).astype(np.float32)
    truth = _smooth(dirs.astype(np.float64))
    errs = []
    for n in (16, 32, 64, 128):
        w, h = 4 * n, 2 * n
        phi, theta = ((np.arange(w) + 0.5) / w - 0.5) * 2.0 * np.pi, (np.arange(h) + 0.5) / h * np.pi
        d = np.stack([np.sin(theta)[:, None] * np.sin(phi)[None, :], np.cos(theta)[:, None] * np.ones(w)[None, :],
                      -np.sin(theta)[:, None] * np.cos(phi)[None, :]], axis=-1)
        picture = _smooth(d.reshape(-1, 3)).reshape(h, w, 3).astype(np.float32)
        env = pkg.hdr.environment_from_equirect(picture, n)
        rc, got = _check(pkg, env, dirs)
        assert rc == 0
        errs.append(float(np.sqrt(np.mean((got - truth) ** 2))))
    print("rms error per doubling:", " ".join(f"{e:.3g}" for e in errs))
    for a, b in zip(errs, errs[1:]):
        assert a >= 3.0 * b, errs


def test_the_scene_key_in_both_parsers(pkg, tmp_path):
    """"environment": {"file", "scale", "size"}: the path is relative to the scene file; scale defaults to 1, size to the picture's
    height; both readers make the same map, bit for bit; and refuse the same entries"""
    _ensure_cli()
    os.makedirs(tmp_path / "sub", exist_ok=True)
    img = np.random.default_rng(8).uniform(0.0, 5.0, (10, 24, 3)).astype(np.float32)
    pkg.hdr.write_hdr(str(tmp_path / "sub" / "sky.hdr"), img, rle=True)
    picture = pkg.hdr.read_hdr(str(tmp_path / "sub" / "sky.hdr"))
    for entry, n, scale in (({"file": "sub/sky.hdr"}, 10, 1.0), ({"file": "sub/sky.hdr", "scale": 0.25}, 10, 0.25),
                            ({"file": "sub/sky.hdr", "size": 7}, 7, 1.0), ({"file": "sub/sky.hdr", "scale": 3, "size": 32}, 32, 3.0)):
        path = _scene_file(tmp_path, entry)
        scene = pkg.json_parser.scene_from_json(path)
        want = pkg.hdr.environment_from_equirect(picture, n, scale)
        assert scene.environment.shape == (n, n, 3) and np.array_equal(_bits(scene.environment), _bits(want)), entry
        assert scene.environment_source == {"file": str(tmp_path / "sub" / "sky.hdr"), "scale": scale, "size": n}
        _, cpp = _dump_environment(tmp_path, [path])
        assert np.array_equal(_bits(cpp), _bits(want)), entry
    # the command line over the scene file, value by value
    _, cpp = _dump_environment(tmp_path, [_scene_file(tmp_path, {"file": "sub/sky.hdr", "scale": 3}), "--environment-size", "5"])
    assert np.array_equal(_bits(cpp), _bits(pkg.hdr.environment_from_equirect(picture, 5, 3.0)))
    assert pkg.json_parser.scene_from_json(_scene_file(tmp_path)).environment is None
    # an absolute "file" is taken as it is, by both
    absolute = _scene_file(tmp_path, {"file": str(tmp_path / "sub" / "sky.hdr"), "size": 6})
    want = pkg.hdr.environment_from_equirect(picture, 6, 1.0)
    assert np.array_equal(_bits(pkg.json_parser.scene_from_json(absolute).environment), _bits(want))
    assert np.array_equal(_bits(_dump_environment(tmp_path, [absolute])[1]), _bits(want))
    # a scene whose own picture is missing renders under the command line's: hip_pt opens only the picture that counts
    missing = _scene_file(tmp_path, {"file": "sub/none.hdr", "scale": 2, "size": 9})
    _, cpp = _dump_environment(tmp_path, [missing, "--environment", str(tmp_path / "sub" / "sky.hdr")])
    assert np.array_equal(_bits(cpp), _bits(pkg.hdr.environment_from_equirect(picture, 9, 2.0)))
    for entry in ("sky.hdr", {"scale": 2}, {"file": 3}, {"file": "sub/sky.hdr", "scale": -1}, {"file": "sub/sky.hdr", "scale": "2"},
                  {"file": "sub/sky.hdr", "size": 1}, {"file": "sub/sky.hdr", "size": 4097}, {"file": "sub/sky.hdr", "size": 7.5},
                  {"file": "sub/sky.hdr", "rotation": 30}, {"file": "sub/none.hdr"}):
        path = _scene_file(tmp_path, entry, "bad.json")
        with pytest.raises((ValueError, OSError)):
            pkg.json_parser.scene_from_json(path)
        r = subprocess.run([HIP_PT, path, "--dump-environment", str(tmp_path / "x.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and ("environment" in r.stderr or "Unable to load" in r.stderr), (entry, r.stderr)


def test_the_asset_scene_reads_in_both(pkg, tmp_path):
    _ensure_cli()
    path = os.path.join(ROOT, "assets", "scenes", "spheres_sky.json")
    scene = pkg.json_parser.scene_from_json(path)
    assert scene.environment.shape == (64, 64, 3) and scene.environment.max() > 5.0 and (scene.environment >= 0).all()
    _, cpp = _dump_environment(tmp_path, [path])
    assert np.array_equal(_bits(cpp), _bits(scene.environment))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "environment", "sky_dusk.hdr")) < 8192


def test_hip_pt_argument_errors(tmp_path):
    """refused before the scene is rendered or a GPU touched, exit status 1, the option named"""
    _ensure_cli()
    scene = _scene_file(tmp_path)
    for args, says in ((["--environment"], "missing an argument"), (["--environment-scale", "-1"], "--environment-scale"),
                       (["--environment-scale", "nan"], "--environment-scale"), (["--environment-scale", "x"], "--environment-scale"),
                       (["--environment-size", "1"], "--environment-size"), (["--environment-size", "4097"], "--environment-size"),
                       (["--environment-size", "8.5"], "--environment-size"), (["--environment-size", "8"], "need an environment"),
                       (["--environment-scale", "2"], "need an environment"), (["--dump-environment", str(tmp_path / "x.bin")], "needs an environment"),
                       (["--environment", str(tmp_path / "missing.hdr")], "Unable to load")):
        r = subprocess.run([HIP_PT, scene, "-o", str(tmp_path / "o.png")] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and says in r.stderr, (args, r.stderr)
