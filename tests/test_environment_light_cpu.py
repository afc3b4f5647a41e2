"""Environment light sampling (ptc_environment_light, "environment_light") without a GPU: the alias table the
library's host code builds (ptc_check_environment_light_table) against the properties section 5k promises; the library's host build of
csrc/pt_env_light.hpp (ptc_check_environment_light) against the numpy restatement tests/env_light_ref.py -- the checker of
tests/test_gpu_environment_light.py -- bit for bit, on random draws and on the edges; the stream; the estimator's expectation against a
binary64 quadrature; the numpy loop with the option off; the hooks' refusals."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import env_light_ref
import env_ref
import loop_ref

SIZES = (2, 5, 64)
T_BOUND = 4.073  # the two-sided 0.1 % point of Student's t, 15 degrees of freedom (test_gpu_direct_loop.test_same_expectation_lower_spread)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sun_map(n, seed):
    """a seeded random HDR sky in [0, 1) with a two-texel sun of 5000"""
    m = np.random.default_rng(seed).uniform(0.0, 1.0, (n, n, 3)).astype(np.float32)
    j, i = n // 3, n // 2
    m[j, i] = m[j, min(i + 1, n - 1)] = (5000.0, 4500.0, 4000.0)
    return m


def sparse_map(n, seed):
    """nine texels in ten are zero"""
    rng = np.random.default_rng(seed)
    m = rng.uniform(0.0, 10.0, (n, n, 3)).astype(np.float32)
    m[rng.uniform(size=(n, n)) < 0.9] = 0.0
    m[n - 1, 0, 1] = 3.0  # (never all zero)
    return m


def one_hot_map(n, seed):
    m = np.zeros((n, n, 3), dtype=np.float32)
    m[n // 2, n - 1, 2] = 7.0
    return m


MAPS = {"sun": sun_map, "sparse": sparse_map, "one_hot": one_hot_map}


def weights_f64(env):
    """section 5k's weights, independently of the library: the 3 x 3 stencil (1/8, 6/8, 1/8) on the aproned map, the largest channel,
    times |w_c|_1^3 at the square's centre -> (w [n n] in table order, neighbourhood-has-a-positive-component [n n])"""
    e = env_ref.apron(env).astype(np.float64)[..., :3]
    n = e.shape[0] - 2
    k = np.array([0.125, 0.75, 0.125])
    filt = sum(k[dj] * k[di] * e[dj:dj + n, di:di + n] for dj in range(3) for di in range(3))
    lum = filt.max(axis=2)
    any_pos = np.zeros((n, n), dtype=bool)
    for dj in range(3):
        for di in range(3):
            any_pos |= (e[dj:dj + n, di:di + n] > 0.0).any(axis=2)
    c = (np.arange(n) + 0.5) / n
    sx, sz = np.meshgrid(c, c)  # [j, i]
    qx, qz = 2.0 * sx - 1.0, 2.0 * sz - 1.0
    y = 1.0 - np.abs(qx) - np.abs(qz)
    low = y < 0.0
    x = np.where(low, (1.0 - np.abs(qz)) * np.where(qx < 0.0, -1.0, 1.0), qx)
    z = np.where(low, (1.0 - np.abs(qx)) * np.where(qz < 0.0, -1.0, 1.0), qz)
    l1 = (np.abs(x) + np.abs(y) + np.abs(z)) / np.sqrt(x * x + y * y + z * z)
    return (lum * l1 ** 3).reshape(-1), any_pos.reshape(-1)


@pytest.mark.parametrize("kind", sorted(MAPS))
@pytest.mark.parametrize("n", SIZES)
def test_table_properties(pkg, n, kind):
    env = MAPS[kind](n, 10 * n + len(kind))
    entries, W, positive = env_light_ref.table_of(pkg, env)
    w, any_pos = weights_f64(env)
    n2 = n * n
    assert entries is not None and len(entries) == n2
    assert W == pytest.approx(w.sum(), rel=1e-12)
    # every square whose neighbourhood has a positive component has weight > 0, and the library counts the same squares
    assert (w[any_pos] > 0.0).all() and (w[~any_pos] == 0.0).all()
    assert positive == int(any_pos.sum())
    q, alias = entries["q"].astype(np.float64), entries["alias"].astype(np.int64)
    assert (alias < n2).all() and (q >= 0.0).all() and (q <= 1.0).all()
    own = np.arange(n2)
    assert (alias[q == 1.0] == own[q == 1.0]).all()
    # the probability a draw gives square k: its own q and the remainders of the entries that name it, over n^2
    gives = alias != own
    recon = q.copy()
    np.add.at(recon, alias[gives], 1.0 - q[gives])
    recon /= n2
    P = w / w.sum()
    # squares of weight 0 are never reachable: q 0, and nobody's alias
    assert (recon[P == 0.0] == 0.0).all()
    assert (q[P == 0.0] == 0.0).all() and not np.isin(alias[gives], own[P == 0.0]).any()
    # 1e-6 relative is binary32 q: a square's own q is off by 2^-24 relative (6e-8), and each remainder 1 - q_e it is given by at most
    # half an ulp of q_e, 2^-25 absolute, against a probability that was at least 1 / n^2 when the square began to receive; sixteen
    # such roundings that all fall the same way are the bound
    rel = np.abs(recon - P)[P > 0.0] / P[P > 0.0]
    assert (rel <= 1e-6).all(), float(rel.max())
    # f = (float)(1 / (P n^2)) of the entry's own square and of its alias's
    want = np.zeros(n2, dtype=np.float32)
    with np.errstate(over="ignore"):
        want[P > 0.0] = (1.0 / (P[P > 0.0] * n2)).astype(np.float32)
    assert (np.abs(entries["f"].astype(np.float64) - want) <= np.spacing(want)).all()
    assert np.array_equal(_bits(entries["f_alias"]), _bits(entries["f"][alias]))


def test_a_map_of_zeros_has_no_table(pkg):
    entries, W, positive = env_light_ref.table_of(pkg, np.zeros((5, 5, 3), dtype=np.float32))
    assert entries is None and W == 0.0 and positive == 0


def _hook(pkg, env, points, normals, v, u):
    env = np.ascontiguousarray(env, dtype=np.float32)
    points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    v = np.ascontiguousarray(v, dtype=np.uint32)
    u = np.ascontiguousarray(u, dtype=np.float32).reshape(-1, 3)
    k = len(points)
    radiance, rays, sampled = np.full((k, 3), -1.0, np.float32), np.full((k, 8), -1.0, np.float32), np.full(k, 7, np.uint8)
    rc = pkg._capi.lib().ptc_check_environment_light(env.ctypes.data_as(C.c_void_p), env.shape[0], points.ctypes.data_as(C.c_void_p),
                                                     normals.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), u.ctypes.data_as(C.c_void_p),
                                                     k, radiance.ctypes.data_as(C.c_void_p), rays.ctypes.data_as(C.c_void_p),
                                                     sampled.ctypes.data_as(C.c_void_p))
    return rc, radiance, rays, sampled


def _raw_for(square, n):
    """the smallest raw value whose entry is `square`: ((v - 1) n^2) >> 31 == square"""
    return -(-(int(square) << 31) // (n * n)) + 1


def draw_set(rng, n, count=4096):
    """`count` random draws, then the edges: v = 1 and 2^31 - 2; u1 exactly 0 and 1.0f; u2 / u3 exactly 0 and 1.0f; every square on the
    fold edge and the four corner squares (the -y pole), at their corners, their edges and their centre; normals that cull"""
    v = [rng.integers(1, 2 ** 31 - 1, count)]
    u = [(rng.integers(0, 2 ** 31, (count, 3)).astype(np.float32) / np.float32(2.0 ** 31)).astype(np.float32)]
    ends = np.array([0.0, 1.0], dtype=np.float32)
    for raw in (1, 2 ** 31 - 2, _raw_for(n * n // 2, n)):
        for u1 in ends:
            for u2 in ends:
                for u3 in ends:
                    v.append([raw])
                    u.append([[u1, u2, u3]])
    c = (np.arange(n) + 0.5) / n * 2.0 - 1.0
    on_fold = [j * n + i for j in range(n) for i in range(n) if abs(abs(c[i]) + abs(c[j]) - 1.0) <= 2.0 / n]
    corners = [0, n - 1, n * (n - 1), n * n - 1]
    for square in on_fold[:256] + corners:
        for u2 in (0.0, 0.5, 1.0):
            for u3 in (0.0, 0.5, 1.0):
                v.append([_raw_for(square, n)])
                u.append([[0.0, u2, u3]])  # u1 = 0 keeps the entry's own square wherever its q > 0
    v = np.concatenate([np.asarray(a, dtype=np.uint32).reshape(-1) for a in v])
    u = np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1, 3) for a in u])
    normals = rng.standard_normal((len(v), 3))
    normals = (normals / np.linalg.norm(normals, axis=1)[:, None]).astype(np.float32)
    normals[count:count + 24:2] = (0.0, 1.0, 0.0)
    points = rng.uniform(-3.0, 3.0, (len(v), 3)).astype(np.float32)
    return points, normals, v, u


@pytest.mark.parametrize("kind", ("sun", "sparse"))
@pytest.mark.parametrize("n", SIZES)
def test_host_sample_equals_the_restatement(pkg, n, kind):
    env = MAPS[kind](n, 300 + n)
    entries, _, _ = env_light_ref.table_of(pkg, env)
    texels = env_ref.apron(env)
    points, normals, v, u = draw_set(np.random.default_rng(n), n)
    want = env_light_ref.sample(entries, texels, points, normals, v, u)
    # ... and each sample again about the opposite normal: whichever of the two culls, culls here
    flipped = env_light_ref.sample(entries, texels, points, -normals, v, u)
    for nrm, ref in ((normals, want), (-normals, flipped)):
        rc, radiance, rays, sampled = _hook(pkg, env, points, nrm, v, u)
        assert rc == 0
        assert np.array_equal(sampled.astype(bool), ref["sampled"])
        bad = (_bits(radiance) != _bits(ref["contribution"])).any(axis=1) | (_bits(rays) != _bits(ref["rays"])).any(axis=1)
        assert not bad.any(), (n, kind, int(bad.sum()), np.nonzero(bad)[0][:4].tolist())
    assert want["sampled"].any() and (~want["sampled"]).any() and (want["sampled"] ^ flipped["sampled"]).sum() >= len(v) - 8
    assert np.isfinite(want["contribution"]).all() and (want["contribution"] >= 0.0).all()
    assert (want["square"] >= 0).all() and (want["square"] < n * n).all()
    # the directions are unit vectors, on both sheets
    assert np.abs(np.linalg.norm(want["w"].astype(np.float64), axis=1) - 1.0).max() < 1e-6
    assert (want["w"][:, 1] > 0).any() and (want["w"][:, 1] < 0).any()


def test_a_sample_lands_in_the_square_it_picked(pkg):
    """decode is the inverse of the lookup's octahedral map: the direction of a point strictly inside square k is located in texel k"""
    n = 5
    env = sun_map(n, 1)
    entries, _, _ = env_light_ref.table_of(pkg, env)
    squares = np.arange(n * n)
    v = np.array([_raw_for(k, n) for k in squares], dtype=np.uint32)
    u = np.tile(np.array([[0.0, 0.5, 0.5]], dtype=np.float32), (n * n, 1))
    s = env_light_ref.sample(entries, env_ref.apron(env), np.zeros((n * n, 3)), np.tile([0.0, 1.0, 0.0], (n * n, 1)), v, u)
    assert np.array_equal(s["square"], squares)
    ok, i0, j0, tx, tz = env_ref.locate(s["w"], n)
    # the centre of square (i, j) is texel (i, j)'s own centre: lower texel of E i, upper weight 1 -- or lower i + 1, weight 0
    i = np.where(tx > 0.5, i0, i0 - 1)
    j = np.where(tz > 0.5, j0, j0 - 1)
    assert ok.all() and np.array_equal(j * n + i, squares)


def _hash32(a):
    m = 0xFFFFFFFF
    a = ((a + 0x7ED55D16) + (a << 12)) & m
    a = ((a ^ 0xC761C23C) ^ (a >> 19)) & m
    a = ((a + 0x165667B1) + (a << 5)) & m
    a = ((a + 0xD3A2646C) ^ (a << 9)) & m
    a = ((a + 0xFD7046C5) + (a << 3)) & m
    a = ((a ^ 0xB55A4F09) ^ (a >> 16)) & m
    return a


def test_the_stream(pkg, orc):
    """the draws the device uses -- seed path_seed(i, sample_index) ^ 0x454e564c, discard(4 b), one raw value, three uniforms --
    from the library's generator (ptc_check_rng), against env_light_ref.stream (the oracle's generator)"""
    indices = np.array([0, 1, 63, 64, 4098, 2 ** 31 - 1, 2 ** 32 - 1], dtype=np.uint64)
    for sample_index in (0, 7, 2 ** 31 - 5):
        for bounce in (0, 1, 7):
            seeds = np.array([_hash32(_hash32(int(i)) ^ sample_index) ^ env_light_ref.SEED_XOR for i in indices], dtype=np.uint32)
            # six words per element: state after seed, after discard, two raw values, the bits of two uniforms.  Two elements per
            # index: discard 4 b gives v and the raw value behind u1, discard 4 b + 2 the bits of ... u2, u3 are its raw values'
            first = np.zeros((len(seeds), 6), dtype=np.uint32)
            second = np.zeros((len(seeds), 6), dtype=np.uint32)
            lib = pkg._capi.lib()
            for disc, out in ((4 * bounce, first), (4 * bounce + 2, second)):
                discards = np.full(len(seeds), disc, dtype=np.uint32)
                assert lib.ptc_check_rng(seeds.ctypes.data_as(C.c_void_p), discards.ctypes.data_as(C.c_void_p), len(seeds),
                                         out.ctypes.data_as(C.c_void_p)) == 0
            to_u = lambda raw: ((raw - np.uint32(1)).astype(np.float32) / np.float32(2.0 ** 31)).astype(np.float32)
            v, u = env_light_ref.stream(orc, indices, sample_index, 4 * bounce)
            assert np.array_equal(v, first[:, 2])
            assert np.array_equal(_bits(u[:, 0]), _bits(to_u(first[:, 3])))
            assert np.array_equal(_bits(u[:, 1]), _bits(to_u(second[:, 2]))) and np.array_equal(_bits(u[:, 2]), _bits(to_u(second[:, 3])))
            assert ((v >= 1) & (v <= 2 ** 31 - 2)).all()
    assert env_light_ref.SEED_XOR not in (0x4C495445, 0x52524C54, 0x4C454E53)  # the lamp, roulette and lens streams


def test_unbiased_against_the_quadrature(pkg):
    """The mean of the unshadowed contribution over 16 blocks of 4096 samples (explicit draws from a seeded generator, in the device's
    form: raw / 2^31) against the binary64 quadrature of  integral L cos d omega / pi  (env_light_ref.irradiance_f64).
    |mean difference| <= 4.073 sd / sqrt(16) per channel; the quadrature at grids 384 and 768 agrees to a tenth of that bound."""
    n, blocks, per_block = 8, 16, 4096
    env = sun_map(n, 77)
    normal = np.array([0.3, 0.9, -0.2])
    normal = (normal / np.linalg.norm(normal)).astype(np.float32)
    rng = np.random.default_rng(2024)
    k = blocks * per_block
    v = rng.integers(1, 2 ** 31 - 1, k).astype(np.uint32)
    u = (rng.integers(0, 2 ** 31, (k, 3)).astype(np.float32) / np.float32(2.0 ** 31)).astype(np.float32)
    rc, radiance, _, sampled = _hook(pkg, env, np.zeros((k, 3), np.float32), np.tile(normal, (k, 1)), v, u)
    assert rc == 0 and sampled.any()
    means = radiance.astype(np.float64).reshape(blocks, per_block, 3).mean(axis=1)
    bound = T_BOUND * means.std(axis=0, ddof=1) / np.sqrt(blocks)
    coarse, fine = env_light_ref.irradiance_f64(env, normal, 384), env_light_ref.irradiance_f64(env, normal, 768)
    print("mean", means.mean(axis=0), "quadrature", fine, "bound", bound, "grids differ by", np.abs(coarse - fine))
    assert (np.abs(coarse - fine) <= 0.1 * bound).all()
    assert (np.abs(means.mean(axis=0) - fine) <= bound).all()


def test_the_loop_with_the_option_off_is_env_ref_s(pkg, orc):
    """loop_ref.render_megakernel with env_light given but inert -- off, or on under no environment or a map of weight 0 -- is the loop
    without the option bit for bit; with it under a map with weight only colour differs"""
    w, h = 12, 8
    scene = pkg.scenes.cornell_spheres((w, h))
    flat = scene.build_scene()
    env = sun_map(5, 3)
    entries, _, _ = env_light_ref.table_of(pkg, env)
    zeros = np.zeros((2, 2, 3), dtype=np.float32)
    for e, ent, on in ((env, entries, False), (None, None, True), (zeros, None, True)):
        want = loop_ref.render_megakernel(orc, flat, scene.camera, w, h, 0, 2, 4, env=e, direct=True, roulette=1)
        got = loop_ref.render_megakernel(orc, flat, scene.camera, w, h, 0, 2, 4, env=e, entries=ent, env_light=on, direct=True, roulette=1)
        for k in ("color", "normal", "depth"):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), k
        assert all(got[k] == want[k] for k in ("rays", "diffuse_hits", "shadow_rays", "unoccluded"))
        assert got["env_diffuse_hits"] == 0
    lit = loop_ref.render_megakernel(orc, flat, scene.camera, w, h, 0, 2, 4, env=env, entries=entries, env_light=True, direct=True, roulette=1)
    off = loop_ref.render_megakernel(orc, flat, scene.camera, w, h, 0, 2, 4, env=env, direct=True, roulette=1)
    assert all(np.array_equal(_bits(lit[k]), _bits(off[k])) for k in ("normal", "depth"))
    assert all(lit[k] == off[k] for k in ("rays", "diffuse_hits", "shadow_rays", "unoccluded"))
    assert lit["env_diffuse_hits"] > 0 and lit["env_diffuse_hits"] >= lit["env_shadow_rays"] >= lit["env_unoccluded"]


def test_the_hooks_refuse(pkg):
    lib = pkg._capi.lib()
    env = sun_map(4, 9)
    W, pos = C.c_double(), C.c_uint64()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.ptc_check_environment_light_table(None, 4, None, C.byref(W), C.byref(pos)) == pkg._capi.PTC_ERR_INVALID
    assert lib.ptc_check_environment_light_table(ptr(env), 4, None, None, C.byref(pos)) == pkg._capi.PTC_ERR_INVALID
    assert lib.ptc_check_environment_light_table(ptr(env), 4, None, C.byref(W), None) == pkg._capi.PTC_ERR_INVALID
    for n in (0, 1, 4097):
        assert lib.ptc_check_environment_light_table(ptr(env), n, None, C.byref(W), C.byref(pos)) == pkg._capi.PTC_ERR_INVALID
    assert lib.ptc_check_environment_light_table(ptr(env), 4, None, C.byref(W), C.byref(pos)) == 0 and W.value > 0.0 and pos.value == 16
    for bad in (np.nan, np.inf, -1.0):
        m = env.copy()
        m[2, 1, 0] = bad
        assert lib.ptc_check_environment_light_table(ptr(m), 4, None, C.byref(W), C.byref(pos)) == pkg._capi.PTC_ERR_INVALID
        assert _hook(pkg, m, np.zeros((1, 3)), [[0, 1, 0]], [5], [[0.5, 0.5, 0.5]])[0] == pkg._capi.PTC_ERR_INVALID
    p, nrm, v, u = np.zeros((1, 3), np.float32), np.array([[0, 1, 0]], np.float32), np.array([5], np.uint32), np.full((1, 3), 0.5, np.float32)
    out = np.zeros((1, 3), np.float32)
    call = lambda *a: lib.ptc_check_environment_light(*a)
    assert call(ptr(env), 4, ptr(p), ptr(nrm), ptr(v), ptr(u), 1, ptr(out), None, None) == 0
    assert call(None, 4, ptr(p), ptr(nrm), ptr(v), ptr(u), 1, ptr(out), None, None) == pkg._capi.PTC_ERR_INVALID
    for k in range(2, 8):  # a NULL among points, normals, v, u, radiance (count itself is the integer at 6)
        if k == 6:
            continue
        args = [ptr(env), 4, ptr(p), ptr(nrm), ptr(v), ptr(u), 1, ptr(out), None, None]
        args[k] = None
        assert call(*args) == pkg._capi.PTC_ERR_INVALID, k
    assert call(ptr(env), 4, None, None, None, None, 0, None, None, None) == 0  # nothing asked
    for n in (1, 4097):
        assert call(ptr(env), n, ptr(p), ptr(nrm), ptr(v), ptr(u), 1, ptr(out), None, None) == pkg._capi.PTC_ERR_INVALID
    for raw in (0, 2 ** 31 - 1, 2 ** 32 - 1):  # no raw value of the generator
        assert _hook(pkg, env, p, nrm, [raw], u)[0] == pkg._capi.PTC_ERR_INVALID
    # a map of weight 0: zeros, nothing sampled
    rc, radiance, rays, sampled = _hook(pkg, np.zeros((4, 4, 3), np.float32), p + 1.0, nrm, v, u)
    assert rc == 0 and (radiance == 0.0).all() and sampled[0] == 0 and rays[0].tolist() == [1.0, 1.0, 1.0, np.float32(1e-4), 0.0, 0.0, 0.0, 0.0]


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_PT = os.path.join(ROOT, "cuda-path-tracer_amd", "host", "hip_pt")


def _ensure_cli():
    if not os.path.exists(HIP_PT):
        subprocess.run(["make"], cwd=os.path.dirname(HIP_PT), check=True, stdout=subprocess.DEVNULL)


def test_hip_pt_refuses_the_flag_without_the_megakernel():
    """--environment-light needs --method megakernel: refused while the arguments are read, before any GPU is touched"""
    _ensure_cli()
    for extra in ([], ["--gpus", "2"]):
        r = subprocess.run([HIP_PT, "scenes/spheres_sun.json", "--environment-light"] + extra, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "--environment-light needs --method megakernel" in r.stderr, r.stderr
    r = subprocess.run([HIP_PT, "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert "--environment-light" in r.stdout + r.stderr


def test_the_light_key_in_both_parsers(pkg, tmp_path):
    """"environment": {.., "light": true / false}: optional, a boolean; both readers take it and refuse anything else; the asset scene
    has it, and spheres_sky.json does not"""
    _ensure_cli()
    sun = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "spheres_sun.json"))
    assert sun.environment_source["light"] is True and sun.environment.shape == (32, 32, 3)
    assert float(sun.environment.max()) > 1000.0 * float(np.median(sun.environment))  # a sky with a sun
    assert "light" not in pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "spheres_sky.json")).environment_source
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "environment", "sky_sun.hdr")) < 2048
    base = json.load(open(os.path.join(ROOT, "assets", "scenes", "spheres_sun.json")))
    base["environment"]["file"] = os.path.join(ROOT, "tests", "golden", "environment", "sky_sun.hdr")
    for value, ok in ((True, True), (False, True), (1, False), ("yes", False), (None, False)):
        base["environment"]["light"] = value
        path = str(tmp_path / "scene.json")
        with open(path, "w") as f:
            json.dump(base, f)
        r = subprocess.run([HIP_PT, path, "--dump-environment", str(tmp_path / "x.bin")], capture_output=True, text=True, timeout=120)
        if ok:
            assert pkg.json_parser.scene_from_json(path).environment_source["light"] is value
            assert r.returncode == 0, r.stderr
        else:
            with pytest.raises(ValueError):
                pkg.json_parser.scene_from_json(path)
            assert r.returncode == 1 and "light" in r.stderr, (value, r.stderr)


def test_the_python_field(pkg):
    """PathTracer.environment_light is a switch (bool()) and, called, the query -- no context is needed to hold the switch's value"""
    assert hasattr(pkg.PathTracer, "environment_light") and hasattr(pkg.PathTracer, "environment_light_stats")
    assert hasattr(pkg.PathTracer, "environment_light_loop_stats") and hasattr(pkg.PathTracer, "environment_light_dev")
