"""Multiple importance sampling in the megakernel (ptc_set_param "mis") without a GPU: the library's host build of the
environment sample's density (ptc_check_environment_light_pdf) against the numpy restatement tests/mis_ref.py -- the checker of
tests/test_gpu_mis.py -- bit for bit, on random directions and on the edges; the density of a sample's own direction against the
factor that sample was weighted with; its normalisation; the per-material array (ptc_light_material_pdf) against the lamp table; the two
weights of one point; the numpy loop with the option off and on; the refusals of the hooks and of hip_pt."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import direct_loop_scenes
import env_light_ref
import env_ref
import loop_ref
import mis_ref

SIZES = (2, 5, 64)
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sun_map(n, seed):
    """a seeded random HDR sky in [0.05, 1) with a two-texel sun"""
    m = np.random.default_rng(seed).uniform(0.05, 1.0, (n, n, 3)).astype(np.float32)
    j, i = n // 3, n // 2
    m[j, i] = m[j, min(i + 1, n - 1)] = (5000.0, 4500.0, 4000.0)
    return m


def sparse_map(n, seed):
    """nine texels in ten are zero: squares of weight 0"""
    rng = np.random.default_rng(seed)
    m = rng.uniform(0.0, 10.0, (n, n, 3)).astype(np.float32)
    m[rng.uniform(size=(n, n)) < 0.9] = 0.0
    m[n - 1, 0, 1] = 3.0
    return m


def _pdf_hook(pkg, env, dirs):
    env = np.ascontiguousarray(env, dtype=np.float32)
    dirs = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    out = np.full(len(dirs), -1.0, dtype=np.float32)
    rc = pkg._capi.lib().ptc_check_environment_light_pdf(env.ctypes.data_as(C.c_void_p), env.shape[0], dirs.ctypes.data_as(C.c_void_p), len(dirs),
                                                         out.ctypes.data_as(C.c_void_p))
    return rc, out


def _unit(v):
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)


def direction_set(rng, n, count=4096):
    """`count` random unit directions, then the edges: +- each axis, dy = -0, points of the fold |q_x| + |q_z| = 1 (y = +-0), directions
    next to the four corners of the square (the -y pole), directions on the lines between squares, a zero and a NaN direction"""
    rows = [_unit(rng.standard_normal((count, 3)))]
    rows.append(np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32))
    rows.append(_unit([[0.3, 1.0, 0.7], [-0.6, 1.0, 0.2]]) * np.array([1.0, -0.0, 1.0], dtype=np.float32))  # dy = -0: the upper rule
    t = np.linspace(0.0, 1.0, 33)
    for sx in (1.0, -1.0):
        for sz in (1.0, -1.0):
            for y in (0.0, -0.0):
                fold = np.stack([sx * t, np.full_like(t, y), sz * (1.0 - t)], axis=-1)
                rows.append(_unit(fold) * np.array([1.0, 0.0, 1.0], dtype=np.float32) + np.array([0.0, y, 0.0], dtype=np.float32))
    e = 1e-3
    rows.append(_unit([[e, -1.0, e], [-e, -1.0, e], [e, -1.0, -e], [-e, -1.0, -e], [0.0, -1.0, 0.0]]))
    c = np.arange(1, n) / n * 2.0 - 1.0  # the lines between squares, on the upper sheet
    for q in c[:16]:
        for other in (0.1, -0.35):
            if abs(q) + abs(other) < 1.0:
                rows.append(_unit([[q, 1.0 - abs(q) - abs(other), other], [other, 1.0 - abs(q) - abs(other), q]]))
    rows.append(np.array([[0.0, 0.0, 0.0], [np.nan, 0.5, 0.5], [0.0, np.nan, 0.0], [np.inf, 0.0, 0.0]], dtype=np.float32))
    return np.concatenate([np.asarray(r, dtype=np.float32).reshape(-1, 3) for r in rows])


# ---- 1. the density against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("sun", "sparse"))
@pytest.mark.parametrize("n", SIZES)
def test_host_density_equals_the_restatement(pkg, n, kind):
    env = {"sun": sun_map, "sparse": sparse_map}[kind](n, 40 + n)
    entries, _, _ = env_light_ref.table_of(pkg, env)
    dirs = direction_set(np.random.default_rng(n), n)
    assert len(dirs) >= 4096 + 6
    rc, got = _pdf_hook(pkg, env, dirs)
    want = mis_ref.pdf(entries, n, dirs)
    assert rc == 0
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (n, kind, int(bad.sum()), np.nonzero(bad)[0][:4].tolist())
    assert (got[-4:] == 0.0).all()  # the zero, NaN and infinite directions
    assert np.isfinite(got).all() and (got >= 0.0).all() and (got > 0.0).any()
    if kind == "sparse" and n > 2:
        assert (got[:4096] == 0.0).any()  # squares of weight 0


def test_the_square_of_a_direction(pkg):
    """square_of on the restatement's side: the centre of every square decodes to a direction that falls back into it"""
    for n in SIZES:
        k = np.arange(n * n)
        j, i = k // n, k % n
        w, _ = env_light_ref.decode(((i + F(0.5)) / F(n)).astype(np.float32), ((j + F(0.5)) / F(n)).astype(np.float32))
        ok, qx, qz = mis_ref.project(w)
        assert ok.all() and np.array_equal(mis_ref.square_of(qx, qz, n), k)


# ---- 2. the round trip ------------------------------------------------------------------------------------------------------------------
def _sample_hook(pkg, env, normals, v, u):
    env = np.ascontiguousarray(env, dtype=np.float32)
    k = len(v)
    points = np.zeros((k, 3), dtype=np.float32)
    normals = np.ascontiguousarray(normals, dtype=np.float32)
    v = np.ascontiguousarray(v, dtype=np.uint32)
    u = np.ascontiguousarray(u, dtype=np.float32)
    radiance, rays, sampled = np.zeros((k, 3), np.float32), np.zeros((k, 8), np.float32), np.zeros(k, np.uint8)
    rc = pkg._capi.lib().ptc_check_environment_light(env.ctypes.data_as(C.c_void_p), env.shape[0], points.ctypes.data_as(C.c_void_p),
                                                     normals.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), u.ctypes.data_as(C.c_void_p),
                                                     k, radiance.ctypes.data_as(C.c_void_p), rays.ctypes.data_as(C.c_void_p),
                                                     sampled.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return rays[:, 4:7].copy(), sampled.astype(bool)


def _library_samples(pkg, env, v, u, rng):
    """the directions of ptc_check_environment_light's samples for the draws: about a random normal and about its opposite, whichever
    of the two does not cull"""
    normals = _unit(rng.standard_normal((len(v), 3)))
    w, got = _sample_hook(pkg, env, normals, v, u)
    w2, got2 = _sample_hook(pkg, env, -normals, v, u)
    w[~got] = w2[~got]
    return w, got | got2


@pytest.mark.parametrize("n", SIZES)
def test_the_density_of_a_sample_is_the_factor_it_was_weighted_with(pkg, n):
    """u2, u3 in [1/16, 15/16]: the sample lies a sixteenth of a texel inside its square, orders above binary32 rounding at n <= 64, so
    its direction falls back into that square and the density there is 1 / ((4 f) l^3) of the sample, bit for bit, in every case"""
    env = sun_map(n, 7 * n)
    entries, _, _ = env_light_ref.table_of(pkg, env)
    rng = np.random.default_rng(100 + n)
    count = 8192
    v = rng.integers(1, 2 ** 31 - 1, count).astype(np.uint32)
    u = rng.uniform(1.0 / 16.0, 15.0 / 16.0, (count, 3)).astype(np.float32)
    u[:, 0] = rng.uniform(0.0, 1.0, count).astype(np.float32)
    w, got = _library_samples(pkg, env, v, u, rng)
    assert got.all()
    ref = env_light_ref.sample(entries, env_ref.apron(env), np.zeros((count, 3)), w, v, u)  # (about w itself: nothing culls)
    assert np.array_equal(_bits(ref["w"]), _bits(w))
    jac, _ = mis_ref.env_terms(entries, n, w, ref["square"], u)
    rc, density = _pdf_hook(pkg, env, w)
    assert rc == 0
    bad = _bits(density) != _bits(mis_ref.env_density(jac))
    assert not bad.any(), (n, int(bad.sum()), np.nonzero(bad)[0][:4].tolist())
    assert (density > 0.0).all()


def test_a_sample_on_the_edge_of_its_square_has_one_of_two_densities(pkg):
    """draws exactly 0 and 1.0f: the direction may fall into the neighbour -- the density is that of the sample's own square or of the
    square its direction is located in"""
    n = 5
    env = sun_map(n, 3)
    entries, _, _ = env_light_ref.table_of(pkg, env)
    rng = np.random.default_rng(8)
    ends = np.array([0.0, 1.0], dtype=np.float32)
    v = rng.integers(1, 2 ** 31 - 1, 512).astype(np.uint32)
    u = np.stack([rng.uniform(0, 1, 512), rng.choice(ends, 512), rng.choice(ends, 512)], axis=-1).astype(np.float32)
    w, got = _library_samples(pkg, env, v, u, rng)
    ref = env_light_ref.sample(entries, env_ref.apron(env), np.zeros((512, 3)), w, v, u)
    _, density = _pdf_hook(pkg, env, w)
    l1 = (np.abs(w[:, 0]) + np.abs(w[:, 1])) + np.abs(w[:, 2])
    l3 = (l1 * l1) * l1
    ok, qx, qz = mis_ref.project(w)
    own = mis_ref.env_density((F(4.0) * entries["f"][ref["square"]]) * l3)
    located = mis_ref.env_density((F(4.0) * entries["f"][mis_ref.square_of(qx, qz, n)]) * l3)
    on = got & ok
    assert on.sum() > 400
    assert ((_bits(density) == _bits(own)) | (_bits(density) == _bits(located)))[on].all()


# ---- 3. normalisation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("sun", "sparse"))
@pytest.mark.parametrize("n", SIZES)
def test_the_density_integrates_to_one(pkg, n, kind):
    """per square the density in ds_x ds_z is 1 / f (the Jacobian 4 l^3 cancels) over an area 1 / n^2: sum 1 / (f n^2) = 1"""
    env = {"sun": sun_map, "sparse": sparse_map}[kind](n, 9 + n)
    entries, _, _ = env_light_ref.table_of(pkg, env)
    f = entries["f"].astype(np.float64)
    assert abs((1.0 / (f[f > 0.0] * n * n)).sum() - 1.0) <= 1e-6


# ---- 4. the per-material array ------------------------------------------------------------------------------------------------------------
def _lamp_scenes(pkg):
    import direct_ref
    return {"cornell_lit": pkg.scenes.cornell_lit(resolution=(16, 12), with_mesh=True), "dark_lamps": direct_ref.dark_lamp_scene(pkg),
            "two_instances": direct_ref.two_instance_scene(pkg), "small_lamp_room": direct_loop_scenes.small_lamp_room(pkg),
            "no_lamps": pkg.scenes.cornell_spheres((16, 12))}


def test_the_material_array_against_the_lamp_table(pkg):
    """every record's inv_pdf is its material's entry, exactly; materials that are not emissive and emissive ones of lum 0 give 0; the
    restatement agrees bit for bit"""
    seen_dark = False
    for name, scene in _lamp_scenes(pkg).items():
        flat = scene.build_scene()
        recs, info = pkg.light_table(flat)
        per_material = pkg.light_material_pdf(flat)
        materials = np.asarray(flat.materials)
        assert len(per_material) == len(materials)
        m_of = (recs["kind_material"] & 0x7FFFFFFF).astype(np.int64)
        assert np.array_equal(_bits(recs["inv_pdf"]), _bits(per_material[m_of])), name
        for m, mat in enumerate(materials):
            lum = max(mat["p"][0], mat["p"][1], mat["p"][2])
            if mat["type"] != 3 or lum == 0.0 or not info["total_weight"] > 0.0:
                assert per_material[m] == 0.0, (name, m)
                seen_dark |= mat["type"] == 3
            else:
                assert per_material[m] == F(info["total_weight"] / float(lum)), (name, m)
        assert np.array_equal(_bits(per_material), _bits(mis_ref.material_pdf(flat))), name
    assert seen_dark


def test_the_material_array_refuses(pkg):
    flat = pkg.scenes.cornell_lit(resolution=(16, 12)).build_scene()
    desc = flat.to_c()
    lib, inv = pkg._capi.lib(), pkg._capi.PTC_ERR_INVALID
    out = np.zeros(len(flat.materials), dtype=np.float32)
    assert lib.ptc_light_material_pdf(None, out.ctypes.data, len(out)) == inv
    assert lib.ptc_light_material_pdf(C.byref(desc), None, len(out)) == inv
    assert lib.ptc_light_material_pdf(C.byref(desc), out.ctypes.data, len(out) - 1) == inv and b"capacity" in lib.ptc_last_error(None)
    assert lib.ptc_light_material_pdf(C.byref(desc), out.ctypes.data, len(out)) == len(out)
    with pytest.raises(pkg.PtcError):
        pkg.light_material_pdf(flat, capacity=1)


# ---- 5. the two weights of one point --------------------------------------------------------------------------------------------------------
def test_the_two_weights_of_one_point_sum_to_one():
    """from identical d^2, cosines and densities: the light sample's weight and the continuation ray's sum to 1 within 1e-6 (a sum, a
    divide and the density's own roundings on each side); with one density 0 the other side's weight is exactly 1"""
    rng = np.random.default_rng(5)
    k = 4096
    d2 = np.exp(rng.uniform(-8, 8, k)).astype(np.float32)
    cos_l, cos_r = rng.uniform(1e-3, 1.0, k).astype(np.float32), rng.uniform(1e-3, 1.0, k).astype(np.float32)
    inv_pdf = np.exp(rng.uniform(-3, 6, k)).astype(np.float32)
    p_l, p_b = mis_ref.lamp_density(d2, cos_l, inv_pdf), mis_ref.lobe_density(cos_r)
    total = mis_ref.balance(p_l, p_b).astype(np.float64) + mis_ref.balance(p_b, p_l).astype(np.float64)
    assert np.abs(total - 1.0).max() <= 1e-6
    jac = np.exp(rng.uniform(-6, 6, k)).astype(np.float32)
    p_e = mis_ref.env_density(jac)
    total = mis_ref.balance(p_e, p_b).astype(np.float64) + mis_ref.balance(p_b, p_e).astype(np.float64)
    assert np.abs(total - 1.0).max() <= 1e-6
    zero = np.zeros(k, dtype=np.float32)
    assert (mis_ref.balance(p_b, zero) == 1.0).all() and (mis_ref.balance(p_l, zero) == 1.0).all()
    assert (mis_ref.balance(zero, p_b) == 0.0).all()
    assert (mis_ref.balance(p_b, mis_ref.lamp_density(d2, cos_l, zero)) == 1.0).all()  # inv_pdf_m 0: the hit counts fully
    assert (mis_ref.balance(p_b, mis_ref.lamp_density(d2, zero, inv_pdf)) == 1.0).all()  # a zero cosine
    assert (mis_ref.balance(p_b, mis_ref.env_density(F(4.0) * zero)) == 1.0).all()  # f == 0
    assert (mis_ref.balance(zero, zero) == 1.0).all() and np.isfinite(mis_ref.balance(F(np.inf), p_b)).all()
    assert (mis_ref.lobe_density(-cos_r) == 0.0).all() and mis_ref.lobe_density(F(np.nan)) == 0.0


# ---- 6. the loop --------------------------------------------------------------------------------------------------------------------------
W, H = 12, 8
SIX = ("diffuse_hits", "shadow_rays", "unoccluded", "env_diffuse_hits", "env_shadow_rays", "env_unoccluded")
_cache = {}


def _room(pkg):
    """cornell_lit with the right wall out, under a sky with a low sun: lamps, emitters hit by continuation rays, and misses"""
    if "room" not in _cache:
        scene = pkg.scenes.cornell_lit(resolution=(W, H), with_mesh=True)
        at = scene.objects_material_mapping_.index("right")
        del scene.objects_[at], scene.objects_material_mapping_[at]
        scene.camera = pkg.scenes._camera_from_look_at((-1.2, 0.0, 4.0), (0.6, -0.1, 0.0), vfov_deg=50.0)
        env = sun_map(7, 6)
        _cache["room"] = (scene, scene.build_scene(), env, env_light_ref.table_of(pkg, env)[0])
    return _cache["room"]


def test_the_loop_with_the_option_off_is_env_light_ref_s(pkg, orc):
    scene, flat, env, entries = _room(pkg)
    for kw in (dict(env=env, entries=entries, env_light=True, direct=True, roulette=1), dict(env=env, entries=entries, env_light=True),
               dict(direct=True), dict(env=env, entries=entries, direct=True, lens=(0.25, 3.5))):
        want = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 0, 2, 4, **kw)
        got = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 0, 2, 4, mis=False, **kw)
        for k in ("color", "normal", "depth"):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (k, sorted(kw))
        assert all(got[k] == want[k] for k in ("rays",) + SIX)
        assert got["mis_emitter_hits"] == 0 and got["mis_misses"] == 0


def test_the_parameter_with_neither_light_in_effect_changes_nothing(pkg, orc):
    """mis with no light parameter, with "environment_light" under a map of weight 0 and with "direct_light" in a scene without lamps:
    the bits of mis 0"""
    scene, flat, env, entries = _room(pkg)
    bare = pkg.scenes.cornell_spheres((W, H))
    cases = ((scene, flat, dict(env=env, entries=entries)), (scene, flat, dict(env=np.zeros((4, 4, 3), np.float32), entries=None, env_light=True)),
             (bare, bare.build_scene(), dict(direct=True)))
    for sc, fl, kw in cases:
        off = loop_ref.render_megakernel(orc, fl, sc.camera, W, H, 0, 2, 4, mis=False, **kw)
        on = loop_ref.render_megakernel(orc, fl, sc.camera, W, H, 0, 2, 4, mis=True, **kw)
        assert all(np.array_equal(_bits(on[k]), _bits(off[k])) for k in ("color", "normal", "depth"))
        assert all(on[k] == off[k] for k in ("rays", "mis_emitter_hits", "mis_misses") + SIX)


@pytest.mark.parametrize("mb", [1, 2, 5])
def test_the_loop_with_the_option_on_changes_colour_alone(pkg, orc, mb):
    """the same normal, depth, rays and six counters; another colour from two bounces on -- with one bounce every diffuse hit is at the
    last bounce and keeps weight 1: the same colour too"""
    scene, flat, env, entries = _room(pkg)
    kw = dict(env=env, entries=entries, env_light=True, direct=True)
    off = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 0, 3, mb, mis=False, **kw)
    on = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 0, 3, mb, mis=True, **kw)
    assert all(np.array_equal(_bits(on[k]), _bits(off[k])) for k in ("normal", "depth"))
    assert all(on[k] == off[k] for k in ("rays",) + SIX)
    assert np.isfinite(on["color"]).all() and (on["color"] >= 0.0).all()
    if mb == 1:
        assert np.array_equal(_bits(on["color"]), _bits(off["color"]))
        assert on["mis_emitter_hits"] == 0 and on["mis_misses"] == 0
    else:
        assert not np.array_equal(_bits(on["color"]), _bits(off["color"]))
        assert on["mis_misses"] > 0
    if mb == 5:
        assert on["mis_emitter_hits"] > 0


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_the_density_hook_refuses(pkg):
    lib, inv = pkg._capi.lib(), pkg._capi.PTC_ERR_INVALID
    env = sun_map(4, 9)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    dirs, out = np.array([[0.0, 1.0, 0.0]], np.float32), np.zeros(1, np.float32)
    assert lib.ptc_check_environment_light_pdf(ptr(env), 4, ptr(dirs), 1, ptr(out)) == 0 and out[0] > 0.0
    assert lib.ptc_check_environment_light_pdf(None, 4, ptr(dirs), 1, ptr(out)) == inv
    assert lib.ptc_check_environment_light_pdf(ptr(env), 4, None, 1, ptr(out)) == inv
    assert lib.ptc_check_environment_light_pdf(ptr(env), 4, ptr(dirs), 1, None) == inv
    assert lib.ptc_check_environment_light_pdf(ptr(env), 4, None, 0, None) == 0
    for n in (0, 1, 4097):
        assert lib.ptc_check_environment_light_pdf(ptr(env), n, ptr(dirs), 1, ptr(out)) == inv
    for bad in (np.nan, np.inf, -1.0):
        m = env.copy()
        m[1, 2, 0] = bad
        assert lib.ptc_check_environment_light_pdf(ptr(m), 4, ptr(dirs), 1, ptr(out)) == inv
    rc, zeros = _pdf_hook(pkg, np.zeros((4, 4, 3), np.float32), dirs)  # a map of weight 0
    assert rc == 0 and zeros[0] == 0.0


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_PT = os.path.join(ROOT, "cuda-path-tracer_amd", "host", "hip_pt")


def test_hip_pt_refuses_the_flag_without_what_it_needs():
    """--mis needs --method megakernel (refused while the arguments are read) and a light that is sampled -- --direct-light,
    --environment-light or the scene's "light": true (refused when the scene has been read): before any GPU is touched"""
    if not os.path.exists(HIP_PT):
        subprocess.run(["make"], cwd=os.path.dirname(HIP_PT), check=True, stdout=subprocess.DEVNULL)
    run = lambda args: subprocess.run([HIP_PT] + args, cwd=ROOT, capture_output=True, text=True, timeout=120)
    for extra in ([], ["--gpus", "2"], ["--direct-light"]):
        r = run(["scenes/spheres_sun.json", "--mis"] + extra)
        assert r.returncode == 1 and "needs --method megakernel" in r.stderr, r.stderr
    for extra in ([], ["--gpus", "2"]):
        r = run(["scenes/cornell_lit.json", "--mis", "--method", "megakernel"] + extra)  # no flag, no "light" key
        assert r.returncode == 1 and "--mis needs --direct-light" in r.stderr, r.stderr
    r = run(["--help"])
    assert "--mis" in r.stdout + r.stderr


def test_the_python_fields(pkg):
    assert isinstance(pkg.PathTracer.mis, property)
    assert hasattr(pkg.PathTracer, "mis_loop_stats") and hasattr(pkg.PathTracer, "environment_light_pdf")
    assert hasattr(pkg.PathTracer, "environment_light_pdf_dev") and callable(pkg.light_material_pdf)
