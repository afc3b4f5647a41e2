"""Normal maps without a GPU (ptc_normal_map_decode_table, ptc_check_normal_map, ptc_check_megakernel_instance2): the
decode table against its formula, the host twin of the rule against the numpy restatement tests/normal_map_ref.py bit for bit and
against a float64 evaluation, the instance rule with its tenth fact against a table held as data, and the restatement's loop against
the loop it extends."""
import ctypes as C
import itertools

import numpy as np
import pytest

import env_light_ref
import loop_ref
import normal_map_ref
import smooth_ref
import texture_ref
from normal_map_ref import BENT, FLAT, KEPT

ENV = smooth_ref.ENV
W, H = 33, 17
E = 2.0 ** -24
IDENTITY = np.eye(4, dtype=np.float32).reshape(16)
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the table ------------------------------------------------------------------------------------------------------------------------
def test_the_table_at_its_exact_entries_and_monotone(pkg):
    t = pkg.normal_map_decode_table()
    assert t[0] == -1.0 and t[1] == -1.0 and t[128] == 0.0 and t[255] == 1.0
    assert t[127] == np.float32(-1.0) / np.float32(127.0) and t[129] == np.float32(1.0) / np.float32(127.0)
    assert not np.signbit(t[128]) and (np.diff(t[1:]) > 0).all() and (np.diff(t) >= 0).all()
    assert np.array_equal(_bits(t), _bits(normal_map_ref.decode_table()))
    assert np.array_equal(t[129:], -t[127:0:-1])  # byte 256 - k is exactly the negative of byte k
    assert pkg.lib().ptc_normal_map_decode_table(None) == pkg._capi.PTC_ERR_INVALID


# ---- 2. the host twin against the restatement ----------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


def _matrix(pkg):
    """a non-uniformly scaled and rotated object matrix, column-major"""
    glm = pkg.glmlite
    return np.asarray(glm.compose([glm.scale((0.5, 1.7, 0.9)), glm.rotate(0.7, (0.3, 1.0, 0.2)), glm.translate((0.4, -0.2, 1.1))]),
                      dtype=np.float32).reshape(4, 4)


def _cases(n, seed, m44=None, tilt=0.0, lo=-1.5, hi=2.5):
    """n random hits: a triangle, its corners' pairs, barycentrics, and g, b, d in the world of the column-major matrix m44 (None:
    identity) -- g the world triangle's normal turned to the ray, b = g tilted by up to `tilt`, d towards the surface"""
    rng = np.random.default_rng(seed)
    m = np.eye(4) if m44 is None else np.asarray(m44, dtype=np.float64).T  # row-major 4 x 4: x' = m @ x
    p = rng.uniform(-1.0, 1.0, (n, 3, 3))
    st = rng.uniform(lo, hi, (n, 3, 2))
    u = rng.uniform(0.0, 1.0, n)
    v = rng.uniform(0.0, 1.0, n) * (1.0 - u)
    e1, e2 = (p[:, 1] - p[:, 0]) @ m[:3, :3].T, (p[:, 2] - p[:, 0]) @ m[:3, :3].T
    g = _unit(np.cross(e1, e2))
    d = _unit(-g + 0.8 * _unit(rng.standard_normal((n, 3))))
    b = _unit(g + tilt * _unit(rng.standard_normal((n, 3))))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(p0=f(p[:, 0]), p1=f(p[:, 1]), p2=f(p[:, 2]), st0=f(st[:, 0]), st1=f(st[:, 1]), st2=f(st[:, 2]), u=f(u), v=f(v),
                m16=f(np.eye(4) if m44 is None else m44).reshape(16), b=f(b), g=f(g), d=f(d))


def _both(pkg, tex, c, what):
    """the library's host twin and the restatement on the cases c: equal bits, equal outcomes -> (n, outcome)"""
    got, how = pkg.check_normal_map(tex, **c)
    want, whow = normal_map_ref.shade(tex, **c)
    assert np.array_equal(how, whow), (what, np.argwhere(how != whow)[:4].tolist())
    assert np.array_equal(_bits(got), _bits(want)), (what, np.argwhere(_bits(got) != _bits(want))[:4].tolist())
    return got, how


def _constant(pkg, rgb, filt="nearest", width=2, height=2):
    t = np.zeros((height, width, 4), dtype=np.uint8)
    t[...] = tuple(rgb) + (7,)
    return pkg.Texture(t, "srgb", filt, "repeat")  # (the encoding is not read)


@pytest.mark.parametrize("width,height", [(1, 1), (2, 2), (3, 5), (4096, 2)])
def test_the_rule_against_the_restatement(pkg, width, height):
    """every filter x wrap x encoding on random maps, under a non-uniformly scaled and rotated matrix, b tilted off g"""
    seen = set()
    for filt in ("nearest", "bilinear"):
        for wrap in ("repeat", "clamp"):
            for enc in ("linear", "srgb"):
                tex = texture_ref.random_texture(pkg, width, height, 5 * width + height, encoding=enc, filter=filt, wrap=wrap)
                c = _cases(257, width + 3 * height, _matrix(pkg), tilt=0.3)
                seen |= set(_both(pkg, tex, c, (filt, wrap, enc))[1].tolist())
    assert BENT in seen and KEPT in seen  # (uniform random bytes: half the texels point into the surface)


def test_4096_random_cases_and_every_outcome(pkg):
    tex = normal_map_ref.bumpy_map(pkg, 7, 5, filter="bilinear", wrap="repeat")
    c = _cases(4096, 17, _matrix(pkg), tilt=0.4)
    c["st0"][::31] = c["st1"][::31] = c["st2"][::31] = np.float32([0.03, 0.04])  # inside texel (0, 0), the flat one, under nearest
    near = pkg.Texture(tex.rgba8, "linear", "nearest", "repeat")
    counts = {}
    for t in (tex, near):
        n, how = _both(pkg, t, c, "random")
        for k in (BENT, FLAT, KEPT):
            counts[k] = counts.get(k, 0) + int((how == k).sum())
        moved = (_bits(n) != _bits(c["b"])).any(axis=1)
        assert (moved <= (how == BENT)).all()  # flat and kept: b's own bits
        l = np.linalg.norm(n[how == BENT].astype(np.float64), axis=1)
        assert np.abs(l - 1.0).max() < 4 * E
    assert all(counts[k] > 0 for k in (BENT, FLAT, KEPT)), counts
    assert counts[BENT] > 4096


@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
def test_the_flat_texel_gives_the_bits_of_b(pkg, filt):
    c = _cases(300, 5, _matrix(pkg), tilt=0.5)
    c["st0"][::3] = np.nan  # ... but a refused coordinate is kept, not flat
    n, how = _both(pkg, _constant(pkg, (128, 128, 255), filt, 3, 2), c, "flat")
    refused = np.isnan(c["st0"]).any(axis=1)
    assert (how[~refused] == FLAT).all() and (how[refused] == KEPT).all() and np.array_equal(_bits(n), _bits(c["b"]))


def test_special_texels(pkg):
    c = _cases(300, 6, None, tilt=0.0)
    _, how = _both(pkg, _constant(pkg, (0, 0, 0)), c, "000")
    assert (how == KEPT).all()  # (-1, -1, -1): dot(n, g) = -1 / sqrt 3
    n, how = _both(pkg, _constant(pkg, (128, 128, 0)), c, "into the surface")
    assert (how == KEPT).all() and np.array_equal(_bits(n), _bits(c["b"]))  # n = -b: step 8
    tilted = _cases(300, 6, None, tilt=0.4)
    _, how = _both(pkg, _constant(pkg, (255, 128, 128)), tilted, "the tangent itself")
    assert BENT in how and KEPT in how  # n = T, at right angles to b: on g's side for some tilts
    _, how = _both(pkg, _constant(pkg, (128, 128, 128)), c, "no length")
    assert (how == KEPT).all()  # (0, 0, 0): step 7's length test


def test_degenerate_mirrored_and_non_finite_coordinates(pkg):
    tex = normal_map_ref.bumpy_map(pkg, 7, 5, filter="bilinear")
    c = _cases(600, 8, _matrix(pkg), tilt=0.2)
    c["st1"][0:100] = c["st2"][0:100] = c["st0"][0:100]  # the corners share one pair: det == 0
    c["st2"][100:200] = c["st0"][100:200] + 2 * (c["st1"][100:200] - c["st0"][100:200])  # collinear pairs: det == 0 but for rounding
    c["st0"][200:250, 0] = np.nan
    c["st1"][250:300, 1] = np.inf
    c["st2"][300:350, 0] = -np.inf
    c["st0"][350:400] = np.float32(3e38)  # finite corners whose differences are not
    n, how = _both(pkg, tex, c, "degenerate")
    assert (how[0:100] == KEPT).all() and (how[200:350] == KEPT).all() and np.array_equal(_bits(n[:100]), _bits(c["b"][:100]))
    assert (how[400:] == BENT).sum() > 100
    mirrored = {k: v.copy() for k, v in c.items()}
    for k in ("st0", "st1", "st2"):
        mirrored[k][:, 0] = np.float32(1.0) - mirrored[k][:, 0]
    _, mhow = _both(pkg, tex, mirrored, "mirrored")
    assert (mhow[400:] == BENT).sum() > 100


def test_a_grazing_ray_is_refused_by_step_8(pkg):
    """d nearly in the surface: it still meets g and b from the front, and the bent normal from behind"""
    c = _cases(500, 9, None, tilt=0.0)
    tex = _constant(pkg, (228, 228, 200))  # leans about 45 degrees off the axis
    side = _unit(np.cross(c["g"].astype(np.float64), np.random.default_rng(1).standard_normal((500, 3))))
    lean = _unit(side - 0.05 * c["g"])
    c["d"] = np.ascontiguousarray(lean, dtype=np.float32)
    n, how = _both(pkg, tex, c, "grazing")
    assert (how == KEPT).sum() > 50 and (how == BENT).sum() > 50
    assert np.array_equal(_bits(n[how == KEPT]), _bits(c["b"][how == KEPT]))


# ---- 3. a float64 cross-check ------------------------------------------------------------------------------------------------------------
def _sheet_case(order=(0, 1, 2), mirror=False):
    """the unit sheet z = 0 with s = x, t = y (mirror: s = 1 - x) under the identity, seen from +z; the corners in the given order"""
    p = np.float32([(0, 0, 0), (1, 0, 0), (0, 1, 0)])[list(order)]
    st = p[:, :2].copy()
    if mirror:
        st[:, 0] = 1.0 - st[:, 0]
    up = np.float32([[0, 0, 1]])
    return dict(p0=p[0:1], p1=p[1:2], p2=p[2:3], st0=st[0:1], st1=st[1:2], st2=st[2:3], u=np.float32([0.25]), v=np.float32([0.5]), m16=IDENTITY,
                b=up, g=up, d=np.float32([[0.0, 0.0, -1.0]]))


# The bound, from the rule's operations on this sheet, with e = 2^-24:
#   - a table entry is one rounding of (k - 128) / 127 (the subtraction is exact): c (1 + e);
#   - the tangent frame is exact: edges, coordinate differences and det are 0 or +-1, T = (+-1, 0, 0), k = 0, normalize multiplies by
#     1 / sqrt(1) = 1, C and B are (0, +-1, 0); T x + B y + b z adds zeros: a = (x, y, z), the table's entries themselves;
#   - l2 = dot(a, a): three products and two sums of terms >= 0, each term passing through at most three roundings: l2 (1 + 3 e);
#   - the square root halves that and rounds: 2.5 e; 1 / it: 3.5 e; the product with a component: 4.5 e -- relative to the normalised
#     table entries;
#   - against the normalised exact entries: the component's own e and the norm's e: 2 e more.
# Together 6.5 e relative (and terms in e^2) on components of magnitude at most 1: 7 e.
F64_BOUND = 7 * E
TEXELS = [(128, 128, 255), (200, 128, 255), (128, 30, 200), (255, 255, 255), (1, 255, 129), (37, 201, 180), (250, 5, 132)]


def _f64_normal(rgb, flip_x=False):
    a = np.maximum((np.float64(rgb) - 128.0) / 127.0, -1.0)
    if flip_x:
        a[0] = -a[0]
    return a / np.sqrt((a * a).sum())


def test_a_constant_texel_on_a_flat_sheet_against_float64(pkg):
    for rgb in TEXELS:
        n, how = _both(pkg, _constant(pkg, rgb), _sheet_case(), rgb)
        want = _f64_normal(rgb)
        err = np.abs(n[0].astype(np.float64) - want).max()
        print("constant texel vs float64", rgb, "error", err, "bound", F64_BOUND)
        assert how[0] == (FLAT if rgb[:2] == (128, 128) else BENT) and err <= F64_BOUND


def test_mirrored_against_unmirrored_mapping(pkg):
    """The same sheet and picture with its corners listed the other way round (det < 0, the same mapping): the same n.  The mapping
    itself mirrored, s = 1 - x, turns the tangent about: the same n from the picture with x negated (byte 256 - k), up to that bound."""
    for rgb in TEXELS:
        tex = _constant(pkg, rgb)
        n, _ = _both(pkg, tex, _sheet_case(), rgb)
        for order in ((0, 2, 1), (1, 0, 2), (2, 1, 0)):
            c = _sheet_case(order)
            ds = (c["st1"][0, 0] - c["st0"][0, 0]) * (c["st2"][0, 1] - c["st0"][0, 1]) - (c["st2"][0, 0] - c["st0"][0, 0]) * (c["st1"][0, 1] - c["st0"][0, 1])
            assert ds < 0
            other, _ = _both(pkg, tex, c, (rgb, order))
            assert np.abs(other.astype(np.float64) - n.astype(np.float64)).max() <= F64_BOUND, (rgb, order)
        if rgb[0] >= 1:
            turned = _constant(pkg, (256 - rgb[0] if rgb[0] > 1 else 255, rgb[1], rgb[2]))
            m, mhow = _both(pkg, turned, _sheet_case(mirror=True), (rgb, "mirror"))
            assert np.abs(m.astype(np.float64) - n.astype(np.float64)).max() <= F64_BOUND, (rgb, "mirror")
            m, _ = _both(pkg, tex, _sheet_case(mirror=True), (rgb, "mirror, same picture"))
            assert np.abs(m[0].astype(np.float64) - _f64_normal(rgb, flip_x=True)).max() <= F64_BOUND


def test_check_normal_map_refusals(pkg):
    c = _cases(4, 1)
    tex = _constant(pkg, (128, 128, 255))
    fn, invalid = pkg.lib().ptc_check_normal_map, pkg._capi.PTC_ERR_INVALID
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    out, how = np.zeros((4, 3), np.float32), np.zeros(4, np.uint8)
    args = [ptr(c[k]) for k in ("p0", "p1", "p2", "st0", "st1", "st2", "u", "v", "m16", "b", "g", "d")]
    d = tex._desc()
    assert fn(C.byref(d), *args, 4, ptr(out), ptr(how)) == 0
    assert fn(None, *args, 4, ptr(out), ptr(how)) == invalid and fn(C.byref(d), *args, 4, None, ptr(how)) == invalid
    for k in range(len(args)):
        assert fn(C.byref(d), *(args[:k] + [None] + args[k + 1:]), 4, ptr(out), ptr(how)) == invalid, k
    d.width = 4097
    assert fn(C.byref(d), *args, 4, ptr(out), ptr(how)) == invalid
    with pytest.raises(ValueError):
        pkg.check_normal_map(tex, **{**c, "u": c["u"][:-1]})
    # what ptc_set_normal_maps and its getter answer without a context
    assert pkg.lib().ptc_set_normal_maps(None, None, 0) == invalid and pkg.lib().ptc_get_normal_maps(None, None) == 0
    assert pkg.lib().ptc_hit_shading_normal(None, None, 0, None, None) == invalid and pkg.lib().ptc_get_normal_map_loop_stats(None, None) == invalid


# ---- 4. the instance rule with its tenth fact -----------------------------------------------------------------------------------------------
FACTS = ("direct", "env", "env_lit", "smooth", "textured", "weigh", "lens", "plays", "emitters", "bent")
INT_MAX = 2 ** 31 - 1
# (the fact that decides, the other facts it needs, kernel, the facts that are its template arguments): the first row that holds
TABLE = [
    ("bent", (), "k_megakernel_nmap", ("weigh", "smooth")),
    ("textured", (), "k_megakernel_tex", ("weigh", "smooth")),
    ("smooth", (), "k_megakernel_smooth", ("weigh",)),
    ("weigh", (), "k_megakernel_mis", ()),
    ("env_lit", (), "k_megakernel_env_light", ()),
    ("env", (), "k_megakernel_env", ("direct",)),
    ("direct", ("lens",), "k_megakernel_direct_lens", ("plays",)),
    ("direct", (), "k_megakernel_direct", ("plays",)),
    ("lens", (), "k_megakernel_lens", ("emitters", "plays")),
    (None, (), "k_megakernel", ("emitters", "plays")),
]


def _expected(f):
    for row, (fact, more, kernel, args) in enumerate(TABLE):
        if (fact is None or f[fact]) and all(f[m] for m in more):
            return row, kernel + ("<%s>" % ", ".join("true" if f[a] else "false" for a in args) if args else "")
    raise AssertionError("the table is total")


def test_all_1024_combinations(pkg):
    seen = {}
    for bits in itertools.product((False, True), repeat=len(FACTS)):
        f = dict(zip(FACTS, bits))
        row, want = _expected(f)
        got, arg = pkg.check_megakernel_instance2(roulette=2, max_bounces=8, **f)
        assert got == want and arg == (2 if f["plays"] else INT_MAX), (f, got, want, arg)
        seen.setdefault(got, set()).add(row)
        if not f["bent"]:  # the old checker is the new one with the fact false
            old = {k: v for k, v in f.items() if k != "bent"}
            assert pkg.check_megakernel_instance(roulette=2, max_bounces=8, **old) == (got, arg), f
    assert len(seen) == 26 and all(len(rows) == 1 for rows in seen.values()), seen
    assert sum(2 ** len(args) for _, _, _, args in TABLE) == 26


def test_the_second_checker_refuses_as_the_first(pkg):
    fn, invalid = pkg.lib().ptc_check_megakernel_instance2, pkg._capi.PTC_ERR_INVALID
    name, arg = C.create_string_buffer(64), C.c_int(0)
    assert fn(*([0] * 12), None, 64, C.byref(arg)) == invalid and fn(*([0] * 12), name, 64, None) == invalid
    bent = [0] * 9 + [1, 0, 8]
    assert fn(*bent, name, len("k_megakernel_nmap<false, false>"), C.byref(arg)) == invalid  # no room for the terminator
    assert fn(*bent, name, len("k_megakernel_nmap<false, false>") + 1, C.byref(arg)) == 0 and name.value == b"k_megakernel_nmap<false, false>"


# ---- 5. the loop restatement -------------------------------------------------------------------------------------------------------------
def _sheet(pkg):
    if "sheet" not in _cache:
        scene = smooth_ref.sheet_scene(pkg, ("diffuse", "metal"))
        flat = scene.build_scene(distinct_meshes=True)
        textures = texture_ref.pool(pkg) + [normal_map_ref.bumpy_map(pkg), normal_map_ref.flat_map(pkg)]
        binding = texture_ref.bind(scene, flat, {"sheet": 0, "diffuse": 1, "metal": 2, "floor": 1})
        bumpy = texture_ref.bind(scene, flat, {"sheet": 3, "diffuse": 3, "metal": 3, "floor": 3})
        _cache["sheet"] = dict(scene=scene, flat=flat, textures=textures, binding=binding, bumpy=bumpy, flat_binding=np.where(bumpy >= 0, 4, -1),
                               st=texture_ref.random_texcoords(flat), nrm=smooth_ref.scene_vertex_normals(flat))
    return _cache["sheet"]


def _lights(pkg, lights):
    if lights == "none":
        return {}
    return dict(env=ENV, entries=env_light_ref.table_of(pkg, ENV)[0], env_light=True, mis=lights == "env_mis")


def test_loop_off_is_the_loop_it_extends(pkg, orc):
    s = _sheet(pkg)
    kw = dict(textures=s["textures"], binding=s["binding"], texcoords=s["st"], textured=True, normals=s["nrm"], smooth=True, **_lights(pkg, "env"))
    want = loop_ref.render_megakernel(orc, s["flat"], s["scene"].camera, W, H, 0, 1, 4, pkg=pkg, **kw)
    unbound = np.full(len(s["bumpy"]), -1, np.int32)
    for nm in (dict(nbinding=s["bumpy"], normal_maps=False), dict(nbinding=None, normal_maps=True), dict(nbinding=unbound, normal_maps=True)):
        got = loop_ref.render_megakernel(orc, s["flat"], s["scene"].camera, W, H, 0, 1, 4, pkg=pkg, **nm, **kw)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        assert all(got[k] == 0 for k in normal_map_ref.COUNTERS)


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("lights", ["none", "env_mis"])
def test_an_all_flat_map_gives_the_bits_of_the_loop_it_extends(pkg, orc, smooth, lights):
    """every texel (128, 128, 255): the loop with the option on walks to the bits of the loop without it -- a flat texel leaves the
    normal, the culls and the absorption where they were"""
    s = _sheet(pkg)
    kw = dict(textures=s["textures"], binding=s["binding"], texcoords=s["st"], textured=True, normals=s["nrm"], smooth=smooth, **_lights(pkg, lights))
    want = loop_ref.render_megakernel(orc, s["flat"], s["scene"].camera, W, H, 0, 1, 4, pkg=pkg, **kw)
    got = loop_ref.render_megakernel(orc, s["flat"], s["scene"].camera, W, H, 0, 1, 4, nbinding=s["flat_binding"], normal_maps=True, pkg=pkg, **kw)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert got["bent"] == 0 and got["kept"] == 0 and got["lookups"] > 0


def test_a_bumpy_map_changes_the_colour_alone_and_both_counters_move(pkg, orc):
    s = _sheet(pkg)
    bad = s["st"].copy()
    bad[::7, 0] = np.nan
    kw = dict(textures=s["textures"], binding=s["binding"], texcoords=bad, textured=False, **_lights(pkg, "env"))
    off = loop_ref.render_megakernel(orc, s["flat"], s["scene"].camera, 65, 33, 0, 1, 8, pkg=pkg, **kw)
    on = loop_ref.render_megakernel(orc, s["flat"], s["scene"].camera, 65, 33, 0, 1, 8, nbinding=s["bumpy"], normal_maps=True, pkg=pkg, **kw)
    assert (on["color"] != off["color"]).any()
    assert np.array_equal(on["normal"], off["normal"]) and np.array_equal(on["depth"], off["depth"])
    assert on["bent"] > 0 and on["kept"] > 0 and on["lookups"] == 0, {k: on[k] for k in normal_map_ref.COUNTERS}
    assert on["absorbed"] + on["culled_light_samples"] > 0  # below the geometry, without smooth shading


# ---- 6. the readers: the scene keys ---------------------------------------------------------------------------------------------------------
import json  # noqa: E402
import os  # noqa: E402
import sys  # noqa: E402

import test_texture_cpu as texture_cpu  # noqa: E402  (its OBJ with a seam, its hip_pt runner, its reader of the dump up to the textures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXTURES = os.path.join(ROOT, "tests", "golden", "textures")


def _scene_json(path, obj, materials, extra=None):
    """a scene file at `path`: one mesh object per material {name: (type, texture or None, normal_map or None)}, files named relative to it"""
    rel = lambda p: os.path.relpath(p, os.path.dirname(path))
    j = {"camera": {"vfov": 45, "resolution": [16, 8]}, "materials": [], "surfaces": []}
    for name, (kind, tex, nmap) in materials.items():
        m = {"type": kind, "name": name}
        m.update({"albedo": [0.5, 0.5, 0.5]} if kind in ("lambertian", "metal") else {"refraction_index": 1.5})
        if kind == "metal":
            m["fuzz"] = 0.1
        for key, value in (("texture", tex), ("normal_map", nmap)):
            if value is not None:
                m[key] = dict(value, file=rel(value["file"])) if isinstance(value, dict) and "file" in value else value
        j["materials"].append(m)
        j["surfaces"].append({"type": "mesh", "filename": rel(obj), "material": name, "transform": {"translate": [0, 0, -3]}})
    j.update(extra or {})
    with open(path, "w") as f:
        json.dump(j, f)
    return path


def _read_dump(path, tmp_path):
    """hip_pt --dump-scene of a scene with normal maps: texture_cpu._read_dump's dump, then the tag NMP0 and the binding"""
    data = open(path, "rb").read()
    at = data.rfind(b"NMP0")
    if at < 0:
        return dict(texture_cpu._read_dump(path), material_normal_map=None)
    n = int(np.frombuffer(data, np.uint64, 1, at + 4)[0])
    assert at + 12 + 4 * n == len(data)
    head = tmp_path / "head.bin"
    head.write_bytes(data[:at])
    return dict(texture_cpu._read_dump(str(head)), material_normal_map=np.frombuffer(data, np.int32, n, at + 12))


def test_the_scene_keys_in_both_readers(pkg, tmp_path):
    """defaults bilinear and repeat; the path relative to the scene file; a picture joins the pool once, also where it is a colour
    texture; "normal_maps": true; and what both readers refuse"""
    obj = tmp_path / "seam.obj"
    obj.write_text(texture_cpu.OBJ)
    checker, ripples = {"file": os.path.join(TEXTURES, "checker.png")}, {"file": os.path.join(TEXTURES, "ripples.png")}
    materials = {"a": ("lambertian", checker, ripples), "b": ("metal", None, dict(ripples, filter="nearest", wrap="clamp")),
                 "c": ("dielectric", None, None), "d": ("lambertian", None, checker), "e": ("metal", ripples, ripples)}
    scene = _scene_json(str(tmp_path / "ok.json"), str(obj), materials, {"normal_maps": True})
    sd = pkg.json_parser.scene_from_json(scene)
    flat = sd.build_scene()
    assert sd.normal_maps is True and sd.textures is False
    # the pool: the colour textures in the materials' order (checker; ripples as e's colour, srgb), then the maps that are new to it
    assert [(os.path.basename(s.file), s.encoding, s.filter, s.wrap) for s in flat.texture_sources] == [
        ("checker.png", "srgb", "bilinear", "repeat"), ("ripples.png", "srgb", "bilinear", "repeat"), ("ripples.png", "linear", "nearest", "clamp")]
    assert flat.material_texture.tolist() == [0, -1, -1, -1, 1] and flat.material_normal_map.tolist() == [1, 2, -1, 0, 1]
    assert flat.texture_sources[1].file == os.path.join(TEXTURES, "ripples.png")
    r = texture_cpu._hip_pt("--method", "megakernel", "--dump-scene", str(tmp_path / "ok.bin"), scene)
    assert r.returncode == 0, r.stderr
    dump = _read_dump(str(tmp_path / "ok.bin"), tmp_path)
    assert [t[2:5] for t in dump["textures"]] == [(1, 1, 0), (1, 1, 0), (0, 0, 1)]
    assert dump["material_texture"].tolist() == [0, -1, -1, -1, 1] and dump["material_normal_map"].tolist() == [1, 2, -1, 0, 1]
    # maps alone: the pool holds them, the colour binding is all -1
    scene = _scene_json(str(tmp_path / "alone.json"), str(obj), {"a": ("lambertian", None, ripples), "b": ("metal", None, None)})
    flat = pkg.json_parser.scene_from_json(scene).build_scene()
    assert flat.material_texture.tolist() == [-1, -1] and flat.material_normal_map.tolist() == [0, -1] and len(flat.texture_sources) == 1
    r = texture_cpu._hip_pt("--method", "megakernel", "--dump-scene", str(tmp_path / "alone.bin"), scene)
    assert r.returncode == 0, r.stderr
    dump = _read_dump(str(tmp_path / "alone.bin"), tmp_path)
    assert dump["material_texture"].tolist() == [-1, -1] and dump["material_normal_map"].tolist() == [0, -1] and len(dump["textures"]) == 1
    # a scene without them: no tail
    r = texture_cpu._hip_pt("--method", "megakernel", "--dump-scene", str(tmp_path / "tex.bin"), "assets/scenes/cornell_textured.json")
    assert r.returncode == 0 and _read_dump(str(tmp_path / "tex.bin"), tmp_path)["material_normal_map"] is None
    # without the method that renders them: the key and a material's map are refused once the scene is read, the flag at once
    for extra, word in (({"normal_maps": True}, '"normal_maps": true'), ({}, 'a material with a "normal_map"')):
        scene = _scene_json(str(tmp_path / "m.json"), str(obj), {"a": ("lambertian", None, ripples if not extra else None)}, extra)
        r = texture_cpu._hip_pt("--dump-scene", str(tmp_path / "m.bin"), scene)
        assert r.returncode != 0 and word in r.stderr and "--method megakernel" in r.stderr, r.stderr
    r = texture_cpu._hip_pt("--normal-maps", "--dump-scene", str(tmp_path / "m.bin"), "assets/scenes/cornell_mesh.json")
    assert r.returncode != 0 and "--normal-maps needs --method megakernel" in r.stderr
    bad = [({"a": ("dielectric", None, ripples)}, {}, "only a lambertian or a metal"), ({"a": ("lambertian", None, dict(ripples, encoding="linear"))}, {}, '"normal_map" must be an object'),
           ({"a": ("lambertian", None, dict(ripples, filter=1))}, {}, '"filter"'), ({"a": ("lambertian", None, dict(ripples, wrap="mirror"))}, {}, '"wrap"'),
           ({"a": ("lambertian", None, "ripples.png")}, {}, '"normal_map" must be an object'),
           ({"a": ("lambertian", None, None)}, {"normal_maps": 1}, '"normal_maps" must be true or false')]
    for materials, extra, word in bad:
        scene = _scene_json(str(tmp_path / "bad.json"), str(obj), materials, extra)
        with pytest.raises(ValueError) as e:
            pkg.json_parser.scene_from_json(scene)
        assert word in str(e.value), (word, str(e.value))
        r = texture_cpu._hip_pt("--method", "megakernel", "--dump-scene", str(tmp_path / "bad.bin"), scene)
        assert r.returncode != 0 and word in r.stderr, (word, r.stderr)


def test_the_asset_scene_and_its_generator(pkg):
    """assets/scenes/cornell_bumpy.json: cornell_textured.json's room with both boxes under tests/golden/textures/ripples.png, whose
    texels are the generator's: 32 x 32, flat at the border, tilted inside"""
    sd = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "cornell_bumpy.json"))
    flat = sd.build_scene()
    assert sd.normal_maps is True and sd.textures is True and len(flat.texture_sources) == 3
    assert sorted(flat.material_normal_map.tolist()) == [-1, -1, -1, -1, -1, 2, 2] and (flat.material_texture >= 0).sum() == 2
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_normal_map_asset as gen
    texels = pkg.png.read_png(os.path.join(TEXTURES, "ripples.png"))
    assert np.array_equal(texels, gen.ripples()) and texels.shape == (32, 32, 4)
    border = np.concatenate([texels[0], texels[-1], texels[:, 0], texels[:, -1]])
    assert (border[:, :3] == (128, 128, 255)).all() and (texels[8:24, 8:24, :2] != 128).any()
    n = pkg.normal_map_decode_table()[texels[..., :3]].astype(np.float64)
    # unit normals up to the byte step; the steepest slope is below 0.035 * 2 pi 3 + the fade's own, < 0.75: z above 0.8
    assert np.abs(np.linalg.norm(n, axis=-1) - 1.0).max() < 0.01 and n[..., 2].min() > 0.8
