"""CPU restatement of image textures (ptc_set_textures, ptc_set_texcoords, ptc_set_param "textures", ptc_sample_texture,
ptc_hit_surface) in numpy binary32 -- TEST INFRASTRUCTURE: the checker of tests/test_texture_cpu.py and
tests/test_gpu_texture.py, not the thing under test.

What stands here: the lookup of section 5o (steps 2 .. 7), every numpy operation one binary32 operation of the rule in its order (numpy
does not contract into FMA), the decode being an index into the table ptc_texture_decode_table hands out; the interpolated coordinate and
the albedo of a closest hit, whose winner is smooth_ref.winners' (learnt from the oracle, not from the code under test).  The loop that
applies them is loop_ref.render_megakernel's under `textured`."""
import numpy as np

import smooth_ref
from ref_f32 import F

FLT_MAX = smooth_ref.FLT_MAX
COUNTERS = ("lookups", "tex_fallbacks")
LINEAR, SRGB = 0, 1
NEAREST, BILINEAR = 0, 1
REPEAT, CLAMP = 0, 1
_tables = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def table(pkg, encoding):
    """the library's decode table of the encoding (read once)"""
    if encoding not in _tables:
        _tables[encoding] = pkg.texture_decode_table(encoding)
    return _tables[encoding]


def table_f64(encoding):
    """the formula the header names, in float64: k / 255, or the piecewise sRGB curve of it"""
    c = np.arange(256, dtype=np.float64) / 255.0
    return c if encoding == LINEAR else np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


# ---- the rule (pt_texture.hpp: lookup) ----------------------------------------------------------------------------------------------------
def _coordinate(x, n, wrap):
    """step 3"""
    if wrap == REPEAT:
        f = x - np.floor(x)
        f = np.where(f >= F(1.0), F(0.0), f)
    else:
        f = np.where(x < F(0.0), F(0.0), np.where(x > F(1.0), F(1.0), x))
    return (f.astype(np.float32) * F(n)).astype(np.float32)


def _nearest(g, n):
    """step 4"""
    return np.minimum(np.floor(g).astype(np.int64), n - 1)


def _bilinear(g, n, wrap):
    """step 5 -> (i0, i1, the weight of i1)"""
    h = g - F(0.5)
    fl = np.floor(h)
    a = (h - fl).astype(np.float32)
    i0 = fl.astype(np.int64)
    i1 = i0 + 1
    if wrap == REPEAT:
        back = lambda i: np.where(i < 0, i + n, np.where(i > n - 1, i - n, i))
    else:
        back = lambda i: np.clip(i, 0, n - 1)
    return back(i0), back(i1), a


def _mix(x, y, a):
    return x * (F(1.0) - a) + y * a


def lookup(pkg, tex, st):
    """Steps 2 .. 7 for the pairs st [n, 2] on one pkg.Texture -> (rgb float32 [n, 3], zeros where refused; rejected bool [n])"""
    st = np.ascontiguousarray(st, dtype=np.float32).reshape(-1, 2)
    tab = table(pkg, int(tex.encoding))
    texels = np.asarray(tex.rgba8)
    hgt, wid = texels.shape[:2]
    with np.errstate(all="ignore"):
        ok = (np.abs(st[:, 0]) <= FLT_MAX) & (np.abs(st[:, 1]) <= FLT_MAX)
        s = np.where(ok, st[:, 0], F(0.0)).astype(np.float32)
        t = np.where(ok, st[:, 1], F(0.0)).astype(np.float32)
        gs, gt = _coordinate(s, wid, int(tex.wrap)), _coordinate(t, hgt, int(tex.wrap))
        if int(tex.filter) == NEAREST:
            rgb = tab[texels[_nearest(gt, hgt), _nearest(gs, wid), :3]]
        else:
            i0, i1, a_s = _bilinear(gs, wid, int(tex.wrap))
            j0, j1, a_t = _bilinear(gt, hgt, int(tex.wrap))
            c00, c10, c01, c11 = (tab[texels[j, i, :3]] for j, i in ((j0, i0), (j0, i1), (j1, i0), (j1, i1)))
            rgb = _mix(_mix(c00, c10, a_s[:, None]), _mix(c01, c11, a_s[:, None]), a_t[:, None])
    return np.where(ok[:, None], rgb, F(0.0)).astype(np.float32), ~ok


def lookup_f64(tex, st):
    """An independent bilinear of the same texels in float64 (finite pairs only): nothing of `lookup` is reused but the texels"""
    st = np.asarray(st, dtype=np.float64).reshape(-1, 2)
    texels = table_f64(int(tex.encoding))[np.asarray(tex.rgba8)[:, :, :3]]
    hgt, wid = texels.shape[:2]
    out = []
    for x, y in st:
        axes = []
        for c, n in ((x, wid), (y, hgt)):
            f = c - np.floor(c) if int(tex.wrap) == REPEAT else min(max(c, 0.0), 1.0)
            h = f * n - 0.5
            i0 = int(np.floor(h))
            a = h - i0
            fold = (lambda i: i % n) if int(tex.wrap) == REPEAT else (lambda i: min(max(i, 0), n - 1))
            axes.append((fold(i0), fold(i0 + 1), a))
        (i0, i1, a), (j0, j1, b) = axes
        out.append((texels[j0, i0] * (1 - a) + texels[j0, i1] * a) * (1 - b) + (texels[j1, i0] * (1 - a) + texels[j1, i1] * a) * b)
    return np.asarray(out)


# ---- the coordinate and the albedo of a closest hit -----------------------------------------------------------------------------------------
def interpolate(a0, a1, a2, u, v):
    """step 1, per component: (a0 w + a1 u) + a2 v, w = (1 - u) - v"""
    with np.errstate(all="ignore"):
        t = F(1.0) - u
        w = t - v
        return ((a0 * w[:, None] + a1 * u[:, None]) + a2 * v[:, None]).astype(np.float32)


def _corner_st(flat, texcoords, obj, first):
    """the three corners' pairs of the winners (object, offset in the mesh's indices) -> [k, 3, 2]"""
    st = np.ascontiguousarray(texcoords, dtype=np.float32).reshape(-1, 2)
    meshes = smooth_ref.mesh_rows(flat)
    out = np.empty((len(obj), 3, 2), dtype=np.float32)
    for k, (o, f) in enumerate(zip(obj, first)):
        fi = meshes[smooth_ref._mesh_of(flat, flat.objects[int(o)])][2]
        out[k] = st[fi + int(f):fi + int(f) + 3]
    return out


def albedo_rows(pkg, flat, textures, binding, texcoords, obj, first, u, v, mat_id):
    """Steps 1 .. 8 at triangle hits: winners (obj, first, u, v) on materials mat_id -> (st [k, 2]; albedo [k, 3]; applied bool [k]: a
    texture was looked up; fell bool [k]: the rule applied and the coordinate was refused)"""
    materials = np.asarray(flat.materials)
    p = materials["p"][mat_id, :3].astype(np.float32)
    c = _corner_st(flat, texcoords, obj, first)
    st = interpolate(c[:, 0], c[:, 1], c[:, 2], np.asarray(u, np.float32), np.asarray(v, np.float32))
    alb = p.copy()
    applied, fell = np.zeros(len(obj), dtype=bool), np.zeros(len(obj), dtype=bool)
    if textures is None:
        return st, alb, applied, fell
    bound = np.asarray(binding, dtype=np.int64)[mat_id]
    wanted = (bound >= 0) & (materials["type"][mat_id] <= 1)
    for ti in np.unique(bound[wanted]):
        rows = np.nonzero(wanted & (bound == ti))[0]
        rgb, rej = lookup(pkg, textures[int(ti)], st[rows])
        alb[rows] = np.where(rej[:, None], p[rows], rgb * p[rows])
        applied[rows], fell[rows] = ~rej, rej
    return st, alb.astype(np.float32), applied, fell


def hit_surface(pkg, orc, flat, rays, textures=None, binding=None, texcoords=None, scene_handle=None):
    """ptc_hit_surface restated -> dict(st [n, 2], albedo [n, 3])"""
    sh = scene_handle or orc.SceneHandle(flat)
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
    recs, hit = orc.intersect_rays(flat, rays, scene_handle=sh)
    hit = hit.astype(bool)
    obj, first, u, v = smooth_ref.winners(orc, flat, sh, rays, recs, hit)
    mat = recs["material_id"].astype(np.int64)
    st = np.zeros((len(rays), 2), dtype=np.float32)
    alb = np.where(hit[:, None], np.asarray(flat.materials)["p"][np.where(hit, mat, 0), :3].astype(np.float32), F(0.0)).astype(np.float32)
    tri = np.nonzero(first >= 0)[0]
    if texcoords is not None and len(tri):
        st[tri], alb[tri] = albedo_rows(pkg, flat, textures, binding, texcoords, obj[tri], first[tri], u[tri], v[tri], mat[tri])[:2]
    return {"st": st, "albedo": alb}


# ---- the textures, coordinates and scenes the CPU and GPU tests share -------------------------------------------------------------------
def random_texture(pkg, width, height, seed, **kw):
    texels = np.random.default_rng(seed).integers(0, 256, (height, width, 4), dtype=np.uint8)
    return pkg.Texture(texels, **kw)


def pool(pkg):
    """three textures of different sizes and settings: an offset bug shows on the second and third"""
    return [random_texture(pkg, 5, 3, 11, encoding="srgb", filter="bilinear", wrap="repeat"),
            random_texture(pkg, 2, 2, 12, encoding="linear", filter="nearest", wrap="clamp"),
            random_texture(pkg, 7, 4, 13, encoding="srgb", filter="bilinear", wrap="clamp")]


def material_index(scene, name):
    """where build_scene puts the material (the table is sorted by name)"""
    return sorted(scene.material_map_, key=lambda s: s.encode()).index(name)


def bind(scene, flat, by_name):
    """{material name: texture} -> material_texture"""
    out = np.full(len(flat.materials), -1, dtype=np.int32)
    for name, ti in by_name.items():
        out[material_index(scene, name)] = ti
    return out


def random_texcoords(flat, seed=3, lo=-1.5, hi=2.5):
    """a pair per corner, every corner its own: each edge of the mesh is a seam, and the range wraps and clamps"""
    return np.random.default_rng(seed).uniform(lo, hi, (len(flat.indices), 2)).astype(np.float32)


def coordinate_set(width, height):
    """the pairs both lookups are compared on: texel centres and edges of the texture, the special values, 4096 random pairs"""
    xs = [0.0, -0.0, 1.0, 1.0 - 2.0 ** -24, -1e-30, 1e7, -1e7, 2.0 ** 24 + 1, -(2.0 ** 24) - 1, float(FLT_MAX), -float(FLT_MAX), np.inf, -np.inf,
          np.nan, 0.5, 0.25, -0.75, 1.5]
    for n in (width, height):
        k = np.unique(np.clip(np.array([0, 1, 2, n // 2, n - 2, n - 1, n]), 0, n))
        xs += list(k / n) + list((k + 0.5) / n) + list(-(k + 0.5) / n) + list(1.0 + k / n)
    xs = np.asarray(xs, dtype=np.float32)
    grid = np.stack(np.meshgrid(xs, xs, indexing="ij"), axis=-1).reshape(-1, 2)
    rnd = np.random.default_rng(width * 8191 + height).uniform(-3.0, 3.0, (4096, 2)).astype(np.float32)
    return np.concatenate([grid, rnd]).astype(np.float32)
