"""CPU restatement of normal maps (ptc_set_normal_maps, ptc_set_param "normal_maps", ptc_hit_shading_normal, ptc_check_normal_map;
DESIGN section 5q) in numpy binary32 -- TEST INFRASTRUCTURE: the checker of tests/test_normal_map_cpu.py and
tests/test_gpu_normal_map.py, not the thing under test.

What stands here: the decode table and the rule of section 5q, every numpy operation one binary32 operation of the rule in its order
(numpy does not contract into FMA), the texel being texture_ref.lookup's with the normal table in place of the encoding's; and the
normal of a closest hit, whose winner is smooth_ref.winners'.  The loop that applies them is loop_ref.render_megakernel's under
`normal_maps`."""
import types

import numpy as np

import smooth_ref
import texture_ref
from ref_f32 import F, _cross, _dot, _normalize

FLT_MAX = smooth_ref.FLT_MAX
COUNTERS = ("bent", "kept")
MISS, NONE, BENT, FLAT, KEPT = 0, 1, 2, 3, 4
NORMAL = 2  # the key of the normal table beside texture_ref's LINEAR and SRGB


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def decode_table():
    """out[k] = max((k - 128) / 127, -1), one binary32 subtraction and one division"""
    k = np.arange(256).astype(np.float32)
    return np.maximum((k - F(128.0)) / F(127.0), F(-1.0)).astype(np.float32)


class _NormalTable:
    """what texture_ref.lookup asks its `pkg` for: the normal table, whatever the encoding"""

    @staticmethod
    def texture_decode_table(encoding):
        return decode_table()


def texel(tex, st):
    """step 2: steps 2 .. 7 of section 5o with the normal table; the texture's filter and wrap hold -> (c [n, 3], refused bool [n])"""
    as_normal = types.SimpleNamespace(rgba8=tex.rgba8, encoding=NORMAL, filter=tex.filter, wrap=tex.wrap)
    return texture_ref.lookup(_NormalTable, as_normal, st)


def _xform_vector(m16, p):
    """transform_vector: (M * (v, 0)).xyz with mat4 * vec4 = (c0 x + c1 y) + (c2 z + c3 w); m16 column-major, [16] or [k, 16]"""
    m = np.asarray(m16, dtype=np.float32).reshape(-1, 16)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([(m[:, r] * x + m[:, 4 + r] * y) + (m[:, 8 + r] * z + m[:, 12 + r] * F(0.0)) for r in range(3)], axis=-1).astype(np.float32)


def _has_length(l2):
    return (l2 > F(0.0)) & (l2 <= FLT_MAX)


def bend(c, refused, p0, p1, p2, st0, st1, st2, m16, b, g, d):
    """Steps 3 .. 8 per row on the texels c (refused: step 2 refused the coordinate) -> (n [k, 3], outcome uint8 [k])"""
    c, p0, p1, p2, b, g, d = (np.asarray(a, dtype=np.float32).reshape(-1, 3) for a in (c, p0, p1, p2, b, g, d))
    st0, st1, st2 = (np.asarray(a, dtype=np.float32).reshape(-1, 2) for a in (st0, st1, st2))
    with np.errstate(all="ignore"):
        x, y, z = c[:, 0], c[:, 1], c[:, 2]
        flat = (x == F(0.0)) & (y == F(0.0)) & (z > F(0.0)) & ~refused
        e1 = p1 - p0
        e2 = p2 - p0
        ds1 = st1[:, 0] - st0[:, 0]
        ds2 = st2[:, 0] - st0[:, 0]
        dt1 = st1[:, 1] - st0[:, 1]
        dt2 = st2[:, 1] - st0[:, 1]
        det = ds1 * dt2 - ds2 * dt1
        ok = ~refused & ((det > F(0.0)) | (det < F(0.0)))
        t_o = e1 * dt2[:, None] - e2 * dt1[:, None]
        b_o = e2 * ds1[:, None] - e1 * ds2[:, None]
        neg = (det < F(0.0))[:, None]
        t_o = np.where(neg, -t_o, t_o).astype(np.float32)
        b_o = np.where(neg, -b_o, b_o).astype(np.float32)
        t_w = _xform_vector(m16, t_o)
        b_w = _xform_vector(m16, b_o)
        k = _dot(t_w, b)
        tp = (t_w - b * k[:, None]).astype(np.float32)
        ok &= _has_length(_dot(tp, tp))
        t = _normalize(tp).astype(np.float32)
        cr = _cross(b, t).astype(np.float32)
        bt = np.where((_dot(cr, b_w) < F(0.0))[:, None], -cr, cr).astype(np.float32)
        a = ((t * x[:, None] + bt * y[:, None]) + b * z[:, None]).astype(np.float32)
        ok &= _has_length(_dot(a, a))
        s = _normalize(a).astype(np.float32)
        ok &= _dot(s, g) > F(0.0)
        ok &= _dot(d, s) < F(0.0)
    bent = ok & ~flat
    outcome = np.where(flat, FLAT, np.where(bent, BENT, KEPT)).astype(np.uint8)
    return np.where(bent[:, None], s, b).astype(np.float32), outcome


def shade(tex, p0, p1, p2, st0, st1, st2, u, v, m16, b, g, d):
    """Steps 1 .. 8 per row on one pkg.Texture -> (n [k, 3], outcome uint8 [k])"""
    st0, st1, st2 = (np.asarray(a, dtype=np.float32).reshape(-1, 2) for a in (st0, st1, st2))
    st = texture_ref.interpolate(st0, st1, st2, np.asarray(u, np.float32).reshape(-1), np.asarray(v, np.float32).reshape(-1))
    c, refused = texel(tex, st)
    return bend(c, refused, p0, p1, p2, st0, st1, st2, m16, b, g, d)


# ---- the normal of a closest hit --------------------------------------------------------------------------------------------------------
def _corner_positions(flat, obj, first):
    """the three corners' object-space positions of the winners -> [k, 3, 3]"""
    pos = np.ascontiguousarray(flat.positions, dtype=np.float32).reshape(-1, 3)
    idx = np.asarray(flat.indices, dtype=np.int64)
    meshes = smooth_ref.mesh_rows(flat)
    out = np.empty((len(obj), 3, 3), dtype=np.float32)
    for k, (o, f) in enumerate(zip(obj, first)):
        fv, _, fi, _ = meshes[smooth_ref._mesh_of(flat, flat.objects[int(o)])]
        out[k] = pos[fv + idx[fi + int(f):fi + int(f) + 3]]
    return out


def normal_rows(flat, textures, nbinding, texcoords, obj, first, u, v, mat_id, base, g, d):
    """The rule at triangle hits: winners (obj, first, u, v) on materials mat_id with base normals `base` -> (n [k, 3]; outcome uint8 [k],
    NONE where no map applies)"""
    materials = np.asarray(flat.materials)
    n = np.ascontiguousarray(base, dtype=np.float32).copy()
    outcome = np.full(len(obj), NONE, dtype=np.uint8)
    if textures is None or texcoords is None or nbinding is None or len(obj) == 0:
        return n, outcome
    bound = np.asarray(nbinding, dtype=np.int64)[mat_id]
    wanted = (bound >= 0) & (materials["type"][mat_id] <= 1)
    if not wanted.any():
        return n, outcome
    c = texture_ref._corner_st(flat, texcoords, obj, first)
    p = _corner_positions(flat, obj, first)
    m = np.asarray(flat.objects["m"], dtype=np.float32).reshape(len(flat.objects), 16)[obj]
    for ti in np.unique(bound[wanted]):
        r = np.nonzero(wanted & (bound == ti))[0]
        n[r], outcome[r] = shade(textures[int(ti)], p[r, 0], p[r, 1], p[r, 2], c[r, 0], c[r, 1], c[r, 2], np.asarray(u, np.float32)[r],
                                 np.asarray(v, np.float32)[r], m[r], n[r], np.asarray(g, np.float32)[r], np.asarray(d, np.float32)[r])
    return n, outcome


def hit_shading_normal(orc, flat, rays, normals=None, textures=None, nbinding=None, texcoords=None, scene_handle=None):
    """ptc_hit_shading_normal restated -> dict(normal [n, 3], outcome uint8 [n])"""
    sh = scene_handle or orc.SceneHandle(flat)
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
    recs, hit = orc.intersect_rays(flat, rays, scene_handle=sh)
    hit = hit.astype(bool)
    obj, first, u, v = smooth_ref.winners(orc, flat, sh, rays, recs, hit)
    normal = np.where(hit[:, None], recs["normal"].astype(np.float32), F(0.0)).astype(np.float32)
    outcome = np.where(hit, NONE, MISS).astype(np.uint8)
    tri = np.nonzero(first >= 0)[0]
    if len(tri):
        g = recs["normal"][tri].astype(np.float32)
        if normals is not None:
            normal[tri] = smooth_ref._shade_rows(flat, normals, obj[tri], first[tri], u[tri], v[tri], g, rays[tri, 4:7])[0]
        normal[tri], outcome[tri] = normal_rows(flat, textures, nbinding, texcoords, obj[tri], first[tri], u[tri], v[tri],
                                                recs["material_id"][tri].astype(np.int64), normal[tri], g, rays[tri, 4:7])
    return {"normal": normal, "outcome": outcome}


# ---- the maps the CPU and GPU tests share -----------------------------------------------------------------------------------------------
def flat_map(pkg, width=3, height=2, **kw):
    """every texel (128, 128, 255): the rule's flat outcome under either filter"""
    t = np.zeros((height, width, 4), dtype=np.uint8)
    t[...] = (128, 128, 255, 255)
    return pkg.Texture(t, **kw)


def bumpy_map(pkg, width=7, height=5, seed=21, tilt=96, **kw):
    """random tangent-space normals that lean up to `tilt` byte steps off the axis, z kept well above 0; one texel exactly flat"""
    rng = np.random.default_rng(seed)
    t = np.zeros((height, width, 4), dtype=np.uint8)
    t[..., 0:2] = rng.integers(128 - tilt, 129 + tilt, (height, width, 2))
    t[..., 2] = rng.integers(200, 256, (height, width))
    t[..., 3] = 255
    t[0, 0] = (128, 128, 255, 255)
    return pkg.Texture(t, **kw)
