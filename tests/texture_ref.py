"""CPU restatement of image textures (ptc_set_textures, ptc_set_texcoords, ptc_set_param "textures", ptc_sample_texture,
ptc_hit_surface) in numpy binary32 -- TEST INFRASTRUCTURE: the checker of tests/test_texture_cpu.py and
tests/test_gpu_texture.py, not the thing under test.

What stands here: the lookup of section 5o (steps 2 .. 7), every numpy operation one binary32 operation of the rule in its order (numpy
does not contract into FMA), the decode being an index into the table ptc_texture_decode_table hands out; the interpolated coordinate and
the albedo of a closest hit, whose winner is smooth_ref.winners' (learnt from the oracle, not from the code under test); and
smooth_ref.render_megakernel's loop stated again with one more option, `textures`, and with smooth shading as a switch inside it."""
import numpy as np

import direct_ref
import env_light_ref
import env_ref
import lens_ref
import lit_ref
import mis_ref
import smooth_ref
from ref_f32 import Draws, F, _dot

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


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------
def render_megakernel(pkg, orc, flat, camera, w, h, iter_begin, iter_count, max_bounces, textures=None, binding=None, texcoords=None,
                      textured=False, normals=None, smooth=False, env=None, entries=None, env_light=False, direct=False, mis=False, roulette=0,
                      lens=None, prev=None, scene_handle=None):
    """smooth_ref.render_megakernel's loop with one more option.  textured with textures and coordinates is the rule of section 5o: at a
    closest hit on a triangle whose material is diffuse or metal and has a texture bound, after the emitter check and roulette and before
    evaluate_material, the material's colour becomes albedo_rows' (counted as a lookup or as a fall-back); nothing else changes.
    Smooth shading is a switch of this statement (smooth with normals), so that both combine.  Without textured, textures or
    coordinates every result is smooth_ref's.  -> smooth_ref's dict and the two counters of COUNTERS."""
    if not textured or textures is None or texcoords is None:
        out = smooth_ref.render_megakernel(orc, flat, camera, w, h, iter_begin, iter_count, max_bounces, normals=normals, smooth=smooth, env=env,
                                           entries=entries, env_light=env_light, direct=direct, mis=mis, roulette=roulette, lens=lens, prev=prev,
                                           scene_handle=scene_handle)
        return {**out, **{k: 0 for k in COUNTERS}}
    sm_on = bool(smooth) and normals is not None
    sh = scene_handle or orc.SceneHandle(flat)
    materials = np.asarray(flat.materials)
    lit = False
    if direct:
        lamps = direct_ref.light_table(flat)
        lit = len(lamps[0]) > 0 and float(lamps[1]["total_weight"]) > 0.0
    lit_env = bool(env_light) and env is not None and entries is not None
    mis = bool(mis) and (lit or lit_env)
    texels = env_ref.apron(env) if lit_env else None
    n_map = texels.shape[0] - 2 if lit_env else 0
    inv_pdf_m = mis_ref.material_pdf(flat, lamps) if (mis and lit) else None
    P = w * h
    frame = lit_ref._frame(prev, P)
    rays = diffuse_hits = shadow_rays = unoccluded = 0
    env_diffuse_hits = env_shadow_rays = env_unoccluded = 0
    mis_emitter_hits = mis_misses = 0
    formed = fallbacks = absorbed = culled = 0
    lookups = tex_fallbacks = 0
    with env_ref._sky_in_place(env), lens_ref._primary_in_place(lens):
        for it in range(iter_count):
            iteration = iter_begin + it
            o, d, tmin, states = lit_ref._primary(orc, camera, w, h, np.arange(P), iteration)
            draws = Draws(orc, states)
            color = np.ones((P, 3), dtype=np.float32)
            radiance = np.zeros((P, 3), dtype=np.float32)
            count_emission = np.ones(P, dtype=bool)
            count_env = np.ones(P, dtype=bool)
            bsdf_pdf = np.zeros(P, dtype=np.float32)
            normal = -d
            depth = np.full(P, F(1e6), dtype=np.float32)
            active = np.arange(P)
            for b in range(max_bounces):
                if len(active) == 0:
                    break
                rays += len(active)
                d_in = d.copy()
                bounce_rays = lit_ref._rays(o[active], tmin[active], d[active])
                recs, em, emission, sc, typ = lit_ref._closest_hits(orc, flat, sh, materials, o, d, tmin, active, b, color, normal, depth)
                hit_at = np.zeros(len(active), dtype=bool)
                at_of = np.full(P, -1, dtype=np.int64)
                at_of[active] = np.arange(len(active))
                hit_at[at_of[em]] = hit_at[at_of[sc]] = True
                w_obj, w_first, w_u, w_v = smooth_ref.winners(orc, flat, sh, bounce_rays, recs[active], hit_at)
                tri = np.zeros(P, dtype=bool)
                tri[active] = w_first >= 0
                shaded = recs.copy()
                trows = active[w_first >= 0]
                if sm_on and len(trows):
                    k = at_of[trows]
                    ns, fell = smooth_ref._shade_rows(flat, normals, w_obj[k], w_first[k], w_u[k], w_v[k], recs["normal"][trows].astype(np.float32),
                                                      d_in[trows])
                    shaded["normal"][trows] = ns
                    formed += int((~fell).sum())
                    fallbacks += int(fell.sum())
                    if b == 0:
                        normal[trows] = ns
                if lit_env:  # a miss behind an environment sample (colour is colour * sky here)
                    hit = np.zeros(P, dtype=bool)
                    hit[em] = hit[sc] = True
                    miss = active[~hit[active]]
                    gated = miss[~count_env[miss]]
                    if mis:
                        mis_misses += len(gated)
                        color[gated] = color[gated] * mis_ref.balance(bsdf_pdf[gated], mis_ref.pdf(entries, n_map, d[gated]))[:, None]
                    else:
                        color[gated] = F(0.0)
                if mis:
                    seen = color[em] * emission
                    gated = ~count_emission[em]
                    mis_emitter_hits += int(gated.sum())
                    t = recs["t"][em].astype(np.float32)
                    cos_l = np.abs(_dot(recs["normal"][em].astype(np.float32), d[em]))  # the geometric normal
                    m_of = recs["material_id"][em].astype(np.int64)
                    p_l = mis_ref.lamp_density(t * t, cos_l, inv_pdf_m[m_of] if inv_pdf_m is not None else np.zeros(len(em), np.float32))
                    color[em] = np.where(gated[:, None], seen * mis_ref.balance(bsdf_pdf[em], p_l)[:, None], seen)
                else:
                    color[em] = np.where(count_emission[em][:, None], color[em] * emission, F(0.0))
                if lit_ref.plays_at(roulette, b, max_bounces):
                    ended, _ = lit_ref.play(orc, color, sc, sc, iteration, b)
                    sc, typ = sc[~ended], typ[~ended]
                # the texture: the paths that reach evaluate_material on a triangle; their material becomes a copy with the albedo
                shade_materials = materials
                trs = sc[tri[sc]]
                if len(trs):
                    k = at_of[trs]
                    mat_id = recs["material_id"][trs].astype(np.int64)
                    _, alb, applied, fell = albedo_rows(pkg, flat, textures, binding, texcoords, w_obj[k], w_first[k], w_u[k], w_v[k], mat_id)
                    lookups += int(applied.sum())
                    tex_fallbacks += int(fell.sum())
                    copies = materials[mat_id].copy()
                    copies["p"][:, :3] = alb
                    shade_materials = np.concatenate([materials, copies])
                    shaded["material_id"][trs] = len(materials) + np.arange(len(trs))
                lit_ref.shade(orc, shade_materials, o, d, tmin, shaded, sc, draws, color)
                df = sc[typ == 0]
                pts = recs["point"][df].astype(np.float32)
                nrm = shaded["normal"][df].astype(np.float32)
                geo = recs["normal"][df].astype(np.float32)
                weigh = mis and b != max_bounces - 1
                if mis:
                    bsdf_pdf[df] = mis_ref.lobe_density(_dot(nrm, d[df]))
                if lit:
                    count_emission[sc] = typ != 0
                    diffuse_hits += len(df)
                    u = direct_ref.light_draws(orc, df, iteration, 3 * b)
                    smp = direct_ref.light_sample(orc, flat, lamps, pts, nrm, u)
                    contribution = smp["contribution"]
                    if weigh and len(df):
                        d2, cos_l, inv_pdf, cos_r = mis_ref.light_terms(orc, flat, lamps, pts, nrm, u)
                        contribution = contribution * mis_ref.balance(mis_ref.lamp_density(d2, cos_l, inv_pdf), mis_ref.lobe_density(cos_r))[:, None]
                    with np.errstate(invalid="ignore"):
                        behind = smp["sampled"] & tri[df] & (_dot(smp["rays"][:, 4:7].astype(np.float32), geo) <= F(0.0)) & sm_on
                    culled += int(behind.sum())
                    got, traced = env_light_ref._arrived(orc, flat, sh, smp["sampled"] & ~behind, smp["rays"])
                    shadow_rays += traced
                    unoccluded += int(got.sum())
                    radiance[df[got]] = radiance[df[got]] + color[df[got]] * contribution[got]
                if lit_env:
                    count_env[sc] = typ != 0
                    env_diffuse_hits += len(df)
                    v, u = env_light_ref.stream(orc, df, iteration, 4 * b)
                    smp = env_light_ref.sample(entries, texels, pts, nrm, v, u)
                    contribution = smp["contribution"]
                    if weigh and len(df):
                        jac, cos_r = mis_ref.env_terms(entries, n_map, nrm, smp["square"], u)
                        contribution = contribution * mis_ref.balance(mis_ref.env_density(jac), mis_ref.lobe_density(cos_r))[:, None]
                    with np.errstate(invalid="ignore"):
                        behind = smp["sampled"] & tri[df] & (_dot(smp["w"].astype(np.float32), geo) <= F(0.0)) & sm_on
                    culled += int(behind.sum())
                    got, traced = env_light_ref._arrived(orc, flat, sh, smp["sampled"] & ~behind, smp["rays"])
                    env_shadow_rays += traced
                    env_unoccluded += int(got.sum())
                    radiance[df[got]] = radiance[df[got]] + color[df[got]] * contribution[got]
                # (smooth) the absorbed continuation: behind the light samples, glass exempt
                with np.errstate(invalid="ignore"):
                    gone = tri[sc] & (typ != 2) & (_dot(d[sc], recs["normal"][sc].astype(np.float32)) <= F(0.0)) & sm_on
                absorbed += int(gone.sum())
                color[sc[gone]] = F(0.0)
                active = sc[~gone]
            total = radiance + color if (lit or lit_env) else color
            lit_ref._deposit(frame, np.arange(P), iteration, total, normal, depth)
    return {**lit_ref._planes(frame, h, w), "rays": rays, "diffuse_hits": diffuse_hits, "shadow_rays": shadow_rays, "unoccluded": unoccluded,
            "env_diffuse_hits": env_diffuse_hits, "env_shadow_rays": env_shadow_rays, "env_unoccluded": env_unoccluded,
            "mis_emitter_hits": mis_emitter_hits, "mis_misses": mis_misses, "shading_normals": formed, "fallbacks": fallbacks,
            "absorbed": absorbed, "culled_light_samples": culled, "lookups": lookups, "tex_fallbacks": tex_fallbacks}


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
