"""CPU restatement of normal maps (ptc_set_normal_maps, ptc_set_param "normal_maps", ptc_hit_shading_normal, ptc_check_normal_map;
DESIGN section 5q) in numpy binary32 -- TEST INFRASTRUCTURE: the checker of tests/test_normal_map_cpu.py and
tests/test_gpu_normal_map.py, not the thing under test.

What stands here: the decode table and the rule of section 5q, every numpy operation one binary32 operation of the rule in its order
(numpy does not contract into FMA), the texel being texture_ref.lookup's with the normal table in place of the encoding's; the normal
of a closest hit, whose winner is smooth_ref.winners'; and texture_ref.render_megakernel's loop stated again with one more option,
`normal_maps`, and with smooth shading and the colour texture as switches inside it."""
import types

import numpy as np

import direct_ref
import env_light_ref
import env_ref
import lens_ref
import lit_ref
import mis_ref
import smooth_ref
import texture_ref
from ref_f32 import Draws, F, _cross, _dot, _normalize

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


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------
def render_megakernel(pkg, orc, flat, camera, w, h, iter_begin, iter_count, max_bounces, textures=None, binding=None, texcoords=None,
                      textured=False, nbinding=None, normal_maps=False, normals=None, smooth=False, env=None, entries=None, env_light=False,
                      direct=False, mis=False, roulette=0, lens=None, prev=None, scene_handle=None):
    """texture_ref.render_megakernel's loop with one more option.  normal_maps with textures, coordinates and a binding that names a map
    is the rule of section 5q: where the albedo fetch runs -- a closest hit on a triangle, after the emitter check and roulette, before
    evaluate_material -- a bound diffuse or metal material's shading normal becomes normal_rows' from there on (evaluate_material, the
    light samples, the lobe's density); the normal plane keeps the normal it had.  Where the map bent the normal, smooth shading's culls
    and its absorption apply as at a triangle under smooth shading.  The colour texture (textured) and smooth shading (smooth with
    normals) are switches of this statement.  Without the option every result is texture_ref's.
    -> texture_ref's dict and the two counters of COUNTERS."""
    nm_on = bool(normal_maps) and textures is not None and texcoords is not None and nbinding is not None and bool((np.asarray(nbinding) >= 0).any())
    if not nm_on:
        out = texture_ref.render_megakernel(pkg, orc, flat, camera, w, h, iter_begin, iter_count, max_bounces, textures=textures, binding=binding,
                                            texcoords=texcoords, textured=textured, normals=normals, smooth=smooth, env=env, entries=entries,
                                            env_light=env_light, direct=direct, mis=mis, roulette=roulette, lens=lens, prev=prev,
                                            scene_handle=scene_handle)
        return {**out, **{k: 0 for k in COUNTERS}}
    tex_on = bool(textured)
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
    n_bent = n_kept = 0
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
                # the paths that reach evaluate_material on a triangle: the map's normal, then the texture's albedo
                shade_materials = materials
                below = tri & sm_on  # where the culls and the absorption apply
                trs = sc[tri[sc]]
                if len(trs):
                    k = at_of[trs]
                    mat_id = recs["material_id"][trs].astype(np.int64)
                    nn, how = normal_rows(flat, textures, nbinding, texcoords, w_obj[k], w_first[k], w_u[k], w_v[k], mat_id,
                                          shaded["normal"][trs].astype(np.float32), recs["normal"][trs].astype(np.float32), d_in[trs])
                    shaded["normal"][trs] = nn
                    n_bent += int((how == BENT).sum())
                    n_kept += int((how == KEPT).sum())
                    if not sm_on:
                        below[trs[how == BENT]] = True
                    if tex_on:
                        _, alb, applied, fell = texture_ref.albedo_rows(pkg, flat, textures, binding, texcoords, w_obj[k], w_first[k], w_u[k], w_v[k],
                                                                        mat_id)
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
                        behind = smp["sampled"] & below[df] & (_dot(smp["rays"][:, 4:7].astype(np.float32), geo) <= F(0.0))
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
                        behind = smp["sampled"] & below[df] & (_dot(smp["w"].astype(np.float32), geo) <= F(0.0))
                    culled += int(behind.sum())
                    got, traced = env_light_ref._arrived(orc, flat, sh, smp["sampled"] & ~behind, smp["rays"])
                    env_shadow_rays += traced
                    env_unoccluded += int(got.sum())
                    radiance[df[got]] = radiance[df[got]] + color[df[got]] * contribution[got]
                # the absorbed continuation: behind the light samples, glass exempt
                with np.errstate(invalid="ignore"):
                    gone = below[sc] & (typ != 2) & (_dot(d[sc], recs["normal"][sc].astype(np.float32)) <= F(0.0))
                absorbed += int(gone.sum())
                color[sc[gone]] = F(0.0)
                active = sc[~gone]
            total = radiance + color if (lit or lit_env) else color
            lit_ref._deposit(frame, np.arange(P), iteration, total, normal, depth)
    return {**lit_ref._planes(frame, h, w), "rays": rays, "diffuse_hits": diffuse_hits, "shadow_rays": shadow_rays, "unoccluded": unoccluded,
            "env_diffuse_hits": env_diffuse_hits, "env_shadow_rays": env_shadow_rays, "env_unoccluded": env_unoccluded,
            "mis_emitter_hits": mis_emitter_hits, "mis_misses": mis_misses, "shading_normals": formed, "fallbacks": fallbacks,
            "absorbed": absorbed, "culled_light_samples": culled, "lookups": lookups, "tex_fallbacks": tex_fallbacks, "bent": n_bent,
            "kept": n_kept}


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
