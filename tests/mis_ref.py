"""CPU restatement of multiple importance sampling in the megakernel (ptc_set_param "mis", ptc_environment_light_pdf,
ptc_light_material_pdf) in numpy binary32 -- TEST INFRASTRUCTURE: the checker of tests/test_mis_cpu.py and
tests/test_gpu_mis.py, not the thing under test.

What stands here: the balance heuristic's weight and the three densities of section 5l, every numpy operation one binary32 operation of
the rule in its order; the square a direction falls in and the environment sample's density there; the per-material array of the lamp
table; and env_light_ref.render_megakernel's loop stated again with one more option, `mis`, from the pinned pieces of lit_ref /
direct_ref / env_ref / env_light_ref / lens_ref.  The terms of a lamp's sample (d^2 and the two cosines) are not among what
direct_ref.light_sample returns: light_terms forms them again from the same draws, with direct_ref's own lines."""
import numpy as np

import direct_ref
import env_light_ref
import env_ref
import lens_ref
import lit_ref
from ref_f32 import PI, PI2, Draws, F, _dot, _normalize, _sincos, _xform_point

FLT_MAX = F(np.finfo(np.float32).max)


# ---- the weight and the densities (pt_mis.hpp) -----------------------------------------------------------------------------------------
def balance(a, b):
    """a / (a + b); 1 where the sum is not > 0 or a is past FLT_MAX"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    with np.errstate(all="ignore"):
        s = a + b
        w = a / s
        return np.where((s > F(0.0)) & (a <= FLT_MAX), w, F(1.0)).astype(np.float32)


def lamp_density(d2, cos_l, inv_pdf):
    """d2 / (cos_l inv_pdf); 0 where the product is not > 0"""
    with np.errstate(all="ignore"):
        den = np.asarray(cos_l, dtype=np.float32) * np.asarray(inv_pdf, dtype=np.float32)
        p = np.asarray(d2, dtype=np.float32) / den
        return np.where(den > F(0.0), p, F(0.0)).astype(np.float32)


def lobe_density(c):
    """c / pi; 0 where c <= 0"""
    c = np.asarray(c, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        p = c / PI
        return np.where(c > F(0.0), p, F(0.0)).astype(np.float32)


def env_density(jac):
    """1 / jac; 0 where jac is not > 0"""
    jac = np.asarray(jac, dtype=np.float32)
    with np.errstate(all="ignore"):
        return np.where(jac > F(0.0), F(1.0) / jac, F(0.0)).astype(np.float32)


# ---- the environment sample's density (pt_env_light.hpp: square_of, density) ------------------------------------------------------------
def project(d):
    """env_rules::project: directions [k, 3] -> (ok [k], qx, qz), the point of the octahedral square; rows that are not ok hold 0"""
    d = np.asarray(d, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        a = (np.abs(d[:, 0]) + np.abs(d[:, 1])) + np.abs(d[:, 2])
        ok = (a > F(0.0)) & (a <= FLT_MAX)
        a_ok = np.where(ok, a, F(1.0))
        dx, dy, dz = (np.where(ok, d[:, k], F(0.0)) for k in range(3))
        px = dx / a_ok
        pz = dz / a_ok
        lower = dy < F(0.0)
        qx = np.where(lower, (F(1.0) - np.abs(pz)) * env_ref._sgn(px), px)
        qz = np.where(lower, (F(1.0) - np.abs(px)) * env_ref._sgn(pz), pz)
    return ok, qx.astype(np.float32), qz.astype(np.float32)


def _cell(q, n):
    m = q * F(0.5)
    s = m + F(0.5)
    f = np.floor(s * F(n))
    return np.where(f >= F(n), n - 1, np.where(f > F(0.0), f, F(0.0)).astype(np.int64)).astype(np.int64)


def square_of(qx, qz, n):
    """the square k = j n + i of the point (qx, qz)"""
    return _cell(qz, n) * n + _cell(qx, n)


def pdf(entries, n, d):
    """env_light::density in the unit directions d [k, 3] -> binary32 [k]; entries: env_light_ref.table_of's, None for a map of weight 0"""
    d = np.asarray(d, dtype=np.float32).reshape(-1, 3)
    if entries is None:
        return np.zeros(len(d), dtype=np.float32)
    ok, qx, qz = project(d)
    f = entries["f"][square_of(qx, qz, n)]
    with np.errstate(all="ignore"):
        l1 = (np.abs(d[:, 0]) + np.abs(d[:, 1])) + np.abs(d[:, 2])
        l3 = (l1 * l1) * l1
        ff = F(4.0) * f
        jac = ff * l3
        return np.where(ok, env_density(jac), F(0.0)).astype(np.float32)


def env_terms(entries, n, normals, square, u):
    """(jac, cos_r) of env_light_ref.sample's sample in `square` from the draws u [k, 3]: the sample's own (4 f) l^3 and its cosine"""
    f = entries["f"][square]
    j = square // n
    i = square - j * n
    sx = (i.astype(np.float32) + u[:, 1]) / F(n)
    sz = (j.astype(np.float32) + u[:, 2]) / F(n)
    w, l3 = env_light_ref.decode(sx, sz)
    ff = F(4.0) * f
    return ff * l3, _dot(np.asarray(normals, dtype=np.float32).reshape(-1, 3), w)


# ---- the lamps' side ---------------------------------------------------------------------------------------------------------------------
def material_pdf(flat, table=None):
    """ptc_light_material_pdf: per material (float)(W / lum), 0 for no lamp, for lum == 0 and for a table of weight 0"""
    table = table if table is not None else direct_ref.light_table(flat)
    materials = np.asarray(flat.materials)
    out = np.zeros(len(materials), dtype=np.float32)
    total = float(table[1]["total_weight"])
    if len(table[0]) == 0 or not total > 0.0:
        return out
    for m, mat in enumerate(materials):
        if mat["type"] != direct_ref.EMISSIVE:
            continue
        lum = float(max(mat["p"][0], mat["p"][1], mat["p"][2]))
        out[m] = F(0.0) if lum == 0.0 else F(total / lum)
    return out


def light_terms(orc, flat, table, p, nrm, draws):
    """(d2, cos_l, inv_pdf, cos_r) of direct_ref.light_sample's sample for the same points and draws, by direct_ref's own lines"""
    recs, _, weights, last = table
    n = len(p)
    if n == 0:
        return (np.zeros(0, dtype=np.float32),) * 4
    raw, u = draws
    u1, u2 = u[:, 0], u[:, 1]
    r = recs[direct_ref.select(weights, last, raw)]
    p0 = r["p0"]
    q = np.zeros((n, 3), dtype=np.float32)
    nl = np.zeros((n, 3), dtype=np.float32)
    sph = np.nonzero(r["kind_material"] >> 31)[0]
    tri = np.nonzero((r["kind_material"] >> 31) == 0)[0]
    if len(tri):
        su = np.sqrt(u1[tri])
        b1 = F(1.0) - su
        b2 = u2[tri] * su
        q[tri] = (p0[tri] + r["e1"][tri] * b1[:, None]) + r["e2"][tri] * b2[:, None]
        nl[tri] = r["n"][tri]
    if len(sph):
        z = F(1.0) - F(2.0) * u1[sph]
        x = F(1.0) - z * z
        rr = np.sqrt(np.where(F(0.0) < x, x, F(0.0)))
        s, c = _sincos(orc, PI2 * u2[sph])
        d = np.stack([rr * c, rr * s, z], axis=-1)
        spheres = np.asarray(flat.spheres, dtype=np.float32).reshape(-1, 4)
        for j, lane in enumerate(sph):
            obj = flat.objects[int(r["object"][lane])]
            sp = spheres[int(obj["index"])]
            q[lane] = _xform_point(obj["m"], sp[:3] + d[j] * sp[3])
        nl[sph] = _normalize(q[sph] - p0[sph])
    v = q - p
    d2 = _dot(v, v)
    with np.errstate(all="ignore"):
        w = v * (F(1.0) / np.sqrt(d2))[:, None]
        return d2, np.abs(_dot(nl, w)), r["inv_pdf"].astype(np.float32), _dot(nrm, w)


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------
def render_megakernel(orc, flat, camera, w, h, iter_begin, iter_count, max_bounces, env=None, entries=None, env_light=False, direct=False,
                      mis=False, roulette=0, lens=None, prev=None, scene_handle=None):
    """env_light_ref.render_megakernel's loop with one more option.  mis in a frame that samples the lamps, the environment or both is
    the rule of section 5l: per path one more number, bsdf_pdf = lobe_density(dot(normal, new direction)) after evaluate_material at a
    diffuse hit; the lamp's sample is weighted balance(lamp_density(d2, cos_l, inv_pdf), lobe_density(cos_r)) and the environment's
    balance(env_density(jac), lobe_density(cos_r)) before colour * contribution, except at the last bounce; an emitter hit while
    count_emission is false counts (colour * emission) * balance(bsdf_pdf, lamp_density(t^2, |dot(n, d)|, inv_pdf_m[material])) and a
    miss while count_env is false (colour * sky) * balance(bsdf_pdf, pdf(d)), each instead of 0.  Without mis, or with neither light in
    effect, every result is env_light_ref.render_megakernel's.
    -> env_light_ref's dict and mis_emitter_hits, mis_misses."""
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
    inv_pdf_m = material_pdf(flat, lamps) if (mis and lit) else None
    P = w * h
    frame = lit_ref._frame(prev, P)
    rays = diffuse_hits = shadow_rays = unoccluded = 0
    env_diffuse_hits = env_shadow_rays = env_unoccluded = 0
    mis_emitter_hits = mis_misses = 0
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
                recs, em, emission, sc, typ = lit_ref._closest_hits(orc, flat, sh, materials, o, d, tmin, active, b, color, normal, depth)
                if lit_env:  # a miss behind an environment sample (colour is colour * sky here)
                    hit = np.zeros(P, dtype=bool)
                    hit[em] = hit[sc] = True
                    miss = active[~hit[active]]
                    gated = miss[~count_env[miss]]
                    if mis:
                        mis_misses += len(gated)
                        color[gated] = color[gated] * balance(bsdf_pdf[gated], pdf(entries, n_map, d[gated]))[:, None]
                    else:
                        color[gated] = F(0.0)
                if mis:
                    seen = color[em] * emission
                    gated = ~count_emission[em]
                    mis_emitter_hits += int(gated.sum())
                    t = recs["t"][em].astype(np.float32)
                    cos_l = np.abs(_dot(recs["normal"][em].astype(np.float32), d[em]))
                    m_of = recs["material_id"][em].astype(np.int64)
                    p_l = lamp_density(t * t, cos_l, inv_pdf_m[m_of] if inv_pdf_m is not None else np.zeros(len(em), np.float32))
                    color[em] = np.where(gated[:, None], seen * balance(bsdf_pdf[em], p_l)[:, None], seen)
                else:
                    color[em] = np.where(count_emission[em][:, None], color[em] * emission, F(0.0))
                if lit_ref.plays_at(roulette, b, max_bounces):
                    ended, _ = lit_ref.play(orc, color, sc, sc, iteration, b)
                    sc, typ = sc[~ended], typ[~ended]
                lit_ref.shade(orc, materials, o, d, tmin, recs, sc, draws, color)
                df = sc[typ == 0]
                pts = recs["point"][df].astype(np.float32)
                nrm = recs["normal"][df].astype(np.float32)
                weigh = mis and b != max_bounces - 1
                if mis:
                    bsdf_pdf[df] = lobe_density(_dot(nrm, d[df]))
                if lit:
                    count_emission[sc] = typ != 0
                    diffuse_hits += len(df)
                    u = direct_ref.light_draws(orc, df, iteration, 3 * b)
                    smp = direct_ref.light_sample(orc, flat, lamps, pts, nrm, u)
                    contribution = smp["contribution"]
                    if weigh and len(df):
                        d2, cos_l, inv_pdf, cos_r = light_terms(orc, flat, lamps, pts, nrm, u)
                        contribution = contribution * balance(lamp_density(d2, cos_l, inv_pdf), lobe_density(cos_r))[:, None]
                    got, traced = env_light_ref._arrived(orc, flat, sh, smp["sampled"], smp["rays"])
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
                        jac, cos_r = env_terms(entries, n_map, nrm, smp["square"], u)
                        contribution = contribution * balance(env_density(jac), lobe_density(cos_r))[:, None]
                    got, traced = env_light_ref._arrived(orc, flat, sh, smp["sampled"], smp["rays"])
                    env_shadow_rays += traced
                    env_unoccluded += int(got.sum())
                    radiance[df[got]] = radiance[df[got]] + color[df[got]] * contribution[got]
                active = sc
            total = radiance + color if (lit or lit_env) else color
            lit_ref._deposit(frame, np.arange(P), iteration, total, normal, depth)
    return {**lit_ref._planes(frame, h, w), "rays": rays, "diffuse_hits": diffuse_hits, "shadow_rays": shadow_rays, "unoccluded": unoccluded,
            "env_diffuse_hits": env_diffuse_hits, "env_shadow_rays": env_shadow_rays, "env_unoccluded": env_unoccluded,
            "mis_emitter_hits": mis_emitter_hits, "mis_misses": mis_misses}
