"""The two render loops of the test tree, in numpy binary32 -- TEST INFRASTRUCTURE: the checker every bit-exact GPU test of a frame
trusts, not the thing under test.  Each loop stands here once and every feature is a switch of it, off by default; the rules the
switches turn on stand in the modules this one imports (lit_ref: the materials, emitters, roulette; direct_ref: the lamps' sample;
env_ref: the sky map; env_light_ref: its sample; lens_ref: the thin lens; mis_ref: the balance weights; smooth_ref: the winner of a hit
and its shading normal; texture_ref: the albedo; normal_map_ref: the bent normal), and none of them imports this one.  The sky and the
lens reach the loops as arguments: nothing is swapped anywhere for the length of a call.  tests/golden/loop_ref.npz and
loop_ref_options.npz pin the bits of every switch (tests/test_loop_ref_golden_cpu.py)."""
import numpy as np

import direct_ref
import env_light_ref
import env_ref
import lens_ref
import lit_ref
import mis_ref
import normal_map_ref
import smooth_ref
import texture_ref
from lit_ref import EMISSIVE, TABLES, _rays, play, plays_at, shade
from ref_f32 import Draws, F, _dot, stream_states

COUNTERS = ("rays", "diffuse_hits", "shadow_rays", "unoccluded", "env_diffuse_hits", "env_shadow_rays", "env_unoccluded",
            "mis_emitter_hits", "mis_misses") + smooth_ref.COUNTERS + texture_ref.COUNTERS + normal_map_ref.COUNTERS


def _fold(fb, local, iteration, value):
    """temporal_accumulate (oracle.c:920-924) into fb[local]."""
    if iteration == 0:
        fb[local] = value
    else:
        sc = F(iteration + 1)
        fb[local] = (fb[local] * (sc - F(1.0)) + value) / sc


def _frame(prev, P):
    """The running means a render folds its samples into, (colour [P, 3], normal [P, 3], depth [P]): zeros, or an earlier
    result's planes (copied: the result handed in stays as it is)."""
    if prev is None:
        return np.zeros((P, 3), np.float32), np.zeros((P, 3), np.float32), np.zeros(P, np.float32)
    return tuple(np.array(prev[k], dtype=np.float32).reshape(shape) for k, shape in (("color", (P, 3)), ("normal", (P, 3)), ("depth", P)))


def _deposit(frame, local, iteration, color, normal, depth):
    """One iteration's samples into the three planes; path i belongs to the frame's place local[i]."""
    for fb, value in zip(frame, (color, normal, depth)):
        _fold(fb, local, iteration, value)


def _planes(frame, rows, w):
    return {"color": frame[0].reshape(rows, w, 3), "normal": frame[1].reshape(rows, w, 3), "depth": frame[2].reshape(rows, w)}


def _sky_of(env):
    """-> (the sky lookup of a frame: the reference's gradient, or the environment's; the map's texels with their apron, or None)"""
    if env is None:
        return lit_ref.sky, None
    texels = env_ref.apron(env)
    return (lambda d: env_ref.lookup(None, d, texels)), texels


def _closest_hits(orc, flat, sh, materials, sky, o, d, tmin, at, bounce, color, normal, depth):
    """The bounce's closest hits of the paths in rows `at`, and what a bounce does before any draw: a miss takes colour * sky(d),
    a hit at bounce 0 records its normal and t, an emitter is told from the rest.
    -> (records [len(o)], rows on an emitter, their emission [.., 3], rows on another material, those materials' types)."""
    recs_at, hit_at = orc.intersect_rays(flat, _rays(o[at], tmin[at], d[at]), scene_handle=sh)
    recs = np.zeros(len(o), dtype=recs_at.dtype)
    recs[at] = recs_at
    hit_at = hit_at.astype(bool)
    miss, hi = at[~hit_at], at[hit_at]
    color[miss] = color[miss] * sky(d[miss])
    if bounce == 0:
        depth[hi] = recs["t"][hi]
        normal[hi] = recs["normal"][hi]
    mat = recs["material_id"][hi].astype(np.int64)
    typ = materials["type"][mat]
    lamp = typ == EMISSIVE
    return recs, hi[lamp], materials["p"][mat[lamp], :3].astype(np.float32), hi[~lamp], typ[~lamp]


def _tally(tables, it, bounce, ended, skip):
    tables["played"][it, bounce], tables["ended"][it, bounce], tables["skipped"][it, bounce] = len(ended), ended.sum(), skip.sum()


def _arrived(orc, flat, sh, sampled, shadow):
    """-> (bool[n]: the sample's shadow ray is free, the number of shadow rays traced)"""
    clear = np.zeros(len(sampled), dtype=bool)
    sel = np.nonzero(sampled)[0]
    if len(sel):
        _, blocked = orc.intersect_rays(flat, shadow[sel], scene_handle=sh)
        clear[sel] = blocked == 0
    return clear, len(sel)


def render_streaming(orc, flat, camera, w, h, iter_begin, iter_count, max_bounces, *, roulette=0, env=None, lens=None, prev=None,
                     pixels=None, slot_offset=None, scene_handle=None, record=None):
    """orc_render_streaming (pixels None) or orc_render_streaming_interleaved (pixels = lit_ref.interleaved_pixels(..),
    slot_offset = the rank's first global slot, added at every bounce) with emitters (a path on an emissive material ends with
    colour * emission, no draw) and, with roulette >= 1, the rule of lit_ref.play on the stream of slot_base + slot.  env: the sky is
    the map's lookup; lens = (radius, focus distance): the primary rays are lens_ref.primary's (section 5i).
    Returns the oracle's dict -- color / normal / depth over the frame's (or the rank's) pixels in order, live [iter, bounce], rays --
    and played / ended / skipped, each [iter, bounce] (0 where no bounce plays).  record: a list that gets play's entries."""
    sh = scene_handle or orc.SceneHandle(flat)
    materials = np.asarray(flat.materials)
    sky, _ = _sky_of(env)
    if pixels is None:
        pixels = np.arange(w * h, dtype=np.int64)
        slot_base = 0
    else:
        slot_base = int(slot_offset)
    P = len(pixels)
    frame = _frame(prev, P)
    live = np.zeros((iter_count, max_bounces), dtype=np.uint32)
    tables = {k: np.zeros((iter_count, max_bounces), dtype=np.int64) for k in TABLES}
    rays = 0
    for it in range(iter_count):
        iteration = iter_begin + it
        o, d, tmin, _ = lens_ref.primary(orc, camera, w, h, pixels, iteration, lens)
        color = np.ones((P, 3), dtype=np.float32)
        normal = -d
        depth = np.full(P, F(1e6), dtype=np.float32)
        local = np.arange(P)  # slot -> the pixel's place in the frame (or in the rank's rows)
        n = P
        for b in range(max_bounces):
            if n == 0:
                break
            live[it, b] = n
            rays += n
            recs, em, emission, sc, _ = _closest_hits(orc, flat, sh, materials, sky, o, d, tmin, np.arange(n), b, color, normal, depth)
            color[em] = color[em] * emission  # the emissive rule: colour * emission, no draw, the path ends
            if plays_at(roulette, b, max_bounces):  # before any material draw of the bounce
                ended, skip = play(orc, color, sc, slot_base + sc, iteration, b, record)
                _tally(tables, it, b, ended, skip)
                sc = sc[~ended]
            states = np.zeros(P, dtype=np.uint32)
            states[sc] = stream_states(orc, slot_base + sc, iteration, 0, b)  # the material stream: keyed on the SLOT, per bounce
            shade(orc, materials, o, d, tmin, recs, sc, Draws(orc, states), color)
            # stable partition on bounces_left > 0 (oracle.c:1082-1104): live first, then the rest, both in order
            goes_on = np.zeros(n, dtype=bool)
            goes_on[sc] = True
            order = np.concatenate([np.nonzero(goes_on)[0], np.nonzero(~goes_on)[0], np.arange(n, P)])
            o, d, tmin, color, normal, depth, local = (a[order] for a in (o, d, tmin, color, normal, depth, local))
            n = len(sc)
        _deposit(frame, local, iteration, color, normal, depth)
    return {**_planes(frame, P // w, w), "live": live, "rays": rays, **tables}


def render_megakernel(orc, flat, camera, w, h, iter_begin, iter_count, max_bounces, *, pkg=None, direct=False, roulette=0, env=None,
                      entries=None, env_light=False, mis=False, normals=None, smooth=False, textures=None, binding=None, texcoords=None,
                      textured=False, nbinding=None, normal_maps=False, lens=None, prev=None, scene_handle=None, record=None):
    """orc_render_megakernel (oracle.c:1280-1330) with the library's extensions: one generator per pixel for the whole path; an emissive
    hit records normal / depth if it is the first hit, then colour *= emission and the path ends, with no draw.  The switches, each in
    effect only under what it needs and inert otherwise:

    env, lens: the sky is the map's lookup; the primary rays are lens_ref.primary's (section 5i).
    direct, in a scene whose lamp table has weight (section 5g): a per-path radiance sum; at every hit on a diffuse material, after
      evaluate_material (colour = throughput x albedo), one light sample (direct_ref.light_sample) at the hit point about the shading
      normal from the stream of direct_ref.light_draws(pixel, iteration, 3 * bounce); a sampled one traces its shadow ray and, if the
      oracle reports no hit, radiance += colour * contribution; an emissive hit ends the path with colour * emission if the vertex
      before drew no lamp sample (the camera, metal, glass), else with 0.
    env_light, with env and its table `entries` (env_light_ref.table_of's; section 5k): after the lamp's sample one environment sample
      from env_light_ref.stream(pixel, iteration, 4 * bounce), counted the same way; a miss takes colour * sky only when the vertex
      before it drew no environment sample, else 0 -- the emission gate in a flag of its own.
    mis, where either light is sampled (section 5l): per path bsdf_pdf = lobe_density(dot(shading normal, new direction)) after
      evaluate_material at a diffuse hit; each light's sample is weighted by the balance of its density against the lobe's, except at
      the last bounce; an emitter hit or a miss behind a gate counts its colour times the balance of bsdf_pdf against the light's
      density, instead of 0.
    smooth, with vertex normals `normals` (section 5n): at every closest hit on a triangle the shading normal (counted as formed or as a
      fall-back) takes the geometric normal's place in the normal plane at bounce 0, in evaluate_material, in the light samples and in
      bsdf_pdf; the geometric normal keeps `side`, the lamp-side cosine of an emitter hit, and the tests below the geometry.
    textured, with textures, a binding and texcoords (section 5o; pkg: the library, for its decode tables): at a triangle hit that
      reaches evaluate_material the material's colour becomes texture_ref.albedo_rows' (counted as a lookup or as a fall-back).
    normal_maps, with textures, texcoords and an nbinding that names a map (section 5q): there, before the albedo, a bound material's
      shading normal becomes normal_map_ref.normal_rows' from there on; the normal plane keeps the normal it had.
    Below the geometry -- at every triangle hit under smooth shading, else where a map bent the normal -- a light's sample whose
      direction has dot(w, g) <= 0 counts as not sampled (culled), and after both samples a diffuse or metal hit whose new direction has
      dot(d, g) <= 0 ends the path with colour 0 (absorbed).
    roulette >= 1: the rule of lit_ref.play on the roulette stream of the PIXEL, after the emitter check and before the map, the texture
      and evaluate_material.  A path that ends leaves colour 0, draws nothing, takes no light sample and counts nowhere; a survivor's
      light samples are weighted with the divided colour.
    Radiance + colour is deposited where either light is sampled, colour itself elsewhere.

    -> dict(color, normal, depth; the counters of COUNTERS, 0 where their switch is off; played, ended, skipped [iter, bounce], 0 where
    no bounce plays).  record: a list that gets play's entries and, per (iteration, bounce) with lamp samples, a "kind": "light" entry
    with the diffuse hits' pixels, points, shading normals, the sample drawn there and which shadow rays came through."""
    sh = scene_handle or orc.SceneHandle(flat)
    materials = np.asarray(flat.materials)
    sky, texels = _sky_of(env)
    lit = False
    if direct:
        lamps = direct_ref.light_table(flat)
        lit = len(lamps[0]) > 0 and float(lamps[1]["total_weight"]) > 0.0
    lit_env = bool(env_light) and env is not None and entries is not None
    mis = bool(mis) and (lit or lit_env)
    n_map = texels.shape[0] - 2 if lit_env else 0
    inv_pdf_m = mis_ref.material_pdf(flat, lamps) if (mis and lit) else None
    sm_on = bool(smooth) and normals is not None
    tex_on = bool(textured) and textures is not None and texcoords is not None
    nm_on = bool(normal_maps) and textures is not None and texcoords is not None and nbinding is not None and bool((np.asarray(nbinding) >= 0).any())
    P = w * h
    frame = _frame(prev, P)
    tables = {k: np.zeros((iter_count, max_bounces), dtype=np.int64) for k in TABLES}
    count = dict.fromkeys(COUNTERS, 0)
    for it in range(iter_count):
        iteration = iter_begin + it
        o, d, tmin, states = lens_ref.primary(orc, camera, w, h, np.arange(P), iteration, lens)
        draws = Draws(orc, states)
        color = np.ones((P, 3), dtype=np.float32)
        radiance = np.zeros((P, 3), dtype=np.float32)
        count_emission = np.ones(P, dtype=bool)  # (stays all True unless lit)
        count_env = np.ones(P, dtype=bool)
        bsdf_pdf = np.zeros(P, dtype=np.float32)
        normal = -d
        depth = np.full(P, F(1e6), dtype=np.float32)
        active = np.arange(P)
        for b in range(max_bounces):
            if len(active) == 0:
                break
            count["rays"] += len(active)
            d_in = d.copy()
            bounce_rays = _rays(o[active], tmin[active], d[active])
            recs, em, emission, sc, typ = _closest_hits(orc, flat, sh, materials, sky, o, d, tmin, active, b, color, normal, depth)
            hit = np.zeros(P, dtype=bool)
            hit[em] = hit[sc] = True
            shaded = recs.copy()  # the records evaluate_material sees: the shading normal, the textured material
            tri = np.zeros(P, dtype=bool)
            if sm_on or tex_on or nm_on:  # the winner of every hit of the bounce (the cost of this statement: five times the rest)
                at_of = np.full(P, -1, dtype=np.int64)
                at_of[active] = np.arange(len(active))
                w_obj, w_first, w_u, w_v = smooth_ref.winners(orc, flat, sh, bounce_rays, recs[active], hit[active])
                tri[active] = w_first >= 0
            trows = active[tri[active]]
            if sm_on and len(trows):  # an emitter's and a path's that roulette will end among them
                k = at_of[trows]
                ns, fell = smooth_ref._shade_rows(flat, normals, w_obj[k], w_first[k], w_u[k], w_v[k], recs["normal"][trows].astype(np.float32),
                                                  d_in[trows])
                shaded["normal"][trows] = ns
                count["shading_normals"] += int((~fell).sum())
                count["fallbacks"] += int(fell.sum())
                if b == 0:
                    normal[trows] = ns
            if lit_env:  # a miss behind an environment sample (colour is colour * sky here)
                miss = active[~hit[active]]
                gated = miss[~count_env[miss]]
                if mis:
                    count["mis_misses"] += len(gated)
                    color[gated] = color[gated] * mis_ref.balance(bsdf_pdf[gated], mis_ref.pdf(entries, n_map, d[gated]))[:, None]
                else:
                    color[gated] = F(0.0)
            if mis:
                seen = color[em] * emission
                gated = ~count_emission[em]
                count["mis_emitter_hits"] += int(gated.sum())
                t = recs["t"][em].astype(np.float32)
                cos_l = np.abs(_dot(recs["normal"][em].astype(np.float32), d[em]))  # the geometric normal
                m_of = recs["material_id"][em].astype(np.int64)
                p_l = mis_ref.lamp_density(t * t, cos_l, inv_pdf_m[m_of] if inv_pdf_m is not None else np.zeros(len(em), np.float32))
                color[em] = np.where(gated[:, None], seen * mis_ref.balance(bsdf_pdf[em], p_l)[:, None], seen)
            else:
                color[em] = np.where(count_emission[em][:, None], color[em] * emission, F(0.0))
            if plays_at(roulette, b, max_bounces):
                ended, skip = play(orc, color, sc, sc, iteration, b, record)
                _tally(tables, it, b, ended, skip)
                sc, typ = sc[~ended], typ[~ended]
            # the paths that reach evaluate_material on a triangle: the map's normal, then the texture's albedo
            shade_materials = materials
            below = tri & sm_on  # where the culls and the absorption apply
            trs = sc[tri[sc]]
            if (nm_on or tex_on) and len(trs):
                k = at_of[trs]
                mat_id = recs["material_id"][trs].astype(np.int64)
                if nm_on:
                    nn, how = normal_map_ref.normal_rows(flat, textures, nbinding, texcoords, w_obj[k], w_first[k], w_u[k], w_v[k], mat_id,
                                                         shaded["normal"][trs].astype(np.float32), recs["normal"][trs].astype(np.float32), d_in[trs])
                    shaded["normal"][trs] = nn
                    count["bent"] += int((how == normal_map_ref.BENT).sum())
                    count["kept"] += int((how == normal_map_ref.KEPT).sum())
                    below[trs[how == normal_map_ref.BENT]] = True
                if tex_on:
                    _, alb, applied, fell = texture_ref.albedo_rows(pkg, flat, textures, binding, texcoords, w_obj[k], w_first[k], w_u[k], w_v[k],
                                                                    mat_id)
                    count["lookups"] += int(applied.sum())
                    count["tex_fallbacks"] += int(fell.sum())
                    copies = materials[mat_id].copy()
                    copies["p"][:, :3] = alb
                    shade_materials = np.concatenate([materials, copies])
                    shaded["material_id"][trs] = len(materials) + np.arange(len(trs))
            shade(orc, shade_materials, o, d, tmin, shaded, sc, draws, color)
            df = sc[typ == 0]
            pts = recs["point"][df].astype(np.float32)
            nrm = shaded["normal"][df].astype(np.float32)
            geo = recs["normal"][df].astype(np.float32)
            weigh = mis and b != max_bounces - 1
            if mis:
                bsdf_pdf[df] = mis_ref.lobe_density(_dot(nrm, d[df]))
            if lit:
                count_emission[sc] = typ != 0
                count["diffuse_hits"] += len(df)
                u = direct_ref.light_draws(orc, df, iteration, 3 * b)
                smp = direct_ref.light_sample(orc, flat, lamps, pts, nrm, u)
                contribution = smp["contribution"]
                if weigh and len(df):
                    d2, cos_l, inv_pdf, cos_r = mis_ref.light_terms(orc, flat, lamps, pts, nrm, u)
                    contribution = contribution * mis_ref.balance(mis_ref.lamp_density(d2, cos_l, inv_pdf), mis_ref.lobe_density(cos_r))[:, None]
                with np.errstate(invalid="ignore"):
                    behind = smp["sampled"] & below[df] & (_dot(smp["rays"][:, 4:7].astype(np.float32), geo) <= F(0.0))
                count["culled_light_samples"] += int(behind.sum())
                got, traced = _arrived(orc, flat, sh, smp["sampled"] & ~behind, smp["rays"])
                count["shadow_rays"] += traced
                count["unoccluded"] += int(got.sum())
                radiance[df[got]] = radiance[df[got]] + color[df[got]] * contribution[got]
                if record is not None:
                    record.append({"kind": "light", "iteration": iteration, "bounce": b, "pixels": df, "points": pts, "normals": nrm,
                                   "sample": smp, "clear": got})
            if lit_env:
                count_env[sc] = typ != 0
                count["env_diffuse_hits"] += len(df)
                v, u = env_light_ref.stream(orc, df, iteration, 4 * b)
                smp = env_light_ref.sample(entries, texels, pts, nrm, v, u)
                contribution = smp["contribution"]
                if weigh and len(df):
                    jac, cos_r = mis_ref.env_terms(entries, n_map, nrm, smp["square"], u)
                    contribution = contribution * mis_ref.balance(mis_ref.env_density(jac), mis_ref.lobe_density(cos_r))[:, None]
                with np.errstate(invalid="ignore"):
                    behind = smp["sampled"] & below[df] & (_dot(smp["w"].astype(np.float32), geo) <= F(0.0))
                count["culled_light_samples"] += int(behind.sum())
                got, traced = _arrived(orc, flat, sh, smp["sampled"] & ~behind, smp["rays"])
                count["env_shadow_rays"] += traced
                count["env_unoccluded"] += int(got.sum())
                radiance[df[got]] = radiance[df[got]] + color[df[got]] * contribution[got]
            # the absorbed continuation: behind the light samples, glass exempt
            with np.errstate(invalid="ignore"):
                gone = below[sc] & (typ != 2) & (_dot(d[sc], recs["normal"][sc].astype(np.float32)) <= F(0.0))
            count["absorbed"] += int(gone.sum())
            color[sc[gone]] = F(0.0)
            active = sc[~gone]
        total = radiance + color if (lit or lit_env) else color  # (no light sampled: the plain kernel deposits colour itself)
        _deposit(frame, np.arange(P), iteration, total, normal, depth)
    return {**_planes(frame, h, w), **count, **tables}
