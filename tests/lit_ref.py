"""CPU restatement of the render loops WITH the library's extensions -- emissive materials (ptc_material type 3), direct lighting in
the megakernel (ptc_set_param "direct_light") and Russian roulette (ptc_set_param "roulette", section 5h) -- in
numpy binary32.  TEST INFRASTRUCTURE: the checker of tests/test_gpu_emissive.py, test_gpu_direct_loop.py and test_gpu_roulette.py,
not the thing under test.  Each loop and each rule stands here once; a feature is an option of its loop.

The reference has none of the three, so the oracle (oracle/oracle.c) cannot check them and stays as it is.  This file restates
the oracle's streaming loop (oracle.c:1055-1125, and its interleaved-rows variant) and its megakernel loop (oracle.c:
1283-1305) with the rules added, built from the oracle's pinned pieces:
  - orc_generate_ray (primary rays), orc_intersect_rays (closest hits, each bounce; the HIT FLAG of the shadow rays),
    orc_path_seed / orc_rng_* (every draw), orc_sincos (random_in_unit_sphere);
  - restated operation by operation: evaluate_material and random_in_unit_sphere (oracle.c:825-916), the sky, the stable
    partition on bounces_left, the cap (paths alive after the last bounce keep the colour the last bounce left) and the
    running-mean gather; direct_ref.light_table / light_sample (the lamp table and section 5f's light sample).
The emissive rule: a path whose closest hit has an emissive material ends at that bounce with colour * emission (a
binary32 multiply per component, like the miss's colour * sky), makes no draw there, and drops out of the partition like a
miss; at bounce 0 it records the hit's normal and t.  The direct-light rule stands at render_megakernel, the roulette rule at
play.  On scenes without emitters, with both options off, every result equals the oracle's bit for bit
(tests/test_lit_ref_cpu.py); tests/golden/loop_ref.npz pins the bits of every option (tests/test_loop_ref_golden_cpu.py).
Every numpy operation below is one binary32 operation of the C source, in its order (numpy does not contract into FMA)."""
import ctypes as C

import numpy as np

import direct_ref
from ref_f32 import PI2, Draws, F, _dot, _normalize, _sign, _sincos, stream_draws, stream_states

FLT_MAX = F(np.finfo(np.float32).max)
SKY_X = np.array([0.5, 0.7, 1.0], dtype=np.float32)
SKY_Y = np.array([1.0, 1.0, 1.0], dtype=np.float32)
EMISSIVE = 3
ROULETTE_XOR = 0x52524C54                       # kRouletteSeedXor (pt_device.hpp)
TABLES = ("played", "ended", "skipped")


def sky(d):
    """get_background_color (oracle.c:816-823)."""
    u = _normalize(d)
    t = F(0.5) * (u[:, 1] + F(1.0))
    return SKY_X[None, :] * (F(1.0) - t)[:, None] + SKY_Y[None, :] * t[:, None]


def shade(orc, materials, o, d, tmin, rec, idx, draws, color):
    """evaluate_material (oracle.c:855-916) for the paths `idx`, which all hit a non-emissive material, in place on
    o, d, tmin (per path) and color; draws.states[idx] are the paths' generators (advanced as the oracle's are)."""
    if len(idx) == 0:
        return
    mat = materials[rec["material_id"][idx].astype(np.int64)]
    typ = mat["type"]
    p = mat["p"].astype(np.float32)
    n = rec["normal"][idx].astype(np.float32)
    pt = rec["point"][idx].astype(np.float32)
    rd = d[idx]
    side = rec["side"][idx]
    new_o = pt - n * (F(1e-4) * _sign(_dot(rd, n)))[:, None]
    new_d = rd.copy()
    col = color[idx]
    new_tmin = tmin[idx].copy()
    # diffuse and metal: random_in_unit_sphere, two draws (phi, then cos_theta)
    dm = np.nonzero(typ <= 1)[0]
    r = np.zeros((len(idx), 3), dtype=np.float32)
    if len(dm):
        u1 = draws.uniform(idx[dm])
        u2 = draws.uniform(idx[dm])
        phi = PI2 * u1
        cos_t = F(2.0) * u2 - F(1.0)
        sin_t = np.sqrt(F(1.0) - cos_t * cos_t)
        s, c = _sincos(orc, phi)
        r[dm] = np.stack([c * sin_t, s * sin_t, cos_t], axis=-1)
    k0 = np.nonzero(typ == 0)[0]
    if len(k0):
        dir0 = _normalize(n[k0] + r[k0])
        tiny = np.all(np.abs(dir0.astype(np.float64)) < 1e-8, axis=1)
        dir0[tiny] = n[k0][tiny]
        new_d[k0] = dir0
        col[k0] = col[k0] * p[k0, :3]
    k1 = np.nonzero(typ == 1)[0]
    if len(k1):
        n1, d1 = n[k1], rd[k1]
        reflected = d1 - (n1 * _dot(n1, d1)[:, None]) * F(2.0)
        dir1 = reflected + r[k1] * p[k1, 3][:, None]
        new_d[k1] = dir1
        up = _dot(dir1, n1) > F(0.0)
        col[k1] = np.where(up[:, None], col[k1] * p[k1, :3], F(0.0))
    k2 = np.nonzero(typ == 2)[0]
    if len(k2):
        n2 = n[k2]
        ior = p[k2, 0]
        ratio = np.where(side[k2] == 0, F(1.0) / ior, ior)
        unit = _normalize(rd[k2])
        x = _dot(-unit, n2)
        cos_t = np.where(F(1.0) < x, F(1.0), x)  # fmin_sel(x, 1)
        with np.errstate(invalid="ignore"):
            sin_t = np.sqrt(F(1.0) - cos_t * cos_t)
        cannot = ratio * sin_t > F(1.0)
        refl = cannot.copy()
        drawn = np.nonzero(~cannot)[0]  # (the draw is made only when refraction is possible: `||` short-circuits)
        if len(drawn):
            u = draws.uniform(idx[k2[drawn]])
            r0 = (F(1.0) - ratio[drawn]) / (F(1.0) + ratio[drawn])
            r0 = r0 * r0
            xx = F(1.0) - cos_t[drawn]
            x2 = xx * xx
            x4 = x2 * x2
            refl[drawn] = (r0 + (F(1.0) - r0) * (x4 * xx)) > u
        dv = _dot(n2, unit)
        kk = F(1.0) - ratio * ratio * (F(1.0) - dv * dv)
        with np.errstate(invalid="ignore"):
            refr = unit * ratio[:, None] - n2 * (ratio * dv + np.sqrt(kk))[:, None]
        refr = np.where((kk >= F(0.0))[:, None], refr, F(0.0))
        reflect_dir = unit - (n2 * _dot(n2, unit)[:, None]) * F(2.0)
        new_d[k2] = np.where(refl[:, None], reflect_dir, refr)
        new_o[k2] = pt[k2]
        new_tmin[k2] = F(1e-5)
    o[idx], d[idx], tmin[idx], color[idx] = new_o, new_d, new_tmin, col


def _rays(o, tmin, d):
    r = np.empty((len(o), 8), dtype=np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmin, d, FLT_MAX
    return r


def _primary(orc, camera, w, h, pixels, iteration):
    """raygen (oracle.c:1014-1034): per pixel a generator seeded from (pixel, iteration), two draws of jitter."""
    lib = orc.lib()
    gcam = orc.OGPUCamera()
    lib.orc_to_gpu_camera(C.byref(orc.camera_c(camera)), w, h, C.byref(gcam))
    o = np.empty((len(pixels), 3), dtype=np.float32)
    d = np.empty((len(pixels), 3), dtype=np.float32)
    tmin = np.empty(len(pixels), dtype=np.float32)
    states = np.empty(len(pixels), dtype=np.uint32)
    st, ray = C.c_uint32(), orc.ORay()
    for k, pixel in enumerate(pixels):
        pixel = int(pixel)
        st.value = lib.orc_rng_seed(lib.orc_path_seed(pixel, iteration))
        fx = F(pixel % w) + F(lib.orc_rng_uniform(C.byref(st)))
        fy = F(pixel // w) + F(lib.orc_rng_uniform(C.byref(st)))
        lib.orc_generate_ray(C.byref(gcam), float(fx), float(fy), C.byref(ray))
        o[k], d[k], tmin[k] = ray.origin[:], ray.direction[:], ray.t_min
        states[k] = st.value
    return o, d, tmin, states


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


def interleaved_pixels(w, h, rank, nranks, block_rows):
    """The rank's slots -> frame pixels (band_slot_to_pixel, oracle.c:996-1004), in the rank's order."""
    rows = []
    for first in range(rank * block_rows, h, nranks * block_rows):
        rows.extend(range(first, min(first + block_rows, h)))
    return (np.asarray(rows, dtype=np.int64)[:, None] * w + np.arange(w)[None, :]).reshape(-1)


def _closest_hits(orc, flat, sh, materials, o, d, tmin, at, bounce, color, normal, depth):
    """The bounce's closest hits of the paths in rows `at`, and what a bounce does before any draw: a miss takes colour * sky,
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


def plays_at(roulette, bounce, max_bounces):
    """Does bounce `bounce` play roulette?  (The host's launch selection, restated.)"""
    return roulette >= 1 and bounce >= roulette and bounce != max_bounces - 1


def play(orc, color, idx, indices, iteration, bounce, record=None):
    """The roulette rule, one binary32 operation per line item.  With k = roulette >= 1, a path plays at
    bounce b iff plays_at(k, b, max_bounces) -- b >= k and b is not the last bounce --, its closest hit exists and the hit's
    material is not emissive; both loops play after the emitter check and before evaluate_material.  c = the throughput that
    came into the bounce:
      1. q = max(max(c.r, c.g), c.b), by compare and select ((a < b) ? b : a);
      2. q >= 1: nothing happens (no draw, no division);
      3. else u = one uniform() of a generator seeded path_seed(index, iteration) ^ 0x52524c54, after discard(b); index =
         slot_base + slot (streaming) or the pixel (megakernel);
      4. !(u < q): the path ends, its sample is (0, 0, 0), it makes no material draw (and takes no light sample);
      5. else c = (c.r / q, c.g / q, c.b / q), and the bounce goes on as without roulette.
    Here: for the paths `idx` (rows of color; all of them play), whose generators' indices are `indices`, in place on color.
    -> (bool[len(idx)]: the path ends, bool[len(idx)]: it skipped with q >= 1); who did neither survived with the division."""
    c = color[idx]
    m = np.where(c[:, 0] < c[:, 1], c[:, 1], c[:, 0])  # sel_max(c.r, c.g)
    q = np.where(m < c[:, 2], c[:, 2], m)              # sel_max(.., c.b)
    skip = q >= F(1.0)
    drawn = np.nonzero(~skip)[0]
    u = stream_draws(orc, np.asarray(indices)[drawn], iteration, ROULETTE_XOR, bounce, 1)[:, 0]
    with np.errstate(invalid="ignore"):
        goes = u < q[drawn]
    ended = np.zeros(len(idx), dtype=bool)
    ended[drawn[~goes]] = True
    div = drawn[goes]
    c[div] = c[div] / q[div][:, None]
    c[ended] = F(0.0)
    color[idx] = c
    if record is not None:
        record.append({"kind": "roulette", "iteration": iteration, "bounce": bounce, "q": q, "skipped": skip, "ended": ended,
                       "after": c[div].copy(), "indices": np.asarray(indices).copy()})
    return ended, skip


def _tally(tables, it, bounce, ended, skip):
    tables["played"][it, bounce], tables["ended"][it, bounce], tables["skipped"][it, bounce] = len(ended), ended.sum(), skip.sum()


def render_streaming(orc, flat, camera, w, h, iter_begin, iter_count, max_bounces, roulette=0, prev=None, pixels=None,
                     slot_offset=None, scene_handle=None, record=None):
    """orc_render_streaming (pixels None) or orc_render_streaming_interleaved (pixels = interleaved_pixels(..),
    slot_offset = the rank's first global slot, added at every bounce) with emitters and, with roulette >= 1, the rule of
    play on the stream of slot_base + slot.  Returns the oracle's dict -- color / normal / depth over the frame's (or the
    rank's) pixels in order, live [iter, bounce], rays -- and played / ended / skipped, each [iter, bounce] (0 where no bounce
    plays).  record: a list that gets play's entries."""
    sh = scene_handle or orc.SceneHandle(flat)
    materials = np.asarray(flat.materials)
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
        o, d, tmin, _ = _primary(orc, camera, w, h, pixels, iteration)
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
            recs, em, emission, sc, _ = _closest_hits(orc, flat, sh, materials, o, d, tmin, np.arange(n), b, color, normal, depth)
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


def render_megakernel(orc, flat, camera, w, h, iter_begin, iter_count, max_bounces, direct=False, roulette=0, prev=None,
                      scene_handle=None, record=None):
    """orc_render_megakernel (oracle.c:1280-1330) with emitters: one generator per pixel for the whole path; an emissive
    hit records normal / depth if it is the first hit, then colour *= emission and the path ends, with no draw.

    direct: the rule of DESIGN section 5g (ptc_set_param "direct_light" 1).  A per-path radiance sum, deposited as radiance +
    colour; at every hit on a diffuse material, after evaluate_material (colour = throughput x albedo), one light sample
    (direct_ref.light_sample: section 5f, items 2-5) at the hit point about the hit's normal from the stream
    seed(path_seed(pixel, iteration) ^ kLightSeedXor), discard(3 * bounce); a sampled sample traces {p, 1e-4, w, d * 0.999} and,
    if the oracle reports no hit, radiance += colour * contribution; an emissive hit ends the path with colour * emission if
    the vertex before drew no light sample (the camera, metal, glass), else with 0.  A scene whose lamp table is empty or has no
    weight renders as without the option.

    roulette >= 1: the rule of play, on the roulette stream of the PIXEL.  A path that ends leaves colour 0, draws nothing, takes
    no light sample and adds nothing to the three loop counters; a survivor's light sample is weighted with the divided colour.

    -> dict(color, normal, depth, rays, diffuse_hits, shadow_rays, unoccluded, played, ended, skipped); the counters are 0
    without direct, the tables ([iter, bounce]) where no bounce plays.  record: a list that gets play's entries and, per
    (iteration, bounce) with light samples, a "kind": "light" entry with the diffuse hits' pixels, points, normals, the sample
    drawn there and which shadow rays came through."""
    sh = scene_handle or orc.SceneHandle(flat)
    materials = np.asarray(flat.materials)
    lit = False
    if direct:
        lamps = direct_ref.light_table(flat)
        lit = len(lamps[0]) > 0 and float(lamps[1]["total_weight"]) > 0.0
    P = w * h
    frame = _frame(prev, P)
    tables = {k: np.zeros((iter_count, max_bounces), dtype=np.int64) for k in TABLES}
    rays = diffuse_hits = shadow_rays = unoccluded = 0
    for it in range(iter_count):
        iteration = iter_begin + it
        o, d, tmin, states = _primary(orc, camera, w, h, np.arange(P), iteration)
        draws = Draws(orc, states)
        color = np.ones((P, 3), dtype=np.float32)
        radiance = np.zeros((P, 3), dtype=np.float32)
        count_emission = np.ones(P, dtype=bool)  # (stays all True unless lit)
        normal = -d
        depth = np.full(P, F(1e6), dtype=np.float32)
        active = np.arange(P)
        for b in range(max_bounces):
            if len(active) == 0:
                break
            rays += len(active)
            recs, em, emission, sc, typ = _closest_hits(orc, flat, sh, materials, o, d, tmin, active, b, color, normal, depth)
            color[em] = np.where(count_emission[em][:, None], color[em] * emission, F(0.0))
            if plays_at(roulette, b, max_bounces):
                ended, skip = play(orc, color, sc, sc, iteration, b, record)
                _tally(tables, it, b, ended, skip)
                sc, typ = sc[~ended], typ[~ended]
            shade(orc, materials, o, d, tmin, recs, sc, draws, color)
            if lit:
                count_emission[sc] = typ != 0
                df = sc[typ == 0]
                diffuse_hits += len(df)
                pts = recs["point"][df].astype(np.float32)
                nrm = recs["normal"][df].astype(np.float32)
                u = direct_ref.light_draws(orc, df, iteration, 3 * b)
                smp = direct_ref.light_sample(orc, flat, lamps, pts, nrm, u)
                sel = np.nonzero(smp["sampled"])[0]
                shadow_rays += len(sel)
                clear = np.zeros(len(df), dtype=bool)
                if len(sel):
                    _, blocked = orc.intersect_rays(flat, smp["rays"][sel], scene_handle=sh)
                    clear[sel] = blocked == 0
                unoccluded += int(clear.sum())
                got = df[clear]
                radiance[got] = radiance[got] + color[got] * smp["contribution"][clear]
                if record is not None:
                    record.append({"kind": "light", "iteration": iteration, "bounce": b, "pixels": df, "points": pts, "normals": nrm,
                                   "sample": smp, "clear": clear})
            active = sc
        total = radiance + color if lit else color   # (no lamp table: the plain kernel deposits colour itself)
        _deposit(frame, np.arange(P), iteration, total, normal, depth)
    return {**_planes(frame, h, w), "rays": rays, "diffuse_hits": diffuse_hits, "shadow_rays": shadow_rays,
            "unoccluded": unoccluded, **tables}
