"""CPU restatement of the render loops WITH emissive materials (ptc_material type 3), in numpy binary32.

The reference has no emitters, so the oracle (oracle/oracle.c) cannot check them and stays as it is.  This file restates
the oracle's streaming loop (oracle.c:1055-1125, and its interleaved-rows variant) and its megakernel loop (oracle.c:
1283-1305) with the emissive rule added, built from the oracle's pinned pieces:
  - orc_generate_ray (primary rays), orc_intersect_rays (closest hits, each bounce), orc_path_seed / orc_rng_* (every draw),
    orc_sincos (random_in_unit_sphere);
  - restated operation by operation: evaluate_material and random_in_unit_sphere (oracle.c:825-916), the sky, the stable
    partition on bounces_left, the cap (paths alive after the last bounce keep the colour the last bounce left) and the
    running-mean gather.
The emissive rule: a path whose closest hit has an emissive material ends at that bounce with colour * emission (a
binary32 multiply per component, like the miss's colour * sky), makes no draw there, and drops out of the partition like a
miss; at bounce 0 it records the hit's normal and t.  On scenes without emitters every result equals the oracle's bit for
bit (tests/test_lit_ref_cpu.py): the restatement is the checker of tests/test_gpu_emissive.py, not the thing under test.
Every numpy operation below is one binary32 operation of the C source, in its order (numpy does not contract into FMA)."""
import ctypes as C

import numpy as np

F = np.float32
PI2 = F(2.0) * F(3.14159265358979323846264338327950288)  # 2.f * pi_f, as the C expression folds it
FLT_MAX = F(np.finfo(np.float32).max)
SKY_X = np.array([0.5, 0.7, 1.0], dtype=np.float32)
SKY_Y = np.array([1.0, 1.0, 1.0], dtype=np.float32)
EMISSIVE = 3


def _dot(a, b):
    t = a * b  # glm::dot: tmp = a * b; tmp.x + tmp.y + tmp.z
    return (t[:, 0] + t[:, 1]) + t[:, 2]


def _normalize(v):
    return v * (F(1.0) / np.sqrt(_dot(v, v)))[:, None]  # v * (1 / sqrt(dot(v, v)))


def _sign(x):
    return ((F(0.0) < x).astype(np.float32) - (x < F(0.0)).astype(np.float32)).astype(np.float32)


class Draws:
    """thrust::minstd_rand states, one per path, advanced through the oracle (orc_rng_uniform)."""

    def __init__(self, orc, states):
        self.h = orc.lib()
        self.states = np.asarray(states, dtype=np.uint32).copy()

    def uniform(self, idx):
        out = np.empty(len(idx), dtype=np.float32)
        st = C.c_uint32()
        for k, i in enumerate(idx):
            st.value = int(self.states[i])
            out[k] = self.h.orc_rng_uniform(C.byref(st))
            self.states[i] = st.value
        return out


def _sincos(orc, phi):
    s, c = np.empty_like(phi), np.empty_like(phi)
    fs, fc = C.c_float(), C.c_float()
    h = orc.lib()
    for k, x in enumerate(phi):
        h.orc_sincos(float(x), C.byref(fs), C.byref(fc))
        s[k], c[k] = fs.value, fc.value
    return s, c


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


def interleaved_pixels(w, h, rank, nranks, block_rows):
    """The rank's slots -> frame pixels (band_slot_to_pixel, oracle.c:996-1004), in the rank's order."""
    rows = []
    for first in range(rank * block_rows, h, nranks * block_rows):
        rows.extend(range(first, min(first + block_rows, h)))
    return (np.asarray(rows, dtype=np.int64)[:, None] * w + np.arange(w)[None, :]).reshape(-1)


def render_streaming(orc, flat, camera, w, h, iter_begin, iter_count, max_bounces, prev=None, pixels=None,
                     slot_offset=None, scene_handle=None):
    """orc_render_streaming (pixels None) or orc_render_streaming_interleaved (pixels = interleaved_pixels(..),
    slot_offset = the rank's first global slot, added at every bounce) with emitters.  Returns the oracle's dict:
    color / normal / depth over the frame's (or the rank's) pixels in order, live [iter, bounce], rays."""
    sh = scene_handle or orc.SceneHandle(flat)
    materials = np.asarray(flat.materials)
    if pixels is None:
        pixels = np.arange(w * h, dtype=np.int64)
        slot_base = 0
    else:
        slot_base = int(slot_offset)
    P = len(pixels)
    rows = P // w
    if prev is None:
        fc, fn, fd = np.zeros((P, 3), np.float32), np.zeros((P, 3), np.float32), np.zeros(P, np.float32)
    else:
        fc = np.array(prev["color"], dtype=np.float32).reshape(P, 3)
        fn = np.array(prev["normal"], dtype=np.float32).reshape(P, 3)
        fd = np.array(prev["depth"], dtype=np.float32).reshape(P)
    lib = orc.lib()
    live = np.zeros((iter_count, max_bounces), dtype=np.uint32)
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
            recs, hit = orc.intersect_rays(flat, _rays(o[:n], tmin[:n], d[:n]), scene_handle=sh)
            hit = hit.astype(bool)
            goes_on = hit.copy()  # bounces_left > 0
            miss = np.nonzero(~hit)[0]
            color[miss] = color[miss] * sky(d[miss])
            hi = np.nonzero(hit)[0]
            if b == 0:
                depth[hi] = recs["t"][hi]
                normal[hi] = recs["normal"][hi]
            mat_type = np.full(n, -1, dtype=np.int64)
            mat_type[hi] = materials["type"][recs["material_id"][hi].astype(np.int64)]
            em = np.nonzero(mat_type == EMISSIVE)[0]
            if len(em):  # the emissive rule: colour * emission, no draw, the path ends
                color[em] = color[em] * materials["p"][recs["material_id"][em].astype(np.int64), :3].astype(np.float32)
                goes_on[em] = False
            sc = np.nonzero(hit & (mat_type != EMISSIVE))[0]
            states = np.zeros(n, dtype=np.uint32)
            st = C.c_uint32()
            for i in sc:
                st.value = lib.orc_rng_seed(lib.orc_path_seed(slot_base + int(i), iteration))
                lib.orc_rng_discard(C.byref(st), b)
                states[i] = st.value
            shade(orc, materials, o, d, tmin, recs, sc, Draws(orc, states), color)
            # stable partition on bounces_left > 0 (oracle.c:1082-1104): live first, then the rest, both in order
            order = np.concatenate([np.nonzero(goes_on)[0], np.nonzero(~goes_on)[0], np.arange(n, P)])
            o, d, tmin, color, normal, depth, local = (a[order] for a in (o, d, tmin, color, normal, depth, local))
            n = int(goes_on.sum())
        for fb, val in ((fc, color), (fn, normal)):
            for k in range(3):
                col = fb[:, k].copy()
                _fold(col, local, iteration, val[:, k])
                fb[:, k] = col
        _fold(fd, local, iteration, depth)
    return {"color": fc.reshape(rows, w, 3), "normal": fn.reshape(rows, w, 3), "depth": fd.reshape(rows, w),
            "live": live, "rays": rays}


def render_megakernel(orc, flat, camera, w, h, iter_begin, iter_count, max_bounces, prev=None, scene_handle=None):
    """orc_render_megakernel (oracle.c:1280-1330) with emitters: one generator per pixel for the whole path; an emissive
    hit records normal / depth if it is the first hit, then colour *= emission and the path ends, with no draw."""
    sh = scene_handle or orc.SceneHandle(flat)
    materials = np.asarray(flat.materials)
    P = w * h
    if prev is None:
        fc, fn, fd = np.zeros((P, 3), np.float32), np.zeros((P, 3), np.float32), np.zeros(P, np.float32)
    else:
        fc = np.array(prev["color"], dtype=np.float32).reshape(P, 3)
        fn = np.array(prev["normal"], dtype=np.float32).reshape(P, 3)
        fd = np.array(prev["depth"], dtype=np.float32).reshape(P)
    rays = 0
    for it in range(iter_count):
        iteration = iter_begin + it
        o, d, tmin, states = _primary(orc, camera, w, h, np.arange(P), iteration)
        draws = Draws(orc, states)
        color = np.ones((P, 3), dtype=np.float32)
        normal = -d
        depth = np.full(P, F(1e6), dtype=np.float32)
        active = np.arange(P)
        for b in range(max_bounces):
            if len(active) == 0:
                break
            rays += len(active)
            recs_a, hit_a = orc.intersect_rays(flat, _rays(o[active], tmin[active], d[active]), scene_handle=sh)
            recs = np.zeros(P, dtype=recs_a.dtype)
            recs[active] = recs_a
            hit = np.zeros(P, dtype=bool)
            hit[active] = hit_a.astype(bool)
            miss = active[~hit[active]]
            color[miss] = color[miss] * sky(d[miss])
            hi = active[hit[active]]
            if b == 0:
                depth[hi] = recs["t"][hi]
                normal[hi] = recs["normal"][hi]
            mt = materials["type"][recs["material_id"][hi].astype(np.int64)]
            em = hi[mt == EMISSIVE]
            color[em] = color[em] * materials["p"][recs["material_id"][em].astype(np.int64), :3].astype(np.float32)
            sc = hi[mt != EMISSIVE]
            shade(orc, materials, o, d, tmin, recs, sc, draws, color)
            active = sc
        for fb, val in ((fc, color), (fn, normal)):
            for k in range(3):
                col = fb[:, k].copy()
                _fold(col, np.arange(P), iteration, val[:, k])
                fb[:, k] = col
        _fold(fd, np.arange(P), iteration, depth)
    return {"color": fc.reshape(h, w, 3), "normal": fn.reshape(h, w, 3), "depth": fd.reshape(h, w), "rays": rays}
