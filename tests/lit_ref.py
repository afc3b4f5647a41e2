"""CPU restatement of what the render loops are built from, WITH the library's extensions -- emissive materials (ptc_material type 3)
and Russian roulette (ptc_set_param "roulette") -- in numpy binary32.  TEST INFRASTRUCTURE: the pieces of
tests/loop_ref.py, the checker of tests/test_gpu_emissive.py, test_gpu_direct_loop.py and test_gpu_roulette.py, not the thing under
test.  Each rule stands here once; the loops that apply them stand in loop_ref.

The reference has neither, so the oracle (oracle/oracle.c) cannot check them and stays as it is.  loop_ref restates the oracle's
streaming loop (oracle.c:1055-1125, and its interleaved-rows variant) and its megakernel loop (oracle.c:1283-1305) with the rules
added, built from the oracle's pinned pieces:
  - orc_generate_ray (primary rays), orc_intersect_rays (closest hits, each bounce; the HIT FLAG of the shadow rays),
    orc_path_seed / orc_rng_* (every draw), orc_sincos (random_in_unit_sphere);
  - restated operation by operation, here: evaluate_material and random_in_unit_sphere (oracle.c:825-916), the sky, the primary
    rays; there: the stable partition on bounces_left, the cap (paths alive after the last bounce keep the colour the last bounce
    left) and the running-mean gather.
The emissive rule: a path whose closest hit has an emissive material ends at that bounce with colour * emission (a
binary32 multiply per component, like the miss's colour * sky), makes no draw there, and drops out of the partition like a
miss; at bounce 0 it records the hit's normal and t.  The roulette rule stands at play.  On scenes without emitters, with every
option off, every result of the loops equals the oracle's bit for bit (tests/test_lit_ref_cpu.py); tests/golden/loop_ref.npz and
loop_ref_options.npz pin the bits of every option (tests/test_loop_ref_golden_cpu.py).
Every numpy operation below is one binary32 operation of the C source, in its order (numpy does not contract into FMA)."""
import ctypes as C

import numpy as np

from ref_f32 import PI2, Draws, F, _dot, _normalize, _sign, _sincos, stream_draws  # noqa: F401  (Draws: for this module's users)

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


def interleaved_pixels(w, h, rank, nranks, block_rows):
    """The rank's slots -> frame pixels (band_slot_to_pixel, oracle.c:996-1004), in the rank's order."""
    rows = []
    for first in range(rank * block_rows, h, nranks * block_rows):
        rows.extend(range(first, min(first + block_rows, h)))
    return (np.asarray(rows, dtype=np.int64)[:, None] * w + np.arange(w)[None, :]).reshape(-1)


def plays_at(roulette, bounce, max_bounces):
    """Does bounce `bounce` play roulette?  (The host's launch selection, restated.)"""
    return roulette >= 1 and bounce >= roulette and bounce != max_bounces - 1


def play(orc, color, idx, indices, iteration, bounce, record=None):
    """The roulette rule, one binary32 operation per line item.  With k = roulette >= 1, a path plays at
    bounce b iff plays_at(k, b, max_bounces) -- b >= k and b is not the last bounce --, its closest hit exists and the hit's
    material is not emissive; both loops (loop_ref) play after the emitter check and before evaluate_material.  c = the throughput that
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
