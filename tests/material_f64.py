"""A float64 reference of the material evaluation at the end of a bounce, independent of oracle/oracle.c and of the kernels.

Written from the reference's text (path_tracer.cu:130-201 evaluate_material and reflectance, distributions.cuh
random_in_unit_sphere, get_background_color, GLSL's reflect and refract as glm states them) as plain formulas in numpy
float64: Snell's law in vector form, Schlick's polynomial with ** 5, the point on the unit sphere with np.sin / np.cos.  It
does not follow the binary32 order of operations and cannot give the oracle's bits; it says what the colour of a pixel is
to about 1e-6, so that a misreading shared by oracle.c and the kernels (a sign in refract, the side that gets 1 / index,
the metal's acceptance test, the power in Schlick) shows as an error of 1e-2 or more.

Inputs per path come from the oracle's pinned pieces: the primary ray (orc_generate_ray), its hit record
(orc_intersect_rays: point, normal, side, material) and the path's draws (orc_rng_*).  Output for a probe frame (one convex
object under open sky, one iteration): the expected colour per pixel, which paths are compared, and the decision margins.

  max_bounces 1: the throughput the material leaves (albedo; 0 for a rejected metal direction; 1 for glass); the sky for a
                 primary ray that misses.
  max_bounces 2: throughput x sky(scattered direction) for paths whose scattered ray leaves the scene (asked of
                 orc_intersect_rays with the float64 ray rounded to binary32); the others are outside the probe's domain.

A path is also left out if one of its decisions is closer than MARGIN to its threshold (schlick - u, ratio * sin_theta - 1,
dot(dir, n) for metal) or |n + r| < DIFFUSE_MARGIN (normalising amplifies rounding): there binary32 may decide otherwise."""
import ctypes as C

import numpy as np

# max |oracle - float64| over every compared path of every probe frame of material_cases.probe_frames, max_bounces 1 and 2
# (the oracle is the binary32 reference; no GPU result enters).  Obtained with
#     python -m pytest tests/test_material_cases_cpu.py -k "float64 or measured" -s
# which prints every frame's figure and "measured max |oracle - float64| = 7.026265251841579e-07" (the inside-sphere probe,
# two bounces); written here rounded up.  test_measured_maximum_is_the_constant re-derives it and fails if it is exceeded.
MEASURED_MAX_ORACLE_ERROR = 7.03e-7
# binary32 chains of this length differ in rounding by a small factor, not by an order of magnitude
TOLERANCE_FACTOR = 4.0
TOLERANCE = TOLERANCE_FACTOR * MEASURED_MAX_ORACLE_ERROR
MARGIN = 1e-5
DIFFUSE_MARGIN = 1e-3
MAX_MARGIN_EXCLUSIONS = 0.01      # of a probe frame's paths
MIN_DOMAIN = 0.5                  # of a probe frame's paths ...
MIN_DOMAIN_INSIDE = 0.2           # ... and of an inside-sphere probe's, where total reflection stays inside

SKY_HORIZON = np.array([0.5, 0.7, 1.0])
SKY_ZENITH = np.array([1.0, 1.0, 1.0])


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def sky(d):
    """get_background_color: the blend of (0.5, 0.7, 1) and (1, 1, 1) by t = (unit(d).y + 1) / 2."""
    t = 0.5 * (_unit(d)[..., 1] + 1.0)
    return SKY_HORIZON * (1.0 - t)[..., None] + SKY_ZENITH * t[..., None]


def on_unit_sphere(u1, u2):
    """random_in_unit_sphere: longitude 2 pi u1, z = 2 u2 - 1 (a point ON the unit sphere)."""
    phi = 2.0 * np.pi * u1
    z = 2.0 * u2 - 1.0
    s = np.sqrt(1.0 - z * z)
    return np.stack([np.cos(phi) * s, np.sin(phi) * s, z], axis=-1)


def schlick(cosine, ratio):
    r0 = ((1.0 - ratio) / (1.0 + ratio)) ** 2
    return r0 + (1.0 - r0) * (1.0 - cosine) ** 5


def scatter(kind, params, direction, point, normal, side, u1, u2):
    """One evaluate_material in float64, for arrays of paths.  kind: 0 diffuse, 1 metal, 2 glass; params [n, 4] (albedo +
    fuzz, or the index first); normal faces the incoming ray; side 0 = front; u1, u2 the path's next two draws (glass uses
    u1 only, and only if it can refract).  Returns origin, t_min, direction, throughput [n, 3], margins [n] (the smallest
    |decision margin| of the path, inf where it has none) and tiny [n] (|n + r| of a diffuse path, inf otherwise)."""
    n = len(kind)
    d = np.asarray(direction, dtype=np.float64)
    nrm = np.asarray(normal, dtype=np.float64)
    pt = np.asarray(point, dtype=np.float64)
    out_d = np.zeros((n, 3))
    thr = np.ones((n, 3))
    margin = np.full(n, np.inf)
    tiny = np.full(n, np.inf)
    origin = pt - 1e-4 * np.sign(_dot(d, nrm))[:, None] * nrm
    tmin = np.full(n, 1e-4)
    r = on_unit_sphere(u1, u2)

    k = kind == 0
    v = nrm[k] + r[k]
    tiny[k] = np.linalg.norm(v, axis=-1)
    out_d[k] = _unit(v)
    thr[k] = params[k, :3]

    k = kind == 1
    mirrored = d[k] - 2.0 * _dot(d[k], nrm[k])[:, None] * nrm[k]
    out_d[k] = mirrored + params[k, 3:4] * r[k]
    up = _dot(out_d[k], nrm[k])
    margin[k] = np.abs(up)
    thr[k] = np.where((up > 0.0)[:, None], params[k, :3], 0.0)

    k = np.nonzero(kind == 2)[0]
    if len(k):
        index = params[k, 0].astype(np.float64)
        ratio = np.where(side[k] == 0, 1.0 / index, index)      # entering from the front: n_outside / n_inside = 1 / index
        i = _unit(d[k])
        cos_t = np.minimum(-_dot(i, nrm[k]), 1.0)
        sin_t = np.sqrt(1.0 - cos_t * cos_t)
        total = ratio * sin_t > 1.0
        m = np.abs(ratio * sin_t - 1.0)
        s = schlick(cos_t, ratio)
        reflect = total | (s > u1[k])
        m = np.where(total, m, np.minimum(m, np.abs(s - u1[k])))
        margin[k] = m
        mirrored = i - 2.0 * _dot(i, nrm[k])[:, None] * nrm[k]
        # Snell: the tangential part scales by the ratio, the normal part is what keeps the result a unit vector
        tangential = ratio[:, None] * (i + cos_t[:, None] * nrm[k])
        bent = tangential - np.sqrt(np.maximum(1.0 - _dot(tangential, tangential), 0.0))[:, None] * nrm[k]
        out_d[k] = np.where(reflect[:, None], mirrored, bent)
        origin[k] = pt[k]
        tmin[k] = 1e-5
    return origin, tmin, out_d, thr, margin, tiny


def predict(orc, lr, flat, camera, w, h, max_bounces, iteration=0, megakernel=False):
    """The probe frame's expected colours after one iteration, for the streaming loop (a bounce's draws come from a
    generator seeded from (slot, iteration) and advanced by the bounce number) or the megakernel's (one generator per
    pixel: the material's draws follow the two of the pixel's jitter).  Returns dict: color [h, w, 3] float64, compared [h, w] bool,
    margin_excluded (count), out_of_domain (count), hits (count of primary hits)."""
    assert max_bounces in (1, 2)
    sh = orc.SceneHandle(flat)
    lib = orc.lib()
    mats = np.asarray(flat.materials)
    P = w * h
    o, d, tmin, after_jitter = lr._primary(orc, camera, w, h, np.arange(P), iteration)
    recs, hit = orc.intersect_rays(flat, lr._rays(o, tmin, d), scene_handle=sh)
    hit = hit.astype(bool)
    # the path's draws at bounce 0
    u = np.zeros((P, 2))
    st = C.c_uint32()
    for p in np.nonzero(hit)[0]:
        st.value = int(after_jitter[p]) if megakernel else lib.orc_rng_seed(lib.orc_path_seed(int(p), iteration))
        u[p, 0] = lib.orc_rng_uniform(C.byref(st))
        u[p, 1] = lib.orc_rng_uniform(C.byref(st))
    color = sky(d.astype(np.float64))
    compared = np.ones(P, dtype=bool)
    hi = np.nonzero(hit)[0]
    mid = recs["material_id"][hi].astype(np.int64)
    so, stm, sd, thr, margin, tiny = scatter(mats["type"][mid], mats["p"][mid].astype(np.float64), d[hi], recs["point"][hi],
                                             recs["normal"][hi], recs["side"][hi], u[hi, 0], u[hi, 1])
    near = (margin < MARGIN) | (tiny < DIFFUSE_MARGIN)
    if max_bounces == 1:
        color[hi] = thr
        outside = np.zeros(len(hi), dtype=bool)
    else:
        _, hit2 = orc.intersect_rays(flat, lr._rays(so.astype(np.float32), stm.astype(np.float32), sd.astype(np.float32)),
                                     scene_handle=sh)
        outside = hit2.astype(bool)
        color[hi] = thr * sky(sd)
    compared[hi] = ~near & ~outside
    return {"color": color.reshape(h, w, 3), "compared": compared.reshape(h, w), "margin_excluded": int(near.sum()),
            "out_of_domain": int((outside & ~near).sum()), "hits": len(hi), "paths": P}


def worst_error(frame_color, prediction):
    """max |frame - prediction| over the compared paths (0 if none)."""
    m = prediction["compared"]
    if not m.any():
        return 0.0
    return float(np.max(np.abs(frame_color.astype(np.float64)[m] - prediction["color"][m])))
