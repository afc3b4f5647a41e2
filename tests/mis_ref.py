"""CPU restatement of multiple importance sampling in the megakernel (ptc_set_param "mis", ptc_environment_light_pdf,
ptc_light_material_pdf) in numpy binary32 -- TEST INFRASTRUCTURE: the checker of tests/test_mis_cpu.py and
tests/test_gpu_mis.py, not the thing under test.

What stands here: the balance heuristic's weight and the three densities of section 5l, every numpy operation one binary32 operation of
the rule in its order; the square a direction falls in and the environment sample's density there; and the per-material array of the
lamp table.  The loop that applies them is loop_ref.render_megakernel's under `mis`.  The terms of a lamp's sample (d^2 and the two
cosines) are not among what direct_ref.light_sample returns: light_terms forms them again from the same draws, with direct_ref's own
lines."""
import numpy as np

import direct_ref
import env_light_ref
import env_ref
from ref_f32 import PI, PI2, F, _dot, _normalize, _sincos, _xform_point

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
