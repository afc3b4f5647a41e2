"""The light sample of DESIGN section 5f in float64, per sample, and the case classes it is compared on -- TEST INFRASTRUCTURE.

sample64: for a given (lamp record, u1, u2) the point q on the lamp, the direction w, the distance d, both cosines, g, the contribution
and the culls, written from the formulas in float64.  Its inputs are what the device's inputs are: the lamp records (binary32 fields,
taken as exact), a sphere lamp's object matrix and sphere, the material's emission, the point and its normal, the draws.

Distances from float64 are counted in units of 2^-24 times a conditioning term, because the classes go where binary32 has little left:
    cond   = 1 + (|p| + the magnitudes q is summed from) / d     (q - p cancels: a rounding of q or p is 2^-24 of its size, not of d)
    cond_l = 1 + (|centre| + R) / R for a sphere lamp, else 0    (n_l = normalize(q - centre) cancels the same way)
    direction     max |w32 - w64|                     / (2^-24 cond)
    tmax          |tmax32 - float32(0.999) d64|       / (2^-24 cond d64)
    contribution  max |c32 - c64|                     / (2^-24 (cond + cond_l) max(Le) inv_pdf / (pi d64^2))
TOLERANCE holds, per class, four times the worst distance of the numpy restatement (tests/direct_ref.py, which is the device's
arithmetic operation for operation) measured on this module's cases on a CPU:

    class        direction   tmax   contribution   (worst distances measured, in the units above)
    far            0.247     0.232     0.513
    sizes          2.701     1.787     2.557
    plane          0.679     0.623     0.357
    inside         0.579     0.479     0.649
    normals        0.585     0.693     0.302
    distant        0.735     0.919     1.813
    edge_draws     0.735     0.834     1.965

Samples that float64 itself puts within the tolerance of a cull boundary (cos_r = 0, d2 = 0, d2 = 2^128) are left out: near_cull picks
them from the float64 values alone, and the classes are built so that it picks at most 1 % of any (the CPU test checks that).  A sample
exactly ON a boundary by construction (a point that coincides with the sampled vertex: d2 = 0 in every precision) stays in."""
import numpy as np

import direct_ref as D

EPS = 2.0 ** -24
F = np.float32
TOLERANCE = {   # class -> (direction, tmax, contribution): 4 x the measured worst distance of the restatement, rounded up
    "far": (1.0, 0.93, 2.1),
    "sizes": (11.0, 7.2, 11.0),
    "plane": (2.8, 2.5, 1.5),
    "inside": (2.4, 2.0, 2.6),
    "normals": (2.4, 2.8, 1.3),
    "distant": (3.0, 3.7, 7.3),
    "edge_draws": (3.0, 3.4, 7.9),
}
BELOW_ONE = float(np.nextafter(F(1.0), F(0.0)))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def sample64(flat, recs, lamp, p, nrm, u1, u2):
    """-> dict of float64 arrays over the samples: q, w, d, d2, cos_r, cos_l, contribution [n, 3], sampled, tmax, cond, cond_l, scale (the
    contribution with both cosines 1).  lamp: record index per sample."""
    r = recs[lamp]
    n = len(lamp)
    p, nrm = np.asarray(p, dtype=np.float64), np.asarray(nrm, dtype=np.float64)
    u1, u2 = np.asarray(u1, dtype=np.float64), np.asarray(u2, dtype=np.float64)
    p0, e1, e2 = r["p0"].astype(np.float64), r["e1"].astype(np.float64), r["e2"].astype(np.float64)
    is_sphere = (r["kind_material"] >> 31) != 0
    q, nl = np.zeros((n, 3)), np.zeros((n, 3))
    size = np.linalg.norm(p0, axis=1) + np.linalg.norm(e1, axis=1) + np.linalg.norm(e2, axis=1)
    cond_l = np.zeros(n)
    su = np.sqrt(u1)
    q_tri = p0 + e1 * (1.0 - su)[:, None] + e2 * (u2 * su)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        n_tri = _unit(np.cross(e1, e2))
    z = 1.0 - 2.0 * u1
    rr = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = 2.0 * np.pi * u2
    direction = np.stack([rr * np.cos(phi), rr * np.sin(phi), z], axis=-1)
    spheres = np.asarray(flat.spheres, dtype=np.float64).reshape(-1, 4)
    for k in np.nonzero(is_sphere)[0]:
        obj = flat.objects[int(r["object"][k])]
        m = np.asarray(obj["m"], dtype=np.float64).reshape(4, 4)   # m[col, row]
        sp = spheres[int(obj["index"])]
        qo = np.append(sp[:3] + direction[k] * sp[3], 1.0) @ m
        co = np.append(sp[:3], 1.0) @ m
        q[k], centre = qo[:3] / qo[3], co[:3] / co[3]
        nl[k] = _unit(q[k] - centre)
        radius = np.linalg.norm(q[k] - centre)
        scale_of_m = np.linalg.norm(m[0, :3])
        size[k] = np.linalg.norm(centre) + radius + scale_of_m * (np.linalg.norm(sp[:3]) + abs(sp[3])) + np.linalg.norm(m[3, :3])
        cond_l[k] = 1.0 + (np.linalg.norm(centre) + radius) / radius
    q[~is_sphere], nl[~is_sphere] = q_tri[~is_sphere], n_tri[~is_sphere]
    v = q - p
    d2 = np.sum(v * v, axis=1)
    valid = (d2 > 0.0) & (d2 < 2.0 ** 128)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.sqrt(d2)
        w = v / d[:, None]
        cos_r = np.sum(nrm * w, axis=1)
        cos_l = np.abs(np.sum(nl * w, axis=1))
        inv_pdf = r["inv_pdf"].astype(np.float64)
        le = np.asarray(flat.materials)["p"][(r["kind_material"] & 0x7FFFFFFF).astype(np.int64), :3].astype(np.float64)
        scale = le.max(axis=1) * inv_pdf / (np.pi * d2)
        g = cos_r * cos_l * inv_pdf / (np.pi * d2)
        cond = 1.0 + (np.linalg.norm(p, axis=1) + size) / d
    sampled = valid & (cos_r > 0.0) & (inv_pdf > 0.0)
    contribution = np.where(sampled[:, None], le * g[:, None], 0.0)
    return {"q": q, "w": w, "d": d, "d2": d2, "cos_r": cos_r, "cos_l": cos_l, "contribution": contribution, "sampled": sampled,
            "tmax": float(F(0.999)) * d, "cond": cond, "cond_l": cond_l, "scale": scale, "valid": valid}


def near_cull(ref, tol):
    """The samples float64 puts within the tolerance of a cull boundary; from ref (sample64's values) alone."""
    reach = 2.0 * tol[0] * EPS * ref["cond"]   # (|cos_r32 - cos_r64| <= sqrt(3) max |w32 - w64| for a unit normal)
    with np.errstate(invalid="ignore"):
        grazing = ref["valid"] & (np.abs(ref["cos_r"]) <= reach)
        coincident = (ref["d2"] > 0.0) & (reach >= 1.0)                       # q - p is all rounding
        overflow = (ref["d2"] > 0.0) & (np.abs(ref["d2"] / 2.0 ** 128 - 1.0) <= reach)
    return grazing | coincident | overflow


def distances(got, ref, keep):
    """(direction, tmax, contribution): the worst distances of a binary32 result (rays [n, 8], contribution [n, 3]) from ref over the
    samples `keep` that ref samples, in the module's units.  A sample ref culls has no distance: its outputs are zeros or they are
    wrong (the caller compares the flags and the zeros)."""
    s = keep & ref["sampled"]
    if not s.any():
        return 0.0, 0.0, 0.0
    cond = ref["cond"][s]
    dw = np.max(np.abs(got["rays"][s, 4:7].astype(np.float64) - ref["w"][s]), axis=1) / (EPS * cond)
    dt = np.abs(got["rays"][s, 7].astype(np.float64) - ref["tmax"][s]) / (EPS * cond * ref["d"][s])
    dc = np.max(np.abs(got["contribution"][s].astype(np.float64) - ref["contribution"][s]), axis=1) / (
        EPS * (cond + ref["cond_l"][s]) * ref["scale"][s])
    return float(dw.max()), float(dt.max()), float(dc.max())


# ---- the classes ------------------------------------------------------------------------------------------------------------
def _scene(pkg, lamps):
    """lamps: ("tri", v0, v1, v2, transform, emission) | ("sphere", centre, radius, transform, emission), in table order."""
    s = pkg.SceneDescription()
    for j, lamp in enumerate(lamps):
        name = "lamp%03d" % j
        s.add_material(name, pkg.EmissiveMaterial(tuple(lamp[-1])))
        if lamp[0] == "sphere":
            s.add_object(pkg.Sphere(tuple(lamp[1]), float(lamp[2])), lamp[3], name)
        else:
            mesh = s.add_mesh("models/%s.obj" % name, pkg.Mesh(np.array(lamp[1:4], dtype=np.float32), np.arange(3, dtype=np.uint32)))
            s.add_object(mesh, lamp[4], name)
    return s.build_scene(distinct_meshes=True)


def _first_states(weights):
    """per lamp the first raw draw that picks it (0: a lamp nothing picks)"""
    t = np.concatenate([[0], D.thresholds(weights).astype(np.int64)])
    return np.where(np.diff(t) > 0, t[:-1] + 1, 0)


def _towards(rng, p, target, spread, away=None):
    """unit normals about the direction from p to target, tilted by `spread`; away: a mask of those turned round"""
    n = _unit(_unit(np.asarray(target, dtype=np.float64) - p) + spread * rng.normal(size=p.shape))
    if away is not None:
        n[away] = -n[away]
    return n


def _finish(flat, lamp, p, nrm, u1, u2):
    recs, _, weights, _ = D.light_table(flat)
    first = _first_states(weights)
    lamp = np.asarray(lamp, dtype=np.int64)
    assert np.all(first[lamp] > 0)
    f32 = lambda a, c: np.ascontiguousarray(a, dtype=np.float32).reshape(-1, c) if c else np.ascontiguousarray(a, dtype=np.float32)
    return {"flat": flat, "recs": recs, "lamp": lamp, "v": first[lamp].astype(np.uint32), "p": f32(p, 3), "nrm": f32(_unit(nrm), 3),
            "u": np.stack([f32(u1, 0), f32(u2, 0)], axis=1)}


def classes(pkg):
    """name -> list of cases dict(flat, recs, lamp, v, p, nrm, u): the lamps of a scene, the points and normals sampled against them,
    the raw draw that picks each sample's lamp and its u1, u2.  Seeded."""
    glm = pkg.glmlite
    rng = np.random.default_rng(5)
    le = (3.0, 2.0, 4.0)
    out = {k: [] for k in TOLERANCE}

    def cloud(n, lo, hi):
        return rng.uniform(lo, hi, (n, 3))

    # far scenes: everything translated by 1e3 and 1e4 on all axes, lamp edges 1 and 0.01
    for shift in (1e3, 1e4):
        for edge in (1.0, 0.01):
            t = glm.translate((shift, shift, shift))
            flat = _scene(pkg, [("tri", (0, 1.5, 0), (edge, 1.5, 0), (0, 1.5, edge), t, le), ("sphere", (0.5, 1.5, -1.0), 0.25 * edge, t, le)])
            n = 1000
            p = cloud(n, (-1, -1, -1), (1, 0.5, 1)) + shift
            lamp = rng.integers(0, 2, n)
            target = np.where(lamp[:, None] == 0, [0.0, 1.5, 0.0], [0.5, 1.5, -1.0]) + shift
            out["far"].append(_finish(flat, lamp, p, _towards(rng, p, target, 0.4, away=rng.random(n) < 0.1), rng.random(n), rng.random(n)))
    # extreme sizes: triangle lamps of edge 1e-4 and 1e4, sphere lamps of radius 1e-4 and 1000 under rotation x uniform scale
    spin = lambda k: glm.compose([glm.rotate(0.6, (1, 1, 0)), glm.scale(k)])
    n = 1000
    flat = _scene(pkg, [("tri", (0, 0, 0), (1e-4, 0, 0), (0, 0, 1e-4), glm.identity(), le)])
    p = _unit(rng.normal(size=(n, 3))) * 10.0 ** rng.uniform(-3, 0, (n, 1))
    out["sizes"].append(_finish(flat, np.zeros(n), p, _towards(rng, p, (0, 0, 0), 0.4), rng.random(n), rng.random(n)))
    flat = _scene(pkg, [("tri", (0, 0, 0), (1e4, 0, 0), (0, 0, 1e4), glm.identity(), le)])
    u1, u2 = rng.random(n), rng.random(n)
    foot = np.stack([1e4 * (1 - np.sqrt(u1)), np.zeros(n), 1e4 * u2 * np.sqrt(u1)], axis=1)   # below the sample, then off to a side
    p = foot + np.stack([rng.normal(size=n), -(10.0 ** rng.uniform(0, 2, n)), rng.normal(size=n)], axis=1)
    out["sizes"].append(_finish(flat, np.zeros(n), p, _towards(rng, p, foot, 0.3), u1, u2))
    flat = _scene(pkg, [("sphere", (0, 0, 0), 1e-3, spin(0.1), le)])
    p = _unit(rng.normal(size=(n, 3))) * 10.0 ** rng.uniform(-2.5, 0, (n, 1))
    out["sizes"].append(_finish(flat, np.zeros(n), p, _towards(rng, p, (0, 0, 0), 0.4), rng.random(n), rng.random(n)))
    flat = _scene(pkg, [("sphere", (0, 0, 0), 500.0, spin(2.0), le)])
    p = _unit(rng.normal(size=(n, 3))) * (1000.0 + 10.0 ** rng.uniform(0, 3, (n, 1)))
    out["sizes"].append(_finish(flat, np.zeros(n), p, _towards(rng, p, (0, 0, 0), 0.3), rng.random(n), rng.random(n)))
    # the lamp's plane (cos_l = 0 exactly: every y is 1), 1e-6 from a lamp, on the sampled vertex itself (u1 = 0: q = p0 + e1, d2 = 0)
    flat = _scene(pkg, [("tri", (0, 1, 0), (1, 1, 0), (0, 1, 1), glm.identity(), le)])
    p = np.stack([rng.uniform(1.5, 3, n), np.ones(n), rng.uniform(1.5, 3, n)], axis=1)
    out["plane"].append(_finish(flat, np.zeros(n), p, _towards(rng, p, (0.3, 1, 0.3), 0.3), rng.random(n), rng.random(n)))
    p = np.tile([1.0, 1.0, 0.0], (n, 1))
    out["plane"].append(_finish(flat, np.zeros(n), p, _unit(rng.normal(size=(n, 3))), np.zeros(n), rng.random(n)))
    flat = _scene(pkg, [("tri", (0, 0, 0), (1e-4, 0, 0), (0, 0, 1e-4), glm.identity(), le)])
    u1, u2 = rng.random(n), rng.random(n)
    foot = np.stack([1e-4 * (1 - np.sqrt(u1)), np.zeros(n), 1e-4 * u2 * np.sqrt(u1)], axis=1)
    p = foot + np.stack([1e-5 * rng.normal(size=n), np.full(n, -1e-6), 1e-5 * rng.normal(size=n)], axis=1)
    out["plane"].append(_finish(flat, np.zeros(n), p, _towards(rng, p, foot, 0.3), u1, u2))
    # inside a sphere lamp, and at its centre
    flat = _scene(pkg, [("sphere", (0.1, 0.2, -0.1), 0.5, glm.compose([glm.rotate(0.6, (1, 1, 0)), glm.scale(2.0), glm.translate((0.9, 1.2, -1.2))]), le)])
    centre = D.light_table(flat)[0]["p0"][0].astype(np.float64)
    p = centre + _unit(rng.normal(size=(n, 3))) * rng.uniform(0, 0.95, (n, 1))
    p[:100] = centre
    u1, u2 = rng.random(n), rng.random(n)
    z = 1 - 2 * u1
    aim = centre + np.stack([np.sqrt(1 - z * z) * np.cos(2 * np.pi * u2), np.sqrt(1 - z * z) * np.sin(2 * np.pi * u2), z], axis=1)   # roughly
    out["inside"].append(_finish(flat, np.zeros(n), p, _towards(rng, p, aim, 0.8, away=rng.random(n) < 0.2), u1, u2))
    # normals: facing away, and at grazing incidence (cos_r = +-1e-3, +-1e-2 about the float64 direction of the very sample)
    flat = _scene(pkg, [("tri", (-0.5, 1.49, -1.3), (0.5, 1.49, -1.3), (-0.5, 1.49, -0.3), glm.identity(), le),
                        ("sphere", (0, 0, 0), 0.25, glm.translate((0.9, 1.5, -1.2)), le)])
    recs = D.light_table(flat)[0]
    n = 2000
    p, lamp, u1, u2 = cloud(n, (-1, -1, -1), (1, 0.5, 1)), rng.integers(0, 2, n), rng.random(n), rng.random(n)
    w = sample64(flat, recs, lamp, p, np.tile([0.0, 1.0, 0.0], (n, 1)), u1, u2)["w"]
    side = _unit(np.cross(w, rng.normal(size=(n, 3))))
    c = rng.choice([1e-3, -1e-3, 1e-2, -1e-2, -0.5, -1.0], n)
    out["normals"].append(_finish(flat, lamp, p, c[:, None] * w + np.sqrt(1 - c * c)[:, None] * side, u1, u2))
    # lamps 1e20 away: d2 overflows, the sample is culled with a zero direction (a near lamp shares the table)
    far = 1e20
    flat = _scene(pkg, [("tri", (far, far, 0), (far + 1e18, far, 0), (far, far, 1e18), glm.identity(), le),
                        ("sphere", (0, 0, 0), 1.0, glm.translate((0.0, far, 0.0)), le),
                        ("tri", (0, 1.5, 0), (1, 1.5, 0), (0, 1.5, 1), glm.identity(), le)])
    n = 1500
    p = cloud(n, (-1, -1, -1), (1, 0.5, 1))
    lamp = rng.integers(0, 3, n)
    out["distant"].append(_finish(flat, lamp, p, np.tile([0.0, 1.0, 0.0], (n, 1)), rng.random(n), rng.random(n)))
    # edge draws: u1, u2 in {0, 1.0f, the largest value below 1} on a triangle and on a sphere lamp
    flat = _scene(pkg, [("tri", (-0.5, 1.5, -1.25), (0.5, 1.5, -1.25), (-0.5, 1.5, -0.25), glm.identity(), le),
                        ("sphere", (0.1, 0.2, -0.1), 0.5, glm.compose([glm.rotate(0.6, (1, 1, 0)), glm.scale(0.5), glm.translate((0.9, 1.2, -1.2))]), le)])
    edge = np.array([0.0, 1.0, BELOW_ONE])
    n = 150
    for a in edge:
        for b in edge:
            p, lamp = cloud(n, (-1, -1, -1), (1, 0.5, 1)), rng.integers(0, 2, n)
            target = np.where(lamp[:, None] == 0, [0.0, 1.5, -0.9], [0.95, 1.3, -1.25])
            out["edge_draws"].append(_finish(flat, lamp, p, _towards(rng, p, target, 0.3, away=rng.random(n) < 0.1), np.full(n, a), np.full(n, b)))
    return out
