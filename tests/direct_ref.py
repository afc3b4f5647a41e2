"""The checker of the direct-light queries (ptc_light_table, ptc_direct_light) -- TEST INFRASTRUCTURE, in the
manner of lit_ref.py.  Three things, none of them the thing under test:

  (a) light_table: the lamp table in numpy -- the records in binary32 with the operations of the library's instance triangles
      (transform_point, edge differences, normalize(cross)), weights / running sum / cdf in binary64 from the records' fields; and
      thresholds / select: the integer thresholds a sample picks its lamp by, from the raw first draw;
  (b) light_sample / sample / query: one light sample per point in numpy binary32, one numpy operation per source operation of
      light_sample_point in the order DESIGN section 5f writes down (numpy does not contract into FMA); its pinned pieces are the
      oracle's orc_path_seed, orc_rng_seed / orc_rng_uniform (the draws: light_draws), orc_sincos and intersect_rays (the
      shadow rays).  light_sample takes its draws from the caller: the query (sample) and the render loop (loop_ref.render_megakernel,
      section 5g) key their light streams differently and share everything else;
  (c) estimate_f64 and the truths: a float64 Monte-Carlo estimator written from the formula
          Le cos_r cos_l / (pi d^2 pdf_area) * visibility
      with numpy's own generator and analytic visibility, a closed form (sphere lamp) and a midpoint quadrature (panel lamp).
      Nothing in (c) calls (b).

Also the scenes and seeded points the CPU and GPU tests share."""
import numpy as np

from ref_f32 import PI, PI2, Draws, F, _cross, _dot, _normalize, _sincos, _xform_point, stream_states

SEED_XOR = 0x4C495445                            # kLightSeedXor (pt_device.hpp)
T_MIN = F(1e-4)
LIGHT_DTYPE = np.dtype([("p0", "<f4", (3,)), ("e1", "<f4", (3,)), ("e2", "<f4", (3,)), ("n", "<f4", (3,)), ("cdf", "<f4"),
                        ("inv_pdf", "<f4"), ("object", "<u4"), ("kind_material", "<u4")])
EMISSIVE = 3


# ---- (a) the table -------------------------------------------------------------------------------------------------------
def _mesh_of(flat, obj):
    positions = np.asarray(flat.positions, dtype=np.float32).reshape(-1, 3)
    indices = np.asarray(flat.indices, dtype=np.uint32).reshape(-1)
    if flat.mesh_ranges is not None:
        r = np.asarray(flat.mesh_ranges, dtype=np.uint32).reshape(-1, 6)[int(obj["index"])]
        positions = positions[r[0]:r[0] + r[1]]
        indices = indices[r[2]:r[2] + r[3]]
    return positions, indices.reshape(-1, 3)


def light_table(flat):
    """-> (records [LIGHT_DTYPE], info dict as PathTracer.light_info, weights float64, last record with a weight > 0)."""
    recs, weights, lums = [], [], []
    info = {"lights": 0, "sphere_lights": 0, "triangle_lights": 0, "emissive_objects": 0, "total_area": 0.0, "total_weight": 0.0}
    areas = []
    for i, obj in enumerate(flat.objects):
        mi = int(flat.object_material_indices[i])
        mat = flat.materials[mi]
        if mat["type"] != EMISSIVE:
            continue
        info["emissive_objects"] += 1
        lum = float(max(mat["p"][0], mat["p"][1], mat["p"][2]))
        m16 = np.asarray(obj["m"], dtype=np.float32)
        if obj["type"] == 0:
            sp = np.asarray(flat.spheres, dtype=np.float32).reshape(-1, 4)[int(obj["index"])]
            r = np.zeros(1, dtype=LIGHT_DTYPE)
            r["p0"][0] = _xform_point(m16, sp[:3])
            col = m16[0:3]
            r["e1"][0, 0] = np.sqrt((col[0] * col[0] + col[1] * col[1]) + col[2] * col[2]) * sp[3]
            r["kind_material"] = mi | (1 << 31)
            area = np.array([4.0 * 3.14159265358979323846 * float(r["e1"][0, 0]) * float(r["e1"][0, 0])])
            info["sphere_lights"] += 1
        else:
            positions, tri = _mesh_of(flat, obj)
            p = [_xform_point(m16, positions[tri[:, k]]) for k in range(3)]
            r = np.zeros(len(tri), dtype=LIGHT_DTYPE)
            r["p0"], r["e1"], r["e2"] = p[0], p[1] - p[0], p[2] - p[0]
            r["n"] = _normalize(_cross(r["e1"], r["e2"]))
            r["kind_material"] = mi
            e1, e2 = r["e1"].astype(np.float64), r["e2"].astype(np.float64)
            cx = e1[:, 1] * e2[:, 2] - e2[:, 1] * e1[:, 2]
            cy = e1[:, 2] * e2[:, 0] - e2[:, 2] * e1[:, 0]
            cz = e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]
            area = 0.5 * np.sqrt(cx * cx + cy * cy + cz * cz)
            info["triangle_lights"] += len(tri)
        r["object"] = i
        recs.append(r)
        areas.append(area)
        weights.append(area * lum)
        lums.append(np.full(len(r), lum))
    if not recs:
        return np.zeros(0, dtype=LIGHT_DTYPE), info, np.zeros(0), 0
    recs, areas, weights, lums = np.concatenate(recs), np.concatenate(areas), np.concatenate(weights), np.concatenate(lums)
    total, total_area = 0.0, 0.0
    for w, a in zip(weights, areas):   # sequential, in table order
        total += float(w)
        total_area += float(a)
    live = np.nonzero(weights > 0.0)[0]
    last = int(live[-1]) if len(live) else 0
    if total > 0.0:
        run = 0.0
        for k in range(len(recs)):
            run += float(weights[k])
            recs["cdf"][k] = F(1.0) if k >= last else F(run / total)
            recs["inv_pdf"][k] = F(0.0) if lums[k] == 0.0 else F(total / lums[k])
    info.update(lights=len(recs), total_area=total_area, total_weight=total)
    return recs, info, weights, last


STATES = 2 ** 31 - 2                             # N: the values n = v - 1 of a raw draw v (minstd_rand: 1 .. 2^31 - 2)
M31 = 2 ** 31 - 1


def thresholds(weights):
    """T_k of include/ptcore.h, in closed form where build_light_table runs a loop: the live records' ideal thresholds
    R_j = floor(run / W * N + 0.5) (j = 0 .. L - 1 in table order; run, W: the sequential binary64 sums), raised
    T_j = j + max_{i <= j}(R_i - i) (each at least its predecessor + 1), capped at N - (L - 1 - j) (the live records behind keep a
    state each), the last live one N; a record of weight 0 repeats its predecessor (0 in front of the first live one), everything
    behind the last live one gets N.  -> uint32[len(weights)]; zeros for a table of weight 0."""
    w = np.asarray(weights, dtype=np.float64)
    out = np.zeros(len(w), dtype=np.uint32)
    live = np.nonzero(w > 0.0)[0]
    if len(live) == 0:
        return out
    run = np.cumsum(w)                 # add.accumulate: sequential, as the library's loop
    j = np.arange(len(live), dtype=np.int64)
    ideal = np.floor(run[live] / run[-1] * float(STATES) + 0.5).astype(np.int64)
    t = np.minimum(j + np.maximum.accumulate(ideal - j), STATES - (len(live) - 1 - j))
    t[-1] = STATES
    owner = np.searchsorted(live, np.arange(len(w)), side="right") - 1   # the live record at or in front of k; -1: none yet
    out[owner >= 0] = t[owner[owner >= 0]]
    return out


def select(weights, last, v):
    """k = min(#{j : T_j <= v - 1}, last) for raw draws v."""
    n = np.asarray(v, dtype=np.int64) - 1
    return np.minimum(np.searchsorted(thresholds(weights), n, side="right"), last)


def light_draws(orc, indices, iteration, discard):
    """The three draws of a sample: per index a generator seeded path_seed(index, iteration) ^ SEED_XOR, discard(discard); the raw value
    v = next(), then u1, u2 = uniform() -> (v uint32[n], u float32[n, 2]).  (The query: discard 0; the render loop: 3 * bounce.)"""
    states = stream_states(orc, indices, iteration, SEED_XOR, discard)
    v = ((states.astype(np.uint64) * np.uint64(48271)) % np.uint64(M31)).astype(np.uint32)   # minstd_rand's step
    draws = Draws(orc, v)
    every = np.arange(len(v))
    return v, np.stack([draws.uniform(every) for _ in range(2)], axis=-1).reshape(-1, 2)


# ---- (b) the sample, binary32 ---------------------------------------------------------------------------------------------
def light_sample(orc, flat, table, p, nrm, draws):
    """light_sample_draws for points p [n, 3] with normals nrm and draws = (v uint32[n] raw, u [n, 2]: u1,
    u2), as light_draws returns them (item 1: whose they are is the caller's business): -> dict(rays [n, 8] as ptc_direct_light returns them, contribution [n, 3] (unshadowed), sampled
    bool[n], lamp int[n]).  table = light_table(flat), total weight > 0."""
    recs, _, weights, last = table
    n = len(p)
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0:3], rays[:, 3] = p, T_MIN
    contribution = np.zeros((n, 3), dtype=np.float32)
    if n == 0:
        return {"rays": rays, "contribution": contribution, "sampled": np.zeros(0, dtype=bool), "lamp": np.zeros(0, dtype=np.int64)}
    raw, u = draws
    u1, u2 = u[:, 0], u[:, 1]
    k = select(weights, last, raw)
    r = recs[k]
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
        rr = np.sqrt(np.where(F(0.0) < x, x, F(0.0)))   # sel_max(0, x)
        phi = PI2 * u2[sph]
        s, c = _sincos(orc, phi)
        d = np.stack([rr * c, rr * s, z], axis=-1)
        spheres = np.asarray(flat.spheres, dtype=np.float32).reshape(-1, 4)
        for j, lane in enumerate(sph):   # (a handful of distinct sphere lamps: the matrix differs per object)
            obj = flat.objects[int(r["object"][lane])]
            sp = spheres[int(obj["index"])]
            qo = sp[:3] + d[j] * sp[3]
            q[lane] = _xform_point(obj["m"], qo)
        nl[sph] = _normalize(q[sph] - p0[sph])
    v = q - p
    d2 = _dot(v, v)
    valid = (d2 > F(0.0)) & (d2 < F(np.inf))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = np.sqrt(d2)
        inv_d = F(1.0) / d
        w = v * inv_d[:, None]
        cos_r = _dot(nrm, w)
        cos_l = np.abs(_dot(nl, w))
        inv_pdf = r["inv_pdf"]
        sampled = valid & (cos_r > F(0.0)) & (inv_pdf > F(0.0))
        g = ((cos_r * cos_l) * inv_pdf) / (PI * d2)
        le = np.asarray(flat.materials)["p"][(r["kind_material"] & 0x7FFFFFFF).astype(np.int64), :3].astype(np.float32)
        cb = le * g[:, None]
        tmax = d * F(0.999)
    contribution[sampled] = cb[sampled]
    rays[sampled, 4:7] = w[sampled]
    rays[sampled, 7] = tmax[sampled]
    return {"rays": rays, "contribution": contribution, "sampled": sampled, "lamp": k}


def sample(orc, flat, points, normals, sample_index, table=None):
    """k_light_sample: light_sample for every point, point i with the first three draws of the generator of index i.  A scene
    without a lamp of weight > 0 samples nothing."""
    table = table if table is not None else light_table(flat)
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    n = len(p)
    if len(table[0]) == 0 or not float(np.sum(table[2])) > 0.0:
        rays = np.zeros((n, 8), dtype=np.float32)
        rays[:, 0:3], rays[:, 3] = p, T_MIN
        return {"rays": rays, "contribution": np.zeros((n, 3), dtype=np.float32), "sampled": np.zeros(n, dtype=bool),
                "lamp": np.zeros(n, dtype=np.int64)}
    return light_sample(orc, flat, table, p, nrm, light_draws(orc, range(n), sample_index, 0))


def query(orc, flat, points, normals, sample_index, table=None, scene_handle=None):
    """ptc_direct_light: -> (radiance [n, 3], rays [n, 8], visible uint8[n], sampled bool[n])."""
    s = sample(orc, flat, points, normals, sample_index, table)
    _, hit = orc.intersect_rays(flat, s["rays"], scene_handle=scene_handle)
    visible = s["sampled"] & (hit == 0)
    radiance = np.where(visible[:, None], s["contribution"], F(0.0)).astype(np.float32)
    return radiance, s["rays"], visible.astype(np.uint8), s["sampled"]


# ---- (c) float64: the estimator from the formula, and the truths ----------------------------------------------------------
def _blocked(p, q, blockers, t_hi):
    """Is the segment p + t (q - p) / |q - p|, t in [1e-4, t_hi], cut by one of the spheres (centre, radius)?  Analytic."""
    v = q - p
    d = np.linalg.norm(v, axis=-1)
    w = v / d[..., None]
    out = np.zeros(d.shape, dtype=bool)
    for c, r in blockers:
        oc = p - np.asarray(c, dtype=np.float64)
        b = np.sum(oc * w, axis=-1)
        cc = np.sum(oc * oc, axis=-1) - r * r
        disc = b * b - cc
        ok = disc >= 0.0
        sq = np.sqrt(np.where(ok, disc, 0.0))
        for t in (-b - sq, -b + sq):
            out |= ok & (t >= 1e-4) & (t <= t_hi)
    return out


def estimate_f64(case, samples, seed):
    """`samples` independent one-sample estimates (rgb, float64) of the radiance leaving a white Lambertian surface at case.p."""
    rng = np.random.default_rng(seed)
    p, n = np.asarray(case["p"], dtype=np.float64), np.asarray(case["n"], dtype=np.float64)
    le = np.asarray(case["le"], dtype=np.float64)
    u1, u2 = rng.random(samples), rng.random(samples)
    blockers = list(case["blockers"])
    if case["lamp"] == "sphere":
        c, r = np.asarray(case["centre"], dtype=np.float64), float(case["radius"])
        z = 1.0 - 2.0 * u1
        s = np.sqrt(np.maximum(0.0, 1.0 - z * z))
        nl = np.stack([s * np.cos(2.0 * np.pi * u2), s * np.sin(2.0 * np.pi * u2), z], axis=-1)
        q = c + r * nl
        area = 4.0 * np.pi * r * r
        blockers.append((c, r))   # the lamp hides its own far side: the shadow ray decides
    else:
        x0, x1, z0, z1, y = case["quad"]
        q = np.stack([x0 + (x1 - x0) * u1, np.full(samples, y), z0 + (z1 - z0) * u2], axis=-1)
        nl = np.broadcast_to(np.array([0.0, 1.0, 0.0]), q.shape)
        area = (x1 - x0) * (z1 - z0)
    v = q - p
    d = np.linalg.norm(v, axis=-1)
    w = v / d[:, None]
    cos_r = w @ n
    cos_l = np.abs(np.sum(nl * w, axis=-1))
    f = np.where(cos_r > 0.0, cos_r * cos_l * area / (np.pi * d * d), 0.0)
    f = np.where(_blocked(p, q, blockers, 0.999 * d), 0.0, f)
    return f[:, None] * le[None, :]


def truth(case, grid=1024):
    """rgb, float64.  Sphere lamp, fully above the horizon, nothing in between: Le (R / D)^2 cos(theta).  Panel: midpoint
    quadrature of Le cos_r cos_l / (pi d^2) over the quad on a grid x grid lattice, with the analytic blocker test."""
    p, n = np.asarray(case["p"], dtype=np.float64), np.asarray(case["n"], dtype=np.float64)
    le = np.asarray(case["le"], dtype=np.float64)
    if case["lamp"] == "sphere":
        assert not case["blockers"]
        v = np.asarray(case["centre"], dtype=np.float64) - p
        dist = np.linalg.norm(v)
        return le * (case["radius"] / dist) ** 2 * float(v @ n) / dist
    x0, x1, z0, z1, y = case["quad"]
    xs = x0 + (x1 - x0) * (np.arange(grid) + 0.5) / grid
    zs = z0 + (z1 - z0) * (np.arange(grid) + 0.5) / grid
    total = 0.0
    for zc in zs:   # row by row: keeps the temporaries small
        q = np.stack([xs, np.full(grid, y), np.full(grid, zc)], axis=-1)
        v = q - p
        d = np.linalg.norm(v, axis=-1)
        w = v / d[:, None]
        cos_r = w @ n
        f = np.where(cos_r > 0.0, cos_r * np.abs(w[:, 1]) / (np.pi * d * d), 0.0)
        if case["blockers"]:
            f = np.where(_blocked(p, q, case["blockers"], 0.999 * d), 0.0, f)
        total += float(np.sum(f))
    return le * total * (x1 - x0) * (z1 - z0) / (grid * grid)


SAMPLE_INDEX = 5          # of every statistical case, chosen once
SAMPLES = 16384
FLOOR_POINT = (0.2, -1.0, 0.1)
UP = (0.0, 1.0, 0.0)
PANEL = (-0.5, 0.5, -1.3, -0.3, 1.49)   # scenes.light_panel_mesh's quad


def truth_cases(pkg):
    """The four statistical cases: name -> (scene, case dict for (c)).  One floor point, nothing but the lamp (and a blocker)."""
    glm = pkg.glmlite

    def lamp_scene(kind, blocker):
        s = pkg.SceneDescription()
        s.add_material("lamp", pkg.EmissiveMaterial((4.0, 3.6, 3.0) if kind == "sphere" else (6.0, 6.0, 5.5)))
        s.add_material("grey", pkg.DiffuseMateral((0.5, 0.5, 0.5)))
        if blocker is not None:
            s.add_object(pkg.Sphere((0, 0, 0), blocker[1]), glm.translate(blocker[0]), "grey")
        if kind == "sphere":
            s.add_object(pkg.Sphere((0, 0, 0), 0.25), glm.translate((0.9, 1.5, -1.2)), "lamp")
        else:
            mesh = s.add_mesh("models/light_panel.obj", pkg.scenes.light_panel_mesh())
            s.add_object(mesh, glm.identity(), "lamp")
        return s

    base = {"p": FLOOR_POINT, "n": UP, "blockers": []}
    sphere = dict(base, lamp="sphere", centre=(0.9, 1.5, -1.2), radius=0.25, le=(4.0, 3.6, 3.0))
    panel = dict(base, lamp="panel", quad=PANEL, le=(6.0, 6.0, 5.5))
    penumbra = ((0.1, 0.3, -0.55), 0.3)
    umbra = ((0.1, 0.2, -0.3), 0.6)
    return {"sphere": (lamp_scene("sphere", None), sphere),
            "panel": (lamp_scene("panel", None), panel),
            "penumbra": (lamp_scene("panel", penumbra), dict(panel, blockers=[penumbra])),
            "umbra": (lamp_scene("panel", umbra), dict(panel, blockers=[umbra]))}


# ---- scenes and points of the table and bit tests -------------------------------------------------------------------------
def two_instance_scene(pkg):
    """cornell_spheres' room and balls with a unit panel at the origin as two instances under rotate o scale(0.5, 2, 1) o translate,
    each with an emissive material of its own (mesh lamps take any matrix: their records are world-space triangles)."""
    glm = pkg.glmlite
    s = pkg.scenes.cornell_spheres((64, 64))
    s.add_material("panel_a", pkg.EmissiveMaterial((5.0, 4.0, 3.0)))
    s.add_material("panel_b", pkg.EmissiveMaterial((1.0, 2.0, 7.0)))
    mesh = s.add_mesh("models/unit_panel.obj", pkg.scenes.light_panel_mesh(-0.5, 0.5, -0.5, 0.5, 0.0))
    s.add_object(mesh, glm.compose([glm.rotate(0.5, (0, 0, 1)), glm.scale((0.5, 2.0, 1.0)), glm.translate((-0.8, 0.9, -0.9))]), "panel_a")
    s.add_object(mesh, glm.compose([glm.rotate(-0.7, (1, 0, 0)), glm.scale((0.5, 2.0, 1.0)), glm.translate((0.9, 0.8, -0.6))]), "panel_b")
    return s


def dark_lamp_scene(pkg):
    """cornell_lit(with_mesh=True) plus two sphere lamps whose emission is 0: in the middle of the object list and at its end."""
    s = pkg.scenes.cornell_lit((64, 64), with_mesh=True)
    s.add_material("dark", pkg.EmissiveMaterial((0.0, 0.0, 0.0)))
    s.objects_.insert(3, (pkg.Sphere((0, 0, 0), 0.2), np.asarray(pkg.glmlite.translate((-1.0, 1.0, -1.0)), dtype=np.float32).reshape(4, 4)))
    s.objects_material_mapping_.insert(3, "dark")
    s.add_object(pkg.Sphere((0, 0, 0), 0.1), pkg.glmlite.translate((1.0, 1.0, 1.0)), "dark")   # and one that ends the table
    return s


def degenerate_scene(pkg):
    """A lamp mesh with a triangle of area 0 in the middle (three collinear vertices) and one with two equal vertices at the end."""
    s = pkg.SceneDescription()
    s.add_material("lamp", pkg.EmissiveMaterial((2.0, 3.0, 1.0)))
    positions = np.array([[-0.5, 1.4, -0.5], [0.5, 1.4, -0.5], [0.5, 1.4, 0.5], [-0.5, 1.4, 0.5], [0.0, 1.4, 0.0], [0.7, 1.2, 0.1]],
                         dtype=np.float32)
    indices = np.array([0, 2, 1, 0, 4, 2, 0, 3, 2, 3, 3, 5], dtype=np.uint32)
    mesh = s.add_mesh("models/lamp.obj", pkg.Mesh(positions, indices))
    s.add_object(mesh, pkg.glmlite.translate((0.1, 0.0, -0.2)), "lamp")
    return s


def sphere_lamp_scene(pkg, transform=None):
    """A sphere lamp whose centre sits in the Sphere struct, under rotation x uniform scale (or `transform`), and a floor."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.add_material("floor", pkg.DiffuseMateral((0.7, 0.7, 0.7)))
    s.add_material("lamp", pkg.EmissiveMaterial((3.0, 2.0, 4.0)))
    s.add_object(pkg.Sphere((0, 0, 0), 1000.0), glm.translate((0.0, -1001.0, 0.0)), "floor")
    if transform is None:
        transform = glm.compose([glm.rotate(0.6, (1, 1, 0)), glm.scale(0.5), glm.translate((0.9, 1.2, -1.2))])
    s.add_object(pkg.Sphere((0.1, 0.2, -0.1), 0.5), transform, "lamp")
    return s


def big_emitter_scene(pkg):
    """The heightfield mesh at nx = 129, nz = 65 (16,384 triangles) as a lamp above a floor: the search runs 14 steps."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.add_material("floor", pkg.DiffuseMateral((0.7, 0.7, 0.7)))
    s.add_material("glow", pkg.EmissiveMaterial((0.5, 0.6, 0.7)))
    s.add_object(pkg.Sphere((0, 0, 0), 1000.0), glm.translate((0.0, -1001.0, 0.0)), "floor")
    mesh = s.add_mesh("models/heightfield.obj", pkg.scenes.heightfield_mesh(129, 65, 3.0, 1.5, seed=7))
    s.add_object(mesh, glm.translate((0.0, 1.2, -0.5)), "glow")
    return s


def room_points(n, seed, lamp_points=()):
    """n seeded points on the room of scenes.cornell_* (floor, back, left and right wall: the planes the wall spheres touch) and on
    its three balls, with their normals; every fifth normal flipped; lamp_points: (point, normal) pairs that replace the first."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 7, n)
    a, b = rng.uniform(-1.9, 1.9, n), rng.uniform(-1.9, 1.9, n)
    h = rng.uniform(-0.95, 1.4, n)
    p = np.zeros((n, 3))
    nr = np.zeros((n, 3))
    planes = [(np.stack([a, np.full(n, -1.0), b], axis=1), (0, 1, 0)), (np.stack([a, h, np.full(n, -2.0)], axis=1), (0, 0, 1)),
              (np.stack([np.full(n, -2.0), h, b], axis=1), (1, 0, 0)), (np.stack([np.full(n, 2.0), h, b], axis=1), (-1, 0, 0))]
    for k, (pts, normal) in enumerate(planes):
        m = kind == k
        p[m], nr[m] = pts[m], normal
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for k, c in enumerate([(0.0, -0.5, -0.6), (1.1, -0.5, 0.1), (-1.1, -0.5, 0.2)]):
        m = kind == 4 + k
        p[m], nr[m] = np.asarray(c) + 0.5 * v[m], v[m]
    nr[::5] = -nr[::5]
    for k, (pt, normal) in enumerate(lamp_points):
        p[k], nr[k] = pt, normal
    return p.astype(np.float32), nr.astype(np.float32)


def cornell_lamp_points():
    """A few points on the lamps of cornell_lit(with_mesh=True) themselves: on the panel, facing down (every sample of the panel
    grazes: cos_r is 0 or a rounding away from it) and on the sphere lamp, facing outwards."""
    out = [((x, 1.49, z), (0.0, -1.0, 0.0)) for x, z in ((0.0, -0.8), (-0.3, -1.1), (0.45, -0.35), (0.1, -0.5))]
    for v in ((0.0, -1.0, 0.0), (0.6, -0.8, 0.0), (0.0, 0.0, 1.0), (-1.0, 0.0, 0.0)):
        out.append((tuple(np.array([0.9, 1.5, -1.2]) + 0.25 * np.array(v)), v))
    return out
