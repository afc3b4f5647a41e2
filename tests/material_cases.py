"""Scenes that carry the material code (evaluate_material / shade_kinds) over its parameter range and to its edges, and the
censuses that say the scenes reach what they were built for.  Deterministic builders, no files read.

  wall(pkg, ...)        a grid of 60 small objects, each with its own material record: every diffuse / metal albedo of ALBEDOS,
                        every metal fuzz of FUZZ (with every albedo), every refraction index of INDICES; half spheres (the
                        centre in the transform, in the Sphere, or a sphere scaled down or up), half instances of one small mesh;
                        object order shuffled by a fixed seed; a large diffuse ground sphere; open sky.  Variants: with two
                        emitters (a sphere and a mesh instance), mesh-only (runs of instances of one mesh), and
                        mesh-first (the persistent launch's shape: one mesh object, then a sphere run).
  three_balls(pkg)      the objects and materials of the reference's three_balls.json (metal fuzz 1.0), built by hand.
  critical_frames(pkg)  frames about 2e-6 rad wide whose primary rays meet glass within ulps of the critical angle (where
                        `cannot_refract` and refract's `k` disagree and the refracted direction is the zero vector), at
                        grazing and at normal incidence.
  probe_frames(pkg)     one convex object under open sky, for the float64 reference of tests/material_f64.py.

The censuses restate the bounce-0 decisions in numpy binary32 from lit_ref's pieces."""
import math

import numpy as np

F = np.float32
ALBEDOS = [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.8, 0.8, 0.8), (4.0, 0.5, 0.0), (1e-12, 1e-12, 1e-12), (1e12, 1e12, 1e12)]
FUZZ = [0.0, 1e-7, 0.5, 1.0, float(np.nextafter(F(1.0), F(2.0))), 1.5, 4.0]
INDICES = [1.0, float(np.nextafter(F(1.0), F(0.0))), float(np.nextafter(F(1.0), F(2.0))), 1.33, 1.5, 2.4, 10.0, 1e3, 0.9, 0.5,
           0.1, 1e-3]
WALL_W, WALL_H, WALL_ITERS = 192, 128, 2
COLS, ROWS = 10, 6


def wall_materials(pkg):
    """[(name, material)]: 6 diffuse, 42 metal (every fuzz with every albedo), 12 glass; the name's number is the
    material's index in the flat scene (names sort)."""
    mats = [pkg.DiffuseMateral(a) for a in ALBEDOS]
    mats += [pkg.MetalMaterial(a, f) for f in FUZZ for a in ALBEDOS]
    mats += [pkg.DielectricMaterial(i) for i in INDICES]
    return [(f"m{k:02d}", m) for k, m in enumerate(mats)]


def wall(pkg, emissive=False, mesh_only=False, mesh_first=False, size=(WALL_W, WALL_H)):
    """mesh_first: the one shape of a scene that the persistent launch ("persist" 1) takes -- ONE mesh object that opens the
    list (here the ground, a small heightfield) and a sphere run that ends it (here all 60 materials, on spheres)."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.resolution = tuple(size)
    mats = wall_materials(pkg)
    assert len(mats) == COLS * ROWS
    for name, m in mats:
        s.add_material(name, m)
    s.add_material("zz_ground", pkg.DiffuseMateral((0.5, 0.5, 0.5)))
    mesh = s.add_mesh("blob", pkg.scenes.displaced_sphere_mesh(8, 16))
    rng = np.random.default_rng(20261)
    order = rng.permutation(len(mats))          # the object list's order: sphere runs in front of, between, behind mesh runs
    cell = rng.permutation(len(mats))           # where each object stands in the grid
    # which shape carries which material: drawn, so that no parameter list is tied to one shape.  A scaled sphere's normal
    # is not of unit length (the reference transforms it and does not normalise): scaled down it is long and a metal's
    # reflection is pushed off the surface, scaled up it is short and the reflection hugs the surface
    shapes = rng.permutation(["mesh"] * 30 + ["moved"] * 8 + ["centre"] * 8 + ["shrunk"] * 7 + ["grown"] * 7)
    r = 0.38
    if mesh_first:
        field = s.add_mesh("field", pkg.scenes.heightfield_mesh(17, 9, 40.0, 30.0))
        s.add_object(field, glm.translate((0.0, -0.7, 0.0)), "zz_ground")
        shapes = np.where(shapes == "mesh", "moved", shapes)
    for k in order:
        k = int(k)
        x, y = float(cell[k] % COLS) - 0.5 * (COLS - 1), float(cell[k] // COLS)
        name, shape = mats[k][0], shapes[k]
        if mesh_only or shape == "mesh":
            turn = glm.rotate(np.float32(0.37 * k), (0.3, 1.0, 0.2 + 0.1 * (k % 5)))
            s.add_object(mesh, glm.compose([turn, glm.scale(2.0 * r), glm.translate((x, y, 0.0))]), name)
        elif shape == "moved":
            s.add_object(pkg.Sphere((0.0, 0.0, 0.0), r), glm.translate((x, y, 0.0)), name)
        elif shape == "centre":
            s.add_object(pkg.Sphere((x, y, 0.0), r), glm.translate((0.0, 0.0, 0.0)), name)   # centre kept in the Sphere
        elif shape == "shrunk":
            s.add_object(pkg.Sphere((0.0, 0.0, 0.0), 1.0), glm.compose([glm.scale(r), glm.translate((x, y, 0.0))]), name)
        else:
            s.add_object(pkg.Sphere((0.0, 0.0, 0.0), 0.5 * r), glm.compose([glm.scale(2.0), glm.translate((x, y, 0.0))]), name)
    if emissive:
        s.add_material("zz_lamp_a", pkg.EmissiveMaterial((6.0, 5.0, 4.0)))
        s.add_material("zz_lamp_b", pkg.EmissiveMaterial((0.5, 2.0, 8.0)))
        s.add_object(pkg.Sphere((0.0, 0.0, 0.0), 0.2), glm.translate((-1.0, 2.5, 2.5)), "zz_lamp_a")
        s.add_object(mesh, glm.compose([glm.scale(0.4), glm.translate((2.0, 1.5, 2.5))]), "zz_lamp_b")
    if not mesh_first:
        s.add_object(pkg.Sphere((0.0, 0.0, 0.0), 1000.0), glm.translate((0.0, -1000.5, 0.0)), "zz_ground")
    s.camera = pkg.scenes._camera_from_look_at((0.0, 2.5, 9.0), (0.0, 2.5, 0.0), vfov_deg=40.0)
    return s


def wall_out_of_range(pkg):
    """(scene, flat): the wall with two records the reference would take and turn into NaN at once -- refraction index 0
    (ratio 1 / 0: total reflection, or a refraction whose k is not a number: the zero vector) and a NaN albedo.  Outside
    what bit parity is pinned for; what is pinned is NaN in the same pixels and equal values everywhere else."""
    s = wall(pkg)
    flat = s.build_scene()
    glass = 6 + len(FUZZ) * len(ALBEDOS)
    assert flat.materials["type"][glass] == 2 and flat.materials["type"][2] == 0
    flat.materials["p"][glass, 0] = 0.0
    flat.materials["p"][2, :3] = np.nan
    return s, flat


def three_balls(pkg, size=(96, 54)):
    """three_balls.json's four spheres and four materials (the file itself does not parse, in the reference either)."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.resolution = tuple(size)
    s.add_material("ground", pkg.DiffuseMateral((0.8, 0.8, 0.0)))
    s.add_material("blue", pkg.DiffuseMateral((0.1, 0.2, 0.5)))
    s.add_material("dielectric", pkg.DielectricMaterial(1.5))
    s.add_material("metal", pkg.MetalMaterial((0.8, 0.6, 0.2), 1.0))
    s.add_object(pkg.Sphere((0, 0, 0), 100.0), glm.translate((0.0, -100.5, -1.0)), "ground")
    s.add_object(pkg.Sphere((0, 0, 0), 0.5), glm.translate((0.0, 0.0, -1.0)), "blue")
    s.add_object(pkg.Sphere((0, 0, 0), 0.5), glm.translate((-1.0, 0.0, -1.0)), "dielectric")
    s.add_object(pkg.Sphere((0, 0, 0), 0.5), glm.translate((1.0, 0.0, -1.0)), "metal")
    s.camera = pkg.Camera(position=(0.0, 0.0, 4.0), rotation=(1.0, 0.0, 0.0, 0.0), vfov=float(np.float32(math.radians(45.0))))
    return s


def walls(pkg):
    """name -> scene.  Every wall renders at scene.resolution with WALL_ITERS iterations."""
    return {"wall": wall(pkg), "wall_lit": wall(pkg, emissive=True), "wall_meshes": wall(pkg, mesh_only=True),
            "wall_mesh_first": wall(pkg, mesh_first=True), "three_balls": three_balls(pkg)}


# ---------------------------------------------------------------------------------------------------------------------------
# rigid placement: everything below is built in a canonical frame and turned by one rotation, object and camera together
# ---------------------------------------------------------------------------------------------------------------------------
def _rotation(seed):
    """A fixed rotation matrix with no special axis (QR of a seeded Gaussian matrix), float64."""
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))[None, :]
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


AXIS_TURNS = {"y": np.eye(3), "x": np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]),
              "z": np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])}   # the named axis goes to the world's y


def _camera(pkg, R, frm, direction, up, vfov):
    frm, direction, up = (R @ np.asarray(v, dtype=np.float64) for v in (frm, direction, up))
    m = pkg.glmlite.look_at(frm, frm + direction, up)
    return pkg.Camera(position=tuple(float(v) for v in m[3, 0:3]),
                      rotation=tuple(float(v) for v in pkg.glmlite.quat_from_matrix(m)), vfov=float(np.float32(vfov)))


def _plate(pkg, R, half=4.0):
    """Two triangles over [-half, half]^2 of the canonical plane y = 0, counter-clockwise seen from +y."""
    v = np.array([[-half, 0.0, -half], [-half, 0.0, half], [half, 0.0, half], [half, 0.0, -half]], dtype=np.float64)
    return pkg.Mesh((v @ R.T).astype(np.float32), np.array([0, 1, 2, 0, 2, 3], dtype=np.uint32))


def _plate_scene(pkg, R, index, direction, up, vfov, size, distance=2.0):
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.resolution = tuple(size)
    s.add_material("glass", pkg.DielectricMaterial(index))
    s.add_object(s.add_mesh("plate", _plate(pkg, R)), glm.identity(), "glass")
    d = np.asarray(direction, dtype=np.float64)
    s.camera = _camera(pkg, R, -distance * d, d, up, vfov)
    return s


CRIT_W, CRIT_H, CRIT_ITERS, CRIT_MB = 24, 16, 4, 3
CRIT_VFOV = 2e-6
TURNS = (0.3, 1.7, 2.9, 4.1)   # the camera's rotations about the surface normal (rad); each also gets its own world rotation


def _incidence(theta, psi, from_above):
    st, ct = math.sin(theta), math.cos(theta)
    return np.array([st * math.cos(psi), -ct if from_above else ct, st * math.sin(psi)])


def critical_frames(pkg):
    """[(name, kind, index, scene)]; kind is 'critical' (both sides of `cannot_refract`), 'grazing' or 'normal'.  Each
    renders at CRIT_W x CRIT_H, CRIT_ITERS iterations, CRIT_MB bounces."""
    out = []
    size = (CRIT_W, CRIT_H)
    n = np.array([0.0, 1.0, 0.0])
    for index, from_above in ((1.5, False), (2.4, False), (10.0, False), (0.75, True), (0.9, True)):
        ratio = float(F(1.0) / F(index)) if from_above else float(F(index))
        theta = math.asin(1.0 / ratio)
        for t, psi in enumerate(TURNS):
            R = _rotation(100 * t + int(index * 10))
            # (at index 10 the critical angle is 5.7 degrees: sin_theta = sqrt(1 - cos^2) carries 3e-7 rad of rounding
            # there, three times the other indices', and the frame is twice as wide to hold both sides of it)
            vfov = 2.0 * CRIT_VFOV if index == 10.0 else CRIT_VFOV
            s = _plate_scene(pkg, R, index, _incidence(theta, psi, from_above), n, vfov, size)
            out.append((f"plate_{index}_{t}", "critical", index, s))
    glm = pkg.glmlite
    # from inside a glass sphere of index 1.5: the camera 0.8 R off the centre, its axis at the angle from the outward radius
    # whose chord meets the surface at the critical angle (sine rule: sin(incidence) = 0.8 sin(angle))
    alpha = math.asin(1.0 / (1.5 * 0.8))
    for room in (False, True):
        for t, psi in enumerate(TURNS):
            R = _rotation(977 + 10 * t + room)
            e = np.array([0.0, 1.0, 0.0])
            d = np.array([math.sin(alpha) * math.cos(psi), math.cos(alpha), math.sin(alpha) * math.sin(psi)])
            centre = np.array([0.3, -0.2, 0.5])
            s = pkg.SceneDescription()
            s.resolution = size
            s.add_material("glass", pkg.DielectricMaterial(1.5))
            if room:
                s.add_material("room", pkg.DiffuseMateral((0.7, 0.7, 0.7)))
                s.add_material("steel", pkg.MetalMaterial((0.8, 0.8, 0.9), 0.5))
                s.add_object(pkg.Sphere((0, 0, 0), 50.0), glm.translate((0.0, 0.0, 0.0)), "room")
            s.add_object(pkg.Sphere((0, 0, 0), 1.0), glm.translate(tuple(R @ centre)), "glass")
            if room:
                blob = s.add_mesh("blob", pkg.scenes.displaced_sphere_mesh(8, 16))
                s.add_object(blob, glm.translate(tuple(R @ (centre + np.array([0.5, 2.5, 0.5])))), "steel")
                s.add_object(blob, glm.compose([glm.scale(0.7), glm.translate(tuple(R @ (centre + np.array([-2.0, 1.0, 0.0]))))]),
                             "room")
                s.add_object(pkg.Sphere((0, 0, 0), 0.6), glm.translate(tuple(R @ (centre + np.array([2.0, 2.0, -1.0])))), "steel")
            s.camera = _camera(pkg, R, centre + 0.8 * e, d, e, CRIT_VFOV)
            out.append((f"inside_{'room' if room else 'alone'}_{t}", "critical", 1.5, s))
    for t, psi in enumerate(TURNS[:2]):
        # grazing: the camera 1e-6 above the plate's plane, two units from its middle, its axis in the plane
        R = _rotation(4000 + t)
        d = np.array([math.cos(psi), 0.0, math.sin(psi)])
        s = _plate_scene(pkg, R, 1.5, d, n, CRIT_VFOV, size)
        s.camera = _camera(pkg, R, -2.0 * d + 1e-6 * n, d, n, CRIT_VFOV)
        out.append((f"grazing_{t}", "grazing", 1.5, s))
        R = _rotation(5000 + t)
        s = _plate_scene(pkg, R, 1.5, -n, (math.cos(psi), 0.0, math.sin(psi)), CRIT_VFOV, size)
        out.append((f"normal_{t}", "normal", 1.5, s))
    return out


PROBE_W, PROBE_H = 32, 24


def probe_frames(pkg):
    """[(name, scene)]: one convex object under open sky, each under the three AXIS_TURNS.  The inside-sphere probes' names
    start with 'inside'."""
    glm = pkg.glmlite
    out = []
    size = (PROBE_W, PROBE_H)
    n = np.array([0.0, 1.0, 0.0])
    for axis, R in AXIS_TURNS.items():
        balls = [("diffuse", pkg.DiffuseMateral((0.7, 0.4, 0.9)))]
        balls += [(f"metal_{f}", pkg.MetalMaterial((0.9, 0.6, 0.3), f)) for f in (0.0, 0.3, 1.0)]
        for name, m in balls:
            s = pkg.SceneDescription()
            s.resolution = size
            s.add_material("ball", m)
            c = np.array([0.2, 0.1, -0.3])
            s.add_object(pkg.Sphere((0, 0, 0), 1.0), glm.translate(tuple(R @ c)), "ball")
            d = np.array([0.3, -0.4, -1.0])
            d /= np.linalg.norm(d)
            s.camera = _camera(pkg, R, c - 2.0 * d, d, n, math.radians(50.0))
            out.append((f"{name}_{axis}", s))
        for index in (1.5, 1.0, 0.75):
            for face, above in (("front", True), ("back", False)):
                d = _incidence(math.radians(48.0), 0.6, above)
                up = n if above else -n
                s = _plate_scene(pkg, R, index, d, up, math.radians(70.0), size, distance=1.5)
                out.append((f"plate_{face}_{index}_{axis}", s))
        s = pkg.SceneDescription()
        s.resolution = size
        s.add_material("glass", pkg.DielectricMaterial(1.5))
        c = np.array([-0.4, 0.3, 0.2])
        s.add_object(pkg.Sphere((0, 0, 0), 1.0), glm.translate(tuple(R @ c)), "glass")
        d = np.array([0.2, 1.0, 0.1])
        d /= np.linalg.norm(d)
        s.camera = _camera(pkg, R, c + 0.8 * d, d, (1.0, 0.0, 0.0), math.radians(100.0))
        out.append((f"inside_sphere_{axis}", s))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# censuses (numpy binary32, from lit_ref's pieces): what the frames' bounce-0 paths do
# ---------------------------------------------------------------------------------------------------------------------------
def _first_hits(orc, lr, flat, camera, w, h, iteration, sh):
    o, d, tmin, states = lr._primary(orc, camera, w, h, np.arange(w * h), iteration)
    recs, hit = orc.intersect_rays(flat, lr._rays(o, tmin, d), scene_handle=sh)
    lib = orc.lib()
    st = np.array([lib.orc_rng_seed(lib.orc_path_seed(p, iteration)) for p in range(w * h)], dtype=np.uint32)
    return o, d, tmin, st, recs, hit.astype(bool)


def glass_census(orc, lr, flat, camera, w, h, iters):
    """Counts over the bounce-0 paths that hit glass: `cannot_refract` true / false-and-reflected / false-and-refracted,
    refracted with k < 0 (the zero vector) and with k == 0, the clamp of cos_theta active, back-face hits."""
    sh = orc.SceneHandle(flat)
    mats = np.asarray(flat.materials)
    c = dict(paths=0, glass=0, cannot=0, reflected=0, refracted=0, zero_vector=0, k_zero=0, clamped=0, back=0)
    for it in range(iters):
        o, d, tmin, st, recs, hit = _first_hits(orc, lr, flat, camera, w, h, it, sh)
        c["paths"] += w * h
        g = np.nonzero(hit & (mats["type"][recs["material_id"].astype(np.int64) % len(mats)] == 2))[0]
        if not len(g):
            continue
        n = recs["normal"][g].astype(np.float32)
        ior = mats["p"][recs["material_id"][g].astype(np.int64), 0].astype(np.float32)
        side = recs["side"][g]
        ratio = np.where(side == 0, F(1.0) / ior, ior)
        unit = lr._normalize(d[g])
        x = lr._dot(-unit, n)
        cos_t = np.where(F(1.0) < x, F(1.0), x)
        sin_t = np.sqrt(F(1.0) - cos_t * cos_t)
        cannot = ratio * sin_t > F(1.0)
        u = lr.Draws(orc, st).uniform(g)
        r0 = (F(1.0) - ratio) / (F(1.0) + ratio)
        r0 = r0 * r0
        xx = F(1.0) - cos_t
        x4 = (xx * xx) * (xx * xx)
        refl = (r0 + (F(1.0) - r0) * (x4 * xx)) > u
        dv = lr._dot(n, unit)
        k = F(1.0) - ratio * ratio * (F(1.0) - dv * dv)
        refr = ~cannot & ~refl
        c["glass"] += len(g)
        c["cannot"] += int(cannot.sum())
        c["reflected"] += int((~cannot & refl).sum())
        c["refracted"] += int(refr.sum())
        c["zero_vector"] += int((refr & (k < 0)).sum())
        c["k_zero"] += int((refr & (k == 0)).sum())
        c["clamped"] += int((F(1.0) < x).sum())
        c["back"] += int((side != 0).sum())
    return c


def wall_census(orc, lr, flat, camera, w, h, iters):
    """Per iteration: bounce-0 hits per material, the fuzz >= 1 metal hits and how many of their directions are rejected
    (dot(dir, n) <= 0), and the paths whose second ray hits the object they left (same material record) at t < 1e-3."""
    sh = orc.SceneHandle(flat)
    mats = np.asarray(flat.materials)
    out = []
    for it in range(iters):
        o, d, tmin, st, recs, hit = _first_hits(orc, lr, flat, camera, w, h, it, sh)
        mid = recs["material_id"].astype(np.int64)
        typ = np.where(hit, mats["type"][mid % len(mats)], -1)
        sc = np.nonzero(hit & (typ != lr.EMISSIVE))[0]
        per_material = np.bincount(mid[hit], minlength=len(mats))
        n0 = recs["normal"].astype(np.float32)
        color = np.ones((w * h, 3), dtype=np.float32)
        lr.shade(orc, mats, o, d, tmin, recs, sc, lr.Draws(orc, st), color)
        wide = np.zeros(w * h, dtype=bool)
        wide[sc] = (typ[sc] == 1) & (mats["p"][mid[sc], 3] >= 1.0)
        rejected = wide & ~(lr._dot(d, n0) > F(0.0))
        recs1, hit1 = orc.intersect_rays(flat, lr._rays(o[sc], tmin[sc], d[sc]), scene_handle=sh)
        again = hit1.astype(bool) & (recs1["material_id"].astype(np.int64) == mid[sc]) & (recs1["t"] < 1e-3)
        out.append(dict(per_material=per_material, wide=int(wide.sum()), rejected=int(rejected.sum()),
                        rehit=int(again.sum()), rehit_types=np.bincount(typ[sc][again], minlength=3)))
    return out


def mismatches(got, want):
    """How many values of a frame differ from the checker's.  x86 and gfx950 give NaN different sign bits, so where the
    checker has NaN the frame must have NaN (any), and everywhere else the values must be equal; a checker's frame
    without NaN is compared as a whole."""
    got, want = np.asarray(got), np.asarray(want).reshape(np.shape(got))
    nan = np.isnan(want)
    if not nan.any():
        return int(np.sum(got != want))
    return int(np.sum(np.isnan(got) != nan) + np.sum((got != want) & ~nan))
