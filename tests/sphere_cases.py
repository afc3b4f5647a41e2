"""Constructed sphere objects and ray families for the sphere code's limits (tests/test_sphere_cases_cpu.py proves on the host
that every family sits where it claims to, tests/test_gpu_sphere_limits.py runs them on every road a sphere can take).

A RUN is a list of sphere objects that stand together in the object list: as the whole list, in front of a small heightfield
(a leading run) or behind it (a trailing run).  A FAMILY is N = 4096 rays (64 wavefronts) built for one bound of the sphere code:

  graze      impact parameter r (1 +- 2^-k), k = 6 .. 24, and exactly r, seen from 1.5 r, 10 r and (big spheres) r + 1 away:
             across the relative margins 1e-4, 1e-5 and 2e-6 of the approximate bounds and down to the float grid
  tmin       the accepted root at t_min (1 +- 2^-k), k = 1 .. 23, for t_min 1e-4 and 1e-5, the near root from outside and the
             far root from inside
  tmax       the closest hit carried in at root (1 +- 2^-k), k = 10 .. 23, and at exactly the t the reference records for the
             object before (a tie: the later object wins, intersections.cuh:30)
  box        ellipsoids: lines that pass an edge of the object's stored world box at 2^-k of its size inside and outside, and
             rays at the part of the ellipsoid that the reference's box (the x axis' stretch alone, scene_description.cpp:29-36)
             leaves outside
  units      the object-space t_min / t_max of a scaled sphere (transform.hpp:51-58): under 1e3 a surface closer than 0.1 is
             below t_min in object units, under 1e-3 a carried closest hit lies between the world and the object-space root
  direction  lengths 1e-3, 0.5, 2 and 1e3, direction components and origin coordinates +0 and -0
  degenerate rays through a sphere of negative radius, of radius 0, with a stored box clipped to half and with a box that is empty on
             one axis, each in front of a wall
  planes     from inside a sphere whose centre is kept in the Sphere, the origin on a coordinate plane of that centre and a
             direction component of +-1e-30 across it: the hit point's coordinate IS the centre's, the outward normal's component
             +0, the back face's -0 -- and transform_normal's sums of products with zeros give it the sign the other components
             leave it (the one case sphere_fold hands back after the fact: its `odd`)
  aimed      random rays at the heap (the oracle's bits only)
  general    the same where binary32 and float64 can be compared (tests/closest_hit_f64.py)

Everything is float64 numpy rounded to binary32 once; the per-object answers come from the oracle on a one-object scene."""
import ctypes as C

import numpy as np

N = 4096
FLT_MAX = np.finfo(np.float32).max
MATERIALS = 10   # material k belongs to object k of the run, the last one to the heightfield

FAMILIES = {
    "radii": ("graze", "tmin", "tmax", "direction", "general"),
    "far": ("graze", "tmax", "planes", "aimed"),
    "pairs": ("graze", "tmax", "aimed"),       # (every hit of a pair is a tie or nearly one: nothing for float64 to say)
    "one": ("general",),
    "two": ("general",),
    "nine": ("general",),
    "two_classes": ("general",),
    "other_class": ("general",),
    "scaled_member": ("general",),
    "ell_rot": ("box", "general"),
    "ell_odd": ("box", "units", "general"),
    "neg_before": ("degenerate", "general"),
    "neg_after": ("degenerate", "general"),
}
# the runs whose trailing form takes sphere_run_lanes (at most eight translated spheres of one class) and those it must refuse
LANES_RUNS = ("radii", "far", "pairs", "one", "two", "other_class", "neg_before", "neg_after")
REFUSED_RUNS = ("nine", "two_classes", "scaled_member", "ell_rot", "ell_odd")


def runs(pkg):
    """name -> [{"center", "radius", "transform", "box"}]; box: None (the box ptc_make_object makes), "half" (clipped to the half
    below the centre's x) or "empty_y" (min and max exchanged on y)"""
    glm = pkg.glmlite
    zero = (0.0, 0.0, 0.0)

    def obj(radius, translation=zero, center=zero, transform=None, box=None):
        return {"center": center, "radius": radius, "transform": glm.translate(translation) if transform is None else transform, "box": box}

    tilt = glm.rotate(np.float32(0.7), (0.3, 1.0, 0.2))

    def ell(scale, at):
        return obj(1.0, transform=glm.compose([glm.scale(scale), tilt, glm.translate(at)]))

    shear = glm.identity()
    shear[1, 0], shear[2, 1] = 0.5, -0.25                      # x += 0.5 y, y -= 0.25 z
    other = glm.translate((0.25, 0.0, 0.0))
    other[1, 0] = -0.0                                         # a translation spelled with a -0: a class of its own
    wall = obj(1000.0, (0.0, 0.0, -1003.0))
    ghosts = [obj(-0.5), obj(0.5, (2.0, 0.0, 0.0), box="half"), obj(0.5, (-2.0, 0.0, 0.0), box="empty_y"), obj(0.0, (0.0, 2.0, 0.0))]
    r = {
        "radii": [obj(1e-3, (0.2, 0.9, -0.4)), obj(0.5), obj(30.0, (60.0, 0.0, 0.0)), obj(1000.0, (0.0, -1000.5, 0.0))],
        # the centre in the transform, in the Sphere, in both; 1e3 .. 1e5 from the origin; a partner or a wall behind each
        "far": [obj(0.5, (1000.0, 800.0, -1200.0)), obj(0.5, zero, (1000.31, 800.0, -1200.0)),
                obj(0.5, (9000.0, -7000.0, 4000.0), (0.3, 0.2, 0.1)), obj(0.35, (9000.0, -7000.0, 4000.0), (-0.55, 0.25, 0.2)),
                obj(0.5, (1e5, -7e4, 4e4), (0.3, 0.2, 0.1)), obj(1000.0, (1e5, -7e4, 4e4), (0.0, 0.0, -1003.0)),
                obj(1000.0, (1000.0, 800.0, -1200.0), (0.0, 0.0, -1003.0))],
        # a coincident pair, and pairs whose centres are 2^-4, 2^-12 and 2^-20 apart
        "pairs": [obj(0.5), obj(0.5), obj(0.5, (3.0, 0.0, 0.0)), obj(0.5, (3.0 + 2.0 ** -4, 0.0, 0.0)), obj(0.5, (6.0, 0.0, 0.0)),
                  obj(0.5, (6.0 + 2.0 ** -12, 0.0, 0.0)), obj(0.5, (9.0, 0.0, 0.0)), obj(0.5, (9.0 + 2.0 ** -20, 0.0, 0.0))],
        "one": [obj(0.5)],
        "two": [obj(0.5), obj(0.5, (0.25, 0.0, 0.0))],
        "nine": [obj(0.3, (0.5 * k - 2.0, 0.1 * (k % 3), -0.2 * k)) for k in range(9)],
        "two_classes": [obj(0.5), obj(0.5, transform=other)],
        "other_class": [obj(0.5, transform=other)],
        "scaled_member": [obj(0.5), obj(1.0, transform=glm.compose([glm.scale(0.5), glm.translate((1.2, 0.0, 0.0))]))],
        "ell_rot": [ell((1.0, 3.0, 1.0), zero), ell((3.0, 1.0, 1.0), (10.0, 0.0, 0.0)), ell((0.2, 1.0, 2.0), (20.0, 0.0, 0.0)),
                    ell((100.0, 1.0, 1.0), (0.0, 500.0, 0.0))],
        "ell_odd": [obj(1.0, transform=glm.compose([shear, glm.translate((30.0, 0.0, 0.0))])),
                    ell((-1.0, 1.5, 1.0), (40.0, 0.0, 0.0)),                 # a mirror: negative determinant
                    obj(1.0, transform=glm.compose([glm.scale(1e-3), glm.translate((0.0, 10.0, 0.0))])),
                    obj(1.0, transform=glm.compose([glm.scale(1e3), glm.translate((0.0, 0.0, 5000.0))]))],
        "neg_before": ghosts + [wall],
        "neg_after": [wall] + ghosts,
    }
    return r


def _edit_box(ob, kind):
    if kind == "half":
        ob["aabb_max"][0] = 0.5 * (ob["aabb_min"][0] + ob["aabb_max"][0])
    elif kind == "empty_y":
        lo, hi = float(ob["aabb_min"][1]), float(ob["aabb_max"][1])
        ob["aabb_min"][1], ob["aabb_max"][1] = hi, lo
    elif kind is not None:
        raise ValueError(kind)


def build(pkg, name, placement="whole"):
    """-> (flat, first): the flat scene with the run as the whole object list ("whole"), in front of a small heightfield
    ("leading") or behind it ("trailing"), and the index of the run's first object"""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.resolution = (8, 8)
    for k in range(MATERIALS):
        s.add_material("m%d" % k, pkg.DiffuseMateral((0.1 + 0.08 * k, 0.5, 0.9 - 0.08 * k)))
    objs = runs(pkg)[name]

    def ground():
        mesh = pkg.scenes.heightfield_mesh(9, 5, 2.0, 1.0, seed=5)
        s.add_mesh("ground", mesh)
        s.add_object(mesh, glm.translate((0.5, -1.5, 0.5)), "m%d" % (MATERIALS - 1))

    if placement == "trailing":
        ground()
    first = len(s.objects_)
    for k, o in enumerate(objs):
        s.add_object(pkg.Sphere(o["center"], o["radius"]), o["transform"], "m%d" % k)
    if placement == "leading":
        ground()
    elif placement not in ("whole", "trailing"):
        raise ValueError(placement)
    flat = s.build_scene()
    for k, o in enumerate(objs):
        _edit_box(flat.objects[first + k], o["box"])
    return flat, first


def subset(pkg, flat, keep):
    """the flat scene with the sphere objects `keep` (indices, in order) alone"""
    keep = list(keep)
    ob = flat.objects[keep].copy()
    ob["index"] = np.arange(len(keep), dtype=np.uint32)
    sph = np.ascontiguousarray(np.asarray(flat.spheres, dtype=np.float32).reshape(-1, 4)[[int(flat.objects[i]["index"]) for i in keep]])
    return pkg.scene_description.FlatScene(objects=ob, object_material_indices=np.ascontiguousarray(flat.object_material_indices[keep]),
                                           spheres=sph, materials=flat.materials, positions=np.zeros((0, 3), dtype=np.float32),
                                           indices=np.zeros((0,), dtype=np.uint32))


def world(flat, i):
    """object i in float64: the matrix' 3 x 3 part [row][col], the world centre, the radius, the largest stretch"""
    ob = flat.objects[i]
    m = np.asarray(ob["m"], dtype=np.float64).reshape(4, 4).T
    c, r = np.asarray(flat.spheres, dtype=np.float64).reshape(-1, 4)[int(ob["index"])][:3], float(np.asarray(flat.spheres).reshape(-1, 4)[int(ob["index"])][3])
    return m[:3, :3], m[:3, :3] @ c + m[:3, 3], r, float(np.linalg.norm(m[:3, :3], 2))


def walk(orc, pkg, flat, first, count, rays):
    """The reference's in-order walk over the run's objects, from the one-object answers with t_max shrinking:
    -> accepted [n, count] (object k is accepted at its turn), t [n] (the closest hit at the end, the ray's t_max if none)"""
    rays = np.array(rays, dtype=np.float32, copy=True).reshape(-1, 8)
    accepted = np.zeros((len(rays), count), dtype=bool)
    for k in range(count):
        recs, hit = orc.intersect_rays(subset(pkg, flat, [first + k]), rays)
        accepted[:, k] = hit.astype(bool)
        rays[:, 7] = np.where(accepted[:, k], recs["t"], rays[:, 7])
    return accepted, rays[:, 7].copy()


def box_gate(orc, flat, i, rays):
    """ray_aabb_intersection_test (intersections.cuh:87-103) of object i's stored box, ray by ray through the oracle"""
    lib = orc.lib()
    box = np.concatenate([flat.objects[i]["aabb_min"], flat.objects[i]["aabb_max"]]).astype(np.float32)
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
    out = np.zeros(len(rays), dtype=bool)
    for j in range(len(rays)):
        out[j] = lib.orc_ray_aabb(C.cast(rays[j:j + 1].ctypes.data, C.POINTER(orc.ORay)), box.ctypes.data) != 0
    return out


# ---- rays --------------------------------------------------------------------------------------------------------------------

def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _perp(rng, d):
    v = _unit(rng, len(d))
    v -= np.einsum("rk,rk->r", v, d)[:, None] * d
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _pack(o, d, tmin, tmax):
    r = np.zeros((len(o), 8), dtype=np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmin, d, tmax
    return r


def _tmins(n):
    return np.where(np.arange(n) % 2 == 0, np.float32(1e-4), np.float32(1e-5)).astype(np.float32)


def _targets(flat, first, count, which=None):
    which = range(count) if which is None else which
    return [(k,) + world(flat, first + k) for k in which]


def aimed(rng, flat, first, count, n=N, which=None, finite_tmax=0.3):
    """random rays at the objects of the run in turn: from 1.5 .. 6 bounding radii away, at a point within 1.3 of them"""
    tg = _targets(flat, first, count, which)
    o, d, tmax = np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, FLT_MAX, dtype=np.float64)
    for j, (k, a, c, r, sig) in enumerate(tg):
        sel = np.arange(n) % len(tg) == j
        m = int(sel.sum())
        rb = max(abs(r) * sig, 0.25)
        o[sel] = c + _unit(rng, m) * rb * rng.uniform(1.5, 6.0, (m, 1))
        at = c + _unit(rng, m) * rb * rng.uniform(0.0, 1.3, (m, 1))
        d[sel] = (at - o[sel]) / np.linalg.norm(at - o[sel], axis=1, keepdims=True)
        tmax[sel] = np.where(rng.uniform(size=m) < finite_tmax, rng.uniform(0.5, 8.0, m) * rb, FLT_MAX)
    return _pack(o, d, _tmins(n), tmax)


def graze(rng, flat, first, count, n=N, which=None):
    """(translated spheres) impact parameter r (1 + s 2^-k), k = 6 .. 24, s = -1, 0, +1, from 1.5 r, 10 r and r + 1 (r >= 30)"""
    tg = _targets(flat, first, count, which)
    combos = []
    for (k, a, c, r, sig) in tg:
        for dist in ([1.5 * r, 10.0 * r] + ([r + 1.0] if r >= 30.0 else [])):
            combos += [(k, c, r, dist, s * 2.0 ** -e) for e in range(6, 25) for s in (-1.0, 1.0)] + [(k, c, r, dist, 0.0)]
    o, d = np.zeros((n, 3)), _unit(rng, n)
    p = _perp(rng, d)
    target, rel = np.zeros(n, dtype=np.int64), np.zeros(n)
    for i in range(n):
        target[i], c, r, dist, rel[i] = combos[i % len(combos)]
        b = r * (1.0 + rel[i])
        dist = max(dist, 1.001 * b)                                # (r + 1 away from a sphere of radius 1000: beside it)
        o[i] = c + b * p[i] - np.sqrt(dist * dist - b * b) * d[i]
    return _pack(o, d, _tmins(n), FLT_MAX), target, rel


def tmin_edge(rng, flat, first, count, n=N, which=None):
    """the origin t_min (1 + s 2^-k) in front of a surface point: entering (the near root) or leaving (the far root, from inside)"""
    tg = _targets(flat, first, count, which)
    d, u = _unit(rng, n), _unit(rng, n)
    tmins = _tmins(n).astype(np.float64)
    i = np.arange(n)
    inside = (i // 2) % 2 == 1
    dots = np.einsum("rk,rk->r", u, d)
    u = np.where(((dots > 0) != inside)[:, None], -u, u)          # outside: the surface faces the ray; inside: it faces away
    u = u + np.where(inside, 1.0, -1.0)[:, None] * d              # ... and steeply (|cos| >= 0.7): the other root is a good part of r away
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    e = 1 + (i // 4) % 23
    s = np.where((i // 92) % 2 == 0, -1.0, 1.0)
    tau = tmins * (1.0 + s * 2.0 ** -e)
    o = np.zeros((n, 3))
    for j, (k, a, c, r, sig) in enumerate(tg):
        sel = (i // 184) % len(tg) == j
        o[sel] = c + r * u[sel] - tau[sel, None] * d[sel]
    return _pack(o, d, tmins.astype(np.float32), FLT_MAX), tau, np.array([t[0] for t in tg])[(i // 184) % len(tg)]


def tmax_edge(rng, orc, pkg, flat, first, count, n=N, which=None):
    """aimed rays with the closest hit carried in at t (1 + s 2^-k), k = 10 .. 23, of the object aimed at (t: the one-object
    oracle's), and -- every fourth ray -- at exactly the t the reference records for the object before it in the list"""
    which = list(range(count) if which is None else which)
    rays = aimed(rng, flat, first, count, n, which, finite_tmax=0.0)
    i = np.arange(n)
    e = 10 + (i // (4 * len(which))) % 14
    s = np.where((i // (56 * len(which))) % 2 == 0, -1.0, 1.0)
    tmax = rays[:, 7].copy()
    target = np.zeros(n, dtype=np.int64)
    for j, k in enumerate(which):
        sel = i % len(which) == j
        target[sel] = k
        recs, hit = orc.intersect_rays(subset(pkg, flat, [first + k]), rays[sel])
        t = recs["t"].astype(np.float64)
        carried = np.where(hit.astype(bool), (t * (1.0 + s[sel] * 2.0 ** -e[sel])).astype(np.float32), FLT_MAX)
        fourth = (i[sel] // len(which)) % 4 == 3
        carried = np.where(fourth & hit.astype(bool), recs["t"], carried)          # (no object before, or it is missed: the target's own t)
        if k > 0:
            before, hit_b = orc.intersect_rays(subset(pkg, flat, [first + k - 1]), rays[sel])
            carried = np.where(fourth & hit_b.astype(bool), before["t"], carried)
        tmax[sel] = carried
    rays[:, 7] = tmax
    return rays, target


def directions(rng, flat, first, count, n=N, which=None):
    """aimed rays with direction lengths 1e-3, 0.5, 2, 1e3; then, in turn: nothing, a +0 and a -0 direction component (the origin
    moved into the target's plane on that axis, so that the ray still meets it), a -0 and a +0 origin coordinate"""
    tg = _targets(flat, first, count, which)
    rays = aimed(rng, flat, first, count, n, which).astype(np.float64)
    i = np.arange(n)
    for j, (k, a, c, r, sig) in enumerate(tg):
        for axis in range(3):
            for kind, value in ((1, 0.0), (2, -0.0)):
                sel = (i % len(tg) == j) & ((i // len(tg)) % 5 == kind) & ((i // (5 * len(tg))) % 3 == axis)
                rays[sel, 4 + axis] = value
                rays[sel, axis] = c[axis] + rng.uniform(-0.6, 0.6, int(sel.sum())) * abs(r)
            for kind, value in ((3, -0.0), (4, 0.0)):
                sel = (i % len(tg) == j) & ((i // len(tg)) % 5 == kind) & ((i // (5 * len(tg))) % 3 == axis)
                rays[sel, axis] = value
    length = np.array([1e-3, 0.5, 2.0, 1e3])[(i // (15 * len(tg))) % 4]
    rays[:, 4:7] *= length[:, None]
    return rays.astype(np.float32)


def planes(rng, flat, first, k, n=N):
    """from inside object k (centre in the Sphere, no translation): origin coordinate `axis` = the centre's, exactly; direction
    component `axis` = +-1e-30, the other two a random unit vector.  For y and z the origin is 0.24 .. 0.44 beyond the centre
    in x (in the run "far": outside the sphere 0.31 in front of it).  -> rays, axis"""
    a, c, r, sig = world(flat, first + k)
    c32 = np.asarray(flat.spheres, dtype=np.float32).reshape(-1, 4)[int(flat.objects[first + k]["index"])][:3]
    i = np.arange(n)
    axis = np.array([1, 2, 0])[i % 3]
    off = rng.uniform(-0.15, 0.15, (n, 3))
    off[:, 0] = np.where(axis == 0, 0.0, rng.uniform(0.24, 0.44, n))
    o = (c32.astype(np.float64) + off).astype(np.float32)
    o[i, axis] = c32[axis]
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    d = np.zeros((n, 3), dtype=np.float32)
    d[i, (axis + 1) % 3], d[i, (axis + 2) % 3] = np.cos(ang), np.sin(ang)
    d[:, 0] = np.abs(d[:, 0])                                   # (away from the sphere in front)
    d[i, axis] = np.where((i // 3) % 2 == 0, np.float32(1e-30), np.float32(-1e-30))
    return _pack(o, d, _tmins(n), FLT_MAX), axis


def box_edges(rng, flat, first, count, n=N, which=None):
    """Ellipsoids.  Three rays of four: a line past an edge of the object's stored box, 2^-k (k = 6 .. 24) of the box' size inside
    or outside it.  The fourth: a ray at a surface point of the ellipsoid outside that box, where the object has one."""
    tg = _targets(flat, first, count, which)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    kind = np.zeros(n, dtype=np.int64)         # 1: inside the edge, -1: outside it, 2: at the part outside the box
    target = np.zeros(n, dtype=np.int64)
    i = np.arange(n)
    for j, (k, a, c, r, sig) in enumerate(tg):
        bmin = np.asarray(flat.objects[first + k]["aabb_min"], dtype=np.float64)
        bmax = np.asarray(flat.objects[first + k]["aabb_max"], dtype=np.float64)
        ext = float(np.max(bmax - bmin))
        u = _unit(rng, 20000)
        surf = c + (r * u) @ a.T
        nrm = u @ np.linalg.inv(a)                                  # transpose(inverse) * u
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        out = np.nonzero(np.any((surf < bmin - 0.02 * ext) | (surf > bmax + 0.02 * ext), axis=1))[0]
        for idx in np.nonzero(i % len(tg) == j)[0]:
            q = idx // len(tg)
            target[idx] = k
            if q % 4 == 3 and len(out) > 50:
                pick = out[rng.integers(len(out))]
                v = nrm[pick] + 0.4 * _unit(rng, 1)[0]
                o[idx] = surf[pick] + v / np.linalg.norm(v) * ext * rng.uniform(0.5, 2.0)
                d[idx] = (surf[pick] - o[idx]) / np.linalg.norm(surf[pick] - o[idx])
                kind[idx] = 2
                continue
            ax = int(rng.integers(3))
            bx, cx = (ax + 1) % 3, (ax + 2) % 3
            sa, sb = rng.choice([-1.0, 1.0]), rng.choice([-1.0, 1.0])
            e = 6 + (q // 8) % 19
            side = 1.0 if (q // 4) % 2 == 0 else -1.0
            p = np.zeros(3)
            p[ax] = (bmax if sa > 0 else bmin)[ax] + sa * side * ext * 2.0 ** -e / np.sqrt(2.0)
            p[bx] = (bmax if sb > 0 else bmin)[bx] + sb * side * ext * 2.0 ** -e / np.sqrt(2.0)
            p[cx] = rng.uniform(bmin[cx], bmax[cx])
            phi = rng.uniform(-0.5, 0.5)
            dir_ = np.zeros(3)
            dir_[ax], dir_[bx], dir_[cx] = sa * np.cos(phi) / np.sqrt(2.0), -sb * np.cos(phi) / np.sqrt(2.0), np.sin(phi)
            if rng.uniform() < 0.5:
                dir_ = -dir_
            o[idx] = p - dir_ * ext * rng.uniform(1.0, 3.0)
            d[idx] = dir_
            kind[idx] = -1 if side > 0 else 1
    return _pack(o, d, _tmins(n), FLT_MAX), target, kind


def units(rng, flat, first, small, big, n=N):
    """Object `big` (scale 1e3): from t_min * 1e3 * (0.05 .. 0.8) above the surface, straight down to 35 degrees off, with a t_max of
    0.5 .. 1.5 -- the surface is nearer than t_max in the world, the near root is below t_min in object units and the far root
    (about 2) beyond t_max: the reference misses.  Object `small` (scale 1e-3): from 0.3 .. 0.8 away at its inner half; the root
    is that distance in the world and a thousand times it in object units; t_max 2 .. 100 (between the two: the reference misses)
    or 1e3 .. 1e4 (beyond both: a hit).  -> rays, target, world_t (the distance to the surface along the ray, float64)"""
    o, d, tmax = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    tmins = _tmins(n).astype(np.float64)
    i = np.arange(n)
    target = np.where(i % 2 == 0, big, small)
    a, c, r, sig = world(flat, first + big)
    sel = target == big
    m = int(sel.sum())
    nrm = _unit(rng, m)
    delta = tmins[sel] * sig * rng.uniform(0.05, 0.8, m)
    o[sel] = c + (abs(r) * sig + delta)[:, None] * nrm
    v = -nrm + np.tan(rng.uniform(0.0, 0.6, (m, 1))) * _perp(rng, nrm)
    d[sel] = v / np.linalg.norm(v, axis=1, keepdims=True)
    tmax[sel] = rng.uniform(0.5, 1.5, m)
    a, c, r, sig = world(flat, first + small)
    sel = target == small
    m = int(sel.sum())
    o[sel] = c + _unit(rng, m) * rng.uniform(0.3, 0.8, (m, 1))
    at = c + _unit(rng, m) * abs(r) * sig * rng.uniform(0.0, 0.5, (m, 1))
    d[sel] = (at - o[sel]) / np.linalg.norm(at - o[sel], axis=1, keepdims=True)
    tmax[sel] = np.where((i[sel] // 2) % 2 == 0, rng.uniform(2.0, 100.0, m), rng.uniform(1e3, 1e4, m))
    rays = _pack(o, d, tmins.astype(np.float32), tmax)
    # the distance to the world-space sphere along the rounded ray (both objects are uniformly scaled: a sphere in the world)
    r64 = rays.astype(np.float64)
    world_t = np.full(n, np.inf)
    for k in (big, small):
        a, c, r, sig = world(flat, first + k)
        sel = target == k
        oc = r64[sel, 0:3] - c
        dn = r64[sel, 4:7] / np.linalg.norm(r64[sel, 4:7], axis=1, keepdims=True)
        b = np.einsum("rk,rk->r", oc, dn)
        disc = b * b - (np.einsum("rk,rk->r", oc, oc) - (r * sig) ** 2)
        t1 = -b - np.sqrt(np.maximum(disc, 0.0))
        world_t[sel] = np.where((disc > 0) & (t1 > 0), t1, np.inf)
    return rays, target, world_t


def degenerate(rng, flat, first, count, ghosts, n=N):
    """from three units in front (+z) of every ghost object's centre, within 0.45 of its axis, towards -z and up to 6 degrees off:
    through the object's inner ball (if it had one) and on to the wall behind.  -> rays, target"""
    tg = _targets(flat, first, count, ghosts)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    target = np.zeros(n, dtype=np.int64)
    for j, (k, a, c, r, sig) in enumerate(tg):
        sel = np.arange(n) % len(tg) == j
        m = int(sel.sum())
        rad, ang = 0.45 * np.sqrt(rng.uniform(size=m)), rng.uniform(0, 2 * np.pi, m)
        o[sel] = c + np.stack([rad * np.cos(ang), rad * np.sin(ang), np.full(m, 3.0)], axis=1)
        v = np.stack([rng.uniform(-0.1, 0.1, m), rng.uniform(-0.1, 0.1, m), -np.ones(m)], axis=1)
        d[sel] = v / np.linalg.norm(v, axis=1, keepdims=True)
        target[sel] = k
    return _pack(o, d, _tmins(n), FLT_MAX), target


def ghost_objects(pkg, name):
    """indices (within the run) of the degenerate objects of a neg_* run, by kind"""
    objs = runs(pkg)[name]
    out = {}
    for k, o in enumerate(objs):
        if o["radius"] < 0:
            out["negative"] = k
        elif o["radius"] == 0:
            out["zero"] = k
        elif o["box"] is not None:
            out[o["box"]] = k
    return out


def family(pkg, orc, name, fam, flat=None, first=0):
    """-> (rays [N, 8] float32, info): info holds what the family's proof needs (targets, kinds, constructed roots)"""
    if flat is None:
        flat, first = build(pkg, name)
    count = len(runs(pkg)[name])
    rng = np.random.default_rng([sorted(FAMILIES).index(name), sorted({f for v in FAMILIES.values() for f in v}).index(fam)])
    round_objects = [k for k in range(count) if runs(pkg)[name][k]["radius"] > 0]
    if fam in ("general", "aimed"):
        return aimed(rng, flat, first, count), {}
    if fam == "graze":
        rays, target, rel = graze(rng, flat, first, count, which=round_objects)
        return rays, {"target": target, "rel": rel}
    if fam == "tmin":
        rays, tau, target = tmin_edge(rng, flat, first, count, which=[0, 1, 2])
        return rays, {"tau": tau, "target": target}
    if fam == "tmax":
        rays, target = tmax_edge(rng, orc, pkg, flat, first, count, which=round_objects)
        return rays, {"target": target}
    if fam == "direction":
        return directions(rng, flat, first, count, which=[1, 3]), {}
    if fam == "planes":
        rays, axis = planes(rng, flat, first, 1)
        return rays, {"axis": axis, "target": 1}
    if fam == "box":
        rays, target, kind = box_edges(rng, flat, first, count)
        return rays, {"target": target, "kind": kind}
    if fam == "units":
        rays, target, world_t = units(rng, flat, first, small=2, big=3)
        return rays, {"target": target, "world_t": world_t}
    if fam == "degenerate":
        g = ghost_objects(pkg, name)
        rays, target = degenerate(rng, flat, first, count, sorted(g.values()))
        return rays, {"target": target, "ghosts": g}
    raise ValueError(fam)


def interleave(parts):
    """rays of several families dealt out in turn (ray i of the result: family i % F), so that the slots of a lane, 256 rays
    apart, and the lanes of a wavefront hold rays of different families.  -> rays, family index per ray"""
    f = len(parts)
    out = np.zeros((f * N, 8), dtype=np.float32)
    for j, p in enumerate(parts):
        out[j::f] = p
    return out, np.arange(f * N) % f


# ---- frames ------------------------------------------------------------------------------------------------------------------

def frame_scene(pkg, kind):
    """-> (scene description, flat scene) of a 64 x 48 frame: "neg_trailing" / "neg_leading" (a sphere of radius -0.5 listed before
    the sphere behind it, in a run behind a heightfield that ends the list / in front of it), "clipped" (a sphere whose stored box
    is clipped to half, in front of another), "ellipsoids" (the (1, 3, 1) ellipsoid in front of a wall that is a unit sphere under
    a scale of 1e3)"""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.resolution = (64, 48)
    s.camera = pkg.Camera(position=(0.0, 0.3, 4.0), rotation=(1.0, 0.0, 0.0, 0.0), vfov=float(np.radians(50)))
    s.add_material("white", pkg.DiffuseMateral((0.8, 0.8, 0.8)))
    s.add_material("red", pkg.DiffuseMateral((0.8, 0.2, 0.2)))
    s.add_material("steel", pkg.MetalMaterial((0.8, 0.8, 0.9), 0.1))
    s.add_material("glass", pkg.DielectricMaterial(1.5))

    def ball(center, radius, material, transform=None):
        s.add_object(pkg.Sphere((0.0, 0.0, 0.0), radius), glm.translate(center) if transform is None else transform, material)

    def ground(at):
        mesh = pkg.scenes.heightfield_mesh(17, 9, 8.0, 6.0, seed=5)
        s.add_mesh("ground", mesh)
        s.add_object(mesh, glm.translate(at), "white")

    # a mesh that opens the list and a sphere run that ends it: the shape the kernels that end a bounce (k_shade_fused, k_persist)
    # walk the run for; "neg_leading" turns it round (k_spheres, or the kernel that ends the bounce before)
    edits = {}
    if kind in ("neg_trailing", "neg_leading", "clipped"):
        if kind != "neg_leading":
            ground((0.0, -0.7, 0.0))
        ghost = len(s.objects_)
        ball((0.0, 0.2, 1.5), -0.5 if kind != "clipped" else 0.5, "steel")
        if kind == "clipped":
            edits[ghost] = "half"
        ball((0.1, 0.3, -0.5), 0.8, "red")                    # behind it, later in the list
        ball((-1.3, 0.0, 0.3), 0.45, "glass")
        ball((0.0, 0.0, -1004.0), 1000.0, "white")            # a wall behind them all
        if kind == "neg_leading":
            ground((0.0, -0.7, 0.0))
    elif kind == "ellipsoids":
        tilt = glm.rotate(np.float32(0.7), (0.3, 1.0, 0.2))
        ground((0.0, -0.9, 0.0))
        ball(None, 1.0, "white", glm.compose([glm.scale(1e3), glm.translate((0.0, 0.0, -1004.0))]))
        ball(None, 0.5, "steel", glm.compose([glm.scale((1.0, 3.0, 1.0)), tilt, glm.translate((-0.6, 0.3, 0.0))]))
        ball((1.2, 0.0, 0.5), 0.5, "glass")
        ball((0.9, 0.1, -1.5), 0.6, "red")
    else:
        raise ValueError(kind)
    flat = s.build_scene()
    for k, e in edits.items():
        _edit_box(flat.objects[k], e)
    return s, flat
