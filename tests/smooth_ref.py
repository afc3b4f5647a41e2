"""CPU restatement of smooth shading (ptc_set_vertex_normals, ptc_set_param "smooth_normals", ptc_hit_attributes) in
numpy binary32 -- TEST INFRASTRUCTURE: the checker of tests/test_smooth_cpu.py and tests/test_gpu_smooth.py, not the thing under test.

What stands here: the host's area-weighted vertex normals and the shading normal of section 5n, every numpy operation one binary32
operation of the rule in its order (numpy does not contract into FMA); the winner of a closest hit -- the oracle's closest hit, and among
the triangles the one whose own binary32 ray_triangle lines reproduce the oracle's t bit for bit, ties resolved by the depth-first leaf
order of the oracle's tree within a mesh and by object order across objects (the reference accepts an equal t, so the one visited last
wins).  The loop that applies them is loop_ref.render_megakernel's under `smooth`."""
import numpy as np

from ref_f32 import F, _cross, _dot, _normalize, _xform_point

FLT_MAX = F(np.finfo(np.float32).max)
EPS = F(0.0000001)
NONE = 0xFFFFFFFF
COUNTERS = ("shading_normals", "fallbacks", "absorbed", "culled_light_samples")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the vertex normals (pt_smooth.hpp: vertex_normals) ----------------------------------------------------------------------------------
def mesh_rows(flat):
    """(first_vertex, vertex_count, first_index, index_count) of every mesh of the scene"""
    ranges = getattr(flat, "mesh_ranges", None)
    if ranges is None:
        return [(0, len(flat.positions), 0, len(flat.indices))] if len(flat.indices) else []
    return [tuple(int(x) for x in r[:4]) for r in np.asarray(ranges).reshape(-1, 6)]


def vertex_normals(positions, indices):
    """One mesh: triangles in index order, c = cross(p1 - p0, p2 - p0) added to the sums of corners 0, 1, 2 in that order; a sum s with
    0 < dot(s, s) <= FLT_MAX becomes normalize(s), every other one (0, 0, 0)"""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1, 3)
    acc = np.zeros_like(pos)
    with np.errstate(all="ignore"):
        p0 = pos[idx[:, 0]]
        c = _cross(pos[idx[:, 1]] - p0, pos[idx[:, 2]] - p0).astype(np.float32)
        for t in range(len(idx)):  # serial: the sums' order is the triangles'
            for k in range(3):
                acc[idx[t, k]] = acc[idx[t, k]] + c[t]
        l2 = _dot(acc, acc)
        ok = (l2 > F(0.0)) & (l2 <= FLT_MAX)
        return np.where(ok[:, None], _normalize(acc), F(0.0)).astype(np.float32)


def scene_vertex_normals(flat):
    """... of a whole scene, mesh by mesh"""
    pos = np.ascontiguousarray(flat.positions, dtype=np.float32).reshape(-1, 3)
    out = np.zeros_like(pos)
    for fv, nv, fi, ni in mesh_rows(flat):
        out[fv:fv + nv] = vertex_normals(pos[fv:fv + nv], np.asarray(flat.indices)[fi:fi + ni])
    return out


def face_normals_unshared(positions, indices):
    """A mesh restated with three vertices of its own per triangle, and per vertex its triangle's cross(e1, e2): the vertex normals that
    reproduce the face normals -> (positions, indices, normals)"""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
    p = pos[idx]
    t = p.reshape(-1, 3, 3)
    c = _cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]).astype(np.float32)
    return p, np.arange(len(idx), dtype=np.uint32), np.repeat(c, 3, axis=0)


# ---- the rule (pt_smooth.hpp: shading_normal) -------------------------------------------------------------------------------------------
def _xform_normal(inv16, n):
    """transform_normal: (transpose(M^-1) * (n, 0)).xyz with mat4 * vec4 = (c0 x + c1 y) + (c2 z + c3 w)"""
    m = np.asarray(inv16, dtype=np.float32).reshape(-1, 16)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    return np.stack([(m[:, 4 * r] * x + m[:, 4 * r + 1] * y) + (m[:, 4 * r + 2] * z + m[:, 4 * r + 3] * F(0.0)) for r in range(3)], axis=-1)


def shading_normal(n0, n1, n2, u, v, g, d, inv16):
    """Section 5n, steps 1-8, per row; inv16 one inverse matrix [16] or one per row [k, 16] -> (n_s [k, 3], fallback bool[k])"""
    n0, n1, n2, g, d = (np.asarray(a, dtype=np.float32).reshape(-1, 3) for a in (n0, n1, n2, g, d))
    u, v = np.asarray(u, dtype=np.float32).reshape(-1), np.asarray(v, dtype=np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        t = F(1.0) - u
        w = t - v
        m = (n0 * w[:, None] + n1 * u[:, None]) + n2 * v[:, None]
        a = _xform_normal(inv16, m).astype(np.float32)
        l2 = _dot(a, a)
        ok = (l2 > F(0.0)) & (l2 <= FLT_MAX)
        s = _normalize(a).astype(np.float32)
        c = _dot(s, g)
        s = np.where((c < F(0.0))[:, None], -s, s)
        ok &= (c < F(0.0)) | (c > F(0.0))
        ok &= _dot(d, s) < F(0.0)
    return np.where(ok[:, None], s, g).astype(np.float32), ~ok


# ---- the winner of a closest hit --------------------------------------------------------------------------------------------------------
def _mesh_of(flat, obj):
    return int(obj["index"]) if getattr(flat, "mesh_ranges", None) is not None else 0


def _tree_of(sh, mesh):
    if sh.mesh_ranges is None:
        return sh.bvh
    r = sh.mesh_ranges[mesh]
    return sh.bvh[int(r[4]):int(r[4]) + int(r[5])]


def leaf_order(nodes):
    """the offsets (in the mesh's indices) of the triangles in the order the reference's depth-first, left-first walk meets them"""
    out, stack = [], [0] if len(nodes) else []
    while stack:
        node = nodes[stack.pop()]
        first = int(node["first_child_or_primitive"])
        if int(node["primitive_count"]) != 0:
            out.append(first)
        else:
            stack.append(first + 1)
            stack.append(first)
    return np.asarray(out, dtype=np.int64)


def _triangle_lines(o, d, tmin, p0, p1, p2):
    """ray_triangle_intersection_test's lines for rays [r] x triangles [t] -> (passes bool[r, t], t, u, v float32[r, t])"""
    with np.errstate(all="ignore"):
        e1, e2 = (p1 - p0)[None, :, :], (p2 - p0)[None, :, :]
        dd = d[:, None, :]
        h = _cross(dd, e2)
        a = _dot(e1, h)
        ok = ~((a > -EPS) & (a < EPS))
        f = F(1.0) / a
        s = o[:, None, :] - p0[None, :, :]
        u = f * _dot(s, h)
        ok &= ~((u < F(0.0)) | (u > F(1.0)))
        q = _cross(s, e1)
        v = f * _dot(dd, q)
        ok &= ~((v < F(0.0)) | (u + v > F(1.0)))
        t = f * _dot(e2, q)
        ok &= ~(t < tmin[:, None])
    return ok, t.astype(np.float32), u.astype(np.float32), v.astype(np.float32)


def winners(orc, flat, sh, rays, recs, hit, chunk=512):
    """Per ray (rays [n, 8], with the oracle's records and hit flags of the same rays) the winner of the closest hit:
    -> (object int64[n], -1 on a miss; first int64[n], the winner's offset in its mesh's indices, -1 for a sphere or a miss; u, v)"""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
    n = len(rays)
    obj_of, first_of = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    u_of, v_of = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    rows = np.nonzero(np.asarray(hit).astype(bool))[0]
    if len(rows) == 0:
        return obj_of, first_of, u_of, v_of
    want = _bits(recs["t"][rows])
    pos = np.ascontiguousarray(flat.positions, dtype=np.float32).reshape(-1, 3)
    meshes = mesh_rows(flat)
    for i, obj in enumerate(flat.objects):
        if int(obj["type"]) == 0:
            # a sphere object: the oracle's closest hit on the scene of this object alone reproduces t
            alone, alone_sh = _alone(orc, flat, i)
            r1, h1 = orc.intersect_rays(alone, rays[rows], scene_handle=alone_sh)
            won = h1.astype(bool) & (_bits(r1["t"]) == want)
            obj_of[rows[won]], first_of[rows[won]], u_of[rows[won]], v_of[rows[won]] = i, -1, F(0.0), F(0.0)
            continue
        mesh = _mesh_of(flat, obj)
        if mesh >= len(meshes) or meshes[mesh][3] == 0:
            continue
        fv, nv, fi, ni = meshes[mesh]
        order = leaf_order(_tree_of(sh, mesh))
        idx = np.asarray(flat.indices, dtype=np.int64)[fi:fi + ni]
        world = _xform_point(obj["m"], pos[fv:fv + nv]).astype(np.float32)
        p0, p1, p2 = world[idx[order]], world[idx[order + 1]], world[idx[order + 2]]
        for c0 in range(0, len(rows), chunk):
            rr = rows[c0:c0 + chunk]
            ok, t, u, v = _triangle_lines(rays[rr, 0:3], rays[rr, 4:7], rays[rr, 3], p0, p1, p2)
            ok &= t.view(np.uint32) == want[c0:c0 + chunk, None]
            any_ = ok.any(axis=1)
            last = ok.shape[1] - 1 - np.argmax(ok[:, ::-1], axis=1)  # the one the walk meets last
            k, sel = np.nonzero(any_)[0], rr[any_]
            obj_of[sel], first_of[sel] = i, order[last[k]]
            u_of[sel], v_of[sel] = u[k, last[k]], v[k, last[k]]
    assert (obj_of[rows] >= 0).all(), "a closest hit of the oracle that no primitive's own lines reproduce"
    return obj_of, first_of, u_of, v_of


_alone_cache = {}


def _alone(orc, flat, i):
    """the scene of object i alone (the tables kept, so its sphere / mesh / material indices stay what they are)"""
    key = (id(flat), i)
    if key not in _alone_cache:
        import copy
        one = copy.copy(flat)
        one.objects = np.ascontiguousarray(flat.objects[i:i + 1])
        one.object_material_indices = np.ascontiguousarray(flat.object_material_indices[i:i + 1])
        one.keepalive = []
        if int(flat.objects[i]["type"]) == 0:  # (a sphere walks no mesh)
            one.positions, one.indices, one.mesh_ranges, one.bvh = np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), None, None
        _alone_cache[key] = (one, orc.SceneHandle(one), flat)
    return _alone_cache[key][:2]


def hit_attributes(orc, flat, rays, normals=None, scene_handle=None):
    """ptc_hit_attributes restated -> dict(object, triangle uint32[n]; uv [n, 2]; normal [n, 3])"""
    sh = scene_handle or orc.SceneHandle(flat)
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
    recs, hit = orc.intersect_rays(flat, rays, scene_handle=sh)
    obj, first, u, v = winners(orc, flat, sh, rays, recs, hit)
    normal = np.where(hit.astype(bool)[:, None], recs["normal"].astype(np.float32), F(0.0)).astype(np.float32)
    tri = np.nonzero(first >= 0)[0]
    if normals is not None and len(tri):
        normal[tri] = _shade_rows(flat, normals, obj[tri], first[tri], u[tri], v[tri], recs["normal"][tri].astype(np.float32), rays[tri, 4:7])[0]
    return {"object": np.where(obj >= 0, obj, NONE).astype(np.uint32), "triangle": np.where(first >= 0, first // 3, NONE).astype(np.uint32),
            "uv": np.stack([u, v], axis=-1), "normal": normal}


def _shade_rows(flat, normals, obj, first, u, v, g, d):
    """the rule at triangle hits: the winner's three vertex normals, its object's inverse matrix -> (n_s, fallback)"""
    normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    meshes = mesh_rows(flat)
    idx = np.asarray(flat.indices, dtype=np.int64)
    corner = np.empty((len(obj), 3), dtype=np.int64)
    for k, (o, f) in enumerate(zip(obj, first)):
        fv, _, fi, _ = meshes[_mesh_of(flat, flat.objects[int(o)])]
        corner[k] = fv + idx[fi + int(f):fi + int(f) + 3]
    inv = np.asarray(flat.objects["inv_m"], dtype=np.float32)[obj]
    return shading_normal(normals[corner[:, 0]], normals[corner[:, 1]], normals[corner[:, 2]], u, v, g, d, inv)


# ---- the meshes and scenes the CPU and GPU tests share ----------------------------------------------------------------------------------
def uv_sphere(n_lat, n_lon, radius=0.5):
    """A closed UV sphere: two pole vertices and n_lat - 1 rings of n_lon, 2 n_lon (n_lat - 1) triangles wound outward
    -> (positions [v, 3], indices, radial vertex normals [v, 3])"""
    rings = []
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        ph = 2.0 * np.pi * np.arange(n_lon) / n_lon
        rings.append(np.stack([np.sin(th) * np.cos(ph), np.full(n_lon, np.cos(th)), np.sin(th) * np.sin(ph)], axis=-1))
    unit = np.concatenate([[[0.0, 1.0, 0.0]]] + rings + [[[0.0, -1.0, 0.0]]])
    tris = []
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    south = 1 + (n_lat - 1) * n_lon
    for j in range(n_lon):
        tris.append((0, ring(1, j + 1), ring(1, j)))
        tris.append((south, ring(n_lat - 1, j), ring(n_lat - 1, j + 1)))
        for i in range(1, n_lat - 1):
            a, b, c, d = ring(i, j), ring(i, j + 1), ring(i + 1, j), ring(i + 1, j + 1)
            tris.append((a, b, c))
            tris.append((b, d, c))
    return (unit * radius).astype(np.float32), np.asarray(tris, dtype=np.uint32).reshape(-1), unit.astype(np.float32)


def sheet(nx, nz, size=1.0, bump=0.0, y=0.0):
    """An open sheet of nx x nz quads in the plane y (raised by bump * a fixed pattern), facing +y -> (positions, indices)"""
    ix, iz = np.meshgrid(np.arange(nx + 1), np.arange(nz + 1), indexing="xy")
    x = (ix / nx - 0.5) * size
    z = (iz / nz - 0.5) * size
    yy = y + bump * np.sin(2.3 * ix + 0.7) * np.cos(1.9 * iz + 0.3)
    pos = np.stack([x, yy, z], axis=-1).reshape(-1, 3).astype(np.float32)
    v = (iz[:-1, :-1] * (nx + 1) + ix[:-1, :-1]).astype(np.uint32)
    tri0 = np.stack([v, v + nx + 1, v + 1], axis=-1)
    tri1 = np.stack([v + 1, v + nx + 1, v + nx + 2], axis=-1)
    return pos, np.stack([tri0, tri1], axis=2).reshape(-1).astype(np.uint32)


def sun_map(n=7, seed=5, sun=400.0):
    """a random sky (no two texels alike) with a two-texel sun in the upper hemisphere"""
    m = np.random.default_rng(seed).uniform(0.05, 1.0, (n, n, 3)).astype(np.float32)
    j, i = (2 * n) // 5, n // 2
    m[j, i] = m[j, min(i + 1, n - 1)] = (sun, 0.9 * sun, 0.8 * sun)
    return m


ENV = sun_map()


def room_scene(pkg):
    """direct_loop_scenes' closed lamp-lit room (a box mesh, a sphere lamp) with a 6 x 12 UV sphere and its half-scale rotated instance"""
    import direct_loop_scenes
    glm = pkg.glmlite
    s = direct_loop_scenes.small_lamp_room(pkg)
    s.add_material("ball", pkg.DiffuseMateral((0.7, 0.6, 0.3)))
    s.add_material("ball2", pkg.DiffuseMateral((0.3, 0.5, 0.8)))
    pos, idx, _ = uv_sphere(6, 12)
    mesh = s.add_mesh("models/uv_sphere.obj", pkg.Mesh(pos, idx))
    s.add_object(mesh, glm.translate((0.6, -0.5, 0.4)), "ball")
    s.add_object(mesh, glm.compose([glm.scale(0.5), glm.rotate(0.7, (0.3, 1.0, 0.2)), glm.translate((-0.7, -0.6, 0.9))]), "ball2")
    return s


def sheet_scene(pkg, materials=("diffuse", "diffuse")):
    """Under the sky: a floor sphere, a bumpy open 3 x 3 sheet hovering over it (light leaks at its rim and under its bumps unless the
    geometric tests hold), and two instances of the 6 x 12 UV sphere in the given materials (diffuse, metal, glass, lamp)"""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.add_material("floor", pkg.DiffuseMateral((0.6, 0.6, 0.6)))
    s.add_material("sheet", pkg.DiffuseMateral((0.8, 0.4, 0.3)))
    s.add_material("diffuse", pkg.DiffuseMateral((0.3, 0.6, 0.8)))
    s.add_material("metal", pkg.MetalMaterial((0.9, 0.8, 0.6), 0.1))
    s.add_material("glass", pkg.DielectricMaterial(1.5))
    s.add_material("lamp", pkg.EmissiveMaterial((5.0, 4.5, 4.0)))
    s.add_object(pkg.Sphere((0, 0, 0), 1000.0), glm.translate((0.0, -1001.0, 0.0)), "floor")
    pos, idx = sheet(3, 3, size=2.4, bump=0.25, y=-0.55)
    s.add_object(s.add_mesh("models/sheet.obj", pkg.Mesh(pos, idx)), glm.translate((0.0, 0.0, -0.3)), "sheet")
    pos, idx, _ = uv_sphere(6, 12)
    mesh = s.add_mesh("models/uv_sphere.obj", pkg.Mesh(pos, idx))
    s.add_object(mesh, glm.translate((0.55, 0.25, -0.2)), materials[0])
    s.add_object(mesh, glm.compose([glm.scale((0.5, 0.7, 0.5)), glm.rotate(0.7, (0.3, 1.0, 0.2)), glm.translate((-0.6, 0.1, 0.3))]), materials[1])
    s.camera = pkg.scenes._camera_from_look_at((0.0, 0.9, 3.2), (0.0, -0.1, -0.2), vfov_deg=45.0)
    return s


def sphere_scene(pkg, n_lat=None, n_lon=None):
    """The convergence measure's frame: one ball of radius 0.5 in front of the camera under the gradient -- the analytic sphere object
    (n_lat None), or the n_lat x n_lon UV sphere mesh in its place"""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.add_material("ball", pkg.DiffuseMateral((0.7, 0.7, 0.7)))
    if n_lat is None:
        s.add_object(pkg.Sphere((0, 0, 0), 0.5), glm.translate((0.0, 0.0, 0.0)), "ball")
    else:
        pos, idx, _ = uv_sphere(n_lat, n_lon)
        s.add_object(s.add_mesh("models/uv_sphere.obj", pkg.Mesh(pos, idx)), glm.translate((0.0, 0.0, 0.0)), "ball")
    s.camera = pkg.scenes._camera_from_look_at((0.3, 0.4, 1.6), (0.0, 0.0, 0.0), vfov_deg=45.0)
    return s
