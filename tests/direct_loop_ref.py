"""CPU restatement of the megakernel loop WITH direct lighting (ptc_set_param "direct_light" 1), in numpy
binary32 -- TEST INFRASTRUCTURE, in the manner of lit_ref.py and direct_ref.py: the checker of tests/test_gpu_direct_loop.py, not
the thing under test.

It is lit_ref.render_megakernel's loop with the rule of section 5g added, built from the pinned pieces:
  - lit_ref._primary / shade / sky / _fold / Draws (primary rays, evaluate_material, the sky, the running mean, the material draws);
  - direct_ref.light_table (the lamp table) and direct_ref's binary32 helpers;
  - orc.intersect_rays (closest hits of the path's rays; the HIT FLAG of the shadow rays);
  - orc_path_seed / orc_rng_seed / orc_rng_discard / orc_rng_uniform (the light stream).
direct_ref.sample draws from the generator of index i without a discard, so the three draws and the sample (section 5f, items 1-5)
are restated here, one numpy operation per source operation of light_sample_point, in its order.

The rule: a per-path radiance sum, deposited as radiance + colour; at every hit on a diffuse material, after evaluate_material
(colour = throughput x albedo), one light sample at the hit point about the hit's normal from the stream
seed(path_seed(pixel, iteration) ^ kLightSeedXor), discard(3 * bounce); a sampled sample traces {p, 1e-4, w, d * 0.999} and, if the
oracle reports no hit, radiance += colour * contribution; an emissive hit ends the path with colour * emission if the vertex
before drew no light sample (the camera, metal, glass), else with 0."""
import ctypes as C
import importlib.util
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


lr = _load("lit_ref")
dr = _load("direct_ref")
F = np.float32
EMISSIVE = 3


def light_draws(orc, pixels, iteration, bounce):
    """u0, u1, u2 of the light stream: per pixel a generator seeded path_seed(pixel, iteration) ^ kLightSeedXor, discard(3 * bounce)."""
    h = orc.lib()
    u = np.empty((len(pixels), 3), dtype=np.float32)
    st = C.c_uint32()
    for k, pixel in enumerate(pixels):
        st.value = h.orc_rng_seed(h.orc_path_seed(int(pixel), int(iteration)) ^ dr.SEED_XOR)
        if bounce:
            h.orc_rng_discard(C.byref(st), 3 * int(bounce))
        u[k, 0] = h.orc_rng_uniform(C.byref(st))
        u[k, 1] = h.orc_rng_uniform(C.byref(st))
        u[k, 2] = h.orc_rng_uniform(C.byref(st))
    return u


def light_sample(orc, flat, table, p, nrm, u):
    """light_sample_point for points p with normals nrm and draws u [n, 3]:
    -> dict(rays [n, 8], contribution [n, 3], sampled bool[n]).  table = direct_ref.light_table(flat), total weight > 0."""
    recs, _, _, last = table
    n = len(p)
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0:3], rays[:, 3] = p, dr.T_MIN
    contribution = np.zeros((n, 3), dtype=np.float32)
    if n == 0:
        return {"rays": rays, "contribution": contribution, "sampled": np.zeros(0, dtype=bool)}
    u0, u1, u2 = u[:, 0], u[:, 1], u[:, 2]
    k = dr.select(recs["cdf"], last, u0)
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
        phi = dr.PI2 * u2[sph]
        s, c = dr._sincos(orc, phi)
        d = np.stack([rr * c, rr * s, z], axis=-1)
        spheres = np.asarray(flat.spheres, dtype=np.float32).reshape(-1, 4)
        for j, lane in enumerate(sph):
            obj = flat.objects[int(r["object"][lane])]
            sp = spheres[int(obj["index"])]
            qo = sp[:3] + d[j] * sp[3]
            q[lane] = dr._xform_point(obj["m"], qo)
        nl[sph] = dr._normalize(q[sph] - p0[sph])
    v = q - p
    d2 = dr._dot(v, v)
    valid = (d2 > F(0.0)) & (d2 < F(np.inf))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = np.sqrt(d2)
        inv_d = F(1.0) / d
        w = v * inv_d[:, None]
        cos_r = dr._dot(nrm, w)
        cos_l = np.abs(dr._dot(nl, w))
        inv_pdf = r["inv_pdf"]
        sampled = valid & (cos_r > F(0.0)) & (inv_pdf > F(0.0))
        g = ((cos_r * cos_l) * inv_pdf) / (dr.PI * d2)
        le = np.asarray(flat.materials)["p"][(r["kind_material"] & 0x7FFFFFFF).astype(np.int64), :3].astype(np.float32)
        cb = le * g[:, None]
        tmax = d * F(0.999)
    contribution[sampled] = cb[sampled]
    rays[sampled, 4:7] = w[sampled]
    rays[sampled, 7] = tmax[sampled]
    return {"rays": rays, "contribution": contribution, "sampled": sampled}


def render_megakernel_direct(orc, flat, camera, w, h, iter_begin, iter_count, max_bounces, prev=None, scene_handle=None, record=None):
    """-> dict(color, normal, depth, rays, diffuse_hits, shadow_rays, unoccluded).  record: a list that gets one dict per
    (iteration, bounce) with the diffuse hits' pixels, points, normals and the light sample drawn there."""
    sh = scene_handle or orc.SceneHandle(flat)
    materials = np.asarray(flat.materials)
    table = dr.light_table(flat)
    lit = len(table[0]) > 0 and float(table[1]["total_weight"]) > 0.0
    P = w * h
    if prev is None:
        fc, fn, fd = np.zeros((P, 3), np.float32), np.zeros((P, 3), np.float32), np.zeros(P, np.float32)
    else:
        fc = np.array(prev["color"], dtype=np.float32).reshape(P, 3)
        fn = np.array(prev["normal"], dtype=np.float32).reshape(P, 3)
        fd = np.array(prev["depth"], dtype=np.float32).reshape(P)
    rays = diffuse_hits = shadow_rays = unoccluded = 0
    for it in range(iter_count):
        iteration = iter_begin + it
        o, d, tmin, states = lr._primary(orc, camera, w, h, np.arange(P), iteration)
        draws = lr.Draws(orc, states)
        color = np.ones((P, 3), dtype=np.float32)
        radiance = np.zeros((P, 3), dtype=np.float32)
        count_emission = np.ones(P, dtype=bool)
        normal = -d
        depth = np.full(P, F(1e6), dtype=np.float32)
        active = np.arange(P)
        for b in range(max_bounces):
            if len(active) == 0:
                break
            rays += len(active)
            recs_a, hit_a = orc.intersect_rays(flat, lr._rays(o[active], tmin[active], d[active]), scene_handle=sh)
            recs = np.zeros(P, dtype=recs_a.dtype)
            recs[active] = recs_a
            hit = np.zeros(P, dtype=bool)
            hit[active] = hit_a.astype(bool)
            miss = active[~hit[active]]
            color[miss] = color[miss] * lr.sky(d[miss])
            hi = active[hit[active]]
            if b == 0:
                depth[hi] = recs["t"][hi]
                normal[hi] = recs["normal"][hi]
            mt = materials["type"][recs["material_id"][hi].astype(np.int64)]
            em = hi[mt == EMISSIVE]
            emitted = color[em] * materials["p"][recs["material_id"][em].astype(np.int64), :3].astype(np.float32)
            color[em] = np.where(count_emission[em][:, None], emitted, F(0.0)) if lit else emitted
            sc = hi[mt != EMISSIVE]
            lr.shade(orc, materials, o, d, tmin, recs, sc, draws, color)
            if lit:
                mt_sc = mt[mt != EMISSIVE]
                count_emission[sc] = mt_sc != 0
                df = sc[mt_sc == 0]
                diffuse_hits += len(df)
                pts = recs["point"][df].astype(np.float32)
                nrm = recs["normal"][df].astype(np.float32)
                smp = light_sample(orc, flat, table, pts, nrm, light_draws(orc, df, iteration, b))
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
                    record.append({"iteration": iteration, "bounce": b, "pixels": df, "points": pts, "normals": nrm, "sample": smp,
                                   "clear": clear})
            active = sc
        total = radiance + color if lit else color   # (no lamp table: the plain kernel deposits colour itself)
        for fb, val in ((fc, total), (fn, normal)):
            for k in range(3):
                col = fb[:, k].copy()
                lr._fold(col, np.arange(P), iteration, val[:, k])
                fb[:, k] = col
        lr._fold(fd, np.arange(P), iteration, depth)
    return {"color": fc.reshape(h, w, 3), "normal": fn.reshape(h, w, 3), "depth": fd.reshape(h, w), "rays": rays,
            "diffuse_hits": diffuse_hits, "shadow_rays": shadow_rays, "unoccluded": unoccluded}


# ---- scenes the CPU and GPU tests share ----------------------------------------------------------------------------------
def glass_lamp_scene(pkg):
    """A sphere lamp inside a glass sphere, over a floor with a diffuse ball: every segment from a diffuse surface to a point of
    the lamp crosses the glass, so every shadow ray is blocked and the lamp's light arrives only by paths that end on it after a
    dielectric vertex (or straight from the camera) -- the emission the gate must keep."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.add_material("floor", pkg.DiffuseMateral((0.7, 0.7, 0.7)))
    s.add_material("ball", pkg.DiffuseMateral((0.2, 0.5, 0.3)))
    s.add_material("glass", pkg.DielectricMaterial(1.5))
    s.add_material("lamp", pkg.EmissiveMaterial((5.0, 4.0, 3.0)))
    s.add_object(pkg.Sphere((0, 0, 0), 1000.0), glm.translate((0.0, -1001.0, 0.0)), "floor")
    s.add_object(pkg.Sphere((0, 0, 0), 0.4), glm.translate((-1.0, -0.6, -0.8)), "ball")
    s.add_object(pkg.Sphere((0, 0, 0), 0.45), glm.translate((0.2, 0.1, -1.0)), "glass")
    s.add_object(pkg.Sphere((0, 0, 0), 0.2), glm.translate((0.2, 0.1, -1.0)), "lamp")
    s.camera = pkg.scenes._camera_from_look_at((0.0, 0.4, 3.0), (0.0, -0.1, -1.0), vfov_deg=45.0)
    return s


def metal_glass_scene(pkg):
    """A panel lamp (a mesh) over a floor, with a metal and a glass ball hanging between the two: shadow rays blocked by either,
    lamp hits after a metal and after a dielectric vertex (counted) and after a diffuse one (not counted)."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.add_material("floor", pkg.DiffuseMateral((0.7, 0.7, 0.7)))
    s.add_material("mirror", pkg.MetalMaterial((0.9, 0.8, 0.7), 0.05))
    s.add_material("glass", pkg.DielectricMaterial(1.5))
    s.add_material("panel", pkg.EmissiveMaterial((6.0, 6.0, 5.5)))
    s.add_object(pkg.Sphere((0, 0, 0), 1000.0), glm.translate((0.0, -1001.0, 0.0)), "floor")
    s.add_object(pkg.Sphere((0, 0, 0), 0.35), glm.translate((-0.35, 0.3, -0.9)), "mirror")
    s.add_object(pkg.Sphere((0, 0, 0), 0.35), glm.translate((0.45, 0.3, -0.7)), "glass")
    s.add_object(s.add_mesh("models/light_panel.obj", pkg.scenes.light_panel_mesh()), glm.identity(), "panel")
    s.camera = pkg.scenes._camera_from_look_at((0.0, 0.6, 3.2), (0.0, 0.1, -0.8), vfov_deg=45.0)
    return s


# The statistical test's room is CLOSED (no path leaves: a plain path ends on the lamp or at the cap), its walls have albedo 0.5, and
# one small sphere lamp hangs under the ceiling.  With direct lighting the diffuse hit at the LAST bounce still draws a light sample,
# a term the plain render (capped there) does not have: its share is below albedo^bounces = 0.5^24 = 6e-8 of the image at
# STAT_BOUNCES bounces, far below what the test resolves.
STAT_BOUNCES = 24


def small_lamp_room(pkg):
    """The closed room as ONE MESH (a box of 12 triangles).  The walls are triangles on purpose: the rule's shadow ray starts AT the
    hit point with t_min 1e-4 (section 5f's epsilons), and a triangle's own test gives t = 0 to within a few ulp of the coordinates
    (~1e-6 here) for a ray that starts in its plane, so no shadow ray is blocked by the wall it starts on.  The stock scenes' walls --
    spheres of radius 1000 -- do not have that property in binary32: c = |o - centre|^2 - R^2 is known to ~0.1 there, the near root
    of the quadratic to ~1e-4 / cos, and 7 % of the shadow rays of small_lamp_sphere_room hit their own wall (measured on the CPU
    oracle: tools/direct_loop_ab.py prints that room's figures).  That is a property of the shadow epsilon on such geometry, not of
    the estimator this test is about."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    x0, x1, y0, y1, z0, z1 = -2.0, 2.0, -1.0, 1.5, -2.0, 4.5
    positions = np.array([[x, y, z] for x in (x0, x1) for y in (y0, y1) for z in (z0, z1)], dtype=np.float32)  # index = 4 ix + 2 iy + iz
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    indices = np.array([i for a, b, c, d in quads for i in (a, b, c, a, c, d)], dtype=np.uint32)
    s.add_material("walls", pkg.DiffuseMateral((0.5, 0.5, 0.5)))
    s.add_object(s.add_mesh("models/closed_room.obj", pkg.Mesh(positions, indices)), glm.identity(), "walls")
    s.add_material("lamp", pkg.EmissiveMaterial((12.0, 11.0, 9.0)))
    s.add_object(pkg.Sphere((0, 0, 0), 0.25), glm.translate((0.6, 1.0, -0.8)), "lamp")
    s.camera = pkg.scenes._camera_from_look_at((0.0, 0.0, 4.0), (0.0, -0.1, 0.0), vfov_deg=45.0)
    return s


def small_lamp_sphere_room(pkg):
    """The same room from six wall spheres of radius 1000 (the stock scenes' walls): NOT the statistical test's scene, see
    small_lamp_room; kept so that the self-shadowing it shows stays measurable."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    big = 1000.0
    for name, rgb, at in (("floor", (0.5, 0.5, 0.5), (0.0, -big - 1.0, 0.0)), ("ceiling", (0.5, 0.5, 0.5), (0.0, big + 1.5, 0.0)),
                          ("back", (0.5, 0.5, 0.5), (0.0, 0.0, -big - 2.0)), ("front", (0.5, 0.5, 0.5), (0.0, 0.0, big + 4.5)),
                          ("left", (0.5, 0.1, 0.1), (-big - 2.0, 0.0, 0.0)), ("right", (0.1, 0.4, 0.15), (big + 2.0, 0.0, 0.0))):
        s.add_material(name, pkg.DiffuseMateral(rgb))
        s.add_object(pkg.Sphere((0, 0, 0), big), glm.translate(at), name)
    s.add_material("lamp", pkg.EmissiveMaterial((12.0, 11.0, 9.0)))
    s.add_object(pkg.Sphere((0, 0, 0), 0.25), glm.translate((0.6, 1.0, -0.8)), "lamp")
    s.camera = pkg.scenes._camera_from_look_at((0.0, 0.0, 4.0), (0.0, -0.1, 0.0), vfov_deg=45.0)
    return s
