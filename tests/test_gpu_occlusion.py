"""Occlusion queries on the GPU (ptc_occluded_rays: k_occlude_spheres + k_occlude4) against the CPU
oracle: occluded[i] == the oracle's hit flag of ray_scene_intersection_test, on EVERY ray -- no tolerances, no rays left
out.  Scenes: a room with two mesh instances, the 1,000,000-triangle heightfield with adversarial rays, coincident
instances with t_max at / one ulp below the hit, several meshes, lamps, spheres at the edges of the sphere arithmetic;
every schedule parameter the any-hit walk honours; the rays outside its fast domain; sizes; no side effects on a
running accumulation; agreement with the library's own closest hit on 1,000,000 rays.  And what the three query calls share
on the host (ptc_intersect_rays, ptc_occluded_rays, ptc_direct_light): the closest-hit call's sizes on both of its paths, the
order of the refusals, a working context after a refused call."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import direct_ref as D
import occlusion_rays as R
from test_gpu_schedules import _adversarial_rays

pytestmark = pytest.mark.gpu
FMAX = np.finfo(np.float32).max


def _occluded(pkg, flat, rays, params=(), variant=None, size=(32, 32)):
    with pkg.PathTracer() as pt:
        for k, v in params:
            pt.set_param(k, v)
        pt.create_buffers(size, flat)
        if variant is not None:
            pt.set_trace_variant(variant)
        occ = pt.occluded_rays(rays)
        st = pt.occlusion_stats()
    assert occ.dtype == np.uint8 and occ.shape == (len(rays),) and set(np.unique(occ)) <= {0, 1}
    assert st["rays"] == len(rays) and st["occluded"] == int(occ.sum())
    return occ, st


def _oracle(orc, flat, rays):
    _, hit = orc.intersect_rays(flat, rays)
    return hit.astype(np.uint8)


@pytest.fixture(scope="module")
def room(pkg, orc):
    scene = R.occlusion_scene(pkg)
    flat = scene.build_scene()
    rays = R.shadow_rays()
    return flat, rays, _oracle(orc, flat, rays)


@pytest.fixture(scope="module")
def big(pkg, orc):
    scene = pkg.scenes.heightfield_scene((1920, 1080))
    flat = scene.build_scene()
    flat.bvh, _ = pkg.bvh_from_mesh(list(scene.mesh_map_.values())[0])
    rng = np.random.default_rng(7)
    n = 20000
    o = np.stack([rng.uniform(-4.5, 4.5, n), rng.uniform(0.05, 3.0, n), rng.uniform(-2.5, 2.5, n)], axis=1)
    target = np.stack([rng.uniform(-4, 4, n), rng.uniform(-0.2, 0.9, n), rng.uniform(-2, 2, n)], axis=1)
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 1e-4, d, FMAX
    rays = np.concatenate([rays, _adversarial_rays(flat, flat.bvh, rng)], axis=0)
    return flat, rays, _oracle(orc, flat, rays)


def test_room_with_instances_against_oracle(pkg, room):
    """1: the helper's scene and its 60,000 shadow-style rays (wall spheres, two mesh instances, a small and a scaled sphere)."""
    flat, rays, want = room
    assert len(rays) == 60000 and 0.2 < want.mean() < 0.8
    occ, st = _occluded(pkg, flat, rays)
    assert np.array_equal(occ, want), np.nonzero(occ != want)[0][:10]
    assert st["launches"] == 3 and st["kernel_ms"] == 0.0   # one sphere launch, one launch per instance; timing is off


def test_benchmark_size_with_adversarial_rays(pkg, big):
    """2: 1,000,000 triangles, 20,000 random rays plus the adversarial ones of the closest-hit test (axis-parallel and subnormal
    directions, origins on box planes, rays through box corners, vertices and along edges).  The degenerate directions are
    set aside at fetch as in the closest-hit walk -- unless a sphere has flagged the ray first (the spheres run before the
    mesh here); the closest-hit test's bound on its own counter, more than 1000 rays redone, holds all the same."""
    flat, rays, want = big
    occ, st = _occluded(pkg, flat, rays)
    assert np.array_equal(occ, want), np.nonzero(occ != want)[0][:10]
    assert st["redone"] > 1000, st


def _ties_scene(pkg):
    # the scene of test_gpu_schedules.test_instance_ties_and_carried_hits: two coincident instances, a sphere in front
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.add_material("a", pkg.DiffuseMateral((0.8, 0.3, 0.3)))
    s.add_material("b", pkg.MetalMaterial((0.9, 0.9, 0.9), 0.1))
    s.add_material("c", pkg.DielectricMaterial(1.5))
    mesh = pkg.scenes.displaced_sphere_mesh(12, 24)
    s.add_mesh("m", mesh)
    s.add_object(mesh, glm.identity(), "a")
    s.add_object(pkg.Sphere((0, 0, 0), 0.3), glm.translate((0.0, 0.0, 1.6)), "c")
    s.add_object(mesh, glm.identity(), "b")
    return s


def test_ties_and_t_max_at_the_hit_distance(pkg, orc):
    """3: coincident instances; every ray again with t_max = the oracle's hit distance (t == t_max is accepted) and one ulp
    below it (the hit is gone unless something else lies in range)."""
    flat = _ties_scene(pkg).build_scene()
    rng = np.random.default_rng(3)
    n = 8000
    o = rng.normal(size=(n, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * 4.0
    d = rng.uniform(-0.6, 0.6, size=(n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 1e-4, d, FMAX
    rays[1::2, 3] = 1e-5
    recs, hit = orc.intersect_rays(flat, rays)
    m = hit.astype(bool)
    again, below = rays[m].copy(), rays[m].copy()
    again[:, 7] = recs["t"][m]
    below[:, 7] = np.nextafter(recs["t"][m], np.float32(0))
    rays = np.concatenate([rays, again, below], axis=0)
    want = _oracle(orc, flat, rays)
    assert want[n:n + len(again)].mean() > 0.9 and want[n + len(again):].mean() < 0.5   # the ulp does decide
    for variant in (3, 0, 1):
        occ, _ = _occluded(pkg, flat, rays, variant=variant)
        assert np.array_equal(occ, want), (variant, np.nonzero(occ != want)[0][:10])


@pytest.mark.parametrize("name", ["two_meshes", "three_meshes_ties"])
def test_several_meshes(pkg, orc, golden_dir, name):
    """4: the committed probe rays of tests/golden/multimesh.npz against a fresh oracle run (distinct meshes per scene)."""
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(golden_dir, "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    scene = mod.multimesh_scenes()[name][0]
    flat = scene.build_scene(distinct_meshes=True)
    golden = np.load(os.path.join(golden_dir, "multimesh.npz"))
    rays = golden[f"{name}_probe_rays"]
    want = _oracle(orc, flat, rays)
    assert np.array_equal(want, golden[f"{name}_probe_hit"]) and 0.1 < want.mean()
    # the probes again as shadow rays: t_max = 0.999 / 1 x the hit distance, both t_min values
    m = want.astype(bool)
    recs, _ = orc.intersect_rays(flat, rays)
    short, exact = rays[m].copy(), rays[m].copy()
    short[:, 7] = np.float32(0.999) * recs["t"][m]
    exact[:, 7] = recs["t"][m]
    exact[:, 3] = 1e-5
    more = np.concatenate([rays, short, exact], axis=0)
    fast = (more[:, 3] == np.float32(1e-4)) | (more[:, 3] == np.float32(1e-5))
    more = more[fast & (more[:, 7] >= 0)]   # (keeps the call on the any-hit kernels whatever the fixture's t_min values are)
    assert len(more) > len(rays) // 2
    want = _oracle(orc, flat, more)
    occ, st = _occluded(pkg, flat, more)
    assert np.array_equal(occ, want), np.nonzero(occ != want)[0][:10]
    occ0, _ = _occluded(pkg, flat, rays)     # and the fixture's rays exactly as committed
    assert np.array_equal(occ0, golden[f"{name}_probe_hit"])


def test_lamps_occlude(pkg, orc):
    """5: scenes.cornell_lit(with_mesh=True): rays from seeded points of the room towards points on both lamps, t_max 0.5 /
    0.999 / 1 / 2 x the distance.  An emissive surface occludes like any other; at factor 1 the lamp's own surface sits at
    t_max within rounding -- the case a renderer's shadow rays produce."""
    flat = pkg.scenes.cornell_lit(with_mesh=True).build_scene()
    rays, factors = R.lamp_rays()
    want = _oracle(orc, flat, rays)
    assert len(rays) == 40000 and 0.2 < want.mean() < 0.8, want.mean()
    by_factor = [float(want[factors == f].mean()) for f in (0.5, 0.999, 1.0, 2.0)]
    assert by_factor[0] < by_factor[1] < by_factor[2] < by_factor[3] == 1.0, by_factor
    occ, _ = _occluded(pkg, flat, rays)
    assert np.array_equal(occ, want), np.nonzero(occ != want)[0][:10]


def _far_spheres(pkg, shift, with_mesh):
    # the scene of test_gpu_spheres.test_small_spheres_far_from_the_origin
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    sx, sy, sz = shift
    s.add_material("white", pkg.DiffuseMateral((0.8, 0.8, 0.8)))
    s.add_material("red", pkg.DiffuseMateral((0.8, 0.2, 0.2)))
    s.add_material("mirror", pkg.MetalMaterial((0.9, 0.9, 0.9), 0.0))
    s.add_material("glass", pkg.DielectricMaterial(1.5))
    s.add_object(pkg.Sphere((0.3, 0.2, 0.1), 0.5), glm.translate(shift), "red")
    s.add_object(pkg.Sphere((-0.55, 0.25, 0.2), 0.35), glm.translate(shift), "glass")
    s.add_object(pkg.Sphere((0.31, 0.2, 0.1), 0.5), glm.translate(shift), "mirror")
    s.add_object(pkg.Sphere((0.0, 0.0, -1003.0), 1000.0), glm.translate(shift), "white")
    s.add_object(pkg.Sphere((0.0, -1000.4, 0.0), 1000.0), glm.translate(shift), "white")
    if with_mesh:
        mesh = pkg.scenes.heightfield_mesh(17, 9, 1.0, 0.5, seed=3)
        s.add_mesh("ground", mesh)
        s.add_object(mesh, glm.translate((sx, sy - 0.3, sz + 0.4)), "white")
    return s


@pytest.mark.parametrize("shift", [(1000.0, 800.0, -1200.0), (9000.0, -7000.0, 4000.0), (0.0, 0.0, 0.0)])
@pytest.mark.parametrize("with_mesh", [False, True])
def test_small_spheres_far_from_the_origin(pkg, orc, shift, with_mesh):
    """6a: spheres with their centre in the Sphere struct and a translation of 1e3 .. 1e4: rays from about a unit away, many
    of them grazing, with a finite t_max around the distance to the sphere they aim at."""
    flat = _far_spheres(pkg, shift, with_mesh).build_scene()
    rng = np.random.default_rng(41)
    n = 12000
    base = np.asarray(shift, dtype=np.float64)
    o = base + np.array([0.3, 0.25, 1.6]) + rng.uniform(-0.4, 0.4, size=(n, 3))
    centres = np.array([[0.3, 0.2, 0.1], [-0.55, 0.25, 0.2], [0.31, 0.2, 0.1], [0.0, 0.05, 0.4]])
    radii = np.array([0.5, 0.35, 0.5, 0.3])
    k = np.arange(n) % 4
    v = rng.normal(size=(n, 3))
    target = base + centres[k] + (radii[k] * rng.uniform(0.9, 1.1, n))[:, None] * v / np.linalg.norm(v, axis=1)[:, None]
    rays, _ = R.towards_points(o, target, (0.9, 1.0, 1.1, 3.0, 1e30), 42)
    want = _oracle(orc, flat, rays)
    assert 0.2 < want.mean() < 0.98, want.mean()
    occ, _ = _occluded(pkg, flat, rays)
    assert np.array_equal(occ, want), np.nonzero(occ != want)[0][:10]


def test_signed_zeros_and_spheres_in_front_of_a_mesh(pkg, orc):
    """6b: the rays of test_gpu_spheres.test_rays_on_the_exceptions_of_the_fold (origins and directions with +0 / -0
    components, origins on a sphere's centre planes, on a wall, at a sphere's centre; huge and small t_max) in the room of
    wall spheres in front of a mesh, with a sphere run that ends the list."""
    from test_gpu_spheres import _soup
    flat = _soup(pkg, "room_mesh").build_scene()
    rng = np.random.default_rng(7)
    n = 16384
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0:3] = rng.uniform(-1.8, 1.8, size=(n, 3)).astype(np.float32)
    rays[:, 1] = rng.uniform(-0.9, 2.3, size=n)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 3] = np.where(rng.uniform(size=n) < 0.5, 1e-4, 1e-5)
    rays[:, 7] = np.where(rng.uniform(size=n) < 0.3, FMAX, rng.uniform(0.05, 3.0, size=n))
    k = np.arange(n)
    for axis in range(3):
        rays[k % 7 == axis, axis] = 0.0
        rays[k % 7 == axis + 3, axis] = -0.0
        rays[k % 11 == axis, 4 + axis] = 0.0
        rays[k % 11 == axis + 3, 4 + axis] = -0.0
    rays[k % 13 == 0, 0:3] = np.float32([-1.0, -0.6, 0.2]) + np.float32([0.0, 0.0, 1.5])
    rays[k % 13 == 0, 4:7] = np.float32([0.0, 0.0, -1.0])
    rays[k % 17 == 0, 1] = -1.0
    rays[k % 19 == 0, 0:3] = np.float32([0.9, -0.5, 0.3])
    want = _oracle(orc, flat, rays)
    assert 0.2 < want.mean() < 0.98, want.mean()
    occ, _ = _occluded(pkg, flat, rays)
    assert np.array_equal(occ, want), np.nonzero(occ != want)[0][:10]


SCHEDULES = [("variant 3", (), 3), ("variant 0", (), 0), ("variant 1", (), 1),
             ("force_slow 1", (("debug_force_slow", 1),), None), ("force_slow 2", (("debug_force_slow", 2),), None),
             ("lds 4", (("debug_lds_entries", 4),), None), ("waves 8", (("traverse_waves", 8),), None),
             ("refill 20", (("refill_lanes", 20),), None), ("refill 48", (("refill_lanes", 48),), None),
             ("static 0", (("static_eighths", 0),), None), ("static 7", (("static_eighths", 7),), None)]


@pytest.mark.parametrize("which", ["room", "big"])
@pytest.mark.parametrize("label,params,variant", SCHEDULES, ids=[s[0].replace(" ", "_") for s in SCHEDULES])
def test_schedules(pkg, room, big, which, label, params, variant):
    """7: the cross-check variants, both forms of the forced exact redo, the stack overflow path, few wavefronts, the refill
    threshold and the static share of the ray feed, on the scenes of 1 and 2: the same bytes."""
    flat, rays, want = room if which == "room" else big
    occ, st = _occluded(pkg, flat, rays, params=params, variant=variant)
    assert np.array_equal(occ, want), (label, np.nonzero(occ != want)[0][:10])
    if label == "force_slow 1":
        # every ray the spheres left open was set aside when fetched, for every mesh object
        assert st["redone"] >= int((want == 0).sum())


def test_rays_outside_the_fast_domain(pkg, orc, room):
    """8: another t_min, a negative t_max, a NaN t_max -- each alone and mixed with ordinary rays -- take the exact closest-hit
    kernel and still equal the oracle's flag."""
    flat, rays, _ = room
    base = rays[:6000]
    other_tmin = base.copy()
    other_tmin[:, 3] = 0.25
    neg = base.copy()
    neg[:, 7] = -np.abs(neg[:, 7])
    nan = base.copy()
    nan[:, 7] = np.nan
    mixed = base.copy()
    mixed[0::4, 3] = 0.25
    mixed[1::4, 7] = -1.0
    mixed[2::4, 7] = np.nan
    with pkg.PathTracer() as pt:
        pt.create_buffers((32, 32), flat)
        for name, q in (("t_min 0.25", other_tmin), ("negative t_max", neg), ("NaN t_max", nan), ("mixed", mixed)):
            want = _oracle(orc, flat, q)
            occ = pt.occluded_rays(q)
            assert np.array_equal(occ, want), (name, np.nonzero(occ != want)[0][:10])
        assert pt.occlusion_stats()["redone"] == 0   # none of these calls ran the any-hit kernels
    assert 0.0 < _oracle(orc, flat, other_tmin).mean() < 1.0


def test_sizes(pkg, orc, room):
    """9: n = 0, 1, 63, 65 and 100,003 (no multiple of a wavefront, of a feed batch or of a sphere workgroup)."""
    flat, rays, _ = room
    many = np.concatenate([rays, R.shadow_rays(n=40003, seed=12)], axis=0)
    assert len(many) == 100003
    want = _oracle(orc, flat, many)
    with pkg.PathTracer() as pt:
        pt.create_buffers((32, 32), flat)
        empty = pt.occluded_rays(np.zeros((0, 8), dtype=np.float32))
        assert empty.shape == (0,) and pt.occlusion_stats()["rays"] == 0
        for n in (1, 63, 65, 100003):
            occ = pt.occluded_rays(many[:n])
            assert np.array_equal(occ, want[:n]), (n, np.nonzero(occ != want[:n])[0][:10])
        # a single occluded ray, a single free one
        i1, i0 = int(np.nonzero(want == 1)[0][0]), int(np.nonzero(want == 0)[0][0])
        assert pt.occluded_rays(many[i1:i1 + 1])[0] == 1 and pt.occluded_rays(many[i0:i0 + 1])[0] == 0
        st = pt.occlusion_stats()
        assert st["rays"] == 1 + 63 + 65 + 100003 + 2


def test_no_side_effects_on_a_running_accumulation(pkg, room):
    """10: three accumulated iterations with a query between them: frames, stats() and the counting fields of profile() equal
    those of the same run without the query (both runs look at stats() at the same points, so their batches are the same)."""
    scene = R.occlusion_scene(pkg, n_lat=24, n_lon=48)
    flat = scene.build_scene()
    _, rays, _ = room

    def run(query):
        with pkg.PathTracer(max_bounces=6) as pt:
            pt.create_buffers((96, 64), flat)
            pt.max_iterations = 3
            pt.reset_profile()
            for i in range(3):
                pt.path_trace(scene.camera)
                pt.stats()
                if query and i < 2:
                    assert pt.occluded_rays(rays[:5000]).shape == (5000,)
            out = {k: pt.download(k) for k in ("color", "normal", "depth")}
            prof = {k: v for k, v in pt.profile().items() if not k.endswith("_ms")}
            return out, pt.stats(), prof, pt.occlusion_stats()

    a, sa, pa, oa = run(False)
    b, sb, pb, ob = run(True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert sa == sb and pa == pb
    assert oa["rays"] == 0 and ob["rays"] == 10000 and ob["launches"] > 0


def test_agrees_with_the_closest_hit_on_a_million_rays(pkg):
    """11: occluded == (intersect_rays(...)[0] >= 0) on 1,000,000 rays of the measurement tool's generator (500,000 shadow rays
    towards a light above the 1,000,000-triangle terrain, 500,000 cosine-spread ones from the same origins); the oracle is
    too slow for this size.  With timing on, kernel_ms is filled."""
    scene = pkg.scenes.heightfield_scene((1920, 1080))
    flat = scene.build_scene()
    flat.bvh, _ = pkg.bvh_from_mesh(list(scene.mesh_map_.values())[0])
    shadow, spread = R.terrain_rays(pkg, 500000)
    rays = np.concatenate([shadow, spread], axis=0)
    with pkg.PathTracer() as pt:
        pt.create_buffers((64, 64), flat)
        pt.set_profiling(True, False)
        occ = pt.occluded_rays(rays)
        st = pt.occlusion_stats()
        t = pt.intersect_rays(rays)[0]
    want = (t >= 0).astype(np.uint8)
    assert np.array_equal(occ, want), np.nonzero(occ != want)[0][:10]
    assert 0.02 < want[:500000].mean() < 0.98 and 0.02 < want[500000:].mean() < 0.98
    assert st["kernel_ms"] > 0.0 and st["launches"] == 2


def _same_hits(got, recs, hit):
    """The per-ray comparison of tests/test_gpu_parity.py: hit / miss, then t, normal, material and side of every hit, bit for bit."""
    t, nrm, mat, side = got
    m = hit.astype(bool)
    assert t.shape == m.shape and nrm.shape == (len(m), 3) and mat.shape == m.shape and side.shape == m.shape
    assert np.array_equal(t >= 0, m)
    assert t[m].tobytes() == recs["t"][m].tobytes() and nrm[m].tobytes() == recs["normal"][m].tobytes()
    assert np.array_equal(mat[m], recs["material_id"][m].astype(np.uint32)) and np.array_equal(side[m], recs["side"][m])
    assert np.all(t[~m] == -1.0) and not mat[~m].any() and not side[~m].any()


@pytest.mark.parametrize("kind", ["path_like", "exact", "force_slow"])
def test_closest_hit_sizes(pkg, orc, kind):
    """12: ptc_intersect_rays with n = 0, 1, 63, 64, 65 and 257 on the small room (spheres in front of a mesh launch, two instances,
    a sphere run that ends the list) against the oracle's records.  path_like: the rays as generated, through the traversal
    launches; exact: the call's last ray with t_min 0.25, which sends the whole call to the exact kernel; force_slow: the first
    set with every ray handed to the exact redo, which profile()'s slow_rays count."""
    flat = R.occlusion_scene(pkg, n_lat=24, n_lon=48).build_scene()
    rays = R.shadow_rays(n=257, seed=12)
    sh = orc.SceneHandle(flat)
    with pkg.PathTracer() as pt:
        if kind == "force_slow":
            pt.set_param("debug_force_slow", 1)
        pt.create_buffers((32, 32), flat)
        slow_before = sum(pt.profile()["slow_rays"])
        for n in (0, 1, 63, 64, 65, 257):
            q = rays[:n].copy()
            if kind == "exact" and n:
                q[-1, 3] = 0.25
            recs, hit = orc.intersect_rays(flat, q, scene_handle=sh)
            got = pt.intersect_rays(q)
            assert [len(a) for a in got] == [n] * 4
            _same_hits(got, recs, hit)
            if n == 257:
                assert 0.2 < hit.mean() < 1.0
        slow = sum(pt.profile()["slow_rays"]) - slow_before
        print(kind, "rays redone exactly:", slow)
        if kind != "path_like":
            assert slow > 0 if kind == "force_slow" else slow == 0    # (the exact kernel sets no ray aside)


@pytest.fixture(scope="module")
def lit(pkg, orc):
    """One lit scene for the three calls: 64 rays with the oracle's records, 64 points with the restatement's answer."""
    flat = pkg.scenes.cornell_lit((64, 64), with_mesh=True).build_scene()
    rays, _ = R.lamp_rays(n=64, seed=23)
    pts, nrm = D.room_points(64, seed=17, lamp_points=D.cornell_lamp_points())
    return flat, rays, orc.intersect_rays(flat, rays), pts, nrm, D.query(orc, flat, pts, nrm, 3)


@pytest.mark.parametrize("which", ["intersect", "occluded", "direct_light"])
def test_refusals_and_the_context_after_them(pkg, lit, which):
    """13: the order of the checks the three calls open with -- no scene (PTC_ERR_NO_SCENE, "no scene uploaded"), a NULL context,
    a NULL output with n = 1 (PTC_ERR_INVALID; ptc_direct_light names the arrays), ptc_direct_light's n = 0 with nothing else
    -- and straight after every refusal a valid query with the oracle's answer."""
    flat, rays, (recs, hit), pts, nrm, (want_rad, want_rays, want_vis, _) = lit
    L, K = pkg.lib(), pkg._capi
    fp, n = C.POINTER(C.c_float), 1
    t, nr = np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    mat, side, occ, rad = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros((n, 3), np.float32)

    def call(ctx, null_output=False):
        if which == "intersect":
            return L.ptc_intersect_rays(ctx, rays.ctypes.data_as(fp), n, t.ctypes.data_as(fp), nr.ctypes.data_as(fp),
                                        mat.ctypes.data_as(C.POINTER(C.c_uint32)), None if null_output else side.ctypes.data_as(C.POINTER(C.c_uint8)))
        if which == "occluded":
            return L.ptc_occluded_rays(ctx, rays.ctypes.data_as(fp), n, None if null_output else occ.ctypes.data_as(C.POINTER(C.c_uint8)))
        return L.ptc_direct_light(ctx, pts.ctypes.data, nrm.ctypes.data, n, 3, None if null_output else rad.ctypes.data, None, None, 0)

    def valid(pt):
        if which == "intersect":
            _same_hits(pt.intersect_rays(rays), recs, hit)
        elif which == "occluded":
            assert np.array_equal(pt.occluded_rays(rays), hit.astype(np.uint8))
        else:
            radiance, shadow, visible = pt.direct_light(pts, nrm, 3, want_rays=True)
            assert shadow.tobytes() == want_rays.tobytes() and np.array_equal(visible, want_vis) and radiance.tobytes() == want_rad.tobytes()

    assert 0 < hit.sum() < len(hit) and 0 < want_vis.sum() < len(want_vis)
    with pkg.PathTracer() as pt:
        assert call(pt._ctx) == K.PTC_ERR_NO_SCENE and L.ptc_last_error(pt._ctx) == b"no scene uploaded"
        assert call(None) == K.PTC_ERR_INVALID
        pt.create_buffers((32, 32), flat)
        valid(pt)
        assert call(None) == K.PTC_ERR_INVALID
        valid(pt)
        assert call(pt._ctx, null_output=True) == K.PTC_ERR_INVALID
        if which == "direct_light":
            assert L.ptc_last_error(pt._ctx) == b"points, normals or radiance is NULL"
        valid(pt)
        assert call(pt._ctx) == K.PTC_OK
        if which == "direct_light":
            assert L.ptc_direct_light(pt._ctx, None, None, 0, 0, None, None, None, 0) == K.PTC_OK
            valid(pt)
