"""The lamp sampler at its limits on the GPU: ptc_direct_light against the numpy restatement (tests/direct_ref.py)
bit for bit in rays, visibility and radiance -- on the inputs of the float64 classes (tests/light_f64.py: far scenes, extreme sizes,
points in a lamp's plane, on it and inside it, distant lamps), on points whose first draw is constructed to be the first and the last
state each lamp of a hostile table owns, through a 2^17-triangle emitter (17 search steps), at sizes around a block, and through the
other trace paths; then one small frame of a scene with the (1, 1e-8, 1) table through each megakernel unit that compiles the sampler in,
against the loop restatements.  What the restatement is worth is settled without a GPU (tests/test_light_limits_cpu.py)."""
import numpy as np
import pytest

import direct_ref as D
import light_census as LC
import light_f64 as L64
import loop_ref
import seed_cases as sc
import smooth_ref

pytestmark = pytest.mark.gpu
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_call(got, want, what):
    """(radiance, rays, visible) of ptc_direct_light against D.query's (radiance, rays, visible, sampled)"""
    radiance, rays, visible = got
    want_rad, want_rays, want_vis, want_sampled = want
    assert rays.shape == want_rays.shape and np.array_equal(_bits(rays), _bits(want_rays)), (
        what, np.nonzero(np.any(_bits(rays) != _bits(want_rays), axis=1))[0][:10])
    assert np.array_equal(visible, want_vis), (what, np.nonzero(visible != want_vis)[0][:10])
    assert np.array_equal(_bits(radiance), _bits(want_rad)), (what, np.nonzero(np.any(_bits(radiance) != _bits(want_rad), axis=1))[0][:10])
    assert np.array_equal(rays[:, 7] > 0, want_sampled), what


def _classes(pkg):
    if "classes" not in _cache:
        _cache["classes"] = L64.classes(pkg)
    return _cache["classes"]


@pytest.mark.parametrize("name", list(L64.TOLERANCE))
def test_class_inputs(pkg, orc, name):
    """The points and normals of every case of the class against its lamps, the draws from the query's own streams (sample index 7).
    edge_draws is one scene nine times over: its first case stands for it here (the draws at the edges are what seed_cases places)."""
    cases = _classes(pkg)[name][:1] if name == "edge_draws" else _classes(pkg)[name]
    sampled = visible_any = 0
    for k, case in enumerate(cases):
        flat, p, nrm = case["flat"], case["p"], case["nrm"]
        want = D.query(orc, flat, p, nrm, 7)
        with pkg.PathTracer() as pt:
            pt.create_buffers((32, 32), flat)
            got = pt.direct_light(p, nrm, 7, want_rays=True)
        _same_call(got, want, (name, k))
        sampled, visible_any = sampled + int(want[3].sum()), visible_any + int(want[2].sum())
    if name == "distant":
        c = cases[0]
        lamp = D.sample(orc, c["flat"], c["p"], c["nrm"], 7)["lamp"]
        assert (lamp < 2).mean() > 0.9 and not want[3][lamp < 2].any()   # the lamps 1e20 away: d2 overflows, culled with a zero direction
    elif name == "inside":
        # the lamp is a sphere under scale 2: ray_object takes a sphere's t in OBJECT space against the world t_max (the reference's
        # rule), here t = d / 2 <= 0.999 d, so the lamp shadows every sample of itself -- library and restatement alike
        assert sampled > 0 and visible_any == 0
    else:
        assert sampled > 0 and visible_any > 0


# ---- hostile tables as scenes: lamps far enough apart that a ray's direction names its lamp ----------------------------------------
def _hostile(pkg, name):
    """-> (flat, the middle of every lamp, weights).  Live lamps are 7.5 or more apart, and no point of one is 2.2 from its middle."""
    if name not in _cache:
        ring = [(-8, 4, 0), (8, 4, 0), (0, 4, -8), (0, 4, 8), (-6, 4, -6), (6, 4, 6), (-6, 4, 6), (6, 4, -6), (0, 8, 0), (-8, 0, 0), (8, 0, 0)]
        if name == "one_tiny_one":
            lamps = [("mesh", 1.0, [1.0, 1e-8, 1.0], [ring[0], (0, 0, 0), ring[1]])]
        elif name == "one_tinier":
            lamps = [("mesh", 1.0, [1.0, 1e-9], [ring[0], (0, 0, 0)])]
        else:   # dark and zero-area lamps first, in the middle, last and in runs, around live ones of very different weight
            lamps = [("mesh", 0.0, [1.0], [ring[2]]), ("mesh", 2.0, [0.0, 0.0, 0.5, 0.0, 1e-7, 3.0, 0.0], [ring[3], ring[3], ring[4], ring[5], (0, 0, 0), ring[6], ring[7]]),
                     ("sphere", 0.0, 0.5, ring[8]), ("sphere", 3.0, 0.25, ring[9]), ("mesh", 0.0, [1.0], [ring[10]])]
        flat = LC.table_scene(pkg, lamps, floor=False).build_scene(distinct_meshes=True)
        recs, _, weights, _ = D.light_table(flat)
        assert np.array_equal(weights, LC.flat_weights(flat))
        middle = recs["p0"].astype(np.float64) + (recs["e1"].astype(np.float64) + recs["e2"]) / 3.0   # centroid; a sphere's centre
        middle[(recs["kind_material"] >> 31) != 0] = recs["p0"][(recs["kind_material"] >> 31) != 0]
        _cache[name] = (flat, middle, weights)
    return _cache[name]


def _cloud(n, seed):
    rng = np.random.default_rng(seed)
    p = np.array([0.0, -3.0, 0.0]) + rng.uniform(-0.25, 0.25, (n, 3))
    nrm = np.array([0.0, 1.0, 0.0]) + 0.2 * rng.normal(size=(n, 3))
    return p.astype(np.float32), (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("name", ["one_tiny_one", "one_tinier", "dead_lamps"])
def test_first_and_last_owning_states(pkg, orc, name):
    """Per lamp of weight > 0 a (point index, sample index) pair whose first draw is the first state the lamp owns, and one for the
    last; and pairs for states 1 and 2^31 - 2.  Every call: all 256 points against the restatement, bit for bit; the placed point's ray
    points at the lamp that owns the state."""
    flat, middle, weights = _hostile(pkg, name)
    t = np.concatenate([[0], D.thresholds(weights).astype(np.int64)])
    live = np.nonzero(weights > 0.0)[0]
    want_states = [(1, live[0]), (LC.N, live[-1])]
    for k in live:
        assert t[k + 1] > t[k]
        want_states += [(int(t[k]) + 1, k), (int(t[k + 1]), k)]   # v = n + 1 for n = T_(k-1) and n = T_k - 1
    p, nrm = _cloud(256, seed=3)
    points = list(range(3, 256, 5))
    sh = orc.SceneHandle(flat)
    table = D.light_table(flat)
    with pkg.PathTracer() as pt:
        pt.create_buffers((32, 32), flat)
        for j, (v, k) in enumerate(want_states):
            index, si, _ = sc.place(sc.seeds_for_draw(v, 1), points[j % len(points):] + points[:j % len(points)], xor=sc.XOR_LIGHT, limit=2 ** 32)
            ref = D.sample(orc, flat, p, nrm, si, table=table)
            assert D.light_draws(orc, [index], si, 0)[0][0] == v and ref["lamp"][index] == k, (name, v, k)
            got = pt.direct_light(p, nrm, si, want_rays=True)
            _same_call(got, D.query(orc, flat, p, nrm, si, table=table, scene_handle=sh), (name, v, k))
            assert ref["sampled"][index], (name, v, k)     # (the cloud looks up at every lamp)
            ray = got[1][index].astype(np.float64)
            q = ray[0:3] + ray[4:7] * (ray[7] / float(np.float32(0.999)))   # where the ray ends: on lamp k, far from every other
            away = np.linalg.norm(middle - q, axis=1)
            others = [j for j in live if j != k]
            assert away[k] < 2.5 and np.all(away[others] > 5.0), (name, v, k, away.tolist())


def test_sizes(pkg, orc):
    """0, 1, 63, 64, 65 and 4,097 points against the (1, 1e-8, 1) table."""
    flat, _, _ = _hostile(pkg, "one_tiny_one")
    p, nrm = _cloud(4097, seed=9)
    want = D.query(orc, flat, p, nrm, 5)
    with pkg.PathTracer() as pt:
        pt.create_buffers((32, 32), flat)
        for n in (0, 1, 63, 64, 65, 4097):
            got = pt.direct_light(p[:n], nrm[:n], 5, want_rays=True)
            _same_call(got, tuple(a[:n] for a in want), n)
    assert want[3].mean() > 0.9 and want[2].mean() > 0.9


def test_search_depth(pkg, orc):
    """A 2^17-triangle emitter (the heightfield mesh at 257 x 257) above a floor: the threshold search runs 17 steps."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.add_material("floor", pkg.DiffuseMateral((0.7, 0.7, 0.7)))
    s.add_material("glow", pkg.EmissiveMaterial((0.5, 0.6, 0.7)))
    s.add_object(pkg.Sphere((0, 0, 0), 1000.0), glm.translate((0.0, -1001.0, 0.0)), "floor")
    s.add_object(s.add_mesh("models/heightfield.obj", pkg.scenes.heightfield_mesh(257, 257, 3.0, 1.5, seed=7)), glm.translate((0.0, 1.2, -0.5)), "glow")
    flat = s.build_scene()
    rng = np.random.default_rng(5)
    n = 2000
    pts = np.stack([rng.uniform(-1.9, 1.9, n), rng.uniform(-1.0, 0.9, n), rng.uniform(-1.6, 0.9, n)], axis=1).astype(np.float32)
    nrm = rng.normal(size=(n, 3)) + np.array([0.0, 1.5, 0.0])
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    table = D.light_table(flat)
    assert table[1]["lights"] == 2 ** 17 and len(np.unique(D.thresholds(table[2]))) == 2 ** 17
    want = D.query(orc, flat, pts, nrm, 2, table=table)
    with pkg.PathTracer() as pt:
        pt.create_buffers((32, 32), flat)
        got = pt.direct_light(pts, nrm, 2, want_rays=True)
        assert pt.light_info() == table[1]
    _same_call(got, want, "2^17 triangles")
    assert len(np.unique(D.sample(orc, flat, pts, nrm, 2, table=table)["lamp"])) > 1900 and want[3].mean() > 0.3 and want[2].mean() > 0.2


@pytest.mark.parametrize("label,params,variant", [("variant 0", (), 0), ("variant 1", (), 1), ("force_slow 1", (("debug_force_slow", 1),), None)],
                         ids=["variant_0", "variant_1", "force_slow_1"])
def test_other_paths_give_the_same_bytes(pkg, orc, label, params, variant):
    """Trace variants 0 and 1 (the exact closest-hit kernel) and debug_force_slow 1 (the any-hit launch's exact redo) on the grazing
    normals, the distant lamps and the (1, 1e-8, 1) table."""
    cases = [(c["flat"], c["p"], c["nrm"]) for c in (_classes(pkg)["normals"][0], _classes(pkg)["distant"][0])]
    cases.append((_hostile(pkg, "one_tiny_one")[0],) + _cloud(500, seed=4))
    for k, (flat, p, nrm) in enumerate(cases):
        if ("want", k) not in _cache:
            _cache[("want", k)] = D.query(orc, flat, p, nrm, 3)
        with pkg.PathTracer() as pt:
            for key, value in params:
                pt.set_param(key, value)
            pt.create_buffers((32, 32), flat)
            if variant is not None:
                pt.set_trace_variant(variant)
            got = pt.direct_light(p, nrm, 3, want_rays=True)
        _same_call(got, _cache[("want", k)], (label, k))


# ---- the megakernel's units --------------------------------------------------------------------------------------------------------
PLANES = ("color", "normal", "depth")
UNITS = {"direct_light": {}, "environment_light": {"env_light": True}, "mis": {"mis": True}, "smooth_normals": {"smooth": True}}


@pytest.mark.parametrize("unit", list(UNITS))
def test_megakernel_units(pkg, orc, unit):
    """One 33 x 17 frame, 2 iterations, 3 bounces of a floor under the (1, 1e-8, 1) table with "direct_light" 1 -- alone, with the
    environment as a light, with mis, with smooth normals: the four kernel units that compile light_sample_point in -- against the loop
    restatement, planes and counters bit for bit."""
    w, h, mb, iters = 33, 17, 3, 2
    if "frame" not in _cache:
        scene = LC.table_scene(pkg, [("mesh", 1.0, [1.0, 1e-8, 1.0], [(-2, 2, -1), (0, 0, 0), (1, 2, -1)])], floor=True)
        scene.camera = pkg.scenes._camera_from_look_at((0.0, 0.3, 3.5), (0.0, 0.0, -0.5), vfov_deg=50.0)
        flat = scene.build_scene(distinct_meshes=True)
        _cache["frame"] = (scene, flat, pkg.compute_vertex_normals(flat))
    scene, flat, normals = _cache["frame"]
    opt = UNITS[unit]
    env = smooth_ref.ENV if opt.get("env_light") else None
    entries = None
    if env is not None:
        import env_light_ref
        entries = env_light_ref.table_of(pkg, env)[0]
    ref = loop_ref.render_megakernel(orc, flat, scene.camera, w, h, 0, iters, mb, normals=normals if opt.get("smooth") else None,
                                       smooth=opt.get("smooth", False), env=env, entries=entries, env_light=opt.get("env_light", False), direct=True,
                                       mis=opt.get("mis", False))
    with pkg.PathTracer(device=0, max_bounces=mb) as pt:
        pt.current_gpu_method = pkg.GPUMethod.megakernel
        pt.direct_light = True
        pt.environment_light = opt.get("env_light", False)
        pt.mis = opt.get("mis", False)
        pt.smooth_normals = opt.get("smooth", False)
        pt.create_buffers((w, h), flat)
        if opt.get("smooth"):
            pt.vertex_normals = normals
        pt.environment = env
        pt.restart()
        pt.max_iterations = iters
        for _ in range(iters):
            pt.path_trace(scene.camera)
        got = {k: pt.download(k) for k in PLANES}
        got["rays"] = pt.stats()["rays_total"]
        got.update(pt.direct_loop_stats())
        got.update({"env_" + k: v for k, v in pt.environment_light_loop_stats().items()})
        st = pt.mis_loop_stats()
        got.update({"mis_emitter_hits": st["weighted_emitter_hits"], "mis_misses": st["weighted_misses"]})
        got.update(pt.smooth_loop_stats())
    for k in PLANES:
        a, b = _bits(got[k]), _bits(np.asarray(ref[k], dtype=np.float32).reshape(got[k].shape))
        assert np.array_equal(a, b), (unit, k, int(np.sum(a != b)), np.argwhere(a != b)[:4].tolist())
    for k in ("rays", "diffuse_hits", "shadow_rays", "unoccluded", "env_diffuse_hits", "env_shadow_rays", "env_unoccluded", "mis_emitter_hits",
              "mis_misses") + tuple(smooth_ref.COUNTERS):
        assert got[k] == ref[k], (unit, k, got[k], ref[k])
    assert ref["diffuse_hits"] > 0 and ref["shadow_rays"] > 0 and ref["unoccluded"] > 0
    if opt.get("env_light"):
        assert ref["env_shadow_rays"] > 0
    if opt.get("smooth"):
        assert ref["shading_normals"] > 0
