"""Normal maps on the GPU (ptc_set_normal_maps, ptc_set_param "normal_maps", ptc_hit_shading_normal): the
shading-normal query and the megakernel's normal-mapped instances against the numpy restatement tests/normal_map_ref.py, bit for bit;
the states in which the feature must change nothing; what the binding is tied to (the scene and its texture pool)."""
import ctypes as C

import numpy as np
import pytest

import env_light_ref
import loop_ref
import normal_map_ref
import smooth_ref
import texture_ref

pytestmark = pytest.mark.gpu

PLANES = ("color", "normal", "depth")
OLD = ("diffuse_hits", "shadow_rays", "unoccluded", "env_diffuse_hits", "env_shadow_rays", "env_unoccluded", "mis_emitter_hits", "mis_misses")
FOURTEEN = OLD + smooth_ref.COUNTERS + texture_ref.COUNTERS
EVERYTHING = PLANES + ("rays",) + FOURTEEN + normal_map_ref.COUNTERS
W, H, ITERS = 33, 17, 2
LENS = (0.25, 3.5)
ENV = smooth_ref.ENV
FLT_MAX = np.float32(np.finfo(np.float32).max)
BUMPY, FLAT_MAP = 3, 4  # where the two maps stand in the pool, behind texture_ref.pool's three
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _entries(pkg):
    if "entries" not in _cache:
        _cache["entries"] = env_light_ref.table_of(pkg, ENV)[0]
    return _cache["entries"]


# name -> (the scene, {material: colour texture}, {material: normal map})
SCENES = {
    "room": (lambda pkg: smooth_ref.room_scene(pkg), {"ball": 0, "ball2": 2, "walls": 1}, {"ball": BUMPY, "ball2": BUMPY, "walls": BUMPY}),
    "sheet": (lambda pkg: smooth_ref.sheet_scene(pkg), {"sheet": 0, "diffuse": 2, "floor": 1}, {"sheet": BUMPY, "diffuse": BUMPY, "floor": BUMPY}),
    "lamp": (lambda pkg: smooth_ref.sheet_scene(pkg, ("lamp", "diffuse")), {"sheet": 0, "diffuse": 1, "lamp": 2}, {"sheet": BUMPY, "diffuse": 0, "lamp": BUMPY}),
    "metal": (lambda pkg: smooth_ref.sheet_scene(pkg, ("metal", "diffuse")), {"metal": 2, "diffuse": 0}, {"metal": BUMPY, "sheet": BUMPY}),
    "ignored": (lambda pkg: smooth_ref.sheet_scene(pkg, ("glass", "lamp")), {"sheet": 2}, {"glass": BUMPY, "lamp": BUMPY, "sheet": BUMPY}),
}


def _scene(pkg, name):
    """name -> dict(scene, flat, textures, binding, nbinding, st, nrm), built once"""
    if name not in _cache:
        scene = SCENES[name][0](pkg)
        flat = scene.build_scene(distinct_meshes=True)
        textures = texture_ref.pool(pkg) + [normal_map_ref.bumpy_map(pkg, filter="bilinear", wrap="repeat"), normal_map_ref.flat_map(pkg)]
        _cache[name] = dict(scene=scene, flat=flat, textures=textures, binding=texture_ref.bind(scene, flat, SCENES[name][1]),
                            nbinding=texture_ref.bind(scene, flat, SCENES[name][2]), st=texture_ref.random_texcoords(flat),
                            nrm=pkg.compute_vertex_normals(flat))
    return _cache[name]


def _tracer(pkg, flat, w=W, h=H, mb=8, mega=True, textured=False, bent=True, table=None, maps=None, st=None, smooth=False, normals=None, mis=False,
            env_light=False, direct=False, roulette=0, lens=None, interleave=None):
    pt = pkg.PathTracer(device=0, max_bounces=mb)
    if mega:
        pt.current_gpu_method = pkg.GPUMethod.megakernel
    pt.textures = textured
    pt.normal_maps = bent
    pt.smooth_normals = smooth
    pt.mis = mis
    pt.environment_light = env_light
    pt.direct_light = direct
    pt.roulette = roulette
    if lens is not None:
        pt.lens = lens
    pt.create_buffers((w, h), flat)
    if table is not None:
        pt.texture_table = table
    if maps is not None:
        pt.normal_map_table = maps
    if st is not None:
        pt.texcoords = st
    if normals is not None:
        pt.vertex_normals = normals
    if interleave is not None:
        pt.set_interleave(*interleave)
    return pt


def _result(pt):
    out = {p: pt.download(p) for p in PLANES}
    out["rays"] = pt.stats()["rays_total"]
    out.update(pt.direct_loop_stats())
    out.update({"env_" + k: v for k, v in pt.environment_light_loop_stats().items()})
    st = pt.mis_loop_stats()
    out.update({"mis_emitter_hits": st["weighted_emitter_hits"], "mis_misses": st["weighted_misses"]})
    out.update(pt.smooth_loop_stats())
    st = pt.texture_loop_stats()
    out.update({"lookups": st["lookups"], "tex_fallbacks": st["fallbacks"]})
    out.update(pt.normal_map_loop_stats())
    return out


def _run(pt, camera, env, iters=ITERS, iter_begin=0):
    pt.environment = env
    pt.restart()
    if iter_begin:
        pt.set_iteration(iter_begin)
    pt.max_iterations = iter_begin + iters
    rays0 = pt.stats()["rays_total"]
    for _ in range(iters):
        pt.path_trace(camera)
    out = _result(pt)
    out["rays"] -= rays0
    return out


def _same(got, ref, keys, what):
    for k in keys:
        if k in PLANES:
            a, b = _bits(got[k]), _bits(np.asarray(ref[k], dtype=np.float32).reshape(got[k].shape))
            assert np.array_equal(a, b), (what, k, int(np.sum(a != b)), np.argwhere(a != b)[:4].tolist())
        else:
            assert got[k] == ref[k], (what, k, got[k], ref[k])


def _against_the_loop(pkg, orc, scene_name, w=W, h=H, mb=8, env=None, iters=ITERS, iter_begin=0, st=None, smooth=False, textured=False, **kw):
    s = _scene(pkg, scene_name)
    st = s["st"] if st is None else st
    entries = _entries(pkg) if env is not None else None
    ref = loop_ref.render_megakernel(orc, s["flat"], s["scene"].camera, w, h, iter_begin, iters, mb, textures=s["textures"],
                                           binding=s["binding"], texcoords=st, textured=textured, nbinding=s["nbinding"], normal_maps=True,
                                           normals=s["nrm"] if smooth else None, smooth=smooth, env=env, entries=entries,
                                           env_light=kw.get("env_light", False), direct=kw.get("direct", False), mis=kw.get("mis", False),
                                           roulette=kw.get("roulette", 0), lens=kw.get("lens"), pkg=pkg)
    with _tracer(pkg, s["flat"], w, h, mb, textured=textured, table=(s["textures"], s["binding"]), maps=s["nbinding"], st=st, smooth=smooth,
                 normals=s["nrm"] if smooth else None, **kw) as pt:
        got = _run(pt, s["scene"].camera, env, iters, iter_begin)
    _same(got, ref, EVERYTHING, (scene_name, w, h, mb, kw, iter_begin))
    return got


# ---- 1. the shading-normal query ---------------------------------------------------------------------------------------------------------
def _rays(o, d, tmin=1e-4, tmax=FLT_MAX):
    o, d = np.asarray(o, dtype=np.float32).reshape(-1, 3), np.asarray(d, dtype=np.float32).reshape(-1, 3)
    r = np.zeros((len(o), 8), dtype=np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmin, d, tmax
    return r


def _query(pkg, orc, flat, rays, normals, textures, nbinding, st):
    want = normal_map_ref.hit_shading_normal(orc, flat, rays, normals=normals, textures=textures if nbinding is not None else None, nbinding=nbinding,
                                             texcoords=st)
    table = None if textures is None else (textures, np.full(len(flat.materials), -1, np.int32))
    with _tracer(pkg, flat, mega=False, bent=False, table=table, maps=nbinding, st=st, normals=normals) as pt:
        got = pt.hit_shading_normal(rays)
    assert np.array_equal(got["outcome"], want["outcome"]), np.argwhere(got["outcome"] != want["outcome"])[:4].tolist()
    assert np.array_equal(_bits(got["normal"]), _bits(want["normal"])), np.argwhere(_bits(got["normal"]) != _bits(want["normal"]))[:4].tolist()
    return got


@pytest.mark.parametrize("what", ["everything", "vertex_normals_alone", "binding_alone", "nothing"])
def test_hit_shading_normal_random_rays(pkg, orc, what):
    """4099 rays (no multiple of 64) from around a two-mesh table whose second mesh starts at first_index > 0, with a sphere object: hits
    on both meshes and both instances, on the sphere (outcome 1), and misses (outcome 0, zeros)"""
    s = _scene(pkg, "sheet")
    flat = s["flat"]
    assert smooth_ref.mesh_rows(flat)[1][2] > 0
    rng = np.random.default_rng(3)
    k = 4099
    o = (rng.standard_normal((k, 3)) * 0.2 + [0.0, 1.5, 2.5]).astype(np.float32)
    at = rng.uniform([-1.4, -0.8, -1.5], [1.4, 0.8, 1.0], (k, 3))
    d = at - o
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
    d[::9] = -d[::9]  # away from everything
    rays = _rays(o, d)
    rays[5::11, 7] = 2.0  # a t_max of the caller's that cuts some hits off
    mapped = what in ("everything", "binding_alone")
    got = _query(pkg, orc, flat, rays, s["nrm"] if what in ("everything", "vertex_normals_alone") else None, s["textures"] if mapped else None,
                 s["nbinding"] if mapped else None, s["st"] if mapped else None)
    how = got["outcome"]
    assert (how == normal_map_ref.MISS).sum() > 400 and not got["normal"][how == normal_map_ref.MISS].any()
    assert (how == normal_map_ref.NONE).sum() > 100  # the floor sphere
    if mapped:
        assert (how == normal_map_ref.BENT).sum() > 300 and (how == normal_map_ref.KEPT).sum() > 0
    else:
        assert (how <= normal_map_ref.NONE).all()


def test_hit_shading_normal_on_a_seam(pkg, orc):
    """rays aimed at the shared edges and the shared vertices of test_hit_surface_on_a_seam's 2 x 2-quad sheet, whose two triangles per
    quad carry different corner coordinates: the winner's corners span the tangent frame (ties: the triangle the walk visits last)"""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.add_material("a", pkg.DiffuseMateral((0.5, 0.75, 0.25)))
    pos, idx = smooth_ref.sheet(2, 2, size=2.0)
    s.add_object(s.add_mesh("sheet.obj", pkg.Mesh(pos, idx)), glm.identity(), "a")
    flat = s.build_scene(distinct_meshes=True)
    st = np.zeros((len(idx), 2), np.float32)
    tri = np.arange(len(idx)) // 3
    corner = np.arange(len(idx)) % 3
    st[:, 0] = tri * 0.125 + np.float32([0.0, 0.0625, 0.03125])[corner]  # every triangle a band of s of its own, and a frame of its own:
    st[:, 1] = np.where(tri % 2 == 0, 0.25, 0.75) + np.float32([0.0, 0.03125, 0.0625])[corner] * (1 + tri % 3)  # det != 0, dyadic
    targets = [(x, 0.0, z) for x in (-1.0, -0.5, 0.0, 0.5, 1.0) for z in (-1.0, -0.5, 0.0, 0.5, 1.0)]
    targets += [(0.25, 0.0, -0.25), (-0.25, 0.0, 0.25), (0.3, 0.0, 0.1), (3.0, 0.0, 3.0)]
    d = np.float32([0.5, -1.0, 0.25])
    o = np.float32([(x - 1.0, y + 2.0, z - 0.5) for x, y, z in targets])
    tex = [normal_map_ref.bumpy_map(pkg, 8, 8, tilt=40, filter="nearest", wrap="repeat")]
    got = _query(pkg, orc, flat, _rays(o, np.tile(d, (len(o), 1))), None, tex, np.zeros(1, np.int32), st)
    assert got["outcome"][-1] == normal_map_ref.MISS and (got["outcome"][:-1] == normal_map_ref.BENT).all()
    assert len({tuple(n) for n in _bits(got["normal"][:-1]).tolist()}) >= 8  # all eight triangles win somewhere


# ---- 2. frames against the restatement ------------------------------------------------------------------------------------------------
SIZES = [(33, 17, 1), (33, 17, 8), (65, 33, 2), (65, 33, 8)]


@pytest.mark.parametrize("w,h,mb", SIZES)
def test_the_lamp_lit_room(pkg, orc, w, h, mb):
    """a mapped diffuse mesh and its scaled, rotated instance (and the room's walls) under "direct_light" """
    got = _against_the_loop(pkg, orc, "room", w, h, mb, direct=True)
    assert got["bent"] > 0 and got["shadow_rays"] > 0 and got["lookups"] == 0


@pytest.mark.parametrize("w,h,mb", SIZES)
def test_a_sheet_under_the_sky(pkg, orc, w, h, mb):
    got = _against_the_loop(pkg, orc, "sheet", w, h, mb, env=ENV, env_light=True)
    assert got["bent"] > 0 and got["env_shadow_rays"] > 0 and got["culled_light_samples"] > 0


@pytest.mark.parametrize("w,h,mb", SIZES)
@pytest.mark.parametrize("smooth", [False, True])
def test_both_lights_with_mis(pkg, orc, w, h, mb, smooth):
    got = _against_the_loop(pkg, orc, "lamp", w, h, mb, env=ENV, env_light=True, direct=True, mis=True, smooth=smooth)
    assert got["bent"] > 0 and (got["shading_normals"] > 0) == smooth and (got["mis_misses"] > 0 or mb == 1)


@pytest.mark.parametrize("w,h,mb", SIZES)
@pytest.mark.parametrize("smooth", [False, True])
def test_a_metal_mesh(pkg, orc, w, h, mb, smooth):
    got = _against_the_loop(pkg, orc, "metal", w, h, mb, env=ENV, smooth=smooth)
    assert got["bent"] > 0


@pytest.mark.parametrize("w,h,mb", SIZES)
@pytest.mark.parametrize("smooth", [False, True])
def test_colour_texture_and_normal_map_together(pkg, orc, w, h, mb, smooth):
    got = _against_the_loop(pkg, orc, "sheet", w, h, mb, env=ENV, env_light=True, textured=True, smooth=smooth)
    assert got["bent"] > 0 and got["lookups"] > 0


@pytest.mark.parametrize("w,h,mb", SIZES)
def test_a_binding_on_glass_and_on_an_emitter_is_ignored(pkg, orc, w, h, mb):
    got = _against_the_loop(pkg, orc, "ignored", w, h, mb, env=ENV, direct=True, textured=True)
    s = _scene(pkg, "ignored")
    only = texture_ref.bind(s["scene"], s["flat"], {"sheet": BUMPY})
    with _tracer(pkg, s["flat"], w, h, mb, textured=True, table=(s["textures"], s["binding"]), maps=only, st=s["st"], direct=True) as pt:
        unbound = _run(pt, s["scene"].camera, ENV)
    _same(got, unbound, EVERYTHING, "ignored")


@pytest.mark.parametrize("w,h,mb", SIZES)
def test_nan_and_infinite_coordinates_are_kept(pkg, orc, w, h, mb):
    bad = _scene(pkg, "sheet")["st"].copy()
    bad[::7, 0] = np.nan
    bad[3::11, 1] = np.inf
    bad[5::13, 0] = -np.inf
    got = _against_the_loop(pkg, orc, "sheet", w, h, mb, env=ENV, env_light=True, st=bad, textured=True)
    assert got["kept"] > 0 and got["bent"] > 0 and got["tex_fallbacks"] > 0


@pytest.mark.parametrize("w,h,mb", SIZES)
def test_roulette_under_the_lens(pkg, orc, w, h, mb):
    _against_the_loop(pkg, orc, "room", w, h, mb, direct=True, roulette=1, lens=LENS)


@pytest.mark.parametrize("w,h,mb", SIZES)
def test_iteration_2_31_minus_5(pkg, orc, w, h, mb):
    _against_the_loop(pkg, orc, "sheet", w, h, mb, iters=2, iter_begin=2 ** 31 - 5, env=ENV, env_light=True)


def test_plain_without_any_light(pkg, orc):
    got = _against_the_loop(pkg, orc, "sheet", mb=4)
    assert got["bent"] > 0 and got["absorbed"] > 0


@pytest.mark.parametrize("w,h,mb", SIZES)
def test_two_interleaved_ranks_against_the_one_context_frame(pkg, w, h, mb):
    s = _scene(pkg, "sheet")
    kw = dict(textured=True, table=(s["textures"], s["binding"]), maps=s["nbinding"], st=s["st"], env_light=True)
    with _tracer(pkg, s["flat"], w, h, mb, **kw) as pt:
        one = _run(pt, s["scene"].camera, ENV)
    parts = []
    for rank in (0, 1):
        with _tracer(pkg, s["flat"], w, h, mb, interleave=(rank, 2, 8), **kw) as pt:
            parts.append(_run(pt, s["scene"].camera, ENV))
        rows = [r for first in range(rank * 8, h, 16) for r in range(first, min(first + 8, h))]
        for p in PLANES:
            assert np.array_equal(_bits(parts[-1][p].reshape(len(rows), w, -1)), _bits(one[p].reshape(h, w, -1)[rows])), (rank, p)
    for k in ("rays",) + FOURTEEN + normal_map_ref.COUNTERS:
        assert parts[0][k] + parts[1][k] == one[k], k
    assert one["bent"] > 0


# ---- 3. the states that must change nothing -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mis", [False, True])
@pytest.mark.parametrize("smooth", [False, True])
def test_a_flat_map_gives_the_bits_of_normal_maps_0(pkg, mis, smooth):
    """every texel (128, 128, 255): n is b's own bits, nothing is culled or absorbed that was not, with the colour texture and without"""
    s = _scene(pkg, "lamp")
    flat_maps = np.where(s["nbinding"] >= 0, FLAT_MAP, -1).astype(np.int32)
    for textured in (False, True):
        kw = dict(textured=textured, table=(s["textures"], s["binding"]), maps=flat_maps, st=s["st"], env_light=True, direct=True, mis=mis,
                  smooth=smooth, normals=s["nrm"])
        with _tracer(pkg, s["flat"], bent=False, **kw) as pt:
            want = _run(pt, s["scene"].camera, ENV)
        with _tracer(pkg, s["flat"], bent=True, **kw) as pt:
            got = _run(pt, s["scene"].camera, ENV)
        _same(got, want, EVERYTHING, ("flat", textured))
        assert got["bent"] == 0 and got["kept"] == 0 and (got["lookups"] > 0) == textured


@pytest.mark.parametrize("mis", [False, True])
@pytest.mark.parametrize("smooth", [False, True])
def test_the_bits_of_the_parent(pkg, mis, smooth):
    """ "normal_maps" 1 with every material unbound, without coordinates or without textures, and "normal_maps" 0 with everything set
    render what a context that never heard of normal maps renders"""
    s = _scene(pkg, "lamp")
    kw = dict(env_light=True, direct=True, mis=mis, smooth=smooth, normals=s["nrm"], roulette=2)
    with _tracer(pkg, s["flat"], bent=False, **kw) as pt:
        want = _run(pt, s["scene"].camera, ENV)
    unbound = np.full(len(s["nbinding"]), -1, np.int32)
    table = (s["textures"], s["binding"])
    cases = {"unbound": dict(bent=True, table=table, maps=unbound, st=s["st"]),
             "no_binding": dict(bent=True, table=table, st=s["st"]),
             "no_coordinates": dict(bent=True, table=table, maps=s["nbinding"]),
             "no_textures": dict(bent=True, st=s["st"]),
             "off": dict(bent=False, table=table, maps=s["nbinding"], st=s["st"])}
    for name, nm in cases.items():
        with _tracer(pkg, s["flat"], **nm, **kw) as pt:
            got = _run(pt, s["scene"].camera, ENV)
        _same(got, want, EVERYTHING, (name, mis, smooth))
        assert got["bent"] == 0 and got["kept"] == 0


# ---- 4. what the binding is tied to ----------------------------------------------------------------------------------------------------
def test_normal_maps_set_changed_and_removed(pkg, orc):
    """set, trace 2; another binding, trace 2; none, trace 2; the first again, trace 2: the restatement continued with prev="""
    s = _scene(pkg, "sheet")
    flat, cam = s["flat"], s["scene"].camera
    other = texture_ref.bind(s["scene"], flat, {"sheet": 0, "diffuse": BUMPY})
    steps = [s["nbinding"], other, None, s["nbinding"]]
    ref = None
    for k, maps in enumerate(steps):
        ref = loop_ref.render_megakernel(orc, flat, cam, W, H, 2 * k, 2, 4, textures=s["textures"], binding=s["binding"], texcoords=s["st"],
                                               textured=True, nbinding=maps, normal_maps=True, prev=ref, pkg=pkg)
    with _tracer(pkg, flat, mb=4, textured=True, table=(s["textures"], s["binding"]), st=s["st"]) as pt:
        pt.max_iterations = 8
        for maps in steps:
            pt.normal_map_table = maps
            bound = C.c_uint32(9)
            assert pt._lib.ptc_get_normal_maps(pt._ctx, C.byref(bound)) == (1 if maps is not None else 0)
            assert bound.value == (int((maps >= 0).sum()) if maps is not None else 0)
            pt.path_trace(cam)
            pt.path_trace(cam)
        _same(_result(pt), ref, PLANES, "changed")


def test_what_drops_the_binding_and_what_keeps_it(pkg):
    s = _scene(pkg, "sheet")
    flat, textures, binding, maps, st = s["flat"], s["textures"], s["binding"], s["nbinding"], s["st"]
    invalid = pkg._capi.PTC_ERR_INVALID
    with _tracer(pkg, flat, mb=4, table=(textures, binding), maps=maps, st=st) as pt:
        lib, ctx = pt._lib, pt._ctx
        bound = C.c_uint32(0)
        assert lib.ptc_get_normal_maps(ctx, C.byref(bound)) == 1 and bound.value == int((maps >= 0).sum())
        for bad, word in ((maps[:-1], "materials"), (np.where(maps == BUMPY, 5, maps), "bound to texture 5"),
                          (np.where(maps == BUMPY, -2, maps), "bound to texture -2")):
            with pytest.raises(pkg.PtcError) as e:
                pt.normal_map_table = bad
            assert e.value.code == invalid and word in str(e.value), (word, str(e.value))
        m = np.ascontiguousarray(maps, dtype=np.int32)
        assert lib.ptc_set_normal_maps(ctx, m.ctypes.data_as(C.c_void_p), 0) == invalid  # not NULL with 0
        assert lib.ptc_set_normal_maps(ctx, None, len(m)) == invalid
        with pytest.raises(pkg.PtcError):
            pt.texture_table = (textures, binding[:-1])  # a refused ptc_set_textures keeps the binding too
        assert lib.ptc_get_normal_maps(ctx, C.byref(bound)) == 1 and bound.value == int((maps >= 0).sum()) and pt.normal_map_table is not None
        before = _run(pt, s["scene"].camera, None)  # ... and what was set still renders
        assert before["bent"] > 0
        pt.resize_image((W + 2, H))  # a resize does not touch it
        assert lib.ptc_get_normal_maps(ctx, None) == 1
        pt.texture_table = (textures[:4], binding)  # a successful ptc_set_textures drops it: its indices named the old pool
        assert lib.ptc_get_normal_maps(ctx, C.byref(bound)) == 0 and bound.value == 0 and pt.normal_map_table is None
        assert _run(pt, s["scene"].camera, None)["bent"] == 0
        pt.normal_map_table = maps
        pt.texture_table = None  # ... and so does their removal
        assert lib.ptc_get_normal_maps(ctx, None) == 0 and pt.normal_map_table is None
        with pytest.raises(pkg.PtcError) as e:
            pt.normal_map_table = maps
        assert e.value.code == invalid and "no textures" in str(e.value)
        pt.texture_table = (textures, binding)
        pt.normal_map_table = maps
        pt.create_buffers((W, H), flat)  # an upload drops it with the scene
        assert lib.ptc_get_normal_maps(ctx, C.byref(bound)) == 0 and bound.value == 0 and pt.normal_map_table is None
        assert _run(pt, s["scene"].camera, None)["bent"] == 0
    with pkg.PathTracer(device=0) as pt:
        with pytest.raises(pkg.PtcError) as e:
            pt.normal_map_table = maps
        assert e.value.code == pkg._capi.PTC_ERR_NO_SCENE


def test_the_streaming_loop_refuses_and_queues_nothing(pkg):
    s = _scene(pkg, "sheet")
    with _tracer(pkg, s["flat"], mega=False, table=(s["textures"], s["binding"]), maps=s["nbinding"], st=s["st"]) as pt:
        pt.max_iterations = 4
        for _ in range(2):
            with pytest.raises(pkg._capi.PtcError) as e:
                pt.path_trace(s["scene"].camera)
            assert e.value.code == pkg._capi.PTC_ERR_INVALID and "normal_maps are rendered by the megakernel" in str(e.value)
        cam = pkg._capi.ptc_camera()
        assert pt._lib.ptc_trace_begin(pt._ctx, C.byref(cam)) == pkg._capi.PTC_ERR_INVALID
        assert pt.iteration() == 0 and pt.stats()["rays_total"] == 0 and pt.stats()["frames"] == 0
        pt.normal_maps = False  # and without it the context renders as ever
        pt.path_trace(s["scene"].camera)
        assert pt.iteration() == 1 and pt.stats()["rays_total"] > 0
    with pkg.PathTracer(device=0) as pt:
        for bad in (-1, 2):
            with pytest.raises(pkg._capi.PtcError) as e:
                pt.set_param("normal_maps", bad)
            assert "normal_maps must be 0 or 1" in str(e.value)


# ---- 5. the command line ----------------------------------------------------------------------------------------------------------------
import json  # noqa: E402
import os  # noqa: E402
import struct  # noqa: E402
import subprocess  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_PT = os.path.join(ROOT, "cuda-path-tracer_amd", "host", "hip_pt")
ASSET = os.path.join(ROOT, "assets", "scenes", "cornell_bumpy.json")


def _read_raw(path):
    data = open(path, "rb").read()
    assert data[:4] == b"PTRF"
    w, h, ch = struct.unpack_from("<III", data, 4)
    assert ch == 7 and len(data) == 16 + 4 * 7 * w * h
    f = np.frombuffer(data, dtype="<f4", offset=16)
    P = w * h
    return {"color": f[:3 * P].reshape(h, w, 3), "normal": f[3 * P:6 * P].reshape(h, w, 3), "depth": f[6 * P:].reshape(h, w)}


def _asset_reference(pkg, orc):
    """the restatement of assets/scenes/cornell_bumpy.json with the Python reader's textures, maps and coordinates, once for the three runs"""
    if "asset" not in _cache:
        scene = pkg.json_parser.scene_from_json(ASSET)
        assert scene.normal_maps is True and scene.textures is True
        flat = scene.build_scene()
        w, h = scene.resolution
        textures = [pkg.Texture(pkg.png.read_png(s.file), s.encoding, s.filter, s.wrap) for s in flat.texture_sources]
        _cache["asset"] = loop_ref.render_megakernel(orc, flat, scene.camera, w, h, 0, 1, 2, textures=textures, binding=flat.material_texture,
                                                           texcoords=flat.texcoords, textured=True, nbinding=flat.material_normal_map,
                                                           normal_maps=True, pkg=pkg)
        assert _cache["asset"]["bent"] > 1000  # (what a run that ignored the option would not reproduce)
    return _cache["asset"]


@pytest.mark.parametrize("how", ["flag", "scene_key", "two_ranks"])
def test_hip_pt_normal_maps_against_the_restatement(pkg, orc, tmp_path, how):
    """hip_pt --method megakernel with --normal-maps (on the asset without its "normal_maps" key), with the scene key, and over two
    ranks: the float framebuffers the run dumps are the restatement's"""
    if not os.path.exists(HIP_PT):
        subprocess.run(["make"], cwd=os.path.dirname(HIP_PT), check=True, stdout=subprocess.DEVNULL)
    want = _asset_reference(pkg, orc)
    scene_file, extra = ASSET, []
    if how == "flag":  # the same scene beside the asset's folder tree, its files named from there, without the key
        with open(ASSET) as f:
            j = json.load(f)
        del j["normal_maps"]
        for s in j["surfaces"]:
            if "filename" in s:
                s["filename"] = os.path.relpath(os.path.join(os.path.dirname(ASSET), s["filename"]), str(tmp_path))
        for m in j["materials"]:
            for key in ("texture", "normal_map"):
                if key in m:
                    m[key]["file"] = os.path.relpath(os.path.join(os.path.dirname(ASSET), m[key]["file"]), str(tmp_path))
        scene_file = str(tmp_path / "no_key.json")
        with open(scene_file, "w") as f:
            json.dump(j, f)
        extra = ["--normal-maps"]
    if how == "two_ranks":
        extra = ["--gpus", "2"]
    raw = tmp_path / "out.raw"
    cmd = [HIP_PT, scene_file, "-o", str(tmp_path / "out.png"), "--spp", "1", "--max-bounces", "2", "--dump-raw", str(raw), "--method", "megakernel"] + extra
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    _same(_read_raw(raw), want, PLANES, how)
