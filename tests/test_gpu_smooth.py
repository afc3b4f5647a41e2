"""Smooth shading on the GPU (ptc_set_vertex_normals, ptc_set_param "smooth_normals", ptc_hit_attributes): the
primitive query and the megakernel's smooth instances against the numpy restatement tests/smooth_ref.py, bit for bit; what vertex
normals are tied to (the scene) and what they must leave alone; the cases in which the parameter must change nothing."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import env_light_ref
import loop_ref
import smooth_ref

pytestmark = pytest.mark.gpu

PLANES = ("color", "normal", "depth")
OLD = ("diffuse_hits", "shadow_rays", "unoccluded", "env_diffuse_hits", "env_shadow_rays", "env_unoccluded", "mis_emitter_hits", "mis_misses")
EVERYTHING = PLANES + ("rays",) + OLD + smooth_ref.COUNTERS
W, H, ITERS = 33, 17, 2
LENS = (0.25, 3.5)
ENV = smooth_ref.ENV
NONE = 0xFFFFFFFF
FLT_MAX = np.float32(np.finfo(np.float32).max)
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _entries(pkg):
    if "entries" not in _cache:
        _cache["entries"] = env_light_ref.table_of(pkg, ENV)[0]
    return _cache["entries"]


def _scene(pkg, name):
    """name -> (scene, flat, the host's vertex normals of the scene), built once"""
    if name not in _cache:
        if name == "room":
            scene = smooth_ref.room_scene(pkg)
        elif name == "glass_metal":
            scene = smooth_ref.sheet_scene(pkg, ("glass", "metal"))
        elif name == "lamp":
            scene = smooth_ref.sheet_scene(pkg, ("lamp", "diffuse"))
        else:
            scene = smooth_ref.sheet_scene(pkg)
        flat = scene.build_scene(distinct_meshes=True)
        _cache[name] = (scene, flat, pkg.compute_vertex_normals(flat))
    return _cache[name]


def _tracer(pkg, flat, w=W, h=H, mb=8, mega=True, smooth=True, normals=None, mis=False, env_light=False, direct=False, roulette=0, lens=None,
            interleave=None):
    pt = pkg.PathTracer(device=0, max_bounces=mb)
    if mega:
        pt.current_gpu_method = pkg.GPUMethod.megakernel
    pt.smooth_normals = smooth
    pt.mis = mis
    pt.environment_light = env_light
    pt.direct_light = direct
    pt.roulette = roulette
    if lens is not None:
        pt.lens = lens
    pt.create_buffers((w, h), flat)
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


def _against_the_loop(pkg, orc, scene_name, w=W, h=H, mb=8, env=None, iters=ITERS, iter_begin=0, normals=None, **kw):
    scene, flat, nrm = _scene(pkg, scene_name)
    nrm = nrm if normals is None else normals
    entries = _entries(pkg) if env is not None else None
    ref = loop_ref.render_megakernel(orc, flat, scene.camera, w, h, iter_begin, iters, mb, normals=nrm, smooth=True, env=env, entries=entries,
                                       env_light=kw.get("env_light", False), direct=kw.get("direct", False), mis=kw.get("mis", False),
                                       roulette=kw.get("roulette", 0), lens=kw.get("lens"))
    with _tracer(pkg, flat, w, h, mb, normals=nrm, **kw) as pt:
        got = _run(pt, scene.camera, env, iters, iter_begin)
    _same(got, ref, EVERYTHING, (scene_name, w, h, mb, kw, iter_begin))
    return got


# ---- 1. the primitive query ------------------------------------------------------------------------------------------------------------
def _query(pkg, orc, flat, rays, normals):
    want = smooth_ref.hit_attributes(orc, flat, rays, normals)
    with _tracer(pkg, flat, mega=False, smooth=False, normals=normals) as pt:
        got = pt.hit_attributes(rays)
    for k in ("object", "triangle"):
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4].tolist())
    for k in ("uv", "normal"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (k, np.argwhere(_bits(got[k]) != _bits(want[k]))[:4].tolist())
    return got


def _rays(o, d, tmin=1e-4, tmax=FLT_MAX):
    o, d = np.asarray(o, dtype=np.float32).reshape(-1, 3), np.asarray(d, dtype=np.float32).reshape(-1, 3)
    r = np.zeros((len(o), 8), dtype=np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmin, d, tmax
    return r


@pytest.mark.parametrize("with_normals", [False, True])
def test_hit_attributes_random_rays(pkg, orc, with_normals):
    """4099 rays (no multiple of 64) from around a two-mesh table whose second mesh starts at first_vertex > 0, with a sphere object: hits
    on both meshes and both instances, on the sphere (triangle 0xffffffff), and misses"""
    scene, flat, nrm = _scene(pkg, "sheet")
    assert smooth_ref.mesh_rows(flat)[1][0] > 0
    rng = np.random.default_rng(3)
    k = 4099
    o = (rng.standard_normal((k, 3)) * 0.2 + [0.0, 1.5, 2.5]).astype(np.float32)
    at = rng.uniform([-1.4, -0.8, -1.5], [1.4, 0.8, 1.0], (k, 3))
    d = at - o
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
    d[::9] = -d[::9]  # away from everything
    rays = _rays(o, d)
    rays[5::11, 7] = 2.0  # a t_max of the caller's that cuts some hits off
    got = _query(pkg, orc, flat, rays, nrm if with_normals else None)
    hit = got["object"] != NONE
    assert (got["object"] == 0).sum() > 100 and (got["object"] == 1).sum() > 100 and (got["object"] == 2).sum() > 100 and (got["object"] == 3).sum() > 30
    assert (~hit).sum() > 400 and np.all(got["triangle"][got["object"] == 0] == NONE) and not got["normal"][~hit].any()


def test_hit_attributes_ties(pkg, orc):
    """rays aimed at the shared edges and the shared vertices of a 2 x 2-quad sheet (ties within a mesh), at two coincident instances of
    it (ties across objects: the later object wins), and at a single-triangle mesh"""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.add_material("a", pkg.DiffuseMateral((0.5, 0.5, 0.5)))
    pos, idx = smooth_ref.sheet(2, 2, size=2.0)
    mesh = s.add_mesh("sheet.obj", pkg.Mesh(pos, idx))
    one = s.add_mesh("one.obj", pkg.Mesh(np.float32([[-0.5, 3.0, -0.5], [0.5, 3.0, -0.5], [0.0, 3.0, 0.5]]), np.uint32([0, 2, 1])))
    s.add_object(mesh, glm.identity(), "a")
    s.add_object(mesh, glm.identity(), "a")
    s.add_object(one, glm.identity(), "a")
    flat = s.build_scene(distinct_meshes=True)
    nrm = pkg.compute_vertex_normals(flat)
    targets = [(x, 0.0, z) for x in (-1.0, -0.5, 0.0, 0.5, 1.0) for z in (-1.0, -0.5, 0.0, 0.5, 1.0)]  # vertices, edge midpoints, diagonals
    targets += [(0.25, 0.0, -0.25), (-0.25, 0.0, 0.25), (0.3, 0.0, 0.1)]
    # every ray runs along (0.5, -1, 0.25) from two steps above its target: dyadic numbers throughout, so the triangle tests are exact and
    # two triangles that share the target give the same t (an axis-parallel ray in a box's face plane is the reference's 0 / 0 instead)
    d = np.float32([0.5, -1.0, 0.25])
    targets += [(0.0, 3.0, 0.0), (0.25, 3.0, -0.25), (3.0, 3.0, 3.0)]
    o = np.float32([(x - 1.0, y + 2.0, z - 0.5) for x, y, z in targets])
    got = _query(pkg, orc, flat, _rays(o, np.tile(d, (len(o), 1))), nrm)
    k = len(targets) - 3
    assert np.all(got["object"][:k] == 1)  # of two coincident instances the later one
    assert len(set(got["triangle"][:k].tolist())) == 8 and (got["uv"][:k] == 0.0).sum() >= 25  # vertices and edges, hit exactly
    assert got["object"][k] == 2 and got["triangle"][k] == 0 and got["object"][k + 1] == 2 and got["object"][k + 2] == NONE


SIZES = [(w, h, mb) for w, h in ((33, 17), (65, 33)) for mb in (1, 2, 8)]


@pytest.mark.parametrize("w,h,mb", SIZES)
def test_the_lamp_lit_room(pkg, orc, w, h, mb):
    got = _against_the_loop(pkg, orc, "room", w, h, mb, direct=True)
    assert got["shading_normals"] > 0 and got["shadow_rays"] > 0


@pytest.mark.parametrize("w,h,mb", SIZES)
def test_under_the_sky(pkg, orc, w, h, mb):
    got = _against_the_loop(pkg, orc, "sheet", w, h, mb, env=ENV, env_light=True)
    assert got["shading_normals"] > 0 and got["env_shadow_rays"] > 0


@pytest.mark.parametrize("w,h,mb", SIZES)
def test_both_lights_with_mis(pkg, orc, w, h, mb):
    got = _against_the_loop(pkg, orc, "lamp", w, h, mb, env=ENV, env_light=True, direct=True, mis=True)
    assert got["shading_normals"] > 0 and (got["mis_misses"] > 0 or mb == 1)  # (one bounce: no miss behind a diffuse vertex)


def test_the_open_sheet_absorbs_and_culls(pkg, orc):
    got = _against_the_loop(pkg, orc, "sheet", 65, 33, 8, env=ENV, env_light=True)
    assert all(got[k] > 0 for k in smooth_ref.COUNTERS), {k: got[k] for k in smooth_ref.COUNTERS}


@pytest.mark.parametrize("kind", ["inverted", "zero", "nan"])
def test_hostile_normals(pkg, orc, kind):
    scene, flat, nrm = _scene(pkg, "sheet")
    bad = {"inverted": -nrm, "zero": np.zeros_like(nrm), "nan": nrm.copy()}[kind]
    if kind == "nan":
        bad[smooth_ref.mesh_rows(flat)[1][0] + 5] = np.nan
    got = _against_the_loop(pkg, orc, "sheet", mb=4, env=ENV, env_light=True, normals=bad)
    assert got["fallbacks"] > 0 if kind != "inverted" else got["shading_normals"] > 0


def test_plain_without_any_light(pkg, orc):
    _against_the_loop(pkg, orc, "sheet", mb=4)


def test_a_glass_mesh_and_a_metal_mesh(pkg, orc):
    _against_the_loop(pkg, orc, "glass_metal", mb=8, env=ENV)


def test_an_emissive_mesh(pkg, orc):
    got = _against_the_loop(pkg, orc, "lamp", mb=4, direct=True)
    assert got["shadow_rays"] > 0


def test_roulette_under_the_lens(pkg, orc):
    _against_the_loop(pkg, orc, "room", mb=8, direct=True, roulette=1, lens=LENS)


def test_iteration_2_31_minus_5(pkg, orc):
    _against_the_loop(pkg, orc, "sheet", mb=4, iters=2, iter_begin=2 ** 31 - 5, env=ENV, env_light=True)


def test_two_interleaved_ranks_against_the_one_context_frame(pkg):
    scene, flat, nrm = _scene(pkg, "sheet")
    with _tracer(pkg, flat, normals=nrm, env_light=True) as pt:
        one = _run(pt, scene.camera, ENV)
    parts = []
    for rank in (0, 1):
        with _tracer(pkg, flat, normals=nrm, env_light=True, interleave=(rank, 2, 8)) as pt:
            parts.append(_run(pt, scene.camera, ENV))
        rows = [r for first in range(rank * 8, H, 16) for r in range(first, min(first + 8, H))]
        for p in PLANES:
            assert np.array_equal(_bits(parts[-1][p].reshape(len(rows), W, -1)), _bits(one[p].reshape(H, W, -1)[rows])), (rank, p)
    for k in ("rays",) + OLD + smooth_ref.COUNTERS:
        assert parts[0][k] + parts[1][k] == one[k], k


# ---- 3. what the normals are tied to ------------------------------------------------------------------------------------------------------
def test_normals_set_changed_and_removed(pkg, orc):
    """set, trace 2; other normals, trace 2; none, trace 2; the first again: the restatement continued with prev=.  Then a context that
    never had any gives the bits of the one whose normals were removed"""
    scene, flat, nrm = _scene(pkg, "sheet")
    other = np.roll(nrm, 1, axis=1)
    ref = None
    for k, n in enumerate((nrm, other, None, nrm)):
        ref = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 2 * k, 2, 4, normals=n, smooth=True, prev=ref)
    with _tracer(pkg, flat, mb=4) as pt:
        pt.max_iterations = 8
        for n in (nrm, other, None, nrm):
            pt.vertex_normals = n
            pt.path_trace(scene.camera)
            pt.path_trace(scene.camera)
        _same(_result(pt), ref, PLANES, "normals")
    runs = []
    for had in (True, False):
        with _tracer(pkg, flat, mb=4, normals=nrm if had else None) as pt:
            if had:
                pt.vertex_normals = None
                assert pt._lib.ptc_get_vertex_normals(pt._ctx, None) == 0
            runs.append(_run(pt, scene.camera, None))
    _same(runs[0], runs[1], EVERYTHING, "removed")
    assert runs[0]["shading_normals"] == 0


def test_an_upload_drops_the_normals_and_refusals_keep_them(pkg):
    scene, flat, nrm = _scene(pkg, "sheet")
    with _tracer(pkg, flat, mb=4, normals=nrm) as pt:
        count = C.c_uint32(0)
        assert pt._lib.ptc_get_vertex_normals(pt._ctx, C.byref(count)) == 1 and count.value == len(nrm)
        with pytest.raises(pkg.PtcError) as e:
            pt.vertex_normals = nrm[:-1]
        assert "vertices" in str(e.value) and pt._lib.ptc_get_vertex_normals(pt._ctx, None) == 1 and pt.vertex_normals is not None
        pt.resize_image((W + 2, H))  # a resize does not touch them
        assert pt._lib.ptc_get_vertex_normals(pt._ctx, None) == 1
        pt.create_buffers((W, H), flat)
        assert pt._lib.ptc_get_vertex_normals(pt._ctx, C.byref(count)) == 0 and count.value == 0 and pt.vertex_normals is None
    with pkg.PathTracer(device=0) as pt:
        with pytest.raises(pkg.PtcError) as e:
            pt.vertex_normals = nrm
        assert e.value.code == pkg._capi.PTC_ERR_NO_SCENE


@pytest.mark.parametrize("case", ["param_without_normals", "normals_without_param"])
def test_the_bits_of_the_parent(pkg, case):
    """ "smooth_normals" 1 without normals, and normals with "smooth_normals" 0, render what a context with neither renders"""
    scene, flat, nrm = _scene(pkg, "lamp")
    kw = dict(env_light=True, direct=True, mis=True, roulette=2)
    with _tracer(pkg, flat, smooth=False, **kw) as pt:
        want = _run(pt, scene.camera, ENV)
    with _tracer(pkg, flat, smooth=case == "param_without_normals", normals=nrm if case == "normals_without_param" else None, **kw) as pt:
        got = _run(pt, scene.camera, ENV)
    _same(got, want, EVERYTHING, case)
    assert got["shading_normals"] == 0 and got["fallbacks"] == 0


def test_the_streaming_loop_refuses_and_queues_nothing(pkg):
    scene, flat, nrm = _scene(pkg, "sheet")
    with _tracer(pkg, flat, mega=False, normals=nrm) as pt:
        pt.max_iterations = 4
        for _ in range(2):
            with pytest.raises(pkg._capi.PtcError) as e:
                pt.path_trace(scene.camera)
            assert e.value.code == pkg._capi.PTC_ERR_INVALID and "smooth_normals is rendered by the megakernel" in str(e.value)
        cam = pkg._capi.ptc_camera()
        assert pt._lib.ptc_trace_begin(pt._ctx, C.byref(cam)) == pkg._capi.PTC_ERR_INVALID
        assert pt.iteration() == 0 and pt.stats()["rays_total"] == 0 and pt.stats()["frames"] == 0
        pt.smooth_normals = False  # and without it the context renders as ever
        pt.path_trace(scene.camera)
        assert pt.iteration() == 1 and pt.stats()["rays_total"] > 0
    with pkg.PathTracer(device=0) as pt:
        for bad in (-1, 2):
            with pytest.raises(pkg._capi.PtcError) as e:
                pt.set_param("smooth_normals", bad)
            assert "smooth_normals must be 0 or 1" in str(e.value)


# ---- 4. the command line ----------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_PT = os.path.join(ROOT, "cuda-path-tracer_amd", "host", "hip_pt")


def _read_raw(path):
    data = open(path, "rb").read()
    assert data[:4] == b"PTRF"
    w, h, ch = struct.unpack_from("<III", data, 4)
    assert ch == 7 and len(data) == 16 + 4 * 7 * w * h
    f = np.frombuffer(data, dtype="<f4", offset=16)
    P = w * h
    return {"color": f[:3 * P].reshape(h, w, 3), "normal": f[3 * P:6 * P].reshape(h, w, 3), "depth": f[6 * P:].reshape(h, w)}


def _asset_reference(pkg, orc):
    """the restatement of assets/scenes/cornell_smooth.json (cornell_mesh.json's room with "smooth_normals": true), once for the three runs"""
    if "asset" not in _cache:
        scene = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "cornell_smooth.json"))
        assert scene.smooth_normals is True
        flat = scene.build_scene()
        w, h = scene.resolution
        nrm = smooth_ref.scene_vertex_normals(flat)
        _cache["asset"] = loop_ref.render_megakernel(orc, flat, scene.camera, w, h, 0, 1, 1, normals=nrm, smooth=True)
        assert _cache["asset"]["shading_normals"] > 1000  # (what a run that ignored the option would not reproduce)
    return _cache["asset"]


@pytest.mark.parametrize("scene_file,extra", [("scenes/cornell_mesh.json", ["--smooth-normals"]), ("scenes/cornell_smooth.json", []),
                                              ("scenes/cornell_mesh.json", ["--smooth-normals", "--gpus", "2"])], ids=["flag", "scene_key", "two_ranks"])
def test_hip_pt_smooth_normals_against_the_restatement(pkg, orc, tmp_path, scene_file, extra):
    """hip_pt --method megakernel with --smooth-normals, with the scene key, and over two ranks: the float framebuffers the run dumps are
    the restatement's with the host's vertex normals"""
    if not os.path.exists(HIP_PT):
        subprocess.run(["make"], cwd=os.path.dirname(HIP_PT), check=True, stdout=subprocess.DEVNULL)
    want = _asset_reference(pkg, orc)
    raw = tmp_path / "out.raw"
    cmd = [HIP_PT, scene_file, "-o", str(tmp_path / "out.png"), "--spp", "1", "--max-bounces", "1", "--dump-raw", str(raw), "--method", "megakernel"] + extra
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    _same(_read_raw(raw), want, PLANES, extra)
