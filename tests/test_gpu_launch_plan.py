"""The launch plan of a bounce (ptcore_trace.cpp) and the parameter table (ptc_set_param), seen through what the library
reports: profile()'s trace_launches[b] (one HIP event pair per traversal launch while launches are timed), listed_rays[b]
(rays the traversal launches of bounce b fetched through a work list) and persist_launches.

The plan of the default variant, by object list (S a sphere, A / B instances of two meshes, E an instance of an empty mesh):
a mesh instance is a traversal launch; consecutive instances of one mesh with nothing between them share a launch
("merge_instances"); an instance of an empty mesh is no launch, but it parts a run; a sphere run in front of a launch lists
that launch's rays ("filter_rays") unless the rays are sorted; bounce 0's first launch is listed by ray generation when
nothing is in front of it; the variants 0 / 1 walk the whole list in one kernel per bounce and list nothing.  `plan` below
is that model; the expectations were checked against the library before its launch plan was rewritten."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, MB, ITERS = 64, 48, 3, 3
SHAPES = ["A", "AS", "SSA", "SAASBS", "AAA", "AEA", "SESA", "SS"]


def plan(shape, merge=True):
    """The traversal launches of one bounce: per launch, is a sphere run in front of it?"""
    front, spheres, prev = [], False, None
    for i, c in enumerate(shape):
        if c == "S":
            spheres = True
        elif c != "E":
            if not (merge and not spheres and prev == (c, i - 1)):
                front.append(spheres)
            spheres, prev = False, (c, i)
    return front


def lists(shape, bounce, merge=True, filter_rays=True, ray_sort=False):
    """Does a traversal launch of this bounce fetch through a work list?"""
    front = plan(shape, merge)
    if not filter_rays or not front:
        return False
    behind_spheres = any(front) and not (ray_sort and bounce >= 1)
    return behind_spheres or (bounce == 0 and not front[0])


def _scene(pkg, shape):
    """The objects of `shape` side by side in front of the camera; the first sphere is the floor they stand on."""
    glm = pkg.glmlite
    sc = pkg.SceneDescription()
    meshes = {"A": pkg.scenes.displaced_sphere_mesh(4, 8),                       # 64 triangles
              "B": pkg.scenes.heightfield_mesh(5, 4, 1.0, 0.6, seed=3),          # 24 triangles
              "E": pkg.Mesh(np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), aabb=(np.zeros(3, np.float32), np.zeros(3, np.float32)))}
    floor = False
    for i, c in enumerate(shape):
        x = (i - (len(shape) - 1) / 2.0) * 0.8
        name = f"m{i}"
        sc.add_material(name, pkg.MetalMaterial((0.8, 0.7, 0.6), 0.3) if i % 2 else pkg.DiffuseMateral((0.3 + 0.1 * i, 0.6, 0.5)))
        if c == "S" and not floor:
            floor = True
            sc.add_object(pkg.Sphere((0, 0, 0), 1000.0), glm.translate((0.0, -1001.0, 0.0)), name)
        elif c == "S":
            sc.add_object(pkg.Sphere((0, 0, 0), 0.3), glm.translate((x, -0.7, 0.0)), name)
        elif c == "A":
            sc.add_object(meshes[c], glm.compose([glm.scale(0.7), glm.translate((x, -0.6, 0.0))]), name)
        else:
            sc.add_object(meshes[c], glm.translate((x, -0.5, 0.0)), name)
    sc.camera = pkg.Camera(position=(0.0, 0.0, 3.5), vfov=0.9)
    return sc, sc.build_scene(distinct_meshes=True)


def _render(pkg, scene, flat, params=(), variant=3, iters=ITERS):
    with pkg.PathTracer(device=0, max_bounces=MB) as pt:
        for k, v in params:
            pt.set_param(k, v)
        pt.create_buffers((W, H), flat)
        pt.set_trace_variant(variant)
        pt.set_profiling(time_trace_kernel=True)
        pt.max_iterations = iters
        for _ in range(iters):
            pt.path_trace(scene.camera)
        out = {k: pt.download(k) for k in ("color", "normal", "depth")}
        out["profile"] = pt.profile()
    return out


ONE = (("frames_in_flight", 1),)   # every iteration a batch of its own: ITERS batches
# knob settings: (what, parameters, variant, batches, arguments of the model)
KNOBS = [("default", ONE, 3, ITERS, {}),
         ("merge_instances 0", ONE + (("merge_instances", 0),), 3, ITERS, {"merge": False}),
         ("filter_rays 0", ONE + (("filter_rays", 0),), 3, ITERS, {"filter_rays": False}),
         ("prefold 0", ONE + (("prefold", 0),), 3, ITERS, {}),
         ("fused_shade 0", ONE + (("fused_shade", 0),), 3, ITERS, {}),
         ("ray_sort 1", ONE + (("ray_sort", 1),), 3, ITERS, {"ray_sort": True}),
         ("variant 0", ONE, 0, ITERS, None),
         ("variant 1", ONE, 1, ITERS, None),
         # batches of two frames on three slots: iterations 0 and 1 share a batch, iteration 2 goes out alone with the download
         ("batches of 2", (("frames_in_flight", 6), ("batch_frames", 2)), 3, 2, {})]


def _check(got, shape, what, batches, model):
    prof = got["profile"]
    if model is None:   # the variants 0 / 1: one kernel per bounce, nothing listed
        want_launches, want_listed = [batches] * MB, [False] * MB
    else:
        runs = len(plan(shape, model.get("merge", True)))
        want_launches = [batches * runs] * MB
        want_listed = [lists(shape, b, **model) for b in range(MB)]
    assert prof["trace_launches"] == want_launches, (shape, what, prof["trace_launches"])
    assert [n != 0 for n in prof["listed_rays"]] == want_listed, (shape, what, prof["listed_rays"])
    assert prof["persist_launches"] == 0, (shape, what)


@pytest.mark.parametrize("shape", SHAPES)
def test_launches_and_lists_of_the_plan(pkg, shape):
    scene, flat = _scene(pkg, shape)
    base = None
    for what, params, variant, batches, model in KNOBS:
        got = _render(pkg, scene, flat, params, variant)
        _check(got, shape, what, batches, model)
        base = base or got
        for k in ("color", "normal", "depth"):
            assert np.array_equal(got[k], base[k]), (shape, what, k)
    assert base["color"].std() > 0


@pytest.mark.parametrize("shape", SHAPES)
def test_persistent_launch_only_where_the_plan_allows_it(pkg, shape):
    """ "persist" 1, two batches of two frames.  One mesh object with nothing in front of it (a sphere run may end the list):
    per batch bounce 0's traversal launch, reported with bounce 0, and the persistent launch, reported with bounce 1.  Any
    other plan keeps the per-bounce launches."""
    scene, flat = _scene(pkg, shape)
    base = _render(pkg, scene, flat, ONE, iters=4)
    got = _render(pkg, scene, flat, (("persist", 1), ("frames_in_flight", 2), ("batch_frames", 2)), iters=4)
    prof = got["profile"]
    if shape in ("A", "AS"):
        assert prof["persist_launches"] == 2
        assert prof["trace_launches"] == [2, 2] + [0] * (MB - 2), prof["trace_launches"]
        assert [n != 0 for n in prof["listed_rays"]] == [True] + [False] * (MB - 1), prof["listed_rays"]   # ray generation's list; nothing after it
    else:
        _check(got, shape, "persist 1", 2, {})
    for k in ("color", "normal", "depth"):
        assert np.array_equal(got[k], base[k]), (shape, k)


# ---- ptc_set_param ---------------------------------------------------------------------------------------------------
INT_MIN, INT_MAX = -2**31, 2**31 - 1
RESIZE, UPLOAD = "ptc_resize", "ptc_upload_scene"
# name: (lowest, highest, the refusal of a value outside them, what it must be set before)
# (debug_lds_entries: 24 is PT_T4_LDS of the default build, pt_device.hpp -- a library built with another value has another bound)
PARAMS = {
    "batch_frames": (1, 32, "batch_frames must be in [1,32]", RESIZE),
    "traverse_waves": (8, 65536, "traverse_waves out of range", UPLOAD),
    "debug_lds_entries": (1, 24, "debug_lds_entries must be in [1,24]", UPLOAD),
    "debug_force_slow": (INT_MIN, INT_MAX, None, None),
    "debug_shade_epoch": (0, 0x3FFFFFFF, "debug_shade_epoch must be in [0,1073741823]", None),
    "layout_on_device": (0, 1, "layout_on_device must be 0 or 1", None),
    "filter_rays": (0, 1, "filter_rays must be 0 or 1", None),
    "fused_shade": (0, 1, "fused_shade must be 0 or 1", None),
    "merge_instances": (0, 1, "merge_instances must be 0 or 1", None),
    "bvh_build_on_device": (0, 1, "bvh_build_on_device must be 0 or 1", None),
    "static_eighths": (0, 8, "static_eighths must be in [0,8]", None),
    "small_waves": (8, 65536, "small_waves out of range", None),
    "small_rays_per_lane": (0, 1024, "small_rays_per_lane out of range", None),
    "run_waves": (8, 65536, "run_waves out of range", None),
    "min_waves": (8, 65536, "min_waves out of range", None),
    "beam": (0, 1, "beam must be 0 or 1", RESIZE),
    "persist": (0, 1, "persist must be 0 or 1", None),
    "persist_service_every": (2, 64, "persist_service_every must be in [2, 64]", None),
    "prefold": (0, 1, "prefold must be 0 or 1", RESIZE),
    "pair_batches": (0, 1, "pair_batches must be 0 or 1", None),
    "persist_help_tiles": (0, 4096, "persist_help_tiles must be in [0, 4096]", None),
    "persist_min_frames": (1, 32, "persist_min_frames must be in [1, 32]", None),
    "sphere_fold": (0, 1, "sphere_fold must be 0 or 1", None),
    "sphere_lanes": (0, 1, "sphere_lanes must be 0 or 1", None),
    "split_idle": (0, 64, "split_idle must be in [0,64]", None),
    "refill_lanes": (1, 64, "refill_lanes must be in [1,64]", None),
    "ray_sort": (0, 1, "ray_sort must be 0 or 1", RESIZE),
    "denoise_variant": (0, 1, "denoise_variant must be 0 or 1", None),
    "slot_offset": (0, INT_MAX, "slot_offset must not be negative", None),
    "frames_in_flight": (1, 256, "frames_in_flight must be in [1,256]", RESIZE),
}


def _set(pkg, pt, name, value):
    """(return code, ptc_last_error after a refusal) of ptc_set_param"""
    lib = pkg._capi.lib()
    rc = lib.ptc_set_param(pt._ctx, name.encode(), C.c_int(value))
    return rc, (lib.ptc_last_error(pt._ctx) if rc else None)


def _outside(lo, hi):
    return [v for v in (lo - 1, hi + 1) if INT_MIN <= v <= INT_MAX]


def test_every_parameter_at_the_ends_of_its_range(pkg):
    assert len(PARAMS) == 30
    invalid = pkg._capi.PTC_ERR_INVALID
    with pkg.PathTracer(device=0, max_bounces=MB) as pt:   # no scene, no frame: every gate is open
        for name, (lo, hi, refusal, _) in PARAMS.items():
            for v in _outside(lo, hi):
                assert _set(pkg, pt, name, v) == (invalid, refusal.encode()), (name, v)
            for v in (lo, hi):
                assert _set(pkg, pt, name, v) == (0, None), (name, v)
        assert _set(pkg, pt, "no_such_knob", 1) == (invalid, b"unknown parameter no_such_knob")
        assert pkg._capi.lib().ptc_set_param(pt._ctx, None, 1) == invalid
    assert pkg._capi.lib().ptc_set_param(None, b"beam", 1) == invalid


def test_refusals_leave_a_working_context(pkg):
    """After ptc_upload_scene and ptc_resize: the range is checked before the gate, a gated parameter is refused whatever its
    value, and the context traces the same frame after every refusal."""
    invalid = pkg._capi.PTC_ERR_INVALID
    scene, flat = _scene(pkg, "SAS")
    with pkg.PathTracer(device=0, max_bounces=MB) as pt:
        pt.create_buffers((32, 32), flat)
        pt.max_iterations = 1

        def frame():
            pt.restart()
            pt.path_trace(scene.camera)
            return pt.download("color")

        first = frame()
        assert first.std() > 0
        refusals = []
        for name, (lo, hi, refusal, gate) in PARAMS.items():
            refusals += [(name, v, refusal) for v in _outside(lo, hi)]
            if gate:
                refusals += [(name, v, f"set {name} before {gate}") for v in (lo, hi)]
        refusals.append(("no_such_knob", 0, "unknown parameter no_such_knob"))
        assert len(refusals) == 2 * 28 + 1 + 2 * 7 + 1
        for name, v, refusal in refusals:
            assert _set(pkg, pt, name, v) == (invalid, refusal.encode()), (name, v)
            assert np.array_equal(frame(), first), (name, v)
