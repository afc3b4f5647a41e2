"""ptc_upload_scene as a whole: the context's scene state is assigned in ONE place, after the last step that
can fail, and every refusal that the caller's arrays decide leaves the scene uploaded before in place.  Three checks on tiny
scenes: a re-upload leaves nothing of the scene before behind; each kind of host-decided refusal keeps the old scene; the
three sources of the reference BVH and the two of the layouts end in the same state for a scene of two meshes."""
import copy

import numpy as np
import pytest

import bvh_meshes as bm
import bvh_shapes as bs
from test_gpu_bvh_hostile import _two_instances
from test_gpu_mesh_limits import _malformed
from test_gpu_multimesh import _scene as _two_mesh_scene

pytestmark = pytest.mark.gpu

W, H, ITERS, MB = 64, 48, 3, 4
BUFFERS = ("color", "normal", "depth")
STATS = ("bvh_node_count", "bvh_max_depth", "triangle_count", "stack_capacity", "rays_total", "last_live")


def _trace(pt, camera, iters=ITERS):
    for _ in range(iters):
        pt.path_trace(camera)
    return {k: pt.download(k) for k in BUFFERS}


def _layouts(pt):
    return {k: pt.download_layout(k) for k in pt.LAYOUTS}


def _stats(pt, layouts):
    """ptc_get_stats' view of the scene; the count of four-wide nodes -- of mesh 0, the one ptc_download_layout shows -- is
    what that call reports of them (64 bytes each)"""
    s = pt.stats()
    return {**{k: s[k] for k in STATS}, "four_wide_nodes": len(layouts["bvh4q"]) // 64}


def _same_arrays(got, want, what):
    assert got.keys() == want.keys(), what
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


# ---- 1. a re-upload leaves nothing behind ---------------------------------------------------------------------------------

def _scene_a(pkg):
    """the box and its three balls in front of two instances of one mesh -- the second one a lamp -- and a sphere lamp"""
    glm = pkg.glmlite
    sc = pkg.scenes.cornell_spheres((W, H))
    mesh = sc.add_mesh("grid", pkg.scenes.heightfield_mesh(9, 5, 2.0, 1.0, seed=1))
    sc.add_material("grid", pkg.DiffuseMateral((0.8, 0.3, 0.2)))
    sc.add_material("panel", pkg.EmissiveMaterial((6.0, 6.0, 5.5)))
    sc.add_material("lamp", pkg.EmissiveMaterial((4.0, 3.6, 3.0)))
    sc.add_object(mesh, glm.translate((0.0, -0.8, 0.6)), "grid")
    sc.add_object(mesh, glm.compose([glm.scale(0.5), glm.translate((0.0, 1.2, -0.5))]), "panel")
    sc.add_object(pkg.Sphere((0, 0, 0), 0.25), glm.translate((0.9, 1.0, -1.2)), "lamp")
    return sc


def _upload_and_look(pt, sc, flat, points, normals):
    pt.create_buffers((W, H), flat)
    pt.max_iterations = ITERS
    out = {"image": _trace(pt, sc.camera), "layouts": _layouts(pt), "light_info": pt.light_info()}
    out["stats"] = _stats(pt, out["layouts"])
    radiance, rays, visible = pt.direct_light(points, normals, sample_index=1, want_rays=True)
    out["direct"] = {"radiance": radiance, "rays": rays, "visible": visible}
    return out


def _same_state(got, want, what):
    for k in ("image", "layouts", "direct"):
        _same_arrays(got[k], want[k], (what, k))
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
    assert got["light_info"] == want["light_info"], (what, got["light_info"], want["light_info"])


def test_reupload_in_one_context_leaves_nothing_behind(pkg):
    """A, B, A in one context: the first and the third state agree bit for bit, and B is B of a fresh context -- images, stats,
    lamp info, the five layout arrays and a direct-light query.  A has a mesh, lamps and ten objects; B has none of them and seven
    objects, so whatever the commit forgot of A would show in B, and of B in the second A."""
    a, b = _scene_a(pkg), pkg.scenes.cornell_spheres((W, H))
    flat_a, flat_b = a.build_scene(), b.build_scene()
    assert len(flat_a.objects) == 10 and len(flat_b.objects) == 7 and len(flat_b.indices) == 0
    rng = np.random.default_rng(3)
    points = np.c_[rng.uniform(-1.5, 1.5, 12), np.full(12, -0.99), rng.uniform(-1.5, 1.0, 12)].astype(np.float32)
    normals = np.tile(np.array([0.0, 1.0, 0.0], dtype=np.float32), (12, 1))
    with pkg.PathTracer(device=0, max_bounces=MB) as pt:
        first_a = _upload_and_look(pt, a, flat_a, points, normals)
        then_b = _upload_and_look(pt, b, flat_b, points, normals)
        again_a = _upload_and_look(pt, a, flat_a, points, normals)
    with pkg.PathTracer(device=0, max_bounces=MB) as pt:
        fresh_b = _upload_and_look(pt, b, flat_b, points, normals)
    assert first_a["light_info"]["sphere_lights"] == 1 and first_a["light_info"]["triangle_lights"] == 64
    assert first_a["stats"]["triangle_count"] == 64 and first_a["stats"]["four_wide_nodes"] > 0
    assert first_a["direct"]["visible"].any() and first_a["direct"]["radiance"].any()
    assert then_b["stats"]["triangle_count"] == 0 and then_b["light_info"]["lights"] == 0 and not then_b["direct"]["radiance"].any()
    _same_state(again_a, first_a, "A after B")
    _same_state(then_b, fresh_b, "B after A")


# ---- 2. refusals the host decides keep the old scene ----------------------------------------------------------------------

def _refusals(pkg, sc, good, broken_trees):
    """(name, scene, status, words of the message): one upload per kind of refusal that the caller's arrays decide"""
    capi = pkg._capi
    bad = copy.copy(good)
    bad.object_material_indices = good.object_material_indices.copy()
    bad.object_material_indices[-1] = len(good.materials)
    yield "material_index", bad, capi.PTC_ERR_INVALID, ("material index out of range",)
    bad = copy.copy(good)
    bad.materials = good.materials.copy()
    bad.materials["type"][1] = 3
    bad.materials["p"][1] = (1.0, -0.5, 1.0, 0.0)
    yield "negative_emission", bad, capi.PTC_ERR_INVALID, ("material 1: emission must be finite and >= 0",)
    tree, node = broken_trees["child_outside_parent"]      # the scenes of test_caller_trees_that_break_a_rule_are_refused
    yield "caller_tree", sc.build_scene(prebuilt_bvh=tree), capi.PTC_ERR_INVALID, (f"BVH node {node}:", "not inside its parent")
    bad = copy.copy(good)
    bad.positions = good.positions.copy()
    vertex = int(good.indices[4])
    bad.positions[vertex, 1] = np.nan
    yield "nan_vertex", bad, capi.PTC_ERR_INVALID, (f"mesh 0: vertex {vertex} has a NaN or infinite coordinate",)
    # 3000 denormal triangles: the SAH cost is NaN at every node and the tree comes out deeper than the stack
    deep = _two_instances(pkg, pkg.Mesh(*bm.family("denormal", 3000))).build_scene()
    yield "deep_tree", deep, capi.PTC_ERR_STACK, ("exceeds the traversal stack",)
    # 32,768 instances of 65,536 triangles: 32,768 x 65,537 = 2,147,516,416 records > 2^31 - 1, refused before anything of
    # that size is allocated
    one = pkg.SceneDescription()
    one.add_material("m", pkg.DiffuseMateral((0.5, 0.5, 0.5)))
    grid = one.add_mesh("grid", pkg.scenes.heightfield_mesh(257, 129, 8.0, 4.0, seed=3))
    one.add_object(grid, pkg.glmlite.identity(), "m")
    many = one.build_scene()
    assert len(many.indices) // 3 == 65_536
    many.objects = np.repeat(many.objects, 32_768)
    many.object_material_indices = np.zeros(32_768, dtype=np.uint32)
    yield "instance_triangles", many, capi.PTC_ERR_OOM, ("too many instance triangles",)


def test_refusals_decided_on_the_host_keep_the_old_scene(pkg):
    """After each refused upload: code and message as ever, the five layout arrays of the scene uploaded before unchanged, and
    the next frames, stats, lamp info and direct-light query those of a context that never saw the refusal (both contexts go
    on accumulating).  The good scene is the room of test_caller_trees_that_break_a_rule_are_refused with a sphere lamp."""
    sc, broken_trees = _malformed(pkg)
    sc.add_material("lamp", pkg.EmissiveMaterial((4.0, 3.6, 3.0)))
    sc.add_object(pkg.Sphere((0, 0, 0), 0.25), pkg.glmlite.translate((0.5, 1.5, 0.0)), "lamp")
    rng = np.random.default_rng(5)
    points = np.c_[rng.uniform(-1.5, 1.5, 12), np.full(12, -0.99), rng.uniform(-1.5, 1.5, 12)].astype(np.float32)
    normals = np.tile(np.array([0.0, 1.0, 0.0], dtype=np.float32), (12, 1))

    def lamps(p):
        radiance, rays, visible = p.direct_light(points, normals, sample_index=2, want_rays=True)
        return p.light_info(), {"radiance": radiance, "rays": rays, "visible": visible}

    good = sc.build_scene(prebuilt_bvh=pkg.bvh_from_mesh(list(sc.mesh_map_.values())[0])[0])
    cases = list(_refusals(pkg, sc, good, broken_trees))
    assert [c[0] for c in cases] == ["material_index", "negative_emission", "caller_tree", "nan_vertex", "deep_tree", "instance_triangles"]
    with pkg.PathTracer(device=0, max_bounces=MB) as ctl, pkg.PathTracer(device=0, max_bounces=MB) as pt:
        for p in (ctl, pt):
            p.create_buffers((W, H), good)
            p.max_iterations = ITERS * (len(cases) + 1)
        _same_arrays(_trace(pt, sc.camera), _trace(ctl, sc.camera), "before any refusal")
        before, ctl_layouts = _layouts(pt), _layouts(ctl)
        _same_arrays(before, ctl_layouts, "before any refusal")
        info, direct = lamps(ctl)
        assert len(before["bvh"]) > 0 and info["sphere_lights"] == 1 and direct["visible"].any() and direct["radiance"].any()
        for name, flat, status, words in cases:
            with pytest.raises(pkg.PtcError) as e:
                pt.create_buffers((W, H), flat)
            assert e.value.code == status, (name, str(e.value))
            for w in words:
                assert w in str(e.value), (name, str(e.value))
            after = _layouts(pt)
            _same_arrays(after, before, name)
            _same_arrays(_trace(pt, sc.camera), _trace(ctl, sc.camera), name)
            assert _stats(pt, after) == _stats(ctl, ctl_layouts), name
            got_info, got_direct = lamps(pt)
            assert got_info == info, (name, got_info, info)
            _same_arrays(got_direct, direct, (name, "direct light"))
        assert pt.iteration() == ctl.iteration() == ITERS * (len(cases) + 1)


# ---- 3. three BVH sources x two layout sources, two meshes --------------------------------------------------------------

def test_every_bvh_and_layout_source_commits_the_same_state(pkg):
    """A scene of two meshes (three mesh objects behind a box of spheres) with the callers' trees, the device builder and the host
    builder, each with the layouts from the device and from the host, and with the second mesh's tree numbered depth-first (that mesh
    alone goes to the host layouts): equal layout bytes, images and stats, and the flags of ptc_upload_times as the parameters say."""
    scene, a, b = _two_mesh_scene(pkg, (W, H))
    bare = scene.build_scene(distinct_meshes=True)
    trees = [pkg.bvh_from_mesh(m)[0] for m in (a, b)]

    def with_trees(first, second):
        flat = copy.copy(bare)
        flat.bvh = np.concatenate([first, second])
        flat.mesh_ranges = bare.mesh_ranges.copy()
        flat.mesh_ranges[0, 4:6] = (0, len(first))
        flat.mesh_ranges[1, 4:6] = (len(first), len(second))
        return flat

    caller = with_trees(*trees)
    renumbered = with_trees(trees[0], bs.depth_first(trees[1]))
    assert not np.array_equal(renumbered.bvh.view(np.uint8), caller.bvh.view(np.uint8))
    # (name, scene, bvh_build_on_device, layout_on_device, the flags expected of ptc_upload_times)
    variants = [(f"{name}/layouts_{'device' if lay else 'host'}", flat, build, lay, (flag, lay))
                for name, flat, build, flag in (("caller", caller, 1, 0), ("device", bare, 1, 1), ("host", bare, 0, 0))
                for lay in (1, 0)]
    variants.append(("caller_depth_first/layouts_device", renumbered, 1, 1, (0, 1)))   # mesh 0 on the device, mesh 1 on the host
    want = None
    for name, flat, build, lay, flags in variants:
        with pkg.PathTracer(device=0, max_bounces=MB) as pt:
            pt.set_param("bvh_build_on_device", build)
            pt.set_param("layout_on_device", lay)
            pt.create_buffers((W, H), flat)
            pt.max_iterations = ITERS
            times = pt.upload_times()
            assert (times["bvh_on_device"], times["layout_on_device"]) == flags, (name, times)
            layouts = _layouts(pt)
            got = {"image": _trace(pt, scene.camera), "layouts": layouts, "stats": _stats(pt, layouts)}
        if want is None:
            want = got
            assert got["stats"]["triangle_count"] == a.triangle_count() + b.triangle_count()
            continue
        _same_arrays(got["image"], want["image"], name)
        _same_arrays(got["layouts"], want["layouts"], name)
        assert got["stats"] == want["stats"], (name, got["stats"], want["stats"])
