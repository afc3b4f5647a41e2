"""The GPU BVH builder (pt_bvh_gpu.hip) on the hostile meshes of tests/bvh_meshes.py: signed zeros, zero areas, denormal
and near-FLT_MAX coordinates, clustered soups (deep and wide), every triangle count from 1 to 400, shared and permuted
vertices, 2,109,440 triangles, vertices that are not finite.  The device tree is held to the host builder's and the
oracle's, byte for byte (as values where a mesh holds both zeros), and to the independent check of
tests/bvh_tree_check.py; the traversal layouts built on the device to the host's; small frames and rays to the oracle.
tests/test_bvh_meshes_cpu.py holds host builder == oracle and the conditions on the inputs without a GPU."""
import copy
import ctypes as C

import numpy as np
import pytest

import bvh_meshes as bm
from bvh_tree_check import check_tree

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
W, H, ITERS, MB = 64, 48, 3, 6
BOTH_ZEROS = ("signed_zeros",)     # the families whose coordinates hold -0.0 and +0.0


def _mesh(pkg, pos, idx, aabb=None):
    return pkg.Mesh(pos, idx, aabb=aabb)


def _same_tree(name, got, want, both_zeros):
    """bytes; for a mesh with both zeros: equal as values, and a bound whose bits differ is a zero in both"""
    assert len(got) == len(want), name
    for k in ("first_child_or_primitive", "primitive_count"):
        assert np.array_equal(got[k], want[k]), (name, k)
    if not both_zeros:
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), name
        return 0
    differing = 0
    for k in ("aabb_min", "aabb_max"):
        assert np.array_equal(got[k], want[k]), (name, k)
        other = got[k].view(np.uint32) != want[k].view(np.uint32)
        assert (got[k][other] == 0).all() and (want[k][other] == 0).all(), (name, k)
        differing += int(other.sum())
    return differing


def test_device_builder_on_every_finite_family(pkg, orc):
    sign_differences = 0
    with pkg.PathTracer() as pt:
        for name, pos, idx in bm.finite_cases():
            both = name.startswith(BOTH_ZEROS)
            mesh = _mesh(pkg, pos, idx)
            got, got_depth = pt.build_bvh(mesh)
            host, host_depth = pkg.bvh_from_mesh(mesh)
            ref, ref_depth = orc.build_bvh(pos, idx)
            assert got_depth == host_depth == ref_depth, name
            assert np.array_equal(host.view(np.uint8), ref.view(np.uint8)), name
            sign_differences += _same_tree(name, got, host, both)
            res = check_tree(got, pos, idx, reported_depth=got_depth, bits=not both)
            assert res.ok(), (name, res.errors)
    print(f"signed_zeros: {sign_differences} zero bounds differ in sign between the device and the host tree")


def test_every_count_in_one_context(pkg, orc):
    """400 builds in one context, 1 to 400 triangles (the builder switches at 2, 4/5 and 32/33); then big, tiny, big in
    the same context: nothing of an earlier build shows in a later one"""
    with pkg.PathTracer() as pt:
        for t in bm.EVERY_COUNT:
            pos, idx = bm.every_count(t)
            mesh = _mesh(pkg, pos, idx)
            got, got_depth = pt.build_bvh(mesh)
            host, host_depth = pkg.bvh_from_mesh(mesh)
            ref, ref_depth = orc.build_bvh(pos, idx)
            assert len(got) == 2 * t - 1 and got_depth == host_depth == ref_depth, t
            assert np.array_equal(got.view(np.uint8), host.view(np.uint8)), t
            assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), t
        big = _mesh(pkg, *bm.family("clustered", 20_000))
        big_host, big_depth = pkg.bvh_from_mesh(big)
        for mesh in (big, _mesh(pkg, *bm.every_count(1)), big, _mesh(pkg, *bm.every_count(2)), _mesh(pkg, *bm.every_count(3)),
                     _mesh(pkg, *bm.every_count(33)), big, _mesh(pkg, *bm.family("planar", 3000)), _mesh(pkg, *bm.every_count(5))):
            got, got_depth = pt.build_bvh(mesh)
            host, host_depth = (big_host, big_depth) if mesh is big else pkg.bvh_from_mesh(mesh)
            assert got_depth == host_depth and np.array_equal(got.view(np.uint8), host.view(np.uint8)), mesh.triangle_count()


def _layouts(pkg, flat, bvh_on_device, layout_on_device, size=(W, H)):
    with pkg.PathTracer() as pt:
        pt.set_param("layout_on_device", layout_on_device)
        pt.set_param("bvh_build_on_device", bvh_on_device)
        pt.create_buffers(size, flat)
        t = pt.upload_times()
        assert t["layout_on_device"] == layout_on_device and t["bvh_on_device"] == bvh_on_device
        return {k: pt.download_layout(k) for k in pt.LAYOUTS}, pt.stats()


# the 32-bit words of one record that hold a box bound (binary32); every other word is a reference, a count or a code
# ("bvh" is the device's copy of the reference nodes: {min.xyz, first}, {max.xyz, count})
_BOUND_WORDS = {"bvh": (8, (0, 1, 2, 4, 5, 6)), "leaf_parent": (4, (0, 1, 2)), "wide": (16, tuple(range(12))), "bvh4q": (16, (0, 1, 2))}


def _same_layouts(name, dev, host, both_zeros):
    for k in dev:
        assert dev[k].shape == host[k].shape, (name, k)
        if not both_zeros or k == "tris":
            assert np.array_equal(dev[k], host[k]), (name, k)
            continue
        # both zeros: the words that differ hold a box bound, and hold a zero on both sides
        record, bounds = _BOUND_WORDS[k]
        a, b = dev[k].view(np.uint32).reshape(-1, record), host[k].view(np.uint32).reshape(-1, record)
        other = a != b
        is_bound = np.zeros(record, dtype=bool)
        is_bound[list(bounds)] = True
        assert not other[:, ~is_bound].any(), (name, k)
        assert ((a[other] & 0x7fffffff) == 0).all() and ((b[other] & 0x7fffffff) == 0).all(), (name, k)


def _two_instances(pkg, mesh):
    glm = pkg.glmlite
    sc = pkg.SceneDescription()
    sc.add_material("m", pkg.DiffuseMateral((0.5, 0.5, 0.5)))
    sc.add_mesh("mesh", mesh)
    sc.add_object(mesh, glm.compose([glm.translate((0.5, -1.0, 2.0))]), "m")
    sc.add_object(mesh, glm.compose([glm.rotate(np.float32(0.6), (0.3, 1.0, 0.2)), glm.scale((0.7, 0.4, 0.9))]), "m")
    return sc


def test_device_layouts_equal_host_layouts_on_every_finite_family(pkg):
    """every kind of ptc_download_layout, one plain and one rotated, unevenly scaled instance: the device's layouts of the
    HOST tree are the host's bytes for every family; device tree + device layouts against host tree + host layouts are the
    same bytes too, except that a mesh with both zeros may differ in the sign of a zero bound and nowhere else.  3000
    denormal or huge triangles come out deeper than the traversal stack (the SAH cost is NaN at every node: split 0):
    their upload is refused alike on both sides, and they are compared at 1000."""
    for family in bm.FAMILIES:
        for n in (300, 1000, 3000):
            if n == 1000 and family not in ("denormal", "huge"):
                continue
            name = f"{family}{n}"
            flat = _two_instances(pkg, _mesh(pkg, *bm.family(family, n))).build_scene()
            if n == 3000 and family in ("denormal", "huge"):
                for on_device in (1, 0):
                    with pytest.raises(pkg.PtcError) as e:
                        _layouts(pkg, flat, on_device, on_device)
                    assert e.value.code == pkg._capi.PTC_ERR_STACK, name
                continue
            host, host_stats = _layouts(pkg, flat, 0, 0)
            mixed, mixed_stats = _layouts(pkg, flat, 0, 1)
            dev, dev_stats = _layouts(pkg, flat, 1, 1)
            _same_layouts(name, mixed, host, False)
            _same_layouts(name, dev, host, family in BOTH_ZEROS)
            for s in (mixed_stats, dev_stats):
                assert s["bvh_node_count"] == host_stats["bvh_node_count"] and s["stack_capacity"] == host_stats["stack_capacity"], name
                assert s["bvh_max_depth"] == host_stats["bvh_max_depth"], name


def test_over_2_20(pkg):
    """2,109,440 triangles: the partition flags' scan and the scan over one level's nodes (1,139,268 of them) recurse
    twice; the tree is the host's bytes and right by itself, the layouts are the host's bytes"""
    pos, idx = bm.over_2_20(pkg.scenes)
    mesh = _mesh(pkg, pos, idx)
    host, host_depth = pkg.bvh_from_mesh(mesh)
    with pkg.PathTracer() as pt:
        got, got_depth = pt.build_bvh(mesh)
    assert len(got) == 2 * 2_109_440 - 1 and got_depth == host_depth
    assert np.array_equal(got.view(np.uint8), host.view(np.uint8))
    res = check_tree(got, pos, idx, reported_depth=got_depth, bits=True)
    assert res.ok(), res.errors
    assert np.diff(res.level_base).max() > 1_048_576
    del got, host, res
    sc = pkg.SceneDescription()
    sc.add_material("m", pkg.DiffuseMateral((0.5, 0.5, 0.5)))
    sc.add_mesh("mesh", mesh)
    sc.add_object(mesh, pkg.glmlite.identity(), "m")
    flat = sc.build_scene()
    dev, _ = _layouts(pkg, flat, 1, 1)
    host, _ = _layouts(pkg, flat, 0, 0)
    assert len(dev["bvh"]) == (2 * 2_109_440 - 1) * 32 and len(dev["tris"]) == (2_109_440 + 1) * 64
    for k in dev:
        assert np.array_equal(dev[k], host[k]), k


# ---- images and rays ------------------------------------------------------------------------------------------------

def _image_scene(pkg, mesh, camera):
    """the mesh twice (plain; rotated and unevenly scaled) in front of four wall spheres, so that paths go on bouncing"""
    glm = pkg.glmlite
    sc = pkg.SceneDescription()
    sc.add_material("a", pkg.DiffuseMateral((0.7, 0.6, 0.5)))
    sc.add_material("b", pkg.MetalMaterial((0.8, 0.8, 0.9), 0.1))
    big = 1000.0
    for off in ((0.0, -big - 6.0, 0.0), (0.0, 0.0, -big - 8.0), (-big - 8.0, 0.0, 0.0), (big + 8.0, 0.0, 0.0)):
        sc.add_object(pkg.Sphere((0.0, 0.0, 0.0), big), glm.translate(off), "a")
    sc.add_mesh("mesh", mesh)
    sc.add_object(mesh, glm.identity(), "a")
    sc.add_object(mesh, glm.compose([glm.translate((0.4, 0.3, -1.0)), glm.rotate(np.float32(0.6), (0.3, 1.0, 0.2)),
                                     glm.scale((0.7, 0.4, 0.9))]), "b")
    sc.camera = camera
    sc.resolution = (W, H)
    return sc


def _frames(pkg, flat, camera, params=(), variant=None):
    with pkg.PathTracer(device=0, max_bounces=MB) as pt:
        for k, v in params:
            pt.set_param(k, v)
        pt.create_buffers((W, H), flat)
        if variant is not None:
            pt.set_trace_variant(variant)
        pt.max_iterations = ITERS
        for _ in range(ITERS):
            pt.path_trace(camera)
        out = {k: pt.download(k) for k in ("color", "normal", "depth")}
        out["stats"] = pt.stats()
        out["upload"] = pt.upload_times()
    return out


def _same_image(got, ref, what):
    for k in ("color", "normal", "depth"):
        assert np.array_equal(got[k], ref[k]), (what, k, int((got[k] != ref[k]).sum()))
    assert got["stats"]["rays_total"] == ref["rays"], what
    live = np.asarray(got["stats"]["last_live"], dtype=np.int64)
    assert np.array_equal(live, ref["live"][-1][:len(live)].astype(np.int64)), (what, live, ref["live"][-1])


IMAGE_CASES = {
    # family, triangles, camera position, looking at
    "signed_zeros": (3000, (0.7, 0.9, 13.0), (0.0, 0.0, 0.0)),
    "signed_zeros_small": (300, (0.0, 0.0, 12.0), (0.0, 0.0, 0.0)),   # the view axis runs through the zero coordinates
    "planar": (3000, (0.3, 0.2, 11.0), (0.0, 0.0, 0.0)),
    "clustered": (3000, (0.2, 0.3, 5.0), (0.0, 0.0, 0.0)),
    "indexed": (3000, (5.0, 6.0, 16.0), (5.0, 0.0, 5.0)),
}


@pytest.mark.parametrize("case", sorted(IMAGE_CASES))
def test_images_with_a_device_built_tree_against_the_oracle(pkg, orc, case):
    """colour, normal, depth, ray and live counts bit for bit, the library building the tree on the device (the default),
    under every trace variant; then with the tree built on the host and with the host builder's tree handed in by the
    caller, which tells the builder from the walk should one of them differ"""
    n, eye, at = IMAGE_CASES[case]
    family = case.replace("_small", "")
    mesh = _mesh(pkg, *bm.family(family, n))
    camera = pkg.scenes._camera_from_look_at(eye, at, vfov_deg=50.0)
    sc = _image_scene(pkg, mesh, camera)
    flat = sc.build_scene()
    assert flat.bvh is None
    ref = orc.render_streaming(flat, camera, W, H, 0, ITERS, MB)
    assert ref["rays"] > 1.5 * W * H * ITERS, ref["rays"]
    for variant in (None, 0, 1):
        got = _frames(pkg, flat, camera, variant=variant)
        assert got["upload"]["bvh_on_device"] == 1 and got["upload"]["layout_on_device"] == 1
        _same_image(got, ref, (case, "device tree", variant))
    _same_image(_frames(pkg, flat, camera, params=(("layout_on_device", 0), ("bvh_build_on_device", 0))), ref, (case, "host tree"))
    handed = copy.copy(flat)
    handed.bvh, _ = pkg.bvh_from_mesh(mesh)
    for variant in (None, 0):
        got = _frames(pkg, handed, camera, variant=variant)
        assert got["upload"]["bvh_on_device"] == 0
        _same_image(got, ref, (case, "caller's tree", variant))


def _zero_rays(rng, n, reach):
    """origins and directions whose coordinates are exact zeros of both signs, mixed with ordinary ones"""
    def with_zeros(a):
        u = rng.uniform(size=a.shape)
        a = a.astype(np.float32)
        a[u < 0.25] = np.float32(0.0)
        a[(u >= 0.25) & (u < 0.5)] = np.float32(-0.0)
        return a
    o = with_zeros(rng.uniform(-reach, reach, size=(n, 3)))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = with_zeros(d)
    d[~d.any(axis=1)] = (0.0, -0.0, 1.0)
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 1e-4, d, FLT_MAX
    return rays


@pytest.mark.parametrize("n", [300, 3000])
def test_signed_zero_rays_against_the_oracle(pkg, orc, n):
    """ptc_intersect_rays on the device-built signed_zeros tree, rays that start on and run along the planes the boxes'
    zero bounds lie in: t, normal, material and side are the oracle's"""
    mesh = _mesh(pkg, *bm.family("signed_zeros", n))
    camera = pkg.scenes._camera_from_look_at((0.0, 0.0, 12.0), (0.0, 0.0, 0.0))
    flat = _image_scene(pkg, mesh, camera).build_scene()
    rays = _zero_rays(np.random.default_rng(n), 4096, 5.0)
    recs, hit = orc.intersect_rays(flat, rays)
    m = hit.astype(bool)
    assert 0.5 < m.mean()
    for params in ((), (("layout_on_device", 0), ("bvh_build_on_device", 0))):
        with pkg.PathTracer() as pt:
            for k, v in params:
                pt.set_param(k, v)
            pt.create_buffers((W, H), flat)
            assert pt.upload_times()["bvh_on_device"] == (0 if params else 1)
            t, nrm, mat, side = pt.intersect_rays(rays)
        assert np.array_equal(t >= 0, m), params
        assert np.array_equal(t[m], recs["t"][m]) and np.array_equal(nrm[m].view(np.uint32), recs["normal"][m].view(np.uint32)), params
        assert np.array_equal(mat[m], recs["material_id"][m].astype(np.uint32)) and np.array_equal(side[m], recs["side"][m]), params


# ---- vertices that are not finite -----------------------------------------------------------------------------------

def _host_rc(pkg, pos, idx):
    nodes = np.zeros(max(2 * (len(idx) // 3), 1), dtype=pkg.scene_description.BVH_NODE_DTYPE)
    return pkg.lib().ptc_build_bvh(pos.ctypes.data_as(C.POINTER(C.c_float)), len(pos), idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                   len(idx), nodes.ctypes.data_as(C.POINTER(pkg._capi.ptc_bvh_node)), None)


def _one_object(pkg, meshes):
    sc = pkg.SceneDescription()
    sc.add_material("m", pkg.DiffuseMateral((0.5, 0.5, 0.5)))
    for k, mesh in enumerate(meshes):
        sc.add_mesh(f"mesh{k}", mesh)
        sc.add_object(mesh, pkg.glmlite.identity(), "m")
    return sc.build_scene(distinct_meshes=len(meshes) > 1)


def test_non_finite_vertices_are_refused_alike(pkg, orc):
    """A NaN or infinite coordinate in a vertex that a triangle uses: PTC_ERR_INVALID from ptc_build_bvh,
    ptc_build_bvh_device and ptc_upload_scene (which names mesh and vertex), whatever the size of the node the triangle
    would end up in; the scene uploaded before stays, and the context builds and renders a good mesh afterwards."""
    invalid = pkg._capi.PTC_ERR_INVALID
    box = (np.full(3, -60, dtype=np.float32), np.full(3, 60, dtype=np.float32))   # (the box of the mesh is the caller's to give)
    good = _mesh(pkg, *bm.soup(40, 9))
    good_host, good_depth = pkg.bvh_from_mesh(good)
    good_flat = _one_object(pkg, [good])
    with pkg.PathTracer() as pt:
        pt.create_buffers((W, H), good_flat)
        before = {k: pt.download_layout(k) for k in pt.LAYOUTS}
        for name, pos, idx, bad in bm.non_finite():
            mesh = _mesh(pkg, pos, idx, aabb=box)
            assert _host_rc(pkg, pos, idx) == invalid, name
            with pytest.raises(pkg.PtcError) as e:
                pt.build_bvh(mesh)
            assert e.value.code == invalid and f"vertex {bad} " in str(e.value), (name, str(e.value))
            for on_device in (1, 0):
                pt.set_param("bvh_build_on_device", on_device)
                with pytest.raises(pkg.PtcError) as e:
                    pt.create_buffers((W, H), _one_object(pkg, [mesh]))
                assert e.value.code == invalid and f"mesh 0: vertex {bad} " in str(e.value), (name, str(e.value))
            with pytest.raises(pkg.PtcError) as e:      # the second mesh of a table; the first one is fine
                pt.create_buffers((W, H), _one_object(pkg, [good, mesh]))
            assert e.value.code == invalid and f"mesh 1: vertex {bad} " in str(e.value), (name, str(e.value))
            flat = _one_object(pkg, [mesh])             # a caller's tree does not excuse the vertex
            flat.bvh, _ = pkg.bvh_from_mesh(_mesh(pkg, np.where(np.isfinite(pos), pos, np.float32(1.0)), idx))
            with pytest.raises(pkg.PtcError) as e:
                pt.create_buffers((W, H), flat)
            assert e.value.code == invalid and f"mesh 0: vertex {bad} " in str(e.value), (name, str(e.value))
            if len(idx) // 3 in (4, 300) and bad < 3:   # now and then: the context is as good as before
                got, got_depth = pt.build_bvh(good)
                assert got_depth == good_depth and np.array_equal(got.view(np.uint8), good_host.view(np.uint8)), name
        # the scene uploaded before the refusals is still there, byte for byte
        for k, v in before.items():
            assert np.array_equal(pt.download_layout(k), v), k
        # a vertex that no triangle uses may hold anything: the three paths build the tree of the used ones
        for n in (2, 4, 40, 300):
            pos, idx = bm.unused_non_finite(n, 5)
            mesh = _mesh(pkg, pos, idx, aabb=box)
            host, host_depth = pkg.bvh_from_mesh(mesh)
            got, got_depth = pt.build_bvh(mesh)
            assert got_depth == host_depth and np.array_equal(got.view(np.uint8), host.view(np.uint8)), n
            assert check_tree(got, pos, idx, got_depth, bits=True).ok()
            pt.set_param("bvh_build_on_device", 1)
            pt.create_buffers((W, H), _one_object(pkg, [mesh]))
            assert pt.stats()["bvh_node_count"] == 2 * n - 1 and pt.upload_times()["bvh_on_device"] == 1
    # and a fresh look at the good mesh through the whole pipeline
    camera = pkg.scenes._camera_from_look_at((0.0, 0.0, 160.0), (0.0, 0.0, 0.0), vfov_deg=40.0)
    got = _frames(pkg, good_flat, camera)
    _same_image(got, orc.render_streaming(good_flat, camera, W, H, 0, ITERS, MB), "good mesh after the refusals")
