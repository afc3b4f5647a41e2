"""The hostile meshes of tests/bvh_meshes.py on the host (no GPU): the library's host builder against the oracle's, byte for
byte, on every family up to 2,109,440 triangles; the independent tree check of tests/bvh_tree_check.py on each tree, and
that the check can see (four mutations); the conditions the families must meet so that the device builder's paths stay
exercised (tests/test_gpu_bvh_hostile.py builds the same meshes on the GPU); the rule for vertices that are not finite."""
import ctypes as C

import numpy as np
import pytest

import bvh_meshes as bm
from bvh_tree_check import check_tree


def _host(pkg, pos, idx):
    return pkg.bvh_from_mesh(pkg.Mesh(pos, idx, aabb=(pos[0], pos[0])))   # (the box of the mesh plays no part in the tree)


def _host_rc(pkg, pos, idx):
    nodes = np.zeros(max(2 * (len(idx) // 3), 1), dtype=pkg.scene_description.BVH_NODE_DTYPE)
    return pkg.lib().ptc_build_bvh(pos.ctypes.data_as(C.POINTER(C.c_float)), len(pos), idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                   len(idx), nodes.ctypes.data_as(C.POINTER(pkg._capi.ptc_bvh_node)), None)


def _agree(pkg, orc, name, pos, idx, bits=True):
    """host builder == oracle in bytes, and the tree is right by the independent check; returns the check's result"""
    got, depth = _host(pkg, pos, idx)
    ref, ref_depth = orc.build_bvh(pos, idx)
    assert depth == ref_depth, name
    assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), name
    res = check_tree(got, pos, idx, reported_depth=depth, bits=bits)
    assert res.ok(), (name, res.errors)
    return res


def _assert_clear_of_coincident_centroids(name, pos, idx):
    c = bm.centroids(pos, idx)
    assert np.isfinite(c).all(), name
    assert len(np.unique(c, axis=0)) == len(c), name


@pytest.fixture(scope="module")
def family_trees(pkg, orc):
    """name -> the tree check's result on the host tree of every finite family (which the oracle's equals in bytes)"""
    out = {}
    for name, pos, idx in bm.finite_cases():
        _assert_clear_of_coincident_centroids(name, pos, idx)
        out[name] = _agree(pkg, orc, name, pos, idx)
    return out


def test_generators_are_deterministic_and_typed():
    for a, b in zip(bm.finite_cases(), bm.finite_cases()):
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
        assert a[1].dtype == np.float32 and a[1].ndim == 2 and a[1].shape[1] == 3 and a[2].dtype == np.uint32
        assert a[2].max() < len(a[1])
    for make, counts, seed in bm.FAMILIES.values():
        if make is not bm.indexed:
            assert all(len(make(n, seed)[1]) == 3 * n for n in counts)


def test_families_are_what_they_say():
    sign = lambda a: np.signbit(a)
    for n in bm.FAMILIES["signed_zeros"][1]:
        pos, _ = bm.family("signed_zeros", n)
        zero = pos == 0
        assert (zero & sign(pos)).any() and (zero & ~sign(pos)).any()
        if n >= 300:   # a good share, about half of each sign
            assert 0.35 < zero.mean() < 0.45 and (zero & sign(pos)).sum() > 0.17 * pos.size and (zero & ~sign(pos)).sum() > 0.17 * pos.size
    pos, _ = bm.family("collinear", 300)
    assert not pos[:, 1:].any() and not sign(pos[:, 1:]).any()      # +0.0 only: compared by bytes on the GPU
    pos, _ = bm.family("planar", 300)
    assert not pos[:, 2].any() and not sign(pos[:, 2]).any() and (pos[:, :2] != 0).all()
    pos, _ = bm.family("points", 300)
    assert np.array_equal(pos[0::3], pos[1::3]) and np.array_equal(pos[0::3], pos[2::3])
    pos, _ = bm.family("denormal", 300)
    tiny = np.finfo(np.float32).tiny
    assert (np.abs(pos) < tiny).all() and (pos != 0).all()
    pos, _ = bm.family("huge", 3000)
    assert np.isfinite(pos).all() and np.abs(pos).max() > 1.5e38
    ext = pos.max(axis=0).astype(np.float64) - pos.min(axis=0)
    assert 2.0 * ext[0] * ext[1] > np.finfo(np.float32).max            # the root's area is not finite in binary32
    pos, idx = bm.family("indexed", 3000)
    used = np.zeros(len(pos), dtype=bool)
    used[idx] = True
    assert (~used).sum() == 7 and not used[-7:].any() and np.bincount(idx).max() >= 6
    tri = idx.reshape(-1, 3)
    assert not np.array_equal(tri[:, 0], np.sort(tri[:, 0]))          # the triangles are not in their natural order
    pos, idx = bm.unused_non_finite(40, 5)
    used = np.zeros(len(pos), dtype=bool)
    used[idx] = True
    assert np.isfinite(pos[used]).all() and not np.isfinite(pos[~used]).all(axis=1).any()


def test_host_builder_equals_oracle_and_trees_are_right(family_trees):
    assert len(family_trees) == sum(len(c) for _, c, _ in bm.FAMILIES.values())
    deep = {k: family_trees[k].depth for k in ("collinear300", "denormal300", "huge300", "clustered20000")}
    # zero areas leave split 0 of 12 to the SAH (every cost is NaN): one bucket's worth peeled off per level
    assert all(d >= 30 for d in deep.values()), deep
    # ... which takes 3000 such triangles past the traversal stack (depth 62): the builders build them, an upload refuses them
    too_deep = {k for k, r in family_trees.items() if r.depth > 62}
    assert too_deep == {"denormal3000", "huge3000"}, too_deep


def test_denormal_and_huge_at_1000_fit_the_traversal_stack(pkg, orc):
    """the size at which tests/test_gpu_bvh_hostile.py compares their layouts instead of 3000"""
    for name in ("denormal", "huge"):
        pos, idx = bm.family(name, 1000)
        _assert_clear_of_coincident_centroids(name, pos, idx)
        assert 40 <= _agree(pkg, orc, name + "1000", pos, idx).depth <= 62


def test_every_count(pkg, orc):
    for t in bm.EVERY_COUNT:
        pos, idx = bm.every_count(t)
        _assert_clear_of_coincident_centroids(t, pos, idx)
        res = _agree(pkg, orc, f"every_count{t}", pos, idx)
        assert res.count[0] == t


@pytest.fixture(scope="module")
def big_tree(pkg, orc):
    pos, idx = bm.over_2_20(pkg.scenes)
    assert len(idx) // 3 == 2_109_440
    return _agree(pkg, orc, "over_2_20", pos, idx)


def test_over_2_20(big_tree):
    assert len(big_tree.count) == 2 * 2_109_440 - 1


def _whole_block(start, count, block):
    """the range [start, start + count) holds a whole aligned block of `block` positions"""
    return (start + block - 1) // block * block + block <= start + count


def test_coverage_of_the_device_builders_paths(family_trees, big_tree):
    """Conditions on the INPUTS, taken from the reference tree: a node's (start, count) is the range of positions the device
    builder hands to its kernels.  It switches at 2 (ordered pair), 4/5 (median of a small node / SAH), 32/33 (one thread
    per node / atomics), takes workgroup bins where a node holds a whole block of 1024 positions, wavefront bounds inside
    a row of 64, and scans a level's nodes in blocks of 1024, recursing once per factor of 1024."""
    trees = dict(family_trees, over_2_20=big_tree)
    start = np.concatenate([r.start for r in trees.values()])
    count = np.concatenate([r.count for r in trees.values()])
    for n in (2, 3, 4, 5, 32, 33):
        assert (count == n).any(), n
    big = count > 32
    has1024 = _whole_block(start, count, 1024)
    has256 = _whole_block(start, count, 256)
    assert (big & has1024).any()
    assert (big & has256 & ~has1024).any()
    assert (big & (start // 64 == (start + count - 1) // 64)).any()
    assert (big & (start % 256 != 0)).any()
    # the families alone (without the large grid) reach the alignment cases too, at offsets a grid does not produce
    s2 = np.concatenate([r.start for r in family_trees.values()])
    c2 = np.concatenate([r.count for r in family_trees.values()])
    assert ((c2 > 32) & _whole_block(s2, c2, 1024)).any() and ((c2 > 32) & (s2 // 64 == (s2 + c2 - 1) // 64)).any()
    # the scan over a level's nodes takes its second recursion above 1024^2 nodes; the flags' scan above 1024^2 triangles
    widest = int(np.diff(big_tree.level_base).max())
    assert widest > 1_048_576, widest
    assert big_tree.count[0] > 1_048_576


def test_tree_check_sees_mutations(pkg):
    pos, idx = bm.family("clustered", 300)
    nodes, depth = _host(pkg, pos, idx)
    assert check_tree(nodes, pos, idx, depth, bits=True).ok()
    leaves = np.nonzero(nodes["primitive_count"] == 1)[0]
    inner = np.nonzero(nodes["primitive_count"] == 0)[0]

    def errors(mutate, **kw):
        m = nodes.copy()
        mutate(m)
        return check_tree(m, pos, idx, kw.pop("depth", depth), **kw).errors

    def swap(m):  # two leaves trade triangles: every triangle is still named once, but the boxes are another's
        a, b = leaves[3], leaves[-5]
        m["first_child_or_primitive"][[a, b]] = m["first_child_or_primitive"][[b, a]]
    e = errors(swap)
    assert e and all("leaf m" in x for x in e), e

    def duplicate(m):
        m["first_child_or_primitive"][leaves[7]] = m["first_child_or_primitive"][leaves[8]]
    e = errors(duplicate)
    assert any("no leaf" in x for x in e) and any("more than one leaf" in x for x in e), e

    def one_ulp(m):  # the root's box one ulp larger: still encloses everything, no longer exact
        m["aabb_max"][0, 1] = np.nextafter(m["aabb_max"][0, 1], np.float32(np.inf))
    e = errors(one_ulp)
    assert e == [x for x in e if "inner max" in x] and len(e) >= 1, e

    def one_ulp_leaf(m):
        m["aabb_min"][leaves[11], 2] = np.nextafter(m["aabb_min"][leaves[11], 2], np.float32(-np.inf))
    e = errors(one_ulp_leaf)
    assert any("leaf min" in x for x in e), e

    def move_pair(m):  # two inner nodes of one level trade their child pairs
        a, b = inner[5], inner[6]
        m["first_child_or_primitive"][[a, b]] = m["first_child_or_primitive"][[b, a]]
    e = errors(move_pair)
    assert any("grow" in x for x in e), e

    assert any("depth" in x for x in errors(lambda m: None, depth=depth + 1))
    assert any("nodes for" in x for x in check_tree(nodes[:-2], pos, idx, depth).errors)

    # a zero of the other sign passes as a value and is seen as bits
    zpos, zidx = bm.family("signed_zeros", 300)
    znodes, zdepth = _host(pkg, zpos, zidx)
    at = np.argwhere((znodes["aabb_min"] == 0) & ~np.signbit(znodes["aabb_min"]) & (znodes["primitive_count"] == 1)[:, None])
    tri = zpos[zidx.reshape(-1, 3)[znodes["first_child_or_primitive"][at[:, 0]] // 3]]   # [leaves, vertex, xyz]
    vert = tri[np.arange(len(at)), :, at[:, 1]]
    only_plus = ~(np.signbit(vert) & (vert == 0)).any(axis=1)   # leaves whose zero bound can only be +0
    i, k = at[only_plus][0]
    flipped = znodes.copy()
    flipped["aabb_min"][i, k] = np.float32(-0.0)
    assert check_tree(flipped, zpos, zidx, zdepth, bits=False).ok()
    assert any("bits of no candidate" in x for x in check_tree(flipped, zpos, zidx, zdepth, bits=True).errors)


def test_non_finite_vertices_are_refused_by_the_host_builder(pkg):
    """a NaN or infinite coordinate in a vertex some triangle uses: PTC_ERR_INVALID, whatever the size of the node it ends
    up in (2 to 4: sorted, more: SAH); a vertex nobody uses may hold anything"""
    cases = list(bm.non_finite())
    assert len(cases) == (2 + 3 + 4 + 6 + 3 + 3) * 3
    for name, pos, idx, bad in cases:
        assert not np.isfinite(pos[bad]).all() and np.isfinite(np.delete(pos, [bad, bad + 1], axis=0)).all(), name
        assert _host_rc(pkg, pos, idx) == pkg._capi.PTC_ERR_INVALID, name
        good = np.where(np.isfinite(pos), pos, np.float32(1.0))
        assert _host_rc(pkg, good, idx) == 2 * (len(idx) // 3) - 1, name
    for n in (2, 4, 40, 300):
        pos, idx = bm.unused_non_finite(n, 5)
        assert _host_rc(pkg, pos, idx) == 2 * n - 1
        nodes, depth = _host(pkg, pos, idx)
        assert check_tree(nodes, pos, idx, depth, bits=True).ok()
