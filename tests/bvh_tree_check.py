"""A check of a reference-layout BVH (32-byte nodes, one triangle per leaf, breadth-first numbering) that shares nothing
with the builders: plain numpy over the node array, the positions and the indices, one set of array operations per level.

check_tree() holds that
  * there are 2T - 1 nodes, primitive_count is 0 or 1;
  * every triangle is named by exactly one leaf, as 3 * t;
  * the children of an inner node are adjacent (first_child, first_child + 1), come after it, first_child grows with the
    node index and every node but the root is the child of exactly one node -- the reference's breadth-first numbering;
  * a leaf's box is the exact min / max of its three vertices, an inner box the exact union of its children's: as VALUES
    (==, so -0.0 and +0.0 agree); with bits=True also as bit patterns: each bound carries the bits of one of the
    candidates it was taken from (which zero survives a min over {-0, +0} is the visiting order's business, but it has to
    be one of them);
  * the depth is the one reported.
It returns every violation as a line of text (none: the tree is right), and for each node its range (start, count): count =
leaves below it, start = leaves to its left in the tree.  That is the range of triangle positions the device builder
gives the node, so conditions on (start, count) are conditions on what its kernels are asked to do."""
from dataclasses import dataclass, field

import numpy as np


@dataclass
class TreeCheck:
    errors: list = field(default_factory=list)
    start: np.ndarray = None       # per node: leaves to its left
    count: np.ndarray = None       # per node: leaves below it
    level_base: np.ndarray = None  # first node of every level, then the node count
    depth: int = -1

    def ok(self):
        return not self.errors


def _some(idx, limit=6):
    idx = np.asarray(idx).reshape(-1)
    return f"{len(idx)} of them, first {idx[:limit].tolist()}"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _box_errors(res, what, nodes_at, got, cands, reduce, bits):
    """got [n, 3] against reduce over the candidates [k][n, 3]"""
    want = cands[0]
    for c in cands[1:]:
        want = reduce(want, c)
    bad = ~(got == want).all(axis=1)
    if bad.any():
        res.errors.append(f"{what}: not the exact bound: nodes {_some(nodes_at[bad])}")
    if bits:
        g = _bits(got)
        seen = np.zeros(got.shape, dtype=bool)
        for c in cands:
            seen |= g == _bits(c)
        bad = ~seen.all(axis=1)
        if bad.any():
            res.errors.append(f"{what}: bits of no candidate: nodes {_some(nodes_at[bad])}")


def check_tree(nodes, positions, indices, reported_depth=None, bits=False):
    res = TreeCheck()
    positions = np.asarray(positions, dtype=np.float32).reshape(-1, 3)
    tri_idx = np.asarray(indices).reshape(-1, 3).astype(np.int64)
    T = len(tri_idx)
    N = len(nodes)
    if N != 2 * T - 1:
        res.errors.append(f"{N} nodes for {T} triangles, want {2 * T - 1}")
        return res
    first = nodes["first_child_or_primitive"].astype(np.int64)
    pc = nodes["primitive_count"]
    lo, hi = nodes["aabb_min"], nodes["aabb_max"]
    if ((pc != 0) & (pc != 1)).any():
        res.errors.append(f"primitive_count not 0 or 1: nodes {_some(np.nonzero((pc != 0) & (pc != 1))[0])}")
        return res
    leaf = pc == 1
    leaves, inner = np.nonzero(leaf)[0], np.nonzero(~leaf)[0]
    if len(leaves) != T:
        res.errors.append(f"{len(leaves)} leaves for {T} triangles")

    # ---- leaves name the triangles
    lf = first[leaves]
    bad = (lf % 3 != 0) | (lf < 0) | (lf >= 3 * T)
    if bad.any():
        res.errors.append(f"leaf offset not 3 * t with t < T: nodes {_some(leaves[bad])}")
        return res
    named = np.bincount(lf // 3, minlength=T)
    if (named == 0).any():
        res.errors.append(f"triangles named by no leaf: {_some(np.nonzero(named == 0)[0])}")
    if (named > 1).any():
        res.errors.append(f"triangles named by more than one leaf: {_some(np.nonzero(named > 1)[0])}")

    # ---- numbering
    fc = first[inner]
    bad = (fc <= inner) | (fc + 1 >= N)
    if bad.any():
        res.errors.append(f"children not after their parent or out of range: nodes {_some(inner[bad])}")
        return res
    if len(fc) > 1 and (np.diff(fc) < 2).any():
        res.errors.append(f"first_child does not grow by at least 2 with the node index: after nodes {_some(inner[:-1][np.diff(fc) < 2])}")
    parents = np.bincount(np.concatenate([fc, fc + 1]), minlength=N)
    if parents[0] != 0 or (parents[1:] != 1).any():
        wrong = np.nonzero(parents != np.r_[0, np.ones(N - 1, dtype=np.int64)])[0]
        res.errors.append(f"not the child of exactly one node (the root: of none): nodes {_some(wrong)}")
    if res.errors and any("child" in e for e in res.errors):
        return res   # the levels below rest on the numbering

    # ---- levels: with this numbering the nodes of a depth are one contiguous range
    base = [0, 1] if N else [0]
    while base[-1] < N:
        a, b = base[-2], base[-1]
        inner_here = int((~leaf[a:b]).sum())
        if inner_here == 0:
            res.errors.append(f"level {len(base) - 2} has no inner node but nodes follow it")
            return res
        base.append(b + 2 * inner_here)
    res.level_base = np.array(base, dtype=np.int64)
    res.depth = len(base) - 2
    if reported_depth is not None and res.depth != reported_depth:
        res.errors.append(f"depth {res.depth}, reported {reported_depth}")

    # ---- boxes
    v = positions[tri_idx[lf // 3]]   # [leaves, 3 vertices, xyz]
    _box_errors(res, "leaf min", leaves, lo[leaves], [v[:, 0], v[:, 1], v[:, 2]], np.minimum, bits)
    _box_errors(res, "leaf max", leaves, hi[leaves], [v[:, 0], v[:, 1], v[:, 2]], np.maximum, bits)
    _box_errors(res, "inner min", inner, lo[inner], [lo[fc], lo[fc + 1]], np.minimum, bits)
    _box_errors(res, "inner max", inner, hi[inner], [hi[fc], hi[fc + 1]], np.maximum, bits)

    # ---- ranges: leaves below (bottom-up), leaves to the left (top-down)
    count = leaf.astype(np.int64)
    for lv in range(len(base) - 2, -1, -1):
        at = np.arange(base[lv], base[lv + 1])
        at = at[~leaf[at]]
        count[at] = count[first[at]] + count[first[at] + 1]
    start = np.zeros(N, dtype=np.int64)
    for lv in range(len(base) - 1):
        at = np.arange(base[lv], base[lv + 1])
        at = at[~leaf[at]]
        start[first[at]] = start[at]
        start[first[at] + 1] = start[at] + count[first[at]]
    res.start, res.count = start, count
    if N and count[0] != T:
        res.errors.append(f"{count[0]} leaves below the root, {T} triangles")
    return res
