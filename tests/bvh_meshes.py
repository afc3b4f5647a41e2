"""Hostile meshes for the BVH builders (plain numpy, no GPU, nothing of the library): signed zeros, zero areas,
denormal and near-FLT_MAX coordinates, clustered soups that come out deep and wide at once, every small triangle count,
shared and permuted vertices, more than 2^20 triangles, and vertices that are not finite.

Every family is a function of a triangle count and a seed, returns (positions float32 [V, 3], indices uint32 [3T]) and is
deterministic.  All but `non_finite` keep the triangles' centroids (centre of the box, as the builders take it) finite and
distinct, because a node of coincident centroids is refused by design: tests/test_bvh_meshes_cpu.py asserts that."""
import numpy as np

INF = np.float32(np.inf)
NAN = np.float32(np.nan)


def _soup64(n, seed, spread=50.0, size=0.7):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-spread, spread, size=(n, 1, 3))
    return centre + rng.normal(scale=size, size=(n, 3, 3)), rng


def _natural(pos64):
    pos = np.ascontiguousarray(pos64.reshape(-1, 3), dtype=np.float32)
    return pos, np.arange(len(pos), dtype=np.uint32)


def soup(n, seed):
    """the friendly case the others are made from: centres in [-50, 50]^3, vertices N(0, 0.7) around them"""
    return _natural(_soup64(n, seed)[0])


def signed_zeros(n, seed):
    """a soup in which 40 % of the coordinates are exactly +0.0 or -0.0 (half each); the others keep their jitter, and so
    does every triangle's first vertex, which keeps the centroids apart"""
    pos, rng = _soup64(n, seed, spread=4.0, size=0.5)
    pos = pos.astype(np.float32)
    u = rng.uniform(size=pos.shape)
    u[:, 0] = 1.0
    pos[u < 0.3] = np.float32(0.0)
    pos[(u >= 0.3) & (u < 0.6)] = np.float32(-0.0)
    return _natural(pos)


def collinear(n, seed):
    """all vertices on the x axis (y = z = +0.0): every box has area 0"""
    pos, _ = _soup64(n, seed)
    pos[..., 1:] = 0.0
    return _natural(pos)


def planar(n, seed):
    """z = +0.0: overlapping coplanar triangles; the boxes' areas are 0 on two of three faces"""
    pos, _ = _soup64(n, seed, spread=4.0, size=0.5)
    pos[..., 2] = 0.0
    return _natural(pos)


def points(n, seed):
    """each triangle's three vertices are equal: every leaf box is a point"""
    pos, _ = _soup64(n, seed)
    return _natural(np.repeat(pos[:, :1], 3, axis=1))


def denormal(n, seed):
    """a soup times 1e-40: every coordinate is a binary32 denormal, every area underflows to 0"""
    return _natural(_soup64(n, seed)[0] * 1e-40)


def huge(n, seed):
    """a soup times 3e36: coordinates reach 1.5e38, extents 3e38; areas and some SAH costs are inf or NaN"""
    return _natural(_soup64(n, seed)[0] * 3e36)


def clustered(n, seed):
    """centres, and the triangles' sizes with them, multiplied by exp(N(0, 3)) per triangle: most triangles crowd the
    origin, a few large ones lie far out, and the SAH peels them off a handful at a time -- a tree that is deep and has
    wide levels"""
    rng = np.random.default_rng(seed)
    scale = np.exp(rng.normal(scale=3.0, size=(n, 1, 1)))
    centre = rng.uniform(-1.0, 1.0, size=(n, 1, 3))
    return _natural((centre + rng.normal(scale=0.15, size=(n, 3, 3))) * scale)


def every_count(t):
    """one seeded clustered soup per triangle count"""
    return clustered(t, 1000 + t)


def indexed(n, seed):
    """a jittered grid whose triangles share vertices (about n triangles, two per cell), the triangles in a seeded
    permutation of the natural order, and 7 vertices no triangle uses at the end of the position array.  The two
    triangles of a cell have the same box wherever their shared diagonal spans it; x is sheared by 0.02 per row (more than
    its jitter), so that their boxes always differ in x and no two centroids coincide."""
    rng = np.random.default_rng(seed)
    nx = max(2, int(round((n / 2) ** 0.5)) + 1)
    nz = max(2, -(-n // (2 * (nx - 1))) + 1)
    ix, iz = np.meshgrid(np.arange(nx), np.arange(nz), indexing="xy")
    pos = np.stack([ix + 0.02 * iz, np.zeros_like(ix), iz], axis=-1).astype(np.float64)
    pos += rng.uniform(-1.0, 1.0, size=(nz, nx, 3)) * [0.008, 0.3, 0.3]
    v = (iz[:-1, :-1] * nx + ix[:-1, :-1]).astype(np.uint32)
    tris = np.stack([np.stack([v, v + nx, v + 1], -1), np.stack([v + 1, v + nx, v + nx + 1], -1)], axis=2).reshape(-1, 3)
    tris = tris[rng.permutation(len(tris))]
    unused = rng.uniform(-2.0, 2.0, size=(7, 3)) + [nx / 2, 3.0, nz / 2]
    positions = np.concatenate([pos.reshape(-1, 3) * 0.25, unused * 0.25]).astype(np.float32)
    return np.ascontiguousarray(positions), np.ascontiguousarray(tris.reshape(-1))


def over_2_20(scenes):
    """2,109,440 triangles: more than 1024^2 positions (the third level of the builder's scan) and, in the reference
    tree, one level of more than 1024^2 nodes.  `scenes` is the package's scenes module."""
    m = scenes.heightfield_mesh(1025, 1031, 8.0, 4.0, seed=3)
    return m.positions, m.indices


# name -> (generator, triangle counts, seed): the finite families of tests/test_bvh_meshes_cpu.py and
# tests/test_gpu_bvh_hostile.py (every_count and over_2_20 are driven separately)
FAMILIES = {
    "signed_zeros": (signed_zeros, (6, 40, 300, 3000), 21),
    "collinear": (collinear, (6, 40, 300, 3000), 22),
    "planar": (planar, (6, 40, 300, 3000), 23),
    "points": (points, (6, 40, 300, 3000), 24),
    "denormal": (denormal, (6, 40, 300, 3000), 25),
    "huge": (huge, (6, 40, 300, 3000), 26),
    "clustered": (clustered, (300, 3000, 20_000), 27),
    "indexed": (indexed, (6, 40, 300, 3000), 28),
}
EVERY_COUNT = tuple(range(1, 401))


def finite_cases():
    """(name, positions, indices) of every finite family at every count"""
    for family, (make, counts, seed) in FAMILIES.items():
        for n in counts:
            yield (f"{family}{n}",) + make(n, seed + n)


def family(name, n):
    make, _, seed = FAMILIES[name]
    return make(n, seed + n)


def centroids(positions, indices):
    """centre of each triangle's box in binary32, the way the builders compute it: (lo + hi) / 2"""
    tri = positions[indices.reshape(-1, 3).astype(np.int64)]
    with np.errstate(over="ignore", invalid="ignore"):
        return (tri.min(axis=1) + tri.max(axis=1)) / np.float32(2.0)


# ---- vertices that are not finite -----------------------------------------------------------------------------------

NON_FINITE_KINDS = ("inf_pair", "nan", "inf")


def _bad_positions(t):
    """which triangle is the bad one: every position of a small mesh, the ends and the middle of a larger one"""
    return tuple(range(t)) if t <= 6 else (0, t // 2, t - 1)


def non_finite():
    """(name, positions, indices, bad vertex): a soup of T triangles in which ONE triangle has, on one axis, +inf and -inf
    (its centroid is NaN), one NaN coordinate, or a single +inf.  `bad vertex` is the first vertex with such a coordinate."""
    for t in (2, 3, 4, 6, 40, 300):
        for at in _bad_positions(t):
            for k, kind in enumerate(NON_FINITE_KINDS):
                pos, idx = soup(t, 300 + t)
                axis = (at + k) % 3
                first = 3 * at + (at % 2)           # the first or the second vertex of the triangle
                if kind == "inf_pair":
                    pos[first, axis] = INF
                    pos[first + 1, axis] = -INF
                elif kind == "nan":
                    pos[first, axis] = NAN
                else:
                    pos[first, axis] = INF
                yield f"{kind}_T{t}_at{at}", pos, idx, first


def unused_non_finite(n, seed):
    """a soup with three more vertices that no triangle uses: NaN, +inf, -inf.  Not an error."""
    pos, idx = soup(n, seed)
    extra = np.array([[NAN, 0, 0], [0, INF, 0], [1, 2, -INF]], dtype=np.float32)
    return np.concatenate([pos, extra]), idx
