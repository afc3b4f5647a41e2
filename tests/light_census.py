"""The census of the lamp selection -- TEST INFRASTRUCTURE.  How many of the generator's N = 2^31 - 2 states pick
each lamp of a table, exactly, from the observable behaviour of a sampler alone: selection is monotone in the raw draw v, so a batched
binary search over v (31 calls of one draw per lamp) finds every boundary.  The samplers: the library's own header on the host
(ptc_check_light_sample), the numpy restatement (direct_ref.select), and parent_rule -- the rule the library had before, a binary search
of u0 = float(v - 1) / 2^31 in the binary32 cdf, kept so that the bounds below stay on record as bounds that rule breaks.

Also the hostile tables themselves, as scenes whose lamp weights are exact: a mesh lamp under the identity matrix whose triangle k is
(0, (a_k, 0, 0), (0, 0, 2)) about its origin (area a_k in every precision), its weight a_k * lum; sphere lamps 4 pi R^2 * lum."""
import numpy as np

import direct_ref as D

N = D.STATES


# ---- the census -------------------------------------------------------------------------------------------------------------
def boundaries(sampler, lamps):
    """b[k] = the smallest raw draw v in [1, N + 1] that picks a lamp behind k (N + 1: none does), for k = 0 .. lamps - 1, by bisection
    on sampler(v uint32[lamps]) -> lamp picked.  Monotone selection is what this relies on; census() checks it on the result."""
    k = np.arange(lamps, dtype=np.int64)
    lo, hi = np.ones(lamps, dtype=np.int64), np.full(lamps, N + 1, dtype=np.int64)
    for _ in range(31):   # hi - lo <= 2^31 - 2 halves to 0
        mid = (lo + hi) // 2
        ask = np.minimum(mid, N)   # (mid == N + 1 only once lo == hi == N + 1: the answer is not used)
        behind = np.asarray(sampler(ask.astype(np.uint32)), dtype=np.int64) > k
        go = lo < hi
        hi = np.where(go & behind, mid, hi)
        lo = np.where(go & ~behind, mid + 1, lo)
    assert np.array_equal(lo, hi)
    return lo


def census(sampler, lamps):
    """-> (states int64[lamps]: how many raw draws pick each lamp, boundaries)."""
    b = boundaries(sampler, lamps)
    assert np.all(np.diff(b) >= 0)
    return np.diff(np.concatenate([[1], b])), b


def library_sampler(pkg, flat):
    def sampler(v):
        n = len(v)
        return pkg.check_light_sample(flat, np.zeros((n, 3), dtype=np.float32), np.tile(np.float32([0, 1, 0]), (n, 1)), v,
                                      np.full((n, 2), 0.5, dtype=np.float32))["lamp"]
    return sampler


def restatement_sampler(weights, last):
    t = D.thresholds(weights)
    return lambda v: np.minimum(np.searchsorted(t, np.asarray(v, dtype=np.int64) - 1, side="right"), last)


def parent_rule(weights, last):
    """The rule before: cdf_k = (float)(run_k / W), 1.0f from the last live lamp on; u0 = (float)(v - 1) / 2^31;
    k = min(#{j : cdf_j <= u0}, last)."""
    w = np.asarray(weights, dtype=np.float64)
    run = np.cumsum(w)
    cdf = (run / run[-1]).astype(np.float32)
    cdf[last:] = np.float32(1.0)

    def sampler(v):
        u0 = (np.asarray(v, dtype=np.int64) - 1).astype(np.float32) / np.float32(2147483648.0)
        return np.minimum(np.searchsorted(cdf, u0, side="right"), last)
    return sampler


def flat_weights(flat):
    """The lamp weights of a scene of this module, float64, straight from the flat scene: mesh lamps under the identity matrix (their
    edges are exact in binary32), sphere lamps under a translation."""
    out = []
    for i, obj in enumerate(flat.objects):
        mat = flat.materials[int(flat.object_material_indices[i])]
        if mat["type"] != D.EMISSIVE:
            continue
        lum = float(max(mat["p"][0], mat["p"][1], mat["p"][2]))
        m = np.asarray(obj["m"], dtype=np.float64).reshape(4, 4)
        assert np.array_equal(m[:3, :3], np.eye(3)) and np.array_equal(m[:, 3], [0, 0, 0, 1])
        if obj["type"] == 0:
            r = float(np.asarray(flat.spheres, dtype=np.float32).reshape(-1, 4)[int(obj["index"]), 3])
            out.append(np.array([4.0 * np.pi * r * r * lum]))
        else:
            assert np.array_equal(m[3, :3], [0, 0, 0])
            positions, tri = D._mesh_of(flat, obj)
            positions, tri = positions.astype(np.float64), tri.astype(np.int64)
            e1, e2 = positions[tri[:, 1]] - positions[tri[:, 0]], positions[tri[:, 2]] - positions[tri[:, 0]]
            out.append(0.5 * np.linalg.norm(np.cross(e1, e2), axis=1) * lum)
    return np.concatenate(out) if out else np.zeros(0)


def check_bounds(states, weights):
    """The promises of include/ptcore.h for a census; -> the list of those it breaks (empty: all hold)."""
    w = np.asarray(weights, dtype=np.float64)
    share = w / np.sum(w) * N
    live = w > 0.0
    m = int(np.sum(live & (share < 1.0)))
    broken = []
    if int(states.sum()) != N:
        broken.append("the states do not add up to N")
    if np.any(states[~live] != 0):
        broken.append("a lamp of weight 0 owns a state")
    if np.any(states[live] < 1):
        broken.append("a lamp of weight > 0 owns no state")
    worst = float(np.max(np.abs(states - share)))
    if worst > 1 + m:
        broken.append("a lamp is %.3f states from its share (bound %d)" % (worst, 1 + m))
    return broken


# ---- the tables -------------------------------------------------------------------------------------------------------------
def table_scene(pkg, lamps, floor=False):
    """lamps: a list of ("mesh", lum, areas[, origins]) and ("sphere", lum, radius, centre) in table order.  A mesh lamp's triangle k is
    (o_k, o_k + (a_k, 0, 0), o_k + (0, 0, 2)) under the identity matrix: area a_k exactly when o_k + a_k is (origins: small integers for
    large areas, 0 for tiny ones).  floor: a diffuse floor sphere below y = -1 first (no lamp: the table does not see it)."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    if floor:
        s.add_material("a_floor", pkg.DiffuseMateral((0.7, 0.7, 0.7)))
        s.add_object(pkg.Sphere((0, 0, 0), 1000.0), glm.translate((0.0, -1001.0, 0.0)), "a_floor")
    for j, lamp in enumerate(lamps):
        name = "lamp%05d" % j
        lum = float(lamp[1])
        s.add_material(name, pkg.EmissiveMaterial((lum, 0.5 * lum, 0.25 * lum)))
        if lamp[0] == "sphere":
            s.add_object(pkg.Sphere((0, 0, 0), float(lamp[2])), glm.translate(tuple(lamp[3])), name)
            continue
        a = np.asarray(lamp[2], dtype=np.float32)
        o = np.zeros((len(a), 3), dtype=np.float32) if len(lamp) < 4 else np.asarray(lamp[3], dtype=np.float32).reshape(len(a), 3)
        positions = np.empty((len(a), 3, 3), dtype=np.float32)
        positions[:, 0], positions[:, 1], positions[:, 2] = o, o, o
        positions[:, 1, 0] += a
        positions[:, 2, 2] += np.float32(2.0)
        mesh = s.add_mesh("models/%s.obj" % name, pkg.Mesh(positions.reshape(-1, 3), np.arange(3 * len(a), dtype=np.uint32)))
        s.add_object(mesh, glm.identity(), name)
    return s


def tables(pkg):
    """name -> the lamps of a table of the census, as table_scene takes them (build with distinct_meshes=True)."""
    rng = np.random.default_rng(20261020)
    sky, bulb = ("sphere", 1.0, 1000.0, (0.0, 0.0, 0.0)), ("sphere", 1.0, 0.05, (0.3, 0.2, 0.1))
    big = lambda n: [("mesh", 1.0, rng.uniform(0.5, 1.5, n).astype(np.float32))]
    return {
        "one_tiny_one": [("mesh", 1.0, [1.0, 1e-8, 1.0])],
        "one_tinier": [("mesh", 1.0, [1.0, 1e-9])],
        "sky_then_bulb": [sky, bulb],
        "bulb_then_sky": [bulb, sky],
        "one_small_one": [("mesh", 1.0, [1.0, 1e-6, 1.0])],
        "uniform_2_20": big(2 ** 20),
        "uniform_2_17": big(2 ** 17),
        "uniform_2_14": big(2 ** 14),
        # dark (lum 0) and zero-area lamps first, in the middle, last and in runs
        "dead_lamps": [("mesh", 0.0, [1.0, 2.0]), ("mesh", 2.0, [0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 1e-7, 3.0, 0.0]),
                       ("sphere", 0.0, 0.5, (1.0, 1.0, 1.0)), ("sphere", 0.0, 0.25, (1.0, 2.0, 1.0)), ("sphere", 3.0, 0.25, (0.0, 2.0, 0.0)),
                       ("mesh", 1.0, [0.0, 1e-9, 0.0]), ("mesh", 0.0, [1.0]), ("mesh", 5.0, [0.0, 0.0])],
        "thousand_specks": [("mesh", 1.0, np.concatenate([[3.0], np.full(1000, 1e-12), [2.0]]))],
        "single": [("mesh", 1.5, [0.75])],
    }


def all_dark_scene(pkg):
    return table_scene(pkg, [("mesh", 0.0, [1.0, 2.0]), ("sphere", 0.0, 0.5, (0.0, 1.0, 0.0))])


PARENT_FAILS = ("one_tiny_one", "one_tinier", "sky_then_bulb")   # the tables on which parent_rule breaks check_bounds
