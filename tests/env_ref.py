"""CPU restatement of environment lighting (ptc_set_environment) in numpy binary32 -- TEST INFRASTRUCTURE: the
checker of tests/test_environment_cpu.py and tests/test_gpu_environment.py, not the thing under test.

The reference's sky is a fixed gradient, so the oracle (oracle/oracle.c) cannot check an environment and stays as it is.  This file
restates the apron and the lookup of section 5j -- every numpy operation below is one binary32 operation of the rule, in its order
(numpy does not contract into FMA) -- and nothing else: the render loops are loop_ref's, which take `env` as an option and hand this
module's lookup to their misses in lit_ref.sky's place.  env None is no environment: the gradient."""
import numpy as np

from ref_f32 import F

FLT_MAX = F(np.finfo(np.float32).max)
MIN_SIZE, MAX_SIZE = 2, 4096


def as_map(env):
    """[n, n, 3] binary32, M[j][i]: row j along z, column i along x"""
    m = np.ascontiguousarray(env, dtype=np.float32)
    assert m.ndim == 3 and m.shape[0] == m.shape[1] and m.shape[2] == 3 and MIN_SIZE <= m.shape[0] <= MAX_SIZE
    return m


def apron(env):
    """E, [n + 2, n + 2, 4] (w = 0): M with the one-texel apron of the octahedral fold, by the table of section 5j.  With i = I - 1,
    j = J - 1 and c(t) = min(max(t, 0), n - 1):  both in range M[j][i];  only i out M[n-1-j][c(i)];  only j out M[c(j)][n-1-i];
    both out M[n-1-c(j)][n-1-c(i)]."""
    m = as_map(env)
    n = m.shape[0]
    e = np.zeros((n + 2, n + 2, 4), dtype=np.float32)
    clamp = lambda t: min(max(t, 0), n - 1)
    for J in range(n + 2):
        for I in range(n + 2):
            i, j = I - 1, J - 1
            i_in, j_in = 0 <= i < n, 0 <= j < n
            if i_in and j_in:
                src = m[j, i]
            elif j_in:
                src = m[n - 1 - j, clamp(i)]
            elif i_in:
                src = m[clamp(j), n - 1 - i]
            else:
                src = m[n - 1 - clamp(j), n - 1 - clamp(i)]
            e[J, I, :3] = src
    return e


def _sgn(t):
    return np.where(t < F(0.0), F(-1.0), F(1.0)).astype(np.float32)  # (-0: +1)


def _axis(q, n):
    """item 5: the lower texel of E along one axis (0 .. n) and the weight of the upper one"""
    m = q * F(0.5)
    s = m + F(0.5)
    f = s * F(n)
    x = f + F(0.5)
    i0 = np.minimum(np.maximum(np.floor(x).astype(np.int64), 0), n)
    t = x - i0.astype(np.float32)
    return i0, t


def _lerp(x, y, a):
    return x * (F(1.0) - a) + y * a  # glm::lerp's form


def locate(d, n):
    """items 1-5 for directions d [k, 3] -> (ok [k]: item 2 lets the direction through, i0, j0, tx, tz); rows that are not ok hold
    index 0 and weight 0"""
    d = np.asarray(d, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        a = (np.abs(d[:, 0]) + np.abs(d[:, 1])) + np.abs(d[:, 2])
        ok = (a > F(0.0)) & (a <= FLT_MAX)
        a_ok = np.where(ok, a, F(1.0))
        dx, dy, dz = (np.where(ok, d[:, k], F(0.0)) for k in range(3))
        px = dx / a_ok
        pz = dz / a_ok
        lower = dy < F(0.0)
        qx = np.where(lower, (F(1.0) - np.abs(pz)) * _sgn(px), px)
        qz = np.where(lower, (F(1.0) - np.abs(px)) * _sgn(pz), pz)
        i0, tx = _axis(qx, n)
        j0, tz = _axis(qz, n)
    return ok, i0, j0, tx, tz


def lookup(env, d, texels=None):
    """The environment's value in the directions d [k, 3] (not normalised) -> [k, 3] binary32.  texels: apron(env), if the caller
    has it."""
    e = apron(env) if texels is None else texels
    n = e.shape[0] - 2
    ok, i0, j0, tx, tz = locate(d, n)
    c00, c10, c01, c11 = e[j0, i0, :3], e[j0, i0 + 1, :3], e[j0 + 1, i0, :3], e[j0 + 1, i0 + 1, :3]
    top = _lerp(c00, c10, tx[:, None])
    bot = _lerp(c01, c11, tx[:, None])
    value = _lerp(top, bot, tz[:, None])
    return np.where(ok[:, None], value, F(0.0)).astype(np.float32)


def direction_set(rng, n, count=4096):
    """The directions the parity tests use: `count` random ones, the six axes, +-0 components, dy = -0 and -1e-30, points on the fold
    edges (|x| + |z| = 1, y = +-0 and a hair below), texel-centre and texel-edge directions of an n-map, and the bad directions of
    item 2 (zero, NaN, infinity, a sum that overflows)."""
    rows = [rng.standard_normal((count, 3)) * np.exp(rng.uniform(-20, 20, (count, 1)))]
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    rows.append(axes)
    rows.append(np.where(axes == 0.0, -0.0, axes))
    rows.append([[0.3, -0.0, 0.7], [0.3, -1e-30, 0.7], [-0.3, -0.0, -0.7], [-0.3, -1e-30, -0.7], [1.0, -1e-30, 0.0], [0.0, -1e-30, -1.0],
                 [0.0, -1.0, 0.0], [1e-30, -1.0, -1e-30], [-0.0, -1.0, 0.0], [0.0, -1.0, -0.0], [1e-38, 1e-38, 1e-38], [1e-45, 0.0, 0.0],
                 [3e38, 0.0, 0.0], [1e38, 1e38, 1e38], [1.7e38, 1.7e38, 0.0]])
    t = np.linspace(-1.0, 1.0, 41)
    for sx in (1.0, -1.0):
        edge = np.stack([sx * (1.0 - np.abs(t)), np.zeros_like(t), t], axis=1)  # the horizon: the fold's edge
        rows += [edge, edge + [0.0, -1e-7, 0.0], edge + [0.0, 1e-7, 0.0], np.where(edge == 0.0, -0.0, edge)]
    k = (np.arange(-1, 2 * n + 2) / (2.0 * n)) * 2.0 - 1.0  # texel centres and edges of the map, both hemispheres
    gx, gz = (g.reshape(-1) for g in np.meshgrid(k, k))
    inside = np.abs(gx) + np.abs(gz) <= 1.0
    up = np.stack([gx, 1.0 - np.abs(gx) - np.abs(gz), gz], axis=1)[inside]
    rows += [up[:512], up[:512] * [1.0, -1.0, 1.0]]
    rows.append([[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [np.nan, 1.0, 0.0], [1.0, np.nan, 0.0], [0.0, 1.0, np.nan], [np.inf, 0.0, 0.0],
                 [0.0, -np.inf, 0.0], [1.0, 1.0, -np.inf], [3e38, 3e38, 0.0], [2e38, -2e38, 2e38]])
    with np.errstate(over="ignore"):
        return np.concatenate([np.asarray(r, dtype=np.float64) for r in rows]).astype(np.float32)
