"""CPU restatement of environment light sampling (ptc_environment_light, ptc_set_param "environment_light") in numpy
binary32 -- TEST INFRASTRUCTURE: the checker of tests/test_environment_light_cpu.py and tests/test_gpu_environment_light.py, not the
thing under test.

What stands here: the sample of section 5k, every numpy operation one binary32 operation of the rule in its order (numpy does not
contract into FMA); the stream it draws from; and a binary64 quadrature of what a sample estimates.  The megakernel's loop with the
environment for a light is loop_ref.render_megakernel's under `env_light`.  The alias TABLE is data to this file: it is built in
binary64 by the library's host code (ptc_check_environment_light_table), its properties are what test_environment_light_cpu.py checks,
and the sample below reads it as the device does."""
import ctypes as C

import numpy as np

import env_ref
from ref_f32 import PI, Draws, F, _dot, stream_states

SEED_XOR = 0x454E564C  # kEnvLightSeedXor (pt_device.hpp)
FLT_MAX = F(np.finfo(np.float32).max)
ENTRY = np.dtype([("q", np.float32), ("alias", np.uint32), ("f", np.float32), ("f_alias", np.float32)])
M31 = (1 << 31) - 1


def table_of(pkg, env):
    """The library's table of the map -> (entries [n n] of ENTRY, or None for a map of weight 0; W; squares of weight > 0)"""
    m = env_ref.as_map(env)
    n = m.shape[0]
    entries = np.zeros(n * n, dtype=ENTRY)
    W, positive = C.c_double(), C.c_uint64()
    rc = pkg._capi.lib().ptc_check_environment_light_table(m.ctypes.data_as(C.c_void_p), n, entries.ctypes.data_as(C.c_void_p), C.byref(W),
                                                           C.byref(positive))
    assert rc == 0, rc
    return (entries if W.value > 0.0 else None), W.value, positive.value


def stream(orc, indices, iteration, discard):
    """The four draws of a sample: per index a generator seeded path_seed(index, iteration) ^ SEED_XOR, discard(discard); the raw
    value v = next(), then u1, u2, u3 = uniform() -> (v uint32[n], u float32[n, 3])"""
    states = stream_states(orc, indices, iteration, SEED_XOR, discard)
    v = ((states.astype(np.uint64) * np.uint64(48271)) % np.uint64(M31)).astype(np.uint32)  # minstd_rand's step
    draws = Draws(orc, v)
    every = np.arange(len(v))
    return v, np.stack([draws.uniform(every) for _ in range(3)], axis=-1).reshape(-1, 3)


def decode(sx, sz):
    """section 5k, item 3: the unit direction of the point (sx, sz) of the octahedral unit square, and its 1-norm cubed"""
    tx = sx * F(2.0)
    qx = tx - F(1.0)
    tz = sz * F(2.0)
    qz = tz - F(1.0)
    ax, az = np.abs(qx), np.abs(qz)
    s1 = ax + az
    y = F(1.0) - s1
    lower = ~(s1 <= F(1.0))
    dx = np.where(lower, (F(1.0) - az) * env_ref._sgn(qx), qx)
    dz = np.where(lower, (F(1.0) - ax) * env_ref._sgn(qz), qz)
    d = np.stack([dx, y, dz], axis=-1).astype(np.float32)
    d2 = _dot(d, d)
    ln = np.sqrt(d2)
    inv = F(1.0) / ln
    w = d * inv[:, None]
    l1 = (np.abs(w[:, 0]) + np.abs(w[:, 1])) + np.abs(w[:, 2])
    l3 = (l1 * l1) * l1
    return w, l3


def sample(entries, texels, points, normals, v, u):
    """One environment sample per point from explicit draws (section 5k, items 1-8).  entries: table_of's; texels: env_ref.apron of the
    map.  -> dict(sampled bool[n], square [n], w [n, 3], contribution [n, 3], rays [n, 8] as the query writes them)"""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    normals = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    v = np.asarray(v, dtype=np.uint32)
    u = np.asarray(u, dtype=np.float32).reshape(-1, 3)
    n = texels.shape[0] - 2
    e = ((v.astype(np.uint64) - np.uint64(1)) * np.uint64(n * n)) >> np.uint64(31)
    ent = entries[e.astype(np.int64)]
    keep = u[:, 0] < ent["q"]
    k = np.where(keep, e, ent["alias"].astype(np.uint64)).astype(np.int64)
    f = np.where(keep, ent["f"], ent["f_alias"]).astype(np.float32)
    j = k // n
    i = k - j * n
    fn = F(n)
    cx = i.astype(np.float32) + u[:, 1]
    sx = cx / fn
    cz = j.astype(np.float32) + u[:, 2]
    sz = cz / fn
    w, l3 = decode(sx, sz)
    L = env_ref.lookup(None, w, texels)
    cos_r = _dot(normals, w)
    with np.errstate(invalid="ignore"):
        sampled = cos_r > F(0.0)
    ff = F(4.0) * f
    jac = ff * l3
    cj = cos_r * jac
    gk = cj / PI
    with np.errstate(invalid="ignore", over="ignore"):
        contribution = np.where(sampled[:, None], L * gk[:, None], F(0.0)).astype(np.float32)
    rays = np.zeros((len(points), 8), dtype=np.float32)
    rays[:, 0:3], rays[:, 3] = points, F(1e-4)
    rays[sampled, 4:7], rays[sampled, 7] = w[sampled], FLT_MAX
    return {"sampled": sampled, "square": k, "w": w, "contribution": contribution, "rays": rays}


def query(orc, flat, entries, texels, points, normals, sample_index, scene_handle=None):
    """ptc_environment_light restated: sample() on the stream of (point index, sample_index), then the shadow rays through the oracle's
    closest hit.  entries None (a map of weight 0): zeros.  -> (radiance [n, 3], rays [n, 8], visible uint8[n], sampled bool[n])"""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    n = len(points)
    if entries is None:
        rays = np.zeros((n, 8), dtype=np.float32)
        rays[:, 0:3], rays[:, 3] = points, F(1e-4)
        return np.zeros((n, 3), np.float32), rays, np.zeros(n, np.uint8), np.zeros(n, bool)
    v, u = stream(orc, np.arange(n), sample_index, 0)
    s = sample(entries, texels, points, normals, v, u)
    visible = np.zeros(n, dtype=bool)
    sel = np.nonzero(s["sampled"])[0]
    if len(sel):
        _, blocked = orc.intersect_rays(flat, s["rays"][sel], scene_handle=scene_handle or orc.SceneHandle(flat))
        visible[sel] = blocked == 0
    radiance = np.where(visible[:, None], s["contribution"], F(0.0)).astype(np.float32)
    return radiance, s["rays"], visible.astype(np.uint8), s["sampled"]


def irradiance_f64(env, normal, grid):
    """Binary64 midpoint quadrature of  integral L(w) max(dot(n, w), 0) d omega / pi  over the octahedral unit square on grid x grid
    points: the numpy lookup (binary32 inside, summed in binary64) times the Jacobian 4 |w|_1^3 -- what the mean of sample()'s
    unshadowed contributions estimates.  -> [3]"""
    texels = env_ref.apron(env)
    s = (np.arange(grid) + 0.5) / grid
    sx, sz = (g.reshape(-1) for g in np.meshgrid(s, s))
    qx, qz = 2.0 * sx - 1.0, 2.0 * sz - 1.0
    y = 1.0 - np.abs(qx) - np.abs(qz)
    low = y < 0.0
    x = np.where(low, (1.0 - np.abs(qz)) * np.where(qx < 0.0, -1.0, 1.0), qx)
    z = np.where(low, (1.0 - np.abs(qx)) * np.where(qz < 0.0, -1.0, 1.0), qz)
    d = np.stack([x, y, z], axis=-1)
    wv = d / np.linalg.norm(d, axis=1)[:, None]
    l1 = np.abs(wv).sum(axis=1)
    L = env_ref.lookup(None, wv.astype(np.float32), texels).astype(np.float64)
    cos_r = np.maximum(wv @ np.asarray(normal, dtype=np.float64), 0.0)
    return (L * (cos_r * 4.0 * l1 ** 3)[:, None]).sum(axis=0) / (grid * grid) / np.pi
