"""The binary32 and generator pieces that the numpy restatements under tests/ share (lit_ref.py: the render loops; direct_ref.py:
the lamp table and the light sample) -- TEST INFRASTRUCTURE.  Every numpy operation is one binary32 operation of the source it
restates, in glm's order (pt_math.hpp; numpy does not contract into FMA); the generator and sincos are the oracle's own."""
import ctypes as C

import numpy as np

F = np.float32
PI = F(3.14159265358979323846264338327950288)  # pi_f
PI2 = F(2.0) * PI                               # 2.f * pi_f, as the C expression folds it


def _dot(a, b):
    t = a * b  # glm::dot: tmp = a * b; tmp.x + tmp.y + tmp.z
    return (t[..., 0] + t[..., 1]) + t[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], axis=-1)


def _normalize(v):
    with np.errstate(divide="ignore", invalid="ignore"):
        return v * (F(1.0) / np.sqrt(_dot(v, v)))[..., None]  # v * (1 / sqrt(dot(v, v)))


def _sign(x):
    return ((F(0.0) < x).astype(np.float32) - (x < F(0.0)).astype(np.float32)).astype(np.float32)


def _xform_point(m16, p):
    """transform_point: (M * (p, 1)).xyz / w with mat4 * vec4 = (c0 x + c1 y) + (c2 z + c3 w); m16 column-major."""
    m = np.asarray(m16, dtype=np.float32)
    p = np.asarray(p, dtype=np.float32)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    row = [(m[0 + r] * x + m[4 + r] * y) + (m[8 + r] * z + m[12 + r] * F(1.0)) for r in range(4)]
    return np.stack([row[0] / row[3], row[1] / row[3], row[2] / row[3]], axis=-1)


def _sincos(orc, phi):
    s, c = np.empty_like(phi), np.empty_like(phi)
    fs, fc = C.c_float(), C.c_float()
    h = orc.lib()
    for k, x in enumerate(phi):
        h.orc_sincos(float(x), C.byref(fs), C.byref(fc))
        s[k], c[k] = fs.value, fc.value
    return s, c


class Draws:
    """thrust::minstd_rand states, one per path, advanced through the oracle (orc_rng_uniform)."""

    def __init__(self, orc, states):
        self.h = orc.lib()
        self.states = np.asarray(states, dtype=np.uint32).copy()

    def uniform(self, idx):
        out = np.empty(len(idx), dtype=np.float32)
        st = C.c_uint32()
        for k, i in enumerate(idx):
            st.value = int(self.states[i])
            out[k] = self.h.orc_rng_uniform(C.byref(st))
            self.states[i] = st.value
        return out


def stream_states(orc, indices, iteration, xor, discard):
    """Every stream of a path is keyed this way: per index a generator seeded path_seed(index, iteration) ^ xor, then
    discard(discard).  xor 0 is the material stream; the light and roulette streams have a constant each.  -> uint32[n]."""
    h = orc.lib()
    states = np.empty(len(indices), dtype=np.uint32)
    st = C.c_uint32()
    for k, index in enumerate(indices):
        st.value = h.orc_rng_seed(h.orc_path_seed(int(index), int(iteration)) ^ xor)
        if discard:
            h.orc_rng_discard(C.byref(st), int(discard))
        states[k] = st.value
    return states


def stream_draws(orc, indices, iteration, xor, discard, count):
    """The next `count` uniform() of stream_states(...), float32[n, count]."""
    draws = Draws(orc, stream_states(orc, indices, iteration, xor, discard))
    every = np.arange(len(indices))
    return np.stack([draws.uniform(every) for _ in range(count)], axis=-1)
