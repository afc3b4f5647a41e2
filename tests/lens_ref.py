"""CPU restatement of the thin lens (ptc_set_lens) in numpy binary32 -- TEST INFRASTRUCTURE: the checker of
tests/test_lens_cpu.py and tests/test_gpu_lens.py, not the thing under test.

The reference's camera is a pinhole, so the oracle (oracle/oracle.c) cannot check a lens and stays as it is.  This file restates the
primary ray under a lens from the oracle's pinned pieces -- orc_to_gpu_camera (the camera matrix), orc_path_seed / orc_rng_* (every
draw, through ref_f32.stream_draws), orc_sincos -- and, operation by operation, orc_generate_ray's u, v and direction (oracle.c:
290-293) and glm's mat4 * vec4 (ref_f32._xform_point's order).  The render loops are loop_ref's, which take `lens` as an option and
draw their primary rays from `primary` below.  lens None, or a radius of 0, is the pinhole: lit_ref._primary's rays themselves.
Every numpy operation below is one binary32 operation of section 5i's list, in its order (numpy does not contract into FMA)."""
import ctypes as C
import ctypes.util

import numpy as np

import lit_ref
from ref_f32 import PI2, F, _normalize, _sincos, _xform_point, stream_draws

LENS_XOR = 0x4C454E53  # kLensSeedXor (pt_device.hpp): "LENS"
_libm = None


def _tanf(x):
    """the platform's tanf, which orc_generate_ray and the library's make_camera both call for the viewport height"""
    global _libm
    if _libm is None:
        _libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.tanf.restype, _libm.tanf.argtypes = C.c_float, [C.c_float]
    return F(_libm.tanf(C.c_float(float(x))))


def is_on(lens):
    return lens is not None and float(F(lens[0])) > 0.0


def camera_matrix(orc, camera, w, h):
    """translate(position) * mat4_cast(rotation), 16 floats column-major (orc_to_gpu_camera)"""
    gcam = orc.OGPUCamera()
    orc.lib().orc_to_gpu_camera(C.byref(orc.camera_c(camera)), w, h, C.byref(gcam))
    return np.array(gcam.camera_matrix[:], dtype=np.float32)


def _xform_vector(m, v):
    """transform_vector: (M * (v, 0)).xyz with mat4 * vec4 = (c0 x + c1 y) + (c2 z + c3 w)"""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.stack([(m[0 + r] * x + m[4 + r] * y) + (m[8 + r] * z + m[12 + r] * F(0.0)) for r in range(3)], axis=-1)


def viewport(camera, w, h):
    """generate_ray's frame constants (the library hoists them into DCamera): (llx, lly, vw, vh), binary32"""
    vh = F(2.0) * _tanf(F(camera.vfov) / F(2.0))
    vw = (F(w) / F(h)) * vh
    llx = ((F(0.0) - vw / F(2.0)) - F(0.0) / F(2.0)) - F(0.0)
    lly = ((F(0.0) - F(0.0) / F(2.0)) - vh / F(2.0)) - F(0.0)
    return llx, lly, vw, vh


def camera_space(orc, camera, w, h, pixels, iteration):
    """Items 1 and 2 of the rule: the path stream's two draws of jitter, then dx, dy as generate_ray computes them.
    -> (dx [n], dy [n], the generators' states behind the two draws [n])"""
    lib = orc.lib()
    pixels = np.asarray(pixels, dtype=np.int64)
    fx = np.empty(len(pixels), dtype=np.float32)
    fy = np.empty(len(pixels), dtype=np.float32)
    states = np.empty(len(pixels), dtype=np.uint32)
    st = C.c_uint32()
    for k, pixel in enumerate(pixels):
        pixel = int(pixel)
        st.value = lib.orc_rng_seed(lib.orc_path_seed(pixel, iteration))
        fx[k] = F(pixel % w) + F(lib.orc_rng_uniform(C.byref(st)))
        fy[k] = F(pixel // w) + F(lib.orc_rng_uniform(C.byref(st)))
        states[k] = st.value
    llx, lly, vw, vh = viewport(camera, w, h)
    u = fx / F(w - 1)
    v = (F(h) - fy) / F(h - 1)
    return llx + vw * u, lly + vh * v, states


def lens_points(orc, pixels, iteration, radius):
    """Items 3 and 4: the lens stream's two draws and the point on the disk.  -> (lx [n], ly [n], u [n, 2])"""
    u = stream_draws(orc, np.asarray(pixels, dtype=np.int64), iteration, LENS_XOR, 0, 2)
    rho = F(radius) * np.sqrt(u[:, 0])
    phi = PI2 * u[:, 1]
    s, c = _sincos(orc, phi)
    return rho * c, rho * s, u


def rays_from_parts(m, dx, dy, lx, ly, focus):
    """Items 5 and 6: the point in focus (dx f, dy f, -f), the ray from the lens point (lx, ly, 0) through it.  -> (o, d)"""
    f = F(focus)
    px, py = dx * f, dy * f
    lens_pt = np.stack([lx, ly, np.zeros_like(lx)], axis=-1)
    to_focus = np.stack([px - lx, py - ly, np.full_like(lx, -f)], axis=-1)
    return _xform_point(m, lens_pt), _normalize(_xform_vector(m, to_focus))


def pinhole_from_parts(orc, camera, w, h, pixels, iteration):
    """generate_ray restated from the same parts (the direction through (dx, dy, -1), the origin M * (0, 0, 0, 1)): what
    tests/test_lens_cpu.py holds against lit_ref._primary, so that dx and dy above are known to be the oracle's."""
    m = camera_matrix(orc, camera, w, h)
    dx, dy, states = camera_space(orc, camera, w, h, pixels, iteration)
    d = _normalize(_xform_vector(m, np.stack([dx, dy, np.full_like(dx, F(-1.0))], axis=-1)))
    zero = F(0.0)
    o = np.array([(m[0 + r] * zero + m[4 + r] * zero) + (m[8 + r] * zero + m[12 + r] * F(1.0)) for r in range(3)], dtype=np.float32)
    return np.broadcast_to(o, d.shape).copy(), d, np.full(len(dx), F(1e-4), dtype=np.float32), states


def primary(orc, camera, w, h, pixels, iteration, lens):
    """The primary rays of `pixels` at `iteration` under lens = (radius, focus_distance), lit_ref._primary's return shape:
    (origin [n, 3], direction [n, 3], t_min [n], the path generators' states behind the jitter [n]).  None / radius 0: the pinhole."""
    if not is_on(lens):
        return lit_ref._primary(orc, camera, w, h, pixels, iteration)
    m = camera_matrix(orc, camera, w, h)
    dx, dy, states = camera_space(orc, camera, w, h, pixels, iteration)
    lx, ly, _ = lens_points(orc, pixels, iteration, lens[0])
    o, d = rays_from_parts(m, dx, dy, lx, ly, lens[1])
    return o, d, np.full(len(dx), F(1e-4), dtype=np.float32), states
