"""A numpy restatement of the denoiser's albedo rule (cuda-path-tracer_amd/csrc/pt_demodulate.hpp).

In binary32, one operation a line, what the kernels and ptc_check_demodulate compute per channel:
    e           = albedo > 1/64 ? albedo : 1/64       (a NaN, a zero of either sign and a negative value take the floor)
    irradiance  = colour / e
    colour'     = filtered * e
and in float64 the whole denoise under "denoise_albedo": demodulate, the reference's passes (tests/denoise_ref.py), remodulate."""
import numpy as np

import denoise_ref as dr

ALBEDO_FLOOR = np.float32(1.0) / np.float32(64.0)


def effective(albedo):
    a = np.asarray(albedo, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(a > ALBEDO_FLOOR, a, ALBEDO_FLOOR).astype(np.float32)


def demodulate(colour, albedo):
    """-> (irradiance, effective albedo), float32 of the arrays' shape"""
    e = effective(albedo)
    with np.errstate(all="ignore"):
        return (np.asarray(colour, dtype=np.float32) / e).astype(np.float32), e


def remodulate(filtered, albedo):
    with np.errstate(all="ignore"):
        return (np.asarray(filtered, dtype=np.float32) * effective(albedo)).astype(np.float32)


def effective_f64(albedo):
    """the same choice on the same binary32 values, the result carried in float64"""
    a = np.asarray(albedo, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(a > float(ALBEDO_FLOOR), a, float(ALBEDO_FLOOR))


def irradiance_f64(colour, albedo):
    with np.errstate(all="ignore"):
        return np.asarray(colour, dtype=np.float64) / effective_f64(albedo)


def demodulated_denoise(orc, camera, w, h, colour, albedo, normal, depth, filter_size=10, c_phi=0.45, n_phi=0.30, p_phi=0.25):
    """ptc_denoise under "denoise_albedo" 1 in float64 ([h, w, 3]), or None when no pass runs: the passes of denoise_ref on
    colour / e, their result times e"""
    k = dr.passes_of(filter_size)
    if k == 0:
        return None
    e = effective_f64(albedo).reshape(h, w, 3)
    irr = irradiance_f64(colour, albedo).reshape(h, w, 3)
    out = dr.denoise_chain(orc, camera, w, h, irr, normal, depth, k, c_phi, n_phi, p_phi)[-1]
    with np.errstate(all="ignore"):
        return out * e
