"""A numpy restatement of the variance-guided A-Trous mode (ptc_set_param "denoise_variance"), vectorised over
pixels, on tests/denoise_ref.py's helpers (the camera, the tap positions, the kernel weights, the pass count): the reference of
tests/test_denoise_variance_cpu.py (against ptc_check_denoise_variance) and tests/test_gpu_denoise_variance.py (against the kernels).

The rule, literally:
  - the estimate: a 7 x 7 window at one-pixel spacing, coordinates clamped to [0, W-1] x [0, H-1]; tap weights
    g = exp(-(|dn|^2 / n_phi + |dx|^2 / p_phi)); m = sum g c / sum g per channel, then v = sum g |c - m|^2 / sum g over the channels;
  - per pass the prefiltered variance of the centre pixel: (1 2 1; 2 4 2; 1 2 1) / 16 of the current variance plane at one-pixel
    spacing, the same clamp;
  - a pass at step s: denoise_ref.denoise_pass with the colour factor exp(-|dc|^2 / (sigma vbar + FLOOR)); a tap's variance is read
    by the tap's index; c' = sum w c / sum w and v' = sum w^2 v / (sum w)^2;
  - the ping-pong of the plain passes, v' beside c'.
`dtype` float64 is the reference; float32 runs every array operation in binary32 and measures what the number format costs (the
tests' tolerance comes from that distance, never from the library's output)."""
import numpy as np

import denoise_ref as dr

FLOOR = 2.0 ** -53      # dvar::kVarianceFloor
RADIUS = 3              # dvar::kVarRadius
SIGMAS = (4.0, 8.0, 16.0)
DEFAULT_SIGMA = 16.0    # chosen by the sweep of profiles/denoise_variance.txt
# (n_phi, p_phi): the defaults of the plain passes and a mixed set (color_weight is not read in this mode)
WEIGHT_SETS = ((0.30, 0.25), (0.8, 0.05))
FILTER_SIZES = (1, 3, 16, 100)


def _ignore():
    return np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def variance_estimate(color, normal, pos, n_phi, p_phi):
    """color, normal, pos: [h, w, 3] of one dtype -> the variance plane [h, w]"""
    h, w, _ = color.shape
    ys, xs = np.mgrid[0:h, 0:w]
    taps = [(np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)) for dy in range(-RADIUS, RADIUS + 1) for dx in range(-RADIUS, RADIUS + 1)]
    with _ignore():
        def weight(v, u):
            t = normal - normal[v, u]
            dn = (t * t).sum(-1)
            t = pos - pos[v, u]
            dp = (t * t).sum(-1)
            return np.exp(-(dn / n_phi + dp / p_phi))
        sg = np.zeros((h, w), dtype=color.dtype)
        sgc = np.zeros_like(color)
        for v, u in taps:   # sweep 1
            g = weight(v, u)
            sg += g
            sgc += g[..., None] * color[v, u]
        m = sgc / sg[..., None]
        acc = np.zeros((h, w), dtype=color.dtype)
        for v, u in taps:   # sweep 2
            t = color[v, u] - m
            acc += weight(v, u) * (t * t).sum(-1)
        return acc / sg


def prefilter(var):
    """[h, w] -> its 3 x 3 Gaussian, coordinates clamped to the image"""
    h, w = var.shape
    ys, xs = np.mgrid[0:h, 0:w]
    out = np.zeros_like(var)
    with _ignore():
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                k = var.dtype.type((2 - abs(dx)) * (2 - abs(dy)) / 16.0)
                out += k * var[np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)]
    return out


def guided_pass(color, var, normal, pos_grid, cval_pos, step, sigma, n_phi, p_phi):
    """One guided pass.  color, normal: [P, 3]; var: [P]; pos_grid[v, u]: denoise_ref.tap_positions; cval_pos: [P, 3]
    -> (colour [P, 3], variance [P])"""
    H1, W1, _ = pos_grid.shape
    H, W = H1 - 1, W1 - 1
    P = W * H
    y, x = np.divmod(np.arange(P), W)
    dt = color.dtype.type
    s = np.zeros((P, 3), dtype=color.dtype)
    sv = np.zeros(P, dtype=color.dtype)
    cum = np.zeros(P, dtype=color.dtype)
    with _ignore():
        denom = dt(sigma) * prefilter(var.reshape(H, W)).reshape(-1) + dt(FLOOR)
        for dy in range(-2, 3):
            v = np.clip(y + dy * step, 0, H)
            for dx in range(-2, 3):
                u = np.clip(x + dx * step, 0, W)
                ti = np.minimum(u + v * W, P - 1)
                ctemp = color[ti]
                t = color - ctemp
                c_w = np.minimum(np.exp(-np.einsum("ij,ij->i", t, t) / denom), dt(1.0))
                t = normal - normal[ti]
                dist2 = np.maximum(np.einsum("ij,ij->i", t, t) / dt(step * step), dt(0.0))
                n_w = np.minimum(np.exp(-dist2 / dt(n_phi)), dt(1.0))
                t = cval_pos - pos_grid[v, u]
                p_w = np.minimum(np.exp(-np.einsum("ij,ij->i", t, t) / dt(p_phi)), dt(1.0))
                wk = c_w * n_w * p_w * dt(dr.KERNEL[min(abs(dx), abs(dy))])
                s += ctemp * wk[:, None]
                sv += wk * wk * var[ti]
                cum += wk
        return s / cum[:, None], sv / (cum * cum)


def guided_chain(orc, camera, w, h, color, normal, depth, passes, sigma=DEFAULT_SIGMA, n_phi=0.30, p_phi=0.25, dtype=np.float64):
    """dict(variance [h, w]: the estimate; prefiltered [h, w]: its 3 x 3 Gaussian; colour: the outputs of the first `passes` passes,
    [h, w, 3] each -- filter size N's result is entry floor(log2 N); var: the variance planes beside them)"""
    n_phi, p_phi, sigma = (float(np.float32(x)) for x in (n_phi, p_phi, sigma))  # the library's weights are floats
    pos_grid = dr.tap_positions(orc, camera, w, h, depth).astype(dtype)
    pval = pos_grid[:h, :w].reshape(-1, 3)
    c = np.asarray(color, dtype=dtype).reshape(-1, 3)
    n = np.asarray(normal, dtype=dtype).reshape(-1, 3)
    dt = np.dtype(dtype).type
    var = variance_estimate(c.reshape(h, w, 3), n.reshape(h, w, 3), pos_grid[:h, :w], dt(n_phi), dt(p_phi))
    out = {"variance": var, "prefiltered": prefilter(var), "colour": [], "var": []}
    v = var.reshape(-1)
    step = 1
    for _ in range(passes):
        c, v = guided_pass(c, v, n, pos_grid, pval, step, sigma, n_phi, p_phi)
        out["colour"].append(c.reshape(h, w, 3))
        out["var"].append(v.reshape(h, w))
        step *= 2
    return out


def guided(orc, camera, w, h, color, normal, depth, filter_size, sigma=DEFAULT_SIGMA, n_phi=0.30, p_phi=0.25, dtype=np.float64):
    """(variance [h, w], result [h, w, 3] or None when no pass runs) for one filter size"""
    ch = guided_chain(orc, camera, w, h, color, normal, depth, dr.passes_of(filter_size), sigma, n_phi, p_phi, dtype)
    return ch["variance"], (ch["colour"][-1] if ch["colour"] else None)


# ---- the synthetic planes the CPU tests feed the library ----
def synthetic_planes(w, h, seed):
    """colour with two flat regions, a low-contrast and a high-contrast edge and noise; normals of two orientations across a diagonal;
    a depth ramp with a step: every edge-stopping term at work at every frame size"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    colour = np.where((xs * 2 >= w)[..., None], 0.65, 0.5) * np.array([1.0, 0.9, 0.8])
    colour = colour + np.where((ys * 3 >= 2 * h)[..., None], 0.6, 0.0) + rng.normal(0.0, 0.05, (h, w, 3))
    normal = np.where((xs + ys >= (w + h) // 2)[..., None], np.array([0.0, 0.6, 0.8]), np.array([0.0, 0.0, 1.0]))
    depth = 2.0 + 0.01 * xs + 0.004 * ys + np.where(xs * 4 >= 3 * w, 0.7, 0.0)
    return colour.astype(np.float32), normal.astype(np.float32), depth.astype(np.float32)


EDGE_SIZE = 64
EDGE_NOISES = (0.02, 0.1, 0.3)
EDGE_DEPTH = 0.01  # (so close to the eye that the 64 x 64 positions are flat against p_phi: 1e-4 of it across the frame)


def edge_image(noise, seed=1):
    """the 64 x 64 image of the issue's table: an edge from 0.5 to 0.65 down the middle, flat normals, flat positions, Gaussian noise
    -> (clean [h, w, 3] float64, noisy float32, normal float32, depth float32, band [h, w] bool: 6 pixels around the edge)"""
    n = EDGE_SIZE
    clean = np.full((n, n, 3), 0.5)
    clean[:, n // 2:] = 0.65
    noisy = (clean + np.random.default_rng(seed).normal(0.0, noise, clean.shape)).astype(np.float32)
    normal = np.zeros((n, n, 3), dtype=np.float32)
    normal[..., 2] = 1.0
    depth = np.full((n, n), EDGE_DEPTH, dtype=np.float32)
    band = np.zeros((n, n), dtype=bool)
    band[:, n // 2 - 3:n // 2 + 3] = True
    return clean, noisy, normal, depth, band


def rmse(a, b, mask=None):
    d = (np.asarray(a, dtype=np.float64) - b) ** 2
    return float(np.sqrt((d[mask] if mask is not None else d).mean()))


# ---- the tolerance the tests share ----
BOUND = 1e-5  # the project's bound for the denoiser (tests/test_gpu_denoise.py): 1e-5 x max(1, M), M the largest value the filter sees


def tolerance(scale, binary32_distance):
    """BOUND x scale, or four times the distance of the binary32 restatement from the float64 one where that is larger (the practice of
    tests/light_f64.py); scale: max(1, M), for a colour and for a variance alike"""
    bound = BOUND * scale
    return bound if binary32_distance <= bound else 4.0 * binary32_distance


def assert_close(got, want, tol, what):
    """every value: non-finite in the same places, |got - want| <= tol elsewhere"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bad_got, bad_want = ~np.isfinite(got), ~np.isfinite(want)
    assert np.array_equal(bad_got, bad_want), (what, int(bad_got.sum()), int(bad_want.sum()))
    ok = ~bad_want
    if ok.any():
        err = float(np.max(np.abs(got[ok] - want[ok])))
        assert err <= tol, (what, err, tol)
