"""A float64 restatement of the reference's A-Trous denoiser (denoising/edge_avoiding_a_trous_denoiser.cu:24-115),
vectorised over pixels: the second checker of the denoiser, next to the CPU oracle (orc_denoise, binary32).

Restated literally, including the reference's corners that this port keeps as a contract:
  - a 5x5 tap kernel whose weight is {3/8, 1/4, 1/16}[min(|dx|, |dy|)]; the step doubles while step <= filter_size;
  - per tap min(exp(-d / phi), 1) for colour, normal and position, the normal distance divided by step^2 (and
    clamped at 0), so that a zero phi gives -0/0 = NaN at the centre tap and a NaN pixel;
  - the tap coordinate clamped to [0, W] x [0, H] INCLUSIVE; a flat index past the end reads element W*H-1; a tap on
    column W or row H keeps its own view ray (generate_ray at (u + 0.5, v + 0.5)) with the depth it read;
  - the (color, back, front) <- (back, front, back) ping-pong, the result being `front`; no pass and no result for
    filter_size < 1.
The view rays are generate_ray (ray_gen.cu:34-61) in float64 on the camera matrix that orc_to_gpu_camera builds."""
import ctypes as C

import numpy as np

KERNEL = (3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)


def gpu_camera(orc, camera, w, h):
    """camera_matrix (float64, m[col][row] as in glm) and vfov of the reference's GPUCamera (camera.cpp:5-13)"""
    g = orc.OGPUCamera()
    orc.lib().orc_to_gpu_camera(C.byref(orc.camera_c(camera)), w, h, C.byref(g))
    return np.array(g.camera_matrix[:], dtype=np.float64).reshape(4, 4), float(g.vfov)


def view_rays(matrix, vfov, w, h, xs, ys):
    """generate_ray(camera, x, y) in float64 for arrays of image coordinates: (origin [3], unit directions [..., 3])"""
    aspect = w / h
    vh = 2.0 * np.tan(vfov / 2.0)
    vw = aspect * vh
    u = np.asarray(xs, dtype=np.float64) / (w - 1)
    v = (h - np.asarray(ys, dtype=np.float64)) / (h - 1)
    d = np.stack(np.broadcast_arrays(-vw / 2.0 + vw * u, -vh / 2.0 + vh * v, -1.0), axis=-1)
    wd = d @ matrix[0:3, 0:3]           # sum_j m[j][i] d_j: the matrix applied to (d, 0)
    wd /= np.linalg.norm(wd, axis=-1, keepdims=True)
    return matrix[3, 0:3].copy(), wd


def denoise_pass(color, normal, pos_grid, cval_pos, step, c_phi, n_phi, p_phi):
    """One denoising_kernel launch.  color / normal: [P, 3] float64 in row-major pixel order; pos_grid[v, u]: the tap
    position of coordinate (u, v) in [0, W] x [0, H] (own view ray, depth of the clamped index); cval_pos: pval."""
    H1, W1, _ = pos_grid.shape
    H, W = H1 - 1, W1 - 1
    P = W * H
    y, x = np.divmod(np.arange(P), W)
    cval, nval = color, normal
    s = np.zeros((P, 3))
    cum = np.zeros(P)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        for dy in range(-2, 3):
            v = np.clip(y + dy * step, 0, H)
            for dx in range(-2, 3):
                u = np.clip(x + dx * step, 0, W)
                ti = np.minimum(u + v * W, P - 1)
                ctemp = color[ti]
                t = cval - ctemp
                c_w = np.minimum(np.exp(-np.einsum("ij,ij->i", t, t) / c_phi), 1.0)
                t = nval - normal[ti]
                dist2 = np.maximum(np.einsum("ij,ij->i", t, t) / float(step * step), 0.0)
                n_w = np.minimum(np.exp(-dist2 / n_phi), 1.0)
                t = cval_pos - pos_grid[v, u]
                p_w = np.minimum(np.exp(-np.einsum("ij,ij->i", t, t) / p_phi), 1.0)
                weight = c_w * n_w * p_w
                k = KERNEL[min(abs(dx), abs(dy))]
                s += ctemp * (weight * k)[:, None]
                cum += weight * k
        return s / cum[:, None]


def tap_positions(orc, camera, w, h, depth):
    """pos_grid[v, u] for (u, v) in [0, W] x [0, H]: origin + direction(u + .5, v + .5) * depth[min(u + v W, P - 1)]"""
    matrix, vfov = gpu_camera(orc, camera, w, h)
    vv, uu = np.meshgrid(np.arange(h + 1), np.arange(w + 1), indexing="ij")
    origin, dirs = view_rays(matrix, vfov, w, h, uu + 0.5, vv + 0.5)
    ti = np.minimum(uu + vv * w, w * h - 1)
    return origin + dirs * np.asarray(depth, dtype=np.float64).reshape(-1)[ti][..., None]


def denoise_chain(orc, camera, w, h, color, normal, depth, passes, c_phi=0.45, n_phi=0.30, p_phi=0.25):
    """The outputs of the first `passes` passes ([h, w, 3] float64 each): the result of filter_size N is entry
    floor(log2 N) of the chain (a filter size only decides how many passes run)."""
    c_phi, n_phi, p_phi = (float(np.float32(x)) for x in (c_phi, n_phi, p_phi))  # the reference's weights are floats
    pos_grid = tap_positions(orc, camera, w, h, depth)
    pval = pos_grid[:h, :w].reshape(-1, 3)
    c = np.asarray(color, dtype=np.float64).reshape(-1, 3)
    n = np.asarray(normal, dtype=np.float64).reshape(-1, 3)
    # (color, back, front) <- (back, front, back) after each pass (cu:102-108); the reference returns front
    bufs = [np.zeros_like(c), np.zeros_like(c)]
    color_buf, back, front = c, 0, 1
    out = []
    step = 1
    for _ in range(passes):
        bufs[back] = denoise_pass(color_buf, n, pos_grid, pval, step, c_phi, n_phi, p_phi)
        color_buf, back, front = bufs[back], front, back
        out.append(bufs[front].reshape(h, w, 3))
        step *= 2
    return out


def passes_of(filter_size):
    """number of passes the reference runs: step = 1, 2, 4, ... while step <= filter_size"""
    n, step = 0, 1
    while step <= filter_size:
        n, step = n + 1, step * 2
    return n


def denoise(orc, camera, w, h, color, normal, depth, filter_size=10, c_phi=0.45, n_phi=0.30, p_phi=0.25):
    """The reference's result for one filter size ([h, w, 3] float64), or None when no pass runs."""
    k = passes_of(filter_size)
    if k == 0:
        return None
    return denoise_chain(orc, camera, w, h, color, normal, depth, k, c_phi, n_phi, p_phi)[-1]


# ---- the cases the denoiser tests share (tests/test_denoise_ref_cpu.py, tests/test_gpu_denoise.py) ----
# filter sizes: every pass count 1..8, both ends of the GUI slider (1-100, gui.cpp:87) and step 128 past it;
# between them every k_denoise_lds<1..32> template and k_denoise at steps 64 and 128
FILTER_SIZES = (1, 2, 3, 8, 16, 31, 32, 63, 64, 100, 200)
DEFAULT_WEIGHTS = (0.45, 0.30, 0.25)
# (c_phi, n_phi, p_phi): the defaults, the ends of the sliders (0-1, gui.cpp:88-89), a mixed set, each weight at 0
WEIGHT_SETS = (DEFAULT_WEIGHTS, (1.0, 1.0, 1.0), (0.01, 0.01, 0.01), (0.2, 0.8, 0.05),
               (0.0, 0.30, 0.25), (0.45, 0.0, 0.25), (0.45, 0.30, 0.0))


def low_camera(pkg):
    """a camera on the heightfield scene whose bottom rows and right column cross the spheres and their edges against
    the ground: contrast on the borders, where the clamped and off-by-one taps are (with the scene's own camera the
    bottom rows are smooth ground and a tap row clamped one row short changes nothing)"""
    return pkg.scenes._camera_from_look_at((0.9, 1.1, 2.6), (0.3, 0.9, 0.0), vfov_deg=50.0)
