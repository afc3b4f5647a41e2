"""The display transform (csrc/pt_display.hpp) restated in numpy, operation for operation: every float line is one
np.float32 operation, the histogram and the level are Python integers.  The checker of tests/test_display_cpu.py and
tests/test_gpu_display.py, never the thing under test.  `params`: anything with the fields of ptc_display_params (pkg.Display)."""
import numpy as np

F = np.float32
BINS, BIN_BASE = 256, 888
BELOW, REJECTED = -1, -2
CAP = F(1048576.0)


def bins_of(rgb):
    """Per pixel of rgb [n, >= 3]: its bin 0 .. 255, BELOW or REJECTED."""
    rgb = np.asarray(rgb, dtype=np.float32)
    with np.errstate(all="ignore"):
        yr = F(0.2126) * rgb[:, 0]
        yg = F(0.7152) * rgb[:, 1]
        yb = F(0.0722) * rgb[:, 2]
        s = yr + yg
        y = s + yb
        rejected = ~(y >= F(0)) | ~(y <= np.finfo(np.float32).max)
        below = ~rejected & (y < F(2.0 ** -16))
    k = (y.view(np.uint32) >> np.uint32(20)).astype(np.int64) - BIN_BASE
    out = np.minimum(k, BINS - 1)
    out[below] = BELOW
    out[rejected] = REJECTED
    return out


def level_bin(hist, low_permille, high_permille):
    """The mean bin of the histogram's trimmed middle, rounded to nearest; -1 for an empty histogram."""
    h = [int(x) for x in hist]
    n = sum(h)
    lo = n * int(low_permille) // 1000
    hi = n - n * (1000 - int(high_permille)) // 1000
    cum = K = S = 0
    for k in range(BINS):
        kept = max(0, min(cum + h[k], hi) - max(cum, lo))
        K += kept
        S += k * kept
        cum += h[k]
    return (2 * S + K) // (2 * K) if K else -1


def level_of(m):
    return np.array([(m + BIN_BASE) << 20], dtype=np.uint32).view(np.float32)[0]


def scale_of(m, key, exposure):
    if m < 0:
        return F(exposure)
    q = F(key) / level_of(m)
    return q * F(exposure)


def meter(rgb, params):
    """What ptc_exposure_info reports for the pixels rgb [n, >= 3] under params."""
    rgb = np.asarray(rgb, dtype=np.float32).reshape(-1, np.shape(rgb)[-1])
    n = len(rgb)
    if not params.metering:
        return {"pixels": n, "counted": 0, "below": 0, "rejected": 0, "level_bin": -1, "level": F(0), "scale": F(params.exposure),
                "histogram": np.zeros(BINS, dtype=np.uint32)}
    b = bins_of(rgb)
    hist = np.bincount(b[b >= 0], minlength=BINS).astype(np.uint32)
    m = level_bin(hist, params.low_permille, params.high_permille)
    return {"pixels": n, "counted": int(hist.sum()), "below": int(np.sum(b == BELOW)), "rejected": int(np.sum(b == REJECTED)),
            "level_bin": m, "level": level_of(m) if m >= 0 else F(0), "scale": scale_of(m, params.key, params.exposure),
            "histogram": hist}


def map_channels(rgb, scale, params):
    """Exposure and curve on every channel of rgb [..., >= 3] -> [..., 3] float32: what k_preview's lines then encode."""
    c = np.asarray(rgb, dtype=np.float32)[..., :3]
    scale = F(scale)
    with np.errstate(all="ignore"):
        e = c * scale
        x = np.where(e > F(0), e, F(0)).astype(np.float32)
        x = np.where(x < CAP, x, CAP).astype(np.float32)
        curve = int(params.curve)
        if curve == 1:
            w2 = F(params.white) * F(params.white)
            q = x / w2
            p = F(1) + q
            num = x * p
            d = F(1) + x
            return (num / d).astype(np.float32)
        if curve == 2:
            a = F(2.51) * x
            b = a + F(0.03)
            num = x * b
            c2 = F(2.43) * x
            d = c2 + F(0.59)
            f = x * d
            den = f + F(0.14)
            return (num / den).astype(np.float32)
        return x


def show(rgb, params):
    """Meter and map: (mapped [..., 3], info)."""
    info = meter(np.asarray(rgb, dtype=np.float32).reshape(-1, np.shape(rgb)[-1]), params)
    return map_channels(rgb, info["scale"], params), info


def same_info(a, b):
    """Two exposure infos, bit for bit (the floats compared by their bits)."""
    for k in ("pixels", "counted", "below", "rejected", "level_bin"):
        if int(a[k]) != int(b[k]):
            return False
    for k in ("level", "scale"):
        if np.float32(a[k]).view(np.uint32) != np.float32(b[k]).view(np.uint32):
            return False
    return np.array_equal(np.asarray(a["histogram"], dtype=np.uint32), np.asarray(b["histogram"], dtype=np.uint32))


def hostile_pixels():
    """The values the metering and the curves must survive, [n, 3] float32: every bin edge as_float(k << 20), k = 880 .. 1150, and its
    predecessor, as grey pixels; +-0, denormals, negatives, +-inf and NaN in each channel; 2^-16 and 2^16 and their neighbours."""
    edges = (np.arange(880, 1151, dtype=np.uint32) << np.uint32(20))
    vals = np.concatenate([edges, edges - np.uint32(1)]).view(np.float32)
    px = [np.repeat(vals[:, None], 3, axis=1)]
    # a grey pixel's luminance is not its value exactly (the weights sum to 1 only nearly): the edges again, in one channel each
    for ch in range(3):
        p = np.zeros((len(vals), 3), dtype=np.float32)
        p[:, ch] = vals
        px.append(p)
    tiny = np.array([1, 0x7fffff, 0x800000], dtype=np.uint32).view(np.float32)  # smallest and largest denormal, smallest normal
    special = np.concatenate([[F(0.0), F(-0.0)], tiny, -tiny, [F(-1.0), F(-1e30), F(np.inf), F(-np.inf), F(np.nan),
                                                                 np.finfo(np.float32).max, F(3e38)]]).astype(np.float32)
    for ch in range(3):
        p = np.full((len(special), 3), 0.25, dtype=np.float32)
        p[:, ch] = special
        px.append(p)
        z = np.zeros((len(special), 3), dtype=np.float32)
        z[:, ch] = special
        px.append(z)
    for base in (F(2.0 ** -16), F(2.0 ** 16), F(2.0 ** 20)):
        n3 = np.array([np.nextafter(base, F(0)), base, np.nextafter(base, F(np.inf))], dtype=np.float32)
        px.append(np.repeat(n3[:, None], 3, axis=1))
        for ch in range(3):
            p = np.zeros((3, 3), dtype=np.float32)
            p[:, ch] = n3
            px.append(p)
    px.append(np.array([[np.inf, -np.inf, 0.0], [np.inf, np.inf, np.inf], [3e38, 3e38, 3e38], [np.nan, np.nan, np.nan]], dtype=np.float32))
    return np.ascontiguousarray(np.concatenate(px, axis=0), dtype=np.float32)


def lognormal_image(n, seed=5, sigma=2.0, mu=-1.0):
    """n pixels whose channels are log-normal: a natural HDR frame's histogram, spread over some ten octaves."""
    rng = np.random.default_rng(seed)
    return np.exp(rng.normal(mu, sigma, size=(n, 3))).astype(np.float32)
