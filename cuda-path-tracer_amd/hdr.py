"""Radiance .hdr (RGBE) images for environment lighting (PathTracer.environment): read_hdr -- flat and
run-length-encoded scanlines, the same rule as host/hdr_image.hpp (tests/test_environment_cpu.py compares the two) --, write_hdr (the
flat form and the run-length form, for the asset generator and the tests) and environment_from_equirect, the library's conversion of an
equirectangular image to the octahedral map the tracer takes.

A pixel is four bytes r, g, b, e: value = mantissa * 2^(e - 136), and 0 when e == 0 -- exact in binary32."""
import ctypes as C

import numpy as np

from . import _capi


def _fail(filename, why):
    raise ValueError(f"Unable to load {filename}: {why}")


def read_hdr(filename):
    """-> [height, width, 3] float32, row 0 the image's top.  Refuses (ValueError) what it does not read: a missing signature or
    format line, another orientation than -Y h +X w, a truncated or malformed scanline."""
    with open(filename, "rb") as f:
        data = f.read()
    end = data.find(b"\n\n")
    if not (data.startswith(b"#?RADIANCE") or data.startswith(b"#?RGBE")) or end < 0:
        _fail(filename, "not a Radiance picture (no #?RADIANCE header)")
    if b"FORMAT=32-bit_rle_rgbe" not in data[:end].split(b"\n"):
        _fail(filename, "FORMAT=32-bit_rle_rgbe expected")
    eol = data.find(b"\n", end + 2)
    dims = data[end + 2:eol].split() if eol >= 0 else []
    if len(dims) != 4 or dims[0] != b"-Y" or dims[2] != b"+X" or not dims[1].isdigit() or not dims[3].isdigit():
        _fail(filename, "resolution line \"-Y height +X width\" expected")
    h, w = int(dims[1]), int(dims[3])
    if not (1 <= w <= 65536 and 1 <= h <= 65536):
        _fail(filename, f"resolution {w} x {h} out of range")
    buf = np.frombuffer(data, dtype=np.uint8, offset=eol + 1)
    rgbe = np.empty((h, w, 4), dtype=np.uint8)
    at = 0
    for y in range(h):
        if 8 <= w <= 32767 and at + 4 <= len(buf) and buf[at] == 2 and buf[at + 1] == 2 and (int(buf[at + 2]) << 8 | int(buf[at + 3])) == w:
            at += 4  # a run-length-encoded scanline: the four channels one after the other
            for c in range(4):
                x = 0
                while x < w:
                    if at >= len(buf):
                        _fail(filename, f"scanline {y} is truncated")
                    count = int(buf[at])
                    at += 1
                    if count > 128:  # a run
                        count -= 128
                        if at >= len(buf) or x + count > w:
                            _fail(filename, f"scanline {y}: a run leaves the scanline or the file")
                        rgbe[y, x:x + count, c] = buf[at]
                        at += 1
                    else:  # literal bytes
                        if count == 0 or at + count > len(buf) or x + count > w:
                            _fail(filename, f"scanline {y}: a literal block of {count} bytes leaves the scanline or the file")
                        rgbe[y, x:x + count, c] = buf[at:at + count]
                        at += count
                    x += count
        else:  # a flat scanline: w pixels of four bytes
            if at + 4 * w > len(buf):
                _fail(filename, f"scanline {y} is truncated")
            rgbe[y] = buf[at:at + 4 * w].reshape(w, 4)
            at += 4 * w
    scale = np.ldexp(np.float32(1.0), rgbe[..., 3].astype(np.int32) - 136).astype(np.float32)
    scale[rgbe[..., 3] == 0] = 0.0
    return (rgbe[..., :3].astype(np.float32) * scale[..., None]).astype(np.float32)


def to_rgbe(image):
    """[h, w, 3] floats >= 0 -> [h, w, 4] uint8: the largest component's exponent, mantissas truncated (the usual float2rgbe)"""
    image = np.asarray(image, dtype=np.float32)
    top = image.max(axis=-1)
    m, e = np.frexp(top)
    out = np.zeros(image.shape[:2] + (4,), dtype=np.uint8)
    ok = top > 1e-32
    factor = np.where(ok, m * 256.0 / np.where(ok, top, 1.0), 0.0)
    out[..., :3] = np.clip(image * factor[..., None], 0, 255).astype(np.uint8)
    out[..., 3] = np.where(ok, e + 128, 0).astype(np.uint8)
    out[~ok] = 0
    return out


def write_hdr(filename, image, rle=False):
    """image: [h, w, 3] floats (encoded by to_rgbe) or [h, w, 4] uint8 RGBE bytes as they are.  rle: run-length-encoded scanlines
    (needs 8 <= w <= 32767)."""
    image = np.asarray(image)
    rgbe = image if image.dtype == np.uint8 and image.shape[-1] == 4 else to_rgbe(image)
    h, w = rgbe.shape[:2]
    out = [b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n", f"-Y {h} +X {w}\n".encode()]
    if not rle:
        out.append(rgbe.tobytes())
    else:
        assert 8 <= w <= 32767
        for y in range(h):
            out.append(bytes([2, 2, w >> 8, w & 255]))
            for c in range(4):
                row, x = rgbe[y, :, c], 0
                while x < w:
                    run = 1
                    while x + run < w and run < 127 and row[x + run] == row[x]:
                        run += 1
                    if run >= 4:
                        out.append(bytes([128 + run, int(row[x])]))
                        x += run
                        continue
                    lit = x  # literals up to the next run of four, at most 128
                    while lit < w and lit - x < 128 and not (lit + 3 < w and row[lit] == row[lit + 1] == row[lit + 2] == row[lit + 3]):
                        lit += 1
                    out.append(bytes([lit - x]) + row[x:lit].tobytes())
                    x = lit
    with open(filename, "wb") as f:
        f.write(b"".join(out))


def environment_from_equirect(image, size=None, scale=1.0):
    """An equirectangular image [h, w, 3] (row 0 up, the centre the direction -z) -> the octahedral map [size, size, 3] float32 that
    PathTracer.environment takes (ptc_environment_from_equirect).  size: the image's height by default, at most 4096."""
    image = np.ascontiguousarray(image, dtype=np.float32)
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError(f"an equirectangular image is [h, w, 3], got shape {image.shape}")
    n = min(image.shape[0], 4096) if size is None else int(size)
    if not 2 <= n <= 4096:
        raise ValueError(f"environment size must be in [2,4096], got {n}")
    out = np.empty((n, n, 3), dtype=np.float32)
    rc = _capi.lib().ptc_environment_from_equirect(image.ctypes.data_as(C.c_void_p), image.shape[1], image.shape[0], n, float(scale),
                                                   out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise ValueError(f"ptc_environment_from_equirect refused (size {n}, scale {scale})")
    return out
