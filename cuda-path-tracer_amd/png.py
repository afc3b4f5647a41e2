"""PNG pictures for image textures (PathTracer.texture_table): read_png -- 8 bits a channel, colour type 2 (RGB) or 6
(RGBA), not interlaced, all five scanline filters, inflated with the zlib module; the same rule as host/png_image.hpp
(tests/test_texture_cpu.py compares the two) -- and write_png, for the asset generator and the tests.  Rows are FLIPPED on load: a PNG's
first row is the top of the picture, a texture's row 0 is t = 0, the bottom."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def read_png(filename):
    """-> [height, width, 4] uint8, row 0 the BOTTOM row of the picture; alpha 255 for an RGB file.  ValueError, naming the file, for
    anything but an 8-bit, non-interlaced RGB / RGBA PNG."""
    with open(filename, "rb") as f:
        data = f.read()
    if data[:8] != SIGNATURE:
        raise ValueError(f"{filename}: not a PNG file")
    pos, header, idat, ended = 8, None, [], False
    while pos + 12 <= len(data) and not ended:
        (length,), kind = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + length]
        if len(body) != length or pos + 12 + length > len(data):
            raise ValueError(f"{filename}: truncated PNG chunk")
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            ended = True
        pos += 12 + length
    if header is None or not ended:
        raise ValueError(f"{filename}: a PNG without IHDR or IEND")
    width, height, depth, colour, compression, filt, interlace = header
    if depth != 8 or colour not in (2, 6) or compression != 0 or filt != 0 or interlace != 0:
        raise ValueError(f"{filename}: only 8-bit RGB or RGBA PNGs without interlacing are read (bit depth {depth}, colour type {colour}, "
                         f"interlace {interlace})")
    if not (1 <= width <= 4096 and 1 <= height <= 4096):
        raise ValueError(f"{filename}: {width} x {height}: each side must be in [1,4096]")
    bpp = 3 if colour == 2 else 4
    stride = width * bpp
    try:
        raw = zlib.decompress(b"".join(idat))
    except zlib.error as e:
        raise ValueError(f"{filename}: {e}") from None
    if len(raw) != height * (stride + 1):
        raise ValueError(f"{filename}: {len(raw)} bytes of picture data, {height * (stride + 1)} expected")
    rows = np.zeros((height, stride), dtype=np.uint8)
    prev = bytearray(stride)
    for y in range(height):
        kind = raw[y * (stride + 1)]
        line = bytearray(raw[y * (stride + 1) + 1:(y + 1) * (stride + 1)])
        if kind == 1:
            for i in range(bpp, stride):
                line[i] = (line[i] + line[i - bpp]) & 255
        elif kind == 2:
            for i in range(stride):
                line[i] = (line[i] + prev[i]) & 255
        elif kind == 3:
            for i in range(stride):
                line[i] = (line[i] + (((line[i - bpp] if i >= bpp else 0) + prev[i]) >> 1)) & 255
        elif kind == 4:
            for i in range(stride):
                line[i] = (line[i] + _paeth(line[i - bpp] if i >= bpp else 0, prev[i], prev[i - bpp] if i >= bpp else 0)) & 255
        elif kind != 0:
            raise ValueError(f"{filename}: scanline filter {kind} in row {y}")
        rows[y] = np.frombuffer(bytes(line), dtype=np.uint8)
        prev = line
    out = np.full((height, width, 4), 255, dtype=np.uint8)
    out[:, :, :bpp] = rows.reshape(height, width, bpp)
    return np.ascontiguousarray(out[::-1])


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def write_png(filename, texels, filters=None, alpha=True, header=None):
    """texels [height, width, 4] uint8 with row 0 at the BOTTOM (a texture's order: rows are flipped on the way out).  filters: per row of
    the FILE (top first) a scanline filter 0 .. 4, cycled; default 0.  alpha False writes colour type 2.  header: the five IHDR bytes
    behind the sizes, for files a reader must refuse."""
    img = np.ascontiguousarray(np.asarray(texels, dtype=np.uint8)[::-1])
    height, width = img.shape[:2]
    bpp = 4 if alpha else 3
    rows = img[:, :, :bpp].reshape(height, width * bpp).astype(np.int64)
    raw = bytearray()
    prev = np.zeros(width * bpp, dtype=np.int64)
    for y in range(height):
        kind = (filters or [0])[y % len(filters or [0])]
        cur = rows[y]
        left = np.concatenate([np.zeros(bpp, np.int64), cur[:-bpp]]) if width * bpp > bpp else np.zeros(width * bpp, np.int64)
        upleft = np.concatenate([np.zeros(bpp, np.int64), prev[:-bpp]]) if width * bpp > bpp else np.zeros(width * bpp, np.int64)
        if kind == 0:
            line = cur
        elif kind == 1:
            line = cur - left
        elif kind == 2:
            line = cur - prev
        elif kind == 3:
            line = cur - ((left + prev) >> 1)
        else:
            line = cur - np.array([_paeth(int(a), int(b), int(c)) for a, b, c in zip(left, prev, upleft)], dtype=np.int64)
        raw.append(kind)
        raw += bytes((line & 255).astype(np.uint8))
        prev = cur
    ihdr = struct.pack(">II", width, height) + bytes(header if header is not None else (8, 6 if alpha else 2, 0, 0, 0))
    with open(filename, "wb") as f:
        f.write(SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(bytes(raw), 9)) + _chunk(b"IEND", b""))
