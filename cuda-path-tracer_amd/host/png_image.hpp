// png_image.hpp -- PNG pictures for image textures (PathTracer::set_textures): read_png -- 8 bits a channel, colour
// type 2 (RGB) or 6 (RGBA), not interlaced, all five scanline filters, inflated with zlib (linked into hip_pt only).  The same rule as
// png.py (tests/test_texture_cpu.py compares the two).  Rows are FLIPPED on load: a PNG's first row is the top of the picture, a
// texture's row 0 is t = 0, the bottom.  Header-only.
#pragma once

#include <zlib.h>

#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

namespace hip_pt {

struct PngImage {
  int width = 0, height = 0;
  std::vector<uint8_t> rgba;  // width * height * 4, row 0 the BOTTOM row of the picture; alpha 255 for an RGB file
};

inline PngImage read_png(const std::string& filename)
{
  std::ifstream file(filename, std::ios::binary);
  if (!file.is_open()) throw std::runtime_error(filename + ": cannot open the file");
  const std::vector<unsigned char> data((std::istreambuf_iterator<char>(file)), std::istreambuf_iterator<char>());
  static const unsigned char kSignature[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  if (data.size() < 8 || !std::equal(kSignature, kSignature + 8, data.begin())) throw std::runtime_error(filename + ": not a PNG file");
  auto be32 = [&](size_t at) { return ((uint32_t)data[at] << 24) | ((uint32_t)data[at + 1] << 16) | ((uint32_t)data[at + 2] << 8) | data[at + 3]; };
  size_t pos = 8;
  bool have_header = false, ended = false;
  uint32_t width = 0, height = 0;
  unsigned char tail[5] = {0, 0, 0, 0, 0};
  std::vector<unsigned char> idat;
  while (pos + 12 <= data.size() && !ended) {
    const size_t length = be32(pos);
    if (pos + 12 + length > data.size()) throw std::runtime_error(filename + ": truncated PNG chunk");
    const std::string kind(data.begin() + (long)pos + 4, data.begin() + (long)pos + 8);
    const unsigned char* body = data.data() + pos + 8;
    if (kind == "IHDR" && length == 13) {
      width = be32(pos + 8);
      height = be32(pos + 12);
      for (int i = 0; i < 5; ++i) tail[i] = body[8 + i];
      have_header = true;
    } else if (kind == "IDAT") {
      idat.insert(idat.end(), body, body + length);
    } else if (kind == "IEND") {
      ended = true;
    }
    pos += 12 + length;
  }
  if (!have_header || !ended) throw std::runtime_error(filename + ": a PNG without IHDR or IEND");
  if (tail[0] != 8 || (tail[1] != 2 && tail[1] != 6) || tail[2] != 0 || tail[3] != 0 || tail[4] != 0)
    throw std::runtime_error(filename + ": only 8-bit RGB or RGBA PNGs without interlacing are read (bit depth " + std::to_string(tail[0]) +
                             ", colour type " + std::to_string(tail[1]) + ", interlace " + std::to_string(tail[4]) + ")");
  if (width < 1 || width > 4096 || height < 1 || height > 4096)
    throw std::runtime_error(filename + ": " + std::to_string(width) + " x " + std::to_string(height) + ": each side must be in [1,4096]");
  const size_t bpp = tail[1] == 2 ? 3 : 4, stride = (size_t)width * bpp;
  std::vector<unsigned char> raw((size_t)height * (stride + 1));
  uLongf got = (uLongf)raw.size();
  if (uncompress(raw.data(), &got, idat.data(), (uLong)idat.size()) != Z_OK || got != raw.size())
    throw std::runtime_error(filename + ": the picture data does not inflate to " + std::to_string(raw.size()) + " bytes");
  PngImage img;
  img.width = (int)width;
  img.height = (int)height;
  img.rgba.assign((size_t)width * height * 4, 255);
  std::vector<unsigned char> prev(stride, 0), line(stride);
  for (size_t y = 0; y < height; ++y) {
    const unsigned char kind = raw[y * (stride + 1)];
    const unsigned char* src = raw.data() + y * (stride + 1) + 1;
    if (kind > 4) throw std::runtime_error(filename + ": scanline filter " + std::to_string(kind) + " in row " + std::to_string(y));
    for (size_t i = 0; i < stride; ++i) {
      const int a = i >= bpp ? line[i - bpp] : 0, b = prev[i], c = i >= bpp ? prev[i - bpp] : 0;
      int pred = 0;
      if (kind == 1) pred = a;
      else if (kind == 2) pred = b;
      else if (kind == 3) pred = (a + b) >> 1;
      else if (kind == 4) {
        const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
        pred = pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
      }
      line[i] = (unsigned char)((src[i] + pred) & 255);
    }
    uint8_t* dst = img.rgba.data() + (size_t)(height - 1 - y) * width * 4;  // the flip
    for (size_t x = 0; x < width; ++x)
      for (size_t k = 0; k < bpp; ++k) dst[4 * x + k] = line[bpp * x + k];
    prev = line;
  }
  return img;
}

}  // namespace hip_pt
