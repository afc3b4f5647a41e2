// hdr_image.hpp -- Radiance .hdr (RGBE) pictures for environment lighting (PathTracer::environment): read_hdr, flat and
// run-length-encoded scanlines, and load_environment, the picture turned into the octahedral map the tracer takes
// (ptc_environment_from_equirect).  The same rule as hdr.py (tests/test_environment_cpu.py compares the two).  Header-only.
// A pixel is four bytes r, g, b, e: value = mantissa * 2^(e - 136), and 0 when e == 0 -- exact in binary32.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/ptcore.h"

namespace hip_pt {

struct HdrImage {
  int width = 0, height = 0;
  std::vector<float> rgb;  // 3 floats per pixel, row 0 the picture's top
};

// The octahedral map of PathTracer::environment: size x size texels of three floats, texel (row j along z, column i along x) at
// rgb[3 (j size + i)], +y up
struct EnvironmentMap {
  uint32_t size = 0;
  std::vector<float> rgb;
};

// Refuses (std::runtime_error) what it does not read: a missing signature or format line, another orientation than -Y h +X w, a
// truncated or malformed scanline.
inline HdrImage read_hdr(const std::string& filename)
{
  const auto fail = [&](const std::string& why) -> std::runtime_error { return std::runtime_error("Unable to load " + filename + ": " + why); };
  std::ifstream file(filename, std::ios::binary);
  if (!file.is_open()) throw fail("cannot open the file");
  const std::string data((std::istreambuf_iterator<char>(file)), std::istreambuf_iterator<char>());
  const size_t end = data.find("\n\n");
  if ((data.rfind("#?RADIANCE", 0) != 0 && data.rfind("#?RGBE", 0) != 0) || end == std::string::npos)
    throw fail("not a Radiance picture (no #?RADIANCE header)");
  if (("\n" + data.substr(0, end) + "\n").find("\nFORMAT=32-bit_rle_rgbe\n") == std::string::npos) throw fail("FORMAT=32-bit_rle_rgbe expected");
  const size_t eol = data.find('\n', end + 2);
  if (eol == std::string::npos) throw fail("resolution line \"-Y height +X width\" expected");
  long h = 0, w = 0;
  {
    const std::string line = data.substr(end + 2, eol - (end + 2));
    char y_key[3] = {0}, x_key[3] = {0}, extra = 0;
    if (std::sscanf(line.c_str(), " %2s %ld %2s %ld %c", y_key, &h, x_key, &w, &extra) != 4 || std::string(y_key) != "-Y" || std::string(x_key) != "+X" ||
        line.find_first_not_of("-+XY0123456789 \t") != std::string::npos)
      throw fail("resolution line \"-Y height +X width\" expected");
  }
  if (w < 1 || w > 65536 || h < 1 || h > 65536) throw fail("resolution " + std::to_string(w) + " x " + std::to_string(h) + " out of range");
  const auto* buf = reinterpret_cast<const unsigned char*>(data.data()) + eol + 1;
  const size_t len = data.size() - (eol + 1);
  std::vector<unsigned char> rgbe((size_t)w * (size_t)h * 4u);
  size_t at = 0;
  for (long y = 0; y < h; ++y) {
    unsigned char* row = rgbe.data() + (size_t)y * (size_t)w * 4u;
    const std::string where = "scanline " + std::to_string(y);
    if (w >= 8 && w <= 32767 && at + 4 <= len && buf[at] == 2 && buf[at + 1] == 2 && ((long)buf[at + 2] << 8 | (long)buf[at + 3]) == w) {
      at += 4;  // a run-length-encoded scanline: the four channels one after the other
      for (int c = 0; c < 4; ++c)
        for (long x = 0; x < w;) {
          if (at >= len) throw fail(where + " is truncated");
          long count = buf[at++];
          if (count > 128) {  // a run
            count -= 128;
            if (at >= len || x + count > w) throw fail(where + ": a run leaves the scanline or the file");
            for (long k = 0; k < count; ++k) row[4 * (x + k) + c] = buf[at];
            ++at;
          } else {  // literal bytes
            if (count == 0 || at + (size_t)count > len || x + count > w)
              throw fail(where + ": a literal block of " + std::to_string(count) + " bytes leaves the scanline or the file");
            for (long k = 0; k < count; ++k) row[4 * (x + k) + c] = buf[at + (size_t)k];
            at += (size_t)count;
          }
          x += count;
        }
    } else {  // a flat scanline: w pixels of four bytes
      if (at + 4u * (size_t)w > len) throw fail(where + " is truncated");
      for (size_t k = 0; k < 4u * (size_t)w; ++k) row[k] = buf[at + k];
      at += 4u * (size_t)w;
    }
  }
  HdrImage img;
  img.width = (int)w;
  img.height = (int)h;
  img.rgb.resize((size_t)w * (size_t)h * 3u);
  for (size_t p = 0; p < (size_t)w * (size_t)h; ++p) {
    const int e = rgbe[4 * p + 3];
    const float scale = e == 0 ? 0.0f : std::ldexp(1.0f, e - 136);
    for (int c = 0; c < 3; ++c) img.rgb[3 * p + c] = (float)rgbe[4 * p + c] * scale;
  }
  return img;
}

// An equirectangular .hdr picture as an environment: size 0 = the picture's height, at most 4096.
inline std::shared_ptr<const EnvironmentMap> load_environment(const std::string& filename, float scale, int size, HdrImage* picture = nullptr)
{
  HdrImage img = read_hdr(filename);
  const int n = size > 0 ? size : (img.height < 4096 ? img.height : 4096);
  if (n < 2 || n > 4096)
    throw std::runtime_error("environment " + filename + ": a map of size " + std::to_string(n) + " is outside [2,4096] (give a size)");
  auto map = std::make_shared<EnvironmentMap>();
  map->size = (uint32_t)n;
  map->rgb.resize((size_t)n * (size_t)n * 3u);
  if (ptc_environment_from_equirect(img.rgb.data(), (uint32_t)img.width, (uint32_t)img.height, (uint32_t)n, scale, map->rgb.data()) != PTC_OK)
    throw std::runtime_error("environment " + filename + ": the conversion refused scale " + std::to_string(scale));
  if (picture) *picture = std::move(img);
  return map;
}

}  // namespace hip_pt
