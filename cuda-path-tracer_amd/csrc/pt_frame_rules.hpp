// pt_frame_rules.hpp -- the sizing rule of ptc_resize: how many frames a context keeps in flight and how they are dealt to its
// slots.  Shared by ptc_resize (ptcore.cpp) and the host's check (ptc_check_frame_plan, tests/test_frame_plan_cpu.py); pure
// arithmetic, the only place the rule lives.
#pragma once

#include <algorithm>

#include "../../include/ptcore.h"
#include "pt_device.hpp"

namespace pt {

// in-flight path state a context allocates when the caller has not chosen frames_in_flight ...
constexpr uint64_t kAutoFrameBytes = 24ull << 30;
// ... divided by these bytes per pixel and frame in flight, without and with "prefold".  They are the DIVISORS of the budget and
// decide how many frames fly at 4K, so they stay as they are; they are not the sum of the allocations, which has grown by a
// buffer since.  By the allocation list of ptc_resize a pixel of a frame in flight takes two path sets of 40 B, hit records of
// 32 B, slow_list 4 B, worklist 4 B and staging 32 B = 152 B, and with "prefold" a second set of hit records and next_flags,
// 33 B more = 185 B (chunk counts, tile descriptors and beam entries are small change per pixel; "ray_sort" adds 5 B).
constexpr uint64_t kAutoBytesPerPixel = 148, kAutoBytesPerPixelPrefold = 181;
// single-frame slots of a context that batches (include/ptcore.h: viewer-style use keeps eight frames in flight as well)
constexpr int kSingleSlots = 8;

// The sizing rule of ptc_resize, the only place it lives (ptc_check_frame_plan shows it to the tests): how many frames are in
// flight, how many of them share the launches of a slot, how many such slots there are and how many single-frame slots beside
// them, and whether samples are staged (k_accumulate) or shaded straight into the framebuffers (one frame in flight).
inline ptc_frame_plan frame_plan(uint32_t width, uint32_t height, int frames_in_flight, bool frames_auto, int batch_frames, bool prefold)
{
  const uint64_t P = (uint64_t)width * height;
  int frames = std::max(1, frames_in_flight);
  if (frames_auto) {
    const uint64_t per_frame = (prefold ? kAutoBytesPerPixelPrefold : kAutoBytesPerPixel) * P;
    frames = (int)std::min<uint64_t>((uint64_t)frames, std::max<uint64_t>(1ull, kAutoFrameBytes / per_frame));
  }
  ptc_frame_plan plan{};
  plan.batch = std::min({std::max(1, batch_frames), frames, (int)kMaxBatch});
  if (frames_auto) frames -= frames % plan.batch;  // whole batches only
  plan.frames = frames;
  plan.big_slots = (frames + plan.batch - 1) / plan.batch;  // slots (streams); each holds a batch
  plan.staged = frames > 1;
  plan.single_slots = (plan.staged && plan.batch > 1) ? kSingleSlots : 0;
  return plan;
}

// "denoise_albedo" (DESIGN section 5r): the planes the stage adds to a frame -- the first-hit albedo and the irradiance, a float4 per
// pixel each -- and the float4 elements of one.  Not part of ptc_frame_plan: they are allocated by the first call that runs the
// stage at a frame size (ptcore.cpp, albedo_planes), not by ptc_resize, and released with the frame.
constexpr int kDenoiseAlbedoPlanes = 2;
inline uint64_t denoise_albedo_floats4(uint32_t width, uint32_t height) { return (uint64_t)width * height; }

// "denoise_variance" (DESIGN section 5s): the planes the mode adds to a frame -- the two scalar variance planes that ping-pong beside
// den_a and den_b (the estimate writes the first; ptc_denoise_variance's prefiltered plane borrows the second), a float per pixel each
// -- and the floats of one.  Allocated and released as the albedo planes are (ptcore.cpp, variance_planes).
constexpr int kDenoiseVariancePlanes = 2;
inline uint64_t denoise_variance_floats(uint32_t width, uint32_t height) { return (uint64_t)width * height; }

}  // namespace pt
