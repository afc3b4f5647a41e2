// pt_demodulate.hpp -- the denoiser's albedo factorisation (ptc_set_param "denoise_albedo", ptc_denoise_albedo): the
// effective albedo of a channel, the irradiance the A-Trous passes filter in the colour's place, and the colour the filtered
// irradiance gives back.  Host-callable; every float line is one IEEE binary32 operation (-ffp-contract=off); k_denoise_albedo and
// k_remodulate (pt_denoise_albedo.hip) and the host's check (ptc_check_demodulate) call it, tests/demodulate_ref.py restates it in numpy.
#pragma once

#include "pt_math.hpp"

namespace pt {
namespace demod {

// The floor of the effective albedo, a design constant: the pair demodulate / remodulate amplifies by at most 64 in between, stays an
// identity on a uniformly dark region, and is continuous in the albedo.
constexpr float kAlbedoFloor = 1.0f / 64.0f;

// step 1: the albedo above the floor, else the floor -- a NaN, a zero of either sign and a negative value take the floor
PT_HD float effective_albedo(const float albedo) { return albedo > kAlbedoFloor ? albedo : kAlbedoFloor; }

// is that channel on the floor (k_denoise_albedo's count)
PT_HD bool floored(const float albedo) { return !(albedo > kAlbedoFloor); }

// step 2: what the passes filter
PT_HD float demodulate(const float colour, const float effective) { return colour / effective; }

// step 3: the colour of a filtered irradiance
PT_HD float remodulate(const float filtered, const float effective) { return filtered * effective; }

}  // namespace demod
}  // namespace pt
