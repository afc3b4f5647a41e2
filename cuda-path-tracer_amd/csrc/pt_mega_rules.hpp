// pt_mega_rules.hpp -- the instance rule of the megakernel: which of its 26 kernels a frame launches, and the roulette argument it
// gets.  Shared by launch_megakernel (pt_kernels.hip) and the host's check (ptc_check_megakernel_instance,
// tests/test_mega_instance_cpu.py); pure, host only, the only place the rule lives.
#pragma once

#include <limits.h>
#include <stdio.h>

namespace pt {
namespace mega_rules {

// What ptc_trace knows about a frame (ptcore_trace.cpp, mega_frame):
//   direct    "direct_light" and a lamp table of weight > 0          env       an environment map is set
//   env_lit   "environment_light", env and a table of weight > 0     smooth    "smooth_normals" and vertex normals
//   textured  "textures", textures and texture coordinates           weigh     "mis" and (direct or env_lit)
//   lens      a lens radius > 0                                       plays     some bounce plays roulette (roulette_frame)
//   emitters  the scene has an emissive material                      bent      "normal_maps", textures, coordinates and a binding
// The rule is total: it assumes no implication between them (env_lit without env, weigh without a light).
struct Facts {
  bool direct, env, env_lit, smooth, textured, weigh, lens, plays, emitters;
  bool bent = false;
};

// The kernels by family, in the rule's order; the units that hold them (the megakernel's six code objects):
//   nmap pt_mega_nmap.hip; tex pt_mega_tex.hip; smooth pt_mega_smooth.hip; mis pt_mega_mis.hip; plain<.., false> pt_kernels.hip; the rest pt_mega_direct.hip
enum class Kernel { tex, smooth, mis, env_light, env, direct_lens, direct, lens, plain, nmap };
constexpr const char* kKernelNames[] = {"k_megakernel_tex",         "k_megakernel_smooth", "k_megakernel_mis",
                                        "k_megakernel_env_light",   "k_megakernel_env",    "k_megakernel_direct_lens",
                                        "k_megakernel_direct",      "k_megakernel_lens",   "k_megakernel",
                                        "k_megakernel_nmap"};

// a, b: the kernel's template arguments in its own order (`args` of them count)
struct Instance {
  Kernel kernel;
  int args;
  bool a, b;
};

// The roulette argument of every instance: the first bounce that plays, or kNoRoulette where none does.  Decided here once.  The
// launchers this rule replaced passed the raw parameter, 0 or INT_MAX for a frame that does not play, by launcher; where those
// differ the instance is compiled without kRoulette and never reads the argument, and an instance that reads it either plays or got
// INT_MAX before as well (the environment's instances and everything behind them compile roulette in and see it play at no bounce).
constexpr int kNoRoulette = INT_MAX;
inline int roulette_argument(bool plays, int roulette) { return plays ? roulette : kNoRoulette; }

// The rule: the first row that matches.
//   0 bent      k_megakernel_nmap<weigh, smooth>
//   1 textured  k_megakernel_tex<weigh, smooth>      5 env     k_megakernel_env<direct>
//   2 smooth    k_megakernel_smooth<weigh>           6 direct  k_megakernel_direct_lens<plays> under a lens, else k_megakernel_direct<plays>
//   3 weigh     k_megakernel_mis                     7 lens    k_megakernel_lens<emitters, plays>
//   4 env_lit   k_megakernel_env_light               8 else    k_megakernel<emitters, plays>
inline Instance instance(const Facts& f)
{
  if (f.bent) return {Kernel::nmap, 2, f.weigh, f.smooth};
  if (f.textured) return {Kernel::tex, 2, f.weigh, f.smooth};
  if (f.smooth) return {Kernel::smooth, 1, f.weigh, false};
  if (f.weigh) return {Kernel::mis, 0, false, false};
  if (f.env_lit) return {Kernel::env_light, 0, false, false};
  if (f.env) return {Kernel::env, 1, f.direct, false};
  if (f.direct) return {f.lens ? Kernel::direct_lens : Kernel::direct, 1, f.plays, false};
  return {f.lens ? Kernel::lens : Kernel::plain, 2, f.emitters, f.plays};
}

// the instance's name as a profile prints it, e.g. "k_megakernel_tex<true, false>"; false: `capacity` is too small
inline bool instance_name(const Instance& in, char* out, size_t capacity)
{
  const char* base = kKernelNames[(int)in.kernel];
  const char* a = in.a ? "true" : "false";
  const char* b = in.b ? "true" : "false";
  const int n = in.args == 2 ? snprintf(out, capacity, "%s<%s, %s>", base, a, b)
                : in.args == 1 ? snprintf(out, capacity, "%s<%s>", base, a)
                               : snprintf(out, capacity, "%s", base);
  return n >= 0 && (size_t)n < capacity;
}

}  // namespace mega_rules
}  // namespace pt
