// pt_launch_flags.hpp -- what the launchers of pt_shade.hip and pt_env.hip share: grid sizes and the step from run-time booleans to a
// kernel instance.
#pragma once
#include <stdint.h>
#include <type_traits>

namespace pt {

static inline uint32_t div_up(uint32_t a, uint32_t b) { return (a + b - 1u) / b; }

// Run-time booleans to template arguments: with_flags(f, a, b, ...) calls f(A{}, B{}, ...) with std::true_type or std::false_type
// in each flag's place, so f (a generic lambda) names its kernel instance as k<decltype(a)::value, ...>.  Every combination is
// compiled: f leaves out, by `if constexpr`, the ones its caller never asks for (they would be kernels nobody launches).
template <class F>
static inline void with_flags(F&& f)
{
  f();
}
template <class F, class... Rest>
static inline void with_flags(F&& f, bool flag, Rest... rest)
{
  if (flag) with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}


}  // namespace pt
