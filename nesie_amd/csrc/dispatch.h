// Runtime value -> template argument.  A launcher writes its kernel launch once, inside a generic
// lambda, and names the constant it was handed as a template argument:
//
//   with_bool(relu, [&](auto R) {
//     with_bool(nt, [&](auto N) { hipLaunchKernelGGL((kernel<R(), N()>), grid, block, 0, s, args...); });
//   });
//   const bool built = with_int<1, 2, 4, 8, 16>(lpr, [&](auto LPR) { ...kernel<LPR()>... });
//   NESIE_REQUIRE(built, W);
//
// No HIP in here: the host compiler alone builds this header (tests/test_dispatch_cpu.py).
#pragma once
#include <type_traits>

namespace nesie {

// f(std::true_type()) or f(std::false_type())
template <typename F>
inline void with_bool(bool v, F &&f) {
  if (v) f(std::true_type());
  else f(std::false_type());
}

// f(std::integral_constant<int, Vi>()) for the first Vi equal to v, once; true when one matched.
// An unlisted v calls nothing and gives false: there is no catch-all arm, so a launcher whose
// validation leaves only the listed values says so with NESIE_REQUIRE on the result, and one that
// folds the other values onto an arm folds v before the call.
template <int... Vs, typename F>
inline bool with_int(int v, F &&f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>()), true) : false) || ...);
}

}  // namespace nesie
