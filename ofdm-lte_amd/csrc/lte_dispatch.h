// Run-time value -> template argument.  A launcher names the values a kernel is
// instantiated for and receives the matching one as an integral_constant, whose
// call operator is a constant expression:
//
//   with_bps(g.bps, [&](auto Q) { hipLaunchKernelGGL((k_foo<R, Q()>), ...); })
//
// Calls nest; `if constexpr` on the constants prunes combinations that are not
// to be instantiated.  Host-only, no HIP: builds with any C++17 compiler.
#pragma once
#include <type_traits>
#include <utility>

template <int V>
using ic = std::integral_constant<int, V>;
template <bool V>
using bc = std::integral_constant<bool, V>;

// f(ic<V>{}) for the first V of Vs equal to v; false (nothing called) if none is
template <int... Vs, class F>
inline bool with_int(int v, F&& f) {
  return (... || (v == Vs ? ((void)f(ic<Vs>{}), true) : false));
}
// ... and f(ic<D>{}) if none is
template <int D, int... Vs, class F>
inline void with_int_or(int v, F&& f) {
  if (!with_int<Vs...>(v, f)) f(ic<D>{});
}

template <class F>
inline void with_bool(bool v, F&& f) {
  if (v) f(bc<true>{});
  else f(bc<false>{});
}
// bits per symbol: QPSK, 16-QAM, 64-QAM
template <class F>
inline bool with_bps(int bps, F&& f) {
  return with_int<2, 4, 6>(bps, std::forward<F>(f));
}
// FFT size: Ns at compile time, any other as ic<0> (the kernel reads g.N)
template <int... Ns, class F>
inline void with_n(int N, F&& f) {
  with_int_or<0, Ns...>(N, std::forward<F>(f));
}
