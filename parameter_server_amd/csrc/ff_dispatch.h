// The FIXING_FLOAT launch layer's dispatch (ff_codec.hip): the runtime
// (value_type, num_bytes) of a launch as compile-time tags for a generic
// lambda that returns a status, and the rules that say which kernel
// instantiations exist.  Plain host C++.
#pragma once
#include <type_traits>
#include <utility>

#include "psf_internal.h"

namespace psf {

// f(float{}) / f(double{}); kErrArg for any other value type
template <typename F>
int with_value_type(int value_type, F&& f) {
  if (value_type == kFloat) return f(float{});
  if (value_type == kDouble) return f(double{});
  return kErrArg;
}
// f(std::integral_constant<int, nb>{}) for nb in [LO, HI]; kErrNbytes outside
template <int LO, int HI, typename F>
int with_nb(int nb, F&& f) {
  if constexpr (LO > HI) {
    return kErrNbytes;
  } else {
    if (nb == LO) return f(std::integral_constant<int, LO>{});
    return with_nb<LO + 1, HI>(nb, std::forward<F>(f));
  }
}
// both, f(value tag, nb tag); the value type is checked first
template <int LO, int HI, typename F>
int with_type_nb(int value_type, int nb, F&& f) {
  return with_value_type(value_type, [&](auto v) {
    return with_nb<LO, HI>(nb, [&](auto n) { return f(v, n); });
  });
}
// f(std::true_type{}) / f(std::false_type{})
template <typename F>
int with_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

// Which instantiations exist:
constexpr int kNbMax = 7;       // single-array encode and decode: nb 1..7
constexpr int kBatchNbMax = 3;  // every batched kernel: nb 1..3 (ff_batchable)
// codes in the stored snappy-stream layout (the kStored encode kernels)
constexpr bool ff_has_stored(int nb) { return nb <= 2; }
// the tile-walking vector decode; wider codes decode element by element
constexpr bool ff_has_vec_decode(int nb) { return nb <= 3; }
// ff_fused_batch and ff_dec_mm_batch take small batches only
constexpr bool ff_has_fused(int cap) { return cap == kFusedArrays; }

}  // namespace psf
