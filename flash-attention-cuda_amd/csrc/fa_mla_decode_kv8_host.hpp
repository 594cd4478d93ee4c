// Host side of the FP8 MLA decode entries of include/fa_mi355x_mla_kv8.h: the
// E4M3 cache's kernel family for fa_mla_decode_host.hpp's entry body and macro
// (the geometry, the plan, the workspace and the statuses are that header's).
#pragma once

#include "fa_mi355x_mla_kv8.h"
#include "fa_mla_decode_host.hpp"
#include "fa_mla_decode_kv8_kernel.hpp"

namespace fa {

struct MlaKernelsKv8 {
  static constexpr bool kKv8 = true;
  static constexpr int kRow = kMla8Row;
  static constexpr int kLds = kMla8LdsBytes;
  template <bool PAGED>
  using Params = std::conditional_t<PAGED, DecodePagedKv8Params, DecodeKv8Params>;
  template <class T, bool WIDE, bool PAGED>
  static constexpr auto kernel = fa_mla_decode_kv8_kernel<T, WIDE, PAGED, Params<PAGED>>;
};

}  // namespace fa
