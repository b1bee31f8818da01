// seg_common.h -- what segloss.hip and segblend.hip share: the register width that holds the C logits of a pixel.
#pragma once
#include <type_traits>

namespace dinox {

static int seg_cp(int C) { return C <= 4 ? 4 : C <= 8 ? 8 : C <= 16 ? 16 : C <= 32 ? 32 : 64; }

// f(std::integral_constant<int, CP>) for the register width that holds C classes
template <typename F>
static inline void seg_by_width(int C, F&& f) {
  switch (seg_cp(C)) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    default: f(std::integral_constant<int, 64>{}); break;
  }
}

}  // namespace dinox
