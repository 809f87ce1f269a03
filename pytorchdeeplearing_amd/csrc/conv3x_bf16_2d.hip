// conv3x tilings for bf16 tensors, 2D (see conv3x_impl.h; split per dtype and dimension for build time)
#include "conv3x_impl.h"

namespace seg {
namespace c3x {
template <> bool launch_2d<bf16>(int id, const Conv3xArgs& a, hipStream_t s) {
    return launch_nd<bf16, 2>(id, a, s, Rows{});
}
}  // namespace c3x
}  // namespace seg
