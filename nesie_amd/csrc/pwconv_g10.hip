// pw_fwd_kernel<8, 1, 8, 1, 1, all rows built>: the input gradient of a 128-channel convolution that is
// max-pooled directly (the MiniPointNet tail): all 128 operand rows come from the pooled gradient's
// entries, no dense dZ is read (nesie_pw_dgrad_bn_reduce_sparse, pwconv.hip)
#include "pwconv_fwd.h"
namespace nesie {
int pw_launch_sparse_8_1_8_1_1(const PwFwd &a, int grid, size_t lds, hipStream_t s) {
  return pw_launch_sparse<8, 1, 8, 1, 1, PW_STORE | PW_BNRED | PW_SPARSE128>(a, grid, lds, s);
}
}  // namespace nesie
