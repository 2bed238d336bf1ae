// The arg-max merge of the RNN-T greedy searches and the wave reduction of a joint row's
// column-block partials, shared by rnnt_advance_kernel / rnnt_reduce_kernel (transducer.hip) and
// rnnt_stream_advance_kernel (transducer_stream.hip): one text, so the one-shot and the
// resumable search pick the same index from the same partials.
#pragma once
#include "kernels.h"

namespace wn {

// (value, index) maximum, the lower index on equal values.  A NaN counts as the largest value,
// as in torch.argmax (the first NaN of a row wins): a merge that never accepted one would leave
// the caller's start index in place, which need not be a column of the matrix.
__device__ __forceinline__ void argmax_merge(float& v, int& i, float ov, int oi) {
  const bool on = ov != ov, vn = v != v;
  const bool gt = ov > v || (on && !vn);
  const bool eq = ov == v || (on && vn);
  if (gt || (eq && oi < i)) { v = ov; i = oi; }
}

// one wave: (max, index) of a row's ncb column-block partials, the same pair in every lane.
// Starts from the row's first partial, so the index is always one that the joint kernel wrote:
// a column in [0, V), or -1 for an inert row.
__device__ __forceinline__ void rnnt_reduce_row(const float* __restrict__ part_max,
                                                const int* __restrict__ part_idx, int64_t base,
                                                int ncb, int lane, float& v, int& i) {
  v = part_max[base];
  i = part_idx[base];
  for (int cb = lane; cb < ncb; cb += 64) argmax_merge(v, i, part_max[base + cb], part_idx[base + cb]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    argmax_merge(v, i, ov, oi);
  }
}

}  // namespace wn
