// silu(u) = u / (1 + exp(-u)): the one definition behind mt_swiglu_fw / mt_swiglu_bw
// (rmsnorm_swiglu.hip) and the gated epilogue of mt_linear_rows_ex (linear_rows.hip), so the fused
// step and the unfused kernels round alike. Contraction off, as gelu_tanh is.
#pragma once
#include <hip/hip_runtime.h>

namespace mt {
__device__ __forceinline__ float silu(float u) {
#pragma clang fp contract(off)
  return u / (1.f + expf(-u));
}
}  // namespace mt
