// Shared between fa_extend.hip (kernel, plan, launcher) and capi_decode.hip (the C ABI).
#pragma once
#include "fa_common.h"

namespace mt {

struct ExtendArgs {
  const void* q; const void* k; const void* v; void* o;
  float* m; float* l;          // [B*H*Nq] or NULL
  const int* kv_len;           // [B] keys held after the append, or NULL (Nk)
  const int* q_len;            // [B] real new queries, or NULL (Nq)
  int64_t qs[3], ks[3], vs[3], os[3];
  int H, Hkv, Nq, Nk, d, causal, o_f32;
  int nqb;                     // query blocks per (b, h)
  float scale_log2;            // log2(e) / sqrt(d)
};

// kernel: the instantiation's id (>= 0); bq: query rows per workgroup; bk: keys per inner tile
struct ExtendPlan { int kernel, bq, bk; };

ExtendPlan extend_plan(int esize, int64_t d);
hipError_t launch_extend(const ExtendArgs& a, bool bf16_in, int64_t B, hipStream_t st);

}  // namespace mt
