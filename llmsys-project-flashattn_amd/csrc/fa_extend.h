// Shared between fa_extend.hip (kernel, plan, launchers) and capi_decode.hip / capi_paged.hip /
// capi_kvq.hip (the C ABI of the extend step on a plain, a paged and a quantised cache).
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

// extend on a paged cache: ExtendArgs with k / v the page pools ([n_pages, Hkv, P, d] through ks / vs =
// (page, head, row) element strides) and Nk = W * P; logical key j of row b is row j % P of page
// table[b * W + j / P]
struct PagedExtendArgs {
  ExtendArgs e;
  const int* table;            // device int32 [B, W]
  int W, lgP, n_pages;         // table width, log2 of the page size, pages in the pool
};

// extend on a quantised cache: ExtendArgs with q / o fp32, k / v the cache storage (ks / vs in storage
// elements: bf16, or bytes for fp8) and the fp8 row scales
struct KvqExtendArgs {
  ExtendArgs e;
  const float* kscale; const float* vscale;  // dense [B, Hkv, Nk] (fp8), NULL for bf16
};

// kernel: the instantiation's id (>= 0); bq: query rows per workgroup; bk: keys per inner tile
struct ExtendPlan { int kernel, bq, bk; };

ExtendPlan extend_plan(int esize, int64_t d);
hipError_t launch_extend(const ExtendArgs& a, bool bf16_in, int64_t B, hipStream_t st);
hipError_t launch_extend_paged(const PagedExtendArgs& a, bool bf16_in, int64_t B, hipStream_t st);
hipError_t launch_extend_kvq(const KvqExtendArgs& a, bool fp8, int64_t B, hipStream_t st);  // the fp32 plan

// argument checks of the extend C ABI (capi_decode.hip; capi_paged.hip applies them at Nk = W * P,
// capi_kvq.hip at MT_F32): 0, or the error status with the message set
int extend_sizes(int dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk, int64_t d);
// the fields of `a` that are neither pointers to K / V / O nor strides, for esize-byte Q rows
void extend_args(ExtendArgs& a, int esize, int causal, float* m, float* l, int64_t H, int64_t Hkv, int64_t Nq,
                 int64_t Nk, int64_t d, const int* kv_len, const int* q_len);

}  // namespace mt
