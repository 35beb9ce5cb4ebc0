// Shared between fa_paged.hip (paged KV cache: decode, append, gather) and capi_paged.hip.
#pragma once
#include "fa_decode.h"

namespace mt {

// decode on a paged cache: DecodeArgs as the plain kernel takes them, with k / v the page pools
// ([n_pages, Hkv, P, d] through ks / vs = (page, head, row) element strides) and Nk = W * P the
// logical capacity; logical key j of row b is row j % P of page table[b * W + j / P]
struct PagedDecodeArgs {
  DecodeArgs d;
  const int* table;            // device int32 [B, W]
  int W, lgP, n_pages;         // table width, log2 of the page size, pages in the pool
};

struct PagedAppendArgs {
  const char* kn; const char* vn; char* kp; char* vp;
  const int* table; const int* pos; const int* count;  // count NULL: Nq rows per batch row
  int64_t kns[3], vns[3], kps[3], vps[3];  // element strides (the pools': page, head, row)
  int64_t total;                           // B * Hkv * Nq * chunks
  int Hkv, Nq, W, lgP, n_pages, chunks, esize;
};

struct PagedGatherArgs {
  const char* kp; const char* vp; char* ko; char* vo;
  const int* table; const int* kv_len;
  int64_t kps[3], vps[3], kos[3], vos[3];  // element strides (the pools': page, head, row)
  int64_t total;                           // B * Hkv * Nk * chunks
  int Hkv, Nk, W, lgP, n_pages, chunks, esize;
};

hipError_t launch_decode_paged(const PagedDecodeArgs& a, bool bf16_in, int64_t B, hipStream_t st);
hipError_t launch_append_paged(const PagedAppendArgs& a, hipStream_t st);
hipError_t launch_gather_paged(const PagedGatherArgs& a, hipStream_t st);

}  // namespace mt
