// Shared between fa_kvq.hip (quantised KV cache: decode, append, dequantise) and capi_kvq.hip.
#pragma once
#include "fa_decode.h"

namespace mt {

// decode on a quantised cache: DecodeArgs as the plain kernel takes them (q / o / m / l fp32, k / v the
// cache storage, ks / vs in storage elements: bf16, or bytes for fp8) and the fp8 row scales
struct KvqDecodeArgs {
  DecodeArgs d;
  const float* kscale; const float* vscale;  // dense [B, Hkv, Nk] (fp8), NULL for bf16
};

struct KvqAppendArgs {
  const float* kn; const float* vn; char* kc; char* vc;
  float* kscale; float* vscale;            // dense [B, Hkv, Nmax] (fp8), NULL for bf16
  const int* pos;
  int64_t kns[3], vns[3], kcs[3], vcs[3];  // element strides (the caches': storage elements)
  int64_t rows;                            // B * Hkv * Nq
  int Hkv, Nq, Nmax, d, lpr, vec_in;       // lpr: lanes per row; vec_in: the new rows allow 16-B loads
};

struct KvqDequantArgs {
  const char* kc; const char* vc; const float* kscale; const float* vscale;
  float* ko; float* vo;
  const int* kv_len;
  int64_t kcs[3], vcs[3], kos[3], vos[3];
  int64_t total;                           // B * Hkv * Nk * chunks
  int Hkv, Nk, chunks;
};

hipError_t launch_decode_kvq(const KvqDecodeArgs& a, bool fp8, int64_t B, hipStream_t st);
hipError_t launch_kvq_append(const KvqAppendArgs& a, bool fp8, hipStream_t st);
hipError_t launch_kvq_dequant(const KvqDequantArgs& a, bool fp8, hipStream_t st);

}  // namespace mt
