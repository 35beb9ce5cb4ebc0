// Shared between fa_kvq.hip (quantised KV cache: decode, append, dequantise) and capi_kvq.hip.
#pragma once
#include "fa_decode.h"

namespace mt {

// the two storage formats: a chunk of 8 elements as loaded (Raw) and widened to fp32 (the fp8 row scale
// is applied by the caller)
struct KvBf16 : Chunk<bf16> {
  static constexpr int kBytes = 2;
  static constexpr bool kScaled = false;
  // the zero of a masked key's select (fa_decode_kernel.h, "masked"): a fresh value here, the named
  // one for fp8 -- per format, the spelling under which every instantiation keeps the registers,
  // AGPRs and waves per SIMD recorded in profiles/decode_kernels_resources.txt
  static __device__ __forceinline__ Raw masked(const Raw&) { return zero(); }
};

struct KvFp8 {
  using Raw = uint2;
  static constexpr int kBytes = 1;
  static constexpr bool kScaled = true;
  static __device__ __forceinline__ Raw zero() { return make_uint2(0u, 0u); }
  static __device__ __forceinline__ const Raw& masked(const Raw& z) { return z; }
  static __device__ __forceinline__ void unpack(const Raw& u, float* f) {
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)u.x, false);
    const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)u.x, true);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)u.y, false);
    const f32x2 e = __builtin_amdgcn_cvt_pk_f32_fp8((int)u.y, true);
    f[0] = a.x; f[1] = a.y; f[2] = b.x; f[3] = b.y;
    f[4] = c.x; f[5] = c.y; f[6] = e.x; f[7] = e.y;
  }
};

constexpr int kKvqEpc = 8;  // elements per chunk, both formats

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
