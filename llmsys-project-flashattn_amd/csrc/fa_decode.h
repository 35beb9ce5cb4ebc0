// Shared between fa_decode.hip, fa_kvq.hip and fa_paged.hip (the plain, quantised and paged caches:
// each instantiates the one decode kernel of fa_decode_kernel.h on its source and owns its append
// and copy kernels) and capi_decode.hip / capi_kvq.hip / capi_paged.hip (the C ABI).
#pragma once
#include "fa_common.h"

namespace mt {

struct DecodeArgs {
  const void* q; const void* k; const void* v; void* o;
  float* m; float* l;          // [B*H*Nq] or NULL
  float* ws;                   // nsplit > 1: [B*H*Nq*nsplit][d] O, then [B*H*Nq*nsplit][2] (m in log2 units, l)
  const int* kv_len;           // [B] or NULL
  int64_t qs[3], ks[3], vs[3], os[3];
  int H, Nq, Nk, d, nsplit, span, causal, o_f32;
  int Hkv, gs, slices;         // kv heads (H % Hkv == 0); query heads and workgroups per group (decode_plan)
  int64_t rows;                // B * H * Nq
  float scale_log2;            // log2(e) / sqrt(d)
};

struct DecodePlan { int lpk, tile, span, nsplit, gs, slices; };

struct AppendArgs {
  const char* kn; const char* vn; char* kc; char* vc;
  const int* pos;
  int64_t kns[3], vns[3], kcs[3], vcs[3];  // element strides
  int64_t total;                           // B * H * Nq * chunks
  int H, Nq, Nmax, chunks, esize;
};

int decode_lpk(int64_t d, int esize);  // lanes per key: the power of two >= 16-B chunks per row, at least 4
DecodePlan decode_plan(int esize, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk, int64_t d);
hipError_t launch_decode(const DecodeArgs& a, bool bf16_in, int64_t B, hipStream_t st);
hipError_t launch_decode_combine(const DecodeArgs& a, int64_t B, hipStream_t st);  // pass 2 alone
hipError_t launch_kv_append(const AppendArgs& a, hipStream_t st);
int set_error(const char* fmt, ...);           // capi_flash.hip
int check_hip(hipError_t e, const char* where);
// argument checks of the decode C ABI (capi_decode.hip; capi_paged.hip applies them at Nk = W * P):
// 0, or the error status with the message set
int decode_sizes(int dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk, int64_t d);
void strides_or_dense(int64_t dst[3], const int64_t* src, int64_t H, int64_t N, int64_t d);
int aligned16(const char* what, const void* p, const int64_t s[3], int esize);
int64_t decode_ws_bytes(const DecodePlan& p, int64_t B, int64_t H, int64_t Nq, int64_t d);
// what the three decode entry points do alike once the sizes are valid: the workspace check (ws_query
// names the entry point's workspace query in the message) and the fields of `a` that are neither
// strides nor o_f32; 0, or the error status with the message set
int decode_args(DecodeArgs& a, const DecodePlan& p, const char* ws_query, int causal, const void* q, const void* k,
                const void* v, void* o, float* m, float* l, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk,
                int64_t d, const int* kv_len, void* workspace, int64_t workspace_bytes);

constexpr int kDecWaves = 4;    // waves per workgroup
constexpr int kDecUnroll = 4;   // key loads of K (and of V) in flight per wave and step

__device__ __forceinline__ float dpp_f(float x, const int ctrl_sel) {
  // DPP controls: 0xB1 quad_perm [1,0,3,2], 0x4E quad_perm [2,3,0,1], 0x141 row_half_mirror,
  // 0x140 row_mirror
  int v = __builtin_bit_cast(int, x), r;
  switch (ctrl_sel) {
    case 0: r = __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true); break;
    case 1: r = __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true); break;
    case 2: r = __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true); break;
    default: r = __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true); break;
  }
  return __builtin_bit_cast(float, r);
}

// the sum of v over the LPK lanes of a key group, in every lane of the group (after each step
// the value is uniform over the lanes already joined, so the mirrors pair the two halves)
template <int LPK> __device__ __forceinline__ float group_sum(float v) {
  v += dpp_f(v, 0);
  v += dpp_f(v, 1);
  if (LPK >= 8) v += dpp_f(v, 2);
  if (LPK >= 16) v += dpp_f(v, 3);
  if (LPK >= 32) v += __shfl_xor(v, 16);
  if (LPK >= 64) v += __shfl_xor(v, 32);
  return v;
}

__device__ __forceinline__ float exp2_fast(float x) { return __builtin_amdgcn_exp2f(x); }

// a 16-B chunk of a Q / K / V row, as loaded (Raw) and widened to fp32
struct Chunk16 {
  using Raw = uint4;
  static __device__ __forceinline__ Raw zero() { return make_uint4(0u, 0u, 0u, 0u); }
};
template <typename T> struct Chunk;
template <> struct Chunk<float> : Chunk16 {
  static constexpr int N = 4;
  static __device__ __forceinline__ void unpack(const uint4& u, float* f) {
    f[0] = __builtin_bit_cast(float, u.x); f[1] = __builtin_bit_cast(float, u.y);
    f[2] = __builtin_bit_cast(float, u.z); f[3] = __builtin_bit_cast(float, u.w);
  }
};
template <> struct Chunk<bf16> : Chunk16 {
  static constexpr int N = 8;
  static __device__ __forceinline__ void unpack(const uint4& u, float* f) {
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = __builtin_bit_cast(float, w[i] << 16);
      f[2 * i + 1] = __builtin_bit_cast(float, w[i] & 0xffff0000u);
    }
  }
};

// 4 consecutive O elements of one row: fp32 (16-B store) or bf16 (8-B store)
__device__ __forceinline__ void store_o4(void* o, int o_f32, int64_t e, const float4& x) {
  if (o_f32) {
    *(float4*)((float*)o + e) = x;
  } else {
    typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
    bf16x4 r = {(bf16)x.x, (bf16)x.y, (bf16)x.z, (bf16)x.w};
    *(bf16x4*)((bf16*)o + e) = r;
  }
}

}  // namespace mt
