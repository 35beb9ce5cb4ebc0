// Quantised KV cache: decode attention on bf16 / fp8 (OCP e4m3) caches with fp32 queries, fp32
// arithmetic and fp32 O (mt_flash_attn_decode_kvq), the quantising append
// (mt_kv_cache_append_quant) and the dequantising copy (mt_kv_cache_dequant).
//
// Storage: K and V rows of d elements, bf16 (2 B) or e4m3 (1 B: bias 7, max 448, no inf, NaN =
// 0x7F / 0xFF, what v_cvt_pk_f32_fp8 reads on gfx950). An fp8 row has one fp32 scale s (dense
// [B, Hkv, Nmax] arrays): the row's values are s * e4m3(code). bf16 rows have no scale.
//
// Decode is the shared kernel (fa_decode_kernel.h) on KvqSrc below: the plan, arithmetic and combine
// pass of a plain cache. A key row is C = d / 8 chunks of 8 elements for both formats (a 16-B load
// of bf16, an 8-B load of fp8; a 16-B fp8 chunk would put 16 fp32 Q and accumulator elements per
// query row in every lane, 256 VGPRs at NQ = 8), so LPK and the plan are those of a bf16 cache. A
// lane's chunk is dequantised to fp32 in registers. The fp8 scale of key j multiplies the logit after
// the group sum (dot * k_scale[j] * scale_log2) and p before the PV fma; a key at or past the span's
// end re-reads the scale of the last visible row, as it does the row, and both are replaced by selects.
#include "fa_kvq.h"
#include "fa_decode_kernel.h"
#include <algorithm>

namespace mt {

// A contiguous cache of bf16 or fp8 rows (strides in storage elements) under fp32 Q and O
template <typename KV> struct KvqSrc : KV {
  using Args = KvqDecodeArgs;
  using Raw = typename KV::Raw;
  using Q = float;
  static constexpr int EPC = kKvqEpc;
  static constexpr int kMaxLpk = 32;  // d <= 256: at most 32 chunks of 8
  static constexpr int waves_per_eu(int, int) { return 1; }
  static __host__ __device__ __forceinline__ const DecodeArgs& base(const Args& sa) { return sa.d; }
  struct QChunk {  // 8 fp32 elements
    float4 x, y;
    __device__ __forceinline__ QChunk() : x(make_float4(0.f, 0.f, 0.f, 0.f)), y(x) {}
    explicit __device__ __forceinline__ QChunk(const float* p) : x(*(const float4*)p), y(*(const float4*)(p + 4)) {}
    __device__ __forceinline__ void unpack(float* f) const {
      f[0] = x.x; f[1] = x.y; f[2] = x.z; f[3] = x.w;
      f[4] = y.x; f[5] = y.y; f[6] = y.z; f[7] = y.w;
    }
  };
  static __device__ __forceinline__ void store_o(const DecodeArgs& a, int64_t e, const float4& x) {
    *(float4*)((float*)a.o + e) = x;
  }

  const Args& sa;
  const char* kb; const char* vb;  // this (b, hkv)'s rows, byte addresses
  int64_t srow;                    // and row scales
  int cc;                          // a lane past the row's chunks re-reads chunk 0 (values dropped)
  __device__ __forceinline__ KvqSrc(const Args& sa_, int b, int hkv, int c, int C)
      : sa(sa_),
        kb((const char*)sa_.d.k + ((int64_t)b * sa_.d.ks[0] + (int64_t)hkv * sa_.d.ks[1]) * KV::kBytes),
        vb((const char*)sa_.d.v + ((int64_t)b * sa_.d.vs[0] + (int64_t)hkv * sa_.d.vs[1]) * KV::kBytes),
        srow(((int64_t)b * sa_.d.Hkv + hkv) * sa_.d.Nk),
        cc(c < C ? c : 0) {}
  template <int GROUPS>
  __device__ __forceinline__ void issue(int t0, int g, int kend, Raw* ku, Raw* vu, float* ks, float* vs) const {
    const DecodeArgs& a = sa.d;
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {
      const int kk = min(t0 + u * GROUPS + g, kend - 1);
      ku[u] = *(const Raw*)(kb + ((int64_t)kk * a.ks[2] + cc * EPC) * KV::kBytes);
      if constexpr (KV::kScaled) ks[u] = sa.kscale[srow + kk];
    }
#pragma unroll
    for (int u = 0; u < kDecUnroll; ++u) {
      const int kk = min(t0 + u * GROUPS + g, kend - 1);
      vu[u] = *(const Raw*)(vb + ((int64_t)kk * a.vs[2] + cc * EPC) * KV::kBytes);
      if constexpr (KV::kScaled) vs[u] = sa.vscale[srow + kk];
    }
  }
};

// Sizes are validated by the caller (capi_kvq.hip); the plan is decode_plan's for 2-byte elements
// (8-element chunks) whatever the format.
hipError_t launch_decode_kvq(const KvqDecodeArgs& a, bool fp8, int64_t B, hipStream_t st) {
  const int lpk = decode_lpk(a.d.d, 2);
  return fp8 ? launch_decode_src<KvqSrc<KvFp8>>(a, lpk, B, st) : launch_decode_src<KvqSrc<KvBf16>>(a, lpk, B, st);
}

// ---- quantising append ----------------------------------------------------------------------
// lpr lanes (a power of two <= 32, >= d / 8) per new row, a lane owning 8 elements of the K row
// and of the V row; the fp8 row maximum is reduced with shuffles inside the lane group. Rows
// outside [0, Nmax) are dropped; nothing but the landed rows and their scale slots is written.
template <bool FP8>
__global__ __launch_bounds__(256) void kvq_append(const KvqAppendArgs a) {
  const int lpr = a.lpr, c = threadIdx.x % lpr;
  const int64_t r_ = (int64_t)blockIdx.x * (256 / lpr) + threadIdx.x / lpr;
  const bool in_rows = r_ < a.rows;
  int64_t r = in_rows ? r_ : a.rows - 1;  // every lane stays for the shuffles; stores are predicated
  const int i = (int)(r % a.Nq);
  r /= a.Nq;
  const int h = (int)(r % a.Hkv);
  const int64_t b = r / a.Hkv;
  const int64_t row = (int64_t)a.pos[b] + i;
  const bool mine = c * kKvqEpc < a.d;
  const bool land = in_rows && mine && row >= 0 && row < a.Nmax;
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    const float* src = which ? a.vn : a.kn;
    const int64_t* ss = which ? a.vns : a.kns;
    const int64_t* cs = which ? a.vcs : a.kcs;
    char* cache = which ? a.vc : a.kc;
    float* scale = which ? a.vscale : a.kscale;
    float x[kKvqEpc];
#pragma unroll
    for (int e = 0; e < kKvqEpc; ++e) x[e] = 0.f;
    if (mine) {
      const float* p = src + b * ss[0] + h * ss[1] + i * ss[2] + c * kKvqEpc;
      if (a.vec_in) {
        const float4 u = *(const float4*)p, w = *(const float4*)(p + 4);
        x[0] = u.x; x[1] = u.y; x[2] = u.z; x[3] = u.w; x[4] = w.x; x[5] = w.y; x[6] = w.z; x[7] = w.w;
      } else {
#pragma unroll
        for (int e = 0; e < kKvqEpc; ++e) x[e] = p[e];
      }
    }
    if constexpr (FP8) {
      float am = 0.f;
      int bad = 0;
#pragma unroll
      for (int e = 0; e < kKvqEpc; ++e) {
        const float ax = fabsf(x[e]);
        am = fmaxf(am, ax);
        bad |= !(ax <= 3.402823466e38f);  // inf or NaN
      }
      for (int off = lpr >> 1; off > 0; off >>= 1) {
        am = fmaxf(am, __shfl_xor(am, off));
        bad |= __shfl_xor(bad, off);
      }
      float s = am > 0.f ? am / 448.f : 1.f;
      unsigned w0 = 0x7F7F7F7Fu, w1 = 0x7F7F7F7Fu;  // a non-finite row: NaN codes, NaN scale
      if (bad) {
        s = __builtin_nanf("");
      } else {
        float y[kKvqEpc];
#pragma unroll
        for (int e = 0; e < kKvqEpc; ++e) y[e] = fminf(fmaxf(x[e] / s, -448.f), 448.f);
        int t = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
        w0 = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], t, true);
        t = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], 0, false);
        w1 = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], t, true);
      }
      if (land) {
        *(uint2*)(cache + b * cs[0] + h * cs[1] + row * cs[2] + c * kKvqEpc) = make_uint2(w0, w1);
        if (c == 0) scale[(b * a.Hkv + h) * a.Nmax + row] = s;
      }
    } else {
      if (land) {
        typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
        const bf16x8 v = {(bf16)x[0], (bf16)x[1], (bf16)x[2], (bf16)x[3],
                          (bf16)x[4], (bf16)x[5], (bf16)x[6], (bf16)x[7]};  // round to nearest even
        *(bf16x8*)(cache + (b * cs[0] + h * cs[1] + row * cs[2] + c * kKvqEpc) * 2) = v;
      }
    }
  }
}

hipError_t launch_kvq_append(const KvqAppendArgs& a, bool fp8, hipStream_t st) {
  const int64_t rpb = 256 / a.lpr, blocks = (a.rows + rpb - 1) / rpb;
  if (fp8) kvq_append<true><<<dim3((unsigned)blocks), 256, 0, st>>>(a);
  else kvq_append<false><<<dim3((unsigned)blocks), 256, 0, st>>>(a);
  return hipGetLastError();
}

// ---- dequantising copy ----------------------------------------------------------------------
// one 8-element chunk of a K row and of the matching V row per thread; rows at or past
// clamp(kv_len[b], 0, Nk) are neither read nor written
template <typename KV>
__global__ __launch_bounds__(256) void kvq_dequant(const KvqDequantArgs a) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.total) return;
  const int c = (int)(t % a.chunks);
  int64_t r = t / a.chunks;
  const int j = (int)(r % a.Nk);
  r /= a.Nk;
  const int h = (int)(r % a.Hkv);
  const int64_t b = r / a.Hkv;
  int n = a.Nk;
  if (a.kv_len) n = min(max(a.kv_len[b], 0), a.Nk);
  if (j >= n) return;
  const int64_t srow = (b * a.Hkv + h) * a.Nk + j;
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    const char* cache = which ? a.vc : a.kc;
    const int64_t* cs = which ? a.vcs : a.kcs;
    const int64_t* os = which ? a.vos : a.kos;
    float* out = which ? a.vo : a.ko;
    const typename KV::Raw raw =
        *(const typename KV::Raw*)(cache + (b * cs[0] + h * cs[1] + (int64_t)j * cs[2] + c * kKvqEpc) * KV::kBytes);
    float f[kKvqEpc];
    KV::unpack(raw, f);
    if constexpr (KV::kScaled) {
      const float s = (which ? a.vscale : a.kscale)[srow];
#pragma unroll
      for (int e = 0; e < kKvqEpc; ++e) f[e] *= s;
    }
    float* p = out + b * os[0] + h * os[1] + (int64_t)j * os[2] + c * kKvqEpc;
    *(float4*)p = make_float4(f[0], f[1], f[2], f[3]);
    *(float4*)(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
  }
}

hipError_t launch_kvq_dequant(const KvqDequantArgs& a, bool fp8, hipStream_t st) {
  const int64_t blocks = (a.total + 255) / 256;
  if (fp8) kvq_dequant<KvFp8><<<dim3((unsigned)blocks), 256, 0, st>>>(a);
  else kvq_dequant<KvBf16><<<dim3((unsigned)blocks), 256, 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace mt
