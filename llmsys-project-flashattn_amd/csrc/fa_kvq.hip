// Quantised KV cache: decode attention on bf16 / fp8 (OCP e4m3) caches with fp32 queries, fp32
// arithmetic and fp32 O (mt_flash_attn_decode_kvq), the quantising append
// (mt_kv_cache_append_quant) and the dequantising copy (mt_kv_cache_dequant).
//
// Storage: K and V rows of d elements, bf16 (2 B) or e4m3 (1 B: bias 7, max 448, no inf, NaN =
// 0x7F / 0xFF, what v_cvt_pk_f32_fp8 reads on gfx950). An fp8 row has one fp32 scale s (dense
// [B, Hkv, Nmax] arrays): the row's values are s * e4m3(code). bf16 rows have no scale.
//
// fa_decode_partial_kvq is fa_decode_partial (fa_decode.hip) with a cache element type of its own:
// the same grid, spans, row packing, masking by selects, online softmax, DPP group sums, wave and
// LDS merges, workspace layout and combine pass (fa_decode_combine, reused as it is). A key row is
// C = d / 8 chunks of 8 elements for both formats (a 16-B load of bf16, an 8-B load of fp8; a
// 16-B fp8 chunk would put 16 fp32 Q and accumulator elements per query row in every lane, 256
// VGPRs at NQ = 8), so LPK and the plan are those of a bf16 cache. A lane's chunk is dequantised
// to fp32 in registers. The fp8 scale of key j multiplies the logit after the group sum
// (dot * k_scale[j] * scale_log2) and p before the PV fma; a key at or past the span's end re-reads
// the scale of the last visible row, as it does the row, and both are replaced by selects.
#include "fa_kvq.h"
#include <algorithm>

namespace mt {

struct KvBf16 {
  using Raw = uint4;
  static constexpr int kBytes = 2;
  static constexpr bool kScaled = false;
  static __device__ __forceinline__ Raw zero() { return make_uint4(0u, 0u, 0u, 0u); }
  static __device__ __forceinline__ void unpack(const Raw& u, float* f) {
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = __builtin_bit_cast(float, w[i] << 16);
      f[2 * i + 1] = __builtin_bit_cast(float, w[i] & 0xffff0000u);
    }
  }
};

struct KvFp8 {
  using Raw = uint2;
  static constexpr int kBytes = 1;
  static constexpr bool kScaled = true;
  static __device__ __forceinline__ Raw zero() { return make_uint2(0u, 0u); }
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

template <typename KV, int LPK, int NQ>
__global__ __launch_bounds__(kDecWaves * 64) void fa_decode_partial_kvq(const KvqDecodeArgs ka_) {
  using Raw = typename KV::Raw;
  constexpr int EPC = kKvqEpc;
  constexpr int GROUPS = 64 / LPK;       // keys per wave-wide load
  constexpr int TILE = kDecUnroll * GROUPS;
  constexpr int DP = LPK * EPC;          // padded head dim of the LDS image
  __shared__ float s_o[kDecWaves][NQ][DP];
  __shared__ float s_ml[kDecWaves][NQ][2];
  const DecodeArgs& a = ka_.d;

  const int split = blockIdx.y;
  const int bk = blockIdx.x / a.slices, slice = blockIdx.x - bk * a.slices;
  const int b = bk / a.Hkv, hkv = bk - b * a.Hkv;
  const int G = a.H / a.Hkv;
  const int h0 = hkv * G + slice * a.gs;     // first query head of this workgroup
  const int nh = min(a.gs, G - slice * a.gs);  // its heads (fewer in a ragged last slice)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c = lane % LPK, g = lane / LPK;
  const int C = a.d / EPC;               // real chunks per row (<= LPK)
  const int d4 = a.d / 4;

  int n = a.Nk;
  if (a.kv_len) n = min(max(a.kv_len[b], 0), a.Nk);
  const int k0 = split * a.span;
  const int kend = min(k0 + a.span, n);
  const bool final_out = a.nsplit == 1;
  const int64_t row0 = ((int64_t)b * a.H + h0) * a.Nq;  // first (b, h, query) row

  if (k0 < kend) {  // workgroup-uniform
    int lim[NQ];
    float qf[NQ][EPC];
    int hh = 0, qi = 0;  // register row i is head h0 + hh, query qi
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const bool row = NQ == 1 || hh < nh;  // nh >= 1
      lim[i] = row ? min(a.causal ? n - a.Nq + 1 + qi : n, kend) : 0;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
      if (row && c < C) {
        const float* qp = (const float*)a.q + (int64_t)b * a.qs[0] + (int64_t)(h0 + hh) * a.qs[1] +
                          (int64_t)qi * a.qs[2] + c * EPC;
        x = *(const float4*)qp;
        y = *(const float4*)(qp + 4);
      }
      qf[i][0] = x.x; qf[i][1] = x.y; qf[i][2] = x.z; qf[i][3] = x.w;
      qf[i][4] = y.x; qf[i][5] = y.y; qf[i][6] = y.z; qf[i][7] = y.w;
      if (++qi == a.Nq) { qi = 0; ++hh; }
    }
    float m[NQ], l[NQ], acc[NQ][EPC];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      m[i] = -INFINITY;
      l[i] = 0.f;
#pragma unroll
      for (int e = 0; e < EPC; ++e) acc[i][e] = 0.f;
    }
    // byte addresses: the strides are in storage elements
    const char* kb = (const char*)a.k + ((int64_t)b * a.ks[0] + (int64_t)hkv * a.ks[1]) * KV::kBytes;
    const char* vb = (const char*)a.v + ((int64_t)b * a.vs[0] + (int64_t)hkv * a.vs[1]) * KV::kBytes;
    const int64_t srow = ((int64_t)b * a.Hkv + hkv) * a.Nk;  // this head's row scales
    const int cc = c < C ? c : 0;  // a lane past the row's chunks re-reads chunk 0 (values dropped)

    // the loads of one tile: K then V chunks of kDecUnroll x GROUPS keys and (fp8) their row scales.
    // Keys at or past kend re-read row kend - 1 (in [k0, n): a visible, initialised row) and its
    // scales; their values are dropped below
    auto issue = [&](int t0, Raw* ku, Raw* vu, float* ks, float* vs) {
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) {
        const int kk = min(t0 + u * GROUPS + g, kend - 1);
        ku[u] = *(const Raw*)(kb + ((int64_t)kk * a.ks[2] + cc * EPC) * KV::kBytes);
        if constexpr (KV::kScaled) ks[u] = ka_.kscale[srow + kk];
      }
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) {
        const int kk = min(t0 + u * GROUPS + g, kend - 1);
        vu[u] = *(const Raw*)(vb + ((int64_t)kk * a.vs[2] + cc * EPC) * KV::kBytes);
        if constexpr (KV::kScaled) vs[u] = ka_.vscale[srow + kk];
      }
    };
    constexpr bool kAhead = NQ <= 4;
    auto consume = [&](int t0, const Raw* ku, const Raw* vu, const float* ks, const float* vs) {
      int key[kDecUnroll];
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) key[u] = t0 + u * GROUPS + g;
      float s[NQ][kDecUnroll];
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) {
        const bool live = key[u] < kend && c < C;
        const Raw kx = live ? ku[u] : KV::zero();
        float kf[EPC];
        KV::unpack(kx, kf);
        float sc = a.scale_log2;
        if constexpr (KV::kScaled) sc = (key[u] < kend ? ks[u] : 0.f) * a.scale_log2;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
          float dot = 0.f;
#pragma unroll
          for (int e = 0; e < EPC; ++e) dot = fmaf(qf[i][e], kf[e], dot);
          dot = group_sum<LPK>(dot) * sc;
          s[i][u] = key[u] < lim[i] ? dot : -INFINITY;  // select: a masked key's data decides nothing
        }
      }
      float p[NQ][kDecUnroll];
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
        float mx = m[i];
#pragma unroll
        for (int u = 0; u < kDecUnroll; ++u) mx = fmaxf(mx, s[i][u]);
        const float ms = mx == -INFINITY ? 0.f : mx;  // no visible key yet: exp2(-inf - 0) = 0
        const float alpha = exp2_fast(m[i] - ms);
        m[i] = mx;
        float sum = 0.f;
#pragma unroll
        for (int u = 0; u < kDecUnroll; ++u) {
          p[i][u] = exp2_fast(s[i][u] - ms);
          sum += p[i][u];
        }
        l[i] = l[i] * alpha + sum;
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[i][e] *= alpha;
      }
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) {
        const bool live = key[u] < kend && c < C;
        const Raw vx = live ? vu[u] : KV::zero();
        float vf[EPC];
        KV::unpack(vx, vf);
        float vsc = 1.f;
        if constexpr (KV::kScaled) vsc = key[u] < kend ? vs[u] : 0.f;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
          const float pv = KV::kScaled ? p[i][u] * vsc : p[i][u];
#pragma unroll
          for (int e = 0; e < EPC; ++e) acc[i][e] = fmaf(pv, vf[e], acc[i][e]);
        }
      }
    };
    constexpr int STEP = kDecWaves * TILE;
    Raw ka[kDecUnroll], va[kDecUnroll];
    float ksa[kDecUnroll], vsa[kDecUnroll];
    if constexpr (kAhead) {
      // two register sets used in turn (no copies: a copy would wait for the tile just issued)
      Raw kb2[kDecUnroll], vb2[kDecUnroll];
      float ksb[kDecUnroll], vsb[kDecUnroll];
      int t0 = k0 + wave * TILE;
      if (t0 < kend) issue(t0, ka, va, ksa, vsa);
      while (t0 < kend) {
        issue(t0 + STEP, kb2, vb2, ksb, vsb);
        __builtin_amdgcn_sched_barrier(0);  // keep the loads ahead of the arithmetic
        consume(t0, ka, va, ksa, vsa);
        t0 += STEP;
        if (t0 >= kend) break;
        issue(t0 + STEP, ka, va, ksa, vsa);
        __builtin_amdgcn_sched_barrier(0);
        consume(t0, kb2, vb2, ksb, vsb);
        t0 += STEP;
      }
    } else {
      for (int t0 = k0 + wave * TILE; t0 < kend; t0 += STEP) {
        issue(t0, ka, va, ksa, vsa);
        consume(t0, ka, va, ksa, vsa);
      }
    }

    // merge the key groups of the wave (lane offsets LPK, 2 LPK, ...: the same chunk of other keys)
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      float mx = m[i];
#pragma unroll
      for (int off = LPK; off < 64; off *= 2) mx = fmaxf(mx, __shfl_xor(mx, off));
      const float ms = mx == -INFINITY ? 0.f : mx;
      const float w = exp2_fast(m[i] - ms);
      float ls = l[i] * w;
#pragma unroll
      for (int off = LPK; off < 64; off *= 2) ls += __shfl_xor(ls, off);
#pragma unroll
      for (int e = 0; e < EPC; ++e) {
        float x = acc[i][e] * w;
#pragma unroll
        for (int off = LPK; off < 64; off *= 2) x += __shfl_xor(x, off);
        acc[i][e] = x;
      }
      if (g == 0) {
#pragma unroll
        for (int e = 0; e < EPC; e += 4)
          *(float4*)&s_o[wave][i][c * EPC + e] = make_float4(acc[i][e], acc[i][e + 1], acc[i][e + 2], acc[i][e + 3]);
        if (c == 0) {
          s_ml[wave][i][0] = mx;
          s_ml[wave][i][1] = ls;
        }
      }
    }
    __syncthreads();
  }

  // merge the waves (fixed order) and write this split's result, 4 O elements per thread
  const bool empty = !(k0 < kend);
  for (int idx = tid; idx < nh * a.Nq * d4; idx += kDecWaves * 64) {
    const int i = idx / d4, e4 = idx - i * d4;  // register row i: head h0 + i / Nq, query i % Nq
    const int hh = NQ == 1 ? 0 : i / a.Nq, qi = i - hh * a.Nq;
    float mx = -INFINITY, ls = 0.f;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!empty) {
#pragma unroll
      for (int w = 0; w < kDecWaves; ++w) mx = fmaxf(mx, s_ml[w][i][0]);
      const float ms = mx == -INFINITY ? 0.f : mx;
#pragma unroll
      for (int w = 0; w < kDecWaves; ++w) {
        const float f = exp2_fast(s_ml[w][i][0] - ms);
        const float4 x = *(const float4*)&s_o[w][i][4 * e4];
        ls += s_ml[w][i][1] * f;
        o.x += x.x * f; o.y += x.y * f; o.z += x.z * f; o.w += x.w * f;
      }
    }
    if (final_out) {
      const float inv = ls > 0.f ? 1.f / ls : 0.f;
      o.x *= inv; o.y *= inv; o.z *= inv; o.w *= inv;
      *(float4*)((float*)a.o + (int64_t)b * a.os[0] + (int64_t)(h0 + hh) * a.os[1] + (int64_t)qi * a.os[2] + 4 * e4) = o;
      if (e4 == 0) {
        if (a.m) a.m[row0 + i] = mx * kLn2;
        if (a.l) a.l[row0 + i] = ls;
      }
    } else {
      const int64_t r = (row0 + i) * a.nsplit + split;
      *(float4*)(a.ws + r * a.d + 4 * e4) = o;
      if (e4 == 0) {
        float* ml = a.ws + a.rows * a.nsplit * a.d + 2 * r;
        ml[0] = mx;
        ml[1] = ls;
      }
    }
  }
}

template <typename KV, int LPK> static hipError_t launch_kvq_nq(const KvqDecodeArgs& a, dim3 grid, hipStream_t st) {
  const int rows = a.d.gs * a.d.Nq;  // register rows of a workgroup
  if (rows == 1) fa_decode_partial_kvq<KV, LPK, 1><<<grid, kDecWaves * 64, 0, st>>>(a);
  else if (rows <= 4) fa_decode_partial_kvq<KV, LPK, 4><<<grid, kDecWaves * 64, 0, st>>>(a);
  else fa_decode_partial_kvq<KV, LPK, 8><<<grid, kDecWaves * 64, 0, st>>>(a);
  return hipGetLastError();
}

template <typename KV> static hipError_t launch_kvq_partial(const KvqDecodeArgs& a, int lpk, dim3 grid, hipStream_t st) {
  switch (lpk) {
    case 4: return launch_kvq_nq<KV, 4>(a, grid, st);
    case 8: return launch_kvq_nq<KV, 8>(a, grid, st);
    case 16: return launch_kvq_nq<KV, 16>(a, grid, st);
    case 32: return launch_kvq_nq<KV, 32>(a, grid, st);  // d <= 256: at most 32 chunks of 8
  }
  return hipErrorInvalidValue;
}

// Sizes are validated by the caller (capi_kvq.hip); the plan is decode_plan's for 2-byte elements
// (8-element chunks) whatever the format.
hipError_t launch_decode_kvq(const KvqDecodeArgs& a, bool fp8, int64_t B, hipStream_t st) {
  const int lpk = decode_lpk(a.d.d, 2);
  const dim3 grid((unsigned)(B * a.d.Hkv * a.d.slices), (unsigned)a.d.nsplit);
  hipError_t e = fp8 ? launch_kvq_partial<KvFp8>(a, lpk, grid, st) : launch_kvq_partial<KvBf16>(a, lpk, grid, st);
  if (e != hipSuccess || a.d.nsplit == 1) return e;
  return launch_decode_combine(a.d, B, st);
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
