// Pass 1 of KV-cache decode attention, the one kernel body behind mt_flash_attn_decode[_gqa]
// (fa_decode.hip), mt_flash_attn_decode_kvq (fa_kvq.hip) and mt_flash_attn_decode_paged
// (fa_paged.hip), and the dispatch over its instantiations.
//
// A decode step has 1-8 query rows per (batch, head) against a cache of up to Nk keys: one
// read of K and V, O(Nk d) bytes and as many FMAs, memory-bound. Nothing is shared between
// waves, so K and V rows go straight from global memory to VGPRs with 16-B loads (no LDS
// staging) and the products run on the VALU in fp32.
//
// Pass 1, fa_decode_partial: grid (B*Hkv*slices, splits), 4 waves per workgroup (Hkv = H, one
// slice: grid (B*H, splits); grouped queries below). A key row is C = d *
// esize / 16 chunks of 16 B; LPK = the power of two >= C (at least 4) lanes share one key, a
// lane owning one chunk, so one wave-wide load covers 64 / LPK keys and a wave takes kUnroll
// such loads of K and of V per step (tile_keys = kUnroll * 64 / LPK keys; with NQ <= 4 query
// rows in registers the next tile's loads are issued before this tile's arithmetic). The waves of a
// workgroup take the tiles of its span round-robin. Each lane group keeps its own online
// softmax (m, l, O chunk) per query over the keys it saw; the groups of a wave are merged with
// lane shuffles, the four waves through LDS, and the workgroup writes (m, l, unnormalised O)
// of its span to the workspace -- or, with one split, the final O, m, l.
//
// Masking: with n = clamp(kv_len[b], 0, Nk) visible keys, query i (position n - Nq + i) sees
// the keys j < n - Nq + 1 + i (causal, bottom-right aligned) or j < n. No key >= n is ever
// loaded (a lane past the end re-reads the last key of the span and its values are replaced by
// zero, its logit by -inf, with selects), so whatever the cache tail holds contributes exactly 0.
//
// Pass 2, fa_decode_combine (fa_decode.hip): one 64-thread workgroup per (b, h, query) merges
// the splits in index order (rescale to the largest m, sum l and O, normalise): a fixed order,
// bit-reproducible.
//
// Grouped queries (Hkv < H, G = H / Hkv): query head h reads kv head h / G. The up to 8 register
// rows of a workgroup are independent of each other, so they hold gs = min(G, 8 / Nq) heads of
// one group, Nq queries each: row r is head hkv*G + slice*gs + r / Nq, query r % Nq, and a
// group takes slices = ceil(G / gs) workgroups per split, each reading the span's K/V once. A
// row whose head is past the group (a ragged last slice) is a row past Nq: limit 0, no load, no
// store. Q, O, m, l and the workspace stay addressed by query head; K and V by hkv.
//
// The plan is a host function of (dtype, B, H, Hkv, Nq, Nk, d) only (decode_plan; the split
// count and span of B, H, Nk, d; the packing of Hkv and Nq), never of kv_len: a captured
// launch replays as the cache fills.
//
// Where the K / V rows live and what they are made of is the kernel's source, Src: a small
// struct per cache kind (PlainSrc<T> in fa_decode.hip, KvqSrc<KV> in fa_kvq.hip, PagedSrc<T>
// in fa_paged.hip; a paged and quantised cache would be a fourth). It gives
//   Args, base(args)        the kernel's argument struct and the DecodeArgs in it
//   waves_per_eu(LPK, NQ)   the occupancy request of an instantiation (1: none)
//   kMaxLpk                 the largest LPK its rows need
//   EPC, Q                  elements per chunk, the element type of Q
//   QChunk                  a lane's Q chunk: zeros, or loaded from an address; unpack() widens it
//   Raw, zero, unpack       a K / V chunk as loaded, and widened to fp32
//   masked(z)               the zero chunk z as the select over a masked key takes it: z itself (an
//                           lvalue) or a fresh value. One select either way, but the two spellings
//                           reach the register allocator in different shapes (seen: up to 10 VGPRs
//                           and a wave per SIMD apart), and every format keeps the one under which
//                           its instantiations have the figures of
//                           profiles/decode_kernels_resources.txt; so the select stays spelled out
//                           in the kernel body and cannot move into a helper
//   kScaled                 rows carry an fp32 scale: on the logit after the group sum, on p
//   Src(args, b, hkv, c, C), issue<GROUPS>   the loads of one tile (and of its row scales)
//   store_o                 4 elements of a final O row
// Everything else -- grid decode, kv_len clamp, row limits, masking, online softmax, look-ahead
// loop, merges, epilogue -- is below, once: the same arithmetic in the same order for every
// source, so the same bits for the same rows however they are stored.
#pragma once
#include "fa_decode.h"

namespace mt {

// the parts of a source that an fp32 / bf16 cache of 16-B chunks has wherever its rows live
template <typename T> struct RowFormat : Chunk<T> {
  using Q = T;
  static constexpr int EPC = Chunk<T>::N;
  static constexpr bool kScaled = false;
  static constexpr int kMaxLpk = sizeof(T) == 4 ? 64 : 32;  // d <= 256: 64 fp32 chunks, 32 bf16
  static __device__ __forceinline__ const uint4& masked(const uint4& z) { return z; }
  struct QChunk {
    uint4 u;
    __device__ __forceinline__ QChunk() : u(make_uint4(0u, 0u, 0u, 0u)) {}
    explicit __device__ __forceinline__ QChunk(const T* p) : u(*(const uint4*)p) {}
    __device__ __forceinline__ void unpack(float* f) const { Chunk<T>::unpack(u, f); }
  };
  static __device__ __forceinline__ void store_o(const DecodeArgs& a, int64_t e, const float4& x) {
    store_o4(a.o, a.o_f32, e, x);
  }
};

template <typename Src, int LPK, int NQ>
__global__ __launch_bounds__(kDecWaves * 64)
__attribute__((amdgpu_waves_per_eu(Src::waves_per_eu(LPK, NQ))))
void fa_decode_partial(const typename Src::Args sa) {
  using Raw = typename Src::Raw;
  constexpr int EPC = Src::EPC;          // elements per chunk
  constexpr int GROUPS = 64 / LPK;       // keys per wave-wide load
  constexpr int TILE = kDecUnroll * GROUPS;
  constexpr int DP = LPK * EPC;          // padded head dim of the LDS image
  __shared__ float s_o[kDecWaves][NQ][DP];
  __shared__ float s_ml[kDecWaves][NQ][2];
  const DecodeArgs& a = Src::base(sa);

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
    // visible-key limit per query (no key at or past it is admitted)
    int lim[NQ];
    float qf[NQ][EPC];
    int hh = 0, qi = 0;  // register row i is head h0 + hh, query qi
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const bool row = NQ == 1 || hh < nh;  // nh >= 1
      lim[i] = row ? min(a.causal ? n - a.Nq + 1 + qi : n, kend) : 0;
      typename Src::QChunk u;
      if (row && c < C)
        u = typename Src::QChunk((const typename Src::Q*)a.q + (int64_t)b * a.qs[0] + (int64_t)(h0 + hh) * a.qs[1] +
                                 (int64_t)qi * a.qs[2] + c * EPC);
      u.unpack(qf[i]);
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
    const Src src(sa, b, hkv, c, C);

    // the loads of one tile: K then V chunks of kDecUnroll x GROUPS keys (and their row scales).
    // Keys at or past kend re-read row kend - 1 (in [k0, n): a visible, initialised row); their
    // values are dropped below
    auto issue = [&](int t0, Raw* ku, Raw* vu, float* ks, float* vs) {
      src.template issue<GROUPS>(t0, g, kend, ku, vu, ks, vs);
    };
    // with registers to spare (NQ <= 4) the next tile's loads are issued before this tile's
    // arithmetic, so a wave always has a tile in flight
    constexpr bool kAhead = NQ <= 4;
    // one tile's arithmetic on the rows in ku / vu
    auto consume = [&](int t0, const Raw* ku, const Raw* vu, const float* ks, const float* vs) {
      int key[kDecUnroll];
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) key[u] = t0 + u * GROUPS + g;
      float s[NQ][kDecUnroll];
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) {
        const bool live = key[u] < kend && c < C;
        const Raw z = Src::zero();
        const Raw kx = live ? ku[u] : Src::masked(z);  // see "masked" above
        float kf[EPC];
        Src::unpack(kx, kf);
        float sc = a.scale_log2;
        if constexpr (Src::kScaled) sc = (key[u] < kend ? ks[u] : 0.f) * a.scale_log2;
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
        const Raw z = Src::zero();
        const Raw vx = live ? vu[u] : Src::masked(z);
        float vf[EPC];
        Src::unpack(vx, vf);
        float vsc = 1.f;
        if constexpr (Src::kScaled) vsc = key[u] < kend ? vs[u] : 0.f;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
          const float pv = Src::kScaled ? p[i][u] * vsc : p[i][u];
#pragma unroll
          for (int e = 0; e < EPC; ++e) acc[i][e] = fmaf(pv, vf[e], acc[i][e]);
        }
      }
    };
    constexpr int STEP = kDecWaves * TILE;
    Raw ka[kDecUnroll], va[kDecUnroll];
    float ksa[kDecUnroll], vsa[kDecUnroll];  // row scales: unused, so gone, unless Src::kScaled
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
      Src::store_o(a, (int64_t)b * a.os[0] + (int64_t)(h0 + hh) * a.os[1] + (int64_t)qi * a.os[2] + 4 * e4, o);
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

// ---- dispatch -------------------------------------------------------------------------------
template <typename Src, int LPK>
static hipError_t launch_partial_nq(const typename Src::Args& sa, dim3 grid, hipStream_t st) {
  const DecodeArgs& a = Src::base(sa);
  const int rows = a.gs * a.Nq;  // register rows of a workgroup
  if (rows == 1) fa_decode_partial<Src, LPK, 1><<<grid, kDecWaves * 64, 0, st>>>(sa);
  else if (rows <= 4) fa_decode_partial<Src, LPK, 4><<<grid, kDecWaves * 64, 0, st>>>(sa);
  else fa_decode_partial<Src, LPK, 8><<<grid, kDecWaves * 64, 0, st>>>(sa);
  return hipGetLastError();
}

// Pass 1 at lpk lanes per key, then the combine pass if the plan has more than one split. Sizes
// are validated by the caller (capi_decode.hip, capi_kvq.hip, capi_paged.hip): 1 <= Nq <= 8,
// d <= 256, whole chunks, Hkv divides H, gs / slices / rows / nsplit / span from decode_plan.
template <typename Src>
static hipError_t launch_decode_src(const typename Src::Args& sa, int lpk, int64_t B, hipStream_t st) {
  const DecodeArgs& a = Src::base(sa);
  const dim3 grid((unsigned)(B * a.Hkv * a.slices), (unsigned)a.nsplit);
  hipError_t e = hipErrorInvalidValue;
  switch (lpk) {
    case 4: e = launch_partial_nq<Src, 4>(sa, grid, st); break;
    case 8: e = launch_partial_nq<Src, 8>(sa, grid, st); break;
    case 16: e = launch_partial_nq<Src, 16>(sa, grid, st); break;
    case 32: e = launch_partial_nq<Src, 32>(sa, grid, st); break;
    case 64:  // fp32 d in (128, 256] only: a row of 8-element chunks has at most 32 of them
      if constexpr (Src::kMaxLpk >= 64) e = launch_partial_nq<Src, 64>(sa, grid, st);
      break;
  }
  if (e != hipSuccess || a.nsplit == 1) return e;
  return launch_decode_combine(a, B, st);
}

}  // namespace mt
