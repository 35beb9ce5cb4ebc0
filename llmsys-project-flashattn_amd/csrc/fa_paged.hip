// Paged KV cache: decode attention on K / V rows that live in scattered pages
// (mt_flash_attn_decode_paged), the append through the block table (mt_kv_cache_append_paged) and
// the copy of a row's pages into a contiguous cache (mt_kv_cache_gather_paged).
//
// Storage, per layer and per K / V: a pool of n_pages pages of P rows (P a power of two >= 16),
// seen as [n_pages, Hkv, P, d] through element strides (page, head, row), unit-stride d. One
// block table, device int32 [B, W]: logical key j of batch row b is row j % P of page
// table[b][j / P]; the logical capacity is Nk = W * P.
//
// fa_decode_partial_paged is fa_decode_partial (fa_decode.hip) with another address for a key row:
// the same grid, plan (decode_plan at Nk = W * P), spans, row packing, masking by selects, online
// softmax, DPP group sums, wave and LDS merges, workspace layout and combine pass
// (fa_decode_combine, reused as it is), the same arithmetic in the same order, so the same bits as
// the plain kernel on a contiguous cache holding the same rows. A wave-wide load covers 64 / LPK
// <= 16 <= P consecutive keys starting at a multiple of that count, so it never straddles a page.
// With n = clamp(kv_len[b], 0, W * P), a key at or past the span's end re-reads key kend - 1
// through that key's own table entry: no table entry at index >= ceil(n / P) and no pool row of a
// key >= n is read. A table entry is brought into [0, n_pages) before it forms an address, so a
// table that breaks the contract reads a wrong page of the pool, never memory outside it.
#include "fa_paged.h"
#include <algorithm>

namespace mt {
// fp32, one row: the plain kernel asks for 5 waves per SIMD (96 VGPRs) at LPK <= 16. The page index
// and the two address products cost a few registers: LPK = 16 (d in (32, 64]) spills 12 B per lane at
// 96, so it is left to the allocator (4 waves per SIMD); LPK 4 and 8 fit and keep the request
template <typename T, int LPK, int NQ>
__global__ __launch_bounds__(kDecWaves * 64)
__attribute__((amdgpu_waves_per_eu(sizeof(T) == 4 && NQ == 1 && LPK <= 8 ? 5 : 1)))
void fa_decode_partial_paged(const PagedDecodeArgs pa_) {
  constexpr int EPC = Chunk<T>::N;      // elements per 16-B chunk
  constexpr int GROUPS = 64 / LPK;       // keys per wave-wide load
  constexpr int TILE = kDecUnroll * GROUPS;
  constexpr int DP = LPK * EPC;          // padded head dim of the LDS image
  __shared__ float s_o[kDecWaves][NQ][DP];
  __shared__ float s_ml[kDecWaves][NQ][2];
  const DecodeArgs& a = pa_.d;

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
      uint4 u = make_uint4(0u, 0u, 0u, 0u);
      if (row && c < C)
        u = *(const uint4*)((const T*)a.q + (int64_t)b * a.qs[0] + (int64_t)(h0 + hh) * a.qs[1] +
                            (int64_t)qi * a.qs[2] + c * EPC);
      Chunk<T>::unpack(u, qf[i]);
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
    const int cc = c < C ? c : 0;  // a lane past the row's chunks re-reads chunk 0 (values dropped)
    // this head's rows of page 0, at the lane's chunk; a page adds ks[0] / vs[0], a row ks[2] / vs[2]
    const T* kb = (const T*)a.k + (int64_t)hkv * a.ks[1] + cc * EPC;
    const T* vb = (const T*)a.v + (int64_t)hkv * a.vs[1] + cc * EPC;
    const int* tb = pa_.table + (int64_t)b * pa_.W;  // this batch row's pages
    const int lgP = pa_.lgP, pmask = (1 << lgP) - 1, pmax = pa_.n_pages - 1;

    // the 16-B loads of one tile: K then V rows of kDecUnroll x GROUPS keys, each through the table
    // entry of its key. Keys at or past kend re-read row kend - 1 (in [k0, n): a visible,
    // initialised row of an allocated page); their values are dropped below
    auto issue = [&](int t0, uint4* ku, uint4* vu) {
      int pg[kDecUnroll];
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) {
        const int kk = min(t0 + u * GROUPS + g, kend - 1);
        pg[u] = (int)min((unsigned)tb[kk >> lgP], (unsigned)pmax);  // a negative entry: the last page
      }
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) {
        const int rw = min(t0 + u * GROUPS + g, kend - 1) & pmask;
        ku[u] = *(const uint4*)(kb + (int64_t)pg[u] * a.ks[0] + (int64_t)rw * a.ks[2]);
      }
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) {
        const int rw = min(t0 + u * GROUPS + g, kend - 1) & pmask;
        vu[u] = *(const uint4*)(vb + (int64_t)pg[u] * a.vs[0] + (int64_t)rw * a.vs[2]);
      }
    };
    // with registers to spare (NQ <= 4) the next tile's loads are issued before this tile's
    // arithmetic, so a wave always has a tile in flight
    constexpr bool kAhead = NQ <= 4;
    // one tile's arithmetic on the rows in ku / vu
    auto consume = [&](int t0, const uint4* ku, const uint4* vu) {
      int key[kDecUnroll];
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) key[u] = t0 + u * GROUPS + g;
      float s[NQ][kDecUnroll];
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) {
        const bool live = key[u] < kend && c < C;
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        const uint4 kx = live ? ku[u] : z;
        float kf[EPC];
        Chunk<T>::unpack(kx, kf);
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
          float dot = 0.f;
#pragma unroll
          for (int e = 0; e < EPC; ++e) dot = fmaf(qf[i][e], kf[e], dot);
          dot = group_sum<LPK>(dot) * a.scale_log2;
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
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        const uint4 vx = live ? vu[u] : z;
        float vf[EPC];
        Chunk<T>::unpack(vx, vf);
#pragma unroll
        for (int i = 0; i < NQ; ++i)
#pragma unroll
          for (int e = 0; e < EPC; ++e) acc[i][e] = fmaf(p[i][u], vf[e], acc[i][e]);
      }
    };
    constexpr int STEP = kDecWaves * TILE;
    uint4 ka[kDecUnroll], va[kDecUnroll];
    if constexpr (kAhead) {
      // two register sets used in turn (no copies: a copy would wait for the tile just issued)
      uint4 kb2[kDecUnroll], vb2[kDecUnroll];
      int t0 = k0 + wave * TILE;
      if (t0 < kend) issue(t0, ka, va);
      while (t0 < kend) {
        issue(t0 + STEP, kb2, vb2);
        __builtin_amdgcn_sched_barrier(0);  // keep the loads ahead of the arithmetic
        consume(t0, ka, va);
        t0 += STEP;
        if (t0 >= kend) break;
        issue(t0 + STEP, ka, va);
        __builtin_amdgcn_sched_barrier(0);
        consume(t0, kb2, vb2);
        t0 += STEP;
      }
    } else {
      for (int t0 = k0 + wave * TILE; t0 < kend; t0 += STEP) {
        issue(t0, ka, va);
        consume(t0, ka, va);
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
      store_o4(a.o, a.o_f32, (int64_t)b * a.os[0] + (int64_t)(h0 + hh) * a.os[1] + (int64_t)qi * a.os[2] + 4 * e4, o);
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

template <typename T, int LPK> static hipError_t launch_paged_nq(const PagedDecodeArgs& a, dim3 grid, hipStream_t st) {
  const int rows = a.d.gs * a.d.Nq;  // register rows of a workgroup
  if (rows == 1) fa_decode_partial_paged<T, LPK, 1><<<grid, kDecWaves * 64, 0, st>>>(a);
  else if (rows <= 4) fa_decode_partial_paged<T, LPK, 4><<<grid, kDecWaves * 64, 0, st>>>(a);
  else fa_decode_partial_paged<T, LPK, 8><<<grid, kDecWaves * 64, 0, st>>>(a);
  return hipGetLastError();
}

template <typename T> static hipError_t launch_paged_partial(const PagedDecodeArgs& a, int lpk, dim3 grid, hipStream_t st) {
  switch (lpk) {
    case 4: return launch_paged_nq<T, 4>(a, grid, st);
    case 8: return launch_paged_nq<T, 8>(a, grid, st);
    case 16: return launch_paged_nq<T, 16>(a, grid, st);
    case 32: return launch_paged_nq<T, 32>(a, grid, st);
    case 64:  // fp32 d in (128, 256]; a bf16 row of d <= 256 has at most 32 chunks
      if constexpr (sizeof(T) == 4) return launch_paged_nq<T, 64>(a, grid, st);
      break;
  }
  return hipErrorInvalidValue;
}

// Sizes are validated by the caller (capi_paged.hip); the plan is decode_plan's at Nk = W * P.
hipError_t launch_decode_paged(const PagedDecodeArgs& a, bool bf16_in, int64_t B, hipStream_t st) {
  const int lpk = decode_lpk(a.d.d, bf16_in ? 2 : 4);
  const dim3 grid((unsigned)(B * a.d.Hkv * a.d.slices), (unsigned)a.d.nsplit);
  hipError_t e = bf16_in ? launch_paged_partial<bf16>(a, lpk, grid, st) : launch_paged_partial<float>(a, lpk, grid, st);
  if (e != hipSuccess || a.d.nsplit == 1) return e;
  return launch_decode_combine(a.d, B, st);
}

// ---- append through the block table -----------------------------------------------------------
// one 16-B chunk of a new K row and of the matching V row per thread. Dropped: a row at or past
// clamp(count[b], 0, Nq), a logical row outside [0, W * P), a row whose table entry is not a page
// of the pool (negative: unallocated). Nothing else in the pools is written
__global__ __launch_bounds__(256) void kv_cache_append_paged(const PagedAppendArgs a) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.total) return;
  const int c = (int)(t % a.chunks);
  int64_t r = t / a.chunks;
  const int i = (int)(r % a.Nq);
  r /= a.Nq;
  const int h = (int)(r % a.Hkv);
  const int64_t b = r / a.Hkv;
  const int cnt = a.count ? min(max(a.count[b], 0), a.Nq) : a.Nq;
  if (i >= cnt) return;
  const int64_t row = (int64_t)a.pos[b] + i;
  if (row < 0 || row >= ((int64_t)a.W << a.lgP)) return;
  const int pg = a.table[b * a.W + (row >> a.lgP)];
  if (pg < 0 || pg >= a.n_pages) return;
  const int64_t pr = row & ((1 << a.lgP) - 1);
  const int64_t es = a.esize, off = (int64_t)c * 16;
  const uint4 kx = *(const uint4*)(a.kn + (b * a.kns[0] + h * a.kns[1] + i * a.kns[2]) * es + off);
  const uint4 vx = *(const uint4*)(a.vn + (b * a.vns[0] + h * a.vns[1] + i * a.vns[2]) * es + off);
  *(uint4*)(a.kp + (pg * a.kps[0] + h * a.kps[1] + pr * a.kps[2]) * es + off) = kx;
  *(uint4*)(a.vp + (pg * a.vps[0] + h * a.vps[1] + pr * a.vps[2]) * es + off) = vx;
}

hipError_t launch_append_paged(const PagedAppendArgs& a, hipStream_t st) {
  const int64_t blocks = (a.total + 255) / 256;
  kv_cache_append_paged<<<dim3((unsigned)blocks), 256, 0, st>>>(a);
  return hipGetLastError();
}

// ---- gather into a contiguous cache -------------------------------------------------------------
// one 16-B chunk of a K row and of the matching V row per thread; rows at or past
// clamp(kv_len[b], 0, Nk) are neither read nor written (a row whose table entry is not a page of
// the pool neither)
__global__ __launch_bounds__(256) void kv_cache_gather_paged(const PagedGatherArgs a) {
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
  const int pg = a.table[b * a.W + (j >> a.lgP)];
  if (pg < 0 || pg >= a.n_pages) return;
  const int64_t pr = j & ((1 << a.lgP) - 1);
  const int64_t es = a.esize, off = (int64_t)c * 16;
  const uint4 kx = *(const uint4*)(a.kp + (pg * a.kps[0] + h * a.kps[1] + pr * a.kps[2]) * es + off);
  const uint4 vx = *(const uint4*)(a.vp + (pg * a.vps[0] + h * a.vps[1] + pr * a.vps[2]) * es + off);
  *(uint4*)(a.ko + (b * a.kos[0] + h * a.kos[1] + (int64_t)j * a.kos[2]) * es + off) = kx;
  *(uint4*)(a.vo + (b * a.vos[0] + h * a.vos[1] + (int64_t)j * a.vos[2]) * es + off) = vx;
}

hipError_t launch_gather_paged(const PagedGatherArgs& a, hipStream_t st) {
  const int64_t blocks = (a.total + 255) / 256;
  kv_cache_gather_paged<<<dim3((unsigned)blocks), 256, 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace mt
