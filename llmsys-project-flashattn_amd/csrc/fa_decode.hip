// KV-cache decode attention (mt_flash_attn_decode) and the cache append (mt_kv_cache_append).
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
// Pass 2, fa_decode_combine: one 64-thread workgroup per (b, h, query) merges the splits in
// index order (rescale to the largest m, sum l and O, normalise): a fixed order, bit-reproducible.
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
#include "fa_decode.h"
#include <algorithm>

namespace mt {

constexpr int kDecTargetWgs = 1024;  // 4 workgroups per CU when B*H alone is short of that

// lanes per key: the power of two >= chunks per row, at least 4
int decode_lpk(int64_t d, int esize) {
  const int c = (int)(d * esize / 16);
  int l = 4;
  while (l < c) l *= 2;
  return l;
}

DecodePlan decode_plan(int esize, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk, int64_t d) {
  DecodePlan p;
  p.lpk = decode_lpk(d, esize);
  p.tile = kDecUnroll * 64 / p.lpk;
  const int64_t G = H / Hkv;
  p.gs = (int)std::min<int64_t>(G, 8 / Nq);
  p.slices = (int)((G + p.gs - 1) / p.gs);
  // The span is sized by the query heads, B * H, whatever Hkv: a packed workgroup streams the
  // keys a plain one does (for gs heads at once), the grid is B * Hkv * slices per split and
  // the workspace and the combine are those of the plain plan. Sizing it by the B * Hkv *
  // slices workgroups instead gives G times the splits at a small B * Hkv, and every split is
  // one more workspace row per query for the combine's serial merge: at (1,16,16384,128) bf16,
  // Hkv = 4, 256 splits took 111 us against 38 us with the plain plan's 64 (and 52 us for
  // the plain kernel on the repeated K/V); DESIGN.md section 3, "Grouped-query decode".
  const int64_t bh = B * H;
  const int64_t want = std::max<int64_t>(1, (kDecTargetWgs + bh - 1) / bh);
  int64_t span = std::max<int64_t>((Nk + want - 1) / want, (int64_t)kDecWaves * p.tile);
  span = (span + p.tile - 1) / p.tile * p.tile;
  p.span = (int)span;
  p.nsplit = (int)((Nk + span - 1) / span);
  return p;
}

// fp32, one row, d <= 64 sits at the 96-VGPR edge of 5 waves per SIMD: ask for them (the allocator
// otherwise lands on 95-98 from one build to the next)
template <typename T, int LPK, int NQ>
__global__ __launch_bounds__(kDecWaves * 64)
__attribute__((amdgpu_waves_per_eu(sizeof(T) == 4 && NQ == 1 && LPK <= 16 ? 5 : 1)))
void fa_decode_partial(const DecodeArgs a) {
  constexpr int EPC = Chunk<T>::N;       // elements per 16-B chunk
  constexpr int GROUPS = 64 / LPK;       // keys per wave-wide load
  constexpr int TILE = kDecUnroll * GROUPS;
  constexpr int DP = LPK * EPC;          // padded head dim of the LDS image
  __shared__ float s_o[kDecWaves][NQ][DP];
  __shared__ float s_ml[kDecWaves][NQ][2];

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
    const T* kb = (const T*)a.k + (int64_t)b * a.ks[0] + (int64_t)hkv * a.ks[1];
    const T* vb = (const T*)a.v + (int64_t)b * a.vs[0] + (int64_t)hkv * a.vs[1];
    const int cc = c < C ? c : 0;  // a lane past the row's chunks re-reads chunk 0 (values dropped)

    // the 16-B loads of one tile: K then V rows of kDecUnroll x GROUPS keys. Keys at or past kend
    // re-read row kend - 1 (in [k0, n): a visible, initialised row); their values are dropped below
    auto issue = [&](int t0, uint4* ku, uint4* vu) {
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) {
        const int kk = min(t0 + u * GROUPS + g, kend - 1);
        ku[u] = *(const uint4*)(kb + (int64_t)kk * a.ks[2] + cc * EPC);
      }
#pragma unroll
      for (int u = 0; u < kDecUnroll; ++u) {
        const int kk = min(t0 + u * GROUPS + g, kend - 1);
        vu[u] = *(const uint4*)(vb + (int64_t)kk * a.vs[2] + cc * EPC);
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

__global__ __launch_bounds__(64) void fa_decode_combine(const DecodeArgs a) {
  const int64_t row = blockIdx.x;  // (b, h, query)
  const int e4 = threadIdx.x, d4 = a.d / 4;
  if (e4 >= d4) return;
  const int64_t bh = row / a.Nq;
  const int i = (int)(row - bh * a.Nq);
  const int b = (int)(bh / a.H), h = (int)(bh % a.H);
  const int64_t rows = (int64_t)gridDim.x;
  const float* wo = a.ws + row * a.nsplit * a.d;
  const float* ml = a.ws + rows * a.nsplit * a.d + 2 * row * a.nsplit;
  float mx = -INFINITY;
  for (int s = 0; s < a.nsplit; ++s) mx = fmaxf(mx, ml[2 * s]);
  const float ms = mx == -INFINITY ? 0.f : mx;
  float ls = 0.f;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < a.nsplit; ++s) {
    const float ms_s = ml[2 * s];
    if (ms_s == -INFINITY) continue;  // a split with no visible key: its O is 0 by construction
    const float f = exp2_fast(ms_s - ms);
    const float4 x = *(const float4*)(wo + (int64_t)s * a.d + 4 * e4);
    ls += ml[2 * s + 1] * f;
    o.x += x.x * f; o.y += x.y * f; o.z += x.z * f; o.w += x.w * f;
  }
  const float inv = ls > 0.f ? 1.f / ls : 0.f;
  o.x *= inv; o.y *= inv; o.z *= inv; o.w *= inv;
  store_o4(a.o, a.o_f32, (int64_t)b * a.os[0] + (int64_t)h * a.os[1] + (int64_t)i * a.os[2] + 4 * e4, o);
  if (e4 == 0) {
    if (a.m) a.m[row] = mx * kLn2;
    if (a.l) a.l[row] = ls;
  }
}

template <typename T, int LPK> static hipError_t launch_partial_nq(const DecodeArgs& a, dim3 grid, hipStream_t st) {
  const int rows = a.gs * a.Nq;  // register rows of a workgroup
  if (rows == 1) fa_decode_partial<T, LPK, 1><<<grid, kDecWaves * 64, 0, st>>>(a);
  else if (rows <= 4) fa_decode_partial<T, LPK, 4><<<grid, kDecWaves * 64, 0, st>>>(a);
  else fa_decode_partial<T, LPK, 8><<<grid, kDecWaves * 64, 0, st>>>(a);
  return hipGetLastError();
}

template <typename T> static hipError_t launch_partial(const DecodeArgs& a, int lpk, dim3 grid, hipStream_t st) {
  switch (lpk) {
    case 4: return launch_partial_nq<T, 4>(a, grid, st);
    case 8: return launch_partial_nq<T, 8>(a, grid, st);
    case 16: return launch_partial_nq<T, 16>(a, grid, st);
    case 32: return launch_partial_nq<T, 32>(a, grid, st);
    case 64:  // fp32 d in (128, 256]; a bf16 row of d <= 256 has at most 32 chunks
      if constexpr (sizeof(T) == 4) return launch_partial_nq<T, 64>(a, grid, st);
      break;
  }
  return hipErrorInvalidValue;
}

// Sizes are validated by the caller (capi_decode.hip): 1 <= Nq <= 8, d <= 256, 16-B rows,
// Hkv divides H, gs / slices / rows from decode_plan.
hipError_t launch_decode(const DecodeArgs& a, bool bf16_in, int64_t B, hipStream_t st) {
  const int lpk = decode_lpk(a.d, bf16_in ? 2 : 4);
  const dim3 grid((unsigned)(B * a.Hkv * a.slices), (unsigned)a.nsplit);
  hipError_t e = bf16_in ? launch_partial<bf16>(a, lpk, grid, st) : launch_partial<float>(a, lpk, grid, st);
  if (e != hipSuccess || a.nsplit == 1) return e;
  return launch_decode_combine(a, B, st);
}

hipError_t launch_decode_combine(const DecodeArgs& a, int64_t B, hipStream_t st) {
  fa_decode_combine<<<dim3((unsigned)(B * a.H * a.Nq)), 64, 0, st>>>(a);
  return hipGetLastError();
}

// ---- cache append ---------------------------------------------------------------------------
// one 16-B chunk of a new K row and of the matching V row per thread; rows outside [0, Nmax)
// are dropped, nothing else in the caches is written
__global__ __launch_bounds__(256) void kv_cache_append(const AppendArgs a) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.total) return;
  const int c = (int)(t % a.chunks);
  int64_t r = t / a.chunks;
  const int i = (int)(r % a.Nq);
  r /= a.Nq;
  const int h = (int)(r % a.H);
  const int64_t b = r / a.H;
  const int64_t row = (int64_t)a.pos[b] + i;
  if (row < 0 || row >= a.Nmax) return;
  const int64_t es = a.esize, off = (int64_t)c * 16;
  const uint4 kx = *(const uint4*)(a.kn + (b * a.kns[0] + h * a.kns[1] + i * a.kns[2]) * es + off);
  const uint4 vx = *(const uint4*)(a.vn + (b * a.vns[0] + h * a.vns[1] + i * a.vns[2]) * es + off);
  *(uint4*)(a.kc + (b * a.kcs[0] + h * a.kcs[1] + row * a.kcs[2]) * es + off) = kx;
  *(uint4*)(a.vc + (b * a.vcs[0] + h * a.vcs[1] + row * a.vcs[2]) * es + off) = vx;
}

hipError_t launch_kv_append(const AppendArgs& a, hipStream_t st) {
  const int64_t blocks = (a.total + 255) / 256;
  kv_cache_append<<<dim3((unsigned)blocks), 256, 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace mt
