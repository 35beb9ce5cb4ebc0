// mt_moe_rows / mt_moe_route (include/minitorch_hip.h): the mixture-of-experts MLP of a cached
// decode step. A router picks k of E gated (SwiGLU) expert MLPs per row; only the chosen experts'
// weights are read. fp32 throughout, products on v_mfma_f32_16x16x4_f32, no atomics.
//
//   xh = norm(x)                      [M <= 64, K <= 1024]   (mt_linear_rows_ex's prologue)
//   r  = xh @ Wr                      [M, E]                 router logits
//   e(m, j), g(m, j), j < k           the k largest logits (lower index wins a tie), softmax over them
//   h(m, j) = silu(xh W_gate[e] + b_gate[e]) * (xh W_up[e] + b_up[e])          [F]
//   y(m, j) = g(m, j) * (h(m, j) W_out[e] + b_out[e])                          [N]
//   out[m]  = residual[m] + ((y(m, 0) + y(m, 1)) + ...)
//
// Four launches, every grid a function of the host arguments alone (a captured step replays):
//  1. route_kernel, a wave per row. The row statistics are linear_rows' (the same per-lane sums
//     and shuffle tree), the normalised row goes to the workspace and to the wave's LDS slice.
//     The 64 lanes are 64 / EP groups of EP = pow2(E) lanes: lane (grp, e) sums xh[k] Wr[k][e]
//     over k = grp, grp + G, ... (a wave instruction reads G consecutive rows of Wr), an xor
//     butterfly over the groups leaves every expert's logit in lane e. Top-k is k rounds of a
//     wave-wide max and a ballot whose lowest set lane is the winner; lane j keeps slot j.
//  2. expert_kernel<GATED = true>, grid (ceil(F / 32), E): the gated tile of mt_linear_rows_ex (32
//     gate columns and the 32 up columns beside them) of ONE expert. Wave 0 builds the list of
//     (row, slot) entries routed to the expert by ballot and prefix count over the M k <= 512
//     entries (ascending, so ascending rows); an expert nobody chose leaves before it has touched
//     a byte of its weights. Otherwise the listed rows of xh are gathered into LDS, zero-padded
//     to 16 RB rows with RB = 1, 2 or 4 chosen from the count, and the K loop is linear_rows':
//     16-byte loads of W, four MFMAs per k-step and row block, K split over four waves when
//     K % 16 == 0, ((p0 + p1) + p2) + p3. The epilogue writes silu(a) * b to h at the entry's slot.
//  3. expert_kernel<GATED = false>, grid (ceil(N / 64), E): the same gather from h, 64 output
//     columns, the epilogue scales by the entry's gate and writes y at the entry's slot.
//  4. combine_kernel: the slots of a row added in ascending order, then the residual. (Folding
//     this into 3 would need one workgroup to own a row's k experts in turn, which serialises
//     the experts, or atomics / counters; so it is its own small launch.)
//
// Row independence: a row's statistics and logits are one wave's fixed trees over that row; its
// dot products are one MFMA accumulation chain per wave in ascending k wherever the row sits in
// the gathered block (D[i][j] reads row i of A only) and RB only adds independent chains. So
// the bits of out row m depend on x row m, residual row m, the weights and the sizes alone.
// An expert's weights never meet a row that did not choose it: 0 * inf cannot happen.
// A row with a non-finite logit gets idx -1 and NaN gates: no expert lists it and combine
// writes NaN for it without reading y.
#include "../../include/minitorch_hip.h"
#include "fa_common.h"
#include "silu.h"
#include <type_traits>

namespace mt {
int set_error(const char* fmt, ...);  // capi_flash.hip
int check_hip(hipError_t e, const char* where);

namespace moe {
constexpr int kTile = 64;   // tile columns per workgroup (gated: 32 gate + 32 up)
constexpr int kChunk = 32;  // k rows a wave stages and multiplies at a time
constexpr int kSteps = kChunk / 4;
constexpr int kXStride = kChunk + 4;
constexpr int kMaxM = 64, kMaxK = 1024, kMaxE = 64, kMaxTop = 8;

typedef float f32x4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

struct RouteArgs {
  const float* x;
  const float* gamma;
  const float* beta;
  const float* Wr;
  float* xh;      // [M, K] or NULL
  int* idx;       // [M, k] or NULL
  float* gate;    // [M, k] or NULL
  int* idx2;      // the caller's copies (mt_moe_rows' optional outputs)
  float* gate2;
  float* mask;    // [M, E] 0 / 1 or NULL
  int64_t ldx;
  int M, K, E, k, ep;  // ep: E rounded up to a power of two
  int norm;
  float eps;
};

__global__ __launch_bounds__(256) void route_kernel(const RouteArgs a) {
  __shared__ __attribute__((aligned(16))) float xs_all[4][kMaxK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool rowok = blockIdx.x * 4 + wave < a.M;  // a wave past the last row redoes it and writes nothing
  const int m = min((int)blockIdx.x * 4 + wave, a.M - 1);
  const int K = a.K, E = a.E;
  float* xs = xs_all[wave];
  const float* xr = a.x + (int64_t)m * a.ldx;

  // linear_rows' statistics: (x + y) + (z + w) per lane and 256 columns, then the wave tree
  float4 v[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) v[t] = *(const float4*)(xr + (4 * lane + 256 * t < K ? 4 * lane + 256 * t : 0));
  float mean = 0.f, rsd = 1.f;
  if (a.norm) {
    float s = 0.f, ss = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float in = 4 * lane + 256 * t < K ? 1.f : 0.f;
      const float4 e = v[t];
      s += in * ((e.x + e.y) + (e.z + e.w));
      ss += in * ((e.x * e.x + e.y * e.y) + (e.z * e.z + e.w * e.w));
    }
    s = wave_sum(s);
    ss = wave_sum(ss);
    mean = a.norm == 2 ? 0.f : s / (float)K;
    const float var = a.norm == 2 ? ss / (float)K + a.eps : ss / (float)K - mean * mean + a.eps;
    rsd = 1.f / sqrtf(var);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = 4 * lane + 256 * t;
    if (c < K) {
      float4 o = v[t];
      if (a.norm == 2) {
        const float4 gm = *(const float4*)(a.gamma + c);
        o = make_float4(gm.x * (o.x * rsd), gm.y * (o.y * rsd), gm.z * (o.z * rsd), gm.w * (o.w * rsd));
      } else if (a.norm == 1) {
        const float4 gm = *(const float4*)(a.gamma + c), bt = *(const float4*)(a.beta + c);
        o = make_float4(gm.x * ((o.x - mean) * rsd) + bt.x, gm.y * ((o.y - mean) * rsd) + bt.y,
                        gm.z * ((o.z - mean) * rsd) + bt.z, gm.w * ((o.w - mean) * rsd) + bt.w);
      }
      *(float4*)(xs + c) = o;
      if (a.xh && rowok) *(float4*)(a.xh + (int64_t)m * K + c) = o;
    }
  }
  __syncthreads();

  // logits: lane (grp, e) takes k = grp, grp + G, ...; four rows of Wr in flight per lane
  const int ep = a.ep, G = 64 / ep;
  const int e = lane & (ep - 1), grp = lane / ep;
  const bool live = e < E;
  const float* wcol = a.Wr + (live ? e : 0);
  float r = 0.f;
  for (int k0 = grp; k0 < K; k0 += 4 * G) {
    float w[4], xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int kk = k0 + u * G;
      const int kc = min(kk, K - 1);
      w[u] = wcol[(int64_t)kc * E];
      xv[u] = kk < K ? xs[kc] : 0.f;
      if (kk >= K) w[u] = 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) r = fmaf(xv[u], w[u], r);
  }
  for (int o = 32; o >= ep; o >>= 1) r += __shfl_xor(r, o, 64);  // every group now holds the sum

  // selection among lanes e < E of group 0
  const bool cand0 = lane < E;
  const bool bad = __ballot(cand0 && !(fabsf(r) <= 3.402823466e38f)) != 0;
  bool taken = false;
  int my_e = -1;
  float my_r = 0.f;
  for (int j = 0; j < a.k; ++j) {
    const bool c = cand0 && !taken;
    const float mx = wave_max(c ? r : -INFINITY);
    const unsigned long long b = __ballot(c && r == mx);
    const int win = b ? __ffsll((long long)b) - 1 : 0;
    if (lane == win) taken = true;
    if (lane == j) { my_e = win; my_r = mx; }
  }
  const float r0 = __shfl(my_r, 0, 64);
  const float ex = lane < a.k ? expf(my_r - r0) : 0.f;
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < kMaxTop; ++j) {
    const float t = __shfl(ex, j, 64);
    if (j < a.k) sum += t;
  }
  float g = ex / sum;
  if (bad) { my_e = -1; g = __builtin_nanf(""); taken = false; }
  if (lane < a.k && rowok) {
    const int64_t o = (int64_t)m * a.k + lane;
    if (a.idx) a.idx[o] = my_e;
    if (a.gate) a.gate[o] = g;
    if (a.idx2) a.idx2[o] = my_e;
    if (a.gate2) a.gate2[o] = g;
  }
  if (a.mask && cand0 && rowok) a.mask[(int64_t)m * E + lane] = taken ? 1.f : 0.f;
}

struct ExpertArgs {
  const float* A;     // the rows to gather: xh [M, lda] (GATED) or h [M k, lda]
  const float* W;     // [E, Kd, ldw]
  const float* bias;  // [E, ldw] or NULL
  const int* idx;     // [M k]
  const float* gate;  // [M k]
  float* out;         // h [M k, ldo] (GATED) or y [M k, ldo]
  int64_t lda, ldo;
  int64_t N;          // output columns (F of the gated stage)
  int Kd;             // reduction length
  int entries, k;     // M k
  int vec_io;
};

// 4 columns of row kk of the expert's W from column col on; rows >= Kd read as zero (from a valid
// address), a column >= N re-reads column 0 (one that exists) and is dropped by the epilogue
template <bool VEC>
__device__ __forceinline__ float4 load_w(const float* __restrict__ W, int64_t ld, int64_t half, int64_t N, int Kd,
                                         int kk, int64_t col) {
  const float* row = W + (int64_t)min(kk, Kd - 1) * ld + half;
  float4 w;
  if (VEC) {
    w = *(const float4*)(row + (col < N ? col : 0));
  } else {
    float e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) e[i] = row[col + i < N ? col + i : 0];
    w = make_float4(e[0], e[1], e[2], e[3]);
  }
  return kk < Kd ? w : make_float4(0.f, 0.f, 0.f, 0.f);
}

// The K loop, K-split combine and epilogue of one expert tile over cnt <= 16 RB gathered rows.
template <int RB, int KS, bool VEC, bool GATED>
__device__ __forceinline__ void expert_tile(const ExpertArgs& a, float* smem, const int* list, int cnt, int ex) {
  constexpr int ROWS = 16 * RB;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int64_t N = a.N;
  const int64_t n0 = (int64_t)blockIdx.x * (GATED ? kTile / 2 : kTile);
  const int64_t ldw = GATED ? 2 * N : N, whalf = GATED && j >= 8 ? N : 0;
  const int64_t wcol = GATED ? n0 + 4 * (j & 7) : n0 + 4 * j;
  const int Kd = a.Kd;
  const float* __restrict__ W = a.W + (int64_t)ex * Kd * ldw;
  auto load = [&](int kk) { return load_w<VEC>(W, ldw, whalf, N, Kd, kk, wcol); };
  const int S = KS > 1 ? Kd / KS : Kd;  // this wave's k rows: [wave S, wave S + S)
  const int kw = wave * S, kend = kw + S;
  const int nch = (S + kChunk - 1) / kChunk;

  float4 wa[kSteps], wb[kSteps];
#pragma unroll
  for (int s = 0; s < kSteps; ++s) wa[s] = load(kw + 4 * s + q);

  f32x4v acc[RB][4];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[rb][c] = f32x4v{0.f, 0.f, 0.f, 0.f};

  float* xs = smem + wave * ROWS * kXStride;
  const int xr = lane >> 3, xc = 4 * (lane & 7);
  // the gathered rows this lane stages: entry -> row of A (the entry's row m for xh, the entry for h)
  const float* arow[ROWS / 8];
#pragma unroll
  for (int p = 0; p < ROWS / 8; ++p) {
    const int en = list[min(8 * p + xr, cnt - 1)];
    arow[p] = a.A + (int64_t)(GATED ? en / a.k : en) * a.lda;
  }
  auto chunk = [&](int ch, auto pf) {
    const int kb = kw + ch * kChunk;
    const int cw = min(kChunk, S - ch * kChunk);
    const bool cok = xc < cw;
    const int kx = cok ? kb + xc : kb;  // lda is a multiple of 4: the 16 bytes are inside the row
    float4 xv[ROWS / 8];
#pragma unroll
    for (int p = 0; p < ROWS / 8; ++p) xv[p] = *(const float4*)(arow[p] + kx);
    if constexpr (decltype(pf)::value) {
#pragma unroll
      for (int s = 0; s < kSteps; ++s) wb[s] = load(kb + kChunk + 4 * s + q);
    }
#pragma unroll
    for (int p = 0; p < ROWS / 8; ++p) {
      // rows past the list, columns past the wave's range (the pad of a row of h) are zero
      const bool rok = 8 * p + xr < cnt && cok;
      xv[p] = make_float4(rok && kx + 0 < kend ? xv[p].x : 0.f, rok && kx + 1 < kend ? xv[p].y : 0.f,
                          rok && kx + 2 < kend ? xv[p].z : 0.f, rok && kx + 3 < kend ? xv[p].w : 0.f);
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < ROWS / 8; ++p) *(float4*)(xs + (8 * p + xr) * kXStride + xc) = xv[p];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      if (4 * s < cw) {
        const float w4[4] = {wa[s].x, wa[s].y, wa[s].z, wa[s].w};
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          const float av = xs[(16 * rb + j) * kXStride + 4 * s + q];
#pragma unroll
          for (int c = 0; c < 4; ++c)
            acc[rb][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w4[c], acc[rb][c], 0, 0, 0);
        }
      }
    }
    if constexpr (decltype(pf)::value) {
#pragma unroll
      for (int s = 0; s < kSteps; ++s) wa[s] = wb[s];
    }
  };
  for (int ch = 0; ch + 1 < nch; ++ch) chunk(ch, std::true_type{});
  chunk(nch - 1, std::false_type{});
  __syncthreads();  // the x slices become the partial tiles

  auto slot_at = [&](int slot, int rb, int r) { return smem + (slot * ROWS + 16 * rb + 4 * q + r) * kTile + 4 * j; };
  if (KS > 1 && wave > 0) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        *(float4*)slot_at(wave - 1, rb, r) = make_float4(acc[rb][0][r], acc[rb][1][r], acc[rb][2][r], acc[rb][3][r]);
  }
  if (KS > 1) __syncthreads();
  if (wave == 0) {  // ((p0 + p1) + p2) + p3 into slot 0
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float4 t = make_float4(acc[rb][0][r], acc[rb][1][r], acc[rb][2][r], acc[rb][3][r]);
#pragma unroll
        for (int w = 1; w < KS; ++w) {
          const float4 p = *(const float4*)slot_at(w - 1, rb, r);
          t.x += p.x; t.y += p.y; t.z += p.z; t.w += p.w;
        }
        *(float4*)slot_at(0, rb, r) = t;
      }
  }
  __syncthreads();

  const float* __restrict__ bias = a.bias ? a.bias + (int64_t)ex * ldw : nullptr;
  if (GATED) {  // 4 gate columns and their 4 up columns per thread and pass -> h at the entry's slot
    for (int i = threadIdx.x; i < cnt * (kTile / 8); i += 64 * KS) {
      const int r = i >> 3, c = 4 * (i & 7);
      const int64_t col = n0 + c;
      if (col >= N) continue;
      const float4 ta = *(const float4*)(smem + r * kTile + c), tb = *(const float4*)(smem + r * kTile + kTile / 2 + c);
      const float va[4] = {ta.x, ta.y, ta.z, ta.w}, vb[4] = {tb.x, tb.y, tb.z, tb.w};
      float* o = a.out + (int64_t)list[r] * a.ldo + col;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = col + e < N;
        float ua = va[e], ub = vb[e];
        if (bias && in) { ua += bias[col + e]; ub += bias[N + col + e]; }
        v[e] = silu(ua) * ub;
      }
      if (a.vec_io) {
        *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (col + e < N) o[e] = v[e];
      }
    }
    return;
  }
  for (int i = threadIdx.x; i < cnt * (kTile / 4); i += 64 * KS) {  // gate * (t + bias) -> y at the slot
    const int r = i >> 4;
    const int64_t col = n0 + 4 * (i & 15);
    if (col >= N) continue;
    const float4 t = *(const float4*)(smem + r * kTile + 4 * (i & 15));
    const int en = list[r];
    const float g = a.gate[en];
    float v[4] = {t.x, t.y, t.z, t.w};
    float* o = a.out + (int64_t)en * a.ldo + col;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (bias && col + e < N) v[e] += bias[col + e];
      v[e] = g * v[e];
    }
    if (a.vec_io) {
      *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (col + e < N) o[e] = v[e];
    }
  }
}

template <int KS, bool VEC, bool GATED>
__global__ __launch_bounds__(64 * KS) void expert_kernel(const ExpertArgs a) {
  constexpr int SLOTS = KS > 1 ? KS - 1 : 1;
  constexpr int XS = KS * kMaxM * kXStride, PS = SLOTS * kMaxM * kTile;
  __shared__ __attribute__((aligned(16))) float smem[XS > PS ? XS : PS];
  __shared__ int list[kMaxM];
  __shared__ int count;
  const int ex = blockIdx.y;
  if (threadIdx.x < 64) {  // wave 0: the entries routed to this expert, ascending
    const int lane = threadIdx.x;
    int base = 0;
    for (int i0 = 0; i0 < a.entries; i0 += 64) {
      const int i = i0 + lane;
      const bool hit = i < a.entries && a.idx[i] == ex;
      const unsigned long long b = __ballot(hit);
      const int pos = base + __popcll(b & ((1ull << lane) - 1ull));
      if (hit && pos < kMaxM) list[pos] = i;  // a row names an expert once: pos < M always
      base += __popcll(b);
    }
    if (lane == 0) count = min(base, kMaxM);
  }
  __syncthreads();
  const int cnt = count;
  if (cnt == 0) return;  // nobody chose this expert: its weights are not read
  if (cnt <= 16) expert_tile<1, KS, VEC, GATED>(a, smem, list, cnt, ex);
  else if (cnt <= 32) expert_tile<2, KS, VEC, GATED>(a, smem, list, cnt, ex);
  else expert_tile<4, KS, VEC, GATED>(a, smem, list, cnt, ex);
}

__global__ __launch_bounds__(256) void combine_kernel(const float* __restrict__ y, const float* __restrict__ gate,
                                                      const float* __restrict__ res, float* __restrict__ out, int M,
                                                      int64_t N, int k) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)M * N) return;
  const int64_t m = i / N, n = i - m * N;
  float s;
  if (gate[m * k] != gate[m * k]) {  // a non-finite router logit: the row is NaN, y was not written
    s = __builtin_nanf("");
  } else {
    s = y[(m * k) * N + n];
    for (int j = 1; j < k; ++j) s += y[(m * k + j) * N + n];
  }
  out[i] = res ? res[i] + s : s;
}

template <bool GATED>
static void launch_expert(const ExpertArgs& a, int tiles, int E, bool vec, hipStream_t st) {
  const dim3 grid(tiles, E);
  if (a.Kd % 16 == 0) {
    if (vec) hipLaunchKernelGGL((expert_kernel<4, true, GATED>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((expert_kernel<4, false, GATED>), grid, dim3(256), 0, st, a);
  } else {
    if (vec) hipLaunchKernelGGL((expert_kernel<1, true, GATED>), grid, dim3(64), 0, st, a);
    else hipLaunchKernelGGL((expert_kernel<1, false, GATED>), grid, dim3(64), 0, st, a);
  }
}

static int64_t up4(int64_t n) { return (n + 3) & ~(int64_t)3; }

// the workspace: xh [M, K] | idx [M k] | gate [M k] | h [M k, up4(F)] | y [M k, N], each from a 16-byte boundary
struct Layout {
  int64_t xh, idx, gate, h, y, total;  // offsets in 4-byte elements
};
static Layout layout(int64_t M, int64_t K, int64_t F, int64_t N, int64_t k) {
  Layout l;
  l.xh = 0;
  l.idx = l.xh + up4(M * K);
  l.gate = l.idx + up4(M * k);
  l.h = l.gate + up4(M * k);
  l.y = l.h + M * k * up4(F);
  l.total = l.y + up4(M * k * N);
  return l;
}

static int check_route(const char* fn, const float* x, int64_t ldx, int64_t M, int64_t maxM, int64_t K, int norm,
                       const float* gamma, const float* beta, float eps, const float* Wr, int64_t E, int64_t k) {
  if (M < 1 || M > maxM) return set_error("%s: M=%lld is outside 1..%lld", fn, (long long)M, (long long)maxM);
  if (K < 4 || K > kMaxK || K % 4) return set_error("%s: K=%lld must be a multiple of 4 in 4..%d", fn, (long long)K, kMaxK);
  if (E < 2 || E > kMaxE) return set_error("%s: E=%lld is outside 2..%d", fn, (long long)E, kMaxE);
  if (k < 1 || k > kMaxTop) return set_error("%s: k=%lld is outside 1..%d", fn, (long long)k, kMaxTop);
  if (k > E) return set_error("%s: k=%lld exceeds E=%lld", fn, (long long)k, (long long)E);
  if (!x) return set_error("%s: x is NULL", fn);
  if (!Wr) return set_error("%s: Wr is NULL", fn);
  if (ldx < K || ldx % 4) return set_error("%s: ldx=%lld must be a multiple of 4 and >= K", fn, (long long)ldx);
  if (norm < 0 || norm > 2) return set_error("%s: norm=%d is outside 0..2 (none, LayerNorm, RMSNorm)", fn, norm);
  if (norm == 0 && (gamma || beta)) return set_error("%s: norm=0 takes no gamma and no beta", fn);
  if (norm == 1 && (!gamma || !beta)) return set_error("%s: gamma and beta are NULL together or not at all", fn);
  if (norm == 2 && !gamma) return set_error("%s: RMSNorm (norm=2) needs gamma", fn);
  if (norm == 2 && beta) return set_error("%s: RMSNorm (norm=2) has no beta", fn);
  if (norm && !(eps >= 0.f)) return set_error("%s: eps=%g is negative", fn, (double)eps);
  if ((uintptr_t)x & 15) return set_error("%s: x is misaligned (16 bytes)", fn);
  if (((uintptr_t)gamma | (uintptr_t)beta) & 15) return set_error("%s: gamma / beta are misaligned (16 bytes)", fn);
  if ((uintptr_t)Wr & 3) return set_error("%s: Wr is misaligned (4 bytes)", fn);
  return 0;
}

static void launch_route(RouteArgs& a, int64_t E, hipStream_t st) {
  a.ep = 2;
  while (a.ep < E) a.ep *= 2;
  hipLaunchKernelGGL(route_kernel, dim3((a.M + 3) / 4), dim3(256), 0, st, a);
}
}  // namespace moe
}  // namespace mt

using namespace mt;
using namespace mt::moe;

extern "C" int mt_moe_rows_workspace_bytes(int64_t M, int64_t K, int64_t F, int64_t N, int64_t E, int64_t k,
                                           int64_t* bytes) {
  const char* fn = "mt_moe_rows_workspace_bytes";
  if (!bytes) return set_error("%s: bytes is NULL", fn);
  if (M < 1 || M > kMaxM) return set_error("%s: M=%lld is outside 1..%d", fn, (long long)M, kMaxM);
  if (K < 4 || K > kMaxK || K % 4) return set_error("%s: K=%lld must be a multiple of 4 in 4..%d", fn, (long long)K, kMaxK);
  if (F < 1 || F > (1 << 20)) return set_error("%s: F=%lld is outside 1..2^20", fn, (long long)F);
  if (N < 1 || N > (1 << 20)) return set_error("%s: N=%lld is outside 1..2^20", fn, (long long)N);
  if (E < 2 || E > kMaxE) return set_error("%s: E=%lld is outside 2..%d", fn, (long long)E, kMaxE);
  if (k < 1 || k > kMaxTop) return set_error("%s: k=%lld is outside 1..%d", fn, (long long)k, kMaxTop);
  if (k > E) return set_error("%s: k=%lld exceeds E=%lld", fn, (long long)k, (long long)E);
  *bytes = layout(M, K, F, N, k).total * 4;
  return 0;
}

extern "C" int mt_moe_route(const float* x, int64_t ldx, int64_t M, int64_t K, int norm, const float* gamma,
                            const float* beta, float eps, const float* Wr, int64_t E, int64_t k, float* xh,
                            int32_t* topk_idx, float* topk_gate, float* mask, void* stream) {
  const char* fn = "mt_moe_route";
  if (int rc = check_route(fn, x, ldx, M, 1 << 24, K, norm, gamma, beta, eps, Wr, E, k)) return rc;
  if (!xh && !topk_idx && !topk_gate && !mask) return set_error("%s: every output is NULL", fn);
  if ((uintptr_t)xh & 15) return set_error("%s: xh is misaligned (16 bytes)", fn);
  if (((uintptr_t)topk_idx | (uintptr_t)topk_gate | (uintptr_t)mask) & 3)
    return set_error("%s: topk_idx, topk_gate or mask is misaligned (4 bytes)", fn);
  RouteArgs a = {};
  a.x = x; a.gamma = gamma; a.beta = beta; a.Wr = Wr; a.xh = xh; a.idx = topk_idx; a.gate = topk_gate; a.mask = mask;
  a.ldx = ldx; a.M = (int)M; a.K = (int)K; a.E = (int)E; a.k = (int)k; a.norm = norm; a.eps = eps;
  launch_route(a, E, (hipStream_t)stream);
  return check_hip(hipGetLastError(), fn);
}

extern "C" int mt_moe_rows(const float* x, int64_t ldx, int64_t M, int64_t K, int norm, const float* gamma,
                           const float* beta, float eps, const float* Wr, int64_t E, int64_t k, const float* W_in,
                           const float* b_in, int64_t F, const float* W_out, const float* b_out, int64_t N,
                           const float* residual, float* out, int32_t* topk_idx, float* topk_gate, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  const char* fn = "mt_moe_rows";
  if (int rc = check_route(fn, x, ldx, M, kMaxM, K, norm, gamma, beta, eps, Wr, E, k)) return rc;
  if (F < 1 || F > (1 << 20)) return set_error("%s: F=%lld is outside 1..2^20", fn, (long long)F);
  if (N < 1 || N > (1 << 20)) return set_error("%s: N=%lld is outside 1..2^20", fn, (long long)N);
  if (!W_in || !W_out) return set_error("%s: W_in or W_out is NULL", fn);
  if (!out) return set_error("%s: out is NULL", fn);
  if (!workspace) return set_error("%s: workspace is NULL", fn);
  if ((uintptr_t)workspace & 15) return set_error("%s: workspace is misaligned (16 bytes)", fn);
  if (((uintptr_t)W_in | (uintptr_t)W_out | (uintptr_t)b_in | (uintptr_t)b_out | (uintptr_t)residual | (uintptr_t)out |
       (uintptr_t)topk_idx | (uintptr_t)topk_gate) & 3)
    return set_error("%s: a weight, bias, residual or output pointer is misaligned (4 bytes)", fn);
  const Layout l = layout(M, K, F, N, k);
  if (workspace_bytes < l.total * 4)
    return set_error("%s: workspace_bytes=%lld is below the %lld bytes mt_moe_rows_workspace_bytes asks for", fn,
                     (long long)workspace_bytes, (long long)(l.total * 4));
  const uintptr_t ob = (uintptr_t)out, oe = ob + (uintptr_t)(M * N * 4);
  const uintptr_t xb = (uintptr_t)x, xe = xb + (uintptr_t)(((M - 1) * ldx + K) * 4);
  if (ob < xe && xb < oe) return set_error("%s: out overlaps x", fn);

  float* ws = (float*)workspace;
  const hipStream_t st = (hipStream_t)stream;
  RouteArgs r = {};
  r.x = x; r.gamma = gamma; r.beta = beta; r.Wr = Wr; r.xh = ws + l.xh; r.idx = (int*)(ws + l.idx); r.gate = ws + l.gate;
  r.idx2 = topk_idx; r.gate2 = topk_gate; r.ldx = ldx; r.M = (int)M; r.K = (int)K; r.E = (int)E; r.k = (int)k;
  r.norm = norm; r.eps = eps;
  launch_route(r, E, st);

  ExpertArgs a = {};
  a.A = ws + l.xh; a.W = W_in; a.bias = b_in; a.idx = r.idx; a.gate = r.gate; a.out = ws + l.h; a.lda = K;
  a.ldo = up4(F); a.N = F; a.Kd = (int)K; a.entries = (int)(M * k); a.k = (int)k; a.vec_io = 1;  // ldo % 4 == 0: whole float4s fit
  launch_expert<true>(a, (int)((F + kTile / 2 - 1) / (kTile / 2)), (int)E, F % 4 == 0 && !((uintptr_t)W_in & 15), st);

  ExpertArgs b = {};
  b.A = ws + l.h; b.W = W_out; b.bias = b_out; b.idx = r.idx; b.gate = r.gate; b.out = ws + l.y; b.lda = up4(F);
  b.ldo = N; b.N = N; b.Kd = (int)F; b.entries = (int)(M * k); b.k = (int)k; b.vec_io = N % 4 == 0;
  launch_expert<false>(b, (int)((N + kTile - 1) / kTile), (int)E, N % 4 == 0 && !((uintptr_t)W_out & 15), st);

  hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((M * N + 255) / 256)), dim3(256), 0, st, ws + l.y, r.gate, residual,
                     out, (int)M, N, (int)k);
  return check_hip(hipGetLastError(), fn);
}
