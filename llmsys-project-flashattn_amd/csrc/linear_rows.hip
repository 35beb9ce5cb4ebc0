// mt_linear_rows (include/minitorch_hip.h): the skinny fp32 linear of a cached decode step.
//   out_g = epilogue_g(prologue(x) @ W_g),  x [M <= 64, K <= 1024],  W_g [K, N_g] row-major,
// for up to three groups that share x (Q, K and V in one launch). prologue: none, or LayerNorm
// with mt_layernorm_fw's formula; epilogue: (+ bias) -> (GELU_tanh, mt_bias_gelu_fw's formula)
// -> (+ residual). fp32 throughout, products on v_mfma_f32_16x16x4_f32.
//
// Work split: over N only. A workgroup owns 64 output columns of one group and all M rows, so
// every element of W leaves HBM once; x is tiny and L2-resident and every workgroup normalises
// it for itself (row statistics included) rather than pay a launch for it.
//
// One wave, one k-step (4 rows of W): lane (j = lane & 15, q = lane >> 4) loads the 16 bytes
// W[k0 + q][n0 + 4j .. + 3]: four 256-byte row segments per wave instruction. Component c of that
// float4 is the B operand of MFMA c (B[k = q][col = j]), whose 16 columns are n0 + 4j + c: the
// four MFMAs of a k-step cover the 64 columns, and the accumulators of a lane, acc[c][r], are
// out[row 4q + r][n0 + 4j + c]: four adjacent columns per row, a 16-byte LDS write. The A operand
// of all four is x[row j][k0 + q], one ds_read_b32 from the wave's staged slice. Up to four row
// blocks of 16 rows (RB) reuse the W fragment: 4 RB MFMAs per 16-byte load and lane.
//
// K split: with K % 16 == 0 the workgroup has four waves (KS = 4) and wave w owns the contiguous
// k range [w K/4, (w + 1) K/4); otherwise one wave owns all of K (KS = 1). A wave walks its
// range in ascending order in chunks of 32 rows: the next chunk's W loads are issued (8 x 16 B per
// lane in flight) before the current chunk's x slice is staged and multiplied. The waves'
// partial tiles meet in LDS and wave 0 adds them as ((p0 + p1) + p2) + p3; then all threads run
// the epilogue on the summed tile, 16 bytes per thread and access where N and the pointers
// allow, else element by element with the same values.
//
// Determinism and row independence: no atomics; the tile width (64) and KS depend on K alone,
// the chunking on nothing; a row's dot product is one MFMA accumulation chain per wave in
// ascending k, untouched by the other rows of its block (D[i][j] reads row i of A only), and the
// row statistics are one wave's fixed shuffle tree over that row. So the bits of out row m are a
// function of x row m, the residual row, the weights and (K, N): not of M, of m, of the group
// count or of which epilogue stages are on.
#include "../../include/minitorch_hip.h"
#include "fa_common.h"
#include "silu.h"
#include <type_traits>

namespace mt {
int set_error(const char* fmt, ...);           // capi_flash.hip
int check_hip(hipError_t e, const char* where);

namespace lr {
constexpr int kTile = 64;        // output columns per workgroup
constexpr int kChunk = 32;       // k rows a wave stages and multiplies at a time
constexpr int kSteps = kChunk / 4;
constexpr int kXStride = kChunk + 4;  // LDS row stride of a staged x slice (16-B aligned rows)
constexpr int kMaxM = 64, kMaxK = 1024, kMaxG = 3;
constexpr float kLnEps = 1e-8f;  // mt_layernorm_fw's

typedef float f32x4v __attribute__((ext_vector_type(4)));

struct Args {
  const float* x;
  const float* gamma;  // NULL: no LayerNorm
  const float* beta;
  const float* W[kMaxG];
  const float* bias[kMaxG];  // NULL: none
  const float* res[kMaxG];   // NULL: none
  float* out[kMaxG];
  int64_t N[kMaxG];
  int64_t ldx;
  int tile_end[kMaxG];  // running count of column tiles through group g
  int M, K;
  int gelu;  // bit g: GELU in group g's epilogue
  int vec;   // bit g: bias_g, residual_g and out_g take 16-B accesses (W: the kernel's VEC)
  // read by the EXT instantiations only (mt_linear_rows_ex)
  int glu;   // bit g: group g is gated (W_g [K, 2 N_g], a tile is 32 gate + 32 up columns)
  int rms;   // gamma scales x * rstd (RMSNorm: no mean, beta unused)
  float eps;
};

// the group's fields by comparison, never by a runtime index into the by-value struct (which
// would put it in scratch)
template <typename T> __device__ __forceinline__ T pick(const T (&v)[kMaxG], int g) {
  return g == 0 ? v[0] : (g == 1 ? v[1] : v[2]);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// mt_bias_gelu_fw's GELU (combine.hip gelu_tanh), operation for operation
__device__ __forceinline__ float gelu_tanh(float u) {
#pragma clang fp contract(off)
  constexpr float k = 0.7978845608028654f;  // sqrt(2 / pi)
  const float u2 = u * u;
  const float t = tanhf(k * fmaf(0.044715f, u2 * u, u));
  return (0.5f * u) * (1.f + t);
}

// 4 columns of W row k from column col on (col % 4 == 0). No branch and no mask: a row >= K or a
// column >= N is replaced by one inside, so the number of loads in flight is the same on every
// path and a wait for an older load leaves the younger ones outstanding. What such a lane loads
// is never used: a k-step past the wave's range is not multiplied, and an output column reads
// its own column of W only, columns >= N being dropped by the epilogue.
template <bool VEC>
__device__ __forceinline__ float4 load_w(const float* __restrict__ W, int64_t N, int K, int k, int64_t col) {
  const float* row = W + (int64_t)min(k, K - 1) * N;
  if (VEC) return *(const float4*)(row + (col < N ? col : 0));  // N % 4 == 0: the four columns are inside together
  float e[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) e[i] = row[col + i < N ? col + i : 0];
  return make_float4(e[0], e[1], e[2], e[3]);
}
// The same for a row of ld elements whose half starting at element `half` (0, or N of a gated
// group: the up columns) holds the N columns addressed by col.
template <bool VEC>
__device__ __forceinline__ float4 load_w_half(const float* __restrict__ W, int64_t ld, int64_t half, int64_t N, int K,
                                              int k, int64_t col) {
  const float* row = W + (int64_t)min(k, K - 1) * ld + half;
  if (VEC) return *(const float4*)(row + (col < N ? col : 0));  // N % 4 == 0, so half % 4 == 0 too
  float e[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) e[i] = row[col + i < N ? col + i : 0];
  return make_float4(e[0], e[1], e[2], e[3]);
}

// RB row blocks of 16 rows (M <= 16 RB), KS waves that split K, VEC: 16-byte loads of W.
// EXT (mt_linear_rows_ex with RMSNorm, a gated group or an eps of its own): the same body with
//  * the prologue's variance term E[x^2] + eps without the mean (a.rms), or LayerNorm's with a.eps;
//  * gated groups (a.glu bit g): W_g is [K, 2 N], the workgroup's 64 tile columns are the 32 gate
//    columns n0 .. n0 + 31 (lanes j < 8) and the 32 up columns N + n0 .. (lanes j >= 8) of the same
//    row of W, so the K loop, the accumulators (acc[rb][c] of lane j: tile columns 4 j + c) and the
//    K-split combine are untouched; the epilogue pairs column c of the summed tile with column
//    c + 32: out[r][n0 + c] = silu(t[r][c] + bias[n0 + c]) * (t[r][c + 32] + bias[N + n0 + c])
//    (+ residual), 8 threads of 4 columns per row.
// Without EXT every EXT branch is compiled out: mt_linear_rows' instantiations are the ones
// they were.
template <int RB, int KS, bool VEC, bool EXT>
__global__ __launch_bounds__(64 * KS) void linear_rows_kernel(const Args a) {
  constexpr int ROWS = 16 * RB;
  constexpr int SLOTS = KS > 1 ? KS - 1 : 1;  // partial tiles of waves 1.., slot 0 then the sum
  constexpr int XS = KS * ROWS * kXStride, PS = SLOTS * ROWS * kTile;
  __shared__ __attribute__((aligned(16))) float smem[XS > PS ? XS : PS];
  __shared__ float stat[ROWS][2];  // mean, 1 / sqrt(var)

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int tile = blockIdx.x;
  const int g = (tile >= a.tile_end[0]) + (tile >= a.tile_end[1]);
  const int tile0 = g == 0 ? 0 : (g == 1 ? a.tile_end[0] : a.tile_end[1]);
  const float* __restrict__ W = pick(a.W, g);
  const int64_t N = pick(a.N, g);
  const bool glu = EXT && ((a.glu >> g) & 1);
  const int64_t n0 = (int64_t)(tile - tile0) * (glu ? kTile / 2 : kTile);
  // this lane's 4 columns of W: of a gated group, gate columns for j < 8 and up columns above
  const int64_t ldw = glu ? 2 * N : N, whalf = glu && j >= 8 ? N : 0;
  const int64_t wcol = glu ? n0 + 4 * (j & 7) : n0 + 4 * j;
  const int M = a.M, K = a.K;
  auto load = [&](int k) {
    if constexpr (EXT) return load_w_half<VEC>(W, ldw, whalf, N, K, k, wcol);
    else return load_w<VEC>(W, N, K, k, n0 + 4 * j);
  };
  const int S = K / KS;           // this wave's k rows: [wave S, wave S + S)
  const int kw = wave * S;
  const int nch = (S + kChunk - 1) / kChunk;
  const bool ln = a.gamma != nullptr;
  const bool rms = EXT && a.rms;  // RMSNorm: the same staging with mean 0 and no beta

  // the first chunk's W rows are on their way while the statistics are computed
  float4 wa[kSteps], wb[kSteps];
#pragma unroll
  for (int s = 0; s < kSteps; ++s) wa[s] = load(kw + 4 * s + q);

  if (ln) {
    // one wave per row, ln_fw_vec's sums: (x + y) + (z + w) per lane and 256 columns, then the
    // wave tree; four rows' loads are in flight together. A lane past the row's end loads the
    // row's first columns again and weighs them 0 (no branch between the loads).
    for (int r0 = wave; r0 < M; r0 += 4 * KS) {
      float4 v[4][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float* xr = a.x + (int64_t)min(r0 + u * KS, M - 1) * a.ldx;
#pragma unroll
        for (int t = 0; t < 4; ++t) v[u][t] = *(const float4*)(xr + (4 * lane + 256 * t < K ? 4 * lane + 256 * t : 0));
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float s = 0.f, ss = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float in = 4 * lane + 256 * t < K ? 1.f : 0.f;
          const float4 e = v[u][t];
          s += in * ((e.x + e.y) + (e.z + e.w));
          ss += in * ((e.x * e.x + e.y * e.y) + (e.z * e.z + e.w * e.w));
        }
        s = wave_sum(s);
        ss = wave_sum(ss);
        const float mean = rms ? 0.f : s / (float)K;
        const float var = rms ? ss / (float)K + a.eps : ss / (float)K - mean * mean + (EXT ? a.eps : kLnEps);
        const int r = r0 + u * KS;
        if (lane == 0 && r < M) { stat[r][0] = mean; stat[r][1] = 1.f / sqrtf(var); }
      }
    }
    __syncthreads();
  }

  f32x4v acc[RB][4];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[rb][c] = f32x4v{0.f, 0.f, 0.f, 0.f};

  float* xs = smem + wave * ROWS * kXStride;  // this wave's slice [ROWS][kXStride]
  const int xr = lane >> 3, xc = 4 * (lane & 7);  // staging: 8 lanes per row, 8 rows per pass
  // One chunk. PF: the next chunk's W rows are loaded meanwhile (every chunk but the last). The
  // loads of a chunk are the same in number on every path (the two of gamma / beta read x when
  // there is no LayerNorm), so the wait for the x rows is a count that leaves W in flight.
  auto chunk = [&](int ch, auto pf) {
    const int kb = kw + ch * kChunk;                 // first k row of the chunk
    const int cw = min(kChunk, S - ch * kChunk);     // its rows (a multiple of 4)
    // the chunk's x rows first, the next chunk's W rows behind them: the wait for x leaves those
    // in flight. Rows >= M and columns >= cw are staged as zero (loaded from a valid address).
    const bool cok = xc < cw;
    const int kx = cok ? kb + xc : kb;
    float4 xv[ROWS / 8];
#pragma unroll
    for (int p = 0; p < ROWS / 8; ++p)
      xv[p] = *(const float4*)(a.x + (int64_t)min(8 * p + xr, M - 1) * a.ldx + kx);
    const float4 gm = *(const float4*)((ln ? a.gamma : a.x) + kx), bt = *(const float4*)((ln && !rms ? a.beta : a.x) + kx);
    if constexpr (decltype(pf)::value) {
#pragma unroll
      for (int s = 0; s < kSteps; ++s) wb[s] = load(kb + kChunk + 4 * s + q);
    }
#pragma unroll
    for (int p = 0; p < ROWS / 8; ++p) {
      const int r = 8 * p + xr;
      if (rms) {
        const float rsd = stat[min(r, M - 1)][1];
        xv[p] = make_float4(gm.x * (xv[p].x * rsd), gm.y * (xv[p].y * rsd), gm.z * (xv[p].z * rsd), gm.w * (xv[p].w * rsd));
      } else if (ln) {
        const float mean = stat[min(r, M - 1)][0], rsd = stat[min(r, M - 1)][1];
        xv[p] = make_float4(gm.x * ((xv[p].x - mean) * rsd) + bt.x, gm.y * ((xv[p].y - mean) * rsd) + bt.y,
                            gm.z * ((xv[p].z - mean) * rsd) + bt.z, gm.w * ((xv[p].w - mean) * rsd) + bt.w);
      }
      if (!(r < M && cok)) xv[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();  // the previous chunk's reads of the slices are done
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
  __syncthreads();  // every wave is done with the x slices: smem becomes the partial tiles

  // lane (j, q), block rb, register r: row 16 rb + 4 q + r, columns 4 j .. 4 j + 3
  auto slot_at = [&](int slot, int rb, int r) { return smem + (slot * ROWS + 16 * rb + 4 * q + r) * kTile + 4 * j; };
  if (KS > 1 && wave > 0) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        *(float4*)slot_at(wave - 1, rb, r) = make_float4(acc[rb][0][r], acc[rb][1][r], acc[rb][2][r], acc[rb][3][r]);
  }
  if (KS > 1) __syncthreads();
  if (wave == 0) {  // ((p0 + p1) + p2) + p3, then the sum into slot 0 (this lane's own addresses)
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

  // epilogue: 4 columns per thread and pass over the M real rows of the summed tile
  const float* __restrict__ bias = pick(a.bias, g);
  const float* __restrict__ res = pick(a.res, g);
  float* __restrict__ out = pick(a.out, g);
  const bool gelu = (a.gelu >> g) & 1, vec_io = (a.vec >> g) & 1;
  if (glu) {  // 4 gate columns and their 4 up columns per thread and pass
    for (int i = threadIdx.x; i < M * (kTile / 8); i += 64 * KS) {
      const int r = i >> 3, c = 4 * (i & 7);
      const int64_t col = n0 + c;
      if (col >= N) continue;
      const float4 ta = *(const float4*)(smem + r * kTile + c), tb = *(const float4*)(smem + r * kTile + kTile / 2 + c);
      float va[4] = {ta.x, ta.y, ta.z, ta.w}, vb[4] = {tb.x, tb.y, tb.z, tb.w};
      const int64_t o = (int64_t)r * N + col;
      if (vec_io) {
        if (bias) {
          const float4 ba = *(const float4*)(bias + col), bb = *(const float4*)(bias + N + col);
          va[0] += ba.x; va[1] += ba.y; va[2] += ba.z; va[3] += ba.w;
          vb[0] += bb.x; vb[1] += bb.y; vb[2] += bb.z; vb[3] += bb.w;
        }
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = silu(va[e]) * vb[e];
        if (res) { const float4 b = *(const float4*)(res + o); v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w; }
        *(float4*)(out + o) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (col + e < N) {
            float ua = va[e], ub = vb[e];
            if (bias) { ua += bias[col + e]; ub += bias[N + col + e]; }
            float u = silu(ua) * ub;
            if (res) u += res[o + e];
            out[o + e] = u;
          }
        }
      }
    }
    return;
  }
  for (int i = threadIdx.x; i < M * (kTile / 4); i += 64 * KS) {
    const int r = i >> 4;
    const int64_t col = n0 + 4 * (i & 15);
    if (col >= N) continue;
    const float4 t = *(const float4*)(smem + r * kTile + 4 * (i & 15));
    float v[4] = {t.x, t.y, t.z, t.w};
    const int64_t o = (int64_t)r * N + col;
    if (vec_io) {  // N % 4 == 0 and 16-B aligned bias / residual / out: the four columns are inside
      if (bias) { const float4 b = *(const float4*)(bias + col); v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w; }
      if (gelu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = gelu_tanh(v[e]);
      }
      if (res) { const float4 b = *(const float4*)(res + o); v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w; }
      *(float4*)(out + o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (col + e < N) {
          float u = v[e];
          if (bias) u += bias[col + e];
          if (gelu) u = gelu_tanh(u);
          if (res) u += res[o + e];
          out[o + e] = u;
        }
      }
    }
  }
}

template <int RB, int KS>
static void launch(const Args& a, int tiles, bool vec, bool ext, hipStream_t st) {
  if (ext) {
    if (vec) hipLaunchKernelGGL((linear_rows_kernel<RB, KS, true, true>), dim3(tiles), dim3(64 * KS), 0, st, a);
    else hipLaunchKernelGGL((linear_rows_kernel<RB, KS, false, true>), dim3(tiles), dim3(64 * KS), 0, st, a);
  } else {
    if (vec) hipLaunchKernelGGL((linear_rows_kernel<RB, KS, true, false>), dim3(tiles), dim3(64 * KS), 0, st, a);
    else hipLaunchKernelGGL((linear_rows_kernel<RB, KS, false, false>), dim3(tiles), dim3(64 * KS), 0, st, a);
  }
}

static bool overlap(const void* p, int64_t pbytes, const void* r, int64_t rbytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)r;
  return a < b + (uintptr_t)rbytes && b < a + (uintptr_t)pbytes;
}
}  // namespace lr
}  // namespace mt

using namespace mt;
using namespace mt::lr;

// Both entries: fn names the caller in the messages. norm: 0 none, 1 LayerNorm, 2 RMSNorm.
static int run(const char* fn, int G, const float* x, int64_t ldx, int64_t M, int64_t K, int norm, const float* gamma,
               const float* beta, float eps, const float* const* W, const int64_t* N, const float* const* bias,
               const float* const* residual, float* const* out, int gelu_mask, int glu_mask, void* stream) {
  if (G < 1 || G > kMaxG) return set_error("%s: G=%d is outside 1..%d", fn, G, kMaxG);
  if (M < 1 || M > kMaxM)
    return set_error("%s: M=%lld is outside 1..%d (the skinny kernel; use mt_matmul_f32)", fn, (long long)M, kMaxM);
  if (K < 4 || K > kMaxK || K % 4)
    return set_error("%s: K=%lld must be a multiple of 4 in 4..%d", fn, (long long)K, kMaxK);
  if (!x) return set_error("%s: x is NULL", fn);
  if (ldx < K || ldx % 4) return set_error("%s: ldx=%lld must be a multiple of 4 and >= K", fn, (long long)ldx);
  if (!W || !N || !out) return set_error("%s: the W, N or out array is NULL", fn);
  if (norm < 0 || norm > 2) return set_error("%s: norm=%d is outside 0..2 (none, LayerNorm, RMSNorm)", fn, norm);
  if (norm == 0 && (gamma || beta)) return set_error("%s: norm=0 takes no gamma and no beta", fn);
  if (norm == 1 && (!gamma || !beta)) return set_error("%s: gamma and beta are NULL together or not at all", fn);
  if (norm == 2 && !gamma) return set_error("%s: RMSNorm (norm=2) needs gamma", fn);
  if (norm == 2 && beta) return set_error("%s: RMSNorm (norm=2) has no beta", fn);
  if (norm && !(eps >= 0.f)) return set_error("%s: eps=%g is negative", fn, (double)eps);
  if ((uintptr_t)x & 15) return set_error("%s: x is misaligned (16 bytes)", fn);
  if (((uintptr_t)gamma | (uintptr_t)beta) & 15) return set_error("%s: gamma / beta are misaligned (16 bytes)", fn);
  if (gelu_mask < 0 || gelu_mask >> G) return set_error("%s: gelu_mask=%d names a group >= G=%d", fn, gelu_mask, G);
  if (glu_mask < 0 || glu_mask >> G) return set_error("%s: glu_mask=%d names a group >= G=%d", fn, glu_mask, G);
  if (gelu_mask & glu_mask)
    return set_error("%s: gelu_mask=%d and glu_mask=%d share a group (GELU or the gate, not both)", fn, gelu_mask, glu_mask);

  Args a = {};
  a.x = x; a.gamma = gamma; a.beta = beta; a.ldx = ldx; a.M = (int)M; a.K = (int)K; a.gelu = gelu_mask;
  a.glu = glu_mask; a.rms = norm == 2; a.eps = eps;
  const int64_t xbytes = ((M - 1) * ldx + K) * 4;
  int64_t tiles = 0;
  bool vec_all = true;
  for (int g = 0; g < G; ++g) {
    const bool glu = (glu_mask >> g) & 1;
    // a gated group's row of W holds 2 N_g columns
    if (N[g] < 1 || N[g] > ((1ll << 31) - kTile) / (glu ? 2 : 1))
      return set_error("%s: N[%d]=%lld is outside 1..%s", fn, g, (long long)N[g], glu ? "2^30-32 (gated)" : "2^31-64");
    if (!W[g]) return set_error("%s: W[%d] is NULL", fn, g);
    if (!out[g]) return set_error("%s: out[%d] is NULL", fn, g);
    const float* b = bias ? bias[g] : nullptr;
    const float* r = residual ? residual[g] : nullptr;
    if (((uintptr_t)W[g] | (uintptr_t)out[g] | (uintptr_t)b | (uintptr_t)r) & 3)
      return set_error("%s: a pointer of group %d is misaligned (4 bytes)", fn, g);
    const int64_t obytes = M * N[g] * 4;
    if (overlap(out[g], obytes, x, xbytes)) return set_error("%s: out[%d] overlaps x", fn, g);
    for (int h = 0; h < G; ++h) {
      const float* rh = residual ? residual[h] : nullptr;
      if (rh && overlap(out[g], obytes, rh, M * N[h] * 4))
        return set_error("%s: out[%d] overlaps residual[%d]", fn, g, h);
      if (h < g && overlap(out[g], obytes, out[h], M * N[h] * 4))
        return set_error("%s: out[%d] overlaps out[%d]", fn, g, h);
    }
    a.W[g] = W[g]; a.N[g] = N[g]; a.bias[g] = b; a.res[g] = r; a.out[g] = out[g];
    // (N % 4 == 0 keeps a gated group's up half, N elements into the row and into the bias, aligned)
    const bool vw = N[g] % 4 == 0 && !((uintptr_t)W[g] & 15);
    const bool vio = N[g] % 4 == 0 && !(((uintptr_t)out[g] | (uintptr_t)b | (uintptr_t)r) & 15);
    vec_all = vec_all && vw;
    a.vec |= (vio ? 1 : 0) << g;
    const int width = glu ? kTile / 2 : kTile;  // output columns per workgroup
    tiles += (N[g] + width - 1) / width;
    if (tiles > (1ll << 30)) return set_error("%s: too many column tiles", fn);
    a.tile_end[g] = (int)tiles;
  }
  for (int g = G; g < kMaxG; ++g) a.tile_end[g] = 0x7fffffff;

  const int ks = K % 16 == 0 ? 4 : 1;  // the plan: a function of K alone (the tile is 64 columns always)
  const hipStream_t st = (hipStream_t)stream;
  const int rb = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
  // What mt_linear_rows can ask for runs on the instantiations it always had, whichever entry asks.
  const bool ext = norm == 2 || glu_mask != 0 || (norm == 1 && eps != kLnEps);
  // 16-byte loads of W in a launch where every group allows them (a property of N and the pointers)
  if (ks == 4) {
    if (rb == 1) launch<1, 4>(a, (int)tiles, vec_all, ext, st);
    else if (rb == 2) launch<2, 4>(a, (int)tiles, vec_all, ext, st);
    else launch<4, 4>(a, (int)tiles, vec_all, ext, st);
  } else {
    if (rb == 1) launch<1, 1>(a, (int)tiles, vec_all, ext, st);
    else if (rb == 2) launch<2, 1>(a, (int)tiles, vec_all, ext, st);
    else launch<4, 1>(a, (int)tiles, vec_all, ext, st);
  }
  return check_hip(hipGetLastError(), fn);
}

extern "C" int mt_linear_rows_ex(int G, const float* x, int64_t ldx, int64_t M, int64_t K, int norm, const float* gamma,
                                 const float* beta, float eps, const float* const* W, const int64_t* N,
                                 const float* const* bias, const float* const* residual, float* const* out,
                                 int gelu_mask, int glu_mask, void* stream) {
  return run("mt_linear_rows_ex", G, x, ldx, M, K, norm, gamma, beta, eps, W, N, bias, residual, out, gelu_mask,
             glu_mask, stream);
}

extern "C" int mt_linear_rows(int G, const float* x, int64_t ldx, int64_t M, int64_t K, const float* gamma,
                              const float* beta, const float* const* W, const int64_t* N,
                              const float* const* bias, const float* const* residual, float* const* out,
                              int gelu_mask, void* stream) {
  if ((gamma == nullptr) != (beta == nullptr))
    return set_error("mt_linear_rows: gamma and beta are NULL together or not at all");
  return run("mt_linear_rows", G, x, ldx, M, K, gamma ? 1 : 0, gamma, beta, kLnEps, W, N, bias, residual, out, gelu_mask,
             0, stream);
}
