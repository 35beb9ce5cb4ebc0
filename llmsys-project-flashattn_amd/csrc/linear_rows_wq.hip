// Weight-only quantised skinny linear (include/minitorch_hip.h, "weight-only quantised linear"):
// mt_linear_rows_ex's contract with the weights stored as bf16, fp8 (e4m3, a scale per column) or
// int4 (a scale per column and 32 rows of K), plus the one-off kernels that write and read that
// storage. Activations, arithmetic and outputs stay fp32; products on v_mfma_f32_16x16x4_f32.
//
// Storage: tile-major, [column tile of 64][k block][64 lanes][16 B]. Lane
// (j = lane & 15, q = lane >> 4) owns, as in linear_rows.hip, the tile columns 4 j .. 4 j + 3 of the
// rows k0 + 4 s + q; its 16 bytes of a k block hold those four columns for kRows / 4 consecutive
// k-steps s (element 4 s + c, little endian: bf16 2 steps, fp8 4, int4 8), so a wave instruction
// reads 1 KB contiguous and a chunk of 32 rows is 4, 2 or 1 loads per lane in place of 8. Every
// tile is whole: columns >= N are zero codes, so no load needs a clamp or a branch. A gated
// group's tile is 32 gate columns then the 32 up columns beside them, as the fp32 kernel sees it.
//
// The hot kernel keeps the fp32 kernel's work split (a workgroup per 64 tile columns, four waves
// over K, wave w the rows [w K/4, (w + 1) K/4) in ascending chunks of 32) and its prologue and
// epilogue operation for operation; the codes are widened in registers to W' (shift; cvt_pk and
// one product by the column scale; nibble -> int -> float and one product by the group scale)
// right before the MFMA that takes them. One accumulation chain per wave in ascending k and
// ((p0 + p1) + p2) + p3 over the waves: the output has the bits of mt_linear_rows_ex on W'.
#include "../../include/minitorch_hip.h"
#include "fa_common.h"
#include "silu.h"
#include <type_traits>

namespace mt {
int set_error(const char* fmt, ...);           // capi_flash.hip
int check_hip(hipError_t e, const char* where);

namespace lrq {
constexpr int kTile = 64;        // tile columns per workgroup
constexpr int kChunk = 32;       // k rows a wave stages and multiplies at a time
constexpr int kSteps = kChunk / 4;
constexpr int kXStride = kChunk + 4;
constexpr int kMaxM = 64, kMaxK = 1024, kMaxG = 3, kKMul = 128, KS = 4;

typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef float f32x2v __attribute__((ext_vector_type(2)));

// rows of K in a lane's 16-byte load
template <int FMT> struct Fmt;
template <> struct Fmt<MT_W_BF16> { static constexpr int kRows = 8, kBits = 16; };
template <> struct Fmt<MT_W_FP8> { static constexpr int kRows = 16, kBits = 8; };
template <> struct Fmt<MT_W_INT4> { static constexpr int kRows = 32, kBits = 4; };

__device__ __forceinline__ uint32_t word(const uint4& v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }

// the stored code of k-step s (within the load), column c: bf16 bits, an e4m3 byte, or the int4 value
template <int FMT> __device__ __forceinline__ int code_of(const uint4& raw, int s, int c) {
  constexpr int B = Fmt<FMT>::kBits;
  const int bit = (4 * s + c) * B;
  const uint32_t w = word(raw, bit >> 5);
  if constexpr (FMT == MT_W_INT4) return (int)(w << (28 - (bit & 31))) >> 28;  // two's-complement nibble
  return (int)((w >> (bit & 31)) & ((1u << B) - 1u));
}

// W' of k-step s (within the load): the four columns' codes widened and scaled (sc: the columns'
// scales, unused for bf16). One fp32 product per element, mt_weight_dequant's.
template <int FMT> __device__ __forceinline__ void widen(const uint4& raw, int s, const float (&sc)[4], float (&w)[4]) {
  if constexpr (FMT == MT_W_FP8) {
    const uint32_t u = word(raw, s);
    const f32x2v lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)u, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)u, true);
    w[0] = lo.x * sc[0]; w[1] = lo.y * sc[1]; w[2] = hi.x * sc[2]; w[3] = hi.y * sc[3];
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if constexpr (FMT == MT_W_BF16) w[c] = __uint_as_float((uint32_t)code_of<FMT>(raw, s, c) << 16);
      else w[c] = (float)code_of<FMT>(raw, s, c) * sc[c];
    }
  }
}

// Column of W ([K, N], or [K, 2 N] gated) behind tile column tc of column tile `tile`, -1 for padding
__device__ __forceinline__ int64_t w_column(int64_t tile, int tc, int64_t N, bool glu) {
  if (glu) {
    const int64_t col = tile * (kTile / 2) + (tc & 31);
    return col < N ? (tc >= 32 ? N + col : col) : -1;
  }
  const int64_t col = tile * kTile + tc;
  return col < N ? col : -1;
}

struct Args {
  const float* x;
  const float* gamma;  // NULL: no norm
  const float* beta;
  const uint4* W[kMaxG];      // packed codes
  const float* scale[kMaxG];  // fp8 [ncols], int4 [K / 32, ncols]
  const float* bias[kMaxG];
  const float* res[kMaxG];
  float* out[kMaxG];
  int64_t N[kMaxG];
  int64_t ldx;
  int tile_end[kMaxG];
  int M, K;
  int gelu, vec, glu, rms;  // linear_rows.hip's Args
  float eps;
};

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

// RB row blocks of 16 rows (M <= 16 RB). The statistics, the staging of x, the K-split combine and
// the epilogue are linear_rows_kernel<RB, 4, *, true>'s, statement for statement (K % 128 == 0, so
// every chunk is whole and its masks are gone); the W side is this file's.
template <int FMT, int RB>
__global__ __launch_bounds__(64 * KS) void linear_rows_wq_kernel(const Args a) {
  constexpr int ROWS = 16 * RB;
  constexpr int R = Fmt<FMT>::kRows, L = kChunk / R, SPL = R / 4;  // loads per chunk, k-steps per load
  constexpr int XS = KS * ROWS * kXStride, PS = (KS - 1) * ROWS * kTile;
  __shared__ __attribute__((aligned(16))) float smem[XS > PS ? XS : PS];
  __shared__ float stat[ROWS][2];  // mean, 1 / sqrt(var)

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int tile = blockIdx.x;
  const int g = (tile >= a.tile_end[0]) + (tile >= a.tile_end[1]);
  const int tile0 = g == 0 ? 0 : (g == 1 ? a.tile_end[0] : a.tile_end[1]);
  const int64_t N = pick(a.N, g);
  const bool glu = (a.glu >> g) & 1;
  const int64_t n0 = (int64_t)(tile - tile0) * (glu ? kTile / 2 : kTile);
  const int M = a.M, K = a.K;
  const int S = K / KS;  // this wave's k rows: [wave S, wave S + S), a multiple of 32
  const int kw = wave * S;
  const int nch = S / kChunk;
  const bool ln = a.gamma != nullptr;
  const bool rms = a.rms;

  // this lane's 16 bytes of the wave's first k block of the tile; block b is 64 uint4 further on
  const uint4* __restrict__ Wl = pick(a.W, g) + ((int64_t)(tile - tile0) * (K / R) + kw / R) * 64 + lane;
  // the scales of the lane's four columns (a padding column takes column 0's: its product is dropped)
  const float* __restrict__ scale = pick(a.scale, g);
  const int64_t ncols = glu ? 2 * N : N;
  int64_t scol[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int64_t col = w_column(tile - tile0, 4 * j + c, N, glu);
    scol[c] = col < 0 ? 0 : col;
  }
  uint4 wa[L], wb[L];
  float sa[4] = {1.f, 1.f, 1.f, 1.f}, sb[4] = {1.f, 1.f, 1.f, 1.f};
  auto load = [&](int ch, uint4 (&w)[L], float (&sc)[4]) {
#pragma unroll
    for (int l = 0; l < L; ++l) w[l] = Wl[(int64_t)(ch * L + l) * 64];
    if constexpr (FMT == MT_W_INT4) {  // the chunk is one scale group: row kw / 32 + ch of [K / 32, ncols]
#pragma unroll
      for (int c = 0; c < 4; ++c) sc[c] = scale[(int64_t)(kw / kChunk + ch) * ncols + scol[c]];
    }
  };
  // the first chunk's codes are on their way while the statistics are computed
  load(0, wa, sa);
  if constexpr (FMT == MT_W_FP8) {  // loop-invariant
#pragma unroll
    for (int c = 0; c < 4; ++c) sa[c] = scale[scol[c]];
  }

  if (ln) {
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
        const float var = rms ? ss / (float)K + a.eps : ss / (float)K - mean * mean + a.eps;
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
  // One chunk. PF: the next chunk's codes (and int4 scales) are loaded behind the chunk's x rows and
  // stay in flight under its arithmetic.
  auto chunk = [&](int ch, auto pf) {
    const int kx = kw + ch * kChunk + xc;
    float4 xv[ROWS / 8];
#pragma unroll
    for (int p = 0; p < ROWS / 8; ++p)
      xv[p] = *(const float4*)(a.x + (int64_t)min(8 * p + xr, M - 1) * a.ldx + kx);
    const float4 gm = *(const float4*)((ln ? a.gamma : a.x) + kx), bt = *(const float4*)((ln && !rms ? a.beta : a.x) + kx);
    if constexpr (decltype(pf)::value) load(ch + 1, wb, sb);
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
      if (!(r < M)) xv[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();  // the previous chunk's reads of the slices are done
#pragma unroll
    for (int p = 0; p < ROWS / 8; ++p) *(float4*)(xs + (8 * p + xr) * kXStride + xc) = xv[p];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      float w4[4];
      widen<FMT>(wa[s / SPL], s % SPL, sa, w4);
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const float av = xs[(16 * rb + j) * kXStride + 4 * s + q];
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[rb][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w4[c], acc[rb][c], 0, 0, 0);
      }
    }
    if constexpr (decltype(pf)::value) {
#pragma unroll
      for (int l = 0; l < L; ++l) wa[l] = wb[l];
      if constexpr (FMT == MT_W_INT4) {
#pragma unroll
        for (int c = 0; c < 4; ++c) sa[c] = sb[c];
      }
    }
  };
  for (int ch = 0; ch + 1 < nch; ++ch) chunk(ch, std::true_type{});
  chunk(nch - 1, std::false_type{});
  __syncthreads();  // every wave is done with the x slices: smem becomes the partial tiles

  // lane (j, q), block rb, register r: row 16 rb + 4 q + r, columns 4 j .. 4 j + 3
  auto slot_at = [&](int slot, int rb, int r) { return smem + (slot * ROWS + 16 * rb + 4 * q + r) * kTile + 4 * j; };
  if (wave > 0) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        *(float4*)slot_at(wave - 1, rb, r) = make_float4(acc[rb][0][r], acc[rb][1][r], acc[rb][2][r], acc[rb][3][r]);
  }
  __syncthreads();
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

// ---- the one-off kernels: pack fp32 W into the storage, and unpack it ------------------------
struct PackArgs {
  const float* W;   // quant: the fp32 source [K, ldw]
  int64_t ldw;
  uint4* codes;
  float* scales;
  float* out;       // dequant: W' [K, ncols]
  void* codes_out;  // dequant: the codes [K, ncols] (uint16 / uint8 / int8), or NULL
  int64_t N;
  int K, glu;
};

__device__ __forceinline__ uint32_t bf16_rne(float x) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;  // NaN stays NaN
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// A workgroup per column tile, a wave per k block (blocks wave, wave + 4, ...: K / kRows is a
// multiple of 4, so the four waves make the same number of trips), a lane per 16 bytes it will
// later load. fp8: the column maxima first, four partial maxima per column over interleaved rows
// combined as max(max(p0, p1), max(p2, p3)). int4: a group's 32 rows of a column sit in the four
// q lanes of its j, eight each, combined by two xor shuffles. No atomics.
template <int FMT>
__global__ __launch_bounds__(256) void weight_quant_kernel(const PackArgs a) {
  constexpr int R = Fmt<FMT>::kRows, SPL = R / 4;
  __shared__ float part[4][kTile];
  __shared__ int partbad[4][kTile];
  __shared__ float colscale[kTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4;
  const int64_t tile = blockIdx.x, N = a.N, ncols = a.glu ? 2 * N : N;
  const int K = a.K;
  if constexpr (FMT == MT_W_FP8) {
    const int64_t col = w_column(tile, lane, N, a.glu);
    float am = 0.f;
    int bad = 0;
    for (int k = wave; k < K; k += 4) {
      const float ax = fabsf(col >= 0 ? a.W[(int64_t)k * a.ldw + col] : 0.f);
      am = fmaxf(am, ax);
      bad |= !(ax <= 3.402823466e38f);  // inf or NaN
    }
    part[wave][lane] = am;
    partbad[wave][lane] = bad;
    __syncthreads();
    if (wave == 0) {
      am = fmaxf(fmaxf(part[0][lane], part[1][lane]), fmaxf(part[2][lane], part[3][lane]));
      bad = partbad[0][lane] | partbad[1][lane] | partbad[2][lane] | partbad[3][lane];
      const float s = bad ? __builtin_nanf("") : (am > 0.f ? am / 448.f : 1.f);
      colscale[lane] = s;
      if (col >= 0) a.scales[col] = s;
    }
    __syncthreads();
  }
  int64_t cols[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) cols[c] = w_column(tile, 4 * j + c, N, a.glu);
  for (int kb = wave; kb < K / R; kb += 4) {
    float v[SPL][4];
#pragma unroll
    for (int s = 0; s < SPL; ++s)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        v[s][c] = cols[c] >= 0 ? a.W[(int64_t)(kb * R + 4 * s + q) * a.ldw + cols[c]] : 0.f;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if constexpr (FMT == MT_W_BF16) {
#pragma unroll
      for (int s = 0; s < SPL; ++s)
#pragma unroll
        for (int c = 0; c < 4; ++c) w[(4 * s + c) >> 1] |= bf16_rne(v[s][c]) << (16 * (c & 1));
    } else if constexpr (FMT == MT_W_FP8) {
      float sc[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) sc[c] = colscale[4 * j + c];
#pragma unroll
      for (int s = 0; s < SPL; ++s) {
        float y[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) y[c] = sc[c] == sc[c] ? fminf(fmaxf(v[s][c] / sc[c], -448.f), 448.f) : 0.f;
        const int t = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
        w[s] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], t, true);
#pragma unroll
        for (int c = 0; c < 4; ++c)  // a non-finite column: NaN codes under its NaN scale
          if (!(sc[c] == sc[c])) w[s] |= 0x7Fu << (8 * c);
      }
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float am = 0.f;
        int bad = 0;
#pragma unroll
        for (int s = 0; s < SPL; ++s) {
          const float ax = fabsf(v[s][c]);
          am = fmaxf(am, ax);
          bad |= !(ax <= 3.402823466e38f);
        }
        am = fmaxf(am, __shfl_xor(am, 16, 64));
        bad |= __shfl_xor(bad, 16, 64);
        am = fmaxf(am, __shfl_xor(am, 32, 64));
        bad |= __shfl_xor(bad, 32, 64);
        const float sc = am > 0.f ? am / 7.f : 1.f;
        if (!bad) {
#pragma unroll
          for (int s = 0; s < SPL; ++s) {
            const int code = (int)fminf(fmaxf(rintf(v[s][c] / sc), -7.f), 7.f);
            w[(4 * s + c) >> 3] |= (uint32_t)(code & 0xF) << (4 * ((4 * s + c) & 7));
          }
        }
        // a group holding a non-finite value: zero codes under a NaN scale
        if (q == 0 && cols[c] >= 0) a.scales[(int64_t)kb * ncols + cols[c]] = bad ? __builtin_nanf("") : sc;
      }
    }
    a.codes[(tile * (K / R) + kb) * 64 + lane] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// The same walk backwards: W' [K, ncols] with widen()'s values, and the codes when asked for.
template <int FMT>
__global__ __launch_bounds__(256) void weight_dequant_kernel(const PackArgs a) {
  constexpr int R = Fmt<FMT>::kRows, SPL = R / 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4;
  const int64_t tile = blockIdx.x, N = a.N, ncols = a.glu ? 2 * N : N;
  const int K = a.K;
  int64_t cols[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) cols[c] = w_column(tile, 4 * j + c, N, a.glu);
  float sc[4] = {1.f, 1.f, 1.f, 1.f};
  if constexpr (FMT == MT_W_FP8) {
#pragma unroll
    for (int c = 0; c < 4; ++c) sc[c] = a.scales[cols[c] < 0 ? 0 : cols[c]];
  }
  for (int kb = wave; kb < K / R; kb += 4) {
    const uint4 raw = a.codes[(tile * (K / R) + kb) * 64 + lane];
    if constexpr (FMT == MT_W_INT4) {
#pragma unroll
      for (int c = 0; c < 4; ++c) sc[c] = a.scales[(int64_t)kb * ncols + (cols[c] < 0 ? 0 : cols[c])];
    }
#pragma unroll
    for (int s = 0; s < SPL; ++s) {
      float w[4];
      widen<FMT>(raw, s, sc, w);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (cols[c] < 0) continue;
        const int64_t o = (int64_t)(kb * R + 4 * s + q) * ncols + cols[c];
        a.out[o] = w[c];
        if (a.codes_out) {
          const int code = code_of<FMT>(raw, s, c);
          if constexpr (FMT == MT_W_BF16) ((uint16_t*)a.codes_out)[o] = (uint16_t)code;
          else if constexpr (FMT == MT_W_FP8) ((uint8_t*)a.codes_out)[o] = (uint8_t)code;
          else ((int8_t*)a.codes_out)[o] = (int8_t)code;
        }
      }
    }
  }
}

template <int FMT> static void launch_rows(const Args& a, int tiles, int rb, hipStream_t st) {
  if (rb == 1) hipLaunchKernelGGL((linear_rows_wq_kernel<FMT, 1>), dim3(tiles), dim3(64 * KS), 0, st, a);
  else if (rb == 2) hipLaunchKernelGGL((linear_rows_wq_kernel<FMT, 2>), dim3(tiles), dim3(64 * KS), 0, st, a);
  else hipLaunchKernelGGL((linear_rows_wq_kernel<FMT, 4>), dim3(tiles), dim3(64 * KS), 0, st, a);
}

static bool overlap(const void* p, int64_t pbytes, const void* r, int64_t rbytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)r;
  return a < b + (uintptr_t)rbytes && b < a + (uintptr_t)pbytes;
}

static int rows_per_load(int fmt) { return fmt == MT_W_BF16 ? 8 : (fmt == MT_W_FP8 ? 16 : 32); }

// what every entry refuses about the storage's shape: 0, or the status of the message set
static int check_shape(const char* fn, int fmt, int64_t K, int64_t N, int glu) {
  if (fmt != MT_W_BF16 && fmt != MT_W_FP8 && fmt != MT_W_INT4)
    return set_error("%s: fmt=%d is not MT_W_BF16, MT_W_FP8 or MT_W_INT4", fn, fmt);
  if (K < kKMul || K > kMaxK || K % kKMul)
    return set_error("%s: K=%lld must be a multiple of %d in %d..%d", fn, (long long)K, kKMul, kKMul, kMaxK);
  if (N < 1 || N > ((1ll << 31) - kTile) / (glu ? 2 : 1))
    return set_error("%s: N=%lld is outside 1..%s", fn, (long long)N, glu ? "2^30-32 (gated)" : "2^31-64");
  return 0;
}

static int64_t tiles_of(int64_t N, int glu) {
  const int width = glu ? kTile / 2 : kTile;
  return (N + width - 1) / width;
}
}  // namespace lrq
}  // namespace mt

using namespace mt;
using namespace mt::lrq;

extern "C" int mt_weight_quant_bytes(int fmt, int64_t K, int64_t N, int glu, int64_t* code_bytes, int64_t* scale_bytes) {
  const char* fn = "mt_weight_quant_bytes";
  if (int e = check_shape(fn, fmt, K, N, glu)) return e;
  if (!code_bytes || !scale_bytes) return set_error("%s: code_bytes or scale_bytes is NULL", fn);
  const int64_t ncols = glu ? 2 * N : N;
  *code_bytes = tiles_of(N, glu) * (K / rows_per_load(fmt)) * 64 * 16;
  *scale_bytes = fmt == MT_W_BF16 ? 0 : (fmt == MT_W_FP8 ? ncols * 4 : (K / 32) * ncols * 4);
  return 0;
}

// the storage pointers of one weight: codes 16-byte aligned, scales (fp8, int4) 4-byte aligned
static int check_storage(const char* fn, int fmt, const void* codes, const float* scales, int g) {
  if (!codes) return set_error("%s: codes[%d] is NULL", fn, g);
  if ((uintptr_t)codes & 15) return set_error("%s: codes[%d] is misaligned (16 bytes)", fn, g);
  if (fmt != MT_W_BF16 && !scales) return set_error("%s: scales[%d] is NULL (fp8 and int4 have scales)", fn, g);
  if ((uintptr_t)scales & 3) return set_error("%s: scales[%d] is misaligned (4 bytes)", fn, g);
  return 0;
}

extern "C" int mt_weight_quant(int fmt, const float* W, int64_t ldw, int64_t K, int64_t N, int glu, void* codes,
                               float* scales, void* stream) {
  const char* fn = "mt_weight_quant";
  if (int e = check_shape(fn, fmt, K, N, glu)) return e;
  if (!W) return set_error("%s: W is NULL", fn);
  if ((uintptr_t)W & 3) return set_error("%s: W is misaligned (4 bytes)", fn);
  if (ldw < (glu ? 2 * N : N)) return set_error("%s: ldw=%lld is below the %lld columns of W", fn, (long long)ldw, (long long)(glu ? 2 * N : N));
  if (int e = check_storage(fn, fmt, codes, scales, 0)) return e;
  PackArgs a = {};
  a.W = W; a.ldw = ldw; a.codes = (uint4*)codes; a.scales = scales; a.N = N; a.K = (int)K; a.glu = glu ? 1 : 0;
  const dim3 grid((unsigned)tiles_of(N, glu));
  const hipStream_t st = (hipStream_t)stream;
  if (fmt == MT_W_BF16) hipLaunchKernelGGL((weight_quant_kernel<MT_W_BF16>), grid, dim3(256), 0, st, a);
  else if (fmt == MT_W_FP8) hipLaunchKernelGGL((weight_quant_kernel<MT_W_FP8>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((weight_quant_kernel<MT_W_INT4>), grid, dim3(256), 0, st, a);
  return check_hip(hipGetLastError(), fn);
}

extern "C" int mt_weight_dequant(int fmt, const void* codes, const float* scales, int64_t K, int64_t N, int glu,
                                 float* W_out, void* codes_out, void* stream) {
  const char* fn = "mt_weight_dequant";
  if (int e = check_shape(fn, fmt, K, N, glu)) return e;
  if (int e = check_storage(fn, fmt, codes, scales, 0)) return e;
  if (!W_out) return set_error("%s: W_out is NULL", fn);
  if ((uintptr_t)W_out & 3) return set_error("%s: W_out is misaligned (4 bytes)", fn);
  if (fmt == MT_W_BF16 && ((uintptr_t)codes_out & 1)) return set_error("%s: codes_out is misaligned (2 bytes)", fn);
  PackArgs a = {};
  a.codes = (uint4*)codes; a.scales = (float*)scales; a.out = W_out; a.codes_out = codes_out; a.N = N; a.K = (int)K;
  a.glu = glu ? 1 : 0;
  const dim3 grid((unsigned)tiles_of(N, glu));
  const hipStream_t st = (hipStream_t)stream;
  if (fmt == MT_W_BF16) hipLaunchKernelGGL((weight_dequant_kernel<MT_W_BF16>), grid, dim3(256), 0, st, a);
  else if (fmt == MT_W_FP8) hipLaunchKernelGGL((weight_dequant_kernel<MT_W_FP8>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((weight_dequant_kernel<MT_W_INT4>), grid, dim3(256), 0, st, a);
  return check_hip(hipGetLastError(), fn);
}

extern "C" int mt_linear_rows_wq(int fmt, int G, const float* x, int64_t ldx, int64_t M, int64_t K, int norm,
                                 const float* gamma, const float* beta, float eps, const void* const* W,
                                 const float* const* scales, const int64_t* N, const float* const* bias,
                                 const float* const* residual, float* const* out, int gelu_mask, int glu_mask,
                                 void* stream) {
  const char* fn = "mt_linear_rows_wq";
  if (fmt != MT_W_BF16 && fmt != MT_W_FP8 && fmt != MT_W_INT4)
    return set_error("%s: fmt=%d is not MT_W_BF16, MT_W_FP8 or MT_W_INT4", fn, fmt);
  if (G < 1 || G > kMaxG) return set_error("%s: G=%d is outside 1..%d", fn, G, kMaxG);
  if (M < 1 || M > kMaxM)
    return set_error("%s: M=%lld is outside 1..%d (the skinny kernel; dequantise and use mt_matmul_f32)", fn, (long long)M, kMaxM);
  if (K < kKMul || K > kMaxK || K % kKMul)
    return set_error("%s: K=%lld must be a multiple of %d in %d..%d", fn, (long long)K, kKMul, kKMul, kMaxK);
  if (!x) return set_error("%s: x is NULL", fn);
  if (ldx < K || ldx % 4) return set_error("%s: ldx=%lld must be a multiple of 4 and >= K", fn, (long long)ldx);
  if (!W || !N || !out) return set_error("%s: the W, N or out array is NULL", fn);
  if (fmt != MT_W_BF16 && !scales) return set_error("%s: the scales array is NULL (fp8 and int4 have scales)", fn);
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
  for (int g = 0; g < G; ++g) {
    const bool glu = (glu_mask >> g) & 1;
    if (N[g] < 1 || N[g] > ((1ll << 31) - kTile) / (glu ? 2 : 1))
      return set_error("%s: N[%d]=%lld is outside 1..%s", fn, g, (long long)N[g], glu ? "2^30-32 (gated)" : "2^31-64");
    const float* sc = scales ? scales[g] : nullptr;
    if (int e = check_storage(fn, fmt, W[g], sc, g)) return e;
    if (!out[g]) return set_error("%s: out[%d] is NULL", fn, g);
    const float* b = bias ? bias[g] : nullptr;
    const float* r = residual ? residual[g] : nullptr;
    if (((uintptr_t)out[g] | (uintptr_t)b | (uintptr_t)r) & 3)
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
    a.W[g] = (const uint4*)W[g]; a.scale[g] = sc; a.N[g] = N[g]; a.bias[g] = b; a.res[g] = r; a.out[g] = out[g];
    const bool vio = N[g] % 4 == 0 && !(((uintptr_t)out[g] | (uintptr_t)b | (uintptr_t)r) & 15);
    a.vec |= (vio ? 1 : 0) << g;
    tiles += tiles_of(N[g], glu);
    if (tiles > (1ll << 30)) return set_error("%s: too many column tiles", fn);
    a.tile_end[g] = (int)tiles;
  }
  for (int g = G; g < kMaxG; ++g) a.tile_end[g] = 0x7fffffff;

  const hipStream_t st = (hipStream_t)stream;
  const int rb = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
  if (fmt == MT_W_BF16) launch_rows<MT_W_BF16>(a, (int)tiles, rb, st);
  else if (fmt == MT_W_FP8) launch_rows<MT_W_FP8>(a, (int)tiles, rb, st);
  else launch_rows<MT_W_INT4>(a, (int)tiles, rb, st);
  return check_hip(hipGetLastError(), fn);
}
