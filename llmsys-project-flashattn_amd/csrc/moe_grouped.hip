// mt_moe_sort / mt_moe_grouped_gemm / mt_moe_combine / mt_moe_gate_grad (include/minitorch_hip.h):
// the routed mixture-of-experts MLP for any number of rows, forward and backward. The M k
// (row, slot) entries are sorted by expert once; every product then runs over the sorted segments,
// an expert's weights against the rows routed to it and no others. fp32 throughout, products on
// v_mfma_f32_32x32x2_f32, no atomics, no allocation, and every grid a function of the host
// arguments alone (no count ever leaves the device: a captured training step replays).
//
// Sort (three launches). The entries are cut into U <= 1024 runs of R consecutive entries, a wave
// per run. count_kernel: the wave walks its run 64 entries at a time; one ballot per expert gives
// the run's count of every expert, written to the workspace cnt [U, E]. scan_kernel (one wave,
// lane e): the exclusive prefix of cnt[:, e] down the runs, then an exclusive scan of the totals
// over the experts: offsets [E + 1]. place_kernel: the wave walks its run again; lane e carries
// offsets[e] + cnt[u][e], the next free position of expert e; an entry's position is its expert's
// base plus the number of lower lanes with the same expert (ballot and prefix count), so entries
// stay ascending inside a segment. It writes perm, pos, and optionally row[p] = entry / k and
// gate[p] = gates[row, expert], the per-position operands of the products below.
//
// Grouped GEMM, one kernel template, three operand forms. A workgroup (256 threads, four waves as
// 2 x 2) owns a tile of 64 rows by 64 NB columns, NB = 2 when the output is at least 128 columns
// wide, and walks the reduction in chunks of 16. Both operand chunks lie in LDS k-major,
// [16][64 (NB) + 4] floats: an operand that is contiguous along the reduction in memory (A of NN
// and NT, W of NT) is loaded as 16 bytes along k and stored transposed, one that is contiguous
// along its rows or columns (W of NN, both operands of TN) is stored as it was loaded. A wave
// reads one float of A and NB floats of B per 32x32x2 MFMA and k pair (lane l: row or column
// l % 32, k = l / 32: 32 consecutive floats per half wave, no bank conflict) and keeps NB
// 32 x 32 accumulators (16 NB registers). The chunks are double-buffered: the 16-byte global loads
// of chunk c + 1 are issued before the MFMAs of chunk c and stored to the other buffer after
// them, one barrier per chunk.
//   NN / NT  grid (floor(P / 64) + E, column tiles): the row-tile bound. A workgroup walks offsets
//            (E <= 64 uniform loads) to its (expert, tile); a surplus workgroup leaves at once and
//            an empty expert owns no tile, so neither touches a weight.
//   TN       grid (tiles of Ka, tiles of N, E): the reduction runs down the expert's segment in
//            ascending position, rows past its end are zeros. The workgroups of Ka tile 0 also
//            add up the (scaled) rows of B for db: thread (q, n) sums the rows 4 q .. 4 q + 3 of
//            every chunk, the four parts are combined as ((s0 + s1) + s2) + s3.
// Accumulation: output (i, j) is one accumulator lane, zero, then one MFMA per k pair in ascending
// k; row i of the result reads row i of A only, so the bits of an NN / NT row depend on its A row,
// the expert's weights, the bias and the sizes, not on the tile, M or the rows beside it. The bias
// is added after the chain, the row scale last (one more rounding).
#include "../../include/minitorch_hip.h"
#include "fa_common.h"

namespace mt {
int set_error(const char* fmt, ...);  // capi_flash.hip
int check_hip(hipError_t e, const char* where);

namespace moeg {
constexpr int kTM = MT_MOE_GROUPED_TM;  // rows of a tile
constexpr int kKC = 16;      // reduction chunk
constexpr int kMaxE = 64, kMaxTop = 8;
constexpr int kMaxRuns = 1024;
constexpr int kDim = 1 << 20;

typedef float f32x16v __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------- sort
struct SortArgs {
  const int* idx;      // [P]
  const float* gates;  // [M, E] or NULL
  int* cnt;            // [U, E]
  int* offsets;        // [E + 1]
  int* perm;           // [P]
  int* pos;            // [P]
  int* row;            // [P] or NULL
  float* gate;         // [P] or NULL
  int64_t P, R;        // entries, entries per run (a multiple of 64)
  int U, E, k;
};

__global__ __launch_bounds__(256) void count_kernel(const SortArgs a) {
  const int lane = threadIdx.x & 63;
  const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= a.U) return;
  const int64_t b0 = (int64_t)u * a.R, b1 = min(b0 + a.R, a.P);
  int mine = 0;  // lane e: the run's count of expert e
  for (int64_t i0 = b0; i0 < b1; i0 += 64) {
    const int64_t i = i0 + lane;
    const int x = i < b1 ? a.idx[i] : -1;
    for (int e = 0; e < a.E; ++e) {
      const int c = __popcll(__ballot(x == e));
      if (lane == e) mine += c;
    }
  }
  if (lane < a.E) a.cnt[(int64_t)u * a.E + lane] = mine;
}

__global__ __launch_bounds__(64) void scan_kernel(const SortArgs a) {
  const int lane = threadIdx.x;
  int total = 0;
  if (lane < a.E) {
    for (int u = 0; u < a.U; ++u) {  // lanes read consecutive ints of row u
      const int c = a.cnt[(int64_t)u * a.E + lane];
      a.cnt[(int64_t)u * a.E + lane] = total;
      total += c;
    }
  }
  int incl = total;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane < a.E) a.offsets[lane + 1] = incl;
  if (lane == 0) a.offsets[0] = 0;
}

__global__ __launch_bounds__(256) void place_kernel(const SortArgs a) {
  const int lane = threadIdx.x & 63;
  const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= a.U) return;
  const int64_t b0 = (int64_t)u * a.R, b1 = min(b0 + a.R, a.P);
  const int total = a.offsets[a.E];
  int base = lane < a.E ? a.offsets[lane] + a.cnt[(int64_t)u * a.E + lane] : 0;
  for (int64_t i0 = b0; i0 < b1; i0 += 64) {
    const int64_t i = i0 + lane;
    int x = i < b1 ? a.idx[i] : -1;
    if (x >= a.E) x = -1;
    int rank = 0, add = 0;
    for (int e = 0; e < a.E; ++e) {
      const unsigned long long b = __ballot(x == e);
      if (x == e) rank = __popcll(b & ((1ull << lane) - 1ull));
      if (lane == e) add = __popcll(b);
    }
    const int p = __shfl(base, x < 0 ? 0 : x, 64) + rank;
    base += add;
    if (i < b1) {
      if (i >= total) a.perm[i] = -1;  // the tail past the last segment (dropped entries)
      a.pos[i] = x < 0 ? -1 : p;
      if (x >= 0) {
        a.perm[p] = (int)i;
        if (a.row) a.row[p] = (int)(i / a.k);
        if (a.gate) a.gate[p] = a.gates[(i / a.k) * a.E + x];
      }
    }
  }
}

// ---------------------------------------------------------------------------------- grouped GEMM
enum { kNN = 0, kNT = 1, kTN = 2 };

struct GemmArgs {
  const float* A;      // NN / NT [a_rows, Kd]; TN [a_rows, Ka]
  const float* B;      // NN W [E, Kd, N]; NT W [E, N, Kd]; TN B [b_rows, N]
  const float* bias;   // [E, N] or NULL (NN)
  const int* src;      // [P] rows of A, or NULL (the position itself)
  const int* srcb;     // [P] rows of B (TN), or NULL
  const float* s;      // [P] row scale (of the output row; TN: of the row of B), or NULL
  const int* offsets;  // [E + 1]
  float* C;            // NN / NT [P, N]; TN [E, Ka, N]
  float* db;           // TN [E, N] or NULL
  int64_t a_rows, b_rows, P;
  int E, Kd, N;        // TN: Kd is Ka, the rows of dW[e]
};

// the expert's segment, held inside [0, P] whatever the device memory says
__device__ __forceinline__ void segment(const GemmArgs& a, int e, int64_t& lo, int64_t& hi) {
  lo = min(max((int64_t)a.offsets[e], (int64_t)0), a.P);
  hi = min(max((int64_t)a.offsets[e + 1], lo), a.P);
}
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ int64_t row_of(const int* src, int64_t p, int64_t rows) {
  return src ? min(max((int64_t)src[p], (int64_t)0), rows - 1) : min(p, rows - 1);
}

template <int FORM, int NB>
__global__ __launch_bounds__(256) void gemm_kernel(const GemmArgs a) {
  constexpr int TN = 64 * NB, SA = kTM + 4, SB = TN + 4;
  __shared__ __attribute__((aligned(16))) float As[2][kKC * SA];
  __shared__ __attribute__((aligned(16))) float Bs[2][kKC * SB];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lk = lane >> 5;

  // which expert, which rows
  int e;
  int64_t p0, p1;  // NN / NT: the tile's positions [p0, p1); TN: the segment
  if (FORM == kTN) {
    e = blockIdx.z;
    segment(a, e, p0, p1);
  } else {
    int64_t left = blockIdx.x;
    p0 = p1 = 0;
    for (e = 0; e < a.E; ++e) {
      int64_t lo, hi;
      segment(a, e, lo, hi);
      const int64_t tiles = (hi - lo + kTM - 1) / kTM;
      if (left < tiles) {
        p0 = lo + left * kTM;
        p1 = min(p0 + kTM, hi);
        break;
      }
      left -= tiles;
    }
    if (e == a.E) return;  // a surplus workgroup
  }
  const int N = a.N, Kd = a.Kd;
  const int64_t m0 = FORM == kTN ? (int64_t)blockIdx.x * kTM : 0;  // TN: first row of dW[e]
  const int64_t n0 = (int64_t)blockIdx.y * TN;
  // the reduction: Kd columns (NN / NT) or the segment's rows (TN)
  const int64_t L = FORM == kTN ? p1 - p0 : Kd;
  const int64_t nch = (L + kKC - 1) / kKC;

  // this thread's share of a chunk: one 16-byte load of A, NB of B
  const int kr = t >> 2, kq = 4 * (t & 3);  // an operand contiguous along k: tile row kr (+ 64 u), k offset kq
  const float* arow = nullptr;
  if (FORM != kTN) arow = a.A + row_of(a.src, min(p0 + kr, p1 - 1), a.a_rows) * Kd;
  const float* brow[NB];
  if (FORM == kNT) {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int64_t n = n0 + kr + 64 * u;
      brow[u] = a.B + ((int64_t)e * N + (n < N ? n : 0)) * Kd;
    }
  }
  const float* W = a.B + (int64_t)e * Kd * N;  // NN

  float4 ra, rb[NB];
  auto fetch = [&](int64_t c) {
    const int64_t k0 = c * kKC;
    if (FORM != kTN) {
      ra = k0 + kq < Kd ? *(const float4*)(arow + k0 + kq) : zero4();
    } else {  // A[src[p]][m0 + 4 (t % 16)], p = p0 + k0 + t / 16
      const int64_t p = p0 + k0 + (t >> 4), col = m0 + 4 * (t & 15);
      ra = p < p1 && col < Kd ? *(const float4*)(a.A + row_of(a.src, p, a.a_rows) * Kd + col) : zero4();
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (FORM == kNT) {
        rb[u] = k0 + kq < Kd ? *(const float4*)(brow[u] + k0 + kq) : zero4();
      } else {
        const int id = t + 256 * u;
        const int kk = id / (TN / 4);
        const int64_t col = n0 + 4 * (id % (TN / 4));
        if (FORM == kNN) {
          rb[u] = k0 + kk < Kd && col < N ? *(const float4*)(W + (k0 + kk) * N + col) : zero4();
        } else {
          const int64_t p = p0 + k0 + kk;
          float4 v = zero4();
          if (p < p1 && col < N) {
            v = *(const float4*)(a.B + row_of(a.srcb, p, a.b_rows) * N + col);
            if (a.s) {
              const float sc = a.s[p];
              v = make_float4(sc * v.x, sc * v.y, sc * v.z, sc * v.w);
            }
          }
          rb[u] = v;
        }
      }
    }
  };
  auto stage = [&](int buf) {
    if (FORM != kTN) {
      float* d = As[buf] + kq * SA + kr;
      d[0] = ra.x; d[SA] = ra.y; d[2 * SA] = ra.z; d[3 * SA] = ra.w;
    } else {
      *(float4*)(As[buf] + (t >> 4) * SA + 4 * (t & 15)) = ra;
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (FORM == kNT) {
        float* d = Bs[buf] + kq * SB + kr + 64 * u;
        d[0] = rb[u].x; d[SB] = rb[u].y; d[2 * SB] = rb[u].z; d[3 * SB] = rb[u].w;
      } else {
        const int id = t + 256 * u;
        *(float4*)(Bs[buf] + (id / (TN / 4)) * SB + 4 * (id % (TN / 4))) = rb[u];
      }
    }
  };

  f32x16v acc[NB];
#pragma unroll
  for (int u = 0; u < NB; ++u)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[u][v] = 0.f;
  const bool want_db = FORM == kTN && a.db && blockIdx.x == 0;
  float colsum = 0.f;  // TN, db: thread (q = t / 64, n = t % 64)

  if (nch > 0) {
    fetch(0);
    stage(0);
  }
  __syncthreads();
  for (int64_t c = 0; c < nch; ++c) {
    const int buf = (int)(c & 1);
    const bool more = c + 1 < nch;
    if (more) fetch(c + 1);
    const float* as = As[buf] + lk * SA + 32 * wm + li;
    const float* bs = Bs[buf] + lk * SB + 32 * NB * wn + li;
#pragma unroll
    for (int s2 = 0; s2 < kKC / 2; ++s2) {
      const float av = as[2 * s2 * SA];
#pragma unroll
      for (int u = 0; u < NB; ++u)
        acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bs[2 * s2 * SB + 32 * u], acc[u], 0, 0, 0);
    }
    if (want_db) {
#pragma unroll
      for (int r = 0; r < 4; ++r) colsum += Bs[buf][(4 * wave + r) * SB + lane];
    }
    if (more) stage(buf ^ 1);
    __syncthreads();
  }

  // epilogue: accumulator v of lane l is row 8 (v / 4) + 4 (l / 32) + v % 4, column l % 32
  const int64_t rows = FORM == kTN ? min((int64_t)kTM, (int64_t)Kd - m0) : p1 - p0;
  float* C = FORM == kTN ? a.C + ((int64_t)e * Kd + m0) * N : a.C + p0 * N;
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    const int64_t col = n0 + 32 * NB * wn + 32 * u + li;
    if (col >= N) continue;
    const float bv = FORM == kNN && a.bias ? a.bias[(int64_t)e * N + col] : 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int i = 32 * wm + 8 * (v >> 2) + 4 * lk + (v & 3);
      if (i >= rows) continue;
      float o = acc[u][v];
      if (FORM != kTN) {
        if (FORM == kNN && a.bias) o += bv;
        if (a.s) o = a.s[p0 + i] * o;
      }
      C[(int64_t)i * N + col] = o;
    }
  }
  if (want_db) {  // ((s0 + s1) + s2) + s3 through LDS (the chunk buffers are free: the loop ended on a barrier)
    float* part = As[0];
    part[wave * 64 + lane] = colsum;
    __syncthreads();
    if (wave == 0 && n0 + lane < N)
      a.db[(int64_t)e * N + n0 + lane] = ((part[lane] + part[64 + lane]) + part[128 + lane]) + part[192 + lane];
  }
}

// ---------------------------------------------------------------------------------- companions
// out[m] = residual[m] + ((g0 y[pos0]) + g1 y[pos1]) + ...; a thread per 4 columns
__global__ __launch_bounds__(256) void combine_kernel(const float* __restrict__ y, const int* __restrict__ pos,
                                                      const float* __restrict__ gates, const int* __restrict__ idx,
                                                      const float* __restrict__ res, float* __restrict__ out, int64_t M,
                                                      int N4, int E, int k) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * N4) return;
  const int64_t m = i / N4, c = 4 * (i - m * N4), P = M * k;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  bool bad = false;
  for (int j = 0; j < k; ++j) {
    const int64_t p = pos[m * k + j];
    if (p < 0 || p >= P) { bad = true; break; }
    const float4 v = *(const float4*)(y + p * (4 * (int64_t)N4) + c);
    float g = 1.f;
    if (gates) {
      const int x = idx[m * k + j];
      if (x < 0 || x >= E) { bad = true; break; }
      g = gates[m * E + x];
    }
    if (j == 0) s = gates ? make_float4(g * v.x, g * v.y, g * v.z, g * v.w) : v;
    else if (gates) s = make_float4(s.x + g * v.x, s.y + g * v.y, s.z + g * v.z, s.w + g * v.w);
    else s = make_float4(s.x + v.x, s.y + v.y, s.z + v.z, s.w + v.w);
  }
  if (bad) {  // a row with a non-finite router logit (mt_moe_rows' rule)
    const float n = __builtin_nanf("");
    s = make_float4(n, n, n, n);
  }
  if (res) {
    const float4 r = *(const float4*)(res + 4 * i);
    s = make_float4(r.x + s.x, r.y + s.y, r.z + s.z, r.w + s.w);
  }
  *(float4*)(out + 4 * i) = s;
}

// dgate[m, idx(m, j)] = <dout[m], y[pos(m, j)]>, a wave per (row, slot); the wave of slot 0 also
// writes the zeros of the experts the row did not choose
__global__ __launch_bounds__(256) void gate_grad_kernel(const float* __restrict__ dout, const float* __restrict__ y,
                                                        const int* __restrict__ pos, const int* __restrict__ idx,
                                                        float* __restrict__ dgate, int64_t M, int N4, int E, int k) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), P = M * k;
  if (w >= P) return;
  const int64_t m = w / k;
  const int j = (int)(w - m * k);
  if (j == 0 && lane < E) {
    bool chosen = false;
    for (int q = 0; q < k; ++q) chosen |= idx[m * k + q] == lane && pos[m * k + q] >= 0;
    if (!chosen) dgate[m * E + lane] = 0.f;
  }
  const int64_t p = pos[w];
  const int x = idx[w];
  if (p < 0 || p >= P || x < 0 || x >= E) return;
  const float4* d4 = (const float4*)(dout + m * 4 * (int64_t)N4);
  const float4* y4 = (const float4*)(y + p * 4 * (int64_t)N4);
  float s = 0.f;
  for (int c = lane; c < N4; c += 64) {
    const float4 dv = d4[c], yv = y4[c];
    s += (dv.x * yv.x + dv.y * yv.y) + (dv.z * yv.z + dv.w * yv.w);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) dgate[m * E + x] = s;
}

static int check_sizes(const char* fn, int64_t M, int64_t E, int64_t k) {
  if (M < 1) return set_error("%s: M=%lld must be at least 1", fn, (long long)M);
  if (E < 2 || E > kMaxE) return set_error("%s: E=%lld is outside 2..%d", fn, (long long)E, kMaxE);
  if (k < 1 || k > kMaxTop) return set_error("%s: k=%lld is outside 1..%d", fn, (long long)k, kMaxTop);
  if (k > E) return set_error("%s: k=%lld exceeds E=%lld", fn, (long long)k, (long long)E);
  if (M > ((int64_t)1 << 31) - 1 || M * k > ((int64_t)1 << 31) - 1)
    return set_error("%s: M k=%lld must be below 2^31", fn, (long long)(M * k));
  return 0;
}

// runs of R entries (a multiple of 64), at most kMaxRuns of them
static void runs(int64_t P, int64_t& R, int& U) {
  const int64_t w = (P + 63) / 64;
  R = 64 * ((w + kMaxRuns - 1) / kMaxRuns);
  U = (int)((P + R - 1) / R);
}

template <int FORM>
static void launch_gemm(const GemmArgs& a, dim3 grid, bool wide, hipStream_t st) {
  if (wide) hipLaunchKernelGGL((gemm_kernel<FORM, 2>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((gemm_kernel<FORM, 1>), grid, dim3(256), 0, st, a);
}
}  // namespace moeg
}  // namespace mt

using namespace mt;
using namespace mt::moeg;

extern "C" int mt_moe_sort_workspace_bytes(int64_t M, int64_t E, int64_t k, int64_t* bytes) {
  const char* fn = "mt_moe_sort_workspace_bytes";
  if (!bytes) return set_error("%s: bytes is NULL", fn);
  if (int rc = check_sizes(fn, M, E, k)) return rc;
  int64_t R;
  int U;
  runs(M * k, R, U);
  *bytes = (int64_t)U * E * 4;
  return 0;
}

extern "C" int mt_moe_sort(const int32_t* topk_idx, const float* gates, int64_t M, int64_t E, int64_t k,
                           int32_t* offsets, int32_t* perm, int32_t* pos, int32_t* row, float* gate, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  const char* fn = "mt_moe_sort";
  if (int rc = check_sizes(fn, M, E, k)) return rc;
  if (!topk_idx) return set_error("%s: topk_idx is NULL", fn);
  if (!offsets || !perm || !pos) return set_error("%s: offsets, perm or pos is NULL", fn);
  if (!workspace) return set_error("%s: workspace is NULL", fn);
  if ((gate != nullptr) != (gates != nullptr)) return set_error("%s: gates and gate go together", fn);
  if (((uintptr_t)topk_idx | (uintptr_t)gates | (uintptr_t)offsets | (uintptr_t)perm | (uintptr_t)pos | (uintptr_t)row |
       (uintptr_t)gate | (uintptr_t)workspace) & 3)
    return set_error("%s: a pointer is misaligned (4 bytes)", fn);
  SortArgs a = {};
  a.idx = topk_idx; a.gates = gates; a.cnt = (int*)workspace; a.offsets = offsets; a.perm = perm; a.pos = pos;
  a.row = row; a.gate = gate; a.P = M * k; a.E = (int)E; a.k = (int)k;
  runs(a.P, a.R, a.U);
  if (workspace_bytes < (int64_t)a.U * E * 4)
    return set_error("%s: workspace_bytes=%lld is below the %lld bytes mt_moe_sort_workspace_bytes asks for", fn,
                     (long long)workspace_bytes, (long long)((int64_t)a.U * E * 4));
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((a.U + 3) / 4);
  hipLaunchKernelGGL(count_kernel, grid, dim3(256), 0, st, a);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(64), 0, st, a);
  hipLaunchKernelGGL(place_kernel, grid, dim3(256), 0, st, a);
  return check_hip(hipGetLastError(), fn);
}

extern "C" int mt_moe_grouped_gemm(int form, const float* A, int64_t a_rows, const int32_t* src, const float* s,
                                   const float* B, int64_t b_rows, const int32_t* srcb, const float* bias,
                                   const int32_t* offsets, int64_t P, int64_t E, int64_t Kd, int64_t N, float* C,
                                   float* db, void* stream) {
  const char* fn = "mt_moe_grouped_gemm";
  if (form < 0 || form > 2) return set_error("%s: form=%d is outside 0..2 (NN, NT, TN)", fn, form);
  if (P < 1 || P > ((int64_t)1 << 31) - 1) return set_error("%s: P=%lld is outside 1..2^31-1", fn, (long long)P);
  if (E < 2 || E > kMaxE) return set_error("%s: E=%lld is outside 2..%d", fn, (long long)E, kMaxE);
  if (Kd < 4 || Kd > kDim || Kd % 4) return set_error("%s: Kd=%lld must be a multiple of 4 in 4..2^20", fn, (long long)Kd);
  if (N < 4 || N > kDim || N % 4) return set_error("%s: N=%lld must be a multiple of 4 in 4..2^20", fn, (long long)N);
  if (!A || !B || !C) return set_error("%s: A, B or C is NULL", fn);
  if (!offsets) return set_error("%s: offsets is NULL", fn);
  if (a_rows < 1 || a_rows > ((int64_t)1 << 31) - 1) return set_error("%s: a_rows=%lld is outside 1..2^31-1", fn, (long long)a_rows);
  if (!src && a_rows < P) return set_error("%s: a_rows=%lld is below P=%lld and there is no src", fn, (long long)a_rows, (long long)P);
  if (form == kTN) {
    if (bias) return set_error("%s: the TN form takes no bias", fn);
    if (b_rows < 1 || b_rows > ((int64_t)1 << 31) - 1) return set_error("%s: b_rows=%lld is outside 1..2^31-1", fn, (long long)b_rows);
    if (!srcb && b_rows < P) return set_error("%s: b_rows=%lld is below P=%lld and there is no srcb", fn, (long long)b_rows, (long long)P);
  } else {
    if (srcb || db) return set_error("%s: srcb and db belong to the TN form", fn);
    if (form == kNT && bias) return set_error("%s: the NT form takes no bias", fn);
  }
  if (((uintptr_t)A | (uintptr_t)B | (uintptr_t)C | (uintptr_t)bias | (uintptr_t)db) & 15)
    return set_error("%s: A, B, C, bias or db is misaligned (16 bytes)", fn);
  if (((uintptr_t)src | (uintptr_t)srcb | (uintptr_t)s | (uintptr_t)offsets) & 3)
    return set_error("%s: src, srcb, s or offsets is misaligned (4 bytes)", fn);
  GemmArgs a = {};
  a.A = A; a.B = B; a.bias = bias; a.src = src; a.srcb = srcb; a.s = s; a.offsets = offsets; a.C = C; a.db = db;
  a.a_rows = a_rows; a.b_rows = b_rows; a.P = P; a.E = (int)E; a.Kd = (int)Kd; a.N = (int)N;
  const hipStream_t st = (hipStream_t)stream;
  const bool wide = form != kTN && N >= 128;
  const unsigned ct = (unsigned)((N + (wide ? 127 : 63)) / (wide ? 128 : 64));
  if (form == kTN) launch_gemm<kTN>(a, dim3((unsigned)((Kd + kTM - 1) / kTM), ct, (unsigned)E), false, st);
  else if (form == kNN) launch_gemm<kNN>(a, dim3((unsigned)(P / kTM + E), ct), wide, st);
  else launch_gemm<kNT>(a, dim3((unsigned)(P / kTM + E), ct), wide, st);
  return check_hip(hipGetLastError(), fn);
}

static int check_rows(const char* fn, int64_t M, int64_t N, int64_t E, int64_t k) {
  if (int rc = check_sizes(fn, M, E, k)) return rc;
  if (N < 4 || N > kDim || N % 4) return set_error("%s: N=%lld must be a multiple of 4 in 4..2^20", fn, (long long)N);
  return 0;
}

extern "C" int mt_moe_combine(const float* y, const int32_t* pos, const float* gates, const int32_t* topk_idx,
                              const float* residual, float* out, int64_t M, int64_t N, int64_t E, int64_t k,
                              void* stream) {
  const char* fn = "mt_moe_combine";
  if (int rc = check_rows(fn, M, N, E, k)) return rc;
  if (!y || !pos || !out) return set_error("%s: y, pos or out is NULL", fn);
  if ((gates != nullptr) != (topk_idx != nullptr)) return set_error("%s: gates and topk_idx go together", fn);
  if (((uintptr_t)y | (uintptr_t)residual | (uintptr_t)out) & 15)
    return set_error("%s: y, residual or out is misaligned (16 bytes)", fn);
  if (((uintptr_t)pos | (uintptr_t)gates | (uintptr_t)topk_idx) & 3)
    return set_error("%s: pos, gates or topk_idx is misaligned (4 bytes)", fn);
  const int64_t n = M * (N / 4);
  if ((n + 255) / 256 > 0x7fffffff) return set_error("%s: M N=%lld is too large", fn, (long long)(M * N));
  hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, pos, gates,
                     topk_idx, residual, out, M, (int)(N / 4), (int)E, (int)k);
  return check_hip(hipGetLastError(), fn);
}

extern "C" int mt_moe_gate_grad(const float* dout, const float* y, const int32_t* pos, const int32_t* topk_idx,
                                float* dgate, int64_t M, int64_t N, int64_t E, int64_t k, void* stream) {
  const char* fn = "mt_moe_gate_grad";
  if (int rc = check_rows(fn, M, N, E, k)) return rc;
  if (!dout || !y || !pos || !topk_idx || !dgate) return set_error("%s: dout, y, pos, topk_idx or dgate is NULL", fn);
  if (((uintptr_t)dout | (uintptr_t)y) & 15) return set_error("%s: dout or y is misaligned (16 bytes)", fn);
  if (((uintptr_t)pos | (uintptr_t)topk_idx | (uintptr_t)dgate) & 3)
    return set_error("%s: pos, topk_idx or dgate is misaligned (4 bytes)", fn);
  hipLaunchKernelGGL(gate_grad_kernel, dim3((unsigned)((M * k + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dout, y, pos,
                     topk_idx, dgate, M, (int)(N / 4), (int)E, (int)k);
  return check_hip(hipGetLastError(), fn);
}
