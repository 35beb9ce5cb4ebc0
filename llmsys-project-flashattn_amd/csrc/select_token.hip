// mt_select_token (include/minitorch_hip.h): the next token of every row of a [B, V] logits
// matrix chosen on the device, greedy or temperature / top-k sampling, so that a generation
// step needs neither a copy of the logits to the host nor a synchronise, and can be captured
// in a hipGraph. Kernel and C entry; the uniform draw is rng.h's (the value mt_rand_uniform
// writes at index b).
//
// One workgroup of 256 threads (4 waves) per row:
//   0. the row is read once (16-B loads from the first 16-B aligned element on) into LDS, and
//      the greedy id found on the way: the maximum of (order key, ~index) packed in 64 bits,
//      a NaN taking the largest key. Greedy rows stop here and never touch LDS.
//   1. top_k < V: the key of the k-th largest entry by a 4-pass, 8-bit radix select over the
//      order-preserving keys (LDS histogram of 256 bins per pass, the row read 16 B per lane;
//      wave 0 picks the digit by a suffix scan of the bins), and, when only some of the
//      entries equal to that key are kept, the index of the last kept one (ballot counts in
//      index order).
//   2. e_i = exp((x_i - max) / T) of the kept entries replaces the row in LDS; each wave sums
//      its quarter of the row in a fixed order, the four totals are added in wave order.
//   3. each wave scans its quarter (4 consecutive entries per lane, a wave prefix sum per 256
//      entries, tiles of zeros skipped) from the total of the quarters before it and reports
//      the first entry whose running sum exceeds u * sum; the lowest such index wins, and the
//      last kept index with e_i > 0 when rounding leaves none.
//  2p. mt_select_token_p / mt_spec_accept_p with top_p < 1 or min_p > 0 only (the NUCLEUS
//      instantiation; every other launch runs the kernel without this phase, whose device code
//      is what it was before the phase existed): the e_i are non-negative, so their bit patterns
//      order as unsigned integers. top_p: the bit pattern of the last entry of the nucleus by
//      the radix select of phase 1 on mass instead of count (the mass of an entry is the integer
//      trunc(e_i 2^40), summed per bin by 64-bit LDS integer atomics: exact, so independent of
//      their order), and the tie cut among the entries equal to it by the ballot walk of phase
//      1 (tie_cut below; phase 1 keeps its own copy of the walk so that its code stays as it
//      was). min_p: e_i >= min_p. What falls outside either is zeroed and the wave totals are
//      formed again in phase 2's order.
// Every sum has a fixed association or is an exact integer sum, so the id is a function of the
// row's bits, T, top_k, top_p, min_p, the seed and b alone. Stores are plain vector stores; the
// only atomics are integer ones on the LDS histograms.
// mt_spec_accept (spec_decode.hip) launches the same kernel over k + 1 logits rows per batch row
// (select_token.h: SelectArgs.rows, count, skip, scratch): row i of batch row b draws with
// seed + count[b] + i and b's uniform, and its id goes to the caller's scratch only.
#include "../../include/minitorch_hip.h"
#include "fa_common.h"
#include "rng.h"
#include "select_token.h"
#include <math.h>

namespace mt {
int set_error(const char* fmt, ...);           // capi_flash.hip
int check_hip(hipError_t e, const char* where);

// fp32 -> u32 with the floats' order (-0 as +0, as the comparison has it); a NaN above +inf
__device__ __forceinline__ uint32_t order_key(float x) {
  if (x != x) return 0xFFFFFFFFu;
  const uint32_t u = __float_as_uint(x == 0.f ? 0.f : x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float wave_sum(float v) {  // the same tree on every lane
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void write_id(const SelectArgs& a, int b, int i, int id) {
  if (a.scratch) {
    a.scratch[(int64_t)b * a.rows + i] = id;
    return;
  }
  if (a.next_f32) a.next_f32[b] = (float)id;
  if (a.next_i32) a.next_i32[b] = id;
  if (a.done && a.eos_id >= 0 && (int64_t)id == a.eos_id) a.done[b] |= 1;
  if (a.history) {
    const int64_t step = *a.step_dev;  // a step outside the row is dropped
    if (step >= 0 && step < a.history_stride) a.history[(int64_t)b * a.history_stride + step] = id;
  }
}

// The index of the `need`-th entry, in index order, for which is_tie holds (1 <= need <= their
// number): each wave counts its quarter [lo, hi) by ballots, the one that holds it walks it again.
// Two barriers; every thread of the workgroup calls it.
template <class F>
__device__ __forceinline__ int tie_cut(F is_tie, int lo, int hi, int need, int lane, int wave, int* ties_w,
                                       int* cut_s) {
  int cnt = 0;
  for (int t = lo; t < hi; t += 64) {
    const int i = t + lane;
    cnt += __popcll(__ballot(i < hi && is_tie(i)));
  }
  if (lane == 0) ties_w[wave] = cnt;
  __syncthreads();
  int run = 0;
  for (int w = 0; w < wave; ++w) run += ties_w[w];
  if (run < need && need <= run + cnt) {
    for (int t = lo; t < hi; t += 64) {
      const int i = t + lane;
      unsigned long long m = __ballot(i < hi && is_tie(i));
      const int c = __popcll(m);
      if (run + c >= need) {
        for (int q = need - run; q > 1; --q) m &= m - 1;
        if (lane == 0) *cut_s = t + __ffsll((long long)m) - 1;
        break;
      }
      run += c;
    }
  }
  __syncthreads();
  return *cut_s;
}

// NUCLEUS: the top-p / min-p phase between phases 2 and 3; false is the kernel without it
template <int CAP, bool NUCLEUS>
__global__ __launch_bounds__(kSelThreads) void select_token_kernel(const SelectArgs a) {
  __shared__ __attribute__((aligned(16))) float row[CAP];
  __shared__ __attribute__((aligned(16))) unsigned hist[256];
  __shared__ unsigned long long best_w[4];
  __shared__ float sum_w[4];
  __shared__ int last_w[4], cand_w[4], ties_w[4];
  __shared__ unsigned sel[2];
  __shared__ int cut_s;

  const int b = blockIdx.x / a.rows, ri = blockIdx.x - b * a.rows;  // the batch row, the logits row in it
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = a.V;
  if (a.skip && a.skip[b]) return;  // workgroup-uniform
  const float* rp = a.logits + (int64_t)b * a.batch_stride + (int64_t)ri * a.row_stride;
  const bool sampling = a.temperature > 0.f;

  // ---- 0: load the row, greedy id --------------------------------------------------------
  unsigned long long best = 0;
  auto take = [&](int i, float x) {
    const unsigned long long p = ((unsigned long long)order_key(x) << 32) | (0xFFFFFFFFu - (unsigned)i);
    best = p > best ? p : best;
    if (sampling) row[i] = x;
  };
  {
    const int mis = (int)(((uintptr_t)rp >> 2) & 3);
    const int head = min(V, (4 - mis) & 3);
    const int nvec = (V - head) >> 2;
    if (tid < head) take(tid, rp[tid]);
    const float4* vp = (const float4*)(rp + head);
    for (int j = tid; j < nvec; j += kSelThreads) {
      const float4 x = vp[j];
      const int i = head + 4 * j;
      take(i, x.x); take(i + 1, x.y); take(i + 2, x.z); take(i + 3, x.w);
    }
    const int i = head + 4 * nvec + tid;
    if (i < V) take(i, rp[i]);
    if (sampling)  // pad to whole 1024-entry tiles (4 waves x 64 lanes x 4): never kept
      for (int p = V + tid; p < ((V + 1023) & ~1023); p += kSelThreads) row[p] = -INFINITY;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(best, o, 64);
    best = t > best ? t : best;
  }
  if (lane == 0) best_w[wave] = best;
  __syncthreads();
  for (int w = 0; w < 4; ++w) best = best_w[w] > best ? best_w[w] : best;
  const int gid = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFu));
  const unsigned gkey = (unsigned)(best >> 32);
  // greedy; also a sampling row whose maximum is a NaN or an infinity
  if (!sampling || gkey >= 0xFF800000u || gkey <= 0x007FFFFFu) {
    if (tid == 0) write_id(a, b, ri, gid);
    return;
  }
  // The maximum, rebuilt from its key in registers (order_key inverted; -0 comes back as +0).
  // Not read from row[gid]: that entry lies in some other wave's quarter, which phase 2
  // overwrites, and with top_k >= V no barrier stands between here and phase 2.
  // Cross-wave accesses of `row` and the barrier that orders each before phase 2's overwrite:
  //   phase 0's stores (any thread, any entry)  - the barrier after best_w above;
  //   phase 1's radix passes (every thread reads the whole row) - the barrier that ends each
  //     pass (a thread leaves a pass only after all threads finished its reads).
  // The tie walk of phase 1, phase 2 and phase 3 touch the wave's own quarter only.
  const float xmax = __uint_as_float((gkey & 0x80000000u) ? (gkey ^ 0x80000000u) : ~gkey);

  // ---- 1: the top-k threshold ------------------------------------------------------------
  // kept: key > tk, or key == tk and index <= cut
  unsigned tk = 0;
  int cut = V - 1;
  const int k = (a.top_k <= 0 || a.top_k >= V) ? V : a.top_k;
  if (k < V) {
    unsigned prefix = 0, need = (unsigned)k;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      hist[tid] = 0;
      __syncthreads();
      for (int i0 = 4 * tid; i0 < V; i0 += 4 * kSelThreads) {  // 16-B LDS reads; the pad is initialised
        const float4 v = *(const float4*)&row[i0];
        const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned key = order_key(x[j]);
          if (i0 + j < V && (pass == 0 || (key >> (shift + 8)) == prefix))
            atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
      }
      __syncthreads();
      if (wave == 0) {
        // lane l owns bins 4l .. 4l+3; `above`: entries in higher bins
        const uint4 h = ((const uint4*)hist)[lane];
        const unsigned s = h.x + h.y + h.z + h.w;
        unsigned suf = s;
        for (int o = 1; o < 64; o <<= 1) {
          const unsigned t = __shfl_down(suf, o, 64);
          if (lane + o < 64) suf += t;
        }
        unsigned above = suf - s;
        const unsigned c[4] = {h.w, h.z, h.y, h.x};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (above < need && need <= above + c[j]) {  // exactly one (lane, j)
            sel[0] = 4u * lane + (3 - j);
            sel[1] = above;
          }
          above += c[j];
        }
      }
      __syncthreads();
      prefix = (prefix << 8) | sel[0];
      need -= sel[1];
    }
    tk = prefix;
    const unsigned ties = hist[tk & 255u];
    if (need < ties) {
      // only the first `need` of the entries equal to the threshold are kept: find the
      // index of the last of them (each wave counts its quarter, one walks it again)
      const int seg = (((V + 3) >> 2) + 255) & ~255;
      const int lo = wave * seg, hi = min(V, lo + seg);
      int cnt = 0;
      for (int t = lo; t < hi; t += 64) {
        const int i = t + lane;
        cnt += __popcll(__ballot(i < hi && order_key(row[i]) == tk));
      }
      if (lane == 0) ties_w[wave] = cnt;
      __syncthreads();
      int run = 0;
      for (int w = 0; w < wave; ++w) run += ties_w[w];
      if (run < (int)need && (int)need <= run + cnt) {
        for (int t = lo; t < hi; t += 64) {
          const int i = t + lane;
          unsigned long long m = __ballot(i < hi && order_key(row[i]) == tk);
          const int c = __popcll(m);
          if (run + c >= (int)need) {
            for (int q = (int)need - run; q > 1; --q) m &= m - 1;
            if (lane == 0) cut_s = t + __ffsll((long long)m) - 1;
            break;
          }
          run += c;
        }
      }
      __syncthreads();
      cut = cut_s;
    }
  }

  // ---- 2: e_i over the kept set, its sum -------------------------------------------------
  const int seg = (((V + 3) >> 2) + 255) & ~255;  // a wave's quarter, whole 256-entry tiles
  const int lo = wave * seg, hi = min(V, lo + seg);
  const float T = a.temperature;
  float lsum = 0.f;
  int last = -1;
  for (int t = lo; t < hi; t += 256) {
    const int i0 = t + 4 * lane;
    float4 v = *(const float4*)&row[i0];
    float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = i0 + j;
      const unsigned key = order_key(e[j]);
      const bool keep = i < V && (key > tk || (key == tk && i <= cut));
      e[j] = keep ? expf((e[j] - xmax) / T) : 0.f;
      lsum += e[j];
      last = e[j] > 0.f ? i : last;  // the fallback never returns an entry of p = 0
    }
    *(float4*)&row[i0] = make_float4(e[0], e[1], e[2], e[3]);
  }
  lsum = wave_sum(lsum);
  for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
  if (lane == 0) { sum_w[wave] = lsum; last_w[wave] = last; }
  __syncthreads();

  // ---- 2p: top-p and min-p over the e_i ----------------------------------------------------
  // The e_i are >= 0 and <= 1, so their bit patterns order as unsigned integers and are below
  // 2^30: the key is the pattern shifted left by 2 (the first 8-bit digit then spreads over the
  // low exponent bits). N: key > tp, or key == tp and index <= pcut; M: e_i >= min_p.
  if constexpr (NUCLEUS) {
    __shared__ __attribute__((aligned(16))) unsigned long long mass[256];
    __shared__ unsigned long long need_s;
    unsigned tp = 0;
    int pcut = V - 1;
    if (a.top_p < 1.f) {
      // The threshold by the radix select of phase 1 on mass instead of count: the mass of an
      // entry is the integer q_i = trunc(e_i 2^40) <= 2^40, so a bin's mass (below 2^55) does not
      // depend on the order of the atomics. Entries of q = 0 (e_i < 2^-40) weigh nothing.
      unsigned prefix = 0;
      unsigned long long need = 0;
      for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        mass[tid] = 0;
        __syncthreads();
        for (int i0 = 4 * tid; i0 < V; i0 += 4 * kSelThreads) {
          const float4 v = *(const float4*)&row[i0];
          const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (i0 + j >= V) continue;
            const unsigned key = __float_as_uint(x[j]) << 2;
            const unsigned long long q = (unsigned long long)(x[j] * 0x1p40f);
            if (q != 0 && (pass == 0 || (key >> (shift + 8)) == prefix)) atomicAdd(&mass[(key >> shift) & 255u], q);
          }
        }
        __syncthreads();
        if (wave == 0) {
          // lane l owns bins 4l .. 4l+3; `above`: the mass in higher bins
          const unsigned long long h[4] = {mass[4 * lane], mass[4 * lane + 1], mass[4 * lane + 2], mass[4 * lane + 3]};
          const unsigned long long s4 = h[0] + h[1] + h[2] + h[3];
          unsigned long long suf = s4;
          for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long t = __shfl_down(suf, o, 64);
            if (lane + o < 64) suf += t;
          }
          if (pass == 0) {
            // the smallest integer mass that reaches top_p Q, Q = sum of all q_i >= 2^40
            const unsigned long long Q = __shfl(suf, 0, 64);
            const double want = ceil((double)a.top_p * (double)Q);
            need = want < 1.0 ? 1ull : (unsigned long long)want;
            need = need > Q ? Q : need;
          }
          unsigned long long above = suf - s4;
#pragma unroll
          for (int j = 3; j >= 0; --j) {
            if (above < need && need <= above + h[j]) {  // exactly one (lane, j)
              sel[0] = 4u * lane + j;
              need_s = need - above;
            }
            above += h[j];
          }
        }
        __syncthreads();
        prefix = (prefix << 8) | sel[0];
        need = need_s;
      }
      tp = prefix;
      // every entry of the threshold's class weighs qt: the first n_need of them, in index order
      const unsigned long long qt = (unsigned long long)(__uint_as_float(tp >> 2) * 0x1p40f);
      const unsigned long long n_need = (need + qt - 1) / qt;
      if (n_need * qt != mass[tp & 255u])
        pcut = tie_cut([&](int i) { return __float_as_uint(row[i]) == (tp >> 2); }, lo, hi, (int)n_need, lane, wave,
                       ties_w, &cut_s);
    }
    // zero what falls outside N and M; the wave totals again, in phase 2's order
    const unsigned tpb = tp >> 2;
    const float floor_e = a.min_p;
    lsum = 0.f;
    last = -1;
    for (int t = lo; t < hi; t += 256) {
      const int i0 = t + 4 * lane;
      float4 v = *(const float4*)&row[i0];
      float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = i0 + j;
        const unsigned bits = __float_as_uint(e[j]);
        const bool keep = (bits > tpb || (bits == tpb && i <= pcut)) && e[j] >= floor_e;
        e[j] = keep ? e[j] : 0.f;
        lsum += e[j];
        last = e[j] > 0.f ? i : last;
      }
      *(float4*)&row[i0] = make_float4(e[0], e[1], e[2], e[3]);
    }
    lsum = wave_sum(lsum);
    for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
    if (lane == 0) { sum_w[wave] = lsum; last_w[wave] = last; }
    __syncthreads();
  }
  float total = 0.f, run = 0.f;
  for (int w = 0; w < 4; ++w) {
    if (w == wave) run = total;
    total += sum_w[w];
  }
  const uint64_t seed = (a.seed_dev ? *a.seed_dev : a.seed) + (a.count ? (uint64_t)((int64_t)a.count[b] + ri) : 0ull);
  const float target = uniform24(seed, b) * total;

  // ---- 3: the first entry whose running sum exceeds u * total ------------------------------
  int found = 0x7FFFFFFF;
  for (int t = lo; t < hi; t += 256) {
    const int i0 = t + 4 * lane;
    const float4 v = *(const float4*)&row[i0];
    const float s1 = v.x, s2 = s1 + v.y, s3 = s2 + v.z, s4 = s3 + v.w;
    if (__ballot(s4 != 0.f) == 0) continue;
    float sc = s4;
    for (int o = 1; o < 64; o <<= 1) {
      const float up = __shfl_up(sc, o, 64);
      if (lane >= o) sc += up;
    }
    float ex = __shfl_up(sc, 1, 64);
    if (lane == 0) ex = 0.f;
    // running sums run + (ex + s_j): an entry of zero repeats its predecessor's sum exactly
    const bool c1 = run + (ex + s1) > target && v.x > 0.f, c2 = run + (ex + s2) > target && v.y > 0.f,
               c3 = run + (ex + s3) > target && v.z > 0.f, c4 = run + (ex + s4) > target && v.w > 0.f;
    const unsigned long long m = __ballot(c1 || c2 || c3 || c4);
    if (m) {
      const int first = __ffsll((long long)m) - 1;
      const int mine = i0 + (c1 ? 0 : c2 ? 1 : c3 ? 2 : 3);
      found = __shfl(mine, first, 64);
      break;
    }
    run += __shfl(sc, 63, 64);
  }
  if (lane == 0) cand_w[wave] = found;
  __syncthreads();
  if (tid == 0) {
    int id = min(min(cand_w[0], cand_w[1]), min(cand_w[2], cand_w[3]));
    if (id == 0x7FFFFFFF) id = max(max(last_w[0], last_w[1]), max(last_w[2], last_w[3]));
    write_id(a, b, ri, id);
  }
}

hipError_t launch_select(const SelectArgs& a, int64_t B, hipStream_t st) {
  const dim3 grid((unsigned)(B * a.rows)), block(kSelThreads);
  // greedy ignores both filters; at their off values the kernel without the phase runs
  if (a.temperature > 0.f && (a.top_p < 1.f || a.min_p > 0.f)) {
    if (a.V <= 4096) select_token_kernel<4096, true><<<grid, block, 0, st>>>(a);
    else if (a.V <= 16384) select_token_kernel<16384, true><<<grid, block, 0, st>>>(a);
    else select_token_kernel<kSelMaxV, true><<<grid, block, 0, st>>>(a);
    return hipGetLastError();
  }
  if (a.V <= 4096) select_token_kernel<4096, false><<<grid, block, 0, st>>>(a);
  else if (a.V <= 16384) select_token_kernel<16384, false><<<grid, block, 0, st>>>(a);
  else select_token_kernel<kSelMaxV, false><<<grid, block, 0, st>>>(a);
  return hipGetLastError();
}

// top_p in (0, 1], min_p in [0, 1]; a NaN fails both
int check_nucleus(const char* who, float top_p, float min_p) {
  if (!(top_p > 0.f && top_p <= 1.f)) return set_error("%s: top_p must be in (0, 1] (got %g)", who, (double)top_p);
  if (!(min_p >= 0.f && min_p <= 1.f)) return set_error("%s: min_p must be in [0, 1] (got %g)", who, (double)min_p);
  return 0;
}
}  // namespace mt

using namespace mt;

static int select_token_impl(const char* who, const float* logits, int64_t B, int64_t V, int64_t row_stride,
                             float temperature, int64_t top_k, float top_p, float min_p, uint64_t seed,
                             const uint64_t* seed_dev, int64_t eos_id, float* next_f32, int32_t* next_i32,
                             int32_t* done, int32_t* history, int64_t history_stride, const int32_t* step_dev,
                             void* stream) {
  if (B <= 0 || V <= 0) return set_error("%s: bad sizes B=%lld V=%lld", who, (long long)B, (long long)V);
  if (V > kSelMaxV)
    return set_error("%s: V=%lld is above the limit of %d (the row is held in LDS)", who, (long long)V, kSelMaxV);
  if (B > (1ll << 31) - 1) return set_error("%s: B=%lld out of range", who, (long long)B);
  if (row_stride < V)
    return set_error("%s: row_stride %lld is below V=%lld", who, (long long)row_stride, (long long)V);
  if (!(temperature >= 0.f)) return set_error("%s: temperature must be >= 0 (got %g)", who, (double)temperature);
  if (!logits) return set_error("%s: logits is NULL", who);
  if ((uintptr_t)logits & 3) return set_error("%s: logits is not 4-B aligned", who);
  if (!next_f32 && !next_i32) return set_error("%s: both outputs (next_f32, next_i32) are NULL", who);
  if (history && !step_dev) return set_error("%s: history needs step_dev", who);
  if (history && history_stride <= 0)
    return set_error("%s: history_stride %lld must be positive", who, (long long)history_stride);
  if (check_nucleus(who, top_p, min_p)) return 1;
  SelectArgs a;
  a.logits = logits; a.row_stride = row_stride; a.V = (int)V;
  a.top_k = (int)(top_k <= 0 || top_k >= V ? 0 : top_k);
  a.temperature = temperature; a.seed = seed; a.seed_dev = seed_dev; a.eos_id = eos_id;
  a.next_f32 = next_f32; a.next_i32 = next_i32; a.done = done;
  a.history = history; a.history_stride = history_stride; a.step_dev = step_dev;
  a.rows = 1; a.batch_stride = row_stride; a.count = nullptr; a.skip = nullptr; a.scratch = nullptr;
  a.top_p = top_p; a.min_p = min_p;
  return check_hip(launch_select(a, B, (hipStream_t)stream), who);
}

extern "C" int mt_select_token(const float* logits, int64_t B, int64_t V, int64_t row_stride,
                               float temperature, int64_t top_k, uint64_t seed, const uint64_t* seed_dev,
                               int64_t eos_id, float* next_f32, int32_t* next_i32, int32_t* done,
                               int32_t* history, int64_t history_stride, const int32_t* step_dev,
                               void* stream) {
  return select_token_impl("mt_select_token", logits, B, V, row_stride, temperature, top_k, 1.f, 0.f, seed, seed_dev,
                           eos_id, next_f32, next_i32, done, history, history_stride, step_dev, stream);
}

extern "C" int mt_select_token_p(const float* logits, int64_t B, int64_t V, int64_t row_stride,
                                 float temperature, int64_t top_k, float top_p, float min_p, uint64_t seed,
                                 const uint64_t* seed_dev, int64_t eos_id, float* next_f32, int32_t* next_i32,
                                 int32_t* done, int32_t* history, int64_t history_stride,
                                 const int32_t* step_dev, void* stream) {
  return select_token_impl("mt_select_token_p", logits, B, V, row_stride, temperature, top_k, top_p, min_p, seed,
                           seed_dev, eos_id, next_f32, next_i32, done, history, history_stride, step_dev, stream);
}
