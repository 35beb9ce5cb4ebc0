// Extend attention: Nq new query rows per (batch, head) at the END of a row of n cached keys,
// with n and the count t of real queries per batch row read on the device (mt_flash_attn_extend,
// include/minitorch_hip.h). The decode contract (csrc/fa_decode.hip: the causal mask aligned
// bottom-right, cache rows >= n never read) on the MFMA structure of the forward's
// fa_fwd_generic_ring (csrc/fa_fwd.hip), for any Nq <= Nk.
//
//  * A 256-thread workgroup (4 waves) owns BQ = 128 queries of one (b, h), 32 per wave, in
//    registers; K / V tiles of BK keys go through a two-slot LDS ring, one barrier per tile.
//    The grid is ceil(Nq / BQ) x B*H workgroups in the XCD-aware order of the forward kernels
//    (the blocks of one (b, h), and with grouped-query attention the heads of one group, which
//    are neighbours in that order, find their K / V in one L2). It depends on the sizes only.
//  * Query on the lane: S^T = K Q^T puts one query per lane column, so the number of keys a
//    query sees, lim = i < t ? clamp(n - t + 1 + i, 0, n) : 0 (n when not causal), is one
//    lane-local scalar and the mask is the single compare key >= lim.
//  * Work skipping from the device values: a workgroup whose first query is >= t loads nothing
//    and stores (0, -inf, 0); the key loop ends at the block's largest lim; a wave whose 32
//    queries all end before a tile skips it.
//  * Rows that must not be read (cache rows >= the block's largest lim, Q rows >= t) are
//    replaced by zeros through a predicated load, their logits by -inf through a select.
//  * fp32, d <= 64 (X3): both products on the bf16 MFMA with three bf16 pieces per operand
//    (fa_common.h mma_x3); each tile's PV goes to a fresh accumulator and joins the running O
//    by a VALU fma, because the bf16 MFMA's accumulation rounds toward -inf (x3_tile_sum).
//    fp32, 64 < d <= 256: the fp32 MFMA. bf16: the bf16 MFMA with P rounded to bf16.
//  * int64 addressing; plain stores only; no workspace.
#include <type_traits>

#include "fa_extend.h"

namespace mt {

template <typename T, int DT, int DV, int KB, bool X3, int MINB>
__global__ __launch_bounds__(256, MINB) void fa_extend_ring(ExtendArgs p) {
  static_assert(!X3 || std::is_same<T, float>::value, "x3: fp32 inputs");
  static_assert(DT % DV == 0 && (!X3 || DV == DT), "O column slices");
  constexpr int BQ = 128, BK = 32 * KB;
  constexpr int NZ = DT / DV;        // O column slices: a workgroup per slice, each recomputing S
  constexpr int PAD = 16 / sizeof(T);
  constexpr int LD = DT + PAD, LDV = DV + PAD;
  constexpr int SLOT = BK * (LD + LDV);  // K then V
  constexpr int LDB = DT + 8;        // X3: a bf16 plane's row (elements)
  constexpr int PLANE = BK * LDB;    // X3: one bf16 plane (elements); a slot is K h, m, l, V h, m, l
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* ring = (T*)smem;
  bf16* ring3 = (bf16*)smem;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hf = lane >> 5, c32 = lane & 31;
  const int d = p.d;
  // XCD-aware order over the flat grid (fa_common.h xcd_order): consecutive workgroups go to the
  // 8 XCDs in turn, so each XCD is dealt one contiguous run of (b, h, block)
  int blk, bh, oc;  // oc: first O / V column of this workgroup's slice
  {
    const int nblk = gridDim.x, hw = blockIdx.x;
    const int xcd = hw & 7, slot = hw >> 3, qd = nblk >> 3, rm = nblk & 7;
    const int logical = (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + slot;
    blk = (logical / NZ) % p.nqb;
    bh = logical / (NZ * p.nqb);
    oc = (logical % NZ) * DV;
  }
  const int b = bh / p.H, hh = bh % p.H, hkv = hh / (p.H / p.Hkv);
  const T* Qg = (const T*)p.q + b * p.qs[0] + hh * p.qs[1];
  const T* Kg = (const T*)p.k + b * p.ks[0] + hkv * p.ks[1];
  const T* Vg = (const T*)p.v + b * p.vs[0] + hkv * p.vs[1];
  constexpr int EPC = 16 / sizeof(T), CPR = DT / EPC, NCK = BK * CPR / 256;
  constexpr int CPV = DV / EPC, NCV = BK * CPV / 256;

  // n keys held, t real queries: query i < t sits at position n - t + i
  const int n = p.kv_len ? max(0, min(p.Nk, p.kv_len[b])) : p.Nk;
  const int t = p.q_len ? max(0, min(p.Nq, p.q_len[b])) : p.Nq;
  const int causal = p.causal;
  auto lim_of = [&](int i) __attribute__((always_inline)) {
    return i < t ? (causal ? max(0, min(n, n - t + 1 + i)) : n) : 0;
  };
  const int q0 = blk * BQ;
  const int my_q = q0 + wave * 32 + c32;
  const int my_lim = lim_of(my_q);
  // lim does not decrease over the real queries: the block's / wave's largest is its last real
  // query's, the wave's smallest its first query's (0 when the wave holds a padding query)
  const int kend = q0 < t ? lim_of(min(q0 + BQ, t) - 1) : 0;
  const int wq0 = q0 + wave * 32;
  const int wave_limmax = wq0 < t ? lim_of(min(wq0 + 32, t) - 1) : 0;
  const int wave_limmin = wq0 + 31 < t ? lim_of(wq0) : 0;

  // Q row my_q, k-step ks: elements 16 ks + 8 hf .. +7, zero past d and for a query >= t
  Frag<T> bq[X3 ? 1 : DT / 16];
  X3Frag bq3[X3 ? DT / 16 : 1];
  {
    const T* qrow = Qg + (int64_t)my_q * p.qs[2];
#pragma unroll
    for (int ks = 0; ks < DT / 16; ++ks) {
      uint4 ch[8 / EPC];
#pragma unroll
      for (int j = 0; j < 8 / EPC; ++j) {
        const int col = 16 * ks + 8 * hf + j * EPC;
        ch[j] = make_uint4(0, 0, 0, 0);
        if (my_q < t && col < d) ch[j] = *(const uint4*)(qrow + col);
      }
      if constexpr (X3)
        bq3[ks] = x3_split(__builtin_bit_cast(f32x8, ch));
      else
        bq[ks] = __builtin_bit_cast(Frag<T>, ch);
    }
  }

  float m_run = -INFINITY, l_run = 0.f;
  f32x16 O[DV / 32];
#pragma unroll
  for (int i = 0; i < DV / 32; ++i) O[i] = f32x16{};

  const int ntiles = (kend + BK - 1) / BK;

  uint4 pk[NCK], pv[NCV];
  auto pre_load = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NCK; ++i) {
      const int ch = tid + 256 * i, r = ch / CPR, cc = (ch % CPR) * EPC, gr = k0 + r;
      pk[i] = make_uint4(0, 0, 0, 0);
      if (gr < kend && cc < d) pk[i] = *(const uint4*)(Kg + (int64_t)gr * p.ks[2] + cc);
    }
#pragma unroll
    for (int i = 0; i < NCV; ++i) {
      const int ch = tid + 256 * i, r = ch / CPV, cc = oc + (ch % CPV) * EPC, gr = k0 + r;
      pv[i] = make_uint4(0, 0, 0, 0);
      if (gr < kend && cc < d) pv[i] = *(const uint4*)(Vg + (int64_t)gr * p.vs[2] + cc);
    }
  };
  auto pre_store = [&](int s) __attribute__((always_inline)) {
    if constexpr (X3) {  // three bf16 planes per tensor: 8 B of each per 16-B chunk
      bf16* sl = ring3 + s * 6 * PLANE;
#pragma unroll
      for (int i = 0; i < NCK; ++i) {
        const int ch = tid + 256 * i, r = ch / CPR, cc = (ch % CPR) * EPC;
        x3_store4(sl + r * LDB + cc, PLANE, pk[i]);
        x3_store4(sl + 3 * PLANE + r * LDB + cc, PLANE, pv[i]);
      }
      return;
    }
    T* sK = ring + s * SLOT;
    T* sV = sK + BK * LD;
#pragma unroll
    for (int i = 0; i < NCK; ++i) {
      const int ch = tid + 256 * i, r = ch / CPR, cc = (ch % CPR) * EPC;
      *(uint4*)(sK + r * LD + cc) = pk[i];
    }
#pragma unroll
    for (int i = 0; i < NCV; ++i) {
      const int ch = tid + 256 * i, r = ch / CPV, cc = (ch % CPV) * EPC;
      *(uint4*)(sV + r * LDV + cc) = pv[i];
    }
  };
  if (ntiles > 0) {
    pre_load(0);
    pre_store(0);
    if (ntiles > 1) pre_load(BK);
  }
  __syncthreads();

  for (int ti = 0; ti < ntiles; ++ti) {
    const int k0 = ti * BK;
    const T* sK = ring + (ti & 1) * SLOT;
    const T* sV = sK + BK * LD;
    const bf16* sK3 = ring3 + (ti & 1) * 6 * PLANE;  // X3: K h, m, l planes, then V's
    const bf16* sV3 = sK3 + 3 * PLANE;
    if (k0 < wave_limmax) {
      f32x16 S[KB];
#pragma unroll
      for (int i = 0; i < KB; ++i) S[i] = f32x16{};
#pragma unroll
      for (int ks = 0; ks < DT / 16; ++ks) {
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
          if constexpr (X3) {
            const X3Frag ak = x3_rows(sK3 + (kb * 32 + c32) * LDB + ks * 16 + 8 * hf, PLANE);
            mma_x3(S[kb], ak, bq3[ks]);
          } else {
            Frag<T> ak = row_frag<T>(sK + (kb * 32 + c32) * LD + ks * 16 + 8 * hf);
            mma(S[kb], ak, bq[ks]);
          }
        }
      }
      // the mask only on tiles that reach past the wave's smallest lim; the row max is taken on
      // the raw scores (the scale c2 > 0), and exp2(c2 s - m) is one fma into one v_exp_f32
      const float c2 = p.scale_log2;
      if (k0 + BK > wave_limmin) {
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = k0 + kb * 32 + acc_row(r, hf);
            if (key >= my_lim) S[kb][r] = -INFINITY;
          }
      }
      float smax = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) smax = fmaxf(smax, S[kb][r]);
      smax = fmaxf(smax, __shfl_xor(smax, 32));
      const float m_new = fmaxf(m_run, smax * c2);
      const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
      float rs = 0.f;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(S[kb][r], c2, -m_use));
          S[kb][r] = e;
          rs += e;
        }
      l_run = l_run * alpha + rs;
      m_run = m_new;
      // X3: the tile's PV in its own accumulator, added to the running O by a VALU fma
      f32x16 Ot[X3 ? DV / 32 : 1];
      if constexpr (X3) {
#pragma unroll
        for (int i = 0; i < DV / 32; ++i) Ot[i] = f32x16{};
      } else {
#pragma unroll
        for (int i = 0; i < DV / 32; ++i) O[i] *= alpha;
      }
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if constexpr (X3) {
            const X3Frag bp = x3_split(acc_frag<float>(S[kb], s));
#pragma unroll
            for (int db = 0; db < DV / 32; ++db) {
              const X3Frag av = x3_cols(sV3, PLANE, LDB, kb * 32 + 16 * s + 4 * hf, db * 32, lane);
              mma_x3(Ot[db], av, bp);
            }
            continue;
          }
          Frag<T> bp = acc_frag<T>(S[kb], s);
#pragma unroll
          for (int db = 0; db < DV / 32; ++db) {
            Frag<T> av = col_frag<T>(sV, LDV, kb * 32 + 16 * s + 4 * hf, db * 32, lane);
            mma(O[db], av, bp);
          }
        }
      if constexpr (X3) {
#pragma unroll
        for (int i = 0; i < DV / 32; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) O[i][r] = __builtin_fmaf(O[i][r], alpha, Ot[i][r]);
      }
    }
    if (ti + 1 < ntiles) {
      pre_store((ti + 1) & 1);
      if (ti + 2 < ntiles) pre_load(k0 + 2 * BK);
    }
    __syncthreads();
  }

  // a query with no visible key (or >= t) stores O = 0, m = -inf, l = 0 exactly
  const float l_tot = l_run + __shfl_xor(l_run, 32);
  const bool some = l_tot > 0.f;
  const float inv_l = some ? 1.f / l_tot : 0.f;
  if (my_q < p.Nq) {
    const int64_t oe = b * p.os[0] + hh * p.os[1] + (int64_t)my_q * p.os[2];
    T* Og = (T*)p.o + oe;
    float* Of = (float*)p.o + oe;  // bf16 inputs with an fp32 output (o_f32)
    const bool f32o = !std::is_same<T, float>::value && p.o_f32;
#pragma unroll
    for (int db = 0; db < DV / 32; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int col = oc + db * 32 + 8 * g + 4 * hf;  // d is a multiple of 4
        float a[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = some ? O[db][4 * g + e] * inv_l : 0.f;
        if (col < d && f32o)
          store4(Of + col, a[0], a[1], a[2], a[3], true);
        else if (col < d)
          store4(Og + col, a[0], a[1], a[2], a[3], true);
      }
    if (hf == 0 && oc == 0) {
      const int64_t row = (int64_t)bh * p.Nq + my_q;
      if (p.m) p.m[row] = some ? m_run * kLn2 : -INFINITY;
      if (p.l) p.l[row] = some ? l_tot : 0.f;
    }
  }
}

template <typename T, int DT, int DV, int KB, bool X3, int MINB>
static hipError_t launch_extend_t(const ExtendArgs& a, int64_t B, hipStream_t st) {
  // two slots of K and V: fp32 / bf16 rows, or (X3) three bf16 planes each
  const size_t smem = X3 ? (size_t)2 * 6 * 32 * KB * (DT + 8) * 2
                         : sizeof(T) * (size_t)(DT + DV + 32 / sizeof(T)) * 2 * 32 * KB;
  auto kfn = fa_extend_ring<T, DT, DV, KB, X3, MINB>;
  hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)smem);
  if (e != hipSuccess) return e;
  dim3 grid((unsigned)(a.nqb * B * a.H * (DT / DV)), 1, 1);
  hipLaunchKernelGGL(kfn, grid, dim3(256), smem, st, a);
  return hipGetLastError();
}

// The instantiation for (element size, d): a function of the sizes only.
//   0 fp32 X3 DT 32 | 1 fp32 X3 DT 64 | 2 fp32 MFMA DT 128 | 3 fp32 MFMA DT 256
//   4 bf16 DT 32    | 5 bf16 DT 64    | 6 bf16 DT 128      | 7 bf16 DT 256
ExtendPlan extend_plan(int esize, int64_t d) {
  if (esize == 4) {
    if (d <= 32) return {0, 128, 32};
    if (d <= 64) return {1, 128, 32};
    if (d <= 128) return {2, 128, 32};
    return {3, 128, 32};
  }
  if (d <= 32) return {4, 128, 64};
  if (d <= 64) return {5, 128, 64};
  if (d <= 128) return {6, 128, 64};
  return {7, 128, 32};
}

hipError_t launch_extend(const ExtendArgs& a, bool bf16_in, int64_t B, hipStream_t st) {
  switch (extend_plan(bf16_in ? 2 : 4, a.d).kernel) {
    case 0: return launch_extend_t<float, 32, 32, 1, true, 2>(a, B, st);
    case 1: return launch_extend_t<float, 64, 64, 1, true, 2>(a, B, st);
    case 2: return launch_extend_t<float, 128, 128, 1, false, 2>(a, B, st);
    case 3: return launch_extend_t<float, 256, 128, 1, false, 1>(a, B, st);
    case 4: return launch_extend_t<bf16, 32, 32, 2, false, 2>(a, B, st);
    case 5: return launch_extend_t<bf16, 64, 64, 2, false, 2>(a, B, st);
    case 6: return launch_extend_t<bf16, 128, 128, 2, false, 2>(a, B, st);
    default: return launch_extend_t<bf16, 256, 256, 1, false, 1>(a, B, st);
  }
}

}  // namespace mt
