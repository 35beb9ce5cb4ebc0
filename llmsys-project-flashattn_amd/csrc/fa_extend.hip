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
//
// Where the K / V rows live and what they are made of is the kernel's source, Src, in the spirit of
// the decode kernel's (fa_decode_kernel.h). K and V enter the kernel in one place -- pre_load fetches
// a tile's chunks into registers, pre_store puts them into the LDS ring -- and a source supplies only
// what differs there, on two axes that compose:
//   place   ExtContig / ExtPaged: the address of key row gr. A paged row goes through the block
//           table entry of its own key, resolved per loaded row (a page may be smaller or larger
//           than the tile), loaded under the row's predicate and clamped into [0, n_pages): no table
//           entry at index >= ceil(n / P) and no pool row of a key >= the block's kend is read, and
//           a table that breaks the contract reads a wrong page of the pool, never memory outside it
//   format  ExtRows<T>: fp32 / bf16 rows in 16-B chunks, staged as they are. ExtQuant<KV>: bf16 /
//           fp8 rows in 8-element chunks (kKvqEpc), kept as loaded until pre_store and widened there
//           to fp32 with kvq_dequant's formulas (KV::unpack, for fp8 one fp32 product with the row's
//           scale, loaded under the row's predicate), so the ring holds what it would hold after
//           mt_kv_cache_dequant and the kernel is the fp32 one from there on
// Everything after the ring -- limits, masks, X3 planes, MFMA order, online softmax, epilogue -- is
// below, once: the same bits for the same rows however they are stored. Instantiated: ExtPlainSrc<T>
// (contiguous rows: mt_flash_attn_extend), ExtPagedSrc<T> (mt_flash_attn_extend_paged) and
// ExtKvqSrc<KV> (mt_flash_attn_extend_kvq); a paged and quantised source would be a fourth.
// Resources of every instantiation: profiles/extend_kernels_resources.txt.
#include <type_traits>

#include "fa_extend.h"
#include "fa_kvq.h"

namespace mt {

// ---- place: the address of a key row ------------------------------------------------------------
// Row: what row(gr, live) resolves for key gr (live: the row may be read) ahead of the tile's loads;
// head(p, b, hkv, s): this kv head's rows (of page 0); at(base, s, gr, row): the row's first element
struct ExtContig {
  using Row = int;
  template <typename E>
  static __device__ __forceinline__ const E* head(const E* p, int b, int hkv, const int64_t* s) {
    return p + b * s[0] + hkv * s[1];
  }
  __device__ __forceinline__ Row row(int gr, bool) const { return gr; }
  template <typename E>
  __device__ __forceinline__ const E* at(const E* base, const int64_t* s, int gr, Row) const {
    return base + (int64_t)gr * s[2];
  }
};
struct ExtPaged {
  using Row = int;  // the page
  const int* tb;    // this batch row's table entries
  int lgP, pmask, pmax;
  template <typename E>
  static __device__ __forceinline__ const E* head(const E* p, int, int hkv, const int64_t* s) { return p + hkv * s[1]; }
  __device__ __forceinline__ Row row(int gr, bool live) const {
    int pg = 0;
    if (live) pg = (int)min((unsigned)tb[gr >> lgP], (unsigned)pmax);  // a negative entry: the last page
    return pg;
  }
  template <typename E>
  __device__ __forceinline__ const E* at(const E* base, const int64_t* s, int gr, Row pg) const {
    return base + (int64_t)pg * s[0] + (int64_t)(gr & pmask) * s[2];
  }
};

// ---- format: what a row is made of ----------------------------------------------------------------
// T: the element type of Q and of the ring; E: a storage element (the unit of ks / vs); Raw: a chunk
// of EPC elements as loaded; stage(): the 16-B ring chunks (EPC * sizeof(T) / 16 of them) it becomes
template <typename T_> struct ExtRows {
  using T = T_;
  using E = T_;
  using Raw = uint4;
  static constexpr int EPC = 16 / sizeof(T_);
  static constexpr bool kScaled = false;
  static __device__ __forceinline__ Raw zero() { return make_uint4(0, 0, 0, 0); }
  static __device__ __forceinline__ void stage(const Raw& u, float, uint4* out) { out[0] = u; }
};
template <typename KV> struct ExtQuant {
  using T = float;
  using E = typename std::conditional<KV::kBytes == 2, bf16, unsigned char>::type;
  using Raw = typename KV::Raw;
  static constexpr int EPC = kKvqEpc;
  static constexpr bool kScaled = KV::kScaled;
  static __device__ __forceinline__ Raw zero() { return KV::zero(); }
  static __device__ __forceinline__ void stage(const Raw& u, float s, uint4* out) {
    float f[kKvqEpc];
    KV::unpack(u, f);
    if constexpr (KV::kScaled) {
      // the product is rounded to fp32 here, as kvq_dequant stores it: the empty asm keeps the X3 split
      // behind it (x - top half of x) from contracting it into an fma on the unrounded product
#pragma unroll
      for (int e = 0; e < kKvqEpc; ++e) {
        f[e] *= s;
        asm("" : "+v"(f[e]));
      }
    }
    out[0] = __builtin_bit_cast(uint4, make_float4(f[0], f[1], f[2], f[3]));
    out[1] = __builtin_bit_cast(uint4, make_float4(f[4], f[5], f[6], f[7]));
  }
};

// ---- the instantiated sources ---------------------------------------------------------------------
// Args, base(args): the kernel's argument struct and the ExtendArgs in it; place; scale(which, gr):
// the fp32 scale of K (0) / V (1) row gr, for a scaled format; kPlain: contiguous rows staged as loaded.
// For kPlain, pre_load and pre_store keep the statements the kernel had before it took a source instead
// of going through place / stage: the same arithmetic either way, but through the general path the eight
// plain kernels came out with another instruction order (same counts, registers and occupancy) and ran
// 1-1.5 % slower at fp32 d = 64 and bf16 d = 128; spelled this way their device code is the earlier
// kernel's instruction for instruction
template <typename T> struct ExtPlainSrc : ExtRows<T> {
  using Args = ExtendArgs;
  static constexpr bool kPlain = true;
  static __host__ __device__ __forceinline__ const ExtendArgs& base(const Args& sa) { return sa; }
  ExtContig place;
  __device__ __forceinline__ ExtPlainSrc(const Args&, int, int) {}
  __device__ __forceinline__ float scale(int, int) const { return 0.f; }
};
template <typename T> struct ExtPagedSrc : ExtRows<T> {
  using Args = PagedExtendArgs;
  static constexpr bool kPlain = false;
  static __host__ __device__ __forceinline__ const ExtendArgs& base(const Args& sa) { return sa.e; }
  ExtPaged place;
  __device__ __forceinline__ ExtPagedSrc(const Args& sa, int b, int)
      : place{sa.table + (int64_t)b * sa.W, sa.lgP, (1 << sa.lgP) - 1, sa.n_pages - 1} {}
  __device__ __forceinline__ float scale(int, int) const { return 0.f; }
};
template <typename KV> struct ExtKvqSrc : ExtQuant<KV> {
  using Args = KvqExtendArgs;
  static constexpr bool kPlain = false;
  static __host__ __device__ __forceinline__ const ExtendArgs& base(const Args& sa) { return sa.e; }
  ExtContig place;
  const float* sc[2];  // this (b, hkv)'s row scales
  __device__ __forceinline__ ExtKvqSrc(const Args& sa, int b, int hkv)
      : sc{nullptr, nullptr} {
    if constexpr (KV::kScaled) {  // an unscaled format has no scale arrays (NULL)
      sc[0] = sa.kscale + ((int64_t)b * sa.e.Hkv + hkv) * sa.e.Nk;
      sc[1] = sa.vscale + ((int64_t)b * sa.e.Hkv + hkv) * sa.e.Nk;
    }
  }
  __device__ __forceinline__ float scale(int which, int gr) const { return sc[which][gr]; }
};

template <typename Src, int DT, int DV, int KB, bool X3, int MINB>
__global__ __launch_bounds__(256, MINB) void fa_extend_ring(const typename Src::Args sa) {
  using T = typename Src::T;
  using E = typename Src::E;
  using Raw = typename Src::Raw;
  const ExtendArgs& p = Src::base(sa);
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
  const Src src(sa, b, hkv);
  const E* Kg = src.place.head((const E*)p.k, b, hkv, p.ks);
  const E* Vg = src.place.head((const E*)p.v, b, hkv, p.vs);
  constexpr int EPC = 16 / sizeof(T);  // elements of a 16-B chunk of Q and of the ring
  // K / V chunks as the source loads them: SPC elements, SUB ring chunks each; a thread takes NCK of K
  // and NCV of V per tile (ALLK / ALLV: every thread has a chunk in each round)
  constexpr int SPC = Src::EPC, SUB = SPC / EPC;
  constexpr int CPR = DT / SPC, NCK = BK * CPR >= 256 ? BK * CPR / 256 : 1;
  constexpr int CPV = DV / SPC, NCV = BK * CPV >= 256 ? BK * CPV / 256 : 1;
  constexpr bool ALLK = BK * CPR >= 256, ALLV = BK * CPV >= 256;
  using Row = typename decltype(src.place)::Row;

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

  Raw pk[NCK], pv[NCV];
  float sk[Src::kScaled ? NCK : 1], sv[Src::kScaled ? NCV : 1];  // row scales: gone unless Src::kScaled
  auto pre_load = [&](int k0) __attribute__((always_inline)) {
    if constexpr (Src::kPlain) {  // see kPlain above
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
    } else {
      // the rows of the tile first (a paged source: its table entries), then their chunks
      Row rk[NCK], rv[NCV];
#pragma unroll
      for (int i = 0; i < NCK; ++i) {
        const int ch = tid + 256 * i, gr = k0 + ch / CPR;
        rk[i] = src.place.row(gr, (ALLK || ch < BK * CPR) && gr < kend);
      }
#pragma unroll
      for (int i = 0; i < NCV; ++i) {
        const int ch = tid + 256 * i, gr = k0 + ch / CPV;
        rv[i] = CPV == CPR ? rk[i] : src.place.row(gr, (ALLV || ch < BK * CPV) && gr < kend);
      }
#pragma unroll
      for (int i = 0; i < NCK; ++i) {
        const int ch = tid + 256 * i, r = ch / CPR, cc = (ch % CPR) * SPC, gr = k0 + r;
        pk[i] = Src::zero();
        if constexpr (Src::kScaled) sk[i] = 0.f;
        if ((ALLK || ch < BK * CPR) && gr < kend && cc < d) {
          pk[i] = *(const Raw*)(src.place.at(Kg, p.ks, gr, rk[i]) + cc);
          if constexpr (Src::kScaled) sk[i] = src.scale(0, gr);
        }
      }
#pragma unroll
      for (int i = 0; i < NCV; ++i) {
        const int ch = tid + 256 * i, r = ch / CPV, cc = oc + (ch % CPV) * SPC, gr = k0 + r;
        pv[i] = Src::zero();
        if constexpr (Src::kScaled) sv[i] = 0.f;
        if ((ALLV || ch < BK * CPV) && gr < kend && cc < d) {
          pv[i] = *(const Raw*)(src.place.at(Vg, p.vs, gr, rv[i]) + cc);
          if constexpr (Src::kScaled) sv[i] = src.scale(1, gr);
        }
      }
    }
  };
  auto pre_store = [&](int s) __attribute__((always_inline)) {
    if constexpr (Src::kPlain && X3) {  // see kPlain above
      bf16* sl = ring3 + s * 6 * PLANE;
#pragma unroll
      for (int i = 0; i < NCK; ++i) {
        const int ch = tid + 256 * i, r = ch / CPR, cc = (ch % CPR) * EPC;
        x3_store4(sl + r * LDB + cc, PLANE, pk[i]);
        x3_store4(sl + 3 * PLANE + r * LDB + cc, PLANE, pv[i]);
      }
      return;
    }
    if constexpr (Src::kPlain) {
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
      return;
    }
    if constexpr (X3) {  // three bf16 planes per tensor: 8 B of each per 16-B chunk
      bf16* sl = ring3 + s * 6 * PLANE;
#pragma unroll
      for (int i = 0; i < NCK; ++i) {
        const int ch = tid + 256 * i, r = ch / CPR, cc = (ch % CPR) * SPC;
        uint4 ck[SUB], cv[SUB];
        Src::stage(pk[i], sk[Src::kScaled ? i : 0], ck);
        Src::stage(pv[i], sv[Src::kScaled ? i : 0], cv);
        if (ALLK || ch < BK * CPR) {
#pragma unroll
          for (int j = 0; j < SUB; ++j) {
            x3_store4(sl + r * LDB + cc + j * EPC, PLANE, ck[j]);
            x3_store4(sl + 3 * PLANE + r * LDB + cc + j * EPC, PLANE, cv[j]);
          }
        }
      }
      return;
    }
    T* sK = ring + s * SLOT;
    T* sV = sK + BK * LD;
#pragma unroll
    for (int i = 0; i < NCK; ++i) {
      const int ch = tid + 256 * i, r = ch / CPR, cc = (ch % CPR) * SPC;
      uint4 c[SUB];
      Src::stage(pk[i], sk[Src::kScaled ? i : 0], c);
      if (ALLK || ch < BK * CPR) {
#pragma unroll
        for (int j = 0; j < SUB; ++j) *(uint4*)(sK + r * LD + cc + j * EPC) = c[j];
      }
    }
#pragma unroll
    for (int i = 0; i < NCV; ++i) {
      const int ch = tid + 256 * i, r = ch / CPV, cc = (ch % CPV) * SPC;
      uint4 c[SUB];
      Src::stage(pv[i], sv[Src::kScaled ? i : 0], c);
      if (ALLV || ch < BK * CPV) {
#pragma unroll
        for (int j = 0; j < SUB; ++j) *(uint4*)(sV + r * LDV + cc + j * EPC) = c[j];
      }
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

template <typename Src, int DT, int DV, int KB, bool X3, int MINB>
static hipError_t launch_extend_t(const typename Src::Args& sa, int64_t B, hipStream_t st) {
  using T = typename Src::T;
  const ExtendArgs& a = Src::base(sa);
  // two slots of K and V: fp32 / bf16 rows, or (X3) three bf16 planes each
  const size_t smem = X3 ? (size_t)2 * 6 * 32 * KB * (DT + 8) * 2
                         : sizeof(T) * (size_t)(DT + DV + 32 / sizeof(T)) * 2 * 32 * KB;
  auto kfn = fa_extend_ring<Src, DT, DV, KB, X3, MINB>;
  hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)smem);
  if (e != hipSuccess) return e;
  dim3 grid((unsigned)(a.nqb * B * a.H * (DT / DV)), 1, 1);
  hipLaunchKernelGGL(kfn, grid, dim3(256), smem, st, sa);
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

// the fp32 plan's instantiations (ids 0-3) on a source with fp32 Q, the bf16 plan's (4-7) on a bf16 one
template <typename Src>
static hipError_t launch_extend_f32(const typename Src::Args& sa, int64_t B, hipStream_t st) {
  switch (extend_plan(4, Src::base(sa).d).kernel) {
    case 0: return launch_extend_t<Src, 32, 32, 1, true, 2>(sa, B, st);
    case 1: return launch_extend_t<Src, 64, 64, 1, true, 2>(sa, B, st);
    case 2: return launch_extend_t<Src, 128, 128, 1, false, 2>(sa, B, st);
    default: return launch_extend_t<Src, 256, 128, 1, false, 1>(sa, B, st);
  }
}
template <typename Src>
static hipError_t launch_extend_bf16(const typename Src::Args& sa, int64_t B, hipStream_t st) {
  switch (extend_plan(2, Src::base(sa).d).kernel) {
    case 4: return launch_extend_t<Src, 32, 32, 2, false, 2>(sa, B, st);
    case 5: return launch_extend_t<Src, 64, 64, 2, false, 2>(sa, B, st);
    case 6: return launch_extend_t<Src, 128, 128, 2, false, 2>(sa, B, st);
    default: return launch_extend_t<Src, 256, 256, 1, false, 1>(sa, B, st);
  }
}

hipError_t launch_extend(const ExtendArgs& a, bool bf16_in, int64_t B, hipStream_t st) {
  return bf16_in ? launch_extend_bf16<ExtPlainSrc<bf16>>(a, B, st) : launch_extend_f32<ExtPlainSrc<float>>(a, B, st);
}

hipError_t launch_extend_paged(const PagedExtendArgs& a, bool bf16_in, int64_t B, hipStream_t st) {
  return bf16_in ? launch_extend_bf16<ExtPagedSrc<bf16>>(a, B, st) : launch_extend_f32<ExtPagedSrc<float>>(a, B, st);
}

hipError_t launch_extend_kvq(const KvqExtendArgs& a, bool fp8, int64_t B, hipStream_t st) {
  return fp8 ? launch_extend_f32<ExtKvqSrc<KvFp8>>(a, B, st) : launch_extend_f32<ExtKvqSrc<KvBf16>>(a, B, st);
}

}  // namespace mt
