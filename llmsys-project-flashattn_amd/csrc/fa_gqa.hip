// Grouped-query attention for training and prefill, fp32 (MT_F32), d <= 128 with 16-B rows:
// forward, dK/dV pass and dQ pass with K, V, dK, dV at Hkv heads ([B, Hkv, N, d]); query head h
// uses kv head h / G, G = H / Hkv. mt_flash_attn_fwd_varlen / mt_flash_attn_bwd_v3's contract
// otherwise (causal, kv_len, padded queries attend the valid keys, an empty row gives O = 0,
// m = -inf, l = 0, padding keys get dK = dV = 0).
//
// The work split:
//  - fa_gqa_fwd, fa_gqa_dq ("query on the lane"): a workgroup owns one (batch, kv head, query
//    block); its four waves are gs = min(G, 4) query heads of the group at the SAME query
//    positions (4 / gs sub-blocks of 32 queries each), ceil(G / gs) slices per group. The causal
//    and kv_len bounds are those of the query positions, so the waves walk the same key tiles:
//    K / V tiles of 32 keys are staged once per workgroup into a two-slot LDS ring (one barrier per
//    tile, the next tile's loads in flight during the products) and read by every wave. A
//    group's K / V is fetched ceil(G / gs) times instead of G times. Each wave keeps its head's
//    Q (and dO) rows in registers.
//  - fa_gqa_dkv ("key on the lane", as fa_bwd_dkv_ring): a workgroup owns 128 keys of one
//    (batch, kv head), 32 per wave, the K / V rows in registers, and sweeps the query tiles of
//    head hkv·G + g for g = 0 .. G-1 in that order through the ring, accumulating dKᵀ / dVᵀ in the
//    same registers: the sum over the group is the order of the sweep. No atomics, no HBM
//    read-modify-write, one store per element, the same bits on every call.
// Both contractions of every pass run on the bf16 MFMA with each fp32 operand in three bf16
// pieces (fa_common.h mma_x3, fp32 accuracy): the staged tiles are split once when written to
// the ring (three planes), register rows per use, P and dS per tile; sums that run across tiles
// take each tile's products in a fresh accumulator added with a VALU fp32 add (x3_tile_sum).
// δ and the log2-LSE come from fa_bwd_prep (per query row, it knows nothing of groups).
#include "fa_common.h"

#include <math.h>

namespace mt {

hipError_t launch_bwd_prep_f32(const AttnArgs& a, hipStream_t st);  // fa_bwd.hip

namespace {

constexpr int kWaves = 4;

// the KS k-step fragments of an fp32 row (zero past d, a multiple of 4)
template <int KS>
__device__ __forceinline__ void gqa_row_frags(f32x8 (&f)[KS], const float* row, int d, int hf) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    uint4 ch[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = 16 * ks + 8 * hf + 4 * j;
      ch[j] = col < d ? *(const uint4*)(row + col) : make_uint4(0, 0, 0, 0);
    }
    f[ks] = __builtin_bit_cast(f32x8, ch);
  }
}

// Where a wave of the query-on-the-lane kernels works: grid (query blocks, B · Hkv · slices).
struct GqaWave {
  int b, hkv, hh;  // batch row, kv head, query head
  int q0, nq;      // the workgroup's first query and query count (32 · sub-blocks)
  int wq0;         // the wave's first query
  bool live;       // false: the wave only stages tiles (group tail, or 4 % gs spare wave)
};
__device__ __forceinline__ GqaWave gqa_wave(const AttnArgs& p, int Hkv, int G, int gs, int wave) {
  const int qs = kWaves / gs, nsl = (G + gs - 1) / gs;
  int qblk, y;
  xcd_order(qblk, y);
  GqaWave w;
  const int sl = y % nsl, bk = y / nsl;
  w.hkv = bk % Hkv;
  w.b = bk / Hkv;
  const int g = sl * gs + wave % gs, qsub = wave / gs;
  w.hh = w.hkv * G + min(g, G - 1);
  w.nq = 32 * qs;
  w.q0 = qblk * w.nq;
  w.wq0 = w.q0 + 32 * min(qsub, qs - 1);
  w.live = g < G && qsub < qs && w.wq0 < p.N;
  return w;
}

// The two-slot K / V ring of the query-on-the-lane kernels: a slot is K's three bf16 planes
// ([32][DT + 8] each), then V's. load() takes tile k0 into registers (rows >= N and columns >= d
// zero), store() splits them into slot s.
template <int DT>
struct KvRing {
  static constexpr int kCPR = DT / 4, NCK = (32 * kCPR + 255) / 256;
  static constexpr int LDB = DT + 8, PLANE = 32 * LDB, SLOT = 6 * PLANE;  // bf16 elements
  uint4 pk[NCK], pv[NCK];
  __device__ __forceinline__ void load(const AttnArgs& p, const float* Kg, const float* Vg, int k0, int tid) {
#pragma unroll
    for (int i = 0; i < NCK; ++i) {
      const int ch = tid + 256 * i, r = ch / kCPR, cc = (ch % kCPR) * 4, gr = k0 + r;
      pk[i] = pv[i] = make_uint4(0, 0, 0, 0);
      if (ch < 32 * kCPR && gr < p.N && cc < p.d) {
        pk[i] = *(const uint4*)(Kg + (int64_t)gr * p.sk[2] + cc);
        pv[i] = *(const uint4*)(Vg + (int64_t)gr * p.sv[2] + cc);
      }
    }
  }
  __device__ __forceinline__ void store(bf16* ring, int s, int tid) const {
#pragma unroll
    for (int i = 0; i < NCK; ++i) {
      const int ch = tid + 256 * i, r = ch / kCPR, cc = (ch % kCPR) * 4;
      if (ch < 32 * kCPR) {
        bf16* k3 = ring + s * SLOT + r * LDB + cc;
        x3_store4(k3, PLANE, pk[i]);
        x3_store4(k3 + 3 * PLANE, PLANE, pv[i]);
      }
    }
  }
};

// ---------------------------------------------------------------------------
// Forward: O, m, l per query head.
template <int DT, bool CAUSAL>
__global__ __launch_bounds__(256, DT == 128 ? 1 : 2) void fa_gqa_fwd(AttnArgs p, int Hkv, int G, int gs) {
  using Ring = KvRing<DT>;
  constexpr int KS = DT / 16, NDB = DT / 32, BK = 32, LDB = Ring::LDB, PLANE = Ring::PLANE;
  extern __shared__ __attribute__((aligned(16))) char gqa_smem[];
  bf16* ring = (bf16*)gqa_smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hf = lane >> 5, c32 = lane & 31;
  const int N = p.N, d = p.d;
  const GqaWave w = gqa_wave(p, Hkv, G, gs, wave);
  const float* Kg = (const float*)p.k + w.b * p.sk[0] + w.hkv * p.sk[1];
  const float* Vg = (const float*)p.v + w.b * p.sv[0] + w.hkv * p.sv[1];
  const float c2 = p.scale_log2;
  const int my_q = w.wq0 + c32, wave_qmax = w.wq0 + 31;

  f32x8 bq[KS];
  gqa_row_frags(bq, (const float*)p.q + w.b * p.sq[0] + w.hh * p.sq[1] + (int64_t)min(my_q, N - 1) * p.sq[2], d, hf);
  f32x16 O[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) O[i] = f32x16{};
  float m_run = -INFINITY, l_run = 0.f;  // log2 units; the whole row's, the same in both lane halves

  const int Nk = kv_keys(p, w.b);
  const int kend = CAUSAL ? min(Nk, w.q0 + w.nq) : Nk;
  const int ntile = (kend + BK - 1) / BK;
  Ring kv;
  if (ntile > 0) {
    kv.load(p, Kg, Vg, 0, tid);
    kv.store(ring, 0, tid);
    if (ntile > 1) kv.load(p, Kg, Vg, BK, tid);
  }
  __syncthreads();

#pragma nounroll
  for (int t = 0; t < ntile; ++t) {
    const int k0 = t * BK;
    const bf16* sK3 = ring + (t & 1) * Ring::SLOT;
    const bf16* sV3 = sK3 + 3 * PLANE;
    if (w.live && !(CAUSAL && k0 > wave_qmax)) {
      // Sᵀ with the query on the lane: rows are keys k0 + acc_row(r, hf)
      f32x16 S = f32x16{};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        asm volatile("" : "+v"(bq[ks]));  // split per use (see fa_bwd_dkv_ring)
        mma_x3(S, x3_rows(sK3 + c32 * LDB + ks * 16 + 8 * hf, PLANE), x3_split(bq[ks]));
      }
      const bool msk = k0 + BK > Nk || (CAUSAL && k0 + BK - 1 > w.wq0);
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = k0 + acc_row(r, hf);
        if (msk && (key >= Nk || (CAUSAL && key > my_q))) S[r] = -INFINITY;
        mx = fmaxf(mx, S[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float m_new = fmaxf(m_run, mx * c2);  // c2 > 0: the max of the scaled logits
      const float mu = m_new == -INFINITY ? 0.f : m_new;  // a tile with no visible key for this row
      const float alpha = __builtin_amdgcn_exp2f(m_run - mu);
      float ps = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(S[r], c2, -mu));
        S[r] = pv;
        ps += pv;
      }
      ps += __shfl_xor(ps, 32);
      l_run = l_run * alpha + ps;
      m_run = m_new;
      // Oᵀ = alpha · Oᵀ + Vᵀ · Pᵀ, the tile's products in a fresh sum (x3_tile_sum)
      const X3Frag bp0 = x3_split(acc_frag<float>(S, 0)), bp1 = x3_split(acc_frag<float>(S, 1));
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        f32x16 acc = f32x16{};
        mma_x3(acc, x3_cols(sV3, PLANE, LDB, 4 * hf, db * 32, lane), bp0);
        mma_x3(acc, x3_cols(sV3, PLANE, LDB, 16 + 4 * hf, db * 32, lane), bp1);
        O[db] = O[db] * alpha + acc;
      }
    }
    if (t + 1 < ntile) {
      kv.store(ring, (t + 1) & 1, tid);
      if (t + 2 < ntile) kv.load(p, Kg, Vg, k0 + 2 * BK, tid);
    }
    __syncthreads();
  }

  // a row with no key (kv_len = 0) stores O = 0, m = -inf, l = 0
  if (w.live && my_q < N) {
    const float inv_l = l_run > 0.f ? 1.f / l_run : 0.f;
    float* Og = (float*)p.out + w.b * p.so[0] + w.hh * p.so[1] + (int64_t)my_q * p.so[2];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int col = db * 32 + 8 * g + 4 * hf;
        if (col < d)
          store4(Og + col, O[db][4 * g] * inv_l, O[db][4 * g + 1] * inv_l, O[db][4 * g + 2] * inv_l,
                 O[db][4 * g + 3] * inv_l, true);
      }
    if (hf == 0) {
      const int64_t row = ((int64_t)w.b * p.H + w.hh) * N + my_q;
      if (p.m) p.m[row] = m_run * kLn2;
      if (p.l) p.l[row] = l_run;
    }
  }
}

// ---------------------------------------------------------------------------
// dQ per query head: the forward's packing; S and dP recomputed with the query on the lane.
template <int DT, bool CAUSAL>
__global__ __launch_bounds__(256, DT == 128 ? 1 : 2) void fa_gqa_dq(AttnArgs p, int Hkv, int G, int gs) {
  using Ring = KvRing<DT>;
  constexpr int KS = DT / 16, NDB = DT / 32, BK = 32, LDB = Ring::LDB, PLANE = Ring::PLANE;
  extern __shared__ __attribute__((aligned(16))) char gqa_smem[];
  bf16* ring = (bf16*)gqa_smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hf = lane >> 5, c32 = lane & 31;
  const int N = p.N, d = p.d;
  const GqaWave w = gqa_wave(p, Hkv, G, gs, wave);
  const float* Kg = (const float*)p.k + w.b * p.sk[0] + w.hkv * p.sk[1];
  const float* Vg = (const float*)p.v + w.b * p.sv[0] + w.hkv * p.sv[1];
  const float c2 = p.scale_log2;
  const int my_q = w.wq0 + c32, wave_qmax = w.wq0 + 31;

  f32x8 bq[KS], bo[KS];
  float lse_q, del_q;
  {
    const int qr = min(my_q, N - 1);
    gqa_row_frags(bq, (const float*)p.q + w.b * p.sq[0] + w.hh * p.sq[1] + (int64_t)qr * p.sq[2], d, hf);
    gqa_row_frags(bo, (const float*)p.dout + w.b * p.sdo[0] + w.hh * p.sdo[1] + (int64_t)qr * p.sdo[2], d, hf);
    const int64_t row = ((int64_t)w.b * p.H + w.hh) * N + qr;
    lse_q = p.lse2[row];
    del_q = p.delta[row];
  }
  f32x16 dQ[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) dQ[i] = f32x16{};

  const int Nk = kv_keys(p, w.b);  // keys >= Nk are padding
  const int kend = CAUSAL ? min(Nk, w.q0 + w.nq) : Nk;
  const int ntile = (kend + BK - 1) / BK;
  Ring kv;
  if (ntile > 0) {
    kv.load(p, Kg, Vg, 0, tid);
    kv.store(ring, 0, tid);
    if (ntile > 1) kv.load(p, Kg, Vg, BK, tid);
  }
  __syncthreads();

#pragma nounroll
  for (int t = 0; t < ntile; ++t) {
    const int k0 = t * BK;
    const bf16* sK3 = ring + (t & 1) * Ring::SLOT;
    const bf16* sV3 = sK3 + 3 * PLANE;
    if (w.live && !(CAUSAL && k0 > wave_qmax)) {
      f32x16 S = f32x16{}, dP = f32x16{};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int col = ks * 16 + 8 * hf;
        asm volatile("" : "+v"(bq[ks]), "+v"(bo[ks]));  // split per use (see fa_bwd_dkv_ring)
        mma_x3(S, x3_rows(sK3 + c32 * LDB + col, PLANE), x3_split(bq[ks]));
        mma_x3(dP, x3_rows(sV3 + c32 * LDB + col, PLANE), x3_split(bo[ks]));
      }
      const bool msk = k0 + BK > Nk || (CAUSAL && k0 + BK - 1 > w.wq0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = k0 + acc_row(r, hf);
        float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(S[r], c2, -lse_q));
        if (msk && (key >= Nk || (CAUSAL && key > my_q))) pv = 0.f;
        dP[r] = pv * (dP[r] - del_q);
      }
      const X3Frag bs0 = x3_split(acc_frag<float>(dP, 0)), bs1 = x3_split(acc_frag<float>(dP, 1));
#pragma unroll
      for (int db = 0; db < NDB; ++db) {  // the tile's products in a fresh sum (x3_tile_sum)
        f32x16 acc = f32x16{};
        mma_x3(acc, x3_cols(sK3, PLANE, LDB, 4 * hf, db * 32, lane), bs0);
        mma_x3(acc, x3_cols(sK3, PLANE, LDB, 16 + 4 * hf, db * 32, lane), bs1);
        dQ[db] += acc;
      }
    }
    if (t + 1 < ntile) {
      kv.store(ring, (t + 1) & 1, tid);
      if (t + 2 < ntile) kv.load(p, Kg, Vg, k0 + 2 * BK, tid);
    }
    __syncthreads();
  }

  if (w.live && my_q < N) {
    float* dQg = (float*)p.dq + w.b * p.sdq[0] + w.hh * p.sdq[1] + (int64_t)my_q * p.sdq[2];
    const float sc = p.scale;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int col = db * 32 + 8 * g + 4 * hf;
        if (col < d)
          store4(dQg + col, dQ[db][4 * g] * sc, dQ[db][4 * g + 1] * sc, dQ[db][4 * g + 2] * sc,
                 dQ[db][4 * g + 3] * sc, true);
      }
  }
}

// ---------------------------------------------------------------------------
// dK, dV at Hkv heads: grid (ceil(N / 128), B · Hkv); 4 waves x 32 keys, K / V rows in registers;
// the Q / dO tiles of 32 queries (with their lse2 / δ) of the group's G query heads, head after
// head, streamed through a two-slot ring. A slot is Q's three bf16 planes, dO's, then lse2 | δ.
template <int DT, bool CAUSAL>
__global__ __launch_bounds__(256, DT == 128 ? 1 : 2) void fa_gqa_dkv(AttnArgs p, int Hkv, int G) {
  constexpr int kCPR = DT / 4, NCK = (32 * kCPR + 255) / 256, KS = DT / 16, NDB = DT / 32;
  constexpr int BKV = 128, BQ = 32, LDB = DT + 8, PLANE = BQ * LDB;
  constexpr int SLOT = 6 * PLANE * 2 + 2 * BQ * 4;  // bytes
  extern __shared__ __attribute__((aligned(16))) char gqa_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hf = lane >> 5, c32 = lane & 31;
  const int N = p.N, d = p.d;
  int kblk, y;
  xcd_order(kblk, y);
  const int b = y / Hkv, hkv = y % Hkv;
  const float* Kg = (const float*)p.k + b * p.sk[0] + hkv * p.sk[1];
  const float* Vg = (const float*)p.v + b * p.sv[0] + hkv * p.sv[1];
  const float c2 = p.scale_log2;
  const int k0 = kblk * BKV;
  const int my_k = k0 + wave * 32 + c32, wave_kmin = k0 + wave * 32;
  // the causal skip bound; non-causal: -1 behind an opaque copy, so the tile body stays a branch
  // (see fa_bwd_dkv_ring)
  int skip_lim = CAUSAL ? wave_kmin : -1;
  if (!CAUSAL) asm volatile("" : "+s"(skip_lim));
  const int Nk = kv_keys(p, b);  // keys >= Nk are padding: zero gradients
  f32x8 bk[KS], bv[KS];
  {
    const int kr = min(my_k, N - 1);
    gqa_row_frags(bk, Kg + (int64_t)kr * p.sk[2], d, hf);
    gqa_row_frags(bv, Vg + (int64_t)kr * p.sv[2], d, hf);
  }
  f32x16 dK[NDB], dV[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) { dK[i] = f32x16{}; dV[i] = f32x16{}; }

  const int qstart = CAUSAL ? k0 : 0;  // k0 is a multiple of BQ
  const int nt = N > qstart && k0 < Nk ? (N - qstart + BQ - 1) / BQ : 0;  // tiles per query head
  const int ntile = nt * G;  // tile t: head hkv·G + t / nt, queries qstart + (t % nt)·32 ...
  uint4 pq[NCK], po[NCK];
  float pl = 0.f, pd = 0.f;
  auto pre_load = [&](int t) __attribute__((always_inline)) {
    const int g = t / nt, qt = qstart + (t - g * nt) * BQ, hh = hkv * G + g;
    const float* Qg = (const float*)p.q + b * p.sq[0] + hh * p.sq[1];
    const float* dOg = (const float*)p.dout + b * p.sdo[0] + hh * p.sdo[1];
#pragma unroll
    for (int i = 0; i < NCK; ++i) {
      const int ch = tid + 256 * i, r = ch / kCPR, cc = (ch % kCPR) * 4, gr = qt + r;
      pq[i] = po[i] = make_uint4(0, 0, 0, 0);
      if (ch < 32 * kCPR && gr < N && cc < d) {
        pq[i] = *(const uint4*)(Qg + (int64_t)gr * p.sq[2] + cc);
        po[i] = *(const uint4*)(dOg + (int64_t)gr * p.sdo[2] + cc);
      }
    }
    if (tid < BQ) {
      const int q = qt + tid;
      const int64_t row = ((int64_t)b * p.H + hh) * N + q;
      pl = q < N ? p.lse2[row] : 0.f;
      pd = q < N ? p.delta[row] : 0.f;
    }
  };
  auto pre_store = [&](int s) __attribute__((always_inline)) {
    bf16* slot = (bf16*)(gqa_smem + s * SLOT);
#pragma unroll
    for (int i = 0; i < NCK; ++i) {
      const int ch = tid + 256 * i, r = ch / kCPR, cc = (ch % kCPR) * 4;
      if (ch < 32 * kCPR) {
        x3_store4(slot + r * LDB + cc, PLANE, pq[i]);
        x3_store4(slot + 3 * PLANE + r * LDB + cc, PLANE, po[i]);
      }
    }
    if (tid < BQ) {
      float* sRow = (float*)(slot + 6 * PLANE);
      sRow[tid] = pl;
      sRow[BQ + tid] = pd;
    }
  };
  if (ntile > 0) {
    pre_load(0);
    pre_store(0);
    if (ntile > 1) pre_load(1);
  }
  __syncthreads();

  int qt = qstart, tq = 0;  // the tile's first query and its index within the head
#pragma nounroll
  for (int t = 0; t < ntile; ++t) {
    const bf16* sQ3 = (const bf16*)(gqa_smem + (t & 1) * SLOT);  // Q planes, then dO's
    const bf16* sO3 = sQ3 + 3 * PLANE;
    const float* sLse = (const float*)(sQ3 + 6 * PLANE);
    const float* sDel = sLse + BQ;
    if (!(qt + BQ - 1 < skip_lim)) {
      // Sᵀ and dPᵀ: the lane's column is key my_k, rows are queries qt + acc_row(r, hf)
      f32x16 S = f32x16{}, dP = f32x16{};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int col = ks * 16 + 8 * hf;
        asm volatile("" : "+v"(bk[ks]), "+v"(bv[ks]));  // keeps the splits inside the loop
        mma_x3(S, x3_rows(sQ3 + c32 * LDB + col, PLANE), x3_split(bk[ks]));
        mma_x3(dP, x3_rows(sO3 + c32 * LDB + col, PLANE), x3_split(bv[ks]));
      }
      const bool msk = qt + BQ > N || k0 + BKV > Nk || (CAUSAL && qt < wave_kmin + 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ql = acc_row(r, hf);
        const int q = qt + ql;
        float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(S[r], c2, -sLse[ql]));
        if (msk && (q >= N || my_k >= Nk || (CAUSAL && my_k > q))) pv = 0.f;
        S[r] = pv;
        dP[r] = pv * (dP[r] - sDel[ql]);
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {  // each k-step's products in a fresh sum (x3_tile_sum)
        const X3Frag bp = x3_split(acc_frag<float>(S, s)), bs = x3_split(acc_frag<float>(dP, s));
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
          f32x16 acc = f32x16{};
          mma_x3(acc, x3_cols(sO3, PLANE, LDB, 16 * s + 4 * hf, db * 32, lane), bp);
          dV[db] += acc;
          acc = f32x16{};
          mma_x3(acc, x3_cols(sQ3, PLANE, LDB, 16 * s + 4 * hf, db * 32, lane), bs);
          dK[db] += acc;
        }
      }
    }
    if (t + 1 < ntile) {
      pre_store((t + 1) & 1);
      if (t + 2 < ntile) pre_load(t + 2);
    }
    __syncthreads();
    if (++tq == nt) { tq = 0; qt = qstart; } else qt += BQ;
  }

  if (my_k < N) {
    float* dKg = (float*)p.dk + b * p.sdk[0] + hkv * p.sdk[1] + (int64_t)my_k * p.sdk[2];
    float* dVg = (float*)p.dv + b * p.sdv[0] + hkv * p.sdv[1] + (int64_t)my_k * p.sdv[2];
    const float sc = p.scale;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int col = db * 32 + 8 * g + 4 * hf;
        if (col < d) {
          store4(dKg + col, dK[db][4 * g] * sc, dK[db][4 * g + 1] * sc, dK[db][4 * g + 2] * sc,
                 dK[db][4 * g + 3] * sc, true);
          store4(dVg + col, dV[db][4 * g], dV[db][4 * g + 1], dV[db][4 * g + 2], dV[db][4 * g + 3], true);
        }
      }
  }
}

template <class K, class... Args>
hipError_t launch_smem(K kfn, dim3 grid, size_t smem, hipStream_t st, Args... args) {
  const hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kfn, grid, dim3(256), smem, st, args...);
  return hipGetLastError();
}

// query heads of a group per workgroup, and the (query blocks, B · Hkv · slices) grid
struct GqaGrid { int gs; dim3 grid; };
GqaGrid gqa_grid(const AttnArgs& a, int Hkv) {
  const int G = a.H / Hkv, gs = G < kWaves ? G : kWaves, bq = 32 * (kWaves / gs);
  return GqaGrid{gs, dim3((unsigned)((a.N + bq - 1) / bq), (unsigned)(a.B * Hkv * ((G + gs - 1) / gs)))};
}

template <int DT, bool CAUSAL>
hipError_t gqa_fwd_t(const AttnArgs& a, int Hkv, hipStream_t st) {
  const GqaGrid g = gqa_grid(a, Hkv);
  return launch_smem(fa_gqa_fwd<DT, CAUSAL>, g.grid, (size_t)2 * KvRing<DT>::SLOT * 2, st, a, Hkv, a.H / Hkv, g.gs);
}
template <int DT, bool CAUSAL>
hipError_t gqa_bwd_t(const AttnArgs& a, int Hkv, hipStream_t st) {
  const size_t slot = (size_t)6 * 32 * (DT + 8) * 2 + 2 * 32 * 4;
  hipError_t e = launch_smem(fa_gqa_dkv<DT, CAUSAL>, dim3((unsigned)((a.N + 127) / 128), (unsigned)(a.B * Hkv)),
                             2 * slot, st, a, Hkv, a.H / Hkv);
  if (e != hipSuccess) return e;
  const GqaGrid g = gqa_grid(a, Hkv);
  return launch_smem(fa_gqa_dq<DT, CAUSAL>, g.grid, (size_t)2 * KvRing<DT>::SLOT * 2, st, a, Hkv, a.H / Hkv, g.gs);
}

}  // namespace

// a: the fp32 arguments with H query heads (16-B rows, d <= 128, host-checked); K, V at Hkv heads
hipError_t launch_gqa_fwd(const AttnArgs& a, int Hkv, bool causal, hipStream_t st) {
  if (a.d <= 32) return causal ? gqa_fwd_t<32, true>(a, Hkv, st) : gqa_fwd_t<32, false>(a, Hkv, st);
  if (a.d <= 64) return causal ? gqa_fwd_t<64, true>(a, Hkv, st) : gqa_fwd_t<64, false>(a, Hkv, st);
  return causal ? gqa_fwd_t<128, true>(a, Hkv, st) : gqa_fwd_t<128, false>(a, Hkv, st);
}

// prep (δ, lse2 into a.delta / a.lse2), then the dK/dV pass and the dQ pass
hipError_t launch_gqa_bwd(const AttnArgs& a, int Hkv, bool causal, hipStream_t st) {
  const hipError_t e = launch_bwd_prep_f32(a, st);
  if (e != hipSuccess) return e;
  if (a.d <= 32) return causal ? gqa_bwd_t<32, true>(a, Hkv, st) : gqa_bwd_t<32, false>(a, Hkv, st);
  if (a.d <= 64) return causal ? gqa_bwd_t<64, true>(a, Hkv, st) : gqa_bwd_t<64, false>(a, Hkv, st);
  return causal ? gqa_bwd_t<128, true>(a, Hkv, st) : gqa_bwd_t<128, false>(a, Hkv, st);
}

}  // namespace mt
