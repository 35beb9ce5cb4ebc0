// Paged KV cache: decode attention on K / V rows that live in scattered pages
// (mt_flash_attn_decode_paged), the append through the block table (mt_kv_cache_append_paged) and
// the copy of a row's pages into a contiguous cache (mt_kv_cache_gather_paged).
//
// Storage, per layer and per K / V: a pool of n_pages pages of P rows (P a power of two >= 16),
// seen as [n_pages, Hkv, P, d] through element strides (page, head, row), unit-stride d. One
// block table, device int32 [B, W]: logical key j of batch row b is row j % P of page
// table[b][j / P]; the logical capacity is Nk = W * P.
//
// Decode is the shared kernel (fa_decode_kernel.h) on PagedSrc below, which differs from a contiguous
// cache only in the address of a key row: the same plan (decode_plan at Nk = W * P), arithmetic and
// combine pass, so the same bits as on a contiguous cache holding the same rows. A wave-wide load
// covers 64 / LPK <= 16 <= P consecutive keys starting at a multiple of that count, so it never
// straddles a page. With n = clamp(kv_len[b], 0, W * P), a key at or past the span's end re-reads key
// kend - 1 through that key's own table entry: no table entry at index >= ceil(n / P) and no pool row
// of a key >= n is read. A table entry is brought into [0, n_pages) before it forms an address, so a
// table that breaks the contract reads a wrong page of the pool, never memory outside it.
#include "fa_paged.h"
#include "fa_decode_kernel.h"
#include <algorithm>

namespace mt {
template <typename T> struct PagedSrc : RowFormat<T> {
  using Args = PagedDecodeArgs;
  static __host__ __device__ __forceinline__ const DecodeArgs& base(const Args& sa) { return sa.d; }
  // fp32, one row: the plain source asks for 5 waves per SIMD (96 VGPRs) at LPK <= 16. The page index
  // and the two address products cost a few registers: LPK = 16 (d in (32, 64]) spills 12 B per lane at
  // 96, so it is left to the allocator (4 waves per SIMD); LPK 4 and 8 fit and keep the request
  static constexpr int waves_per_eu(int lpk, int nq) { return sizeof(T) == 4 && nq == 1 && lpk <= 8 ? 5 : 1; }

  const DecodeArgs& a;
  // this head's rows of page 0, at the lane's chunk (a lane past the row's chunks re-reads chunk 0,
  // values dropped); a page adds ks[0] / vs[0], a row ks[2] / vs[2]
  const T* kb; const T* vb;
  const int* tb;  // this batch row's pages
  int lgP, pmask, pmax;
  __device__ __forceinline__ PagedSrc(const Args& sa, int b, int hkv, int c, int C)
      : a(sa.d),
        kb((const T*)sa.d.k + (int64_t)hkv * sa.d.ks[1] + (c < C ? c : 0) * Chunk<T>::N),
        vb((const T*)sa.d.v + (int64_t)hkv * sa.d.vs[1] + (c < C ? c : 0) * Chunk<T>::N),
        tb(sa.table + (int64_t)b * sa.W),
        lgP(sa.lgP), pmask((1 << sa.lgP) - 1), pmax(sa.n_pages - 1) {}
  // each row through the table entry of its key
  template <int GROUPS>
  __device__ __forceinline__ void issue(int t0, int g, int kend, uint4* ku, uint4* vu, float*, float*) const {
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
  }
};

// Sizes are validated by the caller (capi_paged.hip); the plan is decode_plan's at Nk = W * P.
hipError_t launch_decode_paged(const PagedDecodeArgs& a, bool bf16_in, int64_t B, hipStream_t st) {
  const int lpk = decode_lpk(a.d.d, bf16_in ? 2 : 4);
  return bf16_in ? launch_decode_src<PagedSrc<bf16>>(a, lpk, B, st) : launch_decode_src<PagedSrc<float>>(a, lpk, B, st);
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
