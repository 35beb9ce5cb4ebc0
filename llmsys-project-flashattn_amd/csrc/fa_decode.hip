// KV-cache decode attention on a contiguous fp32 / bf16 cache (mt_flash_attn_decode[_gqa]): the plan,
// the source of the decode kernel (pass 1, fa_decode_kernel.h, where the algorithm is described), the
// combine pass that every cache kind shares, and the cache append (mt_kv_cache_append).
#include "fa_decode_kernel.h"
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

// A contiguous cache [B, Hkv, Nk, d] of fp32 or bf16 rows, through element strides
template <typename T> struct PlainSrc : RowFormat<T> {
  using Args = DecodeArgs;
  static __host__ __device__ __forceinline__ const DecodeArgs& base(const Args& sa) { return sa; }
  // fp32, one row, d <= 64 sits at the 96-VGPR edge of 5 waves per SIMD: ask for them (the allocator
  // otherwise lands on 95-98 from one build to the next)
  static constexpr int waves_per_eu(int lpk, int nq) { return sizeof(T) == 4 && nq == 1 && lpk <= 16 ? 5 : 1; }

  const DecodeArgs& a;
  const T* kb; const T* vb;  // this (b, hkv)'s rows
  int cc;                    // a lane past the row's chunks re-reads chunk 0 (values dropped)
  __device__ __forceinline__ PlainSrc(const Args& sa, int b, int hkv, int c, int C)
      : a(sa),
        kb((const T*)sa.k + (int64_t)b * sa.ks[0] + (int64_t)hkv * sa.ks[1]),
        vb((const T*)sa.v + (int64_t)b * sa.vs[0] + (int64_t)hkv * sa.vs[1]),
        cc(c < C ? c : 0) {}
  // the row address is formed at the load, chunk offset last: folding cc * EPC into kb / vb costs
  // half the instantiations 1-4 VGPRs, and <bf16, 4, 8> its second wave per SIMD
  template <int GROUPS>
  __device__ __forceinline__ void issue(int t0, int g, int kend, uint4* ku, uint4* vu, float*, float*) const {
    constexpr int EPC = Chunk<T>::N;
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
  }
};

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

hipError_t launch_decode(const DecodeArgs& a, bool bf16_in, int64_t B, hipStream_t st) {
  const int lpk = decode_lpk(a.d, bf16_in ? 2 : 4);
  return bf16_in ? launch_decode_src<PlainSrc<bf16>>(a, lpk, B, st) : launch_decode_src<PlainSrc<float>>(a, lpk, B, st);
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
