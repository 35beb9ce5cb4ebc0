// The training-path kernels of a Llama-shaped block (include/minitorch_hip.h), fp32, device pointers:
//   mt_rmsnorm_fw / mt_rmsnorm_bw   y = gamma (x rstd), rstd = 1 / sqrt(mean x^2 + eps)
//   mt_swiglu_fw / mt_swiglu_bw     out = silu(a) b over gu = [a | b] of [rows, 2F]
//
// RMSNorm, hidden % 4 == 0, hidden <= 1024 and 16-byte aligned pointers (the model's widths): one
// wave per row, lane l holding the float4 pieces at columns 4 (l + 64 k), k < NV, in registers
// between the sum of squares and the output pass, so a row leaves HBM once. The backward keeps
// gamma and its rows' gamma_grad partials in registers across the rows a wave visits (grid-stride,
// at most 512 workgroups of 4 rows); a workgroup adds its four waves' partials in LDS in wave order
// and writes one [hidden] slab to the workspace. Other shapes take the scalar kernels, which
// re-read the row (from L2 in practice) and reduce gamma_grad by column blocks over chunks of 256
// rows. Either way the slabs are then summed by one launch of rms_bw_colsum: 16 columns per
// workgroup, 16 slices of the slabs per column added in ascending order, then the slices in
// ascending order. Two fixed stages and no atomics: gamma_grad is deterministic.
//
// SwiGLU is elementwise: a thread takes 4 adjacent columns of a and the same 4 of b (16-byte
// accesses when F % 4 == 0 and the pointers allow), grid-stride.
#include "../../include/minitorch_hip.h"
#include "fa_common.h"
#include "silu.h"

namespace mt {
int set_error(const char* fmt, ...);           // capi_flash.hip
int check_hip(hipError_t e, const char* where);

namespace rs {
constexpr int kMaxVecBlocks = 512;   // workgroups (4 rows at a time) of the register-resident backward
constexpr int kRowsPerChunk = 256;   // rows per first-stage block of the scalar gamma_grad reduction
constexpr int kMaxVecHidden = 1024;  // what a wave holds in one register pass (NV = 4)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int NV>
__global__ __launch_bounds__(256) void rms_fw_vec(float* __restrict__ out, float* __restrict__ rstd,
                                                  const float* __restrict__ inp, const float* __restrict__ gamma,
                                                  int64_t rows, int64_t H, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += nw) {
    float4 v[NV];
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int64_t c = 4 * (lane + 64 * k);
      if (c < H) {
        v[k] = *(const float4*)(inp + r * H + c);
        ss += (v[k].x * v[k].x + v[k].y * v[k].y) + (v[k].z * v[k].z + v[k].w * v[k].w);
      }
    }
    ss = wave_sum(ss);
    const float rsd = 1.f / sqrtf(ss / (float)H + eps);
    if (lane == 0) rstd[r] = rsd;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int64_t c = 4 * (lane + 64 * k);
      if (c < H) {
        const float4 g = *(const float4*)(gamma + c);
        *(float4*)(out + r * H + c) =
            make_float4(g.x * (v[k].x * rsd), g.y * (v[k].y * rsd), g.z * (v[k].z * rsd), g.w * (v[k].w * rsd));
      }
    }
  }
}

__global__ __launch_bounds__(256) void rms_fw_kernel(float* __restrict__ out, float* __restrict__ rstd,
                                                     const float* __restrict__ inp, const float* __restrict__ gamma,
                                                     int64_t rows, int64_t H, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += nw) {
    const float* x = inp + r * H;
    float ss = 0.f;
    for (int64_t j = lane; j < H; j += 64) ss += x[j] * x[j];
    ss = wave_sum(ss);
    const float rsd = 1.f / sqrtf(ss / (float)H + eps);
    if (lane == 0) rstd[r] = rsd;
    for (int64_t j = lane; j < H; j += 64) out[r * H + j] = gamma[j] * (x[j] * rsd);
  }
}

// dx for every row, and this workgroup's slab ws[blockIdx.x][H] = sum over its rows of dy x rstd
template <int NV>
__global__ __launch_bounds__(256) void rms_bw_vec(float* __restrict__ dinp, float* __restrict__ ws,
                                                  const float* __restrict__ dout, const float* __restrict__ inp,
                                                  const float* __restrict__ gamma, const float* __restrict__ rstd,
                                                  int64_t rows, int64_t H) {
  __shared__ float4 sp[4][64 * NV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nw = (int64_t)gridDim.x * 4;
  float4 dg[NV], gm[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int64_t c = 4 * (lane + 64 * k);
    dg[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    gm[k] = c < H ? *(const float4*)(gamma + c) : dg[k];
  }
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += nw) {
    const float rsd = rstd[r];
    float4 g[NV], x[NV];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int64_t c = 4 * (lane + 64 * k);
      if (c < H) {
        const float4 dy = *(const float4*)(dout + r * H + c);
        x[k] = *(const float4*)(inp + r * H + c);
        g[k] = make_float4(dy.x * gm[k].x, dy.y * gm[k].y, dy.z * gm[k].z, dy.w * gm[k].w);
        s += (g[k].x * x[k].x + g[k].y * x[k].y) + (g[k].z * x[k].z + g[k].w * x[k].w);
        dg[k].x += dy.x * (x[k].x * rsd); dg[k].y += dy.y * (x[k].y * rsd);
        dg[k].z += dy.z * (x[k].z * rsd); dg[k].w += dy.w * (x[k].w * rsd);
      }
    }
    s = wave_sum(s);
    const float coef = rsd * rsd * rsd * (s / (float)H);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int64_t c = 4 * (lane + 64 * k);
      if (c < H)
        *(float4*)(dinp + r * H + c) = make_float4(rsd * g[k].x - x[k].x * coef, rsd * g[k].y - x[k].y * coef,
                                                   rsd * g[k].z - x[k].z * coef, rsd * g[k].w - x[k].w * coef);
    }
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) sp[wave][lane + 64 * k] = dg[k];
  __syncthreads();
  for (int c4 = threadIdx.x; c4 < H / 4; c4 += 256) {
    float4 t = sp[0][c4];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float4 u = sp[w][c4];
      t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
    }
    *(float4*)(ws + (int64_t)blockIdx.x * H + 4 * c4) = t;
  }
}

__global__ __launch_bounds__(256) void rms_bw_dx_kernel(float* __restrict__ dinp, const float* __restrict__ dout,
                                                        const float* __restrict__ inp, const float* __restrict__ gamma,
                                                        const float* __restrict__ rstd, int64_t rows, int64_t H) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += nw) {
    const float* x = inp + r * H;
    const float* dy = dout + r * H;
    const float rsd = rstd[r];
    float s = 0.f;
    for (int64_t j = lane; j < H; j += 64) s += (dy[j] * gamma[j]) * x[j];
    s = wave_sum(s);
    const float coef = rsd * rsd * rsd * (s / (float)H);
    for (int64_t j = lane; j < H; j += 64) dinp[r * H + j] = rsd * (dy[j] * gamma[j]) - x[j] * coef;
  }
}

// block (x: 64 columns, y: a chunk of 256 rows): ws[y][H] = the chunk's sum of dy x rstd
__global__ __launch_bounds__(256) void rms_bw_dg_partial(float* __restrict__ ws, const float* __restrict__ dout,
                                                         const float* __restrict__ inp, const float* __restrict__ rstd,
                                                         int64_t rows, int64_t H) {
  __shared__ float sg[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t col = (int64_t)blockIdx.x * 64 + lane;
  const int64_t r0 = (int64_t)blockIdx.y * kRowsPerChunk;
  const int64_t r1 = min(rows, r0 + kRowsPerChunk);
  float dg = 0.f;
  if (col < H)
    for (int64_t r = r0 + wave; r < r1; r += 4) dg += dout[r * H + col] * (inp[r * H + col] * rstd[r]);
  sg[wave][lane] = dg;
  __syncthreads();
  if (wave == 0 && col < H) ws[(int64_t)blockIdx.y * H + col] = ((sg[0][lane] + sg[1][lane]) + sg[2][lane]) + sg[3][lane];
}

// gamma_grad[col] = sum of the nb slabs ws[.][col]: thread (c = t & 15, s = t >> 4) adds slabs
// s, s + 16, ... of column 16 blockIdx.x + c in ascending order, then thread (c, 0) adds the 16
// slices in ascending order.
__global__ __launch_bounds__(256) void rms_bw_colsum(float* __restrict__ gamma_grad, const float* __restrict__ ws,
                                                     int64_t H, int64_t nb) {
  __shared__ float red[16][16];
  const int c = threadIdx.x & 15, s = threadIdx.x >> 4;
  const int64_t col = (int64_t)blockIdx.x * 16 + c;
  float v = 0.f;
  if (col < H) {
#pragma unroll 8
    for (int64_t b = s; b < nb; b += 16) v += ws[b * H + col];
  }
  red[s][c] = v;
  __syncthreads();
  if (s == 0 && col < H) {
    float t = red[0][c];
#pragma unroll
    for (int i = 1; i < 16; ++i) t += red[i][c];
    gamma_grad[col] = t;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void swiglu_fw_kernel(float* __restrict__ out, const float* __restrict__ gu,
                                                        int64_t rows, int64_t F) {
  const int64_t F4 = (F + 3) / 4, n = rows * F4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / F4, c = 4 * (i % F4);
    const float* a = gu + r * 2 * F + c;
    if (VEC) {
      const float4 av = *(const float4*)a, bv = *(const float4*)(a + F);
      *(float4*)(out + r * F + c) = make_float4(silu(av.x) * bv.x, silu(av.y) * bv.y, silu(av.z) * bv.z, silu(av.w) * bv.w);
    } else {
      for (int e = 0; e < 4 && c + e < F; ++e) out[r * F + c + e] = silu(a[e]) * a[F + e];
    }
  }
}

// da = dout b s (1 + a (1 - s)), s = sigmoid(a); db = dout silu(a)
__device__ __forceinline__ void swiglu_grad(float d, float a, float b, float& da, float& db) {
#pragma clang fp contract(off)
  const float s = 1.f / (1.f + expf(-a));
  da = d * b * s * (1.f + a * (1.f - s));
  db = d * silu(a);
}

template <bool VEC>
__global__ __launch_bounds__(256) void swiglu_bw_kernel(float* __restrict__ dgu, const float* __restrict__ dout,
                                                        const float* __restrict__ gu, int64_t rows, int64_t F) {
  const int64_t F4 = (F + 3) / 4, n = rows * F4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / F4, c = 4 * (i % F4);
    const float* a = gu + r * 2 * F + c;
    float* da = dgu + r * 2 * F + c;
    if (VEC) {
      const float4 av = *(const float4*)a, bv = *(const float4*)(a + F), d = *(const float4*)(dout + r * F + c);
      float4 ga, gb;
      swiglu_grad(d.x, av.x, bv.x, ga.x, gb.x);
      swiglu_grad(d.y, av.y, bv.y, ga.y, gb.y);
      swiglu_grad(d.z, av.z, bv.z, ga.z, gb.z);
      swiglu_grad(d.w, av.w, bv.w, ga.w, gb.w);
      *(float4*)da = ga;
      *(float4*)(da + F) = gb;
    } else {
      for (int e = 0; e < 4 && c + e < F; ++e) swiglu_grad(dout[r * F + c + e], a[e], a[F + e], da[e], da[F + e]);
    }
  }
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// float4 pieces per lane of the register-resident kernels (1, 2 or 4); 0: the scalar kernels
static int row_nv(int64_t H) {
  if (H % 4 != 0 || H > kMaxVecHidden) return 0;
  return H <= 256 ? 1 : (H <= 512 ? 2 : 4);
}
static int64_t vec_blocks(int64_t rows) {
  const int64_t g = (rows + 3) / 4;
  return g > kMaxVecBlocks ? kMaxVecBlocks : g;
}
static int64_t chunks(int64_t rows) { return (rows + kRowsPerChunk - 1) / kRowsPerChunk; }
static unsigned row_grid(int64_t rows) {
  const int64_t g = (rows + 3) / 4;
  return (unsigned)(g > 256 * 32 ? 256 * 32 : g);
}
static unsigned flat_grid(int64_t n) {
  const int64_t g = (n + 255) / 256;
  return (unsigned)(g > 256 * 32 ? 256 * 32 : g);
}
}  // namespace rs
}  // namespace mt

using namespace mt;
using namespace mt::rs;

extern "C" {

int mt_rmsnorm_fw(float* out, float* rstd, const float* inp, const float* gamma, int64_t rows, int64_t hidden,
                  float eps, void* stream) {
  if (!out || !rstd || !inp || !gamma) return set_error("mt_rmsnorm_fw: out, rstd, inp or gamma is NULL");
  if (rows <= 0 || hidden <= 0)
    return set_error("mt_rmsnorm_fw: rows=%lld and hidden=%lld must be positive", (long long)rows, (long long)hidden);
  if (!(eps >= 0.f)) return set_error("mt_rmsnorm_fw: eps=%g is negative", (double)eps);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid(row_grid(rows));
  const int nv = al16(out) && al16(inp) && al16(gamma) ? row_nv(hidden) : 0;
#define MT_RMS_FW(NV) hipLaunchKernelGGL(rms_fw_vec<NV>, grid, dim3(256), 0, st, out, rstd, inp, gamma, rows, hidden, eps)
  switch (nv) {
    case 1: MT_RMS_FW(1); break;
    case 2: MT_RMS_FW(2); break;
    case 4: MT_RMS_FW(4); break;
    default: hipLaunchKernelGGL(rms_fw_kernel, grid, dim3(256), 0, st, out, rstd, inp, gamma, rows, hidden, eps); break;
  }
#undef MT_RMS_FW
  return check_hip(hipGetLastError(), "mt_rmsnorm_fw");
}

int64_t mt_rmsnorm_bw_workspace_bytes(int64_t rows, int64_t hidden) {
  if (rows <= 0 || hidden <= 0) return 0;
  const int64_t slabs = vec_blocks(rows) > chunks(rows) ? vec_blocks(rows) : chunks(rows);
  return slabs * hidden * (int64_t)sizeof(float);
}

int mt_rmsnorm_bw(float* gamma_grad, float* inp_grad, const float* out_grad, const float* inp, const float* gamma,
                  const float* rstd, int64_t rows, int64_t hidden, void* workspace, void* stream) {
  if (!gamma_grad || !inp_grad || !out_grad || !inp || !gamma || !rstd)
    return set_error("mt_rmsnorm_bw: gamma_grad, inp_grad, out_grad, inp, gamma or rstd is NULL");
  if (rows <= 0 || hidden <= 0)
    return set_error("mt_rmsnorm_bw: rows=%lld and hidden=%lld must be positive", (long long)rows, (long long)hidden);
  if (!workspace) return set_error("mt_rmsnorm_bw: workspace is NULL (mt_rmsnorm_bw_workspace_bytes)");
  const hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int nv = al16(inp_grad) && al16(out_grad) && al16(inp) && al16(gamma) && al16(ws) ? row_nv(hidden) : 0;
  int64_t nb;
  if (nv) {
    nb = vec_blocks(rows);
#define MT_RMS_BW(NV) hipLaunchKernelGGL(rms_bw_vec<NV>, dim3((unsigned)nb), dim3(256), 0, st, inp_grad, ws, out_grad, inp, gamma, rstd, rows, hidden)
    switch (nv) {
      case 1: MT_RMS_BW(1); break;
      case 2: MT_RMS_BW(2); break;
      default: MT_RMS_BW(4); break;
    }
#undef MT_RMS_BW
    if (check_hip(hipGetLastError(), "mt_rmsnorm_bw(rows)")) return 1;
  } else {
    nb = chunks(rows);
    if (nb > 65535) return set_error("mt_rmsnorm_bw: rows=%lld is too many for this hidden=%lld", (long long)rows, (long long)hidden);
    hipLaunchKernelGGL(rms_bw_dx_kernel, dim3(row_grid(rows)), dim3(256), 0, st, inp_grad, out_grad, inp, gamma, rstd,
                       rows, hidden);
    if (check_hip(hipGetLastError(), "mt_rmsnorm_bw(dx)")) return 1;
    hipLaunchKernelGGL(rms_bw_dg_partial, dim3((unsigned)((hidden + 63) / 64), (unsigned)nb), dim3(256), 0, st, ws,
                       out_grad, inp, rstd, rows, hidden);
    if (check_hip(hipGetLastError(), "mt_rmsnorm_bw(partial)")) return 1;
  }
  hipLaunchKernelGGL(rms_bw_colsum, dim3((unsigned)((hidden + 15) / 16)), dim3(256), 0, st, gamma_grad,
                     (const float*)ws, hidden, nb);
  return check_hip(hipGetLastError(), "mt_rmsnorm_bw(colsum)");
}

int mt_swiglu_fw(float* out, const float* gu, int64_t rows, int64_t F, void* stream) {
  if (!out || !gu) return set_error("mt_swiglu_fw: out or gu is NULL");
  if (rows <= 0 || F <= 0) return set_error("mt_swiglu_fw: rows=%lld and F=%lld must be positive", (long long)rows, (long long)F);
  const dim3 grid(flat_grid(rows * ((F + 3) / 4)));
  if (F % 4 == 0 && al16(out) && al16(gu))
    hipLaunchKernelGGL(swiglu_fw_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, out, gu, rows, F);
  else
    hipLaunchKernelGGL(swiglu_fw_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, out, gu, rows, F);
  return check_hip(hipGetLastError(), "mt_swiglu_fw");
}

int mt_swiglu_bw(float* dgu, const float* dout, const float* gu, int64_t rows, int64_t F, void* stream) {
  if (!dgu || !dout || !gu) return set_error("mt_swiglu_bw: dgu, dout or gu is NULL");
  if (rows <= 0 || F <= 0) return set_error("mt_swiglu_bw: rows=%lld and F=%lld must be positive", (long long)rows, (long long)F);
  const dim3 grid(flat_grid(rows * ((F + 3) / 4)));
  if (F % 4 == 0 && al16(dgu) && al16(dout) && al16(gu))
    hipLaunchKernelGGL(swiglu_bw_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, dgu, dout, gu, rows, F);
  else
    hipLaunchKernelGGL(swiglu_bw_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, dgu, dout, gu, rows, F);
  return check_hip(hipGetLastError(), "mt_swiglu_bw");
}

}  // extern "C"
