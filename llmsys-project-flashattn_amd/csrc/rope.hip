// mt_rope (include/minitorch_hip.h): rotary position embedding of the head rows of one or two
// [B, H, T, d] tensors (Q, and K with its own head count) in one launch, in the half-split
// ("rotate-half") convention: element j < d/2 of a row pairs with element j + d/2, and at
// position p
//   out[j]       = x[j]       * cos[p][j] - x[j + d/2] * sin[p][j]
//   out[j + d/2] = x[j + d/2] * cos[p][j] + x[j]       * sin[p][j]
// (inverse: -sin, the transpose). cos / sin are host-built fp32 tables [n_pos, d/2]: no
// sincosf runs here, the result is a function of the inputs and the table rows alone.
// Token t of batch row b sits at p = min(max(pos0[b], 0) + t, n_pos - 1), pos0 read on the
// device (NULL: 0), so a captured launch follows a cache's device lengths.
//
// A streaming kernel: every element is read once and written once, no LDS. One thread owns
// both halves of its pairs and loads both before it stores, so out == x is allowed.
//   vector body: a thread takes the 16-B chunk at j = 4c and its partner at j + d/2, with 16-B
//     loads of the table rows; consecutive threads take consecutive chunks of a row, then the
//     next row (d % 8 == 0, 16-B aligned bases, strides divisible by 4).
//   scalar body: one pair per thread, any even d.
// The grid is capped and strides over the rest. Which body runs is a host function of the
// arguments (never of pos0's contents).
#include "../../include/minitorch_hip.h"
#include "fa_common.h"

namespace mt {
int set_error(const char* fmt, ...);           // capi_flash.hip
int check_hip(hipError_t e, const char* where);

constexpr int kRopeThreads = 256;
constexpr int64_t kRopeMaxBlocks = 2048;  // 256 CUs x 8 workgroups; the rest by grid stride

struct RopeTensor {
  const float* x;
  float* out;
  int64_t xs[3], os[3];  // (batch, head, token) element strides
};

struct RopeArgs {
  RopeTensor t[2];
  int64_t H, H2;  // heads of t[0] and t[1] (H2 == 0: no second tensor)
  int64_t B, T, d, n_pos;
  const float* cos;
  const float* sin;
  const int* pos0;
  float sign;  // +1, or -1 for the inverse
};

// row r of the launch -> (tensor, b, h, t): rows run over (b, head of Q then of K, t)
struct RopeRow {
  const float* x;
  float* out;
  int64_t p;
};

// (the launch's pairs number fewer than 2^31, mt_rope refuses more: the index arithmetic is 32-bit)
__device__ __forceinline__ RopeRow rope_row(const RopeArgs& a, uint32_t r) {
  const uint32_t T = (uint32_t)a.T, HH = (uint32_t)(a.H + a.H2);
  const uint32_t t = r % T;
  const uint32_t bh = r / T;
  int64_t h = bh % HH;
  const int64_t b = bh / HH;
  const int which = h >= a.H ? 1 : 0;
  if (which) h -= a.H;
  const RopeTensor& ten = a.t[which];
  int64_t p = a.pos0 ? (int64_t)a.pos0[b] : 0;
  p = (p < 0 ? 0 : p) + t;
  p = p > a.n_pos - 1 ? a.n_pos - 1 : p;
  RopeRow row;
  row.x = ten.x + b * ten.xs[0] + h * ten.xs[1] + t * ten.xs[2];
  row.out = ten.out + b * ten.os[0] + h * ten.os[1] + t * ten.os[2];
  row.p = p;
  return row;
}

__global__ __launch_bounds__(kRopeThreads) void rope_vec_kernel(const RopeArgs a) {
  const int64_t half = a.d >> 1;
  const uint32_t chunks = (uint32_t)(a.d >> 3);  // 16-B chunks per half row
  const uint32_t total = (uint32_t)(a.B * (a.H + a.H2) * a.T) * chunks;
  const uint32_t step = gridDim.x * kRopeThreads;
  for (uint32_t i = blockIdx.x * kRopeThreads + threadIdx.x; i < total; i += step) {
    const uint32_t c = i % chunks;
    const RopeRow row = rope_row(a, i / chunks);
    const int64_t j = 4 * c;
    const float4 lo = *(const float4*)(row.x + j);
    const float4 hi = *(const float4*)(row.x + j + half);
    const float4 cs = *(const float4*)(a.cos + row.p * half + j);
    float4 sn = *(const float4*)(a.sin + row.p * half + j);
    sn.x *= a.sign; sn.y *= a.sign; sn.z *= a.sign; sn.w *= a.sign;
    float4 olo, ohi;
    olo.x = lo.x * cs.x - hi.x * sn.x; ohi.x = hi.x * cs.x + lo.x * sn.x;
    olo.y = lo.y * cs.y - hi.y * sn.y; ohi.y = hi.y * cs.y + lo.y * sn.y;
    olo.z = lo.z * cs.z - hi.z * sn.z; ohi.z = hi.z * cs.z + lo.z * sn.z;
    olo.w = lo.w * cs.w - hi.w * sn.w; ohi.w = hi.w * cs.w + lo.w * sn.w;
    *(float4*)(row.out + j) = olo;
    *(float4*)(row.out + j + half) = ohi;
  }
}

__global__ __launch_bounds__(kRopeThreads) void rope_scalar_kernel(const RopeArgs a) {
  const uint32_t half = (uint32_t)(a.d >> 1);
  const uint32_t total = (uint32_t)(a.B * (a.H + a.H2) * a.T) * half;
  const uint32_t step = gridDim.x * kRopeThreads;
  for (uint32_t i = blockIdx.x * kRopeThreads + threadIdx.x; i < total; i += step) {
    const uint32_t j = i % half;
    const RopeRow row = rope_row(a, i / half);
    const float lo = row.x[j], hi = row.x[j + half];
    const float cs = a.cos[row.p * half + j];
    const float sn = a.sin[row.p * half + j] * a.sign;
    row.out[j] = lo * cs - hi * sn;
    row.out[j + half] = hi * cs + lo * sn;
  }
}

static void rope_strides(int64_t dst[3], const int64_t* src, int64_t H, int64_t T, int64_t d) {
  if (src) {
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
  } else {
    dst[0] = H * T * d; dst[1] = T * d; dst[2] = d;
  }
}

static bool rope_vec_ok(const RopeTensor& t) {
  if (((uintptr_t)t.x | (uintptr_t)t.out) & 15) return false;
  for (int i = 0; i < 3; ++i)
    if ((t.xs[i] | t.os[i]) & 3) return false;
  return true;
}
}  // namespace mt

using namespace mt;

extern "C" int mt_rope(int dtype, int inverse, const void* x, void* out, int64_t H, const int64_t* x_strides,
                       const int64_t* out_strides, const void* x2, void* out2, int64_t H2,
                       const int64_t* x2_strides, const int64_t* out2_strides, int64_t B, int64_t T, int64_t d,
                       const float* cos, const float* sin, int64_t n_pos, const int* pos0, void* stream) {
  if (B <= 0 || T <= 0 || H <= 0 || d <= 0 || n_pos <= 0)
    return set_error("mt_rope: bad sizes B=%lld H=%lld T=%lld d=%lld n_pos=%lld", (long long)B, (long long)H,
                     (long long)T, (long long)d, (long long)n_pos);
  if (d & 1) return set_error("mt_rope: d=%lld is odd (the halves of a row pair up)", (long long)d);
  if (d > 256) return set_error("mt_rope: d=%lld is above the limit of 256", (long long)d);
  if (dtype != MT_F32) return set_error("mt_rope: unsupported dtype %d (fp32 only)", dtype);
  if (!x) return set_error("mt_rope: x is NULL");
  if (!out) return set_error("mt_rope: out is NULL");
  if (!cos || !sin) return set_error("mt_rope: the cos / sin table is NULL");
  if (x2 && !out2) return set_error("mt_rope: x2 given but out2 is NULL");
  if (x2 && H2 <= 0) return set_error("mt_rope: x2 given with H2=%lld", (long long)H2);
  if (!x2) H2 = 0;
  // the kernels count the launch's pairs in 32 bits (no 64-bit divisions per thread): fewer than
  // 2^31 of them, 16 GiB of fp32 rows; the element offsets and table offsets are 64-bit
  if ((double)B * (double)(H + H2) * (double)T * (double)(d / 2) >= 2147483648.0 || n_pos > (1ll << 40))
    return set_error("mt_rope: sizes out of range (B (H + H2) T d / 2 must stay below 2^31)");

  RopeArgs a;
  a.t[0].x = (const float*)x; a.t[0].out = (float*)out;
  rope_strides(a.t[0].xs, x_strides, H, T, d);
  rope_strides(a.t[0].os, out_strides, H, T, d);
  a.t[1] = a.t[0];
  if (x2) {
    a.t[1].x = (const float*)x2; a.t[1].out = (float*)out2;
    rope_strides(a.t[1].xs, x2_strides, H2, T, d);
    rope_strides(a.t[1].os, out2_strides, H2, T, d);
  }
  a.H = H; a.H2 = H2; a.B = B; a.T = T; a.d = d; a.n_pos = n_pos;
  a.cos = cos; a.sin = sin; a.pos0 = pos0;
  a.sign = inverse ? -1.f : 1.f;

  const bool vec = d % 8 == 0 && !(((uintptr_t)cos | (uintptr_t)sin) & 15) && rope_vec_ok(a.t[0]) &&
                   (!x2 || rope_vec_ok(a.t[1]));
  const int64_t work = B * (H + H2) * T * (vec ? d / 8 : d / 2);
  int64_t blocks = (work + kRopeThreads - 1) / kRopeThreads;
  if (blocks > kRopeMaxBlocks) blocks = kRopeMaxBlocks;
  const dim3 grid((unsigned)blocks), block(kRopeThreads);
  if (vec) rope_vec_kernel<<<grid, block, 0, (hipStream_t)stream>>>(a);
  else rope_scalar_kernel<<<grid, block, 0, (hipStream_t)stream>>>(a);
  return check_hip(hipGetLastError(), "mt_rope");
}
