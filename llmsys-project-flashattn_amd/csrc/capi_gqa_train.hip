// C ABI of grouped-query attention for training and prefill (include/minitorch_hip.h):
// mt_flash_attn_fwd_gqa, mt_flash_attn_bwd_gqa and the backward's workspace query. Kernels:
// fa_gqa.hip. Hkv == H forwards to mt_flash_attn_fwd_varlen / mt_flash_attn_bwd_v3. Every
// argument is validated before the first device call; no allocation, no synchronisation.
#include "../../include/minitorch_hip.h"
#include "fa_common.h"
#include <math.h>
#include <string.h>

namespace mt {
int set_error(const char* fmt, ...);  // capi_flash.hip
int check_hip(hipError_t e, const char* where);
hipError_t launch_gqa_fwd(const AttnArgs& a, int Hkv, bool causal, hipStream_t st);
hipError_t launch_gqa_bwd(const AttnArgs& a, int Hkv, bool causal, hipStream_t st);

// dtype, sizes, the grouping and the 16-B row rule on d; 0 or the error status
static int gqa_sizes(int dtype, int64_t B, int64_t H, int64_t Hkv, int64_t N, int64_t d) {
  if (dtype != MT_F32) return set_error("unsupported dtype %d (grouped-query training attention is MT_F32)", dtype);
  if (B <= 0 || H <= 0 || N <= 0 || d <= 0)
    return set_error("bad sizes B=%lld H=%lld N=%lld d=%lld", (long long)B, (long long)H, (long long)N,
                     (long long)d);
  if (Hkv <= 0 || Hkv > H || H % Hkv)
    return set_error("kv heads must divide the query heads (H=%lld, Hkv=%lld)", (long long)H, (long long)Hkv);
  if (d > 128) return set_error("head dim out of range (d=%lld; d <= 128)", (long long)d);
  if (d % 4) return set_error("grouped-query attention needs 16-B rows: d=%lld is not a multiple of 4", (long long)d);
  if (N > (1 << 30) || B * H > 65535)  // the grids hold at most B · H rows in y
    return set_error("sizes out of range (N=%lld, B*H=%lld)", (long long)N, (long long)(B * H));
  return 0;
}

static void gqa_strides(int64_t dst[3], const int64_t* src, int64_t H, int64_t N, int64_t d) {
  if (src) {
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
  } else {
    dst[0] = H * N * d; dst[1] = N * d; dst[2] = d;
  }
}

// strides in multiples of 16 B, then the base: given and 16-B aligned
static int gqa_aligned(const char* what, const void* p, const int64_t s[3]) {
  for (int i = 0; i < 3; ++i)
    if (s[i] % 4) return set_error("%s stride %d (%lld elements) is not a multiple of 16 B", what, i, (long long)s[i]);
  if (!p) return set_error("%s is NULL", what);
  if ((uintptr_t)p & 15) return set_error("%s is not 16-B aligned", what);
  return 0;
}

static int64_t gqa_rows_bytes(int64_t B, int64_t H, int64_t N) {
  return (2 * B * H * N * (int64_t)sizeof(float) + 255) / 256 * 256;
}
}  // namespace mt

using namespace mt;

extern "C" {

int mt_flash_attn_fwd_gqa(int dtype, int causal, const void* q, const void* k, const void* v, void* o, float* m,
                          float* l, int64_t B, int64_t H, int64_t Hkv, int64_t N, int64_t d,
                          const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                          const int64_t* o_strides, const int* kv_len, void* stream) {
  if (gqa_sizes(dtype, B, H, Hkv, N, d)) return 1;
  AttnArgs a;
  memset(&a, 0, sizeof(a));
  gqa_strides(a.sq, q_strides, H, N, d);
  gqa_strides(a.sk, k_strides, Hkv, N, d);
  gqa_strides(a.sv, v_strides, Hkv, N, d);
  gqa_strides(a.so, o_strides, H, N, d);
  if (gqa_aligned("q", q, a.sq) || gqa_aligned("k", k, a.sk) || gqa_aligned("v", v, a.sv) ||
      gqa_aligned("o", o, a.so))
    return 1;
  if (Hkv == H)
    return mt_flash_attn_fwd_varlen(dtype, causal, q, k, v, o, m, l, B, H, N, d, q_strides, k_strides, v_strides,
                                    o_strides, kv_len, stream);
  a.q = q; a.k = k; a.v = v; a.out = o; a.m = m; a.l = l;
  a.kv_len = kv_len;
  a.B = (int)B; a.H = (int)H; a.N = (int)N; a.d = (int)d;
  a.scale = (float)(1.0 / sqrt((double)d));
  a.scale_log2 = (float)(1.4426950408889634 / sqrt((double)d));
  return check_hip(launch_gqa_fwd(a, (int)Hkv, causal != 0, (hipStream_t)stream), "mt_flash_attn_fwd_gqa");
}

int64_t mt_flash_attn_bwd_gqa_workspace_bytes(int64_t B, int64_t H, int64_t Hkv, int64_t N, int64_t d) {
  if (gqa_sizes(MT_F32, B, H, Hkv, N, d)) return -1;
  return Hkv == H ? mt_flash_attn_bwd_workspace_bytes(B, H, N, d) : gqa_rows_bytes(B, H, N);
}

int mt_flash_attn_bwd_gqa(int dtype, int causal, const void* q, const void* k, const void* v, const void* o,
                          const void* dout, const float* m, const float* l, void* dq, void* dk, void* dv,
                          int64_t B, int64_t H, int64_t Hkv, int64_t N, int64_t d, const int64_t* strides,
                          const int* kv_len, void* workspace, int64_t workspace_bytes, void* stream) {
  if (gqa_sizes(dtype, B, H, Hkv, N, d)) return 1;
  const int64_t need = mt_flash_attn_bwd_gqa_workspace_bytes(B, H, Hkv, N, d);
  if (workspace_bytes < need)
    return set_error("mt_flash_attn_bwd_gqa: workspace too small: %lld bytes, "
                     "mt_flash_attn_bwd_gqa_workspace_bytes gives %lld", (long long)workspace_bytes, (long long)need);
  AttnArgs a;
  memset(&a, 0, sizeof(a));
  int64_t* dst[8] = {a.sq, a.sk, a.sv, a.so, a.sdo, a.sdq, a.sdk, a.sdv};
  const void* ptr[8] = {q, k, v, o, dout, dq, dk, dv};
  static const char* const name[8] = {"q", "k", "v", "o", "dout", "dq", "dk", "dv"};
  for (int i = 0; i < 8; ++i) {
    const bool kv = i == 1 || i == 2 || i == 6 || i == 7;
    gqa_strides(dst[i], strides ? strides + 3 * i : nullptr, kv ? Hkv : H, N, d);
    if (gqa_aligned(name[i], ptr[i], dst[i])) return 1;
  }
  if (!m || !l) return set_error("mt_flash_attn_bwd_gqa: m or l is NULL");
  if (!workspace || ((uintptr_t)workspace & 15))
    return set_error("mt_flash_attn_bwd_gqa: the workspace is NULL or not 16-B aligned");
  if (Hkv == H)
    return mt_flash_attn_bwd_v3(dtype, causal, q, k, v, o, dout, m, l, dq, dk, dv, B, H, N, d, strides, kv_len,
                                workspace, workspace_bytes, stream);
  a.q = q; a.k = k; a.v = v; a.o = o; a.dout = dout;
  a.dq = dq; a.dk = dk; a.dv = dv;
  a.m = (float*)m; a.l = (float*)l;
  a.kv_len = kv_len;
  a.lse2 = (float*)workspace;
  a.delta = a.lse2 + B * H * N;
  a.B = (int)B; a.H = (int)H; a.N = (int)N; a.d = (int)d;
  a.scale = (float)(1.0 / sqrt((double)d));
  a.scale_log2 = (float)(1.4426950408889634 / sqrt((double)d));
  return check_hip(launch_gqa_bwd(a, (int)Hkv, causal != 0, (hipStream_t)stream), "mt_flash_attn_bwd_gqa");
}

}  // extern "C"
