// C ABI of the quantised KV cache (include/minitorch_hip.h): mt_flash_attn_decode_kvq with its
// split / workspace queries, mt_flash_attn_extend_kvq with its plan query, mt_kv_cache_append_quant
// and mt_kv_cache_dequant. Kernels: fa_kvq.hip, fa_extend.hip.
// Every argument is validated before the first device call.
#include "../../include/minitorch_hip.h"
#include "fa_kvq.h"
#include "fa_extend.h"
#include <math.h>

namespace mt {
static int kvq_dtype(int kv_dtype) {
  if (kv_dtype != MT_KV_BF16 && kv_dtype != MT_KV_FP8) return set_error("unsupported kv_dtype %d", kv_dtype);
  return 0;
}

// format, sizes and the 8-element chunk rule on d (Nq is checked by the caller); 0 or the error status
static int kvq_sizes(int kv_dtype, int64_t B, int64_t Hkv, int64_t N, int64_t d) {
  if (int rc = kvq_dtype(kv_dtype)) return rc;
  if (B <= 0 || Hkv <= 0 || N <= 0 || d <= 0)
    return set_error("bad sizes B=%lld Hkv=%lld N=%lld d=%lld", (long long)B, (long long)Hkv, (long long)N,
                     (long long)d);
  if (d > 256) return set_error("quantised cache head dim out of range (d=%lld; d <= 256)", (long long)d);
  if (d % 8) return set_error("a quantised cache needs rows of 8-element chunks: d=%lld is not a multiple of 8", (long long)d);
  if (N > (1 << 30) || B * Hkv > (1ll << 31) - 1)
    return set_error("sizes out of range (N=%lld, B*Hkv=%lld)", (long long)N, (long long)(B * Hkv));
  return 0;
}

static int kvq_decode_sizes(int kv_dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk, int64_t d) {
  if (int rc = kvq_dtype(kv_dtype)) return rc;
  if (B <= 0 || H <= 0 || Nk <= 0 || d <= 0)
    return set_error("bad sizes B=%lld H=%lld Nk=%lld d=%lld", (long long)B, (long long)H, (long long)Nk, (long long)d);
  if (Hkv <= 0 || Hkv > H || H % Hkv)
    return set_error("kv heads must divide the query heads (H=%lld, Hkv=%lld)", (long long)H, (long long)Hkv);
  if (Nq < 1 || Nq > 8)
    return set_error("decode takes 1 to 8 query rows per head (Nq=%lld)", (long long)Nq);
  if (B * H * Nq > (1ll << 31) - 1)
    return set_error("sizes out of range (B*H*Nq=%lld)", (long long)(B * H * Nq));
  return kvq_sizes(kv_dtype, B, Hkv, Nk, d);
}

// the extend step on a quantised cache: its format, mt_flash_attn_extend's sizes for fp32 rows and the
// 8-element chunk rule on d
static int kvq_extend_sizes(int kv_dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk, int64_t d) {
  if (int rc = kvq_dtype(kv_dtype)) return rc;
  if (int rc = extend_sizes(MT_F32, B, H, Hkv, Nq, Nk, d)) return rc;
  if (d % 8) return set_error("a quantised cache needs rows of 8-element chunks: d=%lld is not a multiple of 8", (long long)d);
  return 0;
}

// base pointer and every stride a multiple of `bytes` (strides in elements of esize bytes)
static int kvq_aligned(const char* what, const void* p, const int64_t s[3], int esize, int bytes) {
  if (!p) return set_error("%s is NULL", what);
  if ((uintptr_t)p % bytes) return set_error("%s is not %d-B aligned", what, bytes);
  for (int i = 0; i < 3; ++i)
    if (s[i] * esize % bytes)
      return set_error("%s stride %d (%lld elements) is not a multiple of %d B", what, i, (long long)s[i], bytes);
  return 0;
}

// a cache: 16-B rows for bf16, 8-B rows for fp8 (one chunk of 8 elements either way)
static int kvq_cache_aligned(const char* what, const void* p, const int64_t s[3], bool fp8) {
  return kvq_aligned(what, p, s, fp8 ? 1 : 2, fp8 ? 8 : 16);
}

static int kvq_scales(bool fp8, const void* k_scale, const void* v_scale) {
  if (!fp8) return 0;
  if (!k_scale || !v_scale) return set_error("an fp8 cache needs k_scale and v_scale (a scale pointer is NULL)");
  if (((uintptr_t)k_scale | (uintptr_t)v_scale) & 3) return set_error("k_scale / v_scale is not 4-B aligned");
  return 0;
}

}  // namespace mt

using namespace mt;

extern "C" {

int mt_flash_attn_decode_kvq_splits(int kv_dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk,
                                    int64_t d, int64_t* span_keys, int64_t* tile_keys) {
  if (kvq_decode_sizes(kv_dtype, B, H, Hkv, Nq, Nk, d)) return 0;
  const DecodePlan p = decode_plan(2, B, H, Hkv, Nq, Nk, d);  // 8-element chunks: a bf16 cache's plan
  if (span_keys) *span_keys = p.span;
  if (tile_keys) *tile_keys = p.tile;
  return p.nsplit;
}

int64_t mt_flash_attn_decode_kvq_workspace_bytes(int kv_dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq,
                                                 int64_t Nk, int64_t d) {
  if (kvq_decode_sizes(kv_dtype, B, H, Hkv, Nq, Nk, d)) return -1;
  return decode_ws_bytes(decode_plan(2, B, H, Hkv, Nq, Nk, d), B, H, Nq, d);
}

int mt_flash_attn_decode_kvq(int kv_dtype, int causal, const void* q, const void* k_cache, const void* v_cache,
                             const float* k_scale, const float* v_scale, void* o, float* m, float* l,
                             int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk, int64_t d,
                             const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                             const int64_t* o_strides, const int* kv_len,
                             void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = kvq_decode_sizes(kv_dtype, B, H, Hkv, Nq, Nk, d)) return rc;
  const bool fp8 = kv_dtype == MT_KV_FP8;
  if (int rc = kvq_scales(fp8, k_scale, v_scale)) return rc;
  const DecodePlan p = decode_plan(2, B, H, Hkv, Nq, Nk, d);
  KvqDecodeArgs ka;
  DecodeArgs& a = ka.d;
  if (int rc = decode_args(a, p, "mt_flash_attn_decode_kvq_workspace_bytes", causal, q, k_cache, v_cache, o, m, l, B,
                           H, Hkv, Nq, Nk, d, kv_len, workspace, workspace_bytes))
    return rc;
  a.o_f32 = 1;
  ka.kscale = fp8 ? k_scale : nullptr; ka.vscale = fp8 ? v_scale : nullptr;
  strides_or_dense(a.qs, q_strides, H, Nq, d);
  strides_or_dense(a.ks, k_strides, Hkv, Nk, d);
  strides_or_dense(a.vs, v_strides, Hkv, Nk, d);
  strides_or_dense(a.os, o_strides, H, Nq, d);
  if (int rc = kvq_aligned("q", q, a.qs, 4, 16)) return rc;
  if (int rc = kvq_cache_aligned("k_cache", k_cache, a.ks, fp8)) return rc;
  if (int rc = kvq_cache_aligned("v_cache", v_cache, a.vs, fp8)) return rc;
  if (int rc = kvq_aligned("o", o, a.os, 4, 16)) return rc;
  return check_hip(launch_decode_kvq(ka, fp8, B, (hipStream_t)stream), "mt_flash_attn_decode_kvq");
}

int mt_flash_attn_extend_kvq_plan(int kv_dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk, int64_t d,
                                  int64_t* block_queries, int64_t* tile_keys) {
  if (kvq_extend_sizes(kv_dtype, B, H, Hkv, Nq, Nk, d)) return -1;
  const ExtendPlan p = extend_plan(4, d);  // the ring holds fp32 rows: the fp32 plan
  if (block_queries) *block_queries = p.bq;
  if (tile_keys) *tile_keys = p.bk;
  return p.kernel;
}

int mt_flash_attn_extend_kvq(int kv_dtype, int causal, const void* q, const void* k_cache, const void* v_cache,
                             const float* k_scale, const float* v_scale, void* o, float* m, float* l,
                             int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk, int64_t d,
                             const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                             const int64_t* o_strides, const int* kv_len, const int* q_len, void* stream) {
  if (int rc = kvq_extend_sizes(kv_dtype, B, H, Hkv, Nq, Nk, d)) return rc;
  const bool fp8 = kv_dtype == MT_KV_FP8;
  if (int rc = kvq_scales(fp8, k_scale, v_scale)) return rc;
  KvqExtendArgs ka;
  ExtendArgs& a = ka.e;
  a.q = q; a.k = k_cache; a.v = v_cache; a.o = o;
  strides_or_dense(a.qs, q_strides, H, Nq, d);
  strides_or_dense(a.ks, k_strides, Hkv, Nk, d);
  strides_or_dense(a.vs, v_strides, Hkv, Nk, d);
  strides_or_dense(a.os, o_strides, H, Nq, d);
  if (int rc = kvq_aligned("q", q, a.qs, 4, 16)) return rc;
  if (int rc = kvq_cache_aligned("k_cache", k_cache, a.ks, fp8)) return rc;
  if (int rc = kvq_cache_aligned("v_cache", v_cache, a.vs, fp8)) return rc;
  if (int rc = kvq_aligned("o", o, a.os, 4, 16)) return rc;
  extend_args(a, 4, causal, m, l, H, Hkv, Nq, Nk, d, kv_len, q_len);
  a.o_f32 = 1;
  ka.kscale = fp8 ? k_scale : nullptr; ka.vscale = fp8 ? v_scale : nullptr;
  return check_hip(launch_extend_kvq(ka, fp8, B, (hipStream_t)stream), "mt_flash_attn_extend_kvq");
}

int mt_kv_cache_append_quant(int kv_dtype, const float* k_new, const float* v_new, void* k_cache, void* v_cache,
                             float* k_scale, float* v_scale, int64_t B, int64_t Hkv, int64_t Nq, int64_t Nmax,
                             int64_t d, const int64_t* knew_strides, const int64_t* vnew_strides,
                             const int64_t* kcache_strides, const int64_t* vcache_strides,
                             const int* pos, void* stream) {
  if (int rc = kvq_sizes(kv_dtype, B, Hkv, Nmax, d)) return rc;
  if (Nq <= 0 || Nq > (1 << 30) || B * Hkv * Nq > (1ll << 40))
    return set_error("bad sizes Nq=%lld (B*Hkv*Nq=%lld)", (long long)Nq, (long long)(B * Hkv * Nq));
  const bool fp8 = kv_dtype == MT_KV_FP8;
  if (int rc = kvq_scales(fp8, k_scale, v_scale)) return rc;
  if (!pos) return set_error("pos is NULL");
  KvqAppendArgs a;
  a.kn = k_new; a.vn = v_new; a.kc = (char*)k_cache; a.vc = (char*)v_cache;
  a.kscale = fp8 ? k_scale : nullptr; a.vscale = fp8 ? v_scale : nullptr;
  a.pos = pos;
  strides_or_dense(a.kns, knew_strides, Hkv, Nq, d);
  strides_or_dense(a.vns, vnew_strides, Hkv, Nq, d);
  strides_or_dense(a.kcs, kcache_strides, Hkv, Nmax, d);
  strides_or_dense(a.vcs, vcache_strides, Hkv, Nmax, d);
  if (int rc = kvq_aligned("k_new", k_new, a.kns, 4, 4)) return rc;
  if (int rc = kvq_aligned("v_new", v_new, a.vns, 4, 4)) return rc;
  if (int rc = kvq_cache_aligned("k_cache", k_cache, a.kcs, fp8)) return rc;
  if (int rc = kvq_cache_aligned("v_cache", v_cache, a.vcs, fp8)) return rc;
  // the new rows take any strides: 16-B loads when both allow them, element loads otherwise
  a.vec_in = 1;
  if (((uintptr_t)k_new | (uintptr_t)v_new) & 15) a.vec_in = 0;
  for (int i = 0; i < 3; ++i)
    if (a.kns[i] % 4 || a.vns[i] % 4) a.vec_in = 0;
  int lpr = 1;
  while (lpr * 8 < d) lpr *= 2;
  a.lpr = lpr;
  a.rows = B * Hkv * Nq;
  if ((a.rows + 256 / lpr - 1) / (256 / lpr) > (1ll << 31) - 1) return set_error("append too large");
  a.Hkv = (int)Hkv; a.Nq = (int)Nq; a.Nmax = (int)Nmax; a.d = (int)d;
  return check_hip(launch_kvq_append(a, fp8, (hipStream_t)stream), "mt_kv_cache_append_quant");
}

int mt_kv_cache_dequant(int kv_dtype, const void* k_cache, const void* v_cache, const float* k_scale,
                        const float* v_scale, float* k_out, float* v_out, int64_t B, int64_t Hkv, int64_t Nk,
                        int64_t d, const int64_t* kcache_strides, const int64_t* vcache_strides,
                        const int64_t* kout_strides, const int64_t* vout_strides, const int* kv_len, void* stream) {
  if (int rc = kvq_sizes(kv_dtype, B, Hkv, Nk, d)) return rc;
  const bool fp8 = kv_dtype == MT_KV_FP8;
  if (int rc = kvq_scales(fp8, k_scale, v_scale)) return rc;
  KvqDequantArgs a;
  a.kc = (const char*)k_cache; a.vc = (const char*)v_cache;
  a.kscale = fp8 ? k_scale : nullptr; a.vscale = fp8 ? v_scale : nullptr;
  a.ko = k_out; a.vo = v_out; a.kv_len = kv_len;
  strides_or_dense(a.kcs, kcache_strides, Hkv, Nk, d);
  strides_or_dense(a.vcs, vcache_strides, Hkv, Nk, d);
  strides_or_dense(a.kos, kout_strides, Hkv, Nk, d);
  strides_or_dense(a.vos, vout_strides, Hkv, Nk, d);
  if (int rc = kvq_cache_aligned("k_cache", k_cache, a.kcs, fp8)) return rc;
  if (int rc = kvq_cache_aligned("v_cache", v_cache, a.vcs, fp8)) return rc;
  if (int rc = kvq_aligned("k_out", k_out, a.kos, 4, 16)) return rc;
  if (int rc = kvq_aligned("v_out", v_out, a.vos, 4, 16)) return rc;
  a.chunks = (int)(d / 8);
  a.total = B * Hkv * Nk * a.chunks;
  if ((a.total + 255) / 256 > (1ll << 31) - 1) return set_error("dequant too large");
  a.Hkv = (int)Hkv; a.Nk = (int)Nk;
  return check_hip(launch_kvq_dequant(a, fp8, (hipStream_t)stream), "mt_kv_cache_dequant");
}

}  // extern "C"
