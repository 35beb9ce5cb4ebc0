// C ABI of the KV-cache decode path (include/minitorch_hip.h): mt_flash_attn_decode[_gqa] and
// their split / workspace queries, mt_kv_cache_append, and the extend step mt_flash_attn_extend
// with its plan query. The plain entry points are the Hkv = H
// case of the grouped-query ones. Kernels: fa_decode.hip, fa_extend.hip. Every argument is
// validated before the first device call, as the other mt_flash_attn_* entry points do.
#include "../../include/minitorch_hip.h"
#include "fa_decode.h"
#include "fa_extend.h"
#include <math.h>

namespace mt {
// dtype, sizes and the 16-B row rule on d; 0 or the error status
int decode_sizes(int dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk, int64_t d) {
  if (dtype != MT_F32 && dtype != MT_BF16 && dtype != MT_BF16_F32OUT)
    return set_error("unsupported dtype %d", dtype);
  if (B <= 0 || H <= 0 || Nk <= 0 || d <= 0)
    return set_error("bad sizes B=%lld H=%lld Nk=%lld d=%lld", (long long)B, (long long)H,
                     (long long)Nk, (long long)d);
  if (Hkv <= 0 || Hkv > H || H % Hkv)
    return set_error("kv heads must divide the query heads (H=%lld, Hkv=%lld)", (long long)H, (long long)Hkv);
  if (Nq < 1 || Nq > 8)
    return set_error("decode takes 1 to 8 query rows per head (Nq=%lld)", (long long)Nq);
  if (d > 256) return set_error("decode head dim out of range (d=%lld; d <= 256)", (long long)d);
  if (Nk > (1 << 30) || B * H * Nq > (1ll << 31) - 1)
    return set_error("sizes out of range (Nk=%lld, B*H*Nq=%lld)", (long long)Nk, (long long)(B * H * Nq));
  const int epc = dtype == MT_F32 ? 4 : 8;
  if (d % epc)
    return set_error("decode needs 16-B rows: d=%lld is not a multiple of %d", (long long)d, epc);
  return 0;
}

// the extend step's sizes: decode's rules with 1 <= Nq <= Nk in place of Nq <= 8
int extend_sizes(int dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk, int64_t d) {
  if (dtype != MT_F32 && dtype != MT_BF16 && dtype != MT_BF16_F32OUT)
    return set_error("unsupported dtype %d", dtype);
  if (B <= 0 || H <= 0 || Nk <= 0 || d <= 0)
    return set_error("bad sizes B=%lld H=%lld Nk=%lld d=%lld", (long long)B, (long long)H,
                     (long long)Nk, (long long)d);
  if (Hkv <= 0 || Hkv > H || H % Hkv)
    return set_error("kv heads must divide the query heads (H=%lld, Hkv=%lld)", (long long)H, (long long)Hkv);
  if (Nq < 1) return set_error("extend takes at least one query row per head (Nq=%lld)", (long long)Nq);
  if (Nq > Nk)
    return set_error("extend takes at most Nk query rows per head (Nq=%lld > Nk=%lld)", (long long)Nq,
                     (long long)Nk);
  if (d > 256) return set_error("extend head dim out of range (d=%lld; d <= 256)", (long long)d);
  // the flat grid holds ceil(Nq / 128) * B * H workgroups, twice that for fp32 d > 128
  if (Nk > (1 << 30) || B * H * Nq > (1ll << 31) - 1 || B * H * ((Nq + 127) / 128) > (1ll << 30) - 1)
    return set_error("sizes out of range (Nk=%lld, B*H*Nq=%lld)", (long long)Nk, (long long)(B * H * Nq));
  const int epc = dtype == MT_F32 ? 4 : 8;
  if (d % epc)
    return set_error("extend needs 16-B rows: d=%lld is not a multiple of %d", (long long)d, epc);
  return 0;
}

void strides_or_dense(int64_t dst[3], const int64_t* src, int64_t H, int64_t N, int64_t d) {
  if (src) {
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
  } else {
    dst[0] = H * N * d; dst[1] = N * d; dst[2] = d;
  }
}

int aligned16(const char* what, const void* p, const int64_t s[3], int esize) {
  const int64_t epc = 16 / esize;
  if (!p) return set_error("%s is NULL", what);
  if ((uintptr_t)p & 15) return set_error("%s is not 16-B aligned", what);
  for (int i = 0; i < 3; ++i)
    if (s[i] % epc) return set_error("%s stride %d (%lld elements) is not a multiple of 16 B", what, i, (long long)s[i]);
  return 0;
}

void extend_args(ExtendArgs& a, int esize, int causal, float* m, float* l, int64_t H, int64_t Hkv, int64_t Nq,
                 int64_t Nk, int64_t d, const int* kv_len, const int* q_len) {
  a.m = m; a.l = l; a.kv_len = kv_len; a.q_len = q_len;
  a.H = (int)H; a.Hkv = (int)Hkv; a.Nq = (int)Nq; a.Nk = (int)Nk; a.d = (int)d;
  a.nqb = (int)((Nq + extend_plan(esize, d).bq - 1) / extend_plan(esize, d).bq);
  a.causal = causal != 0;
  a.scale_log2 = (float)(1.4426950408889634 / sqrt((double)d));
}

int64_t decode_ws_bytes(const DecodePlan& p, int64_t B, int64_t H, int64_t Nq, int64_t d) {
  return p.nsplit == 1 ? 0 : B * H * Nq * p.nsplit * (d + 2) * 4;
}

int decode_args(DecodeArgs& a, const DecodePlan& p, const char* ws_query, int causal, const void* q, const void* k,
                const void* v, void* o, float* m, float* l, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk,
                int64_t d, const int* kv_len, void* workspace, int64_t workspace_bytes) {
  const int64_t need = decode_ws_bytes(p, B, H, Nq, d);
  if (need > 0 && (!workspace || workspace_bytes < need))
    return set_error("decode workspace too small: %lld bytes, %s gives %lld",
                     (long long)(workspace ? workspace_bytes : 0), ws_query, (long long)need);
  if (need > 0 && ((uintptr_t)workspace & 15)) return set_error("decode workspace is not 16-B aligned");
  a.q = q; a.k = k; a.v = v; a.o = o; a.m = m; a.l = l;
  a.ws = (float*)workspace; a.kv_len = kv_len;
  a.H = (int)H; a.Nq = (int)Nq; a.Nk = (int)Nk; a.d = (int)d;
  a.Hkv = (int)Hkv; a.gs = p.gs; a.slices = p.slices; a.rows = B * H * Nq;
  a.nsplit = p.nsplit; a.span = p.span; a.causal = causal != 0;
  a.scale_log2 = (float)(1.4426950408889634 / sqrt((double)d));
  return 0;
}
}  // namespace mt

using namespace mt;

extern "C" {

int mt_flash_attn_decode_gqa_splits(int dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk, int64_t d,
                                    int64_t* span_keys, int64_t* tile_keys) {
  if (decode_sizes(dtype, B, H, Hkv, Nq, Nk, d)) return 0;
  const DecodePlan p = decode_plan(dtype == MT_F32 ? 4 : 2, B, H, Hkv, Nq, Nk, d);
  if (span_keys) *span_keys = p.span;
  if (tile_keys) *tile_keys = p.tile;
  return p.nsplit;
}

int64_t mt_flash_attn_decode_gqa_workspace_bytes(int dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk,
                                                 int64_t d) {
  if (decode_sizes(dtype, B, H, Hkv, Nq, Nk, d)) return -1;
  return decode_ws_bytes(decode_plan(dtype == MT_F32 ? 4 : 2, B, H, Hkv, Nq, Nk, d), B, H, Nq, d);
}

int mt_flash_attn_decode_gqa(int dtype, int causal, const void* q, const void* k_cache, const void* v_cache,
                             void* o, float* m, float* l, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk,
                             int64_t d, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                             const int64_t* o_strides, const int* kv_len,
                             void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = decode_sizes(dtype, B, H, Hkv, Nq, Nk, d)) return rc;
  const int esize = dtype == MT_F32 ? 4 : 2, osize = dtype == MT_BF16 ? 2 : 4;
  const DecodePlan p = decode_plan(esize, B, H, Hkv, Nq, Nk, d);
  DecodeArgs a;
  if (int rc = decode_args(a, p, "mt_flash_attn_decode_workspace_bytes", causal, q, k_cache, v_cache, o, m, l, B, H,
                           Hkv, Nq, Nk, d, kv_len, workspace, workspace_bytes))
    return rc;
  a.o_f32 = osize == 4;
  strides_or_dense(a.qs, q_strides, H, Nq, d);
  strides_or_dense(a.ks, k_strides, Hkv, Nk, d);
  strides_or_dense(a.vs, v_strides, Hkv, Nk, d);
  strides_or_dense(a.os, o_strides, H, Nq, d);
  if (int rc = aligned16("q", q, a.qs, esize)) return rc;
  if (int rc = aligned16("k_cache", k_cache, a.ks, esize)) return rc;
  if (int rc = aligned16("v_cache", v_cache, a.vs, esize)) return rc;
  if (int rc = aligned16("o", o, a.os, osize)) return rc;
  return check_hip(launch_decode(a, esize == 2, B, (hipStream_t)stream), "mt_flash_attn_decode");
}

int mt_flash_attn_decode_splits(int dtype, int64_t B, int64_t H, int64_t Nq, int64_t Nk, int64_t d,
                                int64_t* span_keys, int64_t* tile_keys) {
  return mt_flash_attn_decode_gqa_splits(dtype, B, H, H, Nq, Nk, d, span_keys, tile_keys);
}

int64_t mt_flash_attn_decode_workspace_bytes(int dtype, int64_t B, int64_t H, int64_t Nq, int64_t Nk, int64_t d) {
  return mt_flash_attn_decode_gqa_workspace_bytes(dtype, B, H, H, Nq, Nk, d);
}

int mt_flash_attn_decode(int dtype, int causal, const void* q, const void* k_cache, const void* v_cache,
                         void* o, float* m, float* l, int64_t B, int64_t H, int64_t Nq, int64_t Nk, int64_t d,
                         const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                         const int64_t* o_strides, const int* kv_len,
                         void* workspace, int64_t workspace_bytes, void* stream) {
  return mt_flash_attn_decode_gqa(dtype, causal, q, k_cache, v_cache, o, m, l, B, H, H, Nq, Nk, d, q_strides,
                                  k_strides, v_strides, o_strides, kv_len, workspace, workspace_bytes, stream);
}

int mt_flash_attn_extend_plan(int dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk, int64_t d,
                              int64_t* block_queries, int64_t* tile_keys) {
  if (extend_sizes(dtype, B, H, Hkv, Nq, Nk, d)) return -1;
  const ExtendPlan p = extend_plan(dtype == MT_F32 ? 4 : 2, d);
  if (block_queries) *block_queries = p.bq;
  if (tile_keys) *tile_keys = p.bk;
  return p.kernel;
}

int mt_flash_attn_extend(int dtype, int causal, const void* q, const void* k_cache, const void* v_cache,
                         void* o, float* m, float* l, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk,
                         int64_t d, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                         const int64_t* o_strides, const int* kv_len, const int* q_len, void* stream) {
  if (int rc = extend_sizes(dtype, B, H, Hkv, Nq, Nk, d)) return rc;
  const int esize = dtype == MT_F32 ? 4 : 2, osize = dtype == MT_BF16 ? 2 : 4;
  ExtendArgs a;
  a.q = q; a.k = k_cache; a.v = v_cache; a.o = o;
  strides_or_dense(a.qs, q_strides, H, Nq, d);
  strides_or_dense(a.ks, k_strides, Hkv, Nk, d);
  strides_or_dense(a.vs, v_strides, Hkv, Nk, d);
  strides_or_dense(a.os, o_strides, H, Nq, d);
  if (int rc = aligned16("q", q, a.qs, esize)) return rc;
  if (int rc = aligned16("k_cache", k_cache, a.ks, esize)) return rc;
  if (int rc = aligned16("v_cache", v_cache, a.vs, esize)) return rc;
  if (int rc = aligned16("o", o, a.os, osize)) return rc;
  extend_args(a, esize, causal, m, l, H, Hkv, Nq, Nk, d, kv_len, q_len);
  a.o_f32 = osize == 4;
  return check_hip(launch_extend(a, esize == 2, B, (hipStream_t)stream), "mt_flash_attn_extend");
}

int mt_kv_cache_append(int dtype, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                       int64_t B, int64_t H, int64_t Nq, int64_t Nmax, int64_t d,
                       const int64_t* knew_strides, const int64_t* vnew_strides,
                       const int64_t* kcache_strides, const int64_t* vcache_strides,
                       const int* pos, void* stream) {
  if (dtype == MT_BF16_F32OUT) dtype = MT_BF16;  // the caches and the new rows are bf16 there
  if (dtype != MT_F32 && dtype != MT_BF16) return set_error("unsupported dtype %d", dtype);
  if (B <= 0 || H <= 0 || Nq <= 0 || Nmax <= 0 || d <= 0)
    return set_error("bad sizes B=%lld H=%lld Nq=%lld Nmax=%lld d=%lld", (long long)B, (long long)H,
                     (long long)Nq, (long long)Nmax, (long long)d);
  if (Nmax > (1 << 30) || Nq > (1 << 30) || d > 4096 || B * H > (1ll << 31) - 1)
    return set_error("sizes out of range (Nq=%lld, Nmax=%lld, d=%lld, B*H=%lld)", (long long)Nq,
                     (long long)Nmax, (long long)d, (long long)(B * H));
  const int esize = dtype == MT_F32 ? 4 : 2, epc = 16 / esize;
  if (d % epc)
    return set_error("append needs 16-B rows: d=%lld is not a multiple of %d", (long long)d, epc);
  if (!pos) return set_error("pos is NULL");
  AppendArgs a;
  a.kn = (const char*)k_new; a.vn = (const char*)v_new; a.kc = (char*)k_cache; a.vc = (char*)v_cache;
  a.pos = pos;
  strides_or_dense(a.kns, knew_strides, H, Nq, d);
  strides_or_dense(a.vns, vnew_strides, H, Nq, d);
  strides_or_dense(a.kcs, kcache_strides, H, Nmax, d);
  strides_or_dense(a.vcs, vcache_strides, H, Nmax, d);
  if (int rc = aligned16("k_new", k_new, a.kns, esize)) return rc;
  if (int rc = aligned16("v_new", v_new, a.vns, esize)) return rc;
  if (int rc = aligned16("k_cache", k_cache, a.kcs, esize)) return rc;
  if (int rc = aligned16("v_cache", v_cache, a.vcs, esize)) return rc;
  a.chunks = (int)(d / epc);
  a.total = B * H * Nq * a.chunks;
  if ((a.total + 255) / 256 > (1ll << 31) - 1) return set_error("append too large");
  a.H = (int)H; a.Nq = (int)Nq; a.Nmax = (int)Nmax; a.esize = esize;
  return check_hip(launch_kv_append(a, (hipStream_t)stream), "mt_kv_cache_append");
}

}  // extern "C"
