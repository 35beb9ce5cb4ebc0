// C ABI of the paged KV cache (include/minitorch_hip.h): mt_flash_attn_decode_paged with its
// split / workspace queries, mt_flash_attn_extend_paged with its plan query, mt_kv_cache_append_paged
// and mt_kv_cache_gather_paged. Kernels: fa_paged.hip, fa_extend.hip. Every argument is validated
// before the first device call; the decode's and the extend's sizes, strides and alignment by the
// plain ABI's checks (capi_decode.hip, declared in fa_decode.h / fa_extend.h) at Nk = W * P.
#include "../../include/minitorch_hip.h"
#include "fa_paged.h"
#include "fa_extend.h"
#include <math.h>

namespace mt {
// the page geometry: P a power of two >= 16, W and n_pages positive, W * P within the key range;
// writes log2(P); 0 or the error status
static int paged_geometry(int64_t W, int64_t P, int64_t n_pages, int* lgP) {
  if (P < 16 || (P & (P - 1)))
    return set_error("the page size must be a power of two >= 16 (P=%lld)", (long long)P);
  if (W <= 0) return set_error("the block table needs at least one column (W=%lld)", (long long)W);
  if (n_pages <= 0) return set_error("the pool needs at least one page (n_pages=%lld)", (long long)n_pages);
  if (P > (1 << 30) || W > (1 << 30) || W * P > (1 << 30) || n_pages > (1ll << 31) - 1)
    return set_error("sizes out of range (W=%lld, P=%lld, n_pages=%lld)", (long long)W, (long long)P,
                     (long long)n_pages);
  int lg = 0;
  while ((1ll << lg) < P) ++lg;
  *lgP = lg;
  return 0;
}

// the sizes of the append and the gather: mt_kv_cache_append's rules; writes the element size
static int paged_copy_sizes(int dtype, int64_t B, int64_t Hkv, int64_t N, int64_t d, int* esize) {
  if (dtype == MT_BF16_F32OUT) dtype = MT_BF16;  // the pools and the rows are bf16 there
  if (dtype != MT_F32 && dtype != MT_BF16) return set_error("unsupported dtype %d", dtype);
  if (B <= 0 || Hkv <= 0 || N <= 0 || d <= 0)
    return set_error("bad sizes B=%lld Hkv=%lld N=%lld d=%lld", (long long)B, (long long)Hkv, (long long)N,
                     (long long)d);
  if (N > (1 << 30) || d > 4096 || B * Hkv > (1ll << 31) - 1)
    return set_error("sizes out of range (N=%lld, d=%lld, B*Hkv=%lld)", (long long)N, (long long)d,
                     (long long)(B * Hkv));
  *esize = dtype == MT_F32 ? 4 : 2;
  const int epc = 16 / *esize;
  if (d % epc) return set_error("a paged cache needs 16-B rows: d=%lld is not a multiple of %d", (long long)d, epc);
  return 0;
}

static int paged_table(const int* table) {
  if (!table) return set_error("block_table is NULL");
  if ((uintptr_t)table & 3) return set_error("block_table is not 4-B aligned");
  return 0;
}
}  // namespace mt

using namespace mt;

extern "C" {

int mt_flash_attn_decode_paged_splits(int dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t W, int64_t P,
                                      int64_t d, int64_t* span_keys, int64_t* tile_keys) {
  int lgP;
  if (paged_geometry(W, P, 1, &lgP)) return 0;
  if (decode_sizes(dtype, B, H, Hkv, Nq, W * P, d)) return 0;
  const DecodePlan p = decode_plan(dtype == MT_F32 ? 4 : 2, B, H, Hkv, Nq, W * P, d);
  if (span_keys) *span_keys = p.span;
  if (tile_keys) *tile_keys = p.tile;
  return p.nsplit;
}

int64_t mt_flash_attn_decode_paged_workspace_bytes(int dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq,
                                                   int64_t W, int64_t P, int64_t d) {
  int lgP;
  if (paged_geometry(W, P, 1, &lgP)) return -1;
  if (decode_sizes(dtype, B, H, Hkv, Nq, W * P, d)) return -1;
  return decode_ws_bytes(decode_plan(dtype == MT_F32 ? 4 : 2, B, H, Hkv, Nq, W * P, d), B, H, Nq, d);
}

int mt_flash_attn_decode_paged(int dtype, int causal, const void* q, const void* k_pool, const void* v_pool,
                               void* o, float* m, float* l, int64_t B, int64_t H, int64_t Hkv, int64_t Nq,
                               int64_t W, int64_t P, int64_t n_pages, int64_t d, const int64_t* q_strides,
                               const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides,
                               const int* block_table, const int* kv_len,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  int lgP;
  if (int rc = paged_geometry(W, P, n_pages, &lgP)) return rc;
  const int64_t Nk = W * P;
  if (int rc = decode_sizes(dtype, B, H, Hkv, Nq, Nk, d)) return rc;
  if (int rc = paged_table(block_table)) return rc;
  const int esize = dtype == MT_F32 ? 4 : 2, osize = dtype == MT_BF16 ? 2 : 4;
  const DecodePlan p = decode_plan(esize, B, H, Hkv, Nq, Nk, d);
  PagedDecodeArgs pa;
  DecodeArgs& a = pa.d;
  if (int rc = decode_args(a, p, "mt_flash_attn_decode_paged_workspace_bytes", causal, q, k_pool, v_pool, o, m, l, B,
                           H, Hkv, Nq, Nk, d, kv_len, workspace, workspace_bytes))
    return rc;
  a.o_f32 = osize == 4;
  strides_or_dense(a.qs, q_strides, H, Nq, d);
  strides_or_dense(a.ks, k_strides, Hkv, P, d);
  strides_or_dense(a.vs, v_strides, Hkv, P, d);
  strides_or_dense(a.os, o_strides, H, Nq, d);
  if (int rc = aligned16("q", q, a.qs, esize)) return rc;
  if (int rc = aligned16("k_pool", k_pool, a.ks, esize)) return rc;
  if (int rc = aligned16("v_pool", v_pool, a.vs, esize)) return rc;
  if (int rc = aligned16("o", o, a.os, osize)) return rc;
  pa.table = block_table; pa.W = (int)W; pa.lgP = lgP; pa.n_pages = (int)n_pages;
  return check_hip(launch_decode_paged(pa, esize == 2, B, (hipStream_t)stream), "mt_flash_attn_decode_paged");
}

int mt_flash_attn_extend_paged_plan(int dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t W, int64_t P,
                                    int64_t d, int64_t* block_queries, int64_t* tile_keys) {
  int lgP;
  if (paged_geometry(W, P, 1, &lgP)) return -1;
  if (extend_sizes(dtype, B, H, Hkv, Nq, W * P, d)) return -1;
  const ExtendPlan p = extend_plan(dtype == MT_F32 ? 4 : 2, d);
  if (block_queries) *block_queries = p.bq;
  if (tile_keys) *tile_keys = p.bk;
  return p.kernel;
}

int mt_flash_attn_extend_paged(int dtype, int causal, const void* q, const void* k_pool, const void* v_pool,
                               void* o, float* m, float* l, int64_t B, int64_t H, int64_t Hkv, int64_t Nq,
                               int64_t W, int64_t P, int64_t n_pages, int64_t d, const int64_t* q_strides,
                               const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides,
                               const int* block_table, const int* kv_len, const int* q_len, void* stream) {
  int lgP;
  if (int rc = paged_geometry(W, P, n_pages, &lgP)) return rc;
  const int64_t Nk = W * P;
  if (int rc = extend_sizes(dtype, B, H, Hkv, Nq, Nk, d)) return rc;
  if (int rc = paged_table(block_table)) return rc;
  const int esize = dtype == MT_F32 ? 4 : 2, osize = dtype == MT_BF16 ? 2 : 4;
  PagedExtendArgs pa;
  ExtendArgs& a = pa.e;
  a.q = q; a.k = k_pool; a.v = v_pool; a.o = o;
  strides_or_dense(a.qs, q_strides, H, Nq, d);
  strides_or_dense(a.ks, k_strides, Hkv, P, d);
  strides_or_dense(a.vs, v_strides, Hkv, P, d);
  strides_or_dense(a.os, o_strides, H, Nq, d);
  if (int rc = aligned16("q", q, a.qs, esize)) return rc;
  if (int rc = aligned16("k_pool", k_pool, a.ks, esize)) return rc;
  if (int rc = aligned16("v_pool", v_pool, a.vs, esize)) return rc;
  if (int rc = aligned16("o", o, a.os, osize)) return rc;
  extend_args(a, esize, causal, m, l, H, Hkv, Nq, Nk, d, kv_len, q_len);
  a.o_f32 = osize == 4;
  pa.table = block_table; pa.W = (int)W; pa.lgP = lgP; pa.n_pages = (int)n_pages;
  return check_hip(launch_extend_paged(pa, esize == 2, B, (hipStream_t)stream), "mt_flash_attn_extend_paged");
}

int mt_kv_cache_append_paged(int dtype, const void* k_new, const void* v_new, void* k_pool, void* v_pool,
                             int64_t B, int64_t Hkv, int64_t Nq, int64_t W, int64_t P, int64_t n_pages, int64_t d,
                             const int64_t* knew_strides, const int64_t* vnew_strides,
                             const int64_t* kpool_strides, const int64_t* vpool_strides,
                             const int* block_table, const int* pos, const int* count, void* stream) {
  int lgP, esize;
  if (int rc = paged_geometry(W, P, n_pages, &lgP)) return rc;
  if (int rc = paged_copy_sizes(dtype, B, Hkv, Nq, d, &esize)) return rc;
  if (int rc = paged_table(block_table)) return rc;
  if (!pos) return set_error("pos is NULL");
  PagedAppendArgs a;
  a.kn = (const char*)k_new; a.vn = (const char*)v_new; a.kp = (char*)k_pool; a.vp = (char*)v_pool;
  a.table = block_table; a.pos = pos; a.count = count;
  strides_or_dense(a.kns, knew_strides, Hkv, Nq, d);
  strides_or_dense(a.vns, vnew_strides, Hkv, Nq, d);
  strides_or_dense(a.kps, kpool_strides, Hkv, P, d);
  strides_or_dense(a.vps, vpool_strides, Hkv, P, d);
  if (int rc = aligned16("k_new", k_new, a.kns, esize)) return rc;
  if (int rc = aligned16("v_new", v_new, a.vns, esize)) return rc;
  if (int rc = aligned16("k_pool", k_pool, a.kps, esize)) return rc;
  if (int rc = aligned16("v_pool", v_pool, a.vps, esize)) return rc;
  a.chunks = (int)(d * esize / 16);
  a.total = B * Hkv * Nq * a.chunks;
  if ((a.total + 255) / 256 > (1ll << 31) - 1) return set_error("append too large");
  a.Hkv = (int)Hkv; a.Nq = (int)Nq; a.W = (int)W; a.lgP = lgP; a.n_pages = (int)n_pages; a.esize = esize;
  return check_hip(launch_append_paged(a, (hipStream_t)stream), "mt_kv_cache_append_paged");
}

int mt_kv_cache_gather_paged(int dtype, const void* k_pool, const void* v_pool, void* k_out, void* v_out,
                             int64_t B, int64_t Hkv, int64_t W, int64_t P, int64_t n_pages, int64_t d,
                             const int64_t* kpool_strides, const int64_t* vpool_strides,
                             const int64_t* kout_strides, const int64_t* vout_strides,
                             const int* block_table, const int* kv_len, void* stream) {
  int lgP, esize;
  if (int rc = paged_geometry(W, P, n_pages, &lgP)) return rc;
  const int64_t Nk = W * P;
  if (int rc = paged_copy_sizes(dtype, B, Hkv, Nk, d, &esize)) return rc;
  if (int rc = paged_table(block_table)) return rc;
  PagedGatherArgs a;
  a.kp = (const char*)k_pool; a.vp = (const char*)v_pool; a.ko = (char*)k_out; a.vo = (char*)v_out;
  a.table = block_table; a.kv_len = kv_len;
  strides_or_dense(a.kps, kpool_strides, Hkv, P, d);
  strides_or_dense(a.vps, vpool_strides, Hkv, P, d);
  strides_or_dense(a.kos, kout_strides, Hkv, Nk, d);
  strides_or_dense(a.vos, vout_strides, Hkv, Nk, d);
  if (int rc = aligned16("k_pool", k_pool, a.kps, esize)) return rc;
  if (int rc = aligned16("v_pool", v_pool, a.vps, esize)) return rc;
  if (int rc = aligned16("k_out", k_out, a.kos, esize)) return rc;
  if (int rc = aligned16("v_out", v_out, a.vos, esize)) return rc;
  a.chunks = (int)(d * esize / 16);
  a.total = B * Hkv * Nk * a.chunks;
  if ((a.total + 255) / 256 > (1ll << 31) - 1) return set_error("gather too large");
  a.Hkv = (int)Hkv; a.Nk = (int)Nk; a.W = (int)W; a.lgP = lgP; a.n_pages = (int)n_pages; a.esize = esize;
  return check_hip(launch_gather_paged(a, (hipStream_t)stream), "mt_kv_cache_gather_paged");
}

}  // extern "C"
