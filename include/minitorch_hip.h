/*
 * minitorch_hip.h -- C ABI of libminitorch_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the reference's ctypes-loaded CUDA libraries
 * (reference minitorch/cuda_kernel_ops.py:25-29 loads combine.so, softmax_kernel.so,
 * layernorm_kernel.so, flashattention_kernel.so). Two layers:
 *
 *  1. Reference-compatible host-pointer entry points: same names, argument order
 *     and meaning as the reference's extern "C" launchers. Each copies the host
 *     arrays to the device, runs, synchronises and copies the outputs back, like
 *     the reference. Unlike the reference they never exit() the process: errors are
 *     printed to stderr and kept in mt_last_error().
 *
 *  2. Device-pointer entry points (prefix mt_): stream-ordered on a caller-supplied
 *     hipStream_t (passed as void*), int64 sizes and element strides, dtype
 *     selectable (MT_F32 / MT_BF16), return 0 on success or a nonzero status with
 *     the message in mt_last_error(). No allocation, no synchronisation inside
 *     (graph-capturable); scratch is caller-provided.
 *
 * Strides are in ELEMENTS for the (batch, head, seq) axes of a [B, H, N, d] tensor;
 * the head dimension d must be unit-stride. A NULL stride pointer means contiguous
 * [B, H, N, d].
 */
#ifndef MINITORCH_HIP_H
#define MINITORCH_HIP_H

#include <stdint.h>
#include <stdbool.h>

#ifdef __cplusplus
extern "C" {
#endif

/* MT_BF16_F32OUT (forward only): bf16 Q/K/V with an fp32 O (16-B aligned rows, strides
 * multiples of 4), the bf16 path without the final rounding of O to bf16. */
enum { MT_F32 = 0, MT_BF16 = 1, MT_BF16_F32OUT = 2 };

/* ---- status ------------------------------------------------------------- */
const char* mt_last_error(void);
int mt_abi_version(void);
/* Kernel selection for A/B timing. 0 (default): the bf16 MFMA kernels specialised for
 * d in {64, 128} where the layout allows, else the generic kernels; 1: the generic tiled
 * kernels only; other ids: alternative bf16 schedules, each computing the same attention
 * (the list and what each id selects: csrc/capi_flash.hip, enum kPol*). Returns 0, or 1
 * for an id the library does not know (the policy is then unchanged). Process-wide,
 * read atomically at each launch. */
int mt_flash_set_kernel_policy(int policy);
int mt_flash_get_kernel_policy(void);
/* Device scratch the library holds between calls (stream-ordered buffers of the zero-padded
 * head-dim copies and the column-reduction partials, one per (pool, device, stream)): its
 * bytes, and a release that frees every buffer no captured hipGraph was handed (after a
 * synchronize of the buffer's stream). Buffers are re-allocated on the next call that needs
 * them. (The reference allocates and frees inside each launcher,
 * src/flashattention_kernel.cu:319-324; here the padded copies are chunked to at most
 * 512 MiB per call.) */
int64_t mt_scratch_bytes(void);
int mt_scratch_release(void);

/* ---- FlashAttention, device pointers ------------------------------------- */
/* O = softmax(Q Kᵀ/√d [causal]) V;  m[b,h,n] = row max of the scaled logits,
 * l[b,h,n] = Σ exp(s − m)  (P = exp(s − m)/l, the reference contract,
 * src/flashattention_kernel.cu:194). m, l are fp32 [B*H*N] and may be NULL.
 * The fp32 entry points (MT_F32, forward and backward, and the host-pointer launchers below)
 * require finite Q, K, V, O and dO: they form fp32 products from three bf16 pieces per value,
 * which are NaN for a ±inf value, and may return NaN where an IEEE fp32 product gives ±inf. */
int mt_flash_attn_fwd(int dtype, int causal, const void* q, const void* k, const void* v,
                      void* o, float* m, float* l, int64_t B, int64_t H, int64_t N, int64_t d,
                      const int64_t* q_strides, const int64_t* k_strides,
                      const int64_t* v_strides, const int64_t* o_strides, void* stream);

/* The forward with key padding: kv_len is a device int32 [B] (NULL = none); keys
 * j >= kv_len[b] (clamped to [0, N]) of batch row b are masked for every head and query, as
 * the reference's [B, to_len] additive padding mask does in the fused softmax
 * (src/softmax_kernel.cu:26-33). Queries are not masked (a padded query attends the valid
 * keys). A row with kv_len = 0 gets O = 0, m = -inf, l = 0. bf16 runs the generic / ring
 * kernels here (the d = 64 / 128 MFMA schedules have no per-row key bound), and so does
 * MT_BF16_F32OUT: with kv_len its fp32 O is those kernels' result before the bf16 rounding
 * (fa_fwd_generic_ring for d <= 64, fa_fwd_generic above), the same (m, l) either way. */
int mt_flash_attn_fwd_varlen(int dtype, int causal, const void* q, const void* k, const void* v,
                             void* o, float* m, float* l, int64_t B, int64_t H, int64_t N,
                             int64_t d, const int64_t* q_strides, const int64_t* k_strides,
                             const int64_t* v_strides, const int64_t* o_strides,
                             const int* kv_len, void* stream);

/* Scratch bytes the backward needs: fp32 δ and log2-LSE per row (256-B aligned) and, at
 * d = 64 (N <= 46336), the fused bf16 backward's arrival counters and the dQ partial sums of
 * one group of heads (at most 1 GiB). The layout changed in ABI version 3: size the workspace
 * with this function, never by a formula (mt_flash_attn_bwd_v3 checks the size). */
int64_t mt_flash_attn_bwd_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t d);

/* dQ, dK, dV of the forward above, from Q, K, V, O, dO and the forward's (m, l).
 * strides: NULL or 8 consecutive triples for q, k, v, o, dout, dq, dk, dv. */
int mt_flash_attn_bwd(int dtype, int causal, const void* q, const void* k, const void* v,
                      const void* o, const void* dout, const float* m, const float* l,
                      void* dq, void* dk, void* dv, int64_t B, int64_t H, int64_t N,
                      int64_t d, const int64_t* strides, void* workspace, void* stream);
/* The backward of mt_flash_attn_fwd_varlen (same kv_len): padding keys get dK = dV = 0 and
 * add nothing to dQ. */
int mt_flash_attn_bwd_varlen(int dtype, int causal, const void* q, const void* k, const void* v,
                             const void* o, const void* dout, const float* m, const float* l,
                             void* dq, void* dk, void* dv, int64_t B, int64_t H, int64_t N,
                             int64_t d, const int64_t* strides, const int* kv_len,
                             void* workspace, void* stream);
/* ABI 3: mt_flash_attn_bwd_varlen (kv_len may be NULL) with the workspace's size in bytes;
 * returns an error, launching nothing, when it is below mt_flash_attn_bwd_workspace_bytes. */
int mt_flash_attn_bwd_v3(int dtype, int causal, const void* q, const void* k, const void* v,
                         const void* o, const void* dout, const float* m, const float* l,
                         void* dq, void* dk, void* dv, int64_t B, int64_t H, int64_t N,
                         int64_t d, const int64_t* strides, const int* kv_len,
                         void* workspace, int64_t workspace_bytes, void* stream);

/* ---- KV-cache decode attention, device pointers ---------------------------- */
/* Generation: Nq (1..8) new query rows per (batch, head) against a cache of Nk key / value
 * rows, of which the first n = clamp(kv_len[b], 0, Nk) are visible (kv_len: device int32 [B];
 * NULL = Nk). The queries are the LAST Nq positions of the row: with causal != 0 query i sees
 * the keys j < n - Nq + 1 + i (the causal mask aligned bottom-right), else every key j < n.
 * A query with no visible key gets O = 0, m = -inf, l = 0. Rows j >= n are never read: the
 * cache tail may be uninitialised memory.
 *   q, o:              [B, H, Nq, d], strides (batch, head, row) in elements, NULL = contiguous
 *   k_cache, v_cache:  [B, H, Nk, d] likewise (e.g. [B, Nk, H, d] storage seen through strides)
 *   m, l:              fp32 [B*H*Nq] or NULL; m + log(l) is the row's log-sum-exp
 * dtype: MT_F32, MT_BF16, or MT_BF16_F32OUT (bf16 Q/K/V, fp32 O). Requires 1 <= Nq <= 8,
 * d <= 256 and 16-B rows: d, every stride and every base pointer a multiple of 16 bytes;
 * anything else returns a status before any device call.
 * The keys are split over mt_flash_attn_decode_splits workgroups per (b, h), each writing its
 * fp32 (m, l, unnormalised O) to the workspace ([B*H*Nq*splits][d] O, then [B*H*Nq*splits][2]
 * (m in log2 units, l); nothing with one split), merged in split order by a second launch on
 * the same stream: bit-reproducible. The split count is a function of the arguments of
 * mt_flash_attn_decode_splits only, never of kv_len, so a captured launch can be replayed as
 * the cache fills. A workspace below mt_flash_attn_decode_workspace_bytes is an error and
 * launches nothing. */
int mt_flash_attn_decode_splits(int dtype, int64_t B, int64_t H, int64_t Nq, int64_t Nk, int64_t d,
                                int64_t* span_keys, int64_t* tile_keys);
/* returns the split count (>= 1), or <= 0 on bad sizes; span_keys: keys per split;
 * tile_keys: keys one wave takes per inner step (either may be NULL) */
int64_t mt_flash_attn_decode_workspace_bytes(int dtype, int64_t B, int64_t H, int64_t Nq, int64_t Nk,
                                             int64_t d);
int mt_flash_attn_decode(int dtype, int causal, const void* q, const void* k_cache, const void* v_cache,
                         void* o, float* m, float* l, int64_t B, int64_t H, int64_t Nq, int64_t Nk,
                         int64_t d, const int64_t* q_strides, const int64_t* k_strides,
                         const int64_t* v_strides, const int64_t* o_strides, const int* kv_len,
                         void* workspace, int64_t workspace_bytes, void* stream);
/* Grouped-query decode: H query heads share Hkv key / value heads in groups of G = H / Hkv
 * (Hkv = 1: multi-query); query head h reads kv head h / G.
 *   q, o:              [B, H, Nq, d]
 *   k_cache, v_cache:  [B, Hkv, Nk, d] (NULL strides: dense [B, Hkv, Nk, d])
 *   m, l:              fp32 [B*H*Nq], indexed by query head
 * Row packing: one workgroup serves one kv head and gs = min(G, 8 / Nq) query heads of its
 * group, Nq queries each (its row r is head hkv*G + slice*gs + r / Nq, query r % Nq), so a
 * group's K and V are read ceil(G / gs) times per step instead of G times. The workspace is laid
 * out as above, per (b, query head, query, split): B*H*Nq*splits*(d+2)*4 bytes, 0 with one split.
 * The split count and span are those mt_flash_attn_decode_splits gives for (dtype, B, H, Nq, Nk,
 * d), whatever Hkv (a packed workgroup streams the keys a plain one does), never of kv_len.
 * Hkv == H is mt_flash_attn_decode: the same plan, launches and bits. Refused before any device
 * call: Hkv <= 0, Hkv > H, H % Hkv != 0, and whatever mt_flash_attn_decode refuses. */
int mt_flash_attn_decode_gqa_splits(int dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk,
                                    int64_t d, int64_t* span_keys, int64_t* tile_keys);
int64_t mt_flash_attn_decode_gqa_workspace_bytes(int dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq,
                                                 int64_t Nk, int64_t d);
int mt_flash_attn_decode_gqa(int dtype, int causal, const void* q, const void* k_cache, const void* v_cache,
                             void* o, float* m, float* l, int64_t B, int64_t H, int64_t Hkv, int64_t Nq,
                             int64_t Nk, int64_t d, const int64_t* q_strides, const int64_t* k_strides,
                             const int64_t* v_strides, const int64_t* o_strides, const int* kv_len,
                             void* workspace, int64_t workspace_bytes, void* stream);
/* Extend step: Nq >= 1 new query rows per (batch, head) at the END of a row of cached keys, of
 * which t = clamp(q_len[b], 0, Nq) are real (q_len: device int32 [B]; NULL = Nq; the batch is
 * right-padded). n = clamp(kv_len[b], 0, Nk) is the number of keys row b holds AFTER its new
 * rows were appended (kv_len: device int32 [B]; NULL = Nk). Query i < t sits at position
 * n - t + i: with causal != 0 it sees the keys j < clamp(n - t + 1 + i, 0, n) (the causal mask
 * aligned bottom-right), else every key j < n. A query i >= t, or one with no visible key, gets
 * O = 0, m = -inf, l = 0 exactly. With q_len = NULL and Nq <= 8 this is
 * mt_flash_attn_decode_gqa's contract.
 *   q, o:              [B, H, Nq, d], strides (batch, head, row) in elements, NULL = contiguous
 *   k_cache, v_cache:  [B, Hkv, Nk, d] likewise; query head h reads kv head h / (H / Hkv)
 *   m, l:              fp32 [B*H*Nq] or NULL; m + log(l) is the row's log-sum-exp
 * Cache rows j >= n and Q rows i >= t are never read (the cache tail may be uninitialised
 * memory): their loads are predicated on the row and the logits replaced by -inf through a
 * select, so no product is formed with such a row's data.
 * dtype: MT_F32, MT_BF16, or MT_BF16_F32OUT (bf16 Q/K/V, fp32 O). fp32 with d <= 64 runs both
 * products on the bf16 MFMA with three bf16 pieces per operand (fp32 accuracy), fp32 above that
 * on the fp32 MFMA. Requires 1 <= Nq <= Nk, d <= 256 and 16-B rows as decode defines them: d,
 * every stride and every base pointer a multiple of 16 bytes.
 * Refused with a status and a mt_last_error() message before any device call: whatever
 * mt_flash_attn_decode_gqa refuses (but for Nq > 8), Nq > Nk, Hkv <= 0, Hkv > H, H % Hkv != 0.
 * One launch on the caller's stream: no workspace, no allocation, no synchronisation, plain
 * stores only. The launch (grid and kernel) is a function of the sizes alone, never of kv_len
 * or q_len, which only set loop bounds read on the device: a captured launch can be replayed
 * as the cache fills. A workgroup owns block_queries query rows of one (b, h) and streams the
 * keys in tiles of tile_keys; a workgroup whose queries are all >= t loads nothing.
 * mt_flash_attn_extend_plan: the kernel id (>= 0) mt_flash_attn_extend launches at these sizes
 * (the launcher dispatches through the same function), or a negative value with a message; it
 * writes the query rows per workgroup and the keys per inner tile (either may be NULL) and
 * makes no device call. */
int mt_flash_attn_extend_plan(int dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk,
                              int64_t d, int64_t* block_queries, int64_t* tile_keys);
int mt_flash_attn_extend(int dtype, int causal, const void* q, const void* k_cache, const void* v_cache,
                         void* o, float* m, float* l, int64_t B, int64_t H, int64_t Hkv, int64_t Nq,
                         int64_t Nk, int64_t d, const int64_t* q_strides, const int64_t* k_strides,
                         const int64_t* v_strides, const int64_t* o_strides,
                         const int* kv_len, const int* q_len, void* stream);
/* Copies the Nq new K and V rows of every (b, h) ([B, H, Nq, d]) into the caches
 * ([B, H, Nmax, d]) at rows pos[b] .. pos[b] + Nq - 1 (pos: device int32 [B]); rows outside
 * [0, Nmax) are dropped and nothing else in the caches is written. 16-B rows as above. */
int mt_kv_cache_append(int dtype, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                       int64_t B, int64_t H, int64_t Nq, int64_t Nmax, int64_t d,
                       const int64_t* knew_strides, const int64_t* vnew_strides,
                       const int64_t* kcache_strides, const int64_t* vcache_strides,
                       const int* pos, void* stream);

/* ---- quantised KV cache ------------------------------------------------------
 * K and V stored as bf16 (MT_KV_BF16) or as one byte of OCP e4m3 (MT_KV_FP8: "e4m3fn", bias 7,
 * max 448, no inf, NaN = 0x7F / 0xFF) with one fp32 scale per cached row: a row's values are
 * scale * e4m3(code). Queries, arithmetic, O, m and l stay fp32.
 *   k_cache, v_cache:  [B, Hkv, Nmax, d] through strides in storage elements (bf16, or bytes),
 *                      NULL = contiguous
 *   k_scale, v_scale:  fp8: dense fp32 [B, Hkv, Nmax]; bf16: ignored (pass NULL)
 * Requires d % 8 == 0, d <= 256, unit-stride d, and every row start (base pointer and strides) a
 * multiple of 8 bytes for fp8 and of 16 bytes for bf16. Refused with a status and a
 * mt_last_error() message before any device call: an unknown kv_dtype, fp8 with a NULL scale
 * pointer, d % 8, d > 256, non-positive sizes, misaligned pointers or strides, and for decode Nq
 * outside 1..8, Hkv not dividing H and a workspace below ..._workspace_bytes.
 *
 * mt_kv_cache_append_quant: mt_kv_cache_append's footprint (rows pos[b] .. pos[b] + Nq - 1 of
 * every (b, hkv); rows outside [0, Nmax) dropped; nothing else in the caches or the scales is
 * written) from fp32 new rows [B, Hkv, Nq, d] of any 4-B aligned strides (unit-stride d).
 * bf16: round to nearest even. fp8: amax = the largest |x| of the row's d elements,
 * s = amax > 0 ? amax / 448 : 1, codes = e4m3 round-to-nearest of x / s (fp32 division), s stored
 * at the row's scale slot; a row holding an inf or a NaN is stored as NaN codes (0x7F) with a NaN
 * scale. Plain vector stores, no atomics.
 *
 * mt_flash_attn_decode_kvq: mt_flash_attn_decode_gqa's contract (Nq <= 8, bottom-right causal
 * alignment, (0, -inf, 0) for a query with no visible key, rows >= n never loaded and their
 * scales neither, row packing, two plain launches, fixed-order combine, the same workspace
 * layout) with fp32 q / o / m / l ([B, H, Nq, d], 16-B rows) and quantised caches. Both formats
 * are read in chunks of 8 elements, so the plan (splits, span, tile, packing) is the one
 * mt_flash_attn_decode_gqa_splits gives for MT_BF16 at the same sizes: a function of the sizes
 * only.
 *
 * mt_kv_cache_dequant: writes the fp32 rows j < clamp(kv_len[b], 0, Nk) (kv_len NULL: Nk) of
 * k_out / v_out ([B, Hkv, Nk, d] through strides in elements, 16-B rows): bf16 widened, fp8
 * e4m3(code) * scale (one fp32 product). Rows at or past that count are neither read nor written.
 *
 * mt_flash_attn_extend_kvq: mt_flash_attn_extend's contract (any 1 <= Nq <= Nk, q_len, bottom-right
 * causal alignment, (0, -inf, 0) for a query >= t or one with no visible key, one plain launch, no
 * workspace, a launch that is a function of the sizes alone) with fp32 q / o / m / l and quantised
 * caches read in place: rows are loaded in chunks of 8 elements and widened in registers with
 * mt_kv_cache_dequant's formulas, so O, m and l have the bits of mt_flash_attn_extend(MT_F32) on
 * the fp32 cache that mt_kv_cache_dequant writes from the same rows. Rows j >= n are never loaded
 * and their scales neither. mt_flash_attn_extend_kvq_plan answers as mt_flash_attn_extend_plan does
 * for MT_F32 at the same sizes. Refused: whatever mt_flash_attn_extend refuses for MT_F32 (Nq > Nk
 * included) and the cache arguments this block's first paragraph lists. */
enum { MT_KV_BF16 = 1, MT_KV_FP8 = 2 };
int mt_flash_attn_decode_kvq_splits(int kv_dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk,
                                    int64_t d, int64_t* span_keys, int64_t* tile_keys);
int64_t mt_flash_attn_decode_kvq_workspace_bytes(int kv_dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq,
                                                 int64_t Nk, int64_t d);
int mt_flash_attn_decode_kvq(int kv_dtype, int causal, const void* q, const void* k_cache, const void* v_cache,
                             const float* k_scale, const float* v_scale, void* o, float* m, float* l,
                             int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk, int64_t d,
                             const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                             const int64_t* o_strides, const int* kv_len,
                             void* workspace, int64_t workspace_bytes, void* stream);
int mt_flash_attn_extend_kvq_plan(int kv_dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk,
                                  int64_t d, int64_t* block_queries, int64_t* tile_keys);
int mt_flash_attn_extend_kvq(int kv_dtype, int causal, const void* q, const void* k_cache, const void* v_cache,
                             const float* k_scale, const float* v_scale, void* o, float* m, float* l,
                             int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk, int64_t d,
                             const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                             const int64_t* o_strides, const int* kv_len, const int* q_len, void* stream);
int mt_kv_cache_append_quant(int kv_dtype, const float* k_new, const float* v_new, void* k_cache, void* v_cache,
                             float* k_scale, float* v_scale, int64_t B, int64_t Hkv, int64_t Nq, int64_t Nmax,
                             int64_t d, const int64_t* knew_strides, const int64_t* vnew_strides,
                             const int64_t* kcache_strides, const int64_t* vcache_strides,
                             const int* pos, void* stream);
int mt_kv_cache_dequant(int kv_dtype, const void* k_cache, const void* v_cache, const float* k_scale,
                        const float* v_scale, float* k_out, float* v_out, int64_t B, int64_t Hkv, int64_t Nk,
                        int64_t d, const int64_t* kcache_strides, const int64_t* vcache_strides,
                        const int64_t* kout_strides, const int64_t* vout_strides, const int* kv_len, void* stream);

/* ---- paged KV cache ----------------------------------------------------------
 * K and V rows live in pages of P rows (P a power of two >= 16) taken from a pool, per layer and
 * per K / V:
 *   k_pool, v_pool:  [n_pages, Hkv, P, d] through strides (page, head, row) in elements,
 *                    NULL = contiguous; unit-stride d, 16-B rows as decode defines them
 *   block_table:     device int32 [B, W], dense. Logical key j of batch row b is row j % P of
 *                    page block_table[b][j / P]; the logical capacity is Nk = W * P. A negative
 *                    entry is an unallocated page.
 * Refused with a status and a mt_last_error() message before any device call: P not a power of
 * two or below 16, W <= 0, n_pages <= 0, a NULL block_table, and whatever
 * mt_flash_attn_decode_gqa (decode) or mt_kv_cache_append (append, gather) refuses: Nq outside
 * 1..8, Hkv not dividing H, d > 256, rows not 16-B aligned, a short workspace.
 *
 * mt_flash_attn_decode_paged: mt_flash_attn_decode_gqa's contract (dtypes, 1 <= Nq <= 8,
 * bottom-right causal alignment, row packing, (0, -inf, 0) for a query with no visible key, two
 * plain launches, fixed-order combine, the same workspace layout) on a paged cache. The plan
 * (splits, span, tile, packing, workspace bytes) is the one mt_flash_attn_decode_gqa_splits gives
 * at Nk = W * P: a function of the sizes only, never of kv_len or of the table's contents, so a
 * captured launch replays as the cache fills. The arithmetic and its order are the plain
 * kernel's: O, m and l have the bits mt_flash_attn_decode_gqa gives on a contiguous cache that
 * holds the same rows. With n = clamp(kv_len[b], 0, W * P), no table entry at index
 * >= ceil(n / P) is read and no pool row of a key >= n; every table entry below that must be a
 * page of the pool. Decode does NOT detect an entry that is not: an entry outside [0, n_pages),
 * a negative (unallocated) one included, is clamped into the range (a negative one reads the last
 * page), so its rows enter the softmax as valid keys: a silently wrong result, never an address
 * outside the pool. (Append and gather drop such rows instead.) The caller keeps the entries
 * below ceil(n / P) allocated.
 *
 * mt_kv_cache_append_paged: writes the new rows k_new / v_new ([B, Hkv, Nq, d], any 16-B-row
 * strides) to the logical rows pos[b] .. pos[b] + cnt - 1 of batch row b, cnt =
 * clamp(count[b], 0, Nq) (pos, count: device int32 [B]; count NULL = Nq). Dropped: rows past cnt,
 * logical rows outside [0, W * P), rows whose table entry is negative (or >= n_pages). Nothing
 * else in the pools is written. dtype: MT_F32 or MT_BF16 (MT_BF16_F32OUT is taken as MT_BF16).
 *
 * mt_kv_cache_gather_paged: writes the rows j < clamp(kv_len[b], 0, W * P) (kv_len NULL: W * P) of
 * the contiguous k_out / v_out ([B, Hkv, W * P, d] through strides in elements, 16-B rows) from
 * the pools. Rows at or past that count are neither read nor written (and no table entry at
 * index >= ceil(n / P) is read).
 *
 * mt_flash_attn_extend_paged: mt_flash_attn_extend's contract (dtypes, any 1 <= Nq <= Nk = W * P,
 * q_len, bottom-right causal alignment, (0, -inf, 0) for a query >= t or one with no visible key,
 * one plain launch, no workspace) on a paged cache read in place, the page resolved per loaded
 * row, so P may be smaller or larger than a key tile. The launch is a function of the sizes alone,
 * never of kv_len, q_len or the table's contents; mt_flash_attn_extend_paged_plan answers as
 * mt_flash_attn_extend_plan does at Nk = W * P. The arithmetic and its order are the plain kernel's:
 * O, m and l have the bits mt_flash_attn_extend gives on a contiguous cache that holds the same
 * rows. No table entry at index >= ceil(n / P) is read and no pool row of a key >= n. As in decode,
 * an entry outside [0, n_pages), a negative one included, is NOT detected but clamped into the
 * range (a negative one reads the last page): a silently wrong result, never an address outside
 * the pool. Refused: whatever mt_flash_attn_extend refuses at Nk = W * P and the geometry and
 * table arguments listed above. */
int mt_flash_attn_decode_paged_splits(int dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t W,
                                      int64_t P, int64_t d, int64_t* span_keys, int64_t* tile_keys);
int64_t mt_flash_attn_decode_paged_workspace_bytes(int dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq,
                                                   int64_t W, int64_t P, int64_t d);
int mt_flash_attn_decode_paged(int dtype, int causal, const void* q, const void* k_pool, const void* v_pool,
                               void* o, float* m, float* l, int64_t B, int64_t H, int64_t Hkv, int64_t Nq,
                               int64_t W, int64_t P, int64_t n_pages, int64_t d, const int64_t* q_strides,
                               const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides,
                               const int* block_table, const int* kv_len,
                               void* workspace, int64_t workspace_bytes, void* stream);
int mt_flash_attn_extend_paged_plan(int dtype, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t W,
                                    int64_t P, int64_t d, int64_t* block_queries, int64_t* tile_keys);
int mt_flash_attn_extend_paged(int dtype, int causal, const void* q, const void* k_pool, const void* v_pool,
                               void* o, float* m, float* l, int64_t B, int64_t H, int64_t Hkv, int64_t Nq,
                               int64_t W, int64_t P, int64_t n_pages, int64_t d, const int64_t* q_strides,
                               const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides,
                               const int* block_table, const int* kv_len, const int* q_len, void* stream);
int mt_kv_cache_append_paged(int dtype, const void* k_new, const void* v_new, void* k_pool, void* v_pool,
                             int64_t B, int64_t Hkv, int64_t Nq, int64_t W, int64_t P, int64_t n_pages, int64_t d,
                             const int64_t* knew_strides, const int64_t* vnew_strides,
                             const int64_t* kpool_strides, const int64_t* vpool_strides,
                             const int* block_table, const int* pos, const int* count, void* stream);
int mt_kv_cache_gather_paged(int dtype, const void* k_pool, const void* v_pool, void* k_out, void* v_out,
                             int64_t B, int64_t Hkv, int64_t W, int64_t P, int64_t n_pages, int64_t d,
                             const int64_t* kpool_strides, const int64_t* vpool_strides,
                             const int64_t* kout_strides, const int64_t* vout_strides,
                             const int* block_table, const int* kv_len, void* stream);

/* ---- generation: the next token chosen on the device ------------------------
 * One id per row of the fp32 logits [B, V] (rows row_stride >= V elements apart, unit-stride
 * columns; what lies between the rows is never read). Stream-ordered, allocates nothing, does
 * not synchronise, capturable in a hipGraph. V <= 32768 (the kernel holds one row in LDS).
 *   temperature == 0 (greedy): the lowest index that holds the row's maximum; a NaN counts as
 *     the maximum and the first NaN wins (np.argmax).
 *   temperature > 0 (sampling): the kept set K is the top_k largest entries under the order
 *     (fp32 value descending, index ascending; -0 == +0), every entry when top_k <= 0 or
 *     top_k >= V. p_i = exp((x_i - max_K x) / T) / sum over K. u is the value
 *     mt_rand_uniform(out, B, seed) writes at index b. The id is the first i in K, in index
 *     order, whose running sum of p over K exceeds u (the comparison is made on the unnormalised
 *     sums against u times their total), the last index of K with p > 0 if rounding leaves
 *     none (never an entry of p = 0, such as a -inf logit or an underflowed exp). Entries of
 *     -inf have p = 0. A row whose maximum is not finite (a NaN, +inf, or every entry -inf)
 *     takes the greedy id. top_k == 1 therefore equals greedy.
 *   Every sum has a fixed order: the id is a function of the row's bits, T, top_k, the seed and
 *   b alone, whatever else is in the batch.
 * seed_dev != NULL: the seed is read from that device uint64 when the kernel runs (a captured
 * step whose seed advances on the device); `seed` is then ignored.
 * Outputs, written with plain stores: next_f32[b] = id as a float (the token ids minitorch
 * feeds mt_embedding_fw) and / or next_i32[b] = id (either may be NULL, not both);
 * done (NULL or [B], in/out): done[b] |= (id == eos_id), never cleared; eos_id < 0: no eos;
 * history (NULL or [B] rows of history_stride ints; needs step_dev): history[b * history_stride
 * + *step_dev] = id, *step_dev a device int32 read when the kernel runs; a step outside
 * [0, history_stride) writes nothing.
 * Refused with a status before any device call: B or V <= 0, V > 32768, row_stride < V, a
 * negative or NaN temperature, NULL logits, both outputs NULL, history without step_dev. */
int mt_select_token(const float* logits, int64_t B, int64_t V, int64_t row_stride, float temperature,
                    int64_t top_k, uint64_t seed, const uint64_t* seed_dev, int64_t eos_id,
                    float* next_f32, int32_t* next_i32, int32_t* done, int32_t* history,
                    int64_t history_stride, const int32_t* step_dev, void* stream);

/* mt_select_token_p: mt_select_token with two more filters on the kept set, applied after
 * temperature and top_k in the usual order (temperature, top-k, top-p, min-p). Everything above
 * holds; mt_select_token is this entry at top_p = 1, min_p = 0, where the launch is the same one.
 * With e_i = exp((x_i - max_K x) / T) in fp32 for i in K (so the largest is exactly 1), and K
 * taken in the order (e_i descending, index ascending) - K's own order, except that logits so
 * close that their e_i round to one fp32 value count as equal:
 *   top_p in (0, 1], 1 is off: N is the shortest prefix of K whose mass reaches top_p times the
 *     mass of K. Entries equal in value at the boundary enter in index order, only as many as
 *     are needed (top_k's tie rule). N always holds the first entry of K. The mass of an entry
 *     is the integer trunc(e_i 2^40) and the target the fp64 product rounded up, so the prefix
 *     is exact integer arithmetic; an entry of e_i < 2^-40 weighs nothing and is never needed.
 *   min_p in [0, 1], 0 is off: M is the entries of K with e_i >= min_p, that is
 *     p_i >= min_p p_max. All ties stay; M is a prefix of K's order too.
 *   The kept set is N intersected with M, the shorter of the two prefixes; p is renormalised
 *   over it, and the id is the first kept i, in index order, whose running sum exceeds u times
 *   the kept total (the fallback is mt_select_token's: the last kept index with p > 0).
 *   temperature == 0 (greedy) ignores both, as it ignores top_k, and a row whose maximum is not
 *   finite takes the greedy id.
 * The id is a function of the row's bits, T, top_k, top_p, min_p, the seed and b alone: every
 * sum has a fixed order or is an exact integer sum (no floating-point atomics).
 * Refused with a status before any device call: top_p NaN, <= 0 or > 1; min_p NaN, < 0 or > 1;
 * whatever mt_select_token refuses. */
int mt_select_token_p(const float* logits, int64_t B, int64_t V, int64_t row_stride, float temperature,
                      int64_t top_k, float top_p, float min_p, uint64_t seed, const uint64_t* seed_dev,
                      int64_t eos_id, float* next_f32, int32_t* next_i32, int32_t* done, int32_t* history,
                      int64_t history_stride, const int32_t* step_dev, void* stream);

/* ---- speculative decoding: prompt-lookup drafts, verified on the device ------
 * Both entries are stream-ordered, allocate nothing, do not synchronise, write with plain stores
 * and are capturable in a hipGraph; their launches depend on the sizes alone.
 *
 * mt_spec_draft: tokens is int32 [B, S] (rows token_stride >= S apart, read only): row b holds
 * its prompt followed by everything emitted so far, held[b] (device int32) tokens in all. Per
 * row, with L = clamp(held[b], 1, S):
 *   feed[b, 0] = tokens[b, L - 1] (the token the next step feeds anyway);
 *   for g = min(max_ngram, L - 1) down to 1: the largest s in [0, L - g - 1] with
 *     tokens[b, s .. s + g) == tokens[b, L - g .. L); the first g that has a match wins;
 *   the k drafts feed[b, 1 + i] = ext[s + g + i], ext being tokens[b, :L] with every draft
 *     appended as it is made (a match near the end continues periodically into itself), and
 *     n_draft[b] = k; with no match at any g, n_draft[b] = 0 and the k slots hold feed[b, 0].
 * feed_f32 / feed_i32: dense [B, k + 1], the ids as floats (what mt_embedding_fw reads) and / or
 * as int32 (either may be NULL, not both). One 256-thread workgroup per row.
 * Refused with a status before any device call: k outside 1..7, max_ngram outside 1..8, B or
 * S <= 0, S < k + 2, token_stride < S, NULL tokens / held / n_draft, both outputs NULL.
 *
 * mt_spec_accept: logits is fp32 [B, k + 1, V] (batch rows batch_stride, rows row_stride >= V
 * elements apart, unit-stride columns, V <= 32768), row i of batch row b being the model's
 * output after feed[b, 0 .. i]. A batch row with done[b] != 0 on entry changes nothing. Else:
 *   1. c_i, i = 0..k, is the id mt_select_token defines for the row logits[b, i] with seed
 *      (seed_dev ? *seed_dev : seed) + count[b] + i and the uniform at index b: the token the
 *      non-speculative path chooses as the row's token number count[b] + i (greedy and sampling
 *      rules, NaN and tie rules and the fixed-order sums are mt_select_token's, one kernel).
 *   2. a = the number of leading i < n_draft[b] with feed[b, 1 + i] == c_i (a padding slot past
 *      n_draft never counts).
 *   3. e = min(a + 1, limit[b] - count[b]). c_0 .. c_{e-1} are written to
 *      history[b, count[b] + j] and tokens[b, held[b] + j] (a slot outside the row is dropped),
 *      stopping after the first of them that equals eos_id (eos_id < 0: no eos), which is still
 *      written and sets done[b]. With e' ids written: count[b], held[b] and cache_len[b] grow
 *      by e' (the fed tokens 0 .. e'-1 are then exactly what the KV cache holds: cache_len ==
 *      held - 1 is kept); done[b] |= count[b] == limit[b]; drafted[b] += n_draft[b];
 *      accepted[b] += min(a, e' - 1); steps[b] += 1.
 * scratch: device int32 [B, k + 1], the caller's, holds c between the two launches (one
 * workgroup per logits row, then one thread per batch row). cache_len, drafted, accepted and
 * steps may be NULL. The rejected drafts' K / V rows stay in the cache past cache_len, where
 * nothing reads them and the next step overwrites them.
 * Refused with a status before any device call: k outside 1..7, B, V or S <= 0, V > 32768,
 * S < k + 2, row_stride < V, batch_stride < k row_stride + V, token_stride < S, history_stride
 * <= 0, a negative or NaN temperature, a NULL required pointer.
 *
 * mt_spec_accept_p: mt_spec_accept whose step 1 chooses c_i by mt_select_token_p's rule (top_p,
 * min_p after top_k; the same kernel), so that speculative ids stay those of the non-speculative
 * call; mt_spec_accept is this entry at top_p = 1, min_p = 0. It also refuses top_p NaN, <= 0 or
 * > 1 and min_p NaN, < 0 or > 1. */
int mt_spec_draft(const int32_t* tokens, int64_t B, int64_t S, int64_t token_stride, const int32_t* held,
                  int64_t k, int64_t max_ngram, float* feed_f32, int32_t* feed_i32, int32_t* n_draft,
                  void* stream);
int mt_spec_accept(const float* logits, int64_t B, int64_t k, int64_t V, int64_t batch_stride,
                   int64_t row_stride, const int32_t* feed_i32, const int32_t* n_draft, float temperature,
                   int64_t top_k, uint64_t seed, const uint64_t* seed_dev, int64_t eos_id,
                   const int32_t* limit, int32_t* count, int32_t* held, int32_t* cache_len, int32_t* done,
                   int32_t* drafted, int32_t* accepted, int32_t* steps, int32_t* tokens, int64_t S,
                   int64_t token_stride, int32_t* history, int64_t history_stride, int32_t* scratch,
                   void* stream);
int mt_spec_accept_p(const float* logits, int64_t B, int64_t k, int64_t V, int64_t batch_stride,
                     int64_t row_stride, const int32_t* feed_i32, const int32_t* n_draft, float temperature,
                     int64_t top_k, float top_p, float min_p, uint64_t seed, const uint64_t* seed_dev,
                     int64_t eos_id, const int32_t* limit, int32_t* count, int32_t* held, int32_t* cache_len,
                     int32_t* done, int32_t* drafted, int32_t* accepted, int32_t* steps, int32_t* tokens,
                     int64_t S, int64_t token_stride, int32_t* history, int64_t history_stride,
                     int32_t* scratch, void* stream);

/* ---- rotary position embedding (RoPE) ---------------------------------------
 * The head rows of x [B, H, T, d] rotated by their positions, in the half-split ("rotate-half")
 * convention: element j < d/2 of a row pairs with element j + d/2, and at position p
 *   out[j]       = x[j]       * cos[p][j] - x[j + d/2] * sin[p][j]
 *   out[j + d/2] = x[j + d/2] * cos[p][j] + x[j]       * sin[p][j]
 * inverse != 0 uses -sin: the transpose of the rotation, which is its inverse and its backward.
 * cos / sin: dense fp32 device tables [n_pos, d/2] built by the host (no sincosf runs on the
 * device: the result is a function of x and the table rows alone, each output two rounded
 * products and one rounded sum, or tighter where the compiler fuses them).
 * x / out: (batch, head, token) element strides with unit-stride d; NULL strides mean dense.
 * x2 / out2 / H2: an optional second tensor [B, H2, T, d] (K beside Q) rotated in the same
 * launch at the same positions; x2 == NULL skips it (out2, H2 and its strides are ignored).
 * Token t of batch row b sits at p = min(max(pos0[b], 0) + t, n_pos - 1): pos0 is a device
 * int32 [B] read when the kernel runs (a KV cache's lengths; a captured launch replays), or NULL
 * for 0. The clamp is where padding slots past the last position land; no table row outside
 * [0, n_pos) is read.
 * out == x with equal strides (in place) is allowed: one thread owns both halves of its pairs
 * and loads both before it stores. Any other overlap of inputs and outputs is undefined.
 * Nothing but the d elements of each addressed row is written. Allocates nothing, does not
 * synchronise, stream-ordered. dtype: MT_F32 only. With d % 8 == 0, 16-B aligned x, out, cos,
 * sin and strides divisible by 4 the kernel moves 16 B per access, otherwise one pair per
 * thread; the choice depends on the arguments alone, never on pos0's contents.
 * Refused with a status before any device call: B, T, H, d or n_pos <= 0; d odd; d > 256;
 * dtype != MT_F32; x, out, cos or sin NULL; x2 given with out2 NULL or with H2 <= 0; 2^31 or
 * more pairs in one launch (B (H + H2) T d / 2: the kernels index them in 32 bits). */
int mt_rope(int dtype, int inverse,
            const void* x, void* out, int64_t H, const int64_t* x_strides, const int64_t* out_strides,
            const void* x2, void* out2, int64_t H2, const int64_t* x2_strides, const int64_t* out2_strides,
            int64_t B, int64_t T, int64_t d, const float* cos, const float* sin, int64_t n_pos,
            const int* pos0, void* stream);

/* ---- FlashAttention, reference-compatible host pointers (fp32) ------------ */
/* reference src/flashattention_kernel.cu:259 */
void launch_flashattention_forward(float* Q, float* K, float* V, float* O, float* l, float* m,
                                   int B, int nh, int N, int d);
/* reference src/flashattention_kernel.cu:352 */
void launch_flashattention_backward(float* Q, float* K, float* V, float* O, float* dQ,
                                    float* dK, float* dV, float* dO, float* l, float* m, int B,
                                    int nh, int N, int d);
/* reference src/flashattention_kernel.cu:694 */
void launch_flashattention_forward_causal(float* Q, float* K, float* V, float* O, float* l,
                                          float* m, int B, int nh, int N, int d);
/* reference src/flashattention_kernel.cu:761 */
void launch_flashattention_backward_causal(float* Q, float* K, float* V, float* O, float* dQ,
                                           float* dK, float* dV, float* dO, float* l,
                                           float* m, int B, int nh, int N, int d);


/* ---- companion kernels, device pointers (fp32) ---------------------------- */
/* Row softmax over [B, nh, from, to]: out = exp(x + mask - max) / (sum + 1e-8); out may
 * alias inp. mask: NULL or any tensor broadcastable to [B, nh, from, to] given by 4
 * element strides (b, h, row, col; 0 = broadcast). mask_future masks col > row.
 * (reference src/softmax_kernel.cu:35-224) */
int mt_attn_softmax_fw(float* out, const float* inp, const float* mask, int64_t B, int64_t nh,
                       int64_t from_len, int64_t to_len, const int64_t* mask_strides,
                       int mask_future, void* stream);
/* dinp = soft * (dout - rowsum(dout * soft)); dinp may alias dout. (:308-341) */
int mt_attn_softmax_bw(float* dinp, const float* dout, const float* soft, int64_t rows,
                       int64_t softmax_len, void* stream);
/* LayerNorm over the last dim of [rows, hidden]; var is stored with +1e-8.
 * (reference src/layernorm_kernel.cu:36-98) */
/* Softmax cross-entropy over rows of [rows, classes] fp32 logits (contiguous rows), the
 * reference's softmax_loss (minitorch/nn.py: logsumexp(logits) - logits[target]) in one pass:
 * loss[r] = lse[r] - logits[r, target[r]], lse[r] = log Σ_j exp(logits[r, j]); target holds
 * class ids as floats (minitorch's storage type; truncated toward zero). A target outside
 * [0, classes) picks nothing: loss[r] = lse[r] and the backward subtracts no one-hot. Backward:
 * dlogits[r, j] = dloss[r] (exp(logits[r, j] - lse[r]) - [j == target[r]]).
 * -inf logits are allowed (a mask on banned classes) and weigh zero: they add nothing to lse and
 * their dlogits are 0, whichever kernel the class count and alignment select. A row of only
 * -inf, or one holding +inf or NaN, is unspecified. */
int mt_softmax_xent_fw(float* loss, float* lse, const float* logits, const float* target, int64_t rows,
                       int64_t classes, void* stream);
int mt_softmax_xent_bw(float* dlogits, const float* dloss, const float* logits, const float* target,
                       const float* lse, int64_t rows, int64_t classes, void* stream);
int mt_layernorm_fw(float* ln_res, float* var, float* mean, const float* inp, const float* gamma,
                    const float* beta, int64_t rows, int64_t hidden, void* stream);
int64_t mt_layernorm_bw_workspace_bytes(int64_t rows, int64_t hidden);
/* (reference src/layernorm_kernel.cu:192-368) */
int mt_layernorm_bw(float* gamma_grad, float* beta_grad, float* inp_grad, const float* out_grad,
                    const float* inp, const float* gamma, const float* beta, const float* var,
                    const float* mean, int64_t rows, int64_t hidden, void* workspace,
                    void* stream);

/* ---- generic strided tensor ops, device pointers (fp32) ------------------- */
/* fn ids as the reference's combine.cu:12-29 (1 add, 2 mul, 3 id, 4 neg, 5 lt, 6 eq,
 * 7 sigmoid, 8 relu, 9 relu_back, 10 log, 11 log_back, 12 exp, 13 inv, 14 inv_back,
 * 15 is_close, 16 max, 17 pow, 18 tanh). Shapes broadcast right-aligned; rank <= 8. */
int mt_tensor_map(int fn, float* out, const int64_t* out_shape, const int64_t* out_strides,
                  int out_dims, const float* in, const int64_t* in_shape,
                  const int64_t* in_strides, int in_dims, void* stream);
int mt_tensor_zip(int fn, float* out, const int64_t* out_shape, const int64_t* out_strides,
                  int out_dims, const float* a, const int64_t* a_shape, const int64_t* a_strides,
                  int a_dims, const float* b, const int64_t* b_shape, const int64_t* b_strides,
                  int b_dims, void* stream);
/* out has a's shape with shape[reduce_dim] = 1; out = fn(start, fn-fold of the axis): `start`
 * enters exactly once per output element, whatever kernel the shape selects. The fold's
 * association is fixed for a given shape and layout (a repeated call is bitwise equal) but
 * differs between shapes. ±inf follow IEEE in add and mul folds and compare as usual in a max
 * fold. The result of a max reduction (fn 16, `x > y ? x : y`) over an axis that holds a NaN is
 * unspecified: that select is not associative under NaN, so the value depends on the fold order. */
int mt_tensor_reduce(int fn, float* out, const int64_t* out_shape, const int64_t* out_strides,
                     const float* a, const int64_t* a_shape, const int64_t* a_strides, int dims,
                     int reduce_dim, float start, void* stream);
/* c[b] = a[b] @ b[b]; strides are (batch, row, col) triples, batch stride 0 broadcasts.
 * (reference combine.cu:148-210 MatrixMultiply; cuda_kernel_ops.py:340-437). Plain layouts
 * (a unit stride in one dim of each operand) run on rocBLAS sgemm_strided_batched, others
 * on the library's own fp32 MFMA kernel. */
int mt_matmul_f32(float* c, const float* a, const float* b, int64_t batch, int64_t M, int64_t N,
                  int64_t K, const int64_t* a_strides, const int64_t* b_strides,
                  const int64_t* c_strides, void* stream);
/* 0 (default): rocBLAS for plain layouts; 1: the library's own fp32-MFMA GEMM kernel only;
 * 2: the library's own fp32-accurate GEMM on the bf16 MFMA (three bf16 pieces per operand:
 * 128x128 tiles where they fill the chip, else 64x64 with split-K); 3: that GEMM on 64x64
 * tiles only (A/B). The environment variable MT_GEMM_BACKEND sets the initial value.
 * Every backend propagates ±inf and NaN operands as an IEEE fp32 product does (backends 2 and
 * 3 stage a non-finite value as its own piece; inf times a finite |b| < 2^-126 is NaN there). */
void mt_set_gemm_backend(int backend);
/* The kernel mt_matmul_f32 launches for this problem under `backend` (0..3 as above), decided by
 * the function mt_matmul_f32 itself dispatches through: 0 rocBLAS, 1 rocBLAS on the library's
 * own K slices plus an ordered sum, 2 the fp32-MFMA kernel, 3 the three-piece bf16 GEMM on
 * 64x64 tiles, 4 the same on 128x128 tiles; negative for bad arguments (mt_last_error).
 * out (may be NULL) = {ak, bk, vec, S, ks}: S k-slices of ks each (S = 1: no split); kernels
 * 3 and 4: ak / bk = the operand is read along k, vec = 16-byte loads; rocBLAS: ak / bk = op N
 * on A / B, vec = -1; kernel 2: ak = bk = vec = -1. a, b and c are used for their alignment
 * only, never dereferenced. No device call: the intended plan; a split whose scratch cannot be
 * allocated at run time still runs unsplit (the 128x128 one as the 64x64 plan). */
int mt_matmul_f32_plan(int backend, int64_t batch, int64_t M, int64_t N, int64_t K,
                       const int64_t* a_strides, const int64_t* b_strides, const int64_t* c_strides,
                       const void* a, const void* b, const void* c, int32_t out[5]);

/* out[0..n) <- U[0,1) from a stateless counter-based hash of (seed, index). Replaces the
 * host draws of the reference's dropout paths (minitorch/nn.py dropout via
 * tensor_functions.rand, modules_basic.py Dropout via np.random.binomial), which build and
 * copy a host mask per call. */
int mt_rand_uniform(float* out, int64_t n, uint64_t seed, void* stream);

/* Fused feed-forward pieces (reference minitorch/modules_transfomer.py FeedForward:
 * dropout(linear_out(GELU(linear_in(x))))), fp32, x/dy/out rows of `cols` contiguous floats:
 *   mt_bias_gelu_fw: out = GELU_tanh(x + bias[col])             (linear_in's bias + GELU)
 *   mt_bias_gelu_bw: dx  = dy * GELU_tanh'(x + bias[col])         (dbias = column sums of dx)
 *   mt_dropout:      out = u_i > p ? x * scale : 0, u_i the mt_rand_uniform draw of
 *                    (seed, i), so a backward with the same seed applies the same mask. */
int mt_bias_gelu_fw(float* out, const float* x, const float* bias, int64_t rows, int64_t cols, void* stream);
int mt_bias_gelu_bw(float* dx, const float* dy, const float* x, const float* bias, int64_t rows, int64_t cols,
                    void* stream);
int mt_dropout(float* out, const float* x, int64_t n, float p, float scale, uint64_t seed, void* stream);
/* mt_dropout with the seed read from device memory when the kernel runs (a hipGraph-captured
 * training step writes a fresh seed there before each replay: minitorch/graphs.py) */
int mt_dropout_dseed(float* out, const float* x, int64_t n, float p, float scale, const uint64_t* seed,
                     void* stream);

/* Embedding rows (reference minitorch/modules_basic.py Embedding.forward: one_hot(ids, V) @ W),
 * fp32, ids[ntok] the float token ids, W [V x E] and out / dout [ntok x E] contiguous:
 * A float id f names row trunc(f) iff f >= 0 and trunc(f) < V (-0.0 and 0.9 name row 0); every
 * other value (negative, >= V however large, +-inf, NaN) names none and never indexes memory.
 *   mt_embedding_fw: out[t] = W[ids[t]]            (a row of +0.0 for an id that names none)
 *   mt_embedding_bw: dW[v]  = sum over t with ids[t] == v of dout[t] in a fixed order
 *                    (deterministic); every row of dW is written (zero for ids that do not occur) */
int mt_embedding_fw(float* out, const float* ids, const float* weight, int64_t ntok, int64_t V, int64_t E,
                    void* stream);
int mt_embedding_bw(float* dweight, const float* dout, const float* ids, int64_t ntok, int64_t V, int64_t E,
                    void* stream);

/* Multi-tensor Adam step over n_tensors dense fp32 device tensors (parameters, their
 * gradients, first and second moments, numels[t] elements each), in place:
 *   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= step_size m / (sqrt(v) + eps)
 * step_size = lr sqrt(1 - b2^t) / (1 - b1^t) (host-computed bias correction); b1, b2,
 * 1 - b1, 1 - b2, eps and step_size are each rounded to fp32 once; the update divides by
 * (powf(v, 0.5) + eps) through its reciprocal, as the tensor ops do (bit-identical). Replaces the
 * reference's per-parameter tensor-op Adam (minitorch/optim.py:52-75), one launch per 24
 * tensors. A tensor of 0 elements is skipped and its pointers are not looked at; a NULL pointer
 * of a tensor with elements is an error (tensors of earlier launches are already updated). */
int mt_adam_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                 float* const* exp_avg_sq, const int64_t* numels, double beta1, double beta2, double eps,
                 double step_size, void* stream);
/* mt_adam_step with step_size read (as one fp32) from device memory when the kernel runs: the
 * hipGraph-captured step's per-replay bias correction (minitorch/graphs.py) */
int mt_adam_step_dstep(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                       float* const* exp_avg_sq, const int64_t* numels, double beta1, double beta2, double eps,
                       const float* step_size, void* stream);

/* ---- reference-compatible host-pointer wrappers (companion + combine) ----- */
/* reference src/softmax_kernel.cu:233 (stream: hipStream_t) */
void launch_attn_softmax(float* inp, const float* attn_mask, int batch_size, int nhead,
                         int from_len, int to_len, bool mask_future, void* stream);
/* reference src/softmax_kernel.cu:345 */
void launch_attn_softmax_bw(float* out_grad, const float* soft_inp, int rows, int softmax_len,
                            void* stream);
/* reference src/layernorm_kernel.cu:101 */
void launch_layernorm(float* ln_res, float* vars, float* means, const float* inp,
                      const float* scale, const float* bias, int batch_size, int hidden_dim,
                      void* stream);
/* reference src/layernorm_kernel.cu:370 */
void launch_layernorm_bw(float* gamma_grad, float* betta_grad, float* inp_grad,
                         const float* out_grad, const float* inp, const float* gamma,
                         const float* betta, const float* vars, const float* means,
                         int batch_size, int hidden_dim, void* stream_1, void* stream_2);
/* reference src/combine.cu:385 */
void tensorMap(float* out, int* out_shape, int* out_strides, int out_size, float* in_storage,
               int* in_shape, int* in_strides, int in_size, int shape_size, int fn_id);
/* reference src/combine.cu:443 */
void tensorZip(float* out, int* out_shape, int* out_strides, int out_size, int out_shape_size,
               float* a_storage, int* a_shape, int* a_strides, int a_size, int a_shape_size,
               float* b_storage, int* b_shape, int* b_strides, int b_size, int b_shape_size,
               int fn_id);
/* reference src/combine.cu:523 */
void tensorReduce(float* out, int* out_shape, int* out_strides, int out_size, float* a_storage,
                  int* a_shape, int* a_strides, int reduce_dim, float reduce_value,
                  int shape_size, int fn_id);
/* reference src/combine.cu:315 */
void MatrixMultiply(float* out, int* out_shape, int* out_strides, float* a_storage, int* a_shape,
                    int* a_strides, float* b_storage, int* b_shape, int* b_strides, int batch,
                    int m, int p);

#ifdef __cplusplus
}
#endif
#endif /* MINITORCH_HIP_H */
