// Speculative decoding without a second model (include/minitorch_hip.h): mt_spec_draft proposes
// up to k tokens per row by prompt lookup, mt_spec_accept verifies them against the tokens the
// non-speculative path would have chosen and does the per-row bookkeeping, all on the device, so
// that a whole speculative step can be captured in a hipGraph.
//
// spec_draft_kernel: one workgroup of 256 threads per row. For g = min(max_ngram, L - 1) down to
//   1 (a workgroup-uniform loop) every thread tests the candidate starts s = tid, tid + 256, ..
//   of an earlier occurrence of the row's last g tokens and keeps the largest that matches; the
//   maximum over the workgroup is taken by shuffles and one LDS round. Thread 0 then writes the
//   fed tokens: the last token and the continuation of the match, extended into itself.
// mt_spec_accept is two launches: select_token.hip's kernel over the B (k + 1) logits rows (one
//   workgroup each, the id written to the caller's scratch), then spec_accept_kernel, one thread
//   per batch row, which compares, writes the emitted tokens and advances the counters.
// Stores are plain vector stores; nothing is allocated and nothing synchronises.
#include "../../include/minitorch_hip.h"
#include "fa_common.h"
#include "select_token.h"
#include <math.h>

namespace mt {
int set_error(const char* fmt, ...);           // capi_flash.hip
int check_hip(hipError_t e, const char* where);

constexpr int kDraftThreads = 256;
constexpr int kSpecMaxK = 7;      // k + 1 <= 8: the decode kernel's query rows
constexpr int kSpecMaxNgram = 8;

struct DraftArgs {
  const int32_t* tokens;
  int64_t token_stride;
  int S, k, max_ngram;
  const int32_t* held;
  float* feed_f32;
  int32_t* feed_i32;
  int32_t* n_draft;
};

__global__ __launch_bounds__(kDraftThreads) void spec_draft_kernel(const DraftArgs a) {
  __shared__ int best_w[kDraftThreads / 64];
  __shared__ int32_t feed[kSpecMaxK + 1];  // thread 0's: indexed by a run-time value (LDS, not scratch)
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t* row = a.tokens + (int64_t)b * a.token_stride;
  const int L = min(max(a.held[b], 1), a.S);
  int32_t tail[kSpecMaxNgram];  // the last tokens, tail[j] = row[L - 1 - j]
#pragma unroll
  for (int j = 0; j < kSpecMaxNgram; ++j) tail[j] = j < L ? row[L - 1 - j] : 0;

  int g = min(a.max_ngram, L - 1), s_best = -1;
  for (; g >= 1; --g) {  // g and the exit are workgroup-uniform
    int mine = -1;
    for (int s = tid; s <= L - g - 1; s += kDraftThreads) {
      bool eq = true;
#pragma unroll
      for (int j = 0; j < kSpecMaxNgram; ++j)  // row[s + g - 1 - j] against row[L - 1 - j]
        if (j < g) eq = eq && row[s + g - 1 - j] == tail[j];
      mine = eq ? s : mine;  // s grows: the last match is this thread's largest
    }
    for (int o = 32; o > 0; o >>= 1) mine = max(mine, __shfl_xor(mine, o, 64));
    __syncthreads();  // the previous round's reads of best_w
    if (lane == 0) best_w[wave] = mine;
    __syncthreads();
    s_best = max(max(best_w[0], best_w[1]), max(best_w[2], best_w[3]));
    if (s_best >= 0) break;
  }
  if (tid != 0) return;
  const int n = a.k + 1;
  feed[0] = tail[0];
  for (int i = 0; i < a.k; ++i) {
    // ext = tokens[:L] followed by the drafts made so far; s + g <= L - 1, so p - L < i
    const int p = s_best + g + i;
    feed[1 + i] = s_best < 0 ? feed[0] : (p < L ? row[p] : feed[1 + p - L]);
  }
  for (int i = 0; i < n; ++i) {
    if (a.feed_f32) a.feed_f32[(int64_t)b * n + i] = (float)feed[i];
    if (a.feed_i32) a.feed_i32[(int64_t)b * n + i] = feed[i];
  }
  a.n_draft[b] = s_best < 0 ? 0 : a.k;
}

struct AcceptArgs {
  int B, k, S;
  const int32_t* chosen;  // [B, k + 1]
  const int32_t* feed;    // [B, k + 1]
  const int32_t* n_draft;
  const int32_t* limit;
  int64_t eos_id;
  int32_t *count, *held, *cache_len, *done, *drafted, *accepted, *steps;
  int32_t* tokens;
  int64_t token_stride;
  int32_t* history;
  int64_t history_stride;
};

__global__ __launch_bounds__(64) void spec_accept_kernel(const AcceptArgs p) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= p.B || p.done[b]) return;
  const int n = p.k + 1;
  const int32_t* c = p.chosen + (int64_t)b * n;
  const int32_t* feed = p.feed + (int64_t)b * n;
  const int nd = min(max(p.n_draft[b], 0), p.k);
  const int cnt = p.count[b], h = p.held[b];
  int a = 0;
  while (a < nd && feed[1 + a] == c[a]) ++a;
  const int e = min(a + 1, p.limit[b] - cnt);
  int w = 0;
  bool eos = false;
  while (w < e && !eos) {
    const int id = c[w];
    const int64_t hs = (int64_t)cnt + w, ts = (int64_t)h + w;  // a slot outside the row is dropped
    if (hs >= 0 && hs < p.history_stride) p.history[(int64_t)b * p.history_stride + hs] = id;
    if (ts >= 0 && ts < p.S) p.tokens[(int64_t)b * p.token_stride + ts] = id;
    eos = p.eos_id >= 0 && (int64_t)id == p.eos_id;
    ++w;
  }
  p.count[b] = cnt + w;
  p.held[b] = h + w;
  if (p.cache_len) p.cache_len[b] += w;
  if (eos || cnt + w >= p.limit[b]) p.done[b] |= 1;
  if (p.drafted) p.drafted[b] += nd;
  if (p.accepted) p.accepted[b] += max(min(a, w - 1), 0);
  if (p.steps) p.steps[b] += 1;
}
}  // namespace mt

using namespace mt;

static int check_k(const char* who, int64_t k) {
  if (k < 1 || k > kSpecMaxK)
    return set_error("%s: k=%lld is outside 1..%d (a decode step takes k + 1 <= 8 tokens)", who, (long long)k, kSpecMaxK);
  return 0;
}

extern "C" int mt_spec_draft(const int32_t* tokens, int64_t B, int64_t S, int64_t token_stride,
                             const int32_t* held, int64_t k, int64_t max_ngram, float* feed_f32,
                             int32_t* feed_i32, int32_t* n_draft, void* stream) {
  if (check_k("mt_spec_draft", k)) return 1;
  if (max_ngram < 1 || max_ngram > kSpecMaxNgram)
    return set_error("mt_spec_draft: max_ngram=%lld is outside 1..%d", (long long)max_ngram, kSpecMaxNgram);
  if (B <= 0 || S <= 0) return set_error("mt_spec_draft: bad sizes B=%lld S=%lld", (long long)B, (long long)S);
  if (B > (1ll << 31) - 1 || S > (1ll << 31) - 1)
    return set_error("mt_spec_draft: B=%lld S=%lld out of range", (long long)B, (long long)S);
  if (S < k + 2) return set_error("mt_spec_draft: S=%lld is below k + 2 = %lld", (long long)S, (long long)(k + 2));
  if (token_stride < S)
    return set_error("mt_spec_draft: token_stride %lld is below S=%lld", (long long)token_stride, (long long)S);
  if (!tokens) return set_error("mt_spec_draft: tokens is NULL");
  if (!held) return set_error("mt_spec_draft: held is NULL");
  if (!n_draft) return set_error("mt_spec_draft: n_draft is NULL");
  if (!feed_f32 && !feed_i32) return set_error("mt_spec_draft: both outputs (feed_f32, feed_i32) are NULL");
  DraftArgs a;
  a.tokens = tokens; a.token_stride = token_stride; a.S = (int)S; a.k = (int)k; a.max_ngram = (int)max_ngram;
  a.held = held; a.feed_f32 = feed_f32; a.feed_i32 = feed_i32; a.n_draft = n_draft;
  spec_draft_kernel<<<dim3((unsigned)B), dim3(kDraftThreads), 0, (hipStream_t)stream>>>(a);
  return check_hip(hipGetLastError(), "mt_spec_draft");
}

static int spec_accept_impl(const char* who, const float* logits, int64_t B, int64_t k, int64_t V, int64_t batch_stride,
                            int64_t row_stride, const int32_t* feed_i32, const int32_t* n_draft, float temperature,
                            int64_t top_k, float top_p, float min_p, uint64_t seed, const uint64_t* seed_dev,
                            int64_t eos_id, const int32_t* limit, int32_t* count, int32_t* held,
                            int32_t* cache_len, int32_t* done, int32_t* drafted, int32_t* accepted,
                            int32_t* steps, int32_t* tokens, int64_t S, int64_t token_stride,
                            int32_t* history, int64_t history_stride, int32_t* scratch, void* stream) {
  if (check_k(who, k)) return 1;
  if (B <= 0 || V <= 0 || S <= 0)
    return set_error("%s: bad sizes B=%lld V=%lld S=%lld", who, (long long)B, (long long)V, (long long)S);
  if (V > kSelMaxV)
    return set_error("%s: V=%lld is above the limit of %d (the row is held in LDS)", who, (long long)V, kSelMaxV);
  if (B > ((1ll << 31) - 1) / (k + 1) || S > (1ll << 31) - 1)
    return set_error("%s: B=%lld S=%lld out of range", who, (long long)B, (long long)S);
  if (S < k + 2) return set_error("%s: S=%lld is below k + 2 = %lld", who, (long long)S, (long long)(k + 2));
  if (row_stride < V)
    return set_error("%s: row_stride %lld is below V=%lld", who, (long long)row_stride, (long long)V);
  if (batch_stride < k * row_stride + V)
    return set_error("%s: batch_stride %lld is below the k + 1 = %lld rows of a batch row", who,
                     (long long)batch_stride, (long long)(k + 1));
  if (token_stride < S)
    return set_error("%s: token_stride %lld is below S=%lld", who, (long long)token_stride, (long long)S);
  if (history_stride <= 0)
    return set_error("%s: history_stride %lld must be positive", who, (long long)history_stride);
  if (!(temperature >= 0.f)) return set_error("%s: temperature must be >= 0 (got %g)", who, (double)temperature);
  if (!logits) return set_error("%s: logits is NULL", who);
  if ((uintptr_t)logits & 3) return set_error("%s: logits is not 4-B aligned", who);
  const struct { const void* p; const char* name; } need[] = {
      {feed_i32, "feed_i32"}, {n_draft, "n_draft"}, {limit, "limit"}, {count, "count"}, {held, "held"},
      {done, "done"}, {tokens, "tokens"}, {history, "history"}, {scratch, "scratch"}};
  for (const auto& q : need)
    if (!q.p) return set_error("%s: %s is NULL", who, q.name);
  if (check_nucleus(who, top_p, min_p)) return 1;
  SelectArgs s;
  s.logits = logits; s.row_stride = row_stride; s.V = (int)V;
  s.top_k = (int)(top_k <= 0 || top_k >= V ? 0 : top_k);
  s.temperature = temperature; s.seed = seed; s.seed_dev = seed_dev; s.eos_id = -1;
  s.next_f32 = nullptr; s.next_i32 = nullptr; s.done = nullptr;
  s.history = nullptr; s.history_stride = 0; s.step_dev = nullptr;
  s.rows = (int)(k + 1); s.batch_stride = batch_stride; s.count = count; s.skip = done; s.scratch = scratch;
  s.top_p = top_p; s.min_p = min_p;
  if (check_hip(launch_select(s, B, (hipStream_t)stream), who)) return 1;
  AcceptArgs a;
  a.B = (int)B; a.k = (int)k; a.S = (int)S; a.chosen = scratch; a.feed = feed_i32; a.n_draft = n_draft;
  a.limit = limit; a.eos_id = eos_id; a.count = count; a.held = held; a.cache_len = cache_len; a.done = done;
  a.drafted = drafted; a.accepted = accepted; a.steps = steps; a.tokens = tokens; a.token_stride = token_stride;
  a.history = history; a.history_stride = history_stride;
  spec_accept_kernel<<<dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream>>>(a);
  return check_hip(hipGetLastError(), who);
}

extern "C" int mt_spec_accept(const float* logits, int64_t B, int64_t k, int64_t V, int64_t batch_stride,
                              int64_t row_stride, const int32_t* feed_i32, const int32_t* n_draft,
                              float temperature, int64_t top_k, uint64_t seed, const uint64_t* seed_dev,
                              int64_t eos_id, const int32_t* limit, int32_t* count, int32_t* held,
                              int32_t* cache_len, int32_t* done, int32_t* drafted, int32_t* accepted,
                              int32_t* steps, int32_t* tokens, int64_t S, int64_t token_stride,
                              int32_t* history, int64_t history_stride, int32_t* scratch, void* stream) {
  return spec_accept_impl("mt_spec_accept", logits, B, k, V, batch_stride, row_stride, feed_i32, n_draft, temperature,
                          top_k, 1.f, 0.f, seed, seed_dev, eos_id, limit, count, held, cache_len, done, drafted,
                          accepted, steps, tokens, S, token_stride, history, history_stride, scratch, stream);
}

extern "C" int mt_spec_accept_p(const float* logits, int64_t B, int64_t k, int64_t V, int64_t batch_stride,
                                int64_t row_stride, const int32_t* feed_i32, const int32_t* n_draft,
                                float temperature, int64_t top_k, float top_p, float min_p, uint64_t seed,
                                const uint64_t* seed_dev, int64_t eos_id, const int32_t* limit, int32_t* count,
                                int32_t* held, int32_t* cache_len, int32_t* done, int32_t* drafted,
                                int32_t* accepted, int32_t* steps, int32_t* tokens, int64_t S,
                                int64_t token_stride, int32_t* history, int64_t history_stride, int32_t* scratch,
                                void* stream) {
  return spec_accept_impl("mt_spec_accept_p", logits, B, k, V, batch_stride, row_stride, feed_i32, n_draft,
                          temperature, top_k, top_p, min_p, seed, seed_dev, eos_id, limit, count, held, cache_len,
                          done, drafted, accepted, steps, tokens, S, token_stride, history, history_stride, scratch,
                          stream);
}
