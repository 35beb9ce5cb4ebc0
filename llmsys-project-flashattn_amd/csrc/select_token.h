// The arguments and the launch of select_token.hip's kernel, shared with spec_decode.hip
// (mt_spec_accept chooses k + 1 tokens per batch row with the same device code).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mt {

constexpr int kSelThreads = 256;
constexpr int kSelMaxV = 32768;  // the row in LDS: 128 KiB of the CU's 160

struct SelectArgs {
  const float* logits;
  int64_t row_stride;
  int V, top_k;
  float temperature;
  uint64_t seed;
  const uint64_t* seed_dev;
  int64_t eos_id;
  float* next_f32;
  int32_t* next_i32;
  int32_t* done;
  int32_t* history;
  int64_t history_stride;
  const int32_t* step_dev;
  // mt_spec_accept (spec_decode.hip): `rows` logits rows per batch row, batch_stride apart; row i
  // of batch row b draws with seed + count[b] + i and the uniform at index b, and its id goes to
  // scratch[b * rows + i] and nowhere else; a batch row with skip[b] != 0 is left alone.
  // mt_select_token: rows = 1, batch_stride = row_stride, the three pointers NULL.
  int rows;
  int64_t batch_stride;
  const int32_t* count;
  const int32_t* skip;
  int32_t* scratch;
  // mt_select_token_p / mt_spec_accept_p: the nucleus and min-p filters (1 and 0: off). Last, so
  // that the kernel without the phase reads what it read before they were added.
  float top_p, min_p;
};

// one workgroup per logits row: B * a.rows of them. A sampling launch with top_p < 1 or min_p > 0
// runs select_token_kernel<CAP, true> (the nucleus phase compiled in), every other one
// select_token_kernel<CAP, false>, whose instructions are those of the kernel before the phase.
hipError_t launch_select(const SelectArgs& a, int64_t B, hipStream_t st);
// the shared refusal of both _p entries: top_p outside (0, 1], min_p outside [0, 1], a NaN
int check_nucleus(const char* who, float top_p, float min_p);

}  // namespace mt
