// Shared between fa_decode.hip (kernels, launchers) and capi_decode.hip (the C ABI).
#pragma once
#include "fa_common.h"

namespace mt {

struct DecodeArgs {
  const void* q; const void* k; const void* v; void* o;
  float* m; float* l;          // [B*H*Nq] or NULL
  float* ws;                   // nsplit > 1: [B*H*Nq*nsplit][d] O, then [B*H*Nq*nsplit][2] (m in log2 units, l)
  const int* kv_len;           // [B] or NULL
  int64_t qs[3], ks[3], vs[3], os[3];
  int H, Nq, Nk, d, nsplit, span, causal, o_f32;
  int Hkv, gs, slices;         // kv heads (H % Hkv == 0); query heads and workgroups per group (decode_plan)
  int64_t rows;                // B * H * Nq
  float scale_log2;            // log2(e) / sqrt(d)
};

struct DecodePlan { int lpk, tile, span, nsplit, gs, slices; };

struct AppendArgs {
  const char* kn; const char* vn; char* kc; char* vc;
  const int* pos;
  int64_t kns[3], vns[3], kcs[3], vcs[3];  // element strides
  int64_t total;                           // B * H * Nq * chunks
  int H, Nq, Nmax, chunks, esize;
};

DecodePlan decode_plan(int esize, int64_t B, int64_t H, int64_t Hkv, int64_t Nq, int64_t Nk, int64_t d);
hipError_t launch_decode(const DecodeArgs& a, bool bf16_in, int64_t B, hipStream_t st);
hipError_t launch_kv_append(const AppendArgs& a, hipStream_t st);
int set_error(const char* fmt, ...);           // capi_flash.hip
int check_hip(hipError_t e, const char* where);

}  // namespace mt
