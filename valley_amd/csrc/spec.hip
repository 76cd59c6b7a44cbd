// libvalley_hip_spec.so (include/valley_hip_spec.h): prompt-lookup speculative decoding on gfx950 — the split attention of the
// verify step's k + 1 queries, the draft lookup and the acceptance.  The attention kernel lives in spec_attn.inc and the draft and
// acceptance rules in spec_lookup.inc, both shared with spec_rows.hip: the kernels here say where the ONE sequence's tables and
// position are.
//
// The attention is decode_split_kernel's idea (attention.hip) for a few queries of ONE sequence: a head's keys are streamed
// once, by four workgroups, for all S queries.  What differs is the key partition.  decode_split_kernel cuts [0, kv_len) into
// four contiguous quarters, so the summation order of a query depends on kv_len; here the cut is fixed — 64-key blocks, block
// c to split c mod 4, ascending — and a query joins a block only if the block starts at or before its own position.  The
// arithmetic of the query at position P is then a function of P alone (not of S, not of its index in the launch): the
// position invariance the header states, which makes a speculative generation independent of what was drafted.
//
// Compute form: VALU dot products, not the 16x16x32 MFMA.  With S <= 8 query rows padded to 16 the matrix core would run at
// most half empty, and the launch is bound by the K / V stream (2 x kv_len x 256 B per head), not by arithmetic: per 64-key
// block a thread issues 32 S fmas for the scores and 32 S for P.V against 8 16-byte loads.  The VALU form also keeps every
// sum a fixed chain of fmas (low element first, as vly_dot8), which is what the bit-for-bit contract needs.
//
// One build serves both 16-bit storage types (DT = 0: bf16, 1: IEEE fp16), as wq.hip does.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "common.hpp"
#include "companion_capi.hpp"
#include "../../include/valley_hip_spec.h"

namespace {

#include "spec_attn.inc"      // the attention kernel, shared with spec_rows.hip (ROWS = false here: one position per launch)
static_assert(SPLITS == VLY_SPEC_SPLITS && PART == VLY_SPEC_PARTIAL, "spec_attn.inc and valley_hip_spec.h disagree");
#include "spec_lookup.inc"    // the draft and acceptance rules of one sequence, shared with spec_rows.hip
static_assert(MAX_NGRAM == VLY_SPEC_MAX_NGRAM, "spec_lookup.inc and valley_hip_spec.h disagree");

// ---- vly_spec_draft ---------------------------------------------------------------------------------------------------------
// One workgroup of 1024 threads over the one sequence: lookup_draft with the length clamped into the history.
__global__ void __launch_bounds__(1024) spec_draft_kernel(const int32_t* __restrict__ hist, int ctx_max, const int32_t* __restrict__ len_dev,
                                                          int len_add, int k, int max_ngram, const int32_t* __restrict__ eos, int n_eos,
                                                          int vocab, int lookup, int32_t* __restrict__ draft, int32_t* __restrict__ draft_len,
                                                          int32_t* __restrict__ tok) {
    __shared__ int red[16];
    const int len = max(1, min((len_dev ? len_dev[0] : 0) + len_add, ctx_max));
    lookup_draft(hist, ctx_max, len, k, max_ngram, eos, n_eos, vocab, lookup, draft, draft_len, tok, red);
}

// ---- vly_spec_accept --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) spec_accept_kernel(const int32_t* __restrict__ am, const int32_t* __restrict__ draft,
                                                         const int32_t* __restrict__ draft_len, int k, int32_t* __restrict__ hist,
                                                         int ctx_max, int32_t* __restrict__ pos_dev, int32_t* __restrict__ emit,
                                                         int32_t* __restrict__ tok, int32_t* __restrict__ stats) {
    if (threadIdx.x != 0) return;
    lookup_accept(am, draft, draft_len, k, hist, ctx_max, pos_dev, emit, tok, stats);
}

template <int DT>
int launch_attn(int S, dim3 grid, hipStream_t st, const uint16_t* qkv, const uint16_t* kc, const uint16_t* vc, const uint8_t* key_valid,
                int kv_stride, uint16_t* out, int heads, int past, const int32_t* past_dev, int ctx_max, float* partials, unsigned* arrivals) {
#define VLY_SPEC_CASE(SV)                                                                                                         \
    case SV:                                                                                                                      \
        hipLaunchKernelGGL((spec_attn_kernel<SV, DT, false>), grid, dim3(256), 0, st, qkv, kc, vc, key_valid, kv_stride, out, heads, past, \
                           past_dev, ctx_max, partials, arrivals);                                                                \
        break;
    switch (S) {
        VLY_SPEC_CASE(1) VLY_SPEC_CASE(2) VLY_SPEC_CASE(3) VLY_SPEC_CASE(4) VLY_SPEC_CASE(5) VLY_SPEC_CASE(6) VLY_SPEC_CASE(7) VLY_SPEC_CASE(8)
    }
#undef VLY_SPEC_CASE
    return check_launch("vly_spec_attention");
}

}  // namespace

VLY_COMPANION_CAPI(spec, VLY_SPEC_ABI_VERSION)

extern "C" int vly_spec_attention(const void* qkv, const void* kcache, const void* vcache, const uint8_t* key_valid, int key_valid_stride,
                                  void* out, int B, int S, int heads, int past_len, const int32_t* past_len_dev, int ctx_max,
                                  float* partials, uint32_t* arrivals, int dtype, void* stream) {
    if (B <= 0 || S <= 0 || S > VLY_SPEC_MAX_QUERIES || heads <= 0 || past_len < 0 || (long)past_len + S > ctx_max || B > 65535 ||
        heads > 65535 || (dtype != 0 && dtype != 1) || !qkv || !kcache || !vcache || !out || !partials || !arrivals ||
        ((uintptr_t)qkv & 15) || ((uintptr_t)kcache & 15) || ((uintptr_t)vcache & 15) || ((uintptr_t)out & 7) || ((uintptr_t)partials & 3) ||
        ((uintptr_t)arrivals & 3)) {
        set_error("vly_spec_attention: bad args B=%d S=%d (1..%d) heads=%d past=%d ctx_max=%d dtype=%d (16-byte aligned qkv / caches, "
                  "partials and arrivals required)", B, S, VLY_SPEC_MAX_QUERIES, heads, past_len, ctx_max, dtype);
        return -22;
    }
    // (a device-side position can be anything up to ctx_max - S: the rows must span the cache, as vly_decode_attention_* requires)
    if (key_valid && key_valid_stride < (past_len_dev ? ctx_max : past_len + S)) {
        set_error("vly_spec_attention: key_valid_stride %d < %d (kv_len; ctx_max with a device-side position)", key_valid_stride,
                  past_len_dev ? ctx_max : past_len + S);
        return -22;
    }
    const dim3 grid(heads, B, SPLITS);
    if (dtype == 1)
        return launch_attn<1>(S, grid, (hipStream_t)stream, (const uint16_t*)qkv, (const uint16_t*)kcache, (const uint16_t*)vcache, key_valid,
                              key_valid_stride, (uint16_t*)out, heads, past_len, past_len_dev, ctx_max, partials, arrivals);
    return launch_attn<0>(S, grid, (hipStream_t)stream, (const uint16_t*)qkv, (const uint16_t*)kcache, (const uint16_t*)vcache, key_valid,
                          key_valid_stride, (uint16_t*)out, heads, past_len, past_len_dev, ctx_max, partials, arrivals);
}

extern "C" int vly_spec_draft(const int32_t* hist, int ctx_max, const int32_t* len_dev, int len_add, int k, int max_ngram, const int32_t* eos,
                              int n_eos, int vocab, int lookup, int32_t* draft, int32_t* draft_len, int32_t* tok, void* stream) {
    if (!hist || ctx_max <= 0 || k < 1 || k > VLY_SPEC_MAX_DRAFT || max_ngram < 1 || max_ngram > VLY_SPEC_MAX_NGRAM || n_eos < 0 ||
        (n_eos > 0 && !eos) || !draft || !draft_len || !tok || (!len_dev && len_add < 1)) {
        set_error("vly_spec_draft: bad args ctx_max=%d k=%d (1..%d) max_ngram=%d (1..%d) n_eos=%d len_add=%d (hist, draft, draft_len and tok "
                  "required; eos with n_eos > 0)", ctx_max, k, VLY_SPEC_MAX_DRAFT, max_ngram, VLY_SPEC_MAX_NGRAM, n_eos, len_add);
        return -22;
    }
    hipLaunchKernelGGL(spec_draft_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, hist, ctx_max, len_dev, len_add, k, max_ngram,
                       n_eos ? eos : nullptr, n_eos, vocab, lookup, draft, draft_len, tok);
    return check_launch("vly_spec_draft");
}

extern "C" int vly_spec_accept(const int32_t* am, const int32_t* draft, const int32_t* draft_len, int k, int32_t* hist, int ctx_max,
                               int32_t* pos_dev, int32_t* emit, int32_t* tok, int32_t* stats, void* stream) {
    if (!am || !draft || !draft_len || k < 1 || k > VLY_SPEC_MAX_DRAFT || !hist || ctx_max <= 0 || !pos_dev || !emit || !tok || !stats) {
        set_error("vly_spec_accept: bad args k=%d (1..%d) ctx_max=%d (every pointer required)", k, VLY_SPEC_MAX_DRAFT, ctx_max);
        return -22;
    }
    hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, am, draft, draft_len, k, hist, ctx_max, pos_dev, emit,
                       tok, stats);
    return check_launch("vly_spec_accept");
}
