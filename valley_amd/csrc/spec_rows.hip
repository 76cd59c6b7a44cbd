// libvalley_hip_spec_rows.so (include/valley_hip_spec_rows.h): prompt-lookup speculative decoding for several sequences in one
// verify step on gfx950 — B sequences x (k + 1) rows, every sequence at its own device-side position.  The per-sequence twins of
// vly_rope_kv, vly_spec_attention, vly_spec_draft, vly_spec_accept and vly_spec_counters.
//
// What is new against the single-sequence kernels is only where a row's position comes from (pos_rows[b] + j) and what happens
// at the end of a sequence's cache: a row whose position lies behind it is DEAD — it stores nothing — where the single-sequence
// kernels move the whole step back by clamping the position to ctx_max - S.  The attention is spec.hip's kernel itself
// (spec_attn.inc, ROWS = true), the draft and the acceptance are spec.hip's rules themselves (spec_lookup.inc) on one sequence's
// row of every table, behind the test for an idle slot; the RoPE restates rope_kv_kernel (norm_elementwise.hip) on the dtype code, since a companion
// cannot link the main library: same loads, same rope_rot, same packing, and tests/test_spec_rows_gpu.py compares the bits.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "common.hpp"
#include "companion_capi.hpp"
#include "../../include/valley_hip_spec_rows.h"

namespace {

#include "spec_attn.inc"      // the attention kernel, shared with spec.hip (ROWS = true here: one position per sequence)
static_assert(SPLITS == VLY_SPEC_ROWS_SPLITS && PART == VLY_SPEC_ROWS_PARTIAL, "spec_attn.inc and valley_hip_spec_rows.h disagree");
#include "spec_lookup.inc"    // the draft and acceptance rules of one sequence, shared with spec.hip
static_assert(MAX_NGRAM == VLY_SPEC_ROWS_MAX_NGRAM, "spec_lookup.inc and valley_hip_spec_rows.h disagree");

VLY_DEVICE int row_pos(const int32_t* __restrict__ pos_rows, int b, int ctx_max) { return max(0, min(pos_rows[b], ctx_max - 1)); }

// ---- vly_spec_rows_rope_kv --------------------------------------------------------------------------------------------------
// rope_kv_kernel's layout: 8 lanes per (row, head), lane j rotates dims [8j, 8j + 8) against [64 + 8j, 64 + 8j + 8) with 16-byte
// accesses.  A dead row returns before it has formed a table or cache address.
template <int DT>
__global__ void __launch_bounds__(256) rows_rope_kv_kernel(uint16_t* __restrict__ qkv, uint16_t* __restrict__ kc, uint16_t* __restrict__ vc,
                                                           const float* __restrict__ cos_t, const float* __restrict__ sin_t, int B, int S,
                                                           int heads, const int32_t* __restrict__ pos_rows, int ctx_max) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long unit = t >> 3;                                      // (b*S + s)*heads + h
    if (unit >= (long)B * S * heads) return;
    const int j = (int)(t & 7);
    const int h = (int)(unit % heads);
    const long rs = unit / heads;
    const int s = (int)(rs % S), b = (int)(rs / S);
    const int Hq = heads * 128;
    const int pos = row_pos(pos_rows, b, ctx_max) + s;
    if (pos >= ctx_max) return;                                    // dead
    const float4 c0 = *(const float4*)(cos_t + (size_t)pos * 64 + 8 * j), c1 = *(const float4*)(cos_t + (size_t)pos * 64 + 8 * j + 4);
    const float4 s0 = *(const float4*)(sin_t + (size_t)pos * 64 + 8 * j), s1 = *(const float4*)(sin_t + (size_t)pos * 64 + 8 * j + 4);
    const float cs[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    const float sn[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    uint16_t* q = qkv + (size_t)rs * 3 * Hq + h * 128 + 8 * j;
    uint16_t* k = q + Hq;
    const uint16_t* v = q + 2 * Hq;
    const size_t co = (((size_t)b * heads + h) * ctx_max + pos) * 128 + 8 * j;
    auto rot = [&](const u32x4 lo, const u32x4 hi, u32x4& olo, u32x4& ohi) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float a0 = t_lo<DT>(lo[i]), a1 = t_hi<DT>(lo[i]);
            const float b0 = t_lo<DT>(hi[i]), b1 = t_hi<DT>(hi[i]);
            olo[i] = t_pack2<DT>(rope_rot(a0, b0, cs[2 * i], sn[2 * i], -1.f), rope_rot(a1, b1, cs[2 * i + 1], sn[2 * i + 1], -1.f));
            ohi[i] = t_pack2<DT>(rope_rot(b0, a0, cs[2 * i], sn[2 * i], 1.f), rope_rot(b1, a1, cs[2 * i + 1], sn[2 * i + 1], 1.f));
        }
    };
    u32x4 olo, ohi;
    rot(*(const u32x4*)q, *(const u32x4*)(q + 64), olo, ohi);
    *(u32x4*)q = olo;
    *(u32x4*)(q + 64) = ohi;
    rot(*(const u32x4*)k, *(const u32x4*)(k + 64), olo, ohi);
    *(u32x4*)(kc + co) = olo;
    *(u32x4*)(kc + co + 64) = ohi;
    *(u32x4*)(vc + co) = *(const u32x4*)v;
    *(u32x4*)(vc + co + 64) = *(const u32x4*)(v + 64);
}

// ---- vly_spec_rows_draft ----------------------------------------------------------------------------------------------------
// lookup_draft (spec_lookup.inc) with blockIdx.x = the sequence: 1024 threads over that sequence's row of every table.
__global__ void __launch_bounds__(1024) rows_draft_kernel(const int32_t* __restrict__ hist_all, int ctx_max, const int32_t* __restrict__ pos_rows,
                                                          int len_add, const uint8_t* __restrict__ live, int k, int max_ngram,
                                                          const int32_t* __restrict__ eos, int n_eos, int vocab, int lookup,
                                                          int32_t* __restrict__ draft_all, int32_t* __restrict__ draft_len,
                                                          int32_t* __restrict__ tok_all) {
    __shared__ int red[16];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int32_t* hist = hist_all + (size_t)b * ctx_max;
    int32_t* draft = draft_all + (size_t)b * k;
    int32_t* tok = tok_all + (size_t)b * (k + 1);
    if (live && !live[b]) {                                      // (uniform) an idle slot: nothing drafted, rows of token 0
        if (tid <= k) tok[tid] = 0;
        if (tid == 0) draft_len[b] = 0;
        return;
    }
    const int len = max(1, min(pos_rows[b] + len_add, ctx_max));
    lookup_draft(hist, ctx_max, len, k, max_ngram, eos, n_eos, vocab, lookup, draft, draft_len + b, tok, red);   // drafts sit on live rows only
}

// ---- vly_spec_rows_accept ---------------------------------------------------------------------------------------------------
// one thread per sequence (lookup_accept, spec_lookup.inc); every table row it writes is its own sequence's
__global__ void __launch_bounds__(64) rows_accept_kernel(const int32_t* __restrict__ am_all, const int32_t* __restrict__ draft_all,
                                                         const int32_t* __restrict__ draft_len, const uint8_t* __restrict__ live, int B, int k,
                                                         int32_t* __restrict__ hist_all, int ctx_max, int32_t* __restrict__ pos_rows,
                                                         int32_t* __restrict__ emit_all, int32_t* __restrict__ tok, int32_t* __restrict__ stats_all) {
    for (int b = threadIdx.x; b < B; b += 64) {
        int32_t* emit = emit_all + (size_t)b * (k + 2);
        if (live && !live[b]) {
            emit[0] = 0;
            continue;
        }
        lookup_accept(am_all + (size_t)b * (k + 1), draft_all + (size_t)b * k, draft_len + b, k, hist_all + (size_t)b * ctx_max, ctx_max,
                      pos_rows + b, emit, tok + (size_t)b * (k + 1), stats_all + (size_t)b * 3);
    }
}

// ---- vly_spec_rows_counters -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) rows_counters_kernel(const int32_t* __restrict__ pos_rows, int B, int k, int ctx_max,
                                                           int32_t* __restrict__ ctr) {
    for (int r = threadIdx.x; r < B * (k + 1); r += 64) {
        const int b = r / (k + 1), j = r - b * (k + 1);
        ctr[r] = row_pos(pos_rows, b, ctx_max) + j;
    }
}

template <int DT>
int launch_attn(int S, dim3 grid, hipStream_t st, const uint16_t* qkv, const uint16_t* kc, const uint16_t* vc, const uint8_t* key_valid,
                int kv_stride, uint16_t* out, int heads, const int32_t* pos_rows, int ctx_max, float* partials, unsigned* arrivals) {
#define VLY_SPEC_ROWS_CASE(SV)                                                                                                       \
    case SV:                                                                                                                         \
        hipLaunchKernelGGL((spec_attn_kernel<SV, DT, true>), grid, dim3(256), 0, st, qkv, kc, vc, key_valid, kv_stride, out, heads, 0, \
                           pos_rows, ctx_max, partials, arrivals);                                                                   \
        break;
    switch (S) {
        VLY_SPEC_ROWS_CASE(1) VLY_SPEC_ROWS_CASE(2) VLY_SPEC_ROWS_CASE(3) VLY_SPEC_ROWS_CASE(4) VLY_SPEC_ROWS_CASE(5) VLY_SPEC_ROWS_CASE(6)
        VLY_SPEC_ROWS_CASE(7) VLY_SPEC_ROWS_CASE(8)
    }
#undef VLY_SPEC_ROWS_CASE
    return check_launch("vly_spec_rows_attention");
}

bool bad_k(int k) { return k < 1 || k > VLY_SPEC_ROWS_MAX_DRAFT; }

}  // namespace

VLY_COMPANION_CAPI(spec_rows, VLY_SPEC_ROWS_ABI_VERSION)

extern "C" int vly_spec_rows_rope_kv(void* qkv, void* kcache, void* vcache, const float* cos_table, const float* sin_table, int B, int S,
                                     int heads, const int32_t* pos_rows, int ctx_max, int dtype, void* stream) {
    if (B <= 0 || S <= 0 || S > VLY_SPEC_ROWS_MAX_QUERIES || heads <= 0 || ctx_max <= 0 || (dtype != 0 && dtype != 1) || !qkv || !kcache ||
        !vcache || !cos_table || !sin_table || !pos_rows || ((uintptr_t)qkv & 15) || ((uintptr_t)kcache & 15) || ((uintptr_t)vcache & 15) ||
        ((uintptr_t)cos_table & 15) || ((uintptr_t)sin_table & 15) || ((uintptr_t)pos_rows & 3)) {
        set_error("vly_spec_rows_rope_kv: bad args B=%d S=%d (1..%d) heads=%d ctx_max=%d dtype=%d (16-byte aligned qkv, caches and tables, "
                  "pos_rows required)", B, S, VLY_SPEC_ROWS_MAX_QUERIES, heads, ctx_max, dtype);
        return -22;
    }
    const long units = (long)B * S * heads;
    const dim3 grid((unsigned)((units * 8 + 255) / 256));
    if (dtype == 1)
        hipLaunchKernelGGL(rows_rope_kv_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, (uint16_t*)qkv, (uint16_t*)kcache, (uint16_t*)vcache,
                           cos_table, sin_table, B, S, heads, pos_rows, ctx_max);
    else
        hipLaunchKernelGGL(rows_rope_kv_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, (uint16_t*)qkv, (uint16_t*)kcache, (uint16_t*)vcache,
                           cos_table, sin_table, B, S, heads, pos_rows, ctx_max);
    return check_launch("vly_spec_rows_rope_kv");
}

extern "C" int vly_spec_rows_attention(const void* qkv, const void* kcache, const void* vcache, const uint8_t* key_valid, int key_valid_stride,
                                       void* out, int B, int S, int heads, const int32_t* pos_rows, int ctx_max, float* partials,
                                       uint32_t* arrivals, int dtype, void* stream) {
    if (B <= 0 || S <= 0 || S > VLY_SPEC_ROWS_MAX_QUERIES || heads <= 0 || ctx_max <= 0 || B > 65535 || heads > 65535 ||
        (dtype != 0 && dtype != 1) || !qkv || !kcache || !vcache || !out || !pos_rows || !partials || !arrivals || ((uintptr_t)qkv & 15) ||
        ((uintptr_t)kcache & 15) || ((uintptr_t)vcache & 15) || ((uintptr_t)out & 7) || ((uintptr_t)pos_rows & 3) || ((uintptr_t)partials & 3) ||
        ((uintptr_t)arrivals & 3)) {
        set_error("vly_spec_rows_attention: bad args B=%d S=%d (1..%d) heads=%d ctx_max=%d dtype=%d (16-byte aligned qkv / caches, pos_rows, "
                  "partials and arrivals required)", B, S, VLY_SPEC_ROWS_MAX_QUERIES, heads, ctx_max, dtype);
        return -22;
    }
    if (key_valid && key_valid_stride < ctx_max) {               // a device-side position can be anything: the rows span the cache
        set_error("vly_spec_rows_attention: key_valid_stride %d < ctx_max %d", key_valid_stride, ctx_max);
        return -22;
    }
    const dim3 grid(heads, B, SPLITS);
    if (dtype == 1)
        return launch_attn<1>(S, grid, (hipStream_t)stream, (const uint16_t*)qkv, (const uint16_t*)kcache, (const uint16_t*)vcache, key_valid,
                              key_valid_stride, (uint16_t*)out, heads, pos_rows, ctx_max, partials, arrivals);
    return launch_attn<0>(S, grid, (hipStream_t)stream, (const uint16_t*)qkv, (const uint16_t*)kcache, (const uint16_t*)vcache, key_valid,
                          key_valid_stride, (uint16_t*)out, heads, pos_rows, ctx_max, partials, arrivals);
}

extern "C" int vly_spec_rows_draft(const int32_t* hist, int ctx_max, const int32_t* pos_rows, int len_add, const uint8_t* live, int B, int k,
                                   int max_ngram, const int32_t* eos, int n_eos, int vocab, int lookup, int32_t* draft, int32_t* draft_len,
                                   int32_t* tok, void* stream) {
    if (!hist || ctx_max <= 0 || !pos_rows || B <= 0 || B > 65535 || bad_k(k) || max_ngram < 1 || max_ngram > VLY_SPEC_ROWS_MAX_NGRAM ||
        n_eos < 0 || (n_eos > 0 && !eos) || !draft || !draft_len || !tok) {
        set_error("vly_spec_rows_draft: bad args ctx_max=%d B=%d k=%d (1..%d) max_ngram=%d (1..%d) n_eos=%d (hist, pos_rows, draft, draft_len "
                  "and tok required; eos with n_eos > 0)", ctx_max, B, k, VLY_SPEC_ROWS_MAX_DRAFT, max_ngram, VLY_SPEC_ROWS_MAX_NGRAM, n_eos);
        return -22;
    }
    hipLaunchKernelGGL(rows_draft_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, hist, ctx_max, pos_rows, len_add, live, k, max_ngram,
                       n_eos ? eos : nullptr, n_eos, vocab, lookup, draft, draft_len, tok);
    return check_launch("vly_spec_rows_draft");
}

extern "C" int vly_spec_rows_accept(const int32_t* am, const int32_t* draft, const int32_t* draft_len, const uint8_t* live, int B, int k,
                                    int32_t* hist, int ctx_max, int32_t* pos_rows, int32_t* emit, int32_t* tok, int32_t* stats, void* stream) {
    if (!am || !draft || !draft_len || B <= 0 || bad_k(k) || !hist || ctx_max <= 0 || !pos_rows || !emit || !tok || !stats) {
        set_error("vly_spec_rows_accept: bad args B=%d k=%d (1..%d) ctx_max=%d (every pointer but live required)", B, k,
                  VLY_SPEC_ROWS_MAX_DRAFT, ctx_max);
        return -22;
    }
    hipLaunchKernelGGL(rows_accept_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, am, draft, draft_len, live, B, k, hist, ctx_max, pos_rows,
                       emit, tok, stats);
    return check_launch("vly_spec_rows_accept");
}

extern "C" int vly_spec_rows_counters(const int32_t* pos_rows, int B, int k, int ctx_max, int32_t* ctr, void* stream) {
    if (!pos_rows || !ctr || B <= 0 || B > 65535 || bad_k(k) || ctx_max <= 0 || ((uintptr_t)pos_rows & 3) || ((uintptr_t)ctr & 3)) {
        set_error("vly_spec_rows_counters: bad args B=%d k=%d (1..%d) ctx_max=%d (pos_rows and ctr required, 4-byte aligned)", B, k,
                  VLY_SPEC_ROWS_MAX_DRAFT, ctx_max);
        return -22;
    }
    hipLaunchKernelGGL(rows_counters_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, pos_rows, B, k, ctx_max, ctr);
    return check_launch("vly_spec_rows_counters");
}
