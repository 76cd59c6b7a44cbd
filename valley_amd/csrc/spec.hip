// libvalley_hip_spec.so (include/valley_hip_spec.h): prompt-lookup speculative decoding on gfx950 — the split attention of the
// verify step's k + 1 queries, the draft lookup and the acceptance.
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

typedef __attribute__((ext_vector_type(2))) _Float16 sp_f16x2;
typedef __attribute__((ext_vector_type(2))) __bf16 sp_bf16x2;

template <int DT> VLY_DEVICE float t_h2f(uint16_t v) {
    if constexpr (DT == 1) return (float)__builtin_bit_cast(_Float16, v);
    else return __uint_as_float(((uint32_t)v) << 16);
}
template <int DT> VLY_DEVICE float t_lo(uint32_t w) {
    if constexpr (DT == 1) return (float)__builtin_bit_cast(sp_f16x2, w)[0];
    else return __uint_as_float(w << 16);
}
template <int DT> VLY_DEVICE float t_hi(uint32_t w) {
    if constexpr (DT == 1) return (float)__builtin_bit_cast(sp_f16x2, w)[1];
    else return __uint_as_float(w & 0xffff0000u);
}
template <int DT> VLY_DEVICE uint32_t t_pack2(float lo, float hi) {
    const vly_f32x2 v = {lo, hi};
    if constexpr (DT == 1) return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, sp_f16x2));
    else return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, sp_bf16x2));
}

constexpr float LOG2E = 1.4426950408889634f;
constexpr float NEG_BIG = -1.0e30f;
constexpr int SPLITS = VLY_SPEC_SPLITS;
constexpr int PART = VLY_SPEC_PARTIAL;

// x + x[lane ^ 1], then + [lane ^ 2]: the four lanes of a quad end with the same bits ((a0 + a1) + (a2 + a3), commutative adds)
VLY_DEVICE float quad_sum(float v) {
    v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0xb1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
    v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x4e, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
    return v;
}

// ---- vly_spec_attention -----------------------------------------------------------------------------------------------------
// grid (heads, B, SPLITS), 256 threads.  Per 64-key block: thread t holds a quarter (32 dims) of K row t >> 2 for the scores and
// 8 dims of V rows (t >> 4) + 16 u, u < 4, for P.V; the next block of the split is requested before the current one is used.
// Per query: running max m, sum l (replicated in every thread) and the thread's 8 x (its 4 keys) share of P.V; at the end the
// sixteen key groups are added in LDS in a fixed order and (m, l, o[128]) is published for the merge.
template <int S, int DT>
__global__ void __launch_bounds__(256) spec_attn_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ kc,
                                                        const uint16_t* __restrict__ vc, const uint8_t* __restrict__ key_valid,
                                                        int kv_stride, uint16_t* __restrict__ out, int heads, int past,
                                                        const int32_t* __restrict__ past_dev, int ctx_max,
                                                        float* __restrict__ partials, unsigned* __restrict__ arrivals) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float qs[S][128];
    __shared__ float sc[S][64];
    __shared__ float red[2][S][4];
    __shared__ __attribute__((aligned(16))) float acc_s[16][128];
    __shared__ int last_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x, b = blockIdx.y, sp = blockIdx.z;
    const int Hq = heads * 128;
    if (past_dev) past = max(0, min(past_dev[0], ctx_max - S));
    const int kv_len = past + S;                                 // <= ctx_max: every row index below is clamped to kv_len - 1
    const int nblk = (kv_len + 63) >> 6;
    const uint16_t* kbase = kc + ((size_t)b * heads + h) * ctx_max * 128;
    const uint16_t* vbase = vc + ((size_t)b * heads + h) * ctx_max * 128;
    const uint8_t* kvld = key_valid ? key_valid + (size_t)b * kv_stride : nullptr;

    for (int e = tid; e < S * 128; e += 256) {
        const int i = e >> 7, d = e & 127;
        qs[i][d] = t_h2f<DT>(qkv[((size_t)b * S + i) * 3 * Hq + h * 128 + d]) * (0.08838834764831845f * LOG2E);
    }

    const int kr = tid >> 2, qd = tid & 3;                       // score role: key row of the block, quarter of its dims
    const int kg = tid >> 4, dc = tid & 15;                      // P.V role: key group, 8-dim chunk
    u32x4 kk[4], vv[4], kn[4], vn[4];
    uint8_t kval = 1, kvaln = 1;
    auto request = [&](int c, u32x4 (&k4)[4], u32x4 (&v4)[4], uint8_t& valid) {
        const int jk = min(c * 64 + kr, kv_len - 1);
        const u32x4* kp = (const u32x4*)(kbase + (size_t)jk * 128 + 32 * qd);
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) k4[cc] = kp[cc];
        valid = kvld ? kvld[jk] : (uint8_t)1;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jv = min(c * 64 + kg + 16 * u, kv_len - 1);
            v4[u] = *(const u32x4*)(vbase + (size_t)jv * 128 + 8 * dc);
        }
    };
    if (sp < nblk) request(sp, kk, vv, kval);

    float m_run[S], l_run[S], o[S][8];
#pragma unroll
    for (int i = 0; i < S; ++i) {
        m_run[i] = NEG_BIG;
        l_run[i] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[i][e] = 0.f;
    }
    __syncthreads();

#pragma unroll 1
    for (int c = sp; c < nblk; c += SPLITS) {
        if (c + SPLITS < nblk) request(c + SPLITS, kn, vn, kvaln);
        const int c0 = c * 64, jk = c0 + kr;
        // rows from kv_len on (clamped loads of the newest row) count as zero: never 0 x stale data
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (c0 + kg + 16 * u >= kv_len) vv[u] = u32x4{0u, 0u, 0u, 0u};
        float s[S], alpha[S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
            s[i] = NEG_BIG;
            if (c0 <= past + i) {                                // (uniform) the block holds keys of this query's past
                float a = 0.f;
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    const f32x4 q0 = *(const f32x4*)(&qs[i][32 * qd + 8 * cc]), q1 = *(const f32x4*)(&qs[i][32 * qd + 8 * cc + 4]);
                    a = __builtin_fmaf(t_lo<DT>(kk[cc][0]), q0[0], a); a = __builtin_fmaf(t_hi<DT>(kk[cc][0]), q0[1], a);
                    a = __builtin_fmaf(t_lo<DT>(kk[cc][1]), q0[2], a); a = __builtin_fmaf(t_hi<DT>(kk[cc][1]), q0[3], a);
                    a = __builtin_fmaf(t_lo<DT>(kk[cc][2]), q1[0], a); a = __builtin_fmaf(t_hi<DT>(kk[cc][2]), q1[1], a);
                    a = __builtin_fmaf(t_lo<DT>(kk[cc][3]), q1[2], a); a = __builtin_fmaf(t_hi<DT>(kk[cc][3]), q1[3], a);
                }
                a = quad_sum(a);
                if (jk <= past + i && kval) s[i] = a;            // a select: a NaN score of a masked key is dropped
                const float mc = wave_max(s[i]);
                if (lane == 0) red[0][i][wave] = mc;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < S; ++i) {
            if (c0 <= past + i) {
                const float mc = fmaxf(fmaxf(red[0][i][0], red[0][i][1]), fmaxf(red[0][i][2], red[0][i][3]));
                const float m_new = fmaxf(m_run[i], mc);
                alpha[i] = __builtin_amdgcn_exp2f(m_run[i] - m_new);
                const float p = s[i] > 0.5f * NEG_BIG ? __builtin_amdgcn_exp2f(s[i] - m_new) : 0.f;   // masked keys never count
                m_run[i] = m_new;
                if (qd == 0) sc[i][kr] = p;
                const float lc = wave_sum(qd == 0 ? p : 0.f);
                if (lane == 0) red[1][i][wave] = lc;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < S; ++i) {
            if (c0 <= past + i) {
                const float lc = ((red[1][i][0] + red[1][i][1]) + red[1][i][2]) + red[1][i][3];
                l_run[i] = l_run[i] * alpha[i] + lc;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[i][e] *= alpha[i];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float pj = sc[i][kg + 16 * u];
                    o[i][0] = __builtin_fmaf(pj, t_lo<DT>(vv[u][0]), o[i][0]); o[i][1] = __builtin_fmaf(pj, t_hi<DT>(vv[u][0]), o[i][1]);
                    o[i][2] = __builtin_fmaf(pj, t_lo<DT>(vv[u][1]), o[i][2]); o[i][3] = __builtin_fmaf(pj, t_hi<DT>(vv[u][1]), o[i][3]);
                    o[i][4] = __builtin_fmaf(pj, t_lo<DT>(vv[u][2]), o[i][4]); o[i][5] = __builtin_fmaf(pj, t_hi<DT>(vv[u][2]), o[i][5]);
                    o[i][6] = __builtin_fmaf(pj, t_lo<DT>(vv[u][3]), o[i][6]); o[i][7] = __builtin_fmaf(pj, t_hi<DT>(vv[u][3]), o[i][7]);
                }
            }
        }
        // (no barrier here: the next block writes red[0] before its first barrier, sc / red[1] behind it, and every read of
        // them above lies before this thread's next arrival at that barrier)
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) { kk[cc] = kn[cc]; vv[cc] = vn[cc]; }
        kval = kvaln;
    }

    // ---- publish (m, l, o[128]) per query: write-through stores, as split_publish (attention.hip)
#pragma unroll
    for (int i = 0; i < S; ++i) {
        float* part = partials + ((((size_t)b * heads + h) * S + i) * SPLITS + sp) * PART;
        __syncthreads();                                         // acc_s: the previous query's sums have been read
#pragma unroll
        for (int e = 0; e < 8; ++e) acc_s[kg][8 * dc + e] = o[i][e];
        __syncthreads();
        if (tid < 128) {
            float t = 0.f;
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) t += acc_s[k2][tid];
            __hip_atomic_store(part + 4 + tid, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (tid < 132) {
            __hip_atomic_store(part + tid - 128, tid == 128 ? m_run[i] : tid == 129 ? l_run[i] : 0.f, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
    }

    // ---- the last of the head's four workgroups to get here merges (split_merge_if_last's ticket, in its fenced form): the
    // partials are drained and released before the ticket, acquired behind it; nobody waits for anybody
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned* ctr = arrivals + (size_t)b * heads + h;
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_s = t == SPLITS - 1;
        if (t == SPLITS - 1) {
            __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
    }
    __syncthreads();
    if (!last_s || tid >= 32 * S) return;
    // 32 lanes x 4 dims per query, split_merge_if_last's arithmetic in split order
    const int i = tid >> 5, ln = tid & 31;
    const float* hb = partials + (((size_t)b * heads + h) * S + i) * (SPLITS * PART);
    float ms[SPLITS], ls[SPLITS], os[SPLITS][4];
#pragma unroll
    for (int q = 0; q < SPLITS; ++q) {
        ms[q] = __hip_atomic_load(hb + q * PART, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ls[q] = __hip_atomic_load(hb + q * PART + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int r = 0; r < 4; ++r) os[q][r] = __hip_atomic_load(hb + q * PART + 4 + 4 * ln + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    float mx = ms[0];
#pragma unroll
    for (int q = 1; q < SPLITS; ++q) mx = fmaxf(mx, ms[q]);
    float L = 0.f, O[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < SPLITS; ++q) {
        const float w = exp2f(ms[q] - mx);
        L = __builtin_fmaf(ls[q], w, L);
#pragma unroll
        for (int r = 0; r < 4; ++r) O[r] = __builtin_fmaf(os[q][r], w, O[r]);
    }
    u32x2 pk;
    pk[0] = t_pack2<DT>(O[0] / L, O[1] / L);
    pk[1] = t_pack2<DT>(O[2] / L, O[3] / L);
    *(u32x2*)(out + ((size_t)b * S + i) * Hq + h * 128 + 4 * ln) = pk;
}

// ---- vly_spec_draft ---------------------------------------------------------------------------------------------------------
// One workgroup of 1024 threads.  For each n-gram size, largest first, thread t tests the window starts t, t + 1024, ... in
// ascending order and keeps its first hit; the earliest hit of the block is a minimum over the waves' minima (no atomics).
__global__ void __launch_bounds__(1024) spec_draft_kernel(const int32_t* __restrict__ hist, int ctx_max, const int32_t* __restrict__ len_dev,
                                                          int len_add, int k, int max_ngram, const int32_t* __restrict__ eos, int n_eos,
                                                          int vocab, int lookup, int32_t* __restrict__ draft, int32_t* __restrict__ draft_len,
                                                          int32_t* __restrict__ tok) {
    __shared__ int red[16];
    const int tid = threadIdx.x;
    const int len = max(1, min((len_dev ? len_dev[0] : 0) + len_add, ctx_max));
    const int last = hist[len - 1];
    const int cap = min(k, ctx_max - len);                       // the verify step's last real position stays inside the cache
    if (!lookup) {
        if (tid == 0) {
            const int dl = max(0, min(draft_len[0], cap));
            tok[0] = last;
            for (int i = 0; i < k; ++i) tok[1 + i] = i < dl ? draft[i] : last;
        }
        return;
    }
    int start = -1;                                              // first token of the continuation, -1: no match
    for (int n = min(max_ngram, len - 1); n >= 1; --n) {
        int tl[VLY_SPEC_MAX_NGRAM];
#pragma unroll
        for (int d = 0; d < VLY_SPEC_MAX_NGRAM; ++d) tl[d] = d < n ? hist[len - n + d] : 0;
        int best = INT_MAX;
        for (int i = tid; i < len - n; i += 1024) {              // i + n - 1 <= len - 2: columns from len on are never read
            bool m = true;
#pragma unroll
            for (int d = 0; d < VLY_SPEC_MAX_NGRAM; ++d)
                if (d < n) m = m && hist[i + d] == tl[d];
            if (m) {
                best = i;
                break;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) best = min(best, __shfl_xor(best, off, 64));
        __syncthreads();                                         // red: the previous size's minima have been read
        if ((tid & 63) == 0) red[tid >> 6] = best;
        __syncthreads();
        best = red[0];
#pragma unroll
        for (int w = 1; w < 16; ++w) best = min(best, red[w]);
        if (best != INT_MAX) {                                   // (uniform) the first size with a match decides
            start = best + n;
            break;
        }
    }
    if (tid != 0) return;
    int dl = 0;
    if (start >= 0) {
        dl = min(start + k, len) - start;
        for (int j = 0; j < dl; ++j) {                           // cropped in front of the first EOS (or unusable id)
            const int t = hist[start + j];
            bool stop = t < 0 || (vocab > 0 && t >= vocab);
            for (int e = 0; e < n_eos; ++e) stop = stop || t == eos[e];
            if (stop) {
                dl = j;
                break;
            }
        }
        dl = min(dl, cap);
    }
    dl = max(dl, 0);
    tok[0] = last;
    for (int j = 0; j < k; ++j) {
        const int t = j < dl ? hist[start + j] : last;
        draft[j] = t;
        tok[1 + j] = t;
    }
    draft_len[0] = dl;
}

// ---- vly_spec_accept --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) spec_accept_kernel(const int32_t* __restrict__ am, const int32_t* __restrict__ draft,
                                                         const int32_t* __restrict__ draft_len, int k, int32_t* __restrict__ hist,
                                                         int ctx_max, int32_t* __restrict__ pos_dev, int32_t* __restrict__ emit,
                                                         int32_t* __restrict__ tok, int32_t* __restrict__ stats) {
    if (threadIdx.x != 0) return;
    const int pos = pos_dev[0];
    // vly_spec_draft's clamp (len = pos + 1): the rows behind it were fed the last token, not the draft, and are not compared
    const long room = (long)ctx_max - ((long)pos + 1);
    const int dl = (int)max(0L, min((long)min(draft_len[0], k), room));
    int n = 0;
    while (n < dl && draft[n] == am[n]) ++n;
    emit[0] = n + 1;
    for (int j = 0; j <= k; ++j) emit[1 + j] = j <= n ? am[j] : -1;
    for (int j = 0; j <= n; ++j) {
        const long c = (long)pos + 1 + j;
        if (c >= 0 && c < ctx_max) hist[c] = am[j];
    }
    tok[0] = am[n];
    stats[0] += 1;
    stats[1] += dl;
    stats[2] += n;
    pos_dev[0] = pos + n + 1;
}

template <int DT>
int launch_attn(int S, dim3 grid, hipStream_t st, const uint16_t* qkv, const uint16_t* kc, const uint16_t* vc, const uint8_t* key_valid,
                int kv_stride, uint16_t* out, int heads, int past, const int32_t* past_dev, int ctx_max, float* partials, unsigned* arrivals) {
#define VLY_SPEC_CASE(SV)                                                                                                         \
    case SV:                                                                                                                      \
        hipLaunchKernelGGL((spec_attn_kernel<SV, DT>), grid, dim3(256), 0, st, qkv, kc, vc, key_valid, kv_stride, out, heads, past, \
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
