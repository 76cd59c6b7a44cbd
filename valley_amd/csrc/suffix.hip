// libvalley_hip_suffix.so (include/valley_hip_suffix.h): causal attention of 1..64 new queries over a cached prefix, split over
// the keys — the launch a conversation's next turn makes when the earlier turns' K / V are still in the cache.
//
// llama_attn2_kernel (attention.hip) is the model: the same LDS-DMA double buffer (K swizzled on the source address, V row-major
// and read through ds_read_b64_tr_b16), the same fragments (S^T = K Q^T with K as the A operand, so P is born in the B position
// of O^T = V^T P^T), the same fp32 online softmax.  What differs:
//   * grid (heads, B, splits): a workgroup walks a contiguous range of the 64-key tiles, not all of them;
//   * four waves, not eight; wave w owns the queries 16w .. 16w + 15, and a wave with 16w >= S only stages;
//   * each split publishes (m, l, o[128]) per query and the last workgroup of the (sequence, head) to arrive merges them in
//     split order (the ticket hand-off of spec_attn.inc, in its fenced form).
// One build serves both 16-bit storage types (DT = 0: bf16, 1: IEEE fp16), as spec.hip does.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "common.hpp"
#include "companion_capi.hpp"
#include "../../include/valley_hip_suffix.h"

namespace {

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) _Float16 sx_h8;
typedef __attribute__((ext_vector_type(2))) _Float16 sx_f16x2;
typedef __attribute__((ext_vector_type(2))) __bf16 sx_bf16x2;

constexpr float LOG2E = 1.4426950408889634f;
constexpr float NEG_BIG = -1.0e30f;
constexpr int PART = VLY_SUFFIX_PARTIAL;
constexpr int MAX_SPLITS = VLY_SUFFIX_MAX_SPLITS;
constexpr int TILES_PER_SPLIT = VLY_SUFFIX_TILES_PER_SPLIT;
constexpr int SX_TILE = 64 * 256;            // one K or V tile: 64 keys x 128 d x 2 B
constexpr int SX_BUF = 2 * SX_TILE;
constexpr int SC1 = 16;                      // cache-policy bit of a buffer load / store: agent scope (through to where every XCD sees it)
static_assert(PART >= 132 && PART % 4 == 0, "m, l, 2 unused, o[128]; 16-byte aligned o");

// the header's rule, for the host (the grid) and the device (a position read there)
__host__ __device__ inline int suffix_splits(int kv_len) {
    const int tiles = (kv_len + 63) >> 6;
    const int s = (tiles + TILES_PER_SPLIT - 1) / TILES_PER_SPLIT;
    return s < 1 ? 1 : (s > MAX_SPLITS ? MAX_SPLITS : s);
}

template <int DT> VLY_DEVICE f32x4 t_mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
    if constexpr (DT == 1) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(sx_h8, a), __builtin_bit_cast(sx_h8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <int DT> VLY_DEVICE uint32_t t_pack2(float lo, float hi) {
    const vly_f32x2 v = {lo, hi};
    if constexpr (DT == 1) return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, sx_f16x2));
    else return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, sx_bf16x2));
}

VLY_DEVICE int opaque_i32(int v) {            // (attention.hip: keeps the per-dt V offsets out of loop-invariant registers)
    asm volatile("" : "+v"(v));
    return v;
}

// v (op)= v[lane ^ 16], then v[lane ^ 32]: the four lane groups of a query column (attention.hip's rows4_reduce)
template <typename OP>
VLY_DEVICE float rows4_reduce(float v, OP op) {
    {
        const uint32_t x = __float_as_uint(v);
        const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
        v = op(__uint_as_float(r[0]), __uint_as_float(r[1]));
    }
    {
        const uint32_t x = __float_as_uint(v);
        const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
        v = op(__uint_as_float(r[0]), __uint_as_float(r[1]));
    }
    return v;
}

VLY_DEVICE bf16x8 vt_frag256(const char* lo_addr) {          // two transpose reads: keys +0..3 and +16..19 of this lane group's rows
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lo_addr));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lo_addr + 16 * 256));
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// grid (heads, B, splits), 256 threads.  partials fp32 [((b * heads + h) * S + i) * splits + sp][PART]; arrivals uint32 [B * heads].
template <int DT>
__global__ void __launch_bounds__(256, 2) suffix_attn_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ kc,
                                                            const uint16_t* __restrict__ vc, const uint8_t* __restrict__ key_valid,
                                                            int kv_stride, uint16_t* __restrict__ out, int S, int heads, int past,
                                                            const int32_t* __restrict__ past_dev, int ctx_max,
                                                            float* __restrict__ partials, unsigned* __restrict__ arrivals) {
    __shared__ __attribute__((aligned(16))) char smem[2 * SX_BUF];
    __shared__ int last_s;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int h = blockIdx.x, b = blockIdx.y, sp = blockIdx.z;
    const int Hq = heads * 128;
    if (past_dev) past = max(0, min(past_dev[0], ctx_max - S));
    const int kv_len = past + S;
    // the grid's z extent is the rule at the HOST's position (at ctx_max with a device-side one): the splits beyond the rule
    // at the position in force have nothing to do and take no ticket
    const int nsplit = suffix_splits(kv_len);
    if (sp >= nsplit) return;
    const int ntiles = (kv_len + 63) >> 6;
    const int t0 = sp * ntiles / nsplit, t1 = (sp + 1) * ntiles / nsplit;

    const int q = wave * 16 + l15;                        // query row inside this call
    const int qc = min(q, S - 1);
    const int qpos = past + q;                            // absolute position: keys <= qpos are visible
    const bool owner = wave * 16 < S;                     // (wave-uniform) this wave has queries
    const int wave_qpos_max = past + min(wave * 16 + 15, S - 1);

    // ---- staging: wave w issues K pieces 4w .. 4w + 3 and V pieces 4w .. 4w + 3 of a tile (piece p = rows 4p .. 4p + 3);
    // descriptors at THIS (batch, head)'s rows, 32-bit lane offsets inside the head (llama_attn2_kernel)
    const size_t head_off = ((size_t)b * heads + h) * (size_t)ctx_max * 128;
    const __amdgpu_buffer_rsrc_t rsK = vly_rsrc(kc + head_off), rsV = vly_rsrc(vc + head_off);
    const __amdgpu_buffer_rsrc_t rsM = vly_rsrc(key_valid ? key_valid + (size_t)b * kv_stride : key_valid);
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    uint32_t okraw = 1u;
    bool okin = false;
    auto stage = [&](int kt, int buf) {
        const int kv0 = kt * 64;
#pragma unroll
        for (int pp = 0; pp < 4; ++pp) {
            const int pc = 4 * wave + pp, row = 4 * pc + (lane >> 4), cp = lane & 15;
            const uint32_t rb = (uint32_t)min(kv0 + row, kv_len - 1) * 256u;               // (rows past kv_len re-read the last key: masked)
            const uint32_t voK = rb + (uint32_t)((cp ^ (row & 15)) << 4);
            const uint32_t voV = rb + (uint32_t)((cp ^ ((row & 7) << 1)) << 4);
            const uint32_t dst = __builtin_amdgcn_readfirstlane(lds0 + (uint32_t)buf * SX_BUF + (uint32_t)pc * 1024u);
            asm volatile("s_mov_b32 m0, %0" ::"s"(dst) : "memory");
            asm volatile("s_nop 0" ::: "memory");
            asm volatile("buffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(voK), "s"(rsK) : "memory");
            asm volatile("s_mov_b32 m0, %0" ::"s"(dst + (uint32_t)SX_TILE) : "memory");
            asm volatile("s_nop 0" ::: "memory");
            asm volatile("buffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(voV), "s"(rsV) : "memory");
        }
        const int kvl = kv0 + lane;
        okin = kvl < kv_len;
        if (key_valid) okraw = (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rsM, (uint32_t)min(kvl, kv_len - 1), 0, 0);
    };
    const int vr = 4 * g + (l15 >> 2);
    const int vbase0 = SX_TILE + vr * 256 + (l15 & 1) * 8 + (((l15 & 3) >> 1) << 4), vx0 = (vr & 7) << 5;

    if (t0 < t1) stage(t0, 0);
    const uint16_t* qp = qkv + ((size_t)b * S + qc) * 3 * Hq + h * 128;
    bf16x8 qf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[kk] = *(const bf16x8*)(qp + kk * 32 + g * 8);

    const float sc = 0.08838834764831845f * LOG2E;        // 128^-0.5 * log2(e)
    float m = NEG_BIG, l = 0.f;
    f32x4 o[8];
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kt = t0; kt < t1; ++kt) {
        const int kv0 = kt * 64, buf = (kt - t0) & 1;
        const char* sK = smem + buf * SX_BUF;
        // this wave's pieces of tile kt have landed (the BUILTIN wait: vmcnt(0) alone), then everyone's, and everyone is done
        // with the other buffer
        __builtin_amdgcn_s_waitcnt(0x0f70);
        __syncthreads();
        const unsigned long long vmask = __ballot(okin && (okraw & 0xffu) != 0u);
        if (kt + 1 < t1) stage(kt + 1, buf ^ 1);          // in flight while this tile is multiplied
        if (!owner || kv0 > wave_qpos_max) continue;      // no queries here, or every key of this tile is in this wave's future
        const int vbase = opaque_i32(vbase0), vx = opaque_i32(vx0);

        // ---- S^T tile ---------------------------------------------------------------------------
        f32x4 s[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const bf16x8 kf = *(const bf16x8*)(sK + (t * 16 + l15) * 256 + (((kk * 4 + g) ^ l15) << 4));
                acc = t_mfma16<DT>(kf, qf[kk], acc);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kl = t * 16 + 4 * g + r;
                const bool vis = ((vmask >> kl) & 1ull) && (kv0 + kl <= qpos);
                s[t][r] = vis ? acc[r] * sc : NEG_BIG;
            }
        }
        // ---- online softmax ------------------------------------------------------------------------
        float rm = NEG_BIG;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) rm = fmaxf(rm, s[t][r]);
        rm = rows4_reduce(rm, [](float a, float c) { return fmaxf(a, c); });
        const float mn = fmaxf(m, rm);
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        m = mn;
        float ps = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(s[t][r] - mn);
                s[t][r] = p;
                ps += p;
            }
        l = l * alpha + ps;                                // per-lane partial; the 4 g-lanes share alpha
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) o[dt] *= alpha;
        // ---- O^T += V^T P^T ------------------------------------------------------------------------
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            u32x4 pk;
            pk[0] = t_pack2<DT>(s[2 * c][0], s[2 * c][1]);
            pk[1] = t_pack2<DT>(s[2 * c][2], s[2 * c][3]);
            pk[2] = t_pack2<DT>(s[2 * c + 1][0], s[2 * c + 1][1]);
            pk[3] = t_pack2<DT>(s[2 * c + 1][2], s[2 * c + 1][3]);
            const bf16x8 pf = __builtin_bit_cast(bf16x8, pk);
#pragma unroll
            for (int dt = 0; dt < 8; ++dt)
                o[dt] = t_mfma16<DT>(vt_frag256(sK + vbase + ((dt << 5) ^ vx) + c * 8192), pf, o[dt]);
        }
    }
    l = rows4_reduce(l, [](float a, float c) { return a + c; });

    // ---- one split (kv_len <= 64 x VLY_SUFFIX_TILES_PER_SPLIT): nothing to merge, the rows leave as llama_attn2_kernel's do —
    // the bits the merge of one partial would give (weight exp2(0) = 1), without the partials and the ticket
    if (nsplit == 1) {
        if (q < S) {
            const float inv = 1.f / l;
            uint16_t* op = out + ((size_t)b * S + q) * Hq + h * 128 + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) {
                u32x2 pk;
                pk[0] = t_pack2<DT>(o[dt][0] * inv, o[dt][1] * inv);
                pk[1] = t_pack2<DT>(o[dt][2] * inv, o[dt][3] * inv);
                *(u32x2*)(op + dt * 16) = pk;
            }
        }
        return;
    }

    // ---- publish (m, l, o[128]) of this split's queries: 16-byte write-through stores (sc1: agent scope, what the relaxed
    // agent-scope atomic stores of spec_attn.inc compile to, four floats at a time — a lane's o[dt] IS four consecutive d).  A
    // query that saw no tile here (a range wholly in its future) leaves m = NEG_BIG, l = 0, o = 0: weight exp2(NEG_BIG - m) = 0.
    // The descriptor starts at this (sequence, head)'s block of S x nsplit partials (at most 64 x 16 x 528 B): 32-bit offsets.
    const __amdgpu_buffer_rsrc_t rsP = vly_rsrc(partials + ((size_t)b * heads + h) * (size_t)S * nsplit * PART);
    if (q < S) {
        const uint32_t pb = (uint32_t)((q * nsplit + sp) * PART) * 4u;
        if (g == 0) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f32x4{m, l, 0.f, 0.f}), rsP, pb, 0, SC1);
#pragma unroll
        for (int dt = 0; dt < 8; ++dt)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o[dt]), rsP, pb + (uint32_t)(4 + dt * 16 + 4 * g) * 4u, 0, SC1);
    }

    // ---- the last of the head's workgroups to get here merges: the partials are drained and released before the ticket,
    // acquired behind it; nobody waits for anybody
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned* ctr = arrivals + (size_t)b * heads + h;
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_s = t == (unsigned)(nsplit - 1);
        if (t == (unsigned)(nsplit - 1)) {
            __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
    }
    __syncthreads();
    if (!last_s) return;
    // 32 lanes x 4 dims per query, in split order: m = max m_s, L = sum l_s w_s, O = sum o_s w_s with w_s = exp2(m_s - m); the
    // loads are 16-byte agent-scope ones (sc1), all of a split's in flight together
    for (int item = tid; item < S * 32; item += 256) {
        const int i = item >> 5, ln = item & 31;
        const uint32_t hb = (uint32_t)(i * nsplit * PART) * 4u;
        float mx = NEG_BIG;
#pragma unroll 4
        for (int s2 = 0; s2 < nsplit; ++s2)
            mx = fmaxf(mx, __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsP, hb + (uint32_t)(s2 * PART) * 4u, 0, SC1))[0]);
        float L = 0.f;
        f32x4 O = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int s2 = 0; s2 < nsplit; ++s2) {
            const f32x4 ml = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsP, hb + (uint32_t)(s2 * PART) * 4u, 0, SC1));
            const f32x4 os = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsP, hb + (uint32_t)(s2 * PART + 4 + 4 * ln) * 4u, 0, SC1));
            const float w = __builtin_amdgcn_exp2f(ml[0] - mx);
            L = __builtin_fmaf(ml[1], w, L);
#pragma unroll
            for (int r = 0; r < 4; ++r) O[r] = __builtin_fmaf(os[r], w, O[r]);
        }
        const float inv = 1.f / L;
        u32x2 pk;
        pk[0] = t_pack2<DT>(O[0] * inv, O[1] * inv);
        pk[1] = t_pack2<DT>(O[2] * inv, O[3] * inv);
        *(u32x2*)(out + ((size_t)b * S + i) * Hq + h * 128 + 4 * ln) = pk;
    }
}

}  // namespace

VLY_COMPANION_CAPI(suffix, VLY_SUFFIX_ABI_VERSION)

extern "C" size_t vly_suffix_scratch_bytes(int B, int S, int heads) {
    if (B <= 0 || S <= 0 || S > VLY_SUFFIX_MAX_QUERIES || heads <= 0) return 0;
    return ((size_t)B * heads * S * MAX_SPLITS * PART + (size_t)B * heads) * 4;
}

extern "C" int vly_suffix_attention(const void* qkv, const void* kcache, const void* vcache, const uint8_t* key_valid, int key_valid_stride,
                                    void* out, int B, int S, int heads, int past, const int32_t* past_dev, int ctx_max, int dtype,
                                    void* scratch, void* stream) {
    if (B <= 0 || S <= 0 || S > VLY_SUFFIX_MAX_QUERIES || heads <= 0 || past < 0 || (long)past + S > ctx_max || B > 65535 || heads > 65535 ||
        (dtype != 0 && dtype != 1) || !qkv || !kcache || !vcache || !out || !scratch || ((uintptr_t)qkv & 15) || ((uintptr_t)kcache & 15) ||
        ((uintptr_t)vcache & 15) || ((uintptr_t)out & 7) || ((uintptr_t)scratch & 15)) {
        set_error("vly_suffix_attention: bad args B=%d S=%d (1..%d) heads=%d past=%d ctx_max=%d dtype=%d (16-byte aligned qkv / caches / "
                  "scratch required)", B, S, VLY_SUFFIX_MAX_QUERIES, heads, past, ctx_max, dtype);
        return -22;
    }
    // (a device-side position can be anything up to ctx_max - S: the rows must span the cache)
    if (key_valid && key_valid_stride < (past_dev ? ctx_max : past + S)) {
        set_error("vly_suffix_attention: key_valid_stride %d < %d (kv_len; ctx_max with a device-side position)", key_valid_stride,
                  past_dev ? ctx_max : past + S);
        return -22;
    }
    float* partials = (float*)scratch;
    unsigned* arrivals = (unsigned*)(partials + (size_t)B * heads * S * MAX_SPLITS * PART);
    // the rule at the host's position; with a device-side one the largest the rule can give inside this cache (workgroups
    // beyond the rule at the position in force return at once)
    const dim3 grid(heads, B, past_dev ? suffix_splits(ctx_max) : suffix_splits(past + S));
    if (dtype == 1)
        hipLaunchKernelGGL(suffix_attn_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, (const uint16_t*)qkv, (const uint16_t*)kcache,
                           (const uint16_t*)vcache, key_valid, key_valid_stride, (uint16_t*)out, S, heads, past, past_dev, ctx_max, partials,
                           arrivals);
    else
        hipLaunchKernelGGL(suffix_attn_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, (const uint16_t*)qkv, (const uint16_t*)kcache,
                           (const uint16_t*)vcache, key_valid, key_valid_stride, (uint16_t*)out, S, heads, past, past_dev, ctx_max, partials,
                           arrivals);
    return check_launch("vly_suffix_attention");
}
