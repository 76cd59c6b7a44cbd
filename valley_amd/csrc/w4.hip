// Weight-only INT4 decode (include/valley_hip_w4.h): the group quantizer and the weight-streaming GEMVs over the
// 4-bit copy of the projections.  wq.hip's plan with a quarter of the 16-bit bytes per weight: every wave (K < 8192) or four-wave
// workgroup (K >= 8192) owns one PAIR of weight rows — (gate, up) under SwiGLU — and streams them once with 16-byte non-temporal
// loads, thirty-two weights per load; no LDS round trip for the weights (the operand is not shared between waves), the few
// activation rows stay L1 / L2 resident.  Algorithmic bytes per launch = N * K / 2 + N * K / 32 (weights + scales).
//
// The inner loop is not wq.hip's (extract, convert and fma per weight would cost ~7 VALU operations per weight byte): one
// v_and_or_b32 turns the two nibbles ((x >> 4 j) & 0x000f000f) of a word into two 16-bit floats c0 + u by OR-ing the exponent of
// c0 in (bf16: 128 = 0x4300, fp16: 1024 = 0x6400; ulp 1 at that exponent, so c0 + u is exact), and v_dot2c_f32_bf16 /
// v_dot2c_f32_f16 multiplies the pair with two activations AS THEY LIE IN MEMORY.  The offset c = c0 + 8 (u = q + 8) leaves again
// as c * sum(a) per 32-weight chunk, one dot2 chain with (1, 1) that both rows of the wave share.  Per chunk and activation row:
// 2 x (7 shift / and-or per word x 4 words, shared by the rows m) + 3 x 16 dot2 + 4 fma.
//
// Arithmetic, fixed for every form in this file (the header states it): per chunk d = dot2 chain from 0 over the sixteen pairs in
// k order, t = the same chain with (1, 1), e = fmaf(-c, t, d), acc = fmaf(scale[n, g], e, acc); lane l owns the chunks l, l + S,
// l + 2 S, ... (S = 64 lanes, or 256 threads where four waves split K).  Then the 64-lane butterfly (common.hpp), the fixed-order
// sum over the waves and gemv_kernel's epilogue.  The order depends on K alone: not on M, not on what the other activation rows
// hold, not on the epilogue, not on whether the norm ran in the prologue — so a request's tokens do not depend on its neighbours,
// and w4_gemv_norm_kernel is bit-identical to vly_rmsnorm + w4_gemv_kernel.
//
// One build serves both 16-bit storage types (DT = 0: bf16, 1: IEEE fp16, the codes of vly_storage_dtype).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "common.hpp"
#include "../../include/valley_hip_w4.h"

namespace {

thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return -(1000 + (int)e);
    }
    return 0;
}

typedef __attribute__((ext_vector_type(2))) _Float16 w4_f16x2;
typedef __attribute__((ext_vector_type(2))) __bf16 w4_bf16x2;

template <int DT> VLY_DEVICE float t_lo(uint32_t w) {
    if constexpr (DT == 1) return (float)__builtin_bit_cast(w4_f16x2, w)[0];
    else return __uint_as_float(w << 16);
}
template <int DT> VLY_DEVICE float t_hi(uint32_t w) {
    if constexpr (DT == 1) return (float)__builtin_bit_cast(w4_f16x2, w)[1];
    else return __uint_as_float(w & 0xffff0000u);
}
template <int DT> VLY_DEVICE uint16_t t_f2h(float f) {                    // round-to-nearest-even
    if constexpr (DT == 1) return __builtin_bit_cast(uint16_t, (_Float16)f);
    else return __builtin_bit_cast(uint16_t, (__bf16)f);
}
template <int DT> VLY_DEVICE uint32_t t_pack2(float lo, float hi) {
    const vly_f32x2 v = {lo, hi};
    if constexpr (DT == 1) return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, w4_f16x2));
    else return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, w4_bf16x2));
}

// the exponent OR-ed over a nibble pair (c0 + u in both halves), (1, 1), and c = c0 + 8
template <int DT> constexpr uint32_t W4_MAGIC = DT == 1 ? 0x64006400u : 0x43004300u;
template <int DT> constexpr uint32_t W4_ONES = DT == 1 ? 0x3c003c00u : 0x3f803f80u;
template <int DT> constexpr float W4_C = DT == 1 ? 1032.0f : 136.0f;

// x0 y0 + x1 y1 + acc over two 16-bit pairs: v_dot2c_f32_f16 / v_dot2c_f32_bf16
template <int DT> VLY_DEVICE float w4_dot2(uint32_t x, uint32_t y, float acc) {
    if constexpr (DT == 1) return __builtin_amdgcn_fdot2(__builtin_bit_cast(w4_f16x2, x), __builtin_bit_cast(w4_f16x2, y), acc, false);
    else return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(w4_bf16x2, x), __builtin_bit_cast(w4_bf16x2, y), acc, false);
}

// the thirty-two weights of one 16-byte chunk as sixteen pairs of 16-bit floats c0 + u, pair j = elements (2 j, 2 j + 1)
// (x & mask) | magic as ONE instruction: hipcc splits the expression into v_and_b32 + v_or_b32 with two literals (VOP3 takes no
// literal on gfx9), which makes the unpack eleven operations a word instead of seven
VLY_DEVICE uint32_t w4_and_or(uint32_t x, uint32_t mask, uint32_t magic) {
    uint32_t r;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "s"(mask), "v"(magic));
    return r;
}

template <int DT> VLY_DEVICE void w4_unpack32(const u32x4& x, uint32_t (&p)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) p[4 * i + j] = w4_and_or(x[i] >> (4 * j), 0x000f000fu, W4_MAGIC<DT>);
}

// one chunk of both rows against activation row a[0 .. 3] (thirty-two 16-bit values): the header's d, t, e and acc, operation
// for operation.  Pinned: builtins and explicit fmas, never contracted or re-associated, so every kernel of this file rounds alike.
template <int DT>
VLY_DEVICE void w4_chunk(const uint32_t (&p0)[16], const uint32_t (&p1)[16], float s0, float s1, const u32x4 (&a)[4], float& acc0,
                         float& acc1) {
#pragma clang fp contract(off)
    float d0 = 0.f, d1 = 0.f, t = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            d0 = w4_dot2<DT>(a[i][j], p0[4 * i + j], d0);
            d1 = w4_dot2<DT>(a[i][j], p1[4 * i + j], d1);
            t = w4_dot2<DT>(a[i][j], W4_ONES<DT>, t);
        }
    acc0 = __builtin_fmaf(s0, __builtin_fmaf(-W4_C<DT>, t, d0), acc0);
    acc1 = __builtin_fmaf(s1, __builtin_fmaf(-W4_C<DT>, t, d1), acc1);
}

// gemv_kernel's epilogue for the row pair (n, n + 1) of activation row m: v0 / v1 are the finished sums (scales applied per group)
template <int EPI, int OUT, int DT>
VLY_DEVICE void w4_store_pair(float v0, float v1, const float* __restrict__ R, void* __restrict__ Cv, int m, int n, int N, int ldc, int ldr) {
    const bool has1 = n + 1 < N;
    if constexpr (EPI == VLY_W4_EPI_SWIGLU) {
        float o = x_sigmoid(v0, 1.f) * v1;
        // an fp32 VALUE before it is stored (gemv_kernel: keeps hipcc from folding multiply + conversion into v_fma_mixlo_f16)
        asm volatile("" : "+v"(o));
        const size_t off = (size_t)m * ldc + (n >> 1);
        if constexpr (OUT == VLY_W4_OUT_16) ((uint16_t*)Cv)[off] = t_f2h<DT>(o);
        else ((float*)Cv)[off] = o;
    } else {
        if (R) {
            v0 += R[(size_t)m * ldr + n];
            if (has1) v1 += R[(size_t)m * ldr + n + 1];
        }
        const size_t off = (size_t)m * ldc + n;
        if constexpr (OUT == VLY_W4_OUT_16) {
            ((uint16_t*)Cv)[off] = t_f2h<DT>(v0);
            if (has1) ((uint16_t*)Cv)[off + 1] = t_f2h<DT>(v1);
        } else {
            ((float*)Cv)[off] = v0;
            if (has1) ((float*)Cv)[off + 1] = v1;
        }
    }
}

// KS = 1: each of the workgroup's four waves owns a row pair (K < 8192: a 13B q|k|v / o / gate|up row is 2.5 KB, 2.5 wave loads).
// KS = 4: the workgroup owns one pair and its waves split K (the down projection's 6.75 KB rows), partial sums meet in LDS.
template <int MR, int EPI, int OUT, int DT, int KS>
__global__ void __launch_bounds__(256) w4_gemv_kernel(const uint16_t* __restrict__ A, const uint8_t* __restrict__ W,
                                                      const float* __restrict__ scale, const float* __restrict__ R,
                                                      void* __restrict__ Cv, int M, int N, int K, int lda, int ldw, int ldc, int ldr) {
    __shared__ float red[KS == 1 ? 1 : KS * 2 * MR];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = (KS == 1 ? blockIdx.x * 4 + wave : blockIdx.x) * 2;
    if (n0 >= N) return;
    const int n1 = min(n0 + 1, N - 1);                                    // a row past the end re-reads the last one; never stored
    const int G = K >> 7;
    const uint8_t* w0 = W + (size_t)n0 * ldw;
    const uint8_t* w1 = W + (size_t)n1 * ldw;
    const float* sc0 = scale + (size_t)n0 * G;
    const float* sc1 = scale + (size_t)n1 * G;
    float acc0[MR], acc1[MR];
#pragma unroll
    for (int m = 0; m < MR; ++m) { acc0[m] = 0.f; acc1[m] = 0.f; }
    const int nch = K >> 5;                                               // 16-byte chunks of thirty-two weights, four per group
    // U chunks per trip, unrolled by hand (the asm of w4_and_or is convergent: hipcc unrolls no loop with a remainder around it).
    // Their loads leave together and unconditionally — a chunk past the row re-reads chunk 0 and is never accumulated — so a
    // 13B row (160 or 432 chunks) is one trip with every byte in flight at once.  The chunk order per lane stays ascending.
    constexpr int U = MR <= 2 ? (KS == 1 ? 3 : 2) : 1, S = 64 * KS;
#pragma unroll 1
    for (int cb = (KS == 1 ? lane : wave * 64 + lane); cb < nch; cb += S * U) {
        u32x4 x0[U], x1[U];
        float s0[U], s1[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = cb + S * u, cc = c < nch ? c : 0;
            x0[u] = __builtin_nontemporal_load((const u32x4*)(w0 + 16 * cc));
            x1[u] = __builtin_nontemporal_load((const u32x4*)(w1 + 16 * cc));
            s0[u] = sc0[cc >> 2];
            s1[u] = sc1[cc >> 2];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = cb + S * u;
            if (c < nch) {
                uint32_t p0[16], p1[16];
                w4_unpack32<DT>(x0[u], p0);
                w4_unpack32<DT>(x1[u], p1);
#pragma unroll
                for (int m = 0; m < MR; ++m) {
                    const u32x4* ap = (const u32x4*)(A + (size_t)min(m, M - 1) * lda + 32 * c);
                    const u32x4 a[4] = {ap[0], ap[1], ap[2], ap[3]};
                    w4_chunk<DT>(p0, p1, s0[u], s1[u], a, acc0[m], acc1[m]);
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MR; ++m) { acc0[m] = wave_sum(acc0[m]); acc1[m] = wave_sum(acc1[m]); }
    if constexpr (KS > 1) {
        if (lane == 0) {
#pragma unroll
            for (int m = 0; m < MR; ++m) { red[(wave * MR + m) * 2] = acc0[m]; red[(wave * MR + m) * 2 + 1] = acc1[m]; }
        }
        __syncthreads();
        if (wave != 0) return;
#pragma unroll
        for (int m = 0; m < MR; ++m) {                       // fixed order: wave 0 + 1 + 2 + 3
            float s0 = red[m * 2], s1 = red[m * 2 + 1];
#pragma unroll
            for (int wv = 1; wv < KS; ++wv) { s0 += red[(wv * MR + m) * 2]; s1 += red[(wv * MR + m) * 2 + 1]; }
            acc0[m] = s0;
            acc1[m] = s1;
        }
    }
    if (lane != 0) return;
#pragma unroll
    for (int m = 0; m < MR; ++m) {
        if (m >= M) break;
        w4_store_pair<EPI, OUT, DT>(acc0[m], acc1[m], R, Cv, m, n0, N, ldc, ldr);
    }
}

// ---------------------------------------------------------------------------------------------
// RMSNorm in the prologue (decode: input_layernorm -> q|k|v, post_attention_layernorm -> gate|up), wq_gemv_norm_kernel's plan:
// 8-wave workgroups; the first four waves of each compute x = rmsnorm(H) with norm_row_kernel's arithmetic, operation for
// operation (256 threads, float4 c = tid + 256 i, the same wave and LDS sums), into LDS; every wave then walks row pairs exactly
// as a w4_gemv_kernel<.., KS = 1> wave does, reading x from LDS.  A wave's FIRST pair (weights and scales) is requested before
// the norm, so the weight stream starts with the kernel; the next pair's loads leave as soon as the registers are consumed, ahead
// of the current pair's butterfly and epilogue.  Pair p belongs to workgroup p % grid: every CU streams the same number of rows.
// CH = 16-byte chunks per lane and row that are held in registers (K <= 2048 CH); NV = float4 per norm thread (K <= 1024 NV).
// ---------------------------------------------------------------------------------------------
template <int MR, int EPI, int OUT, int DT, int CH>
__global__ void __launch_bounds__(512) w4_gemv_norm_kernel(const float* __restrict__ H, const float* __restrict__ gamma, float eps,
                                                            const uint8_t* __restrict__ W, const float* __restrict__ scale,
                                                            const float* __restrict__ R, void* __restrict__ Cv, int M, int N, int K,
                                                            int ldh, int ldw, int ldc, int ldr) {
    extern __shared__ __attribute__((aligned(16))) char w4_dyn[];
    uint16_t* xs = (uint16_t*)w4_dyn;                                    // [MR][K]
    __shared__ float nred[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nvec = K >> 2, nch = K >> 5, G = K >> 7, pairs = (N + 1) >> 1;
    u32x4 x0[CH], x1[CH];
    float s0[CH], s1[CH];
    auto load_pair = [&](int p) {
        // unconditional, branch-free loads (gemv_norm_kernel): a chunk past the row, and the pair past the end a wave requests in
        // its last trip, read W[0..15] / scale[0] and are never accumulated
        const bool live = p < pairs;
        const int r0 = live ? 2 * p : 0, r1 = live ? min(2 * p + 1, N - 1) : 0;
        const uint8_t* w0 = W + (size_t)r0 * ldw;
        const uint8_t* w1 = W + (size_t)r1 * ldw;
        const float* sc0 = scale + (size_t)r0 * G;
        const float* sc1 = scale + (size_t)r1 * G;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = lane + 64 * i;
            const int cc = (live && c < nch) ? c : 0;
            x0[i] = __builtin_nontemporal_load((const u32x4*)(w0 + 16 * cc));
            x1[i] = __builtin_nontemporal_load((const u32x4*)(w1 + 16 * cc));
            s0[i] = sc0[cc >> 2];
            s1[i] = sc1[cc >> 2];
        }
    };
    const int first = (int)blockIdx.x + (int)gridDim.x * wave, stride = (int)gridDim.x * 8;
    if (wave < 4) {
        constexpr int NV = 2 * CH;                                       // ceil(K / 1024) <= 2 CH float4 per thread cover a row
        float4 v[NV];
        auto load_h = [&](int m) {
            const float4* hr = (const float4*)(H + (size_t)min(m, M - 1) * ldh);
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = tid + 256 * i;
                const float4 t = hr[min(c, nvec - 1)];
                v[i] = (c < nvec) ? t : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        };
        load_h(0);                                                       // issue order: H first, then the weights (vmcnt retires in order)
        load_pair(first);
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            if (m > 0) load_h(m);
            float s = 0.f;                                               // norm_row_kernel's arithmetic, operation for operation
#pragma unroll
            for (int i = 0; i < NV; ++i) s += vly_sumsq4(v[i].x, v[i].y, v[i].z, v[i].w);
            s = wave_sum(s);
            if (lane == 0) nred[wave] = s;
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            s = nred[0] + nred[1] + nred[2] + nred[3];
            const float rstd = rsqrtf(s / (float)K + eps);
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = tid + 256 * i;
                if (c >= nvec) continue;
                const float4 gm = ((const float4*)gamma)[c];
                float4 o;
                o.x = gm.x * (v[i].x * rstd); o.y = gm.y * (v[i].y * rstd);
                o.z = gm.z * (v[i].z * rstd); o.w = gm.w * (v[i].w * rstd);
                u32x2 pk;
                pk[0] = t_pack2<DT>(o.x, o.y);
                pk[1] = t_pack2<DT>(o.z, o.w);
                *(u32x2*)(xs + (size_t)m * K + 4 * c) = pk;
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        }
    } else {
        load_pair(first);
#pragma unroll
        for (int m = 0; m < MR; ++m) {                                   // the other waves arrive at the same 2 MR barriers
            asm volatile("s_barrier" ::: "memory");
            asm volatile("s_barrier" ::: "memory");
        }
    }
#pragma unroll 1
    for (int p = first; p < pairs; p += stride) {
        float acc0[MR], acc1[MR];
#pragma unroll
        for (int m = 0; m < MR; ++m) { acc0[m] = 0.f; acc1[m] = 0.f; }
#pragma unroll
        for (int i = 0; i < CH; ++i) {                                   // chunk order per lane as w4_gemv_kernel<.., 1>: lane, lane + 64, ...
            const int c = lane + 64 * i;
            if (c < nch) {
                uint32_t p0[16], p1[16];
                w4_unpack32<DT>(x0[i], p0);
                w4_unpack32<DT>(x1[i], p1);
#pragma unroll
                for (int m = 0; m < MR; ++m) {
                    const u32x4* ap = (const u32x4*)(xs + (size_t)m * K + 32 * c);
                    const u32x4 a[4] = {ap[0], ap[1], ap[2], ap[3]};
                    w4_chunk<DT>(p0, p1, s0[i], s1[i], a, acc0[m], acc1[m]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);                           // one chunk's LDS reads and dot2s at a time
        }
        load_pair(p + stride);                                           // the registers are free: the next pair leaves now
#pragma unroll
        for (int m = 0; m < MR; ++m) { acc0[m] = wave_sum(acc0[m]); acc1[m] = wave_sum(acc1[m]); }
        if (lane == 0) {
#pragma unroll
            for (int m = 0; m < MR; ++m) {
                if (m >= M) break;
                w4_store_pair<EPI, OUT, DT>(acc0[m], acc1[m], R, Cv, m, 2 * p, N, ldc, ldr);
            }
        }
    }
}

// ---- the quantizer: one 256-thread workgroup per row, one pass; a thread holds eight weights (one packed word), the sixteen
// consecutive lanes of a group agree on its amax by a four-step xor exchange (a group never straddles a wave: 64 % 16 == 0, and
// K % 128 == 0 keeps the sixteen lanes of a group in or out of the loop together) ----
template <int DT>
__global__ void __launch_bounds__(256) w4_quantize_kernel(const uint16_t* __restrict__ W, uint8_t* __restrict__ Q, float* __restrict__ S,
                                                          int K, int ldw) {
    const int tid = threadIdx.x;
    const uint16_t* w = W + (size_t)blockIdx.x * ldw;
    uint32_t* q = (uint32_t*)(Q + (size_t)blockIdx.x * (K >> 1));
    float* sr = S + (size_t)blockIdx.x * (K >> 7);
    const int nch = K >> 3;                                              // 16-byte chunks of eight weights = one packed word
    for (int c = tid; c < nch; c += 256) {
        const u32x4 x = *(const u32x4*)(w + 8 * c);
        float amax = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) amax = fmaxf(amax, fmaxf(fabsf(t_lo<DT>(x[i])), fabsf(t_hi<DT>(x[i]))));
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 16));
        const float s = amax > 0.f ? __fdiv_rn(amax, 7.0f) : 1.0f;
        if ((tid & 15) == 0) sr[c >> 4] = s;
        auto q4 = [&](float f) {
            const float r = fminf(fmaxf(rintf(__fdiv_rn(f, s)), -7.f), 7.f);
            return (uint32_t)((int)r + 8);
        };
        uint32_t o = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) o |= (q4(t_lo<DT>(x[i])) << (4 * i)) | (q4(t_hi<DT>(x[i])) << (4 * i + 16));
        q[c] = o;
    }
}

int cu_count() {
    static const int cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        return n;
    }();
    return cus;
}

struct GemvArgs {
    const void* A;
    const uint8_t* W;
    const float *scale, *R;
    void* C;
    int M, N, K, lda, ldw, ldc, ldr;
};

template <int MR, int EPI, int OUT, int DT>
void launch_plain(const GemvArgs& g, hipStream_t st) {
    if (g.K >= 8192)
        hipLaunchKernelGGL((w4_gemv_kernel<MR, EPI, OUT, DT, 4>), dim3((g.N + 1) / 2), dim3(256), 0, st, (const uint16_t*)g.A, g.W, g.scale, g.R,
                           g.C, g.M, g.N, g.K, g.lda, g.ldw, g.ldc, g.ldr);
    else
        hipLaunchKernelGGL((w4_gemv_kernel<MR, EPI, OUT, DT, 1>), dim3((g.N + 7) / 8), dim3(256), 0, st, (const uint16_t*)g.A, g.W, g.scale, g.R,
                           g.C, g.M, g.N, g.K, g.lda, g.ldw, g.ldc, g.ldr);
}

template <int EPI, int OUT, int DT>
void launch_rows(const GemvArgs& g, hipStream_t st) {
    if (g.M == 1) launch_plain<1, EPI, OUT, DT>(g, st);
    else if (g.M == 2) launch_plain<2, EPI, OUT, DT>(g, st);
    else if (g.M <= 4) launch_plain<4, EPI, OUT, DT>(g, st);
    else launch_plain<8, EPI, OUT, DT>(g, st);
}

struct NormArgs {
    const float *H, *gamma;
    float eps;
    int ldh;
};

template <int EPI, int OUT, int DT>
void launch_norm(const NormArgs& n, const GemvArgs& g, hipStream_t st) {
    const size_t lds = (size_t)g.M * g.K * 2;
    const int pairs = (g.N + 1) / 2, wgs = (pairs + 7) / 8, slots = 2 * cu_count();    // resident workgroups (see the kernel)
    const dim3 grid(wgs < slots ? wgs : slots), block(512);
#define VLY_W4_NORM(MR, CH)                                                                                                        \
    hipLaunchKernelGGL((w4_gemv_norm_kernel<MR, EPI, OUT, DT, CH>), grid, block, lds, st, n.H, n.gamma, n.eps, g.W, g.scale, g.R, g.C, g.M, \
                       g.N, g.K, n.ldh, g.ldw, g.ldc, g.ldr)
    if (g.M == 1) {
        if (g.K <= 2048) VLY_W4_NORM(1, 1);
        else if (g.K <= 4096) VLY_W4_NORM(1, 2);
        else VLY_W4_NORM(1, 3);
    } else {
        if (g.K <= 2048) VLY_W4_NORM(2, 1);
        else if (g.K <= 4096) VLY_W4_NORM(2, 2);
        else VLY_W4_NORM(2, 3);
    }
#undef VLY_W4_NORM
}

// shared argument checks of the two GEMV entries; -> 0 or -22 with the message set
int check_gemv(const char* name, const GemvArgs& g, int max_m, int epilogue, int out, int dtype) {
    if (dtype != 0 && dtype != 1) {
        set_error("%s: dtype must be 0 (bf16) or 1 (fp16), got %d", name, dtype);
        return -22;
    }
    if (!((epilogue == VLY_W4_EPI_NONE && (out == VLY_W4_OUT_16 || out == VLY_W4_OUT_F32)) || (epilogue == VLY_W4_EPI_SWIGLU && out == VLY_W4_OUT_16))) {
        set_error("%s: unsupported epilogue/out combination (%d,%d)", name, epilogue, out);
        return -22;
    }
    if (g.M <= 0 || g.M > max_m || g.N <= 0 || g.K <= 0 || g.K % VLY_W4_GROUP || g.ldw % 16 || g.ldw < g.K / 2 || ((uintptr_t)g.W & 15) || !g.W ||
        !g.scale || ((uintptr_t)g.scale & 3) || !g.C || g.ldc <= 0 || (epilogue == VLY_W4_EPI_SWIGLU && (g.N % 2 || g.R))) {
        set_error("%s: unsupported shape/alignment M=%d N=%d K=%d ldw_bytes=%d (M <= %d, K %% 128 == 0, ldw_bytes %% 16 == 0, even N and no "
                  "residual under SwiGLU)", name, g.M, g.N, g.K, g.ldw, max_m);
        return -22;
    }
    return 0;
}

}  // namespace

extern "C" int vly_w4_abi_version(void) { return VLY_W4_ABI_VERSION; }

extern "C" const char* vly_w4_last_error(void) { return g_err; }

extern "C" int vly_w4_quantize_rows(const void* w16, int ldw, int N, int K, int dtype, uint8_t* q_out, float* scale_out, void* stream) {
    if ((dtype != 0 && dtype != 1) || N <= 0 || K <= 0 || K % VLY_W4_GROUP || ldw % 8 || ldw < K || !w16 || !q_out || !scale_out ||
        ((uintptr_t)w16 & 15) || ((uintptr_t)q_out & 3) || ((uintptr_t)scale_out & 3)) {
        set_error("vly_w4_quantize_rows: unsupported shape/alignment N=%d K=%d ldw=%d dtype=%d (K %% 128 == 0, ldw %% 8 == 0, 16-byte aligned)", N,
                  K, ldw, dtype);
        return -22;
    }
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 1) hipLaunchKernelGGL((w4_quantize_kernel<1>), dim3(N), dim3(256), 0, st, (const uint16_t*)w16, q_out, scale_out, K, ldw);
    else hipLaunchKernelGGL((w4_quantize_kernel<0>), dim3(N), dim3(256), 0, st, (const uint16_t*)w16, q_out, scale_out, K, ldw);
    return check_launch("vly_w4_quantize_rows");
}

#define VLY_W4_DISPATCH(CALL)                                                                  \
    do {                                                                                       \
        if (dtype == 1) {                                                                      \
            if (epilogue == VLY_W4_EPI_SWIGLU) CALL(VLY_W4_EPI_SWIGLU, VLY_W4_OUT_16, 1);      \
            else if (out == VLY_W4_OUT_F32) CALL(VLY_W4_EPI_NONE, VLY_W4_OUT_F32, 1);          \
            else CALL(VLY_W4_EPI_NONE, VLY_W4_OUT_16, 1);                                      \
        } else {                                                                               \
            if (epilogue == VLY_W4_EPI_SWIGLU) CALL(VLY_W4_EPI_SWIGLU, VLY_W4_OUT_16, 0);      \
            else if (out == VLY_W4_OUT_F32) CALL(VLY_W4_EPI_NONE, VLY_W4_OUT_F32, 0);          \
            else CALL(VLY_W4_EPI_NONE, VLY_W4_OUT_16, 0);                                      \
        }                                                                                      \
    } while (0)

extern "C" int vly_w4_gemv(const void* A16, int lda, const uint8_t* Wq, int ldw_bytes, const float* scale, const float* residual_f32, int ldr,
                           void* C, int ldc, int M, int N, int K, int epilogue, int out, int dtype, void* stream) {
    const GemvArgs g{A16, Wq, scale, residual_f32, C, M, N, K, lda, ldw_bytes, ldc, ldr};
    if (const int rc = check_gemv("vly_w4_gemv", g, 8, epilogue, out, dtype)) return rc;
    if (!A16 || lda % 8 || lda < K || ((uintptr_t)A16 & 15)) {
        set_error("vly_w4_gemv: activations need lda %% 8 == 0, lda >= K and a 16-byte aligned pointer (lda=%d K=%d)", lda, K);
        return -22;
    }
    hipStream_t st = (hipStream_t)stream;
#define VLY_W4_PLAIN(E, O, D) launch_rows<E, O, D>(g, st)
    VLY_W4_DISPATCH(VLY_W4_PLAIN);
#undef VLY_W4_PLAIN
    return check_launch("vly_w4_gemv");
}

extern "C" int vly_w4_gemv_rmsnorm_supported(int M, int K) { return M >= 1 && M <= 2 && K >= 2048 && K <= 6144 && K % VLY_W4_GROUP == 0; }

extern "C" int vly_w4_gemv_rmsnorm(const float* H_f32, int ldh, const float* gamma, float eps, const uint8_t* Wq, int ldw_bytes, const float* scale,
                                   const float* residual_f32, int ldr, void* C, int ldc, int M, int N, int K, int epilogue, int out, int dtype,
                                   void* stream) {
    const GemvArgs g{nullptr, Wq, scale, residual_f32, C, M, N, K, 0, ldw_bytes, ldc, ldr};
    if (!vly_w4_gemv_rmsnorm_supported(M, K)) {
        set_error("vly_w4_gemv_rmsnorm: unsupported shape M=%d K=%d (M <= 2, 2048 <= K <= 6144, K %% 128 == 0)", M, K);
        return -22;
    }
    if (const int rc = check_gemv("vly_w4_gemv_rmsnorm", g, 2, epilogue, out, dtype)) return rc;
    if (!H_f32 || !gamma || ldh % 4 || ldh < K || ((uintptr_t)H_f32 & 15) || ((uintptr_t)gamma & 15)) {
        set_error("vly_w4_gemv_rmsnorm: H and gamma need 16-byte aligned pointers, ldh %% 4 == 0 and ldh >= K (ldh=%d K=%d)", ldh, K);
        return -22;
    }
    {   // no aliasing of the output with H: every workgroup re-reads H for its norm while others write C
        const char *h0 = (const char*)H_f32, *h1 = h0 + ((size_t)(M - 1) * ldh + K) * 4;
        const int No = epilogue == VLY_W4_EPI_SWIGLU ? N / 2 : N;
        const char *c0 = (const char*)C, *c1 = c0 + ((size_t)(M - 1) * ldc + No) * (out == VLY_W4_OUT_F32 ? 4 : 2);
        if (c0 < h1 && h0 < c1) {
            set_error("vly_w4_gemv_rmsnorm: C overlaps H (the norm re-reads H while C is written: not an in-place operation)");
            return -22;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const NormArgs n{H_f32, gamma, eps, ldh};
#define VLY_W4_NORMED(E, O, D) launch_norm<E, O, D>(n, g, st)
    VLY_W4_DISPATCH(VLY_W4_NORMED);
#undef VLY_W4_NORMED
    return check_launch("vly_w4_gemv_rmsnorm");
}
