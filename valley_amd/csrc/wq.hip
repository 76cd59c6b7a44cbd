// Weight-only INT8 decode (include/valley_hip_wq.h): the per-row quantizer and the weight-streaming GEMVs
// over the int8 copy of the projections.  gemv_bf16.hip's VALU form with half the bytes per weight: every wave (K < 8192)
// or four-wave workgroup (K >= 8192) owns one PAIR of weight rows — (gate, up) under SwiGLU — and streams them once with
// 16-byte non-temporal loads, sixteen weights per load; no LDS round trip for the weights (the operand is not shared
// between waves), the few activation rows stay L1 / L2 resident.  Algorithmic bytes per launch = N * K.
//
// Arithmetic, fixed for every form in this file: a weight byte becomes an fp32 value exactly, the 16-bit activation too,
// and acc = fmaf(w, a, acc) runs over a lane's chunks in order, low element first; lane l owns the chunks l, l + S,
// l + 2 S, ... (S = 64 lanes, or 256 threads where four waves split K).  Then the 64-lane butterfly (common.hpp), the
// fixed-order sum over the waves, ONE multiplication by the row's scale and gemv_kernel's epilogue.  The order depends on
// K alone: not on M, not on what the other activation rows hold, not on the epilogue, not on whether the norm ran in the
// prologue — so a request's tokens do not depend on its neighbours, and wq_gemv_norm_kernel is bit-identical to
// vly_rmsnorm + wq_gemv_kernel.
//
// One build serves both 16-bit storage types (DT = 0: bf16, 1: IEEE fp16, the codes of vly_storage_dtype), so the
// conversions are templates here; they are common.hpp's expressions (h_lo / h_hi / f2h / pack_h2) for the type named.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "common.hpp"
#include "../../include/valley_hip_wq.h"

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

typedef __attribute__((ext_vector_type(2))) _Float16 wq_f16x2;
typedef __attribute__((ext_vector_type(2))) __bf16 wq_bf16x2;

template <int DT> VLY_DEVICE float t_lo(uint32_t w) {
    if constexpr (DT == 1) return (float)__builtin_bit_cast(wq_f16x2, w)[0];
    else return __uint_as_float(w << 16);
}
template <int DT> VLY_DEVICE float t_hi(uint32_t w) {
    if constexpr (DT == 1) return (float)__builtin_bit_cast(wq_f16x2, w)[1];
    else return __uint_as_float(w & 0xffff0000u);
}
template <int DT> VLY_DEVICE uint16_t t_f2h(float f) {                    // round-to-nearest-even
    if constexpr (DT == 1) return __builtin_bit_cast(uint16_t, (_Float16)f);
    else return __builtin_bit_cast(uint16_t, (__bf16)f);
}
template <int DT> VLY_DEVICE uint32_t t_pack2(float lo, float hi) {
    const vly_f32x2 v = {lo, hi};
    if constexpr (DT == 1) return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, wq_f16x2));
    else return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, wq_bf16x2));
}

// sixteen int8 weights of one 16-byte chunk as fp32 (exact), element order = byte order
VLY_DEVICE void wq_unpack16(const u32x4& x, float (&f)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) f[4 * i + j] = (float)(int)(int8_t)(x[i] >> (8 * j));
}

// acc += sixteen products, a chain of sixteen fmas, low element first.  Pinned like vly_dot8 (common.hpp): explicit fmas, never
// contracted or re-associated, so every kernel of this file rounds alike.
template <int DT>
VLY_DEVICE float wq_dot16(const float (&w)[16], const u32x4& a0, const u32x4& a1, float acc) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        acc = __builtin_fmaf(w[2 * i], t_lo<DT>(a0[i]), acc);
        acc = __builtin_fmaf(w[2 * i + 1], t_hi<DT>(a0[i]), acc);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        acc = __builtin_fmaf(w[8 + 2 * i], t_lo<DT>(a1[i]), acc);
        acc = __builtin_fmaf(w[8 + 2 * i + 1], t_hi<DT>(a1[i]), acc);
    }
    return acc;
}

// gemv_kernel's epilogue for the row pair (n, n + 1) of activation row m: s0 / s1 are the finished integer-weight sums
template <int EPI, int OUT, int DT>
VLY_DEVICE void wq_store_pair(float s0, float s1, const float* __restrict__ scale, const float* __restrict__ R, void* __restrict__ Cv,
                              int m, int n, int N, int ldc, int ldr) {
    const bool has1 = n + 1 < N;
    float v0 = scale[n] * s0, v1 = has1 ? scale[n + 1] * s1 : 0.f;
    if constexpr (EPI == VLY_WQ_EPI_SWIGLU) {
        float o = x_sigmoid(v0, 1.f) * v1;
        // an fp32 VALUE before it is stored (gemv_kernel: keeps hipcc from folding multiply + conversion into v_fma_mixlo_f16)
        asm volatile("" : "+v"(o));
        const size_t off = (size_t)m * ldc + (n >> 1);
        if constexpr (OUT == VLY_WQ_OUT_16) ((uint16_t*)Cv)[off] = t_f2h<DT>(o);
        else ((float*)Cv)[off] = o;
    } else {
        if (R) {
            v0 += R[(size_t)m * ldr + n];
            if (has1) v1 += R[(size_t)m * ldr + n + 1];
        }
        const size_t off = (size_t)m * ldc + n;
        if constexpr (OUT == VLY_WQ_OUT_16) {
            ((uint16_t*)Cv)[off] = t_f2h<DT>(v0);
            if (has1) ((uint16_t*)Cv)[off + 1] = t_f2h<DT>(v1);
        } else {
            ((float*)Cv)[off] = v0;
            if (has1) ((float*)Cv)[off + 1] = v1;
        }
    }
}

// KS = 1: each of the workgroup's four waves owns a row pair (K < 8192: a 13B q|k|v / o / gate|up row is five 1 KB wave loads).
// KS = 4: the workgroup owns one pair and its waves split K (the down projection's 13.5 KB rows), partial sums meet in LDS.
template <int MR, int EPI, int OUT, int DT, int KS>
__global__ void __launch_bounds__(256) wq_gemv_kernel(const uint16_t* __restrict__ A, const int8_t* __restrict__ W,
                                                      const float* __restrict__ scale, const float* __restrict__ R,
                                                      void* __restrict__ Cv, int M, int N, int K, int lda, int ldw, int ldc, int ldr) {
    __shared__ float red[KS == 1 ? 1 : KS * 2 * MR];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = (KS == 1 ? blockIdx.x * 4 + wave : blockIdx.x) * 2;
    if (n0 >= N) return;
    const int8_t* w0 = W + (size_t)n0 * ldw;
    const int8_t* w1 = W + (size_t)min(n0 + 1, N - 1) * ldw;          // a row past the end re-reads the last one; never stored
    float acc0[MR], acc1[MR];
#pragma unroll
    for (int m = 0; m < MR; ++m) { acc0[m] = 0.f; acc1[m] = 0.f; }
    const int nch = K >> 4;
#pragma clang loop unroll_count(MR <= 2 ? 4 : 2)
    for (int c = (KS == 1 ? lane : wave * 64 + lane); c < nch; c += 64 * KS) {
        const u32x4 x0 = __builtin_nontemporal_load((const u32x4*)(w0 + 16 * c));
        const u32x4 x1 = __builtin_nontemporal_load((const u32x4*)(w1 + 16 * c));
        float f0[16], f1[16];
        wq_unpack16(x0, f0);
        wq_unpack16(x1, f1);
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            const u32x4* ap = (const u32x4*)(A + (size_t)min(m, M - 1) * lda + 16 * c);
            const u32x4 a0 = ap[0], a1 = ap[1];
            acc0[m] = wq_dot16<DT>(f0, a0, a1, acc0[m]);
            acc1[m] = wq_dot16<DT>(f1, a0, a1, acc1[m]);
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
        wq_store_pair<EPI, OUT, DT>(acc0[m], acc1[m], scale, R, Cv, m, n0, N, ldc, ldr);
    }
}

// ---------------------------------------------------------------------------------------------
// RMSNorm in the prologue (decode: input_layernorm -> q|k|v, post_attention_layernorm -> gate|up), gemv_norm_kernel's plan:
// 8-wave workgroups, two per CU where the registers allow (M = 1; M = 2 holds ~145 VGPRs and runs one); the first four waves
// of each compute x = rmsnorm(H) with norm_row_kernel's arithmetic, operation for operation (256 threads, float4 c = tid + 256 i, the same wave and LDS sums), into LDS; every wave then walks row pairs
// exactly as a wq_gemv_kernel<.., KS = 1> wave does, reading x from LDS.  A wave's FIRST pair is requested before the norm,
// so the weight stream starts with the kernel; the next pair's loads leave as soon as the registers are consumed, ahead of the
// current pair's butterfly and epilogue.  Pair p belongs to workgroup p % grid: every CU streams the same number of rows.
// CH = 16-byte chunks per lane and row that are held in registers (K <= 1024 CH).
// ---------------------------------------------------------------------------------------------
template <int MR, int EPI, int OUT, int DT, int CH>
__global__ void __launch_bounds__(512) wq_gemv_norm_kernel(const float* __restrict__ H, const float* __restrict__ gamma, float eps,
                                                            const int8_t* __restrict__ W, const float* __restrict__ scale,
                                                            const float* __restrict__ R, void* __restrict__ Cv, int M, int N, int K,
                                                            int ldh, int ldw, int ldc, int ldr) {
    extern __shared__ __attribute__((aligned(16))) char wq_dyn[];
    uint16_t* xs = (uint16_t*)wq_dyn;                                    // [MR][K]
    __shared__ float nred[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nvec = K >> 2, nch = K >> 4, pairs = (N + 1) >> 1;
    u32x4 x0[CH], x1[CH];
    auto load_pair = [&](int p) {
        // unconditional, branch-free loads (gemv_norm_kernel): a chunk past the row, and the pair past the end a wave requests in
        // its last trip, read W[0..15] and are never accumulated
        const bool live = p < pairs;
        const int8_t* w0 = W + (live ? (size_t)(2 * p) * ldw : 0);
        const int8_t* w1 = W + (live ? (size_t)min(2 * p + 1, N - 1) * ldw : 0);
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = lane + 64 * i;
            const int off = (live && c < nch) ? 16 * c : 0;
            x0[i] = __builtin_nontemporal_load((const u32x4*)(w0 + off));
            x1[i] = __builtin_nontemporal_load((const u32x4*)(w1 + off));
        }
    };
    const int first = (int)blockIdx.x + (int)gridDim.x * wave, stride = (int)gridDim.x * 8;
    if (wave < 4) {
        constexpr int NV = CH;                                           // ceil(K / 1024) <= CH float4 per thread cover a row
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
        for (int i = 0; i < CH; ++i) {                                   // chunk order per lane as wq_gemv_kernel<.., 1>: lane, lane + 64, ...
            const int c = lane + 64 * i;
            if (c < nch) {
                float f0[16], f1[16];
                wq_unpack16(x0[i], f0);
                wq_unpack16(x1[i], f1);
#pragma unroll
                for (int m = 0; m < MR; ++m) {
                    const u32x4* ap = (const u32x4*)(xs + (size_t)m * K + 16 * c);
                    const u32x4 a0 = ap[0], a1 = ap[1];
                    acc0[m] = wq_dot16<DT>(f0, a0, a1, acc0[m]);
                    acc1[m] = wq_dot16<DT>(f1, a0, a1, acc1[m]);
                }
            }
            // one chunk's LDS reads and fmas at a time: hoisting all CH chunks' activations costs the second workgroup per CU its registers
            __builtin_amdgcn_sched_barrier(0);
        }
        load_pair(p + stride);                                           // the registers are free: the next pair leaves now
#pragma unroll
        for (int m = 0; m < MR; ++m) { acc0[m] = wave_sum(acc0[m]); acc1[m] = wave_sum(acc1[m]); }
        if (lane == 0) {
#pragma unroll
            for (int m = 0; m < MR; ++m) {
                if (m >= M) break;
                wq_store_pair<EPI, OUT, DT>(acc0[m], acc1[m], scale, R, Cv, m, 2 * p, N, ldc, ldr);
            }
        }
    }
}

// ---- the quantizer: one 256-thread workgroup per row, two passes over the row (the second one hits L2) ----
template <int DT>
__global__ void __launch_bounds__(256) wq_quantize_kernel(const uint16_t* __restrict__ W, int8_t* __restrict__ Q, float* __restrict__ S,
                                                          int K, int ldw) {
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint16_t* w = W + (size_t)blockIdx.x * ldw;
    const int nch = K >> 3;                                              // 16-byte chunks of eight weights
    float amax = 0.f;
    for (int c = tid; c < nch; c += 256) {
        const u32x4 x = *(const u32x4*)(w + 8 * c);
#pragma unroll
        for (int i = 0; i < 4; ++i) amax = fmaxf(amax, fmaxf(fabsf(t_lo<DT>(x[i])), fabsf(t_hi<DT>(x[i]))));
    }
    amax = wave_max(amax);
    if (lane == 0) red[wave] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float s = amax > 0.f ? __fdiv_rn(amax, 127.0f) : 1.0f;
    if (tid == 0) S[blockIdx.x] = s;
    int8_t* q = Q + (size_t)blockIdx.x * K;
    auto q8 = [&](float f) {
        const float r = fminf(fmaxf(rintf(__fdiv_rn(f, s)), -127.f), 127.f);
        return (uint32_t)(int)r & 0xffu;
    };
    for (int c = tid; c < nch; c += 256) {
        const u32x4 x = *(const u32x4*)(w + 8 * c);
        u32x2 o;
        o[0] = q8(t_lo<DT>(x[0])) | (q8(t_hi<DT>(x[0])) << 8) | (q8(t_lo<DT>(x[1])) << 16) | (q8(t_hi<DT>(x[1])) << 24);
        o[1] = q8(t_lo<DT>(x[2])) | (q8(t_hi<DT>(x[2])) << 8) | (q8(t_lo<DT>(x[3])) << 16) | (q8(t_hi<DT>(x[3])) << 24);
        *(u32x2*)(q + 8 * c) = o;
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
    const int8_t* W;
    const float *scale, *R;
    void* C;
    int M, N, K, lda, ldw, ldc, ldr;
};

template <int MR, int EPI, int OUT, int DT>
void launch_plain(const GemvArgs& g, hipStream_t st) {
    if (g.K >= 8192)
        hipLaunchKernelGGL((wq_gemv_kernel<MR, EPI, OUT, DT, 4>), dim3((g.N + 1) / 2), dim3(256), 0, st, (const uint16_t*)g.A, g.W, g.scale, g.R,
                           g.C, g.M, g.N, g.K, g.lda, g.ldw, g.ldc, g.ldr);
    else
        hipLaunchKernelGGL((wq_gemv_kernel<MR, EPI, OUT, DT, 1>), dim3((g.N + 7) / 8), dim3(256), 0, st, (const uint16_t*)g.A, g.W, g.scale, g.R,
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
    const int pairs = (g.N + 1) / 2, wgs = (pairs + 7) / 8, slots = (g.M == 1 ? 2 : 1) * cu_count();    // resident workgroups (see the kernel)
    const dim3 grid(wgs < slots ? wgs : slots), block(512);
#define VLY_WQ_NORM(MR, CH)                                                                                                        \
    hipLaunchKernelGGL((wq_gemv_norm_kernel<MR, EPI, OUT, DT, CH>), grid, block, lds, st, n.H, n.gamma, n.eps, g.W, g.scale, g.R, g.C, g.M, \
                       g.N, g.K, n.ldh, g.ldw, g.ldc, g.ldr)
    if (g.M == 1) {
        if (g.K <= 4096) VLY_WQ_NORM(1, 4);
        else if (g.K <= 5120) VLY_WQ_NORM(1, 5);
        else VLY_WQ_NORM(1, 6);
    } else {
        if (g.K <= 4096) VLY_WQ_NORM(2, 4);
        else if (g.K <= 5120) VLY_WQ_NORM(2, 5);
        else VLY_WQ_NORM(2, 6);
    }
#undef VLY_WQ_NORM
}

// shared argument checks of the two GEMV entries; -> 0 or -22 with the message set
int check_gemv(const char* name, const GemvArgs& g, int max_m, int epilogue, int out, int dtype) {
    if (dtype != 0 && dtype != 1) {
        set_error("%s: dtype must be 0 (bf16) or 1 (fp16), got %d", name, dtype);
        return -22;
    }
    if (!((epilogue == VLY_WQ_EPI_NONE && (out == VLY_WQ_OUT_16 || out == VLY_WQ_OUT_F32)) || (epilogue == VLY_WQ_EPI_SWIGLU && out == VLY_WQ_OUT_16))) {
        set_error("%s: unsupported epilogue/out combination (%d,%d)", name, epilogue, out);
        return -22;
    }
    if (g.M <= 0 || g.M > max_m || g.N <= 0 || g.K <= 0 || g.K % 16 || g.ldw % 16 || g.ldw < g.K || ((uintptr_t)g.W & 15) || !g.W || !g.scale ||
        !g.C || g.ldc <= 0 || (epilogue == VLY_WQ_EPI_SWIGLU && (g.N % 2 || g.R))) {
        set_error("%s: unsupported shape/alignment M=%d N=%d K=%d ldw_bytes=%d (M <= %d, K %% 16 == 0, ldw_bytes %% 16 == 0, even N and no "
                  "residual under SwiGLU)", name, g.M, g.N, g.K, g.ldw, max_m);
        return -22;
    }
    return 0;
}

}  // namespace

extern "C" int vly_wq_abi_version(void) { return VLY_WQ_ABI_VERSION; }

extern "C" const char* vly_wq_last_error(void) { return g_err; }

extern "C" int vly_wq_quantize_rows(const void* w16, int ldw, int N, int K, int dtype, int8_t* q_out, float* scale_out, void* stream) {
    if ((dtype != 0 && dtype != 1) || N <= 0 || K <= 0 || K % 16 || ldw % 8 || ldw < K || !w16 || !q_out || !scale_out ||
        ((uintptr_t)w16 & 15) || ((uintptr_t)q_out & 15)) {
        set_error("vly_wq_quantize_rows: unsupported shape/alignment N=%d K=%d ldw=%d dtype=%d (K %% 16 == 0, ldw %% 8 == 0, 16-byte aligned)", N, K,
                  ldw, dtype);
        return -22;
    }
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 1) hipLaunchKernelGGL((wq_quantize_kernel<1>), dim3(N), dim3(256), 0, st, (const uint16_t*)w16, q_out, scale_out, K, ldw);
    else hipLaunchKernelGGL((wq_quantize_kernel<0>), dim3(N), dim3(256), 0, st, (const uint16_t*)w16, q_out, scale_out, K, ldw);
    return check_launch("vly_wq_quantize_rows");
}

#define VLY_WQ_DISPATCH(CALL)                                                                  \
    do {                                                                                       \
        if (dtype == 1) {                                                                      \
            if (epilogue == VLY_WQ_EPI_SWIGLU) CALL(VLY_WQ_EPI_SWIGLU, VLY_WQ_OUT_16, 1);      \
            else if (out == VLY_WQ_OUT_F32) CALL(VLY_WQ_EPI_NONE, VLY_WQ_OUT_F32, 1);          \
            else CALL(VLY_WQ_EPI_NONE, VLY_WQ_OUT_16, 1);                                      \
        } else {                                                                               \
            if (epilogue == VLY_WQ_EPI_SWIGLU) CALL(VLY_WQ_EPI_SWIGLU, VLY_WQ_OUT_16, 0);      \
            else if (out == VLY_WQ_OUT_F32) CALL(VLY_WQ_EPI_NONE, VLY_WQ_OUT_F32, 0);          \
            else CALL(VLY_WQ_EPI_NONE, VLY_WQ_OUT_16, 0);                                      \
        }                                                                                      \
    } while (0)

extern "C" int vly_wq_gemv(const void* A16, int lda, const int8_t* Wq, int ldw_bytes, const float* scale, const float* residual_f32, int ldr,
                           void* C, int ldc, int M, int N, int K, int epilogue, int out, int dtype, void* stream) {
    const GemvArgs g{A16, Wq, scale, residual_f32, C, M, N, K, lda, ldw_bytes, ldc, ldr};
    if (const int rc = check_gemv("vly_wq_gemv", g, 8, epilogue, out, dtype)) return rc;
    if (!A16 || lda % 8 || lda < K || ((uintptr_t)A16 & 15)) {
        set_error("vly_wq_gemv: activations need lda %% 8 == 0, lda >= K and a 16-byte aligned pointer (lda=%d K=%d)", lda, K);
        return -22;
    }
    hipStream_t st = (hipStream_t)stream;
#define VLY_WQ_PLAIN(E, O, D) launch_rows<E, O, D>(g, st)
    VLY_WQ_DISPATCH(VLY_WQ_PLAIN);
#undef VLY_WQ_PLAIN
    return check_launch("vly_wq_gemv");
}

extern "C" int vly_wq_gemv_rmsnorm_supported(int M, int K) { return M >= 1 && M <= 2 && K >= 2048 && K <= 6144 && K % 16 == 0; }

extern "C" int vly_wq_gemv_rmsnorm(const float* H_f32, int ldh, const float* gamma, float eps, const int8_t* Wq, int ldw_bytes, const float* scale,
                                   const float* residual_f32, int ldr, void* C, int ldc, int M, int N, int K, int epilogue, int out, int dtype,
                                   void* stream) {
    const GemvArgs g{nullptr, Wq, scale, residual_f32, C, M, N, K, 0, ldw_bytes, ldc, ldr};
    if (!vly_wq_gemv_rmsnorm_supported(M, K)) {
        set_error("vly_wq_gemv_rmsnorm: unsupported shape M=%d K=%d (M <= 2, 2048 <= K <= 6144, K %% 16 == 0)", M, K);
        return -22;
    }
    if (const int rc = check_gemv("vly_wq_gemv_rmsnorm", g, 2, epilogue, out, dtype)) return rc;
    if (!H_f32 || !gamma || ldh % 4 || ldh < K || ((uintptr_t)H_f32 & 15) || ((uintptr_t)gamma & 15)) {
        set_error("vly_wq_gemv_rmsnorm: H and gamma need 16-byte aligned pointers, ldh %% 4 == 0 and ldh >= K (ldh=%d K=%d)", ldh, K);
        return -22;
    }
    {   // no aliasing of the output with H: every workgroup re-reads H for its norm while others write C
        const char *h0 = (const char*)H_f32, *h1 = h0 + ((size_t)(M - 1) * ldh + K) * 4;
        const int No = epilogue == VLY_WQ_EPI_SWIGLU ? N / 2 : N;
        const char *c0 = (const char*)C, *c1 = c0 + ((size_t)(M - 1) * ldc + No) * (out == VLY_WQ_OUT_F32 ? 4 : 2);
        if (c0 < h1 && h0 < c1) {
            set_error("vly_wq_gemv_rmsnorm: C overlaps H (the norm re-reads H while C is written: not an in-place operation)");
            return -22;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const NormArgs n{H_f32, gamma, eps, ldh};
#define VLY_WQ_NORMED(E, O, D) launch_norm<E, O, D>(n, g, st)
    VLY_WQ_DISPATCH(VLY_WQ_NORMED);
#undef VLY_WQ_NORMED
    return check_launch("vly_wq_gemv_rmsnorm");
}
