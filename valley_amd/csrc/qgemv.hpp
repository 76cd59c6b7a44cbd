// The skeleton of the weight-only decode GEMVs, included by wq.hip (int8 rows) and w4.hip (4-bit groups, §4.11) and by
// nothing else: gemv_bf16.hip's VALU form over packed weights.  Every wave (K < 8192) or four-wave workgroup (K >= 8192) owns one
// PAIR of weight rows — (gate, up) under SwiGLU — and streams them once with 16-byte non-temporal loads; no LDS round trip for the
// weights (the operand is not shared between waves), the few activation rows stay L1 / L2 resident.
//
// The kernels are templates on a FORMAT type F (Int8Rows, Int4Groups) that supplies what the formats do not share:
//   weight_t                 the packed element type
//   k_loop<MR, DT, KS>       the plain kernel's whole K loop over a lane's chunks (the two loops are unrolled differently)
//   finish()                 a finished sum -> the value the epilogue sees
//   norm_kernel<..>          the format's fused-norm kernel: it calls norm_prologue and store_pair, its pair loop stays with the format
//   K_MULT, row_bytes(), scale_ok()          the shape rule of the argument checks
//   NORM_KMAX, NORM_CH, norm_wgs_per_cu()    the fused kernel's CH ladder and resident workgroups per CU
// Nothing here asks which format it serves.
//
// Arithmetic that every format keeps (the format file states its chunk's chain): lane l owns the chunks l, l + S, l + 2 S, ...
// (S = 64 lanes, or 256 threads where four waves split K) and accumulates them in ascending order.  Then the 64-lane butterfly
// (common.hpp), the fixed-order sum over the waves, F::finish and gemv_kernel's epilogue.  The order depends on K alone: not on M, not
// on what the other activation rows hold, not on the epilogue, not on whether the norm ran in the prologue — so a request's tokens do
// not depend on its neighbours, and a format's fused-norm kernel is bit-identical to vly_rmsnorm + qgemv_kernel.
//
// One build serves both 16-bit storage types (DT = 0: bf16, 1: IEEE fp16, the codes of vly_storage_dtype), so the
// conversions are templates here; they are common.hpp's expressions (h_lo / h_hi / f2h / pack_h2) for the type named.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "common.hpp"
#include "companion_capi.hpp"

namespace {

// the epilogue and output codes of valley_hip_wq.h and valley_hip_w4.h (each format file asserts that its header agrees)
enum { QG_EPI_NONE = 0, QG_EPI_SWIGLU = 2, QG_OUT_16 = 0, QG_OUT_F32 = 1 };

typedef __attribute__((ext_vector_type(2))) _Float16 qg_f16x2;
typedef __attribute__((ext_vector_type(2))) __bf16 qg_bf16x2;

template <int DT> VLY_DEVICE float t_lo(uint32_t w) {
    if constexpr (DT == 1) return (float)__builtin_bit_cast(qg_f16x2, w)[0];
    else return __uint_as_float(w << 16);
}
template <int DT> VLY_DEVICE float t_hi(uint32_t w) {
    if constexpr (DT == 1) return (float)__builtin_bit_cast(qg_f16x2, w)[1];
    else return __uint_as_float(w & 0xffff0000u);
}
template <int DT> VLY_DEVICE uint16_t t_f2h(float f) {                    // round-to-nearest-even
    if constexpr (DT == 1) return __builtin_bit_cast(uint16_t, (_Float16)f);
    else return __builtin_bit_cast(uint16_t, (__bf16)f);
}
template <int DT> VLY_DEVICE uint32_t t_pack2(float lo, float hi) {
    const vly_f32x2 v = {lo, hi};
    if constexpr (DT == 1) return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, qg_f16x2));
    else return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, qg_bf16x2));
}

// gemv_kernel's epilogue for the row pair (n, n + 1) of activation row m: s0 / s1 are the finished sums, F::finish makes them values
template <class F, int EPI, int OUT, int DT>
VLY_DEVICE void store_pair(float s0, float s1, const float* __restrict__ scale, const float* __restrict__ R, void* __restrict__ Cv, int m, int n,
                           int N, int ldc, int ldr) {
    const bool has1 = n + 1 < N;
    float v0 = s0, v1 = s1;
    F::finish(v0, v1, scale, n, has1);
    if constexpr (EPI == QG_EPI_SWIGLU) {
        float o = x_sigmoid(v0, 1.f) * v1;
        // an fp32 VALUE before it is stored (gemv_kernel: keeps hipcc from folding multiply + conversion into v_fma_mixlo_f16)
        asm volatile("" : "+v"(o));
        const size_t off = (size_t)m * ldc + (n >> 1);
        if constexpr (OUT == QG_OUT_16) ((uint16_t*)Cv)[off] = t_f2h<DT>(o);
        else ((float*)Cv)[off] = o;
    } else {
        if (R) {
            v0 += R[(size_t)m * ldr + n];
            if (has1) v1 += R[(size_t)m * ldr + n + 1];
        }
        const size_t off = (size_t)m * ldc + n;
        if constexpr (OUT == QG_OUT_16) {
            ((uint16_t*)Cv)[off] = t_f2h<DT>(v0);
            if (has1) ((uint16_t*)Cv)[off + 1] = t_f2h<DT>(v1);
        } else {
            ((float*)Cv)[off] = v0;
            if (has1) ((float*)Cv)[off + 1] = v1;
        }
    }
}

// KS = 1: each of the workgroup's four waves owns a row pair (K < 8192: a 13B q|k|v / o / gate|up row is a few 1 KB wave loads).
// KS = 4: the workgroup owns one pair and its waves split K (the down projection's rows), partial sums meet in LDS.
template <class F, int MR, int EPI, int OUT, int DT, int KS>
__global__ void __launch_bounds__(256) qgemv_kernel(const uint16_t* __restrict__ A, const typename F::weight_t* __restrict__ W,
                                                    const float* __restrict__ scale, const float* __restrict__ R,
                                                    void* __restrict__ Cv, int M, int N, int K, int lda, int ldw, int ldc, int ldr) {
    __shared__ float red[KS == 1 ? 1 : KS * 2 * MR];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = (KS == 1 ? blockIdx.x * 4 + wave : blockIdx.x) * 2;
    if (n0 >= N) return;
    const int n1 = min(n0 + 1, N - 1);                                    // a row past the end re-reads the last one; never stored
    float acc0[MR], acc1[MR];
#pragma unroll
    for (int m = 0; m < MR; ++m) { acc0[m] = 0.f; acc1[m] = 0.f; }
    F::template k_loop<MR, DT, KS>(A, lda, M, W, ldw, scale, n0, n1, K, KS == 1 ? lane : wave * 64 + lane, acc0, acc1);
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
        store_pair<F, EPI, OUT, DT>(acc0[m], acc1[m], scale, R, Cv, m, n0, N, ldc, ldr);
    }
}

// ---------------------------------------------------------------------------------------------
// RMSNorm in the prologue (decode: input_layernorm -> q|k|v, post_attention_layernorm -> gate|up), gemv_norm_kernel's plan:
// 8-wave workgroups, two per CU where the registers allow (F::norm_wgs_per_cu); the first four waves of each compute
// x = rmsnorm(H) with norm_row_kernel's arithmetic, operation for operation (256 threads, float4 c = tid + 256 i, the same wave
// and LDS sums), into LDS; every wave then walks row pairs exactly as a qgemv_kernel<.., KS = 1> wave does, reading x from LDS.
// A wave's FIRST pair is requested before the norm, so the weight stream starts with the kernel; the next pair's loads leave as
// soon as the registers are consumed, ahead of the current pair's butterfly and epilogue.  Pair p belongs to workgroup p % grid:
// every CU streams the same number of rows.  NV = float4 per norm thread (K <= 1024 NV).
// ---------------------------------------------------------------------------------------------
// The norm prologue of a format's fused kernel, called by all eight waves: waves 0-3 load H, call first_loads() (the wave's first
// pair: issue order H first, then the weights, vmcnt retires in order) and leave x in xs [MR][K]; waves 4-7 call first_loads() and
// arrive at the same 2 MR barriers.
template <int MR, int DT, int NV, class First>
VLY_DEVICE void norm_prologue(const float* __restrict__ H, const float* __restrict__ gamma, float eps, uint16_t* xs, int M, int K, int ldh,
                              First&& first_loads) {
    __shared__ float nred[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nvec = K >> 2;
    if (wave < 4) {
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
        load_h(0);
        first_loads();
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
        first_loads();
#pragma unroll
        for (int m = 0; m < MR; ++m) {                                   // the other waves arrive at the same 2 MR barriers
            asm volatile("s_barrier" ::: "memory");
            asm volatile("s_barrier" ::: "memory");
        }
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

template <class F>
struct GemvArgs {
    const void* A;
    const typename F::weight_t* W;
    const float *scale, *R;
    void* C;
    int M, N, K, lda, ldw, ldc, ldr;
};

struct NormArgs {
    const float *H, *gamma;
    float eps;
    int ldh;
};

template <class F, int MR, int EPI, int OUT, int DT>
void launch_plain(const GemvArgs<F>& g, hipStream_t st) {
    if (g.K >= 8192)
        hipLaunchKernelGGL((qgemv_kernel<F, MR, EPI, OUT, DT, 4>), dim3((g.N + 1) / 2), dim3(256), 0, st, (const uint16_t*)g.A, g.W, g.scale, g.R,
                           g.C, g.M, g.N, g.K, g.lda, g.ldw, g.ldc, g.ldr);
    else
        hipLaunchKernelGGL((qgemv_kernel<F, MR, EPI, OUT, DT, 1>), dim3((g.N + 7) / 8), dim3(256), 0, st, (const uint16_t*)g.A, g.W, g.scale, g.R,
                           g.C, g.M, g.N, g.K, g.lda, g.ldw, g.ldc, g.ldr);
}

template <class F, int EPI, int OUT, int DT>
void launch_rows(const GemvArgs<F>& g, hipStream_t st) {
    if (g.M == 1) launch_plain<F, 1, EPI, OUT, DT>(g, st);
    else if (g.M == 2) launch_plain<F, 2, EPI, OUT, DT>(g, st);
    else if (g.M <= 4) launch_plain<F, 4, EPI, OUT, DT>(g, st);
    else launch_plain<F, 8, EPI, OUT, DT>(g, st);
}

template <class F, int MR, int EPI, int OUT, int DT, int CH>
void launch_norm_ch(const NormArgs& n, const GemvArgs<F>& g, hipStream_t st) {
    const size_t lds = (size_t)g.M * g.K * 2;
    const int pairs = (g.N + 1) / 2, wgs = (pairs + 7) / 8, slots = F::norm_wgs_per_cu(g.M) * cu_count();    // resident workgroups (see the kernel)
    hipLaunchKernelGGL((F::template norm_kernel<MR, EPI, OUT, DT, CH>), dim3(wgs < slots ? wgs : slots), dim3(512), lds, st, n.H, n.gamma, n.eps,
                       g.W, g.scale, g.R, g.C, g.M, g.N, g.K, n.ldh, g.ldw, g.ldc, g.ldr);
}

template <class F, int MR, int EPI, int OUT, int DT>
void launch_norm_rows(const NormArgs& n, const GemvArgs<F>& g, hipStream_t st) {
    if (g.K <= F::NORM_KMAX[0]) launch_norm_ch<F, MR, EPI, OUT, DT, F::NORM_CH[0]>(n, g, st);
    else if (g.K <= F::NORM_KMAX[1]) launch_norm_ch<F, MR, EPI, OUT, DT, F::NORM_CH[1]>(n, g, st);
    else launch_norm_ch<F, MR, EPI, OUT, DT, F::NORM_CH[2]>(n, g, st);
}

template <class F, int EPI, int OUT, int DT>
void launch_norm(const NormArgs& n, const GemvArgs<F>& g, hipStream_t st) {
    if (g.M == 1) launch_norm_rows<F, 1, EPI, OUT, DT>(n, g, st);
    else launch_norm_rows<F, 2, EPI, OUT, DT>(n, g, st);
}

// fn(EPI, OUT, DT) with the three codes as compile-time constants, for a combination check_gemv accepted
template <class Fn>
void dispatch(int epilogue, int out, int dtype, Fn&& fn) {
    auto by_dt = [&](auto dt) {
        if (epilogue == QG_EPI_SWIGLU) fn(std::integral_constant<int, QG_EPI_SWIGLU>{}, std::integral_constant<int, QG_OUT_16>{}, dt);
        else if (out == QG_OUT_F32) fn(std::integral_constant<int, QG_EPI_NONE>{}, std::integral_constant<int, QG_OUT_F32>{}, dt);
        else fn(std::integral_constant<int, QG_EPI_NONE>{}, std::integral_constant<int, QG_OUT_16>{}, dt);
    };
    if (dtype == 1) by_dt(std::integral_constant<int, 1>{});
    else by_dt(std::integral_constant<int, 0>{});
}

// shared argument checks of the two GEMV entries; -> 0 or -22 with the message set
template <class F>
int check_gemv(const char* name, const GemvArgs<F>& g, int max_m, int epilogue, int out, int dtype) {
    if (dtype != 0 && dtype != 1) {
        set_error("%s: dtype must be 0 (bf16) or 1 (fp16), got %d", name, dtype);
        return -22;
    }
    if (!((epilogue == QG_EPI_NONE && (out == QG_OUT_16 || out == QG_OUT_F32)) || (epilogue == QG_EPI_SWIGLU && out == QG_OUT_16))) {
        set_error("%s: unsupported epilogue/out combination (%d,%d)", name, epilogue, out);
        return -22;
    }
    if (g.M <= 0 || g.M > max_m || g.N <= 0 || g.K <= 0 || g.K % F::K_MULT || g.ldw % 16 || g.ldw < F::row_bytes(g.K) || ((uintptr_t)g.W & 15) ||
        !g.W || !F::scale_ok(g.scale) || !g.C || g.ldc <= 0 || (epilogue == QG_EPI_SWIGLU && (g.N % 2 || g.R))) {
        set_error("%s: unsupported shape/alignment M=%d N=%d K=%d ldw_bytes=%d (M <= %d, K %% %d == 0, ldw_bytes %% 16 == 0, even N and no "
                  "residual under SwiGLU)", name, g.M, g.N, g.K, g.ldw, max_m, F::K_MULT);
        return -22;
    }
    return 0;
}

// the body of vly_*_gemv; `name` is the entry's own
template <class F>
int gemv_entry(const char* name, const void* A16, int lda, const typename F::weight_t* Wq, int ldw_bytes, const float* scale,
               const float* residual_f32, int ldr, void* C, int ldc, int M, int N, int K, int epilogue, int out, int dtype, void* stream) {
    const GemvArgs<F> g{A16, Wq, scale, residual_f32, C, M, N, K, lda, ldw_bytes, ldc, ldr};
    if (const int rc = check_gemv(name, g, 8, epilogue, out, dtype)) return rc;
    if (!A16 || lda % 8 || lda < K || ((uintptr_t)A16 & 15)) {
        set_error("%s: activations need lda %% 8 == 0, lda >= K and a 16-byte aligned pointer (lda=%d K=%d)", name, lda, K);
        return -22;
    }
    dispatch(epilogue, out, dtype, [&](auto e, auto o, auto d) { launch_rows<F, e(), o(), d()>(g, (hipStream_t)stream); });
    return check_launch(name);
}

template <class F>
int gemv_rmsnorm_supported(int M, int K) { return M >= 1 && M <= 2 && K >= 2048 && K <= 6144 && K % F::K_MULT == 0; }

// the body of vly_*_gemv_rmsnorm
template <class F>
int gemv_rmsnorm_entry(const char* name, const float* H_f32, int ldh, const float* gamma, float eps, const typename F::weight_t* Wq,
                       int ldw_bytes, const float* scale, const float* residual_f32, int ldr, void* C, int ldc, int M, int N, int K,
                       int epilogue, int out, int dtype, void* stream) {
    const GemvArgs<F> g{nullptr, Wq, scale, residual_f32, C, M, N, K, 0, ldw_bytes, ldc, ldr};
    if (!gemv_rmsnorm_supported<F>(M, K)) {
        set_error("%s: unsupported shape M=%d K=%d (M <= 2, 2048 <= K <= 6144, K %% %d == 0)", name, M, K, F::K_MULT);
        return -22;
    }
    if (const int rc = check_gemv(name, g, 2, epilogue, out, dtype)) return rc;
    if (!H_f32 || !gamma || ldh % 4 || ldh < K || ((uintptr_t)H_f32 & 15) || ((uintptr_t)gamma & 15)) {
        set_error("%s: H and gamma need 16-byte aligned pointers, ldh %% 4 == 0 and ldh >= K (ldh=%d K=%d)", name, ldh, K);
        return -22;
    }
    {   // no aliasing of the output with H: every workgroup re-reads H for its norm while others write C
        const char *h0 = (const char*)H_f32, *h1 = h0 + ((size_t)(M - 1) * ldh + K) * 4;
        const int No = epilogue == QG_EPI_SWIGLU ? N / 2 : N;
        const char *c0 = (const char*)C, *c1 = c0 + ((size_t)(M - 1) * ldc + No) * (out == QG_OUT_F32 ? 4 : 2);
        if (c0 < h1 && h0 < c1) {
            set_error("%s: C overlaps H (the norm re-reads H while C is written: not an in-place operation)", name);
            return -22;
        }
    }
    const NormArgs n{H_f32, gamma, eps, ldh};
    dispatch(epilogue, out, dtype, [&](auto e, auto o, auto d) { launch_norm<F, e(), o(), d()>(n, g, (hipStream_t)stream); });
    return check_launch(name);
}

}  // namespace
