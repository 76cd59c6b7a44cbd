// Weight-only INT8 decode (include/valley_hip_wq.h): the per-row quantizer and the int8 format of the
// weight-streaming GEMVs of qgemv.hpp, which holds the plain kernel's frame, the norm prologue, the epilogue, the launches and the checks.  Half
// the 16-bit bytes per weight, sixteen weights per 16-byte load.  Algorithmic bytes per launch = N * K.
//
// Arithmetic, fixed for every form in this file: a weight byte becomes an fp32 value exactly, the 16-bit activation too,
// and acc = fmaf(w, a, acc) runs over a lane's chunks in order, low element first (the chunk order, the reductions and what keeps
// the order a function of K alone: qgemv.hpp).  A finished sum meets ONE multiplication by the row's scale before the epilogue.
#include "qgemv.hpp"
#include "../../include/valley_hip_wq.h"

static_assert(VLY_WQ_EPI_NONE == QG_EPI_NONE && VLY_WQ_EPI_SWIGLU == QG_EPI_SWIGLU && VLY_WQ_OUT_16 == QG_OUT_16 && VLY_WQ_OUT_F32 == QG_OUT_F32,
              "qgemv.hpp's codes are valley_hip_wq.h's");

namespace {

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

struct Int8Rows;

// The fused-norm kernel (qgemv.hpp describes the plan and holds its prologue): its pair registers, their loads and the pair loop
// stay here, in the form they were measured in — hipcc's code for the `live` tests below changes with any re-housing of this lambda
// or of the arrays it fills.  CH = 16-byte chunks per lane and row that are held in registers (K <= 1024 CH).
template <int MR, int EPI, int OUT, int DT, int CH>
__global__ void __launch_bounds__(512) wq_gemv_norm_kernel(const float* __restrict__ H, const float* __restrict__ gamma, float eps,
                                                            const int8_t* __restrict__ W, const float* __restrict__ scale,
                                                            const float* __restrict__ R, void* __restrict__ Cv, int M, int N, int K,
                                                            int ldh, int ldw, int ldc, int ldr) {
    extern __shared__ __attribute__((aligned(16))) char qg_dyn[];
    uint16_t* xs = (uint16_t*)qg_dyn;                                    // [MR][K]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nch = K >> 4, pairs = (N + 1) >> 1;
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
    // NV = CH float4 per norm thread cover a row: ceil(K / 1024) <= NV
    norm_prologue<MR, DT, CH>(H, gamma, eps, xs, M, K, ldh, [&] { load_pair(first); });
#pragma unroll 1
    for (int p = first; p < pairs; p += stride) {
        float acc0[MR], acc1[MR];
#pragma unroll
        for (int m = 0; m < MR; ++m) { acc0[m] = 0.f; acc1[m] = 0.f; }
#pragma unroll
        for (int i = 0; i < CH; ++i) {                                   // chunk order per lane as qgemv_kernel<.., 1>: lane, lane + 64, ...
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
                store_pair<Int8Rows, EPI, OUT, DT>(acc0[m], acc1[m], scale, R, Cv, m, 2 * p, N, ldc, ldr);
            }
        }
    }
}

struct Int8Rows {
    typedef int8_t weight_t;
    static constexpr int K_MULT = 16;
    static constexpr int NORM_KMAX[2] = {4096, 5120}, NORM_CH[3] = {4, 5, 6};
    static int row_bytes(int K) { return K; }
    static bool scale_ok(const float* scale) { return scale != nullptr; }
    // resident workgroups per CU: two at M = 1; M = 2 holds ~145 VGPRs and runs one
    static int norm_wgs_per_cu(int M) { return M == 1 ? 2 : 1; }

    static VLY_DEVICE void finish(float& v0, float& v1, const float* __restrict__ scale, int n, bool has1) {
        v0 = scale[n] * v0;
        v1 = has1 ? scale[n + 1] * v1 : 0.f;
    }

    template <int MR, int DT, int KS>
    static VLY_DEVICE void k_loop(const uint16_t* __restrict__ A, int lda, int M, const int8_t* __restrict__ W, int ldw, const float*, int n0,
                                  int n1, int K, int c0, float (&acc0)[MR], float (&acc1)[MR]) {
        const int8_t* w0 = W + (size_t)n0 * ldw;
        const int8_t* w1 = W + (size_t)n1 * ldw;
        const int nch = K >> 4;
#pragma clang loop unroll_count(MR <= 2 ? 4 : 2)
        for (int c = c0; c < nch; c += 64 * KS) {
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
    }

    template <int MR, int EPI, int OUT, int DT, int CH>
    static constexpr auto norm_kernel = wq_gemv_norm_kernel<MR, EPI, OUT, DT, CH>;
};

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

}  // namespace

VLY_COMPANION_CAPI(wq, VLY_WQ_ABI_VERSION)

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

extern "C" int vly_wq_gemv(const void* A16, int lda, const int8_t* Wq, int ldw_bytes, const float* scale, const float* residual_f32, int ldr,
                           void* C, int ldc, int M, int N, int K, int epilogue, int out, int dtype, void* stream) {
    return gemv_entry<Int8Rows>("vly_wq_gemv", A16, lda, Wq, ldw_bytes, scale, residual_f32, ldr, C, ldc, M, N, K, epilogue, out, dtype, stream);
}

extern "C" int vly_wq_gemv_rmsnorm_supported(int M, int K) { return gemv_rmsnorm_supported<Int8Rows>(M, K); }

extern "C" int vly_wq_gemv_rmsnorm(const float* H_f32, int ldh, const float* gamma, float eps, const int8_t* Wq, int ldw_bytes, const float* scale,
                                   const float* residual_f32, int ldr, void* C, int ldc, int M, int N, int K, int epilogue, int out, int dtype,
                                   void* stream) {
    return gemv_rmsnorm_entry<Int8Rows>("vly_wq_gemv_rmsnorm", H_f32, ldh, gamma, eps, Wq, ldw_bytes, scale, residual_f32, ldr, C, ldc, M, N, K,
                                        epilogue, out, dtype, stream);
}
