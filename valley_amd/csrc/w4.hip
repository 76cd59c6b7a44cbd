// Weight-only INT4 decode (include/valley_hip_w4.h): the group quantizer and the 4-bit format of the
// weight-streaming GEMVs of qgemv.hpp, which holds the plain kernel's frame, the norm prologue, the epilogue, the launches and the checks.  A
// quarter of the 16-bit bytes per weight, thirty-two weights per 16-byte load.  Algorithmic bytes per launch = N * K / 2 +
// N * K / 32 (weights + scales).
//
// The inner loop is not wq.hip's (extract, convert and fma per weight would cost ~7 VALU operations per weight byte): one
// v_and_or_b32 turns the two nibbles ((x >> 4 j) & 0x000f000f) of a word into two 16-bit floats c0 + u by OR-ing the exponent of
// c0 in (bf16: 128 = 0x4300, fp16: 1024 = 0x6400; ulp 1 at that exponent, so c0 + u is exact), and v_dot2c_f32_bf16 /
// v_dot2c_f32_f16 multiplies the pair with two activations AS THEY LIE IN MEMORY.  The offset c = c0 + 8 (u = q + 8) leaves again
// as c * sum(a) per 32-weight chunk, one dot2 chain with (1, 1) that both rows of the wave share.  Per chunk and activation row:
// 2 x (7 shift / and-or per word x 4 words, shared by the rows m) + 3 x 16 dot2 + 4 fma.
//
// Arithmetic, fixed for every form in this file (the header states it): per chunk d = dot2 chain from 0 over the sixteen pairs in
// k order, t = the same chain with (1, 1), e = fmaf(-c, t, d), acc = fmaf(scale[n, g], e, acc) (the chunk order, the reductions and
// what keeps the order a function of K alone: qgemv.hpp).  The scales are applied per group, so a finished sum is the value.
#include "qgemv.hpp"
#include "../../include/valley_hip_w4.h"

static_assert(VLY_W4_EPI_NONE == QG_EPI_NONE && VLY_W4_EPI_SWIGLU == QG_EPI_SWIGLU && VLY_W4_OUT_16 == QG_OUT_16 && VLY_W4_OUT_F32 == QG_OUT_F32,
              "qgemv.hpp's codes are valley_hip_w4.h's");

namespace {

// the exponent OR-ed over a nibble pair (c0 + u in both halves), (1, 1), and c = c0 + 8
template <int DT> constexpr uint32_t W4_MAGIC = DT == 1 ? 0x64006400u : 0x43004300u;
template <int DT> constexpr uint32_t W4_ONES = DT == 1 ? 0x3c003c00u : 0x3f803f80u;
template <int DT> constexpr float W4_C = DT == 1 ? 1032.0f : 136.0f;

// x0 y0 + x1 y1 + acc over two 16-bit pairs: v_dot2c_f32_f16 / v_dot2c_f32_bf16
template <int DT> VLY_DEVICE float w4_dot2(uint32_t x, uint32_t y, float acc) {
    if constexpr (DT == 1) return __builtin_amdgcn_fdot2(__builtin_bit_cast(qg_f16x2, x), __builtin_bit_cast(qg_f16x2, y), acc, false);
    else return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(qg_bf16x2, x), __builtin_bit_cast(qg_bf16x2, y), acc, false);
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

struct Int4Groups;

// The fused-norm kernel (qgemv.hpp describes the plan and holds its prologue): its pair registers, their loads and the pair loop
// stay here, in the form they were measured in — hipcc's code for the `live` tests below changes with any re-housing of this lambda
// or of the arrays it fills.  CH = 16-byte chunks per lane and row that are held in registers (K <= 2048 CH).
template <int MR, int EPI, int OUT, int DT, int CH>
__global__ void __launch_bounds__(512) w4_gemv_norm_kernel(const float* __restrict__ H, const float* __restrict__ gamma, float eps,
                                                            const uint8_t* __restrict__ W, const float* __restrict__ scale,
                                                            const float* __restrict__ R, void* __restrict__ Cv, int M, int N, int K,
                                                            int ldh, int ldw, int ldc, int ldr) {
    extern __shared__ __attribute__((aligned(16))) char qg_dyn[];
    uint16_t* xs = (uint16_t*)qg_dyn;                                    // [MR][K]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nch = K >> 5, G = K >> 7, pairs = (N + 1) >> 1;
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
    // NV = 2 * CH float4 per norm thread cover a row: ceil(K / 1024) <= NV
    norm_prologue<MR, DT, 2 * CH>(H, gamma, eps, xs, M, K, ldh, [&] { load_pair(first); });
#pragma unroll 1
    for (int p = first; p < pairs; p += stride) {
        float acc0[MR], acc1[MR];
#pragma unroll
        for (int m = 0; m < MR; ++m) { acc0[m] = 0.f; acc1[m] = 0.f; }
#pragma unroll
        for (int i = 0; i < CH; ++i) {                                   // chunk order per lane as qgemv_kernel<.., 1>: lane, lane + 64, ...
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
                store_pair<Int4Groups, EPI, OUT, DT>(acc0[m], acc1[m], scale, R, Cv, m, 2 * p, N, ldc, ldr);
            }
        }
    }
}

struct Int4Groups {
    typedef uint8_t weight_t;
    static constexpr int K_MULT = VLY_W4_GROUP;
    static constexpr int NORM_KMAX[2] = {2048, 4096}, NORM_CH[3] = {1, 2, 3};
    static int row_bytes(int K) { return K / 2; }
    static bool scale_ok(const float* scale) { return scale && !((uintptr_t)scale & 3); }
    static int norm_wgs_per_cu(int) { return 2; }                        // resident workgroups per CU

    static VLY_DEVICE void finish(float&, float&, const float*, int, bool) {}

    template <int MR, int DT, int KS>
    static VLY_DEVICE void k_loop(const uint16_t* __restrict__ A, int lda, int M, const uint8_t* __restrict__ W, int ldw,
                                  const float* __restrict__ scale, int n0, int n1, int K, int c0, float (&acc0)[MR], float (&acc1)[MR]) {
        const int G = K >> 7;
        const uint8_t* w0 = W + (size_t)n0 * ldw;
        const uint8_t* w1 = W + (size_t)n1 * ldw;
        const float* sc0 = scale + (size_t)n0 * G;
        const float* sc1 = scale + (size_t)n1 * G;
        const int nch = K >> 5;
    // U chunks per trip, unrolled by hand (the asm of w4_and_or is convergent: hipcc unrolls no loop with a remainder around it).
    // Their loads leave together and unconditionally — a chunk past the row re-reads chunk 0 and is never accumulated — so a
    // 13B row (160 or 432 chunks) is one trip with every byte in flight at once.  The chunk order per lane stays ascending.
    constexpr int U = MR <= 2 ? (KS == 1 ? 3 : 2) : 1, S = 64 * KS;
#pragma unroll 1
        for (int cb = c0; cb < nch; cb += S * U) {
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
    }

    template <int MR, int EPI, int OUT, int DT, int CH>
    static constexpr auto norm_kernel = w4_gemv_norm_kernel<MR, EPI, OUT, DT, CH>;
};

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

}  // namespace

VLY_COMPANION_CAPI(w4, VLY_W4_ABI_VERSION)

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

extern "C" int vly_w4_gemv(const void* A16, int lda, const uint8_t* Wq, int ldw_bytes, const float* scale, const float* residual_f32, int ldr,
                           void* C, int ldc, int M, int N, int K, int epilogue, int out, int dtype, void* stream) {
    return gemv_entry<Int4Groups>("vly_w4_gemv", A16, lda, Wq, ldw_bytes, scale, residual_f32, ldr, C, ldc, M, N, K, epilogue, out, dtype,
                                  stream);
}

extern "C" int vly_w4_gemv_rmsnorm_supported(int M, int K) { return gemv_rmsnorm_supported<Int4Groups>(M, K); }

extern "C" int vly_w4_gemv_rmsnorm(const float* H_f32, int ldh, const float* gamma, float eps, const uint8_t* Wq, int ldw_bytes, const float* scale,
                                   const float* residual_f32, int ldr, void* C, int ldc, int M, int N, int K, int epilogue, int out, int dtype,
                                   void* stream) {
    return gemv_rmsnorm_entry<Int4Groups>("vly_w4_gemv_rmsnorm", H_f32, ldh, gamma, eps, Wq, ldw_bytes, scale, residual_f32, ldr, C, ldc, M, N, K,
                                          epilogue, out, dtype, stream);
}
