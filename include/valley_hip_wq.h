/*
 * valley_hip_wq.h — C ABI of libvalley_hip_wq.so: weight-only INT8 decode for gfx950.  A per-row symmetric quantizer of
 * the 16-bit projection weights and the weight-streaming GEMVs over the int8 copy (one byte per weight instead of two:
 * the decode step is a pure weight stream).
 *
 * A companion of libvalley_hip.so / libvalley_hip_f16.so with its own ABI version.  ONE build serves both 16-bit storage
 * types: every compute entry takes `dtype`, the code of vly_storage_dtype() (0 = bf16, 1 = IEEE fp16), for its 16-bit
 * operands (weights to quantize, activations, 16-bit outputs).  Conventions as in valley_hip.h: device pointers owned by
 * the caller, nothing allocated, `stream` is a hipStream_t passed as void*, 0 on success, -22 (EINVAL) on bad arguments
 * (message in vly_wq_last_error(), thread-local; nothing is launched), -(1000 + hipError_t) if a launch failed.
 *
 * Arithmetic (every GEMV form): products a[m,k] * q[n,k] are exact in fp32 (|q| <= 127 and a 16-bit a), accumulated in
 * fp32 by explicit fmas in a fixed order that depends on K only — never on M, on the other activation rows or on the
 * epilogue — so a row's result depends on that row and the weights alone.  The row scale multiplies the finished sum,
 * once; then the epilogue of vly_gemv_bf16 (same expressions: for equal pre-activation sums, the same bits).
 */
#ifndef VALLEY_HIP_WQ_H
#define VALLEY_HIP_WQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VLY_WQ_ABI_VERSION 1

/* epilogue and output codes: the values of valley_hip.h's VLY_EPI_NONE / VLY_EPI_SWIGLU and VLY_OUT_BF16 / VLY_OUT_F32 */
#define VLY_WQ_EPI_NONE 0
#define VLY_WQ_EPI_SWIGLU 2
#define VLY_WQ_OUT_16 0 /* the 16-bit storage type named by `dtype` */
#define VLY_WQ_OUT_F32 1

int vly_wq_abi_version(void);
const char *vly_wq_last_error(void);

/* Per-row symmetric int8 quantization of w16 [N, K] (16-bit storage `dtype`, row stride ldw elements; K % 16 == 0,
 * ldw % 8 == 0, 16-byte aligned pointers).  For row n: amax = max |w|, s = amax / 127.0f (IEEE fp32 division; s = 1 for
 * an all-zero row), q = clamp(rintf(w / s), -127, 127) (IEEE division, ties to even).  -128 is never produced.
 *   q_out int8 [N, K] contiguous, scale_out fp32 [N].  One 256-thread workgroup per row. */
int vly_wq_quantize_rows(const void *w16, int ldw, int N, int K, int dtype, int8_t *q_out, float *scale_out, void *stream);

/* C[M <= 8, N'] = epi(scale[n] * sum_k A[m,k] * Wq[n,k]) + residual.
 *   A16 16-bit [M, K], row stride lda elements (lda % 8 == 0, 16-byte aligned); Wq int8 [N, K], row stride ldw_bytes
 *   (ldw_bytes % 16 == 0, ldw_bytes >= K, 16-byte aligned), streamed once with 16-byte non-temporal loads; scale fp32 [N];
 *   K % 16 == 0; any N >= 1.
 *   epilogue VLY_WQ_EPI_NONE: N' = N; residual_f32 [M, N] (row stride ldr) or NULL is added in fp32 before the output
 *     rounding.  VLY_WQ_EPI_SWIGLU: rows 2j / 2j + 1 of Wq are gate / up (each with its own scale), N' = N / 2,
 *     C[m, j] = silu(gate) * up; N even, no residual, 16-bit output only.
 *   out: VLY_WQ_OUT_16 (storage `dtype`) or VLY_WQ_OUT_F32 (EPI_NONE only); C row stride ldc elements of that type.
 *   Rows of C past M and columns past N' are never written; C may alias residual_f32 (each element is read, then written,
 *   by one thread).
 * Form: two weight rows per wave (K < 8192) or per four-wave workgroup (K >= 8192, the waves split K and meet in LDS in
 * the fixed order 0 + 1 + 2 + 3); lane l takes the 16-byte chunks l, l + 64 (or + 256), ... of both rows in order. */
int vly_wq_gemv(const void *A16, int lda, const int8_t *Wq, int ldw_bytes, const float *scale, const float *residual_f32,
                int ldr, void *C, int ldc, int M, int N, int K, int epilogue, int out, int dtype, void *stream);

/* The same GEMV with the RMSNorm of the fp32 residual stream as prologue: A = rmsnorm(H; gamma, eps) rounded to the
 * 16-bit type, H fp32 [M, K] (row stride ldh, ldh % 4 == 0), gamma fp32 [K]; M <= 2 and 2048 <= K <= 6144
 * (vly_wq_gemv_rmsnorm_supported).  Bit-identical to vly_rmsnorm followed by vly_wq_gemv.  C must not overlap H. */
int vly_wq_gemv_rmsnorm(const float *H_f32, int ldh, const float *gamma, float eps, const int8_t *Wq, int ldw_bytes,
                        const float *scale, const float *residual_f32, int ldr, void *C, int ldc, int M, int N, int K,
                        int epilogue, int out, int dtype, void *stream);

/* 1 when vly_wq_gemv_rmsnorm takes (M, K), else 0 (the caller then runs vly_rmsnorm + vly_wq_gemv). */
int vly_wq_gemv_rmsnorm_supported(int M, int K);

#ifdef __cplusplus
}
#endif

#endif /* VALLEY_HIP_WQ_H */
