/*
 * valley_hip_w4.h — C ABI of libvalley_hip_w4.so: weight-only INT4 decode for gfx950.  A symmetric quantizer of the 16-bit
 * projection weights with one fp32 scale per group of 128 consecutive k of a row, and the weight-streaming GEMVs over the
 * 4-bit copy (half a byte per weight plus 1/32 byte of scale instead of two: the decode step is a pure weight stream,
 * DESIGN.md §4.8, §4.11).
 *
 * A companion of libvalley_hip.so / libvalley_hip_f16.so with its own ABI version.  ONE build serves both 16-bit storage
 * types: every compute entry takes `dtype`, the code of vly_storage_dtype() (0 = bf16, 1 = IEEE fp16), for its 16-bit
 * operands (weights to quantize, activations, 16-bit outputs).  Conventions as in valley_hip.h: device pointers owned by
 * the caller, nothing allocated, `stream` is a hipStream_t passed as void*, 0 on success, -22 (EINVAL) on bad arguments
 * (message in vly_w4_last_error(), thread-local; nothing is launched), -(1000 + hipError_t) if a launch failed.
 *
 * Layout.  q in [-7, 7] is stored offset-binary, u = q + 8 in [1, 15], two weights per byte, eight per little-endian
 * 32-bit word.  With K2 = K / 2 bytes per row (row stride ldw_bytes >= K2), element (n, k) lies in
 *     word   d = k / 8                          (byte offset n * ldw_bytes + 4 * d),
 *     nibble p = (k % 8) / 2 + 4 * (k % 2)      of that word: bits 4 p .. 4 p + 3,
 *   i.e. byte n * ldw_bytes + 4 * (k / 8) + p / 2, low nibble when p is even, high nibble when p is odd.
 *   ((word >> 4 j) & 0x000f000f lifts the neighbours k = 8 d + 2 j and 8 d + 2 j + 1 into the two halves of a word.)
 * Scales: fp32 [N, G], G = K / 128, row-major: the scale of (n, k) is scale[n * G + k / 128].
 *
 * Arithmetic (every GEMV form).  A nibble u becomes the 16-bit float c0 + u exactly (bf16: c0 = 128, fp16: c0 = 1024, by
 * OR-ing the exponent into the word), so the kernel multiplies by q + c with
 *     c = 136 (bf16)   c = 1032 (fp16)
 * and removes c * sum(a) again.  K is cut into chunks of 32 consecutive k (one 16-byte load).  For a chunk, with
 * dot2(x, y, z) = v_dot2c_f32_bf16 / v_dot2c_f32_f16 (x0 y0 + x1 y1 + z in fp32):
 *     d = 0; for j = 0 .. 15: d = dot2(a[2j, 2j+1], (q + c)[2j, 2j+1], d)
 *     t = 0; for j = 0 .. 15: t = dot2(a[2j, 2j+1], (1, 1), t)
 *     e = fmaf(-c, t, d);   acc = fmaf(scale[n, g], e, acc)            (g = the chunk's group)
 * Lane l of a wave takes the chunks l, l + S, l + 2 S, ... in order (S = 64, or 256 where four waves split K: K >= 8192);
 * then the 64-lane butterfly, the fixed-order sum over the waves (0 + 1 + 2 + 3) and the epilogue of vly_gemv_bf16 (same
 * expressions: for equal pre-activation sums, the same bits).  The order of every fp32 operation depends on K only — never
 * on M, on the other activation rows, on the epilogue or on whether the norm ran in the prologue — so a row's result
 * depends on that row and the weights alone.  |q + c| <= 1039 times a 16-bit activation is exact in fp32; where the
 * chunk sums are exact (integer activations), every step above is.
 */
#ifndef VALLEY_HIP_W4_H
#define VALLEY_HIP_W4_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VLY_W4_ABI_VERSION 1
#define VLY_W4_GROUP 128 /* consecutive k of a row that share one scale */

/* epilogue and output codes: the values of valley_hip.h's VLY_EPI_NONE / VLY_EPI_SWIGLU and VLY_OUT_BF16 / VLY_OUT_F32 */
#define VLY_W4_EPI_NONE 0
#define VLY_W4_EPI_SWIGLU 2
#define VLY_W4_OUT_16 0 /* the 16-bit storage type named by `dtype` */
#define VLY_W4_OUT_F32 1

int vly_w4_abi_version(void);
const char *vly_w4_last_error(void);

/* Group-wise symmetric 4-bit quantization of w16 [N, K] (16-bit storage `dtype`, row stride ldw elements; K % 128 == 0,
 * ldw % 8 == 0, 16-byte aligned pointers).  For row n and group g: amax = max |w| over the group, s = amax / 7.0f (IEEE
 * fp32 division; s = 1 for an all-zero group), q = clamp(rintf(w / s), -7, 7) (IEEE division, ties to even).  -8 is never
 * produced.  q_out uint8 [N, K / 2] contiguous in the layout above, scale_out fp32 [N, K / 128].  One launch, one
 * 256-thread workgroup per row. */
int vly_w4_quantize_rows(const void *w16, int ldw, int N, int K, int dtype, uint8_t *q_out, float *scale_out, void *stream);

/* C[M <= 8, N'] = epi(sum_g scale[n, g] * sum_{k in g} A[m,k] * q[n,k]) + residual.
 *   A16 16-bit [M, K], row stride lda elements (lda % 8 == 0, 16-byte aligned); Wq uint8 [N, K / 2], row stride ldw_bytes
 *   (ldw_bytes % 16 == 0, ldw_bytes >= K / 2, 16-byte aligned), streamed once with 16-byte non-temporal loads; scale fp32
 *   [N, K / 128] contiguous; K % 128 == 0; any N >= 1.
 *   epilogue VLY_W4_EPI_NONE: N' = N; residual_f32 [M, N] (row stride ldr) or NULL is added in fp32 before the output
 *     rounding.  VLY_W4_EPI_SWIGLU: rows 2j / 2j + 1 of Wq are gate / up, N' = N / 2, C[m, j] = silu(gate) * up; N even,
 *     no residual, 16-bit output only.
 *   out: VLY_W4_OUT_16 (storage `dtype`) or VLY_W4_OUT_F32 (EPI_NONE only); C row stride ldc elements of that type.
 *   Rows of C past M and columns past N' are never written; C may alias residual_f32 (each element is read, then written,
 *   by one thread).
 * Form: two weight rows per wave (K < 8192) or per four-wave workgroup (K >= 8192, the waves split K and meet in LDS). */
int vly_w4_gemv(const void *A16, int lda, const uint8_t *Wq, int ldw_bytes, const float *scale, const float *residual_f32,
                int ldr, void *C, int ldc, int M, int N, int K, int epilogue, int out, int dtype, void *stream);

/* The same GEMV with the RMSNorm of the fp32 residual stream as prologue: A = rmsnorm(H; gamma, eps) rounded to the
 * 16-bit type, H fp32 [M, K] (row stride ldh, ldh % 4 == 0), gamma fp32 [K]; M <= 2 and 2048 <= K <= 6144
 * (vly_w4_gemv_rmsnorm_supported).  Bit-identical to vly_rmsnorm followed by vly_w4_gemv.  C must not overlap H. */
int vly_w4_gemv_rmsnorm(const float *H_f32, int ldh, const float *gamma, float eps, const uint8_t *Wq, int ldw_bytes,
                        const float *scale, const float *residual_f32, int ldr, void *C, int ldc, int M, int N, int K,
                        int epilogue, int out, int dtype, void *stream);

/* 1 when vly_w4_gemv_rmsnorm takes (M, K), else 0 (the caller then runs vly_rmsnorm + vly_w4_gemv). */
int vly_w4_gemv_rmsnorm_supported(int M, int K);

#ifdef __cplusplus
}
#endif

#endif /* VALLEY_HIP_W4_H */
