/*
 * valley_hip_score.h — C ABI of libvalley_hip_score.so, the gfx950 kernels of token log-probabilities: the log-softmax of
 * a chosen token, the n most probable alternatives, the decode step's per-token record and the forward-only cross-entropy.
 * torch.log_softmax / torch.topk / torch.nn.functional.cross_entropy(ignore_index=-100) are the specification.
 *
 * A companion of libvalley_hip.so / libvalley_hip_f16.so, independent of their 16-bit storage type: it reads fp32 logits
 * and int32 ids only, so one build serves the bf16, fp16 and fp32 engines.  Conventions as in valley_hip_logits.h: device
 * pointers owned by the caller, nothing allocated, `stream` is a hipStream_t passed as void*, 0 on success, -22 (EINVAL)
 * on bad arguments (message in vly_score_last_error(), thread-local), -(1000 + hipError_t) if a launch failed.  Every
 * value that changes from one decode step to the next (logits, tokens, positions) is read on the device, so the launches
 * can live in a captured graph and replay with new values.
 */
#ifndef VALLEY_HIP_SCORE_H
#define VALLEY_HIP_SCORE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VLY_SCORE_ABI_VERSION 1
#define VLY_SCORE_MAX_TOP 20

int vly_score_abi_version(void);
const char *vly_score_last_error(void);

/* Over the rows of logits fp32 [R, ld] (V <= ld, V <= 262144, R <= 2^24), read only; one 1024-thread workgroup per row,
 * columns [V, ld) never read.  Every output is optional (NULL: not computed, nothing written).
 *   lse fp32 [R]: m + log(sum exp(x - m)) over the row's non-NaN values, 0 when the maximum m is not finite — the routine
 *     and reduction order of vly_logits_process(log_softmax = 1) and vly_beam_candidates: the same bits.
 *   target int32 [R] with target_lp fp32 [R] (both or neither): target_lp[r] = x[r, t] - lse[r] for t = target[r] in
 *     [0, V); any other id (-100 included) gives 0.0f.
 *   n_top in [0, 20] with top_id int32 [R, n_top] and top_lp fp32 [R, n_top] (n_top > 0: both): the n_top largest
 *     non-NaN values of the row, best first, ties to the lower index (-0 and +0 tie); top_lp = x - lse.  A row with fewer
 *     than n_top non-NaN values ends in id -1 / -inf.
 *   copy fp32 [R, copy_ld] (copy_ld >= V): columns [0, V) of the row unchanged; columns [V, copy_ld) are not written.
 * Rows up to 32768 wide are held in registers; wider rows are streamed again by every pass, in the same visiting order. */
int vly_score_rows(const float *logits, int ld, int V, int R, const int32_t *target, float *target_lp, float *lse, int n_top,
                   int32_t *top_id, float *top_lp, float *copy, int copy_ld, void *stream);

/* The decode step's tail, once the step's token is chosen: for each row r of raw fp32 [R, raw_ld] (the logits
 * vly_score_rows saw, or its copy) lp = raw[r, tok[r]] - lse[r], 0.0f for a token outside [0, V), written to
 * lp_table[r, c] of the fp32 [R, table_ld] table; with n_top > 0 row r of top_id / top_lp [R, n_top] goes to
 * [r, c, :] of top_id_table int32 / top_lp_table fp32 [R, table_ld, n_top].
 *   c = (len_dev ? len_dev[len_per_row ? r : 0] : 0) + len_add (vly_logits_process's length convention); a row whose c is
 *   outside [0, table_ld) writes nothing.  Plain stores, no atomics. */
int vly_score_record(const float *raw, int raw_ld, int V, int R, const float *lse, const int32_t *tok, const int32_t *len_dev,
                     int len_per_row, int len_add, float *lp_table, int table_ld, int n_top, const int32_t *top_id,
                     const float *top_lp, int32_t *top_id_table, float *top_lp_table, void *stream);

/* The mean negative log-likelihood of target_lp fp32 [M] over the rows whose target int32 [M] lies in [0, V):
 *   count int32 [1] = the number of such rows; loss fp32 [1] = -(sum of their target_lp) / count, NaN when count == 0.
 * One 1024-thread workgroup: thread t adds elements t, t + 1024, ... in float64, the 1024 partial sums are added by a
 * binary tree in LDS, and the quotient is rounded to fp32 once: the same bits at every launch. */
int vly_score_loss(const float *target_lp, const int32_t *target, int M, int V, float *loss, int32_t *count, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VALLEY_HIP_SCORE_H */
