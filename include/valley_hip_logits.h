/*
 * valley_hip_logits.h — C ABI of libvalley_hip_logits.so, the gfx950 kernels of HF's logits processors inside the decode
 * step: repetition penalty, no-repeat n-grams and the minimum-length EOS mask, plus what beam search needs around them
 * (the token history following its parent beams, and the beam candidates over processed scores).
 * transformers.generation.logits_process (RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor,
 * MinLengthLogitsProcessor, MinNewTokensLengthLogitsProcessor, in _get_logits_processor's order) is the specification.
 *
 * A companion of libvalley_hip.so / libvalley_hip_f16.so, independent of their 16-bit storage type: it reads fp32 logits
 * and int32 ids only, so one build serves the bf16, fp16 and fp32 engines.  Conventions as in valley_hip.h: device
 * pointers owned by the caller, nothing allocated, `stream` is a hipStream_t passed as void*, 0 on success, -22 (EINVAL)
 * on bad arguments (message in vly_logits_last_error(), thread-local), -(1000 + hipError_t) if a launch failed.  Every
 * argument that changes from one decode step to the next (parameters, history, lengths, tokens, parents) is read on the
 * device, so the launches can live in a captured graph and replay with new values.
 */
#ifndef VALLEY_HIP_LOGITS_H
#define VALLEY_HIP_LOGITS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VLY_LOGITS_ABI_VERSION 1

int vly_logits_abi_version(void);
const char *vly_logits_last_error(void);

/* HF's processors over the rows of logits fp32 [R, ld] (V <= ld, V <= 262144), in place; one 1024-thread workgroup per row.
 *   params int32 [R, 4] per row: { repetition penalty p as fp32 bits (1.0 = off, p > 0), no-repeat n-gram size n (0 = off),
 *     absolute minimum length m (the EOS ids are masked while len < m; 0 = off), reserved (0) }.
 *   hist int32 [R, hist_ld]: row r's token ids, positions [0, len); the whole input_ids row of HF (prompt, left padding
 *     and placeholder ids included, then every generated token).
 *   len = (len_dev ? len_dev[len_per_row ? r : 0] : 0) + len_add, clamped to hist_ld: the row's length HF's cur_len.
 *   tok int32 [R] or NULL: first hist[r, len - 1] = tok[r] (the token fed to this step is appended on the device); after
 *     the clamp, so a clamped row appends at hist_ld - 1, and a row with len < 1 appends nothing.
 * In order, for each row:
 *   log_softmax != 0: x <- x - lse, lse = m + log(sum exp(x - m)) over the row's non-NaN values (0 when m is not finite),
 *     the same routine and reduction order as vly_beam_candidates (beam search's processors see log-probabilities);
 *   p != 1: every DISTINCT id t in hist[r, :len] with 0 <= t < V gets s < 0 ? s * p : s / p, exactly once (IEEE
 *     division);
 *   n > 0 and len >= n: every window [i, i + n) of hist[r, :len] whose first n - 1 ids equal the last n - 1 bans its
 *     last id (-inf);
 *   len < m: every EOS id of eos int32 [n_eos] in [0, V) gets -inf.
 * Ids outside [0, V) are skipped: they are not penalised, not banned as a window's last id and not masked as EOS ids, but
 * inside a window's first n - 1 ids they compare like any other id.  A row with p == 1, n == 0, len >= m and
 * log_softmax == 0 is not written. */
int vly_logits_process(float *logits, int ld, int V, int R, const int32_t *params, int32_t *hist, int hist_ld,
                       const int32_t *len_dev, int len_per_row, int len_add, const int32_t *tok, const int32_t *eos, int n_eos,
                       int log_softmax, void *stream);

/* Beam search's history: in place, row r <- row parent[r] of hist int32 [R, hist_ld] over positions [lo, hi),
 * hi = (len_dev ? *len_dev : 0) + hi_add clamped to hist_ld, read on the device (vly_kv_beam_reorder's contract for the
 * token ids).  Any parent map is correct: one 256-thread workgroup owns a run of positions of every row (64 while
 * R <= 128, 8192 / R above) and stages the source ids in LDS before it writes any row.  Rows with parent[r] == r are
 * neither read nor written.  R <= 8192; the grid covers [lo, hist_ld). */
int vly_logits_history_gather(int32_t *hist, int R, int hist_ld, const int32_t *parent, int lo, const int32_t *len_dev,
                              int hi_add, void *stream);

/* Bytes of the zeroed device scratch of vly_logits_beam_candidates (the layout of vly_beam_scratch_bytes). */
size_t vly_logits_beam_scratch_bytes(int B, int nb, int K);

/* vly_beam_candidates over scores the caller has processed (vly_logits_process with log_softmax = 1):
 *   acc[r, t] = scores[r, t] + running[r] in fp32, no log-softmax; per prompt the K largest over its nb * V values, ties
 *   to the lower flat index, best first.  Arguments, outputs, limits and the NaN / signed-zero rules as
 *   vly_beam_candidates'.  The same row top-K and merge (one source): for a row the processors left alone the outputs
 *   equal vly_beam_candidates' on the raw logits. */
int vly_logits_beam_candidates(const float *scores, int ld, int V, int B, int nb, const float *running, int K,
                               const int32_t *eos, int n_eos, void *scratch, float *score, int32_t *token, int32_t *beam,
                               uint8_t *hit, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VALLEY_HIP_LOGITS_H */
