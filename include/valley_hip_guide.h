/*
 * valley_hip_guide.h — C ABI of libvalley_hip_guide.so, the gfx950 kernels of classifier-free guidance inside the decode
 * step: a prompt is decoded in two rows, a conditional one (with the video) and an unconditional one (without it, with
 * degraded frames, or behind a negative prompt), and the two rows' log-probabilities are combined before anything else
 * sees the logits.  transformers.generation.logits_process.UnbatchedClassifierFreeGuidanceLogitsProcessor (HF's
 * guidance_scale / negative_prompt_ids) is the specification of the combine; the plausibility cut-off is the "adaptive
 * plausibility constraint" of contrastive decoding (Li et al. 2023) and visual contrastive decoding (Leng et al. 2024).
 *
 * A companion of libvalley_hip.so / libvalley_hip_f16.so, independent of their 16-bit storage type: it reads fp32 logits
 * and int32 only, so one build serves the bf16, fp16, int8 and int4 engines.  Conventions as in valley_hip.h: device
 * pointers owned by the caller, nothing allocated, `stream` is a hipStream_t passed as void*, 0 on success, -22 (EINVAL)
 * on bad arguments (message in vly_guide_last_error(), thread-local), -(1000 + hipError_t) if a launch failed.
 * Every per-row value — roles, partners, scales, cut-offs — is read on the device, so a launch can live in a captured graph
 * and replay with new pairs and scales; only the pointers, ld, V and R are fixed at capture.
 */
#ifndef VALLEY_HIP_GUIDE_H
#define VALLEY_HIP_GUIDE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VLY_GUIDE_ABI_VERSION 1

/* a row's role */
#define VLY_GUIDE_NEUTRAL 0
#define VLY_GUIDE_COND 1
#define VLY_GUIDE_UNCOND 2

int vly_guide_abi_version(void);
const char *vly_guide_last_error(void);

/* The combine over the rows of logits fp32 [R, ld] (V <= ld, V < 2^24, R <= 65535), in place; one 1024-thread workgroup per
 * row; the columns [V, ld) are never touched.
 *   rows int32 [R, 4] per row: { role, partner, scale (fp32 bits), log_beta (fp32 bits) }.
 * A row whose role is not VLY_GUIDE_COND is neither read nor written.  A conditional row whose partner is outside [0, R), is
 * the row itself or names a row whose role is not VLY_GUIDE_UNCOND is left alone likewise: a malformed table changes what is
 * guided, it never reads outside [logits, logits + R * ld).  For a valid conditional row c with partner u (x = the logits):
 *   lc = x_c - lse_c, lu = x_u - lse_u, lse = m + log(sum exp(x - m)) over the row's non-NaN values (0 when the row's
 *     maximum m is not finite), in the fixed reduction order of vly_logits_process(log_softmax = 1): lc has its bits;
 *   out = scale * (lc - lu) + lu, three separately rounded fp32 operations (no FMA): HF's expression in HF's order, written
 *     into row c; row u keeps its bits.  A scale of exactly 1 gives lc itself, as HF returns the log-softmax at 1.
 *   Where HF's expression would give NaN: x_c NaN or -inf gives -inf; otherwise x_u NaN or -inf gives lc (that column gets
 *     no guidance); whatever is still NaN (infinities of equal sign, 0 * inf) gives lc.  No NaN is ever written.
 *   Plausibility cut-off: with log_beta > -inf a column with lc < (m_c - lse_c) + log_beta becomes -inf: only tokens whose
 *     conditional probability reaches beta times the most probable token's survive.  log_beta = -inf switches it off (HF).
 * A pair gives the same bits at every launch, whatever its row indices and its neighbours. */
int vly_guide_apply(float *logits, int ld, int V, int R, const int32_t *rows, void *stream);

/* Behind the argmax / draw over tok int32 [R]: every unconditional row u whose partner p is inside [0, R), is not u and has
 * the role VLY_GUIDE_COND takes tok[u] = tok[p], its conditional row's chosen token; every other entry keeps its value.  One
 * workgroup; the rows read (conditional) and the rows written (unconditional) are disjoint. */
int vly_guide_follow(int32_t *tok, int R, const int32_t *rows, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VALLEY_HIP_GUIDE_H */
