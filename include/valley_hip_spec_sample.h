/*
 * valley_hip_spec_sample.h — C ABI of libvalley_hip_spec_sample.so, the one gfx950 kernel that prompt-lookup speculative
 * decoding adds under SEEDED SAMPLING: the draw counters of the verify step's k + 1 rows, written from the device-side
 * position so that the captured step needs no host value.
 *
 * A companion of libvalley_hip_spec.so (include/valley_hip_spec.h), whose exports and ABI version stay as they are: a greedy
 * speculative generation never maps this library.  int32 only, so one build serves every storage type.  Conventions as in
 * valley_hip_spec.h: device pointers owned by the caller, nothing allocated, `stream` is a hipStream_t passed as void*, 0 on
 * success, -22 (EINVAL) on bad arguments (message in vly_spec_sample_last_error(), thread-local), -(1000 + hipError_t) if
 * the launch failed.
 *
 * Why counters are all the sampled verify step needs.  vly_argmax (include/valley_hip.h) draws by Gumbel-max with Philox
 * noise at (seed, c), c = the index, in the row's sequence, of the token being drawn.  The token drawn at index P is
 * therefore a function of the logits at P and the seed alone — not of the launch, nor of the row of it, that computed them.
 * Row j of the verify step holds the logits behind position pos + j, so it draws the token of index pos + j + 1: with
 * rows = k + 1 copies of the sequence's vly_sample_row, ctr = the table below, ctr_per_row = 1 and ctr_add = 1 it draws
 * exactly what the one-token step draws there with ctr = pos, ctr_add = 1.  vly_spec_accept then compares the drafts with
 * those draws instead of with the argmax: the leading drafts that equal the draws of the rows before them are the tokens
 * plain seeded decoding would have drawn, and the draw behind the last accepted draft is one more.
 */
#ifndef VALLEY_HIP_SPEC_SAMPLE_H
#define VALLEY_HIP_SPEC_SAMPLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VLY_SPEC_SAMPLE_ABI_VERSION 1
#define VLY_SPEC_SAMPLE_MAX_DRAFT 7 /* = VLY_SPEC_MAX_DRAFT */

int vly_spec_sample_abi_version(void);
const char *vly_spec_sample_last_error(void);

/* ctr int32 [k + 1]: ctr[j] = p + j, where p = pos_dev[0] clamped to [0, ctx_max - (k + 1)] — the clamp vly_spec_attention
 * and vly_rope_kv apply to the same word, so the counters name the positions the step's rows were computed at.
 *   1 <= k <= 7, ctx_max >= k + 1.  Nothing outside ctr[0 .. k] is written.
 * Plain vector stores from one workgroup. */
int vly_spec_counters(const int32_t *pos_dev, int k, int ctx_max, int32_t *ctr, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VALLEY_HIP_SPEC_SAMPLE_H */
