/*
 * valley_hip_spec.h — C ABI of libvalley_hip_spec.so, the gfx950 kernels of prompt-lookup speculative decoding: the split
 * attention of a few queries of one sequence over the KV cache, the draft lookup (HF's PromptLookupCandidateGenerator) and
 * the acceptance of a verified draft.
 *
 * A companion of libvalley_hip.so / libvalley_hip_f16.so.  One build serves both 16-bit storage types: the attention takes
 * the `dtype` code of vly_storage_dtype (0: bf16, 1: IEEE fp16); the other two read and write int32 only.  Conventions as
 * in valley_hip_score.h: device pointers owned by the caller, nothing allocated, `stream` is a hipStream_t passed as void*,
 * 0 on success, -22 (EINVAL) on bad arguments (message in vly_spec_last_error(), thread-local), -(1000 + hipError_t) if a
 * launch failed.  Every value that changes from one step to the next (position, history, draft, tokens) is read on the
 * device, so the launches can live in a captured graph and replay with new values.
 *
 * Greedy or seeded sampling.  vly_spec_accept compares the drafts with whatever ids `am` holds: the argmax of the verify step's
 * k + 1 logit rows, or — under seeded sampling — their DRAWS, row j drawn by vly_argmax with the counter of the position it
 * would occupy (pos + j + 1).  A draw is a function of (logits, seed, counter) alone, so the accepted tokens are the ones plain
 * seeded decoding draws.  The counters come from vly_spec_counters in the companion libvalley_hip_spec_sample.so
 * (valley_hip_spec_sample.h); this library's entries, signatures and ABI version are unchanged by it.
 */
#ifndef VALLEY_HIP_SPEC_H
#define VALLEY_HIP_SPEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VLY_SPEC_ABI_VERSION 1
#define VLY_SPEC_MAX_QUERIES 8 /* S of vly_spec_attention: k + 1 */
#define VLY_SPEC_MAX_DRAFT 7   /* k */
#define VLY_SPEC_MAX_NGRAM 8
#define VLY_SPEC_SPLITS 4       /* = VLY_DECODE_SPLITS */
#define VLY_SPEC_PARTIAL 132    /* fp32 per (sequence, head, query, split): m, l, 2 unused, o[128] */

int vly_spec_abi_version(void);
const char *vly_spec_last_error(void);

/* Causal attention of the S queries (1 <= S <= 8) of each of B sequences over the KV cache, head_dim 128 — what
 * vly_llama_attention(S, past_len_dev) computes, spread over VLY_SPEC_SPLITS workgroups per (sequence, head).
 *   qkv 16-bit [B*S, 3*heads*128], as vly_rope_kv leaves it: the first third holds the ROTATED q (the rest is not read);
 *   kcache / vcache 16-bit [B, heads, ctx_max, 128] with the rows of positions past .. past+S-1 already written; read only.
 *   out 16-bit [B*S, heads*128].
 *   past = past_len, or past_len_dev[0] clamped to [0, ctx_max - S] when past_len_dev is given (one position per launch).
 *   key_valid uint8 [B, key_valid_stride] (key_valid_stride >= past_len + S; >= ctx_max with past_len_dev) or NULL.
 * Key j is visible to query i iff j <= past + i and key_valid[b][j]; a masked key contributes exactly 0; 64-key blocks that
 * lie wholly in the future of every query are not read, and cache rows from past + S on are never read.
 * Keys are cut into fixed 64-key blocks, block c belongs to split c mod 4, a split visits its blocks in ascending order, a
 * query takes part in a block only if the block starts at or before its position, and the splits' (max, sum, P.V) are
 * merged in split order by the last workgroup of the (sequence, head) to finish (a ticket; no workgroup waits).  So the
 * output row of the query at absolute position P depends only on its q row, the head's K / V rows [0, P] and key_valid:
 * NOT on S, nor on the query's index in the launch — bit for bit.
 *   partials fp32 [B*heads*S*4*132]: scratch; arrivals uint32 [B*heads]: tickets, zero before the first launch and zero
 *   again after every completed one. */
int vly_spec_attention(const void *qkv, const void *kcache, const void *vcache, const uint8_t *key_valid, int key_valid_stride,
                       void *out, int B, int S, int heads, int past_len, const int32_t *past_len_dev, int ctx_max,
                       float *partials, uint32_t *arrivals, int dtype, void *stream);

/* HF's PromptLookupCandidateGenerator.get_candidates for one sequence, over hist int32 [ctx_max] with
 * len = (len_dev ? len_dev[0] : 0) + len_add known tokens (clamped to [1, ctx_max]); columns [len, ctx_max) are never read.
 *   For n = min(max_ngram, len - 1) down to 1: the SMALLEST i in [0, len - n) with hist[i .. i+n) == hist[len-n .. len);
 *   the first n with a match decides.  The draft is hist[i+n .. min(i+n+k, len)), cropped in front of the first token that
 *   is one of eos int32 [n_eos] (NULL / 0: none) or lies outside [0, vocab) (vocab <= 0: only negative ids); if the crop
 *   leaves nothing the draft is empty and nothing else is searched.  No match gives an empty draft.  draft_len is capped at
 *   ctx_max - len, so that the verify step's last position stays inside the cache.
 *   1 <= k <= 7, 1 <= max_ngram <= 8.
 *   draft int32 [k] (entries behind draft_len = hist[len-1], a valid id), draft_len int32 [1],
 *   tok int32 [k+1] = hist[len-1] followed by draft.
 *   lookup == 0: no search; draft / draft_len are the caller's and are left as they are, tok is built from them
 *   (draft_len read as clamped to [0, min(k, ctx_max - len)]).
 * One workgroup of 1024 threads; the earliest match is a block-wide minimum; no atomics. */
int vly_spec_draft(const int32_t *hist, int ctx_max, const int32_t *len_dev, int len_add, int k, int max_ngram, const int32_t *eos,
                   int n_eos, int vocab, int lookup, int32_t *draft, int32_t *draft_len, int32_t *tok, void *stream);

/* Behind vly_argmax over the k + 1 logit rows (am int32 [k+1]: the argmax, or the seeded draws): with pos = pos_dev[0], n = the number of leading
 * i < dl with draft[i] == am[i], where dl = draft_len[0] clamped to [0, min(k, ctx_max - (pos + 1))] — vly_spec_draft's
 * clamp, so only rows that were fed a draft are compared.  Then:
 *   hist[pos+1 .. pos+n+1] = am[0 .. n] (only the columns inside [0, ctx_max)),
 *   emit int32 [k+2] = (n + 1, am[0 .. n], -1 ...), tok[0] = am[n], stats int32 [3] += (1, dl, n),
 *   pos_dev[0] = pos + n + 1.
 * Plain stores from one workgroup. */
int vly_spec_accept(const int32_t *am, const int32_t *draft, const int32_t *draft_len, int k, int32_t *hist, int ctx_max,
                    int32_t *pos_dev, int32_t *emit, int32_t *tok, int32_t *stats, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VALLEY_HIP_SPEC_H */
