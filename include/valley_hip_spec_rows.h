/*
 * valley_hip_spec_rows.h — C ABI of libvalley_hip_spec_rows.so, the gfx950 kernels of prompt-lookup speculative decoding for
 * SEVERAL sequences in one verify step: B sequences of S = k + 1 rows each, every sequence at its own position, with its own
 * history, draft and acceptance count.  The per-sequence twins of valley_hip_spec.h's entries (and of vly_rope_kv and
 * vly_spec_counters), for the captured step of a continuous batcher.
 *
 * A companion of libvalley_hip.so / libvalley_hip_f16.so; valley_hip_spec.h's and valley_hip_spec_sample.h's entries, signatures
 * and ABI versions are unchanged by it.  One build serves both 16-bit storage types through the `dtype` code of
 * vly_storage_dtype (0: bf16, 1: IEEE fp16).  Conventions as in valley_hip_spec.h: device pointers owned by the caller, nothing
 * allocated, `stream` is a hipStream_t passed as void*, 0 on success, -22 (EINVAL) on bad arguments (message in
 * vly_spec_rows_last_error(), thread-local), -(1000 + hipError_t) if a launch failed.  Every value that changes from one step to
 * the next is read on the device.
 *
 * Positions.  pos_rows is a device int32 [B]: one position per sequence, p_b = pos_rows[b] clamped to [0, ctx_max - 1].  Row j
 * of sequence b sits at absolute position p_b + j.  A row with p_b + j >= ctx_max is DEAD: it writes nothing to the cache, the
 * history or any other sequence's data, its outputs are unspecified but finite, and nothing it does reads or writes outside the
 * buffers.  (The single-sequence kernels clamp the position to ctx_max - S instead, which would overwrite real rows of a
 * sequence near the end of its cache; with dead rows a sequence decodes its last positions inside the same step, one token at
 * a time.)
 */
#ifndef VALLEY_HIP_SPEC_ROWS_H
#define VALLEY_HIP_SPEC_ROWS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VLY_SPEC_ROWS_ABI_VERSION 1
#define VLY_SPEC_ROWS_MAX_QUERIES 8 /* S = k + 1 */
#define VLY_SPEC_ROWS_MAX_DRAFT 7   /* k */
#define VLY_SPEC_ROWS_MAX_NGRAM 8
#define VLY_SPEC_ROWS_SPLITS 4      /* = VLY_SPEC_SPLITS */
#define VLY_SPEC_ROWS_PARTIAL 132   /* = VLY_SPEC_PARTIAL */

int vly_spec_rows_abi_version(void);
const char *vly_spec_rows_last_error(void);

/* Rotate-half RoPE of q and k of qkv 16-bit [B*S, 3*heads*128] (head_dim 128) and the KV append, per sequence: q is rotated in
 * place, the rotated k and v go to row p_b + j of sequence b in kcache / vcache 16-bit [B, heads, ctx_max, 128].
 * cos / sin fp32 [>= ctx_max, 64] as vly_rope_kv takes them.  For every live row the bits of the rotated q and of the cache row
 * equal what vly_rope_kv(B = 1, S, past_len = p_b) writes for that sequence.  A dead row is left as it is (q not rotated). */
int vly_spec_rows_rope_kv(void *qkv, void *kcache, void *vcache, const float *cos_table, const float *sin_table, int B, int S,
                          int heads, const int32_t *pos_rows, int ctx_max, int dtype, void *stream);

/* vly_spec_attention with past = p_b per sequence and kv_len = min(p_b + S, ctx_max): the same 64-key blocks (block c to split
 * c mod 4, ascending), the same merge by the last workgroup on a ticket, the same partials fp32 [B*heads*S*4*132], arrivals
 * uint32 [B*heads] (zero before the first launch, zero again after every completed one) and grid (heads, B, 4).
 *   key_valid uint8 [B, key_valid_stride >= ctx_max] or NULL.
 * The output row of the query at absolute position P depends only on its q row, the head's K / V rows [0, P] and key_valid — not
 * on S, B, the query's index or the other sequences' positions — and is bit for bit the row vly_spec_attention writes for that
 * position.  A dead row is computed as a query at the cache's last position. */
int vly_spec_rows_attention(const void *qkv, const void *kcache, const void *vcache, const uint8_t *key_valid, int key_valid_stride,
                            void *out, int B, int S, int heads, const int32_t *pos_rows, int ctx_max, float *partials,
                            uint32_t *arrivals, int dtype, void *stream);

/* vly_spec_draft's rule, independently per sequence: hist int32 [B, ctx_max], len_b = pos_rows[b] + len_add clamped to
 * [1, ctx_max], draft int32 [B, k], draft_len int32 [B], tok int32 [B, k+1]; the cap ctx_max - len_b applies per sequence.
 * eos / n_eos / vocab / lookup as in vly_spec_draft (lookup == 0: draft / draft_len are the caller's, tok is built from them).
 *   live uint8 [B] or NULL (all live): a sequence with live[b] == 0 gets draft_len[b] = 0 and tok[b, :] = 0; its draft row is
 *   left as it is.
 * One workgroup of 1024 threads per sequence; no atomics. */
int vly_spec_rows_draft(const int32_t *hist, int ctx_max, const int32_t *pos_rows, int len_add, const uint8_t *live, int B, int k,
                        int max_ngram, const int32_t *eos, int n_eos, int vocab, int lookup, int32_t *draft, int32_t *draft_len,
                        int32_t *tok, void *stream);

/* vly_spec_accept per sequence: am int32 [B*(k+1)], draft int32 [B, k], draft_len int32 [B], hist int32 [B, ctx_max],
 * emit int32 [B, k+2], tok int32 [B*(k+1)], stats int32 [B, 3].  With pos = pos_rows[b] and n_b the accepted drafts of b:
 *   hist[b, pos+1 .. pos+n_b+1] = am[b*(k+1) + 0 .. n_b] (columns inside [0, ctx_max) only),
 *   emit[b] = (n_b + 1, those tokens, -1 ...), tok[b*(k+1)] = am[b*(k+1) + n_b], stats[b] += (1, dl_b, n_b),
 *   pos_rows[b] = pos + n_b + 1.
 * A sequence with live[b] == 0 (live uint8 [B] or NULL: all live) gets emit[b, 0] = 0; its pos_rows[b], hist row, tok and stats
 * row are left untouched, so an idle slot stays where it is.  Plain stores, one thread per sequence. */
int vly_spec_rows_accept(const int32_t *am, const int32_t *draft, const int32_t *draft_len, const uint8_t *live, int B, int k,
                         int32_t *hist, int ctx_max, int32_t *pos_rows, int32_t *emit, int32_t *tok, int32_t *stats, void *stream);

/* ctr int32 [B*(k+1)]: ctr[b*(k+1) + j] = p_b + j — vly_spec_counters per sequence, for vly_argmax's per-row draw counters
 * (ctr_add = 1: row j draws the token of sequence index p_b + j + 1) under seeded sampling. */
int vly_spec_rows_counters(const int32_t *pos_rows, int B, int k, int ctx_max, int32_t *ctr, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VALLEY_HIP_SPEC_ROWS_H */
