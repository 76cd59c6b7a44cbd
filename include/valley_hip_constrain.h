/*
 * valley_hip_constrain.h — C ABI of libvalley_hip_constrain.so, the gfx950 kernel of the token constraints inside the
 * decode step: the processors of HF's generate() that MASK the vocabulary from token lists — bad words, suppressed and
 * begin-suppressed tokens, the forced EOS — and an allowed-sequence trie, the tensor form of prefix_allowed_tokens_fn for a
 * closed answer set.  transformers.generation.logits_process (NoBadWordsLogitsProcessor, PrefixConstrainedLogitsProcessor,
 * ForcedEOSTokenLogitsProcessor, SuppressTokensLogitsProcessor, SuppressTokensAtBeginLogitsProcessor, in
 * _get_logits_processor's order) is the specification.
 *
 * A companion of libvalley_hip.so / libvalley_hip_f16.so, independent of their 16-bit storage type: it reads fp32 logits
 * and int32 ids only, so one build serves the bf16, fp16 and fp32 engines.  Conventions as in valley_hip.h: device
 * pointers owned by the caller, nothing allocated, `stream` is a hipStream_t passed as void*, 0 on success, -22 (EINVAL)
 * on bad arguments (message in vly_constrain_last_error(), thread-local), -(1000 + hipError_t) if a launch failed.
 * Everything that changes from one decode step or one request to the next — the per-row parameters, the lengths, the
 * history and the CONTENTS of every table, their counts included — is read on the device, so the launch can live in a
 * captured graph and replay with new values; only pointers and capacities are fixed at capture.
 */
#ifndef VALLEY_HIP_CONSTRAIN_H
#define VALLEY_HIP_CONSTRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VLY_CONSTRAIN_ABI_VERSION 1
#define VLY_CONSTRAIN_MAX_WORD 64   /* tokens of one bad word */
#define VLY_CONSTRAIN_MAX_DEPTH 64  /* tokens of one allowed sequence: the trie walk's dependent steps */
#define VLY_CONSTRAIN_HEADER 16     /* int32 words in front of the tables' regions */

/* the bits of a row's flags */
#define VLY_CONSTRAIN_BAD_WORDS 1
#define VLY_CONSTRAIN_TRIE 2
#define VLY_CONSTRAIN_FORCED_EOS 4
#define VLY_CONSTRAIN_SUPPRESS 8
#define VLY_CONSTRAIN_BEGIN_SUPPRESS 16

int vly_constrain_abi_version(void);
const char *vly_constrain_last_error(void);

/* The constraints over the rows of logits fp32 [R, ld] (V <= ld, V <= 262144), in place; one 1024-thread workgroup per
 * row; the columns [V, ld) are never touched.
 *   rows int32 [R, 4] per row: { flags, begin, max_length, trie_root }.  begin: the prompt's length (HF's begin_index, and
 *     where the trie walk starts); max_length: the forced EOS acts at len == max_length - 1 (0 = off); trie_root: offset of
 *     the row's root node inside the trie region (-1 = no trie).
 *   hist int32 [R, hist_ld], len = (len_dev ? len_dev[len_per_row ? r : 0] : 0) + len_add clamped to hist_ld: the row's
 *     token ids and length, vly_logits_process's (which has appended the token fed to this step); only read here.
 *   tables int32 [tables_len]: a header of VLY_CONSTRAIN_HEADER words, then five regions.  Header:
 *       [0] n_eos   [1] n_suppress   [2] n_begin   [3] n_words                        (counts, read at every launch)
 *       [4] off_eos [5] off_suppress [6] off_begin [7] off_words [8] off_trie         (word offsets from tables[0])
 *       [9] cap_words [10] cap_trie                                                   (words of those two regions)
 *     eos / suppress / begin regions: that many token ids.
 *     words region: n_words pairs { start, L } (start in words from the region's begin, 1 <= L <= 64), then the words'
 *       tokens wherever the pairs point.
 *     trie region: nodes, addressed by their word offset p from the region's begin: { n, ends, n pairs { token, child p } }
 *       with the pairs sorted by token (no duplicates); ends != 0 where an allowed sequence ends at the node.  Several tries
 *       (one per batcher slot) live side by side; a row's trie_root picks its own.
 *     Every index formed from the tables' contents is checked against its region and tables_len before it is used: a
 *     malformed table masks more or less, it never reads outside [tables, tables + tables_len).
 * In order, for each row (x = its logits; ids outside [0, V) are skipped):
 *   1. flags & BAD_WORDS: a word [t] gives x[t] += -inf; a word w of L >= 2 tokens gives x[w[L-1]] += -inf iff L <= len and
 *      hist[len-L+1 .. len) == w[:L-1] (the whole row counts: prompt, left padding, placeholder ids);
 *   2. flags & TRIE and trie_root >= 0, unless rule 3 fires (it overwrites the row): walk from the root over
 *      hist[begin .. len); allowed = the node's child tokens, and every EOS id where the node ends a sequence; a leaf, a
 *      history that left the trie or len - begin > 64 allow the EOS ids only; every other id gets x + (-inf);
 *   3. flags & FORCED_EOS, max_length > 0 and len == max_length - 1: the whole row becomes -inf, then every EOS id 0;
 *   4. flags & SUPPRESS: the listed ids become -inf exactly;
 *   5. flags & BEGIN_SUPPRESS and len == begin: the begin list's ids become -inf exactly.
 * A logit no rule bans keeps its bits; a row none of whose rules is switched on is neither read nor written. */
int vly_constrain_apply(float *logits, int ld, int V, int R, const int32_t *rows, const int32_t *tables, int tables_len,
                        const int32_t *hist, int hist_ld, const int32_t *len_dev, int len_per_row, int len_add, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VALLEY_HIP_CONSTRAIN_H */
