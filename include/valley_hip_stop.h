/*
 * valley_hip_stop.h — C ABI of libvalley_hip_stop.so, the gfx950 kernel that decides inside the decode step whether a row's
 * generation is over: an EOS id, or a stop string at the end of the row's tokens.  The stop-string test is
 * transformers.generation.stopping_criteria.StopStringCriteria.__call__ (HF's generate(stop_strings=, tokenizer=)), whose
 * per-token int32 table the host builds once; the verdict is a function of the last few token ids alone, so it runs behind
 * the argmax / draw over the history the logits processors keep, and the host may replay several steps before it looks.
 *
 * A companion of libvalley_hip.so / libvalley_hip_f16.so, independent of their 16-bit storage type: it reads int32 only, so
 * one build serves the bf16, fp16, int8 and int4 engines.  Conventions as in valley_hip.h: device pointers owned by the
 * caller, nothing allocated, `stream` is a hipStream_t passed as void*, 0 on success, -22 (EINVAL) on bad arguments (message
 * in vly_stop_last_error(), thread-local), -(1000 + hipError_t) if a launch failed.
 * Every per-row value, the position, the EOS ids and the stop tables with their dimensions are read on the device, so a
 * launch can live in a captured graph and replay with new rows, a cleared state and other stop strings; only the pointers,
 * ld, table_words, n_eos and R are fixed at capture.
 */
#ifndef VALLEY_HIP_STOP_H
#define VALLEY_HIP_STOP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VLY_STOP_ABI_VERSION 1

#define VLY_STOP_MAX_STRINGS 8    /* stop strings of one table */
#define VLY_STOP_MAX_LEN 64       /* characters (bytes in HF's byte modes) of a stop string = tokens walked */
#define VLY_STOP_MAX_WIDTH 1024   /* ints of one table row */
#define VLY_STOP_HEADER 16        /* ints in front of the table rows */

/* bits of a row's flags */
#define VLY_STOP_WATCH 1          /* the row is tested */
#define VLY_STOP_PAD_AFTER 2      /* once finished, the row's chosen tokens are overwritten with its pad id */

int vly_stop_abi_version(void);
const char *vly_stop_last_error(void);

/* Behind the argmax / draw over tok int32 [R], one 64-thread workgroup per row r:
 *   hist int32 [R, ld]: the row's token history; p = pos[per_row ? r : 0] + pos_add (pos NULL: p = pos_add) is the index of
 *     its last valid entry, and tok[r] is the token of index p + 1 in the row's sequence.
 *   rows int32 [R, 4] per row: { flags, begin, pad id, reserved }.
 *   state int32 [R, 2] per row: { finished (0 / 1), end }: end is the index in the row's sequence of the token that finished
 *     the row, -1 before that (the caller clears a row to { 0, -1 }).
 *   tables int32 [table_words]: { n strings, max_valid_positions, max_valid_end_lens, maximum_token_len, T, W, 0, 0,
 *     target_lens[8] } and then HF's embedding_vec [T, W], W = n * (max_valid_positions + max_valid_end_lens) + 1: per token
 *     id and string its valid positions, its possible end overlaps, and last the token's length; row T - 1 is all -1.
 *   eos int32 [n_eos] (NULL with n_eos = 0: no EOS rule).
 * A row without VLY_STOP_WATCH touches nothing.  A watched row that has finished: with VLY_STOP_PAD_AFTER tok[r] = pad,
 * nothing else.  Otherwise the row finishes — state[r] = { 1, p + 1 } — if tok[r] is one of eos, or if the stop-string test
 * fires on the ids hist[r][max(begin, p + 2 - maximum_token_len) .. p] followed by tok[r]: for every string s and every end
 * overlap e > 0 of the newest token, the chain starts at the length e and goes back one token at a time; it survives a
 * token while its length is one of that token's valid positions for s, and then grows by the token's length; the test fires
 * as soon as a surviving chain reaches target_lens[s].  An id outside [0, T - 1) uses row T - 1 (HF's clamp).
 * Whatever the tables and rows hold, hist is read inside [max(begin, 0), min(p, ld - 1)] of its own row only and the tables
 * inside [0, table_words): a p outside [0, ld) walks no history, a header that does not describe a table inside table_words
 * (or names more than 8 strings, 64 tokens, 1024 ints a row) switches the string test off; such values change verdicts,
 * never which memory is touched.  A row's result does not depend on its index or on its neighbours.
 * R <= 65535, ld >= 1, table_words >= VLY_STOP_HEADER, 0 <= n_eos <= 64. */
int vly_stop_apply(int32_t *tok, const int32_t *hist, int ld, const int32_t *pos, int per_row, int pos_add,
                   const int32_t *rows, int32_t *state, const int32_t *tables, int table_words, const int32_t *eos,
                   int n_eos, int R, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VALLEY_HIP_STOP_H */
