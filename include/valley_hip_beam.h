/*
 * valley_hip_beam.h — C ABI of libvalley_hip_beam.so, the gfx950 kernels of beam search: the per-step selection of the
 * best continuations across the beams of a prompt, and the reorder of the KV cache that makes every beam row follow its
 * parent.  HF `generate(num_beams > 1)` (transformers generation/utils.py `_beam_search`) is the specification.
 *
 * A companion of libvalley_hip.so / libvalley_hip_f16.so, independent of their 16-bit storage type: the selection kernels
 * read fp32 logits and int32 indices, the reorder copies opaque 2- or 4-byte elements.  One build serves the bf16 and fp16
 * libraries and the fp32 engine's caches.  Conventions as in valley_hip.h: device pointers owned by the caller, nothing
 * allocated, `stream` is a hipStream_t passed as void*, 0 on success, -22 (EINVAL) on bad arguments (message in
 * vly_beam_last_error(), thread-local), -(1000 + hipError_t) if a launch failed.  Every argument that changes from one
 * decode step to the next is read on the device, so the three launches can live in a captured graph.
 *
 * Notation: B prompts, nb beams per prompt (nb <= 16), R = B * nb rows; row r = b * nb + j is beam j of prompt b.
 * K = max(2, 1 + n_eos) * nb candidates per prompt (HF's beams_to_keep), K <= 64.
 */
#ifndef VALLEY_HIP_BEAM_H
#define VALLEY_HIP_BEAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VLY_BEAM_ABI_VERSION 1

int vly_beam_abi_version(void);
const char *vly_beam_last_error(void);

/* Bytes of the device scratch vly_beam_candidates needs for (B, nb, K).  Zero it once when it is allocated: it holds a
 * ticket counter per prompt, which every launch leaves at zero. */
size_t vly_beam_scratch_bytes(int B, int nb, int K);

/* The top K continuations of every prompt, best first (HF _get_top_k_continuations, not sampled):
 *   acc[r, t] = log_softmax(logits[r, :V])[t] + running[r] in fp32, with lse = m + log(sum exp(x - m)) over the row's
 *   non-NaN logits, and acc = (x - lse) + running[r];
 *   per prompt, the K largest acc over its nb * V values, ties broken by the lower flat index j * V + t.  NaN logits
 *   are never selected while K others exist; -inf is allowed.  A NaN acc ranks below -inf: a prompt with fewer than K
 *   non-NaN values fills the rest of its K with NaN entries in flat-index order, their score a NaN (bits 0xffffffff).
 *   -0 and +0 are one value (a tie, reported as +0).
 * logits fp32 [R, ld] (ld >= V >= K), running fp32 [R], eos int32 [n_eos] (NULL when n_eos == 0).
 * Outputs [B * K]: score fp32, token int32, beam int32 (the ABSOLUTE parent row b * nb + j), hit uint8 (token in eos).
 * One 1024-thread workgroup per row finds the row's top K (radix descent over an order-preserving key); the last
 * workgroup of a prompt to finish merges the nb sorted lists (ticket counter in the scratch). */
int vly_beam_candidates(const float *logits, int ld, int V, int B, int nb, const float *running, int K, const int32_t *eos,
                        int n_eos, void *scratch, float *score, int32_t *token, int32_t *beam, uint8_t *hit, void *stream);

/* The running beams of the next step (HF _get_running_beams_for_next_iteration): per prompt, the nb best of
 * v = score + hit * (-1e9) over its K candidates, stable in candidate order.  hit may come from vly_beam_candidates
 * (EOS) or from the host (any stopping criterion).  Outputs [R]: tok int32 (the token fed to the next step), parent
 * int32 (absolute row), running fp32 (= v). */
int vly_beam_select(const float *score, const int32_t *token, const int32_t *beam, const uint8_t *hit, int B, int nb, int K,
                    int32_t *tok, int32_t *parent, float *running, void *stream);

/* In place, for every layer l < L and both caches: row r <- row parent[r] over positions [lo, hi) of the
 * [R, heads, ctx_max, 128] caches whose base pointers are table[l][0] (K) and table[l][1] (V) (int64 [L, 2], device).
 * hi = (pos_dev ? *pos_dev : 0) + hi_add, clamped to ctx_max, read on the device.  elem_bytes is 2 or 4; 16-byte
 * aligned bases.  Rows with parent[r] == r are neither read (as destinations) nor written, and a row whose parent lies
 * outside [0, R) (-1, R, ...) is left alone in the same way.  Any parent map is correct
 * (swaps, cycles, many-to-one): one workgroup owns a (layer, K | V, head) slab of every row and stages the source rows
 * of a run of positions in LDS before it writes any of them.  Copies are 16-byte vectors: bit-exact.
 * R * 128 * elem_bytes <= 32768 (R <= 128 for 2-byte, 64 for 4-byte elements). */
int vly_kv_beam_reorder(const int64_t *table, int L, int R, int heads, int ctx_max, int elem_bytes, const int32_t *parent,
                        int lo, const int32_t *pos_dev, int hi_add, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VALLEY_HIP_BEAM_H */
