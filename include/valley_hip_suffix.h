/*
 * valley_hip_suffix.h — C ABI of libvalley_hip_suffix.so: causal attention of a SHORT run of new queries (1..64) over a long
 * cached prefix, split over the keys.  The shape of a conversation's next turn: 10-60 new tokens over the hundreds of keys the
 * earlier turns (and the video) left in the KV cache.
 *
 * vly_llama_attention gives such a launch ONE workgroup per (sequence, head), which walks every 64-key tile in turn with all
 * eight waves multiplying, also the waves whose query rows lie behind S.  Here a (sequence, head) is `splits` workgroups of
 * four waves, each over a contiguous range of tiles, and a wave without queries multiplies nothing.
 *
 * A companion of libvalley_hip.so / libvalley_hip_f16.so.  One build serves both 16-bit storage types (`dtype`: the code of
 * vly_storage_dtype, 0 bf16, 1 IEEE fp16).  Conventions as in valley_hip_spec.h: device pointers owned by the caller, nothing
 * allocated, `stream` is a hipStream_t passed as void*, 0 on success, -22 (EINVAL) on bad arguments (message in
 * vly_suffix_last_error(), thread-local), -(1000 + hipError_t) if the launch failed.
 */
#ifndef VALLEY_HIP_SUFFIX_H
#define VALLEY_HIP_SUFFIX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VLY_SUFFIX_ABI_VERSION 1
#define VLY_SUFFIX_MAX_QUERIES 64 /* S: four waves x 16 query rows */
#define VLY_SUFFIX_PARTIAL 132    /* fp32 per (sequence, head, query, split): m, l, 2 unused, o[128] */

/* The split rule, a pure function of kv_len = past + S:
 *     tiles  = ceil(kv_len / 64)
 *     splits = min(VLY_SUFFIX_MAX_SPLITS, ceil(tiles / VLY_SUFFIX_TILES_PER_SPLIT))
 * and split s walks the tiles [s * tiles / splits, (s + 1) * tiles / splits) in ascending order (integer division: contiguous
 * ranges whose lengths differ by at most one).  The two constants come from the measurement in profiles/r13/prefix_ab.jsonl
 * (tools/prefix_ab.py; README "Conversation KV reuse"). */
#ifndef VLY_SUFFIX_TILES_PER_SPLIT
#define VLY_SUFFIX_TILES_PER_SPLIT 8
#endif
#define VLY_SUFFIX_MAX_SPLITS 16

int vly_suffix_abi_version(void);
const char *vly_suffix_last_error(void);

/* Bytes of `scratch` for a launch of B sequences x S queries x heads: the fp32 partials
 * [B * heads * S * VLY_SUFFIX_MAX_SPLITS * VLY_SUFFIX_PARTIAL] followed by the uint32 ticket counters [B * heads].  The caller
 * zeroes the buffer ONCE; every completed launch leaves the counters at zero again.  0 for arguments out of range. */
size_t vly_suffix_scratch_bytes(int B, int S, int heads);

/* What vly_llama_attention computes for the same arguments, head_dim 128:
 *   qkv 16-bit [B*S, 3*heads*128] with the ROTATED q in its first third (what vly_gemm_qkv_rope / vly_rope_kv leave; the rest
 *   is not read); kcache / vcache 16-bit [B, heads, ctx_max, 128] with the rows [past, past + S) already appended — read only;
 *   out 16-bit [B*S, heads*128].
 *   1 <= S <= 64, past >= 0, past + S <= ctx_max.  A non-NULL past_dev[0], clamped to [0, ctx_max - S], replaces past.
 *   key_valid uint8 [B, key_valid_stride] (key_valid_stride >= past + S; >= ctx_max with past_dev) or NULL.
 * Query i sees key j iff j <= past + i and key_valid[b][j] != 0.  Cache rows from past + S on are never read.
 *
 * Grid (heads, B, splits), four waves per workgroup: wave w owns the queries 16w .. 16w + 15, a wave with 16w >= S stages
 * tiles and multiplies nothing, a tile wholly in a wave's future is skipped.  Scores and P.V run on v_mfma_f32_16x16x32 with
 * llama_attn2_kernel's fragments (K is the A operand of S^T; P is packed to 16 bits in the B position of the second product),
 * the online softmax is fp32 with exp2, masked keys score NEG_BIG.  K / V tiles arrive by LDS-DMA into a double buffer.  Each
 * split leaves (m, l, o[128]) in fp32 per query; the last workgroup of a (sequence, head) to arrive (a ticket; nobody waits)
 * merges them in split order with weights exp2(m_s - m), one reciprocal, one rounding.  A split in which a query sees no key
 * has m_s = NEG_BIG and merges with weight exactly 0.  With ONE split (kv_len <= 64 x VLY_SUFFIX_TILES_PER_SPLIT) the
 * workgroup writes its rows itself — the bits the merge of one partial gives — and scratch is not touched.  The same inputs
 * give the same bits. */
int vly_suffix_attention(const void *qkv, const void *kcache, const void *vcache, const uint8_t *key_valid,
                         int key_valid_stride, void *out, int B, int S, int heads, int past, const int32_t *past_dev,
                         int ctx_max, int dtype /* 0 bf16, 1 fp16 */, void *scratch, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* VALLEY_HIP_SUFFIX_H */
