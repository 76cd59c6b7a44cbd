// The draft and acceptance rules of a speculative verify step, shared by libvalley_hip_spec.so (spec.hip: one sequence) and
// libvalley_hip_spec_rows.so (spec_rows.hip: blockIdx.x / the loop index = the sequence).  Included inside the unit's anonymous
// namespace, behind common.hpp and <limits.h>.  Both functions see ONE sequence: the kernels form that sequence's pointers and its
// length, the per-sequence ones also skip an idle slot; the lookup rule, the crop and the end-of-cache cap live here alone.

constexpr int MAX_NGRAM = 8;                                     // = VLY_SPEC_MAX_NGRAM = VLY_SPEC_ROWS_MAX_NGRAM

// HF's prompt lookup for a block of 1024 threads over hist[0, len), 1 <= len <= ctx_max (clamped by the caller): draft[k],
// draft_len[0] and the verify step's tok[k + 1] (the last token, then the draft).  For each n-gram size, largest first, thread t
// tests the window starts t, t + 1024, ... in ascending order and keeps its first hit; the earliest hit of the block is a minimum
// over the waves' minima in ``red`` (the kernel's __shared__ int [16]; no atomics).
VLY_DEVICE void lookup_draft(const int32_t* __restrict__ hist, int ctx_max, int len, int k, int max_ngram, const int32_t* __restrict__ eos,
                             int n_eos, int vocab, int lookup, int32_t* __restrict__ draft, int32_t* __restrict__ draft_len,
                             int32_t* __restrict__ tok, int* red) {
    const int tid = threadIdx.x;
    const int last = hist[len - 1];
    const int cap = min(k, ctx_max - len);                       // the verify step's last real position stays inside the cache
    if (!lookup) {
        if (tid == 0) {
            const int dl = max(0, min(draft_len[0], cap));
            tok[0] = last;
            for (int i = 0; i < k; ++i) tok[1 + i] = i < dl ? draft[i] : last;
        }
        return;
    }
    int start = -1;                                              // first token of the continuation, -1: no match
    for (int n = min(max_ngram, len - 1); n >= 1; --n) {
        int tl[MAX_NGRAM];
#pragma unroll
        for (int d = 0; d < MAX_NGRAM; ++d) tl[d] = d < n ? hist[len - n + d] : 0;
        int best = INT_MAX;
        for (int i = tid; i < len - n; i += 1024) {              // i + n - 1 <= len - 2: columns from len on are never read
            bool m = true;
#pragma unroll
            for (int d = 0; d < MAX_NGRAM; ++d)
                if (d < n) m = m && hist[i + d] == tl[d];
            if (m) {
                best = i;
                break;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) best = min(best, __shfl_xor(best, off, 64));
        __syncthreads();                                         // red: the previous size's minima have been read
        if ((tid & 63) == 0) red[tid >> 6] = best;
        __syncthreads();
        best = red[0];
#pragma unroll
        for (int w = 1; w < 16; ++w) best = min(best, red[w]);
        if (best != INT_MAX) {                                   // (uniform) the first size with a match decides
            start = best + n;
            break;
        }
    }
    if (tid != 0) return;
    int dl = 0;
    if (start >= 0) {
        dl = min(start + k, len) - start;
        for (int j = 0; j < dl; ++j) {                           // cropped in front of the first EOS (or unusable id)
            const int t = hist[start + j];
            bool stop = t < 0 || (vocab > 0 && t >= vocab);
            for (int e = 0; e < n_eos; ++e) stop = stop || t == eos[e];
            if (stop) {
                dl = j;
                break;
            }
        }
        dl = min(dl, cap);
    }
    dl = max(dl, 0);
    tok[0] = last;
    for (int j = 0; j < k; ++j) {
        const int t = j < dl ? hist[start + j] : last;
        draft[j] = t;
        tok[1 + j] = t;
    }
    draft_len[0] = dl;
}

// One thread, behind the argmax (or draws) am[k + 1] of a sequence's rows: n = the leading drafts that equal them;
// hist[pos + 1 .. pos + n + 1] = am[0 .. n], emit[k + 2] = (n + 1, am[0 .. n], -1 ...), tok[0] = am[n], stats[3] += (1, draft_len, n),
// pos_dev[0] += n + 1.
VLY_DEVICE void lookup_accept(const int32_t* __restrict__ am, const int32_t* __restrict__ draft, const int32_t* __restrict__ draft_len, int k,
                              int32_t* __restrict__ hist, int ctx_max, int32_t* __restrict__ pos_dev, int32_t* __restrict__ emit,
                              int32_t* __restrict__ tok, int32_t* __restrict__ stats) {
    const int pos = pos_dev[0];
    // lookup_draft's cap (len = pos + 1): the rows behind it were fed the last token, not the draft, and are not compared
    const long room = (long)ctx_max - ((long)pos + 1);
    const int dl = (int)max(0L, min((long)min(draft_len[0], k), room));
    int n = 0;
    while (n < dl && draft[n] == am[n]) ++n;
    emit[0] = n + 1;
    for (int j = 0; j <= k; ++j) emit[1 + j] = j <= n ? am[j] : -1;
    for (int j = 0; j <= n; ++j) {
        const long c = (long)pos + 1 + j;
        if (c >= 0 && c < ctx_max) hist[c] = am[j];
    }
    tok[0] = am[n];
    stats[0] += 1;
    stats[1] += dl;
    stats[2] += n;
    pos_dev[0] = pos + n + 1;
}
