// Token constraints on the device (include/valley_hip_constrain.h; DESIGN.md "decode: token constraints"): HF's bad words,
// forced EOS, suppressed and begin-suppressed tokens and an allowed-sequence trie over fp32 logits, behind
// vly_logits_process in the decode step.
//
// vly_constrain_apply: one 1024-thread workgroup per row, everything read on the device — the row's parameters, its
// length, the tables' counts and contents.  Bad words: one word per thread (as many passes as the count needs), each
// compared against the tail of the row's history.  The trie: wave 0 walks it, stateless, from the root over the generated
// ids — the ids sit one per lane, a node's sorted { token, child } pairs are searched 64 at a time with a ballot (one
// dependent load per step while a node has at most 64 children, a 64-ary descent above) — and leaves the node in LDS; the
// workgroup then sets one bit per allowed id in an LDS bitmap of V bits and masks every id whose bit is clear.
//
// This unit is compiled into its own library and includes no storage-type header: nothing here depends on bf16 / fp16.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "companion_capi.hpp"
#include "../../include/valley_hip_constrain.h"

namespace {

constexpr int THREADS = 1024;
constexpr int MAX_V = 1 << 18;                      // the bitmap: V / 32 words of dynamic LDS, at most 32 KB
constexpr int HEADER = VLY_CONSTRAIN_HEADER;

__global__ void __launch_bounds__(THREADS) constrain_kernel(float* __restrict__ logits, int ld, int V,
                                                            const int32_t* __restrict__ rows, const int32_t* __restrict__ tab,
                                                            int tlen, const int32_t* __restrict__ hist, int hist_ld,
                                                            const int32_t* __restrict__ len_dev, int len_per_row, int len_add) {
    extern __shared__ uint32_t allow[];                          // (V + 31) / 32 words
    __shared__ int s_node;
    const int tid = threadIdx.x, r = blockIdx.x;
    const int flags = rows[4 * r], begin0 = rows[4 * r + 1], max_len = rows[4 * r + 2], root = rows[4 * r + 3];
    const bool trie_on = (flags & VLY_CONSTRAIN_TRIE) && root >= 0;
    const bool forced_on = (flags & VLY_CONSTRAIN_FORCED_EOS) && max_len > 0;
    if (!(flags & (VLY_CONSTRAIN_BAD_WORDS | VLY_CONSTRAIN_SUPPRESS | VLY_CONSTRAIN_BEGIN_SUPPRESS)) && !trie_on && !forced_on)
        return;                                                  // a neutral row: neither read nor written
    float* x = logits + (size_t)r * ld;
    const int32_t* h = hist + (size_t)r * hist_ld;
    int len = (len_dev ? len_dev[len_per_row ? r : 0] : 0) + len_add;
    len = len < hist_ld ? len : hist_ld;
    len = len > 0 ? len : 0;

    // every read of the tables goes through here: an index outside [0, tlen) reads as -1, which no rule takes for an id
    auto at = [&](long i) -> int { return (i >= 0 && i < (long)tlen) ? tab[i] : -1; };
    auto count = [&](int n, int off) { return (off < HEADER || n < 0) ? 0 : (n < tlen ? n : tlen); };
    const int off_eos = tab[4], off_sup = tab[5], off_beg = tab[6], off_words = tab[7], off_trie = tab[8];
    const int n_eos = count(tab[0], off_eos), n_sup = count(tab[1], off_sup), n_beg = count(tab[2], off_beg);
    const int cap_words = count(tab[9], off_words), cap_trie = count(tab[10], off_trie);
    const int n_words = tab[3] < 0 ? 0 : (tab[3] < cap_words / 2 ? tab[3] : cap_words / 2);
    const bool fire = forced_on && len == max_len - 1;           // rule 3 overwrites the row: rules 1 and 2 are skipped then

    if ((flags & VLY_CONSTRAIN_BAD_WORDS) && !fire) {
        auto word = [&](int i) { return at((long)off_words + i); };
        for (int w = tid; w < n_words; w += THREADS) {
            const int st = word(2 * w), L = word(2 * w + 1);
            if (L < 1 || L > VLY_CONSTRAIN_MAX_WORD || st < 0 || st > cap_words - L) continue;
            const int last = word(st + L - 1);
            if ((unsigned)last >= (unsigned)V) continue;
            bool hit = true;
            if (L > 1) {
                hit = L <= len;                                  // (HF: a word longer than the context is ignored)
                const int p0 = len - L + 1;
                for (int k = 0; hit && k < L - 1; ++k) hit = h[p0 + k] == word(st + k);
            }
            // several words may ban one id: -inf added once or twice is the same value, whatever the interleaving
            if (hit) x[last] = x[last] + (-INFINITY);
        }
    }
    __syncthreads();

    if (trie_on && !fire) {
        auto node = [&](int i) { return i < cap_trie ? at((long)off_trie + i) : -1; };
        const int words32 = (V + 31) >> 5;
        for (int w = tid; w < words32; w += THREADS) allow[w] = 0u;
        if (tid < 64) {                                          // wave 0 walks; every quantity below is uniform over it
            const int lane = tid;
            const int begin = begin0 < 0 ? 0 : (begin0 < len ? begin0 : len);
            const int depth = len - begin;
            int p = (depth <= VLY_CONSTRAIN_MAX_DEPTH && root <= cap_trie - 2) ? root : -1;
            const int hv = (p >= 0 && lane < depth) ? h[begin + lane] : -1;
            for (int i = 0; i < depth && p >= 0; ++i) {
                const int t = __shfl(hv, i);
                const int n = node(p);
                if (n < 0 || n > (cap_trie - p - 2) / 2) {       // a malformed node: out of the trie
                    p = -1;
                    break;
                }
                int lo = 0, hi = n;
                while (hi - lo > 64) {                           // 64-ary descent: lane l probes the end of the l-th part
                    const int stride = (hi - lo + 63) >> 6;
                    int idx = lo + (lane + 1) * stride - 1;
                    idx = idx < hi ? idx : hi - 1;
                    const unsigned long long m = __ballot(node(p + 2 + 2 * idx) >= t);
                    if (!m) {
                        lo = hi;
                        break;
                    }
                    const int f = __ffsll((long long)m) - 1;
                    lo += f * stride;
                    hi = lo + stride < hi ? lo + stride : hi;
                }
                const int idx = lo + lane;
                int tk = -2, ch = -1;
                if (idx < hi) {
                    tk = node(p + 2 + 2 * idx);
                    ch = node(p + 3 + 2 * idx);
                }
                const unsigned long long m = __ballot(idx < hi && tk == t);
                const int child = m ? __shfl(ch, __ffsll((long long)m) - 1) : -1;
                p = (child >= 0 && child <= cap_trie - 2) ? child : -1;
            }
            if (lane == 0) s_node = p;
        }
        __syncthreads();
        const int p = s_node;                                    // -1: only the EOS ids are allowed
        int n = p >= 0 ? node(p) : 0;
        n = (n < 0 || p < 0 || n > (cap_trie - p - 2) / 2) ? 0 : n;
        const bool ends = p < 0 || node(p + 1) != 0 || n == 0;
        for (int c = tid; c < n; c += THREADS) {
            const int t = node(p + 2 + 2 * c);
            if ((unsigned)t < (unsigned)V) atomicOr(&allow[t >> 5], 1u << (t & 31));
        }
        if (ends)
            for (int e = tid; e < n_eos; e += THREADS) {
                const int t = at((long)off_eos + e);
                if ((unsigned)t < (unsigned)V) atomicOr(&allow[t >> 5], 1u << (t & 31));
            }
        __syncthreads();
        for (int i = tid; i < V; i += THREADS)
            if (!((allow[i >> 5] >> (i & 31)) & 1u)) x[i] = x[i] + (-INFINITY);
    }
    __syncthreads();

    if (fire) {
        for (int i = tid; i < V; i += THREADS) x[i] = -INFINITY;
        __syncthreads();
        for (int e = tid; e < n_eos; e += THREADS) {
            const int t = at((long)off_eos + e);
            if ((unsigned)t < (unsigned)V) x[t] = 0.f;
        }
    }
    __syncthreads();

    if (flags & VLY_CONSTRAIN_SUPPRESS)
        for (int e = tid; e < n_sup; e += THREADS) {
            const int t = at((long)off_sup + e);
            if ((unsigned)t < (unsigned)V) x[t] = -INFINITY;
        }
    if ((flags & VLY_CONSTRAIN_BEGIN_SUPPRESS) && len == begin0)
        for (int e = tid; e < n_beg; e += THREADS) {
            const int t = at((long)off_beg + e);
            if ((unsigned)t < (unsigned)V) x[t] = -INFINITY;
        }
}

}  // namespace

VLY_COMPANION_CAPI(constrain, VLY_CONSTRAIN_ABI_VERSION)

extern "C" int vly_constrain_apply(float* logits, int ld, int V, int R, const int32_t* rows, const int32_t* tables, int tables_len,
                                   const int32_t* hist, int hist_ld, const int32_t* len_dev, int len_per_row, int len_add,
                                   void* stream) {
    if (!logits || !rows || !tables || !hist || R <= 0 || R > 65535 || V <= 0 || V > MAX_V || ld < V || hist_ld <= 0 ||
        tables_len < HEADER || (len_per_row && !len_dev) || ((uintptr_t)logits & 3) || ((uintptr_t)rows & 3) ||
        ((uintptr_t)tables & 3) || ((uintptr_t)hist & 3) || ((uintptr_t)len_dev & 3)) {
        set_error("vly_constrain_apply: bad args R=%d V=%d ld=%d hist_ld=%d tables_len=%d len_per_row=%d (0 < V <= 262144, "
                  "ld >= V, R <= 65535, tables_len >= 16, non-NULL logits / rows / tables / hist, len_dev with len_per_row, "
                  "4-byte aligned)", R, V, ld, hist_ld, tables_len, len_per_row);
        return -22;
    }
    const size_t lds = (size_t)((V + 31) >> 5) * sizeof(uint32_t);
    hipLaunchKernelGGL(constrain_kernel, dim3(R), dim3(THREADS), lds, (hipStream_t)stream, logits, ld, V, rows, tables,
                       tables_len, hist, hist_ld, len_dev, len_per_row, len_add);
    return check_launch("vly_constrain_apply");
}
