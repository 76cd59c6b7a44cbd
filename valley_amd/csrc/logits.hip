// HF's logits processors on the device (include/valley_hip_logits.h; DESIGN.md "decode: logits processors"): repetition
// penalty, no-repeat n-grams and the minimum-length EOS mask over fp32 logits, the token history of beam rows following
// their parents, and the beam candidates over processed scores (beam_rows.inc, shared with beam.hip).
//
// vly_logits_process: one 1024-thread workgroup per row, everything read on the device.  The row's history is walked
// once for the penalty: each distinct id sets one bit of an LDS bitmap of V bits, and the thread whose atomicOr set the
// bit rescales that logit, so a repeated id is penalised exactly once.  Then a barrier, the n-gram windows (one per
// thread, compared against the last n - 1 ids), a barrier, the EOS mask.
//
// This unit is compiled into its own library and includes no storage-type header: nothing here depends on bf16 / fp16.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "companion_capi.hpp"
#include "../../include/valley_hip_logits.h"

namespace {

#include "beam_rows.inc"

constexpr int PROC_MAX_V = 1 << 18;                 // the bitmap: V / 32 words of dynamic LDS, at most 32 KB

__global__ void __launch_bounds__(ROW_THREADS) logits_process_kernel(float* __restrict__ logits, int ld, int V,
                                                                     const int32_t* __restrict__ params, int32_t* hist,
                                                                     int hist_ld, const int32_t* __restrict__ len_dev,
                                                                     int len_per_row, int len_add, const int32_t* __restrict__ tok,
                                                                     const int32_t* __restrict__ eos, int n_eos, int log_softmax) {
    extern __shared__ uint32_t seen[];                           // (V + 31) / 32 words
    __shared__ float red[16];
    const int tid = threadIdx.x, r = blockIdx.x;
    float* x = logits + (size_t)r * ld;
    int32_t* h = hist + (size_t)r * hist_ld;
    const float pen = __int_as_float(params[4 * r]);
    const int n = params[4 * r + 1], min_len = params[4 * r + 2];
    int len = (len_dev ? len_dev[len_per_row ? r : 0] : 0) + len_add;
    len = len < hist_ld ? len : hist_ld;
    // the token fed to this step sits at len - 1: read from tok by every thread (no global write-then-read inside the
    // launch), stored into the history by thread 0 for the next step
    const bool append = tok != nullptr && len >= 1;
    const int32_t t_new = append ? tok[r] : 0;
    if (append && tid == 0) h[len - 1] = t_new;
    auto id_at = [&](int i) { return (append && i == len - 1) ? t_new : h[i]; };

    if (log_softmax) {                                           // beam search: the processors see log-probabilities
        const float lse = row_lse([&](auto&& f) { for (int i = tid; i < V; i += ROW_THREADS) f(i, x[i]); }, red);
        for (int i = tid; i < V; i += ROW_THREADS) x[i] = x[i] - lse;
        __syncthreads();                                         // (each x[i] is rewritten by the thread that owns i)
    }
    if (pen != 1.0f && len > 0) {
        const int words = (V + 31) >> 5;
        for (int w = tid; w < words; w += ROW_THREADS) seen[w] = 0u;
        __syncthreads();
        for (int i = tid; i < len; i += ROW_THREADS) {
            const int t = id_at(i);
            if ((unsigned)t < (unsigned)V) {
                const uint32_t b = 1u << (t & 31);
                if (!(atomicOr(&seen[t >> 5], b) & b)) {             // this thread set the bit: the one penalty of id t
                    const float s = x[t];
                    x[t] = s < 0.f ? s * pen : s / pen;
                }
            }
        }
    }
    __syncthreads();
    if (n > 0 && len >= n) {
        const int p0 = len - n + 1;                              // the prefix: the last n - 1 ids, [p0, len)
        for (int i = tid; i + n <= len; i += ROW_THREADS) {
            bool eq = true;
            for (int k = 0; k < n - 1 && eq; ++k) eq = id_at(i + k) == id_at(p0 + k);
            if (eq) {
                const int t = id_at(i + n - 1);
                if ((unsigned)t < (unsigned)V) x[t] = -INFINITY;
            }
        }
    }
    __syncthreads();
    if (len < min_len)
        for (int e = tid; e < n_eos; e += ROW_THREADS) {
            const int t = eos[e];
            if ((unsigned)t < (unsigned)V) x[t] = -INFINITY;
        }
}

constexpr int G_THREADS = 256;
constexpr int G_STAGE = 8192;                       // ids staged per workgroup: 32 KB of LDS
constexpr int G_POS = 64;                           // positions per workgroup while R <= 128; G_STAGE / R above
constexpr int G_MAX_R = G_STAGE;                    // (at least one position per workgroup)

// one workgroup per run of P positions: every row whose parent differs from itself <- its parent's row, over the run's
// part of [lo, hi); all source ids of the run are staged in LDS before any row is written
__global__ void __launch_bounds__(G_THREADS) history_gather_kernel(int32_t* __restrict__ hist, int R, int hist_ld,
                                                                   const int32_t* __restrict__ parent, int lo,
                                                                   const int32_t* __restrict__ len_dev, int hi_add, int P) {
    __shared__ int32_t stage[G_STAGE];
    const int tid = threadIdx.x;
    int hi = (len_dev ? len_dev[0] : 0) + hi_add;
    hi = hi < hist_ld ? hi : hist_ld;
    const int p0 = lo + blockIdx.x * P;
    if (p0 >= hi) return;
    const int np = hi - p0 < P ? hi - p0 : P, total = R * np;  // total <= G_STAGE: R * P <= G_STAGE on the host
    for (int e = tid; e < total; e += G_THREADS) {
        const int r = e / np, off = e - r * np;
        const int p = parent[r];
        if (p != r && p >= 0 && p < R) stage[e] = hist[(size_t)p * hist_ld + p0 + off];
    }
    __syncthreads();                                             // every source id is in LDS before any row is written
    for (int e = tid; e < total; e += G_THREADS) {
        const int r = e / np, off = e - r * np;
        const int p = parent[r];
        if (p != r && p >= 0 && p < R) hist[(size_t)r * hist_ld + p0 + off] = stage[e];
    }
}

}  // namespace

VLY_COMPANION_CAPI(logits, VLY_LOGITS_ABI_VERSION)

extern "C" int vly_logits_process(float* logits, int ld, int V, int R, const int32_t* params, int32_t* hist, int hist_ld,
                                  const int32_t* len_dev, int len_per_row, int len_add, const int32_t* tok, const int32_t* eos,
                                  int n_eos, int log_softmax, void* stream) {
    if (!logits || !params || !hist || R <= 0 || R > 65535 || V <= 0 || V > PROC_MAX_V || ld < V || hist_ld <= 0 ||
        (len_per_row && !len_dev) || n_eos < 0 || (n_eos > 0 && !eos) || ((uintptr_t)logits & 3) || ((uintptr_t)params & 3) ||
        ((uintptr_t)hist & 3) || ((uintptr_t)len_dev & 3) || ((uintptr_t)tok & 3) || ((uintptr_t)eos & 3)) {
        set_error("vly_logits_process: bad args R=%d V=%d ld=%d hist_ld=%d len_per_row=%d n_eos=%d (0 < V <= 262144, ld >= V, "
                  "R <= 65535, non-NULL logits / params / hist, len_dev with len_per_row, 4-byte aligned)", R, V, ld, hist_ld,
                  len_per_row, n_eos);
        return -22;
    }
    const size_t lds = (size_t)((V + 31) >> 5) * sizeof(uint32_t);
    hipLaunchKernelGGL(logits_process_kernel, dim3(R), dim3(ROW_THREADS), lds, (hipStream_t)stream, logits, ld, V, params, hist,
                       hist_ld, len_dev, len_per_row, len_add, tok, eos, n_eos, log_softmax);
    return check_launch("vly_logits_process");
}

extern "C" int vly_logits_history_gather(int32_t* hist, int R, int hist_ld, const int32_t* parent, int lo, const int32_t* len_dev,
                                         int hi_add, void* stream) {
    if (!hist || !parent || R <= 0 || R > G_MAX_R || hist_ld <= 0 || lo < 0 || ((uintptr_t)hist & 3) || ((uintptr_t)parent & 3) ||
        ((uintptr_t)len_dev & 3)) {
        set_error("vly_logits_history_gather: bad args R=%d hist_ld=%d lo=%d (0 < R <= 8192, lo >= 0, non-NULL hist / parent)", R,
                  hist_ld, lo);
        return -22;
    }
    if (lo >= hist_ld || (!len_dev && hi_add <= lo)) return 0;
    const int P = R <= G_STAGE / G_POS ? G_POS : G_STAGE / R;
    hipLaunchKernelGGL(history_gather_kernel, dim3((hist_ld - lo + P - 1) / P), dim3(G_THREADS), 0, (hipStream_t)stream, hist, R,
                       hist_ld, parent, lo, len_dev, hi_add, P);
    return check_launch("vly_logits_history_gather");
}

extern "C" size_t vly_logits_beam_scratch_bytes(int B, int nb, int K) { return beam_scratch_bytes(B, nb, K); }

extern "C" int vly_logits_beam_candidates(const float* scores, int ld, int V, int B, int nb, const float* running, int K,
                                          const int32_t* eos, int n_eos, void* scratch, float* score, int32_t* token,
                                          int32_t* beam, uint8_t* hit, void* stream) {
    if (!beam_rows_args_ok(scores, ld, V, B, nb, running, K, eos, n_eos, scratch, score, token, beam, hit)) {
        set_error("vly_logits_beam_candidates: bad args B=%d nb=%d K=%d V=%d ld=%d n_eos=%d (nb <= 16, nb <= K <= 64, "
                  "K <= V < 2^24, scratch 256-byte aligned)", B, nb, K, V, ld, n_eos);
        return -22;
    }
    launch_beam_rows<false>(scores, ld, V, B, nb, running, K, eos, n_eos, scratch, score, token, beam, hit, (hipStream_t)stream);
    return check_launch("vly_logits_beam_candidates");
}
