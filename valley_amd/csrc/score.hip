// Token log-probabilities on the device (include/valley_hip_score.h; DESIGN.md §4.9 "Token log-probabilities and the
// forward-only loss"): the log-softmax of a chosen token, the n most probable alternatives, the decode step's per-token
// record, and the forward-only cross-entropy.
//
// vly_score_rows: one 1024-thread workgroup per row.  The log-sum-exp is beam_rows.inc's row_lse, visited in its documented
// order, so a row's lse has the bits vly_logits_process(log_softmax = 1) and vly_beam_candidates compute for it.  The top-n
// (n <= 20) is n rounds of a block-wide maximum over 64-bit keys (order-preserving value key, then the complemented index:
// ties go to the lower index), each round taking the largest key below the previous round's.  Rows up to 32768 wide are held
// in registers (one read of the row); wider rows are streamed again by every pass.
//
// This unit is compiled into its own library and includes no storage-type header: nothing here depends on bf16 / fp16.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "companion_capi.hpp"
#include "../../include/valley_hip_score.h"

namespace {

#include "beam_rows.inc"

constexpr int SCORE_MAX_V = 1 << 18;
constexpr int SCORE_MAX_R = 1 << 24;

// fixed order (lanes by xor tree, waves in index order); the maximum does not depend on it anyway
BM_DEVICE uint64_t block_max_u64(uint64_t v, uint64_t* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t hi = __shfl_xor((uint32_t)(v >> 32), o, 64), lo = __shfl_xor((uint32_t)v, o, 64);
        const uint64_t u = ((uint64_t)hi << 32) | lo;
        v = u > v ? u : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t m = red[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) m = red[w] > m ? red[w] : m;
    return m;
}

template <bool REG>
__global__ void __launch_bounds__(ROW_THREADS) score_rows_kernel(const float* __restrict__ logits, int ld, int V,
                                                                 const int32_t* __restrict__ target, float* __restrict__ target_lp,
                                                                 float* __restrict__ lse_out, int n_top, int32_t* __restrict__ top_id,
                                                                 float* __restrict__ top_lp, float* __restrict__ copy, int copy_ld) {
    __shared__ float red[16];
    __shared__ uint64_t red64[16];
    const int tid = threadIdx.x, r = blockIdx.x;
    const float* x = logits + (size_t)r * ld;

    float xv[REG ? REG_J : 1];
    if constexpr (REG) {
#pragma unroll
        for (int j = 0; j < REG_J; ++j) {
            const int i = j * ROW_THREADS + tid;
            xv[j] = i < V ? x[i] : __builtin_nanf("");
        }
    }
    // f(i, x_i) over the thread's elements i = tid, tid + ROW_THREADS, ...: row_lse's visiting order in both forms
    auto visit_x = [&](auto&& f) {
        if constexpr (REG) {
#pragma unroll
            for (int j = 0; j < REG_J; ++j) {
                const int i = j * ROW_THREADS + tid;
                if (i < V) f(i, xv[j]);
            }
        } else {
            for (int i = tid; i < V; i += ROW_THREADS) f(i, x[i]);
        }
    };
    const float lse = row_lse(visit_x, red);
    if (tid == 0) {
        if (lse_out) lse_out[r] = lse;
        if (target_lp) {
            const int t = target[r];
            target_lp[r] = (unsigned)t < (unsigned)V ? x[t] - lse : 0.f;
        }
    }
    if (copy) {
        float* c = copy + (size_t)r * copy_ld;
        visit_x([&](int i, float v) { c[i] = v; });
    }
    // round k: the largest (value key, ~index) strictly below round k - 1's; a NaN's value key is 0 and never enters
    uint64_t prev = ~0ull;
    for (int k = 0; k < n_top; ++k) {
        uint64_t best = 0ull;
        visit_x([&](int i, float v) {
            const uint32_t key = okey(v);
            const uint64_t c = ((uint64_t)key << 32) | (0xffffffffu - (uint32_t)i);
            if (key != 0u && c < prev && c > best) best = c;
        });
        best = block_max_u64(best, red64);
        if (tid == 0) {
            const size_t o = (size_t)r * n_top + k;
            if (best >> 32) {
                const int id = (int)(0xffffffffu - (uint32_t)best);
                top_id[o] = id;
                top_lp[o] = x[id] - lse;
            } else {
                top_id[o] = -1;
                top_lp[o] = -INFINITY;
            }
        }
        prev = best;                                             // 0 once the row is exhausted: every later round finds nothing
    }
}

constexpr int REC_THREADS = 64;

__global__ void __launch_bounds__(REC_THREADS) score_record_kernel(const float* __restrict__ raw, int raw_ld, int V,
                                                                   const float* __restrict__ lse, const int32_t* __restrict__ tok,
                                                                   const int32_t* __restrict__ len_dev, int len_per_row, int len_add,
                                                                   float* __restrict__ lp_table, int table_ld, int n_top,
                                                                   const int32_t* __restrict__ top_id, const float* __restrict__ top_lp,
                                                                   int32_t* __restrict__ top_id_table, float* __restrict__ top_lp_table) {
    const int tid = threadIdx.x, r = blockIdx.x;
    const int c = (len_dev ? len_dev[len_per_row ? r : 0] : 0) + len_add;
    if (c < 0 || c >= table_ld) return;
    const size_t cell = (size_t)r * table_ld + c;
    if (tid == 0) {
        const int t = tok[r];
        lp_table[cell] = (unsigned)t < (unsigned)V ? raw[(size_t)r * raw_ld + t] - lse[r] : 0.f;
    }
    if (tid < n_top) {
        top_id_table[cell * n_top + tid] = top_id[(size_t)r * n_top + tid];
        top_lp_table[cell * n_top + tid] = top_lp[(size_t)r * n_top + tid];
    }
}

constexpr int LOSS_THREADS = 1024;

__global__ void __launch_bounds__(LOSS_THREADS) score_loss_kernel(const float* __restrict__ target_lp, const int32_t* __restrict__ target,
                                                                  int M, int V, float* __restrict__ loss, int32_t* __restrict__ count) {
    __shared__ double ssum[LOSS_THREADS];
    __shared__ int32_t scnt[LOSS_THREADS];
    const int tid = threadIdx.x;
    double s = 0.0;
    int32_t n = 0;
    for (int i = tid; i < M; i += LOSS_THREADS)
        if ((unsigned)target[i] < (unsigned)V) {
            s += (double)target_lp[i];
            ++n;
        }
    ssum[tid] = s;
    scnt[tid] = n;
    __syncthreads();
    for (int h = LOSS_THREADS / 2; h > 0; h >>= 1) {             // binary tree: the same order at every launch
        if (tid < h) {
            ssum[tid] += ssum[tid + h];
            scnt[tid] += scnt[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        count[0] = scnt[0];
        loss[0] = scnt[0] > 0 ? (float)(-ssum[0] / (double)scnt[0]) : __builtin_nanf("");
    }
}

}  // namespace

VLY_COMPANION_CAPI(score, VLY_SCORE_ABI_VERSION)

extern "C" int vly_score_rows(const float* logits, int ld, int V, int R, const int32_t* target, float* target_lp, float* lse, int n_top,
                              int32_t* top_id, float* top_lp, float* copy, int copy_ld, void* stream) {
    if (!logits || R <= 0 || R > SCORE_MAX_R || V <= 0 || V > SCORE_MAX_V || ld < V || (target == nullptr) != (target_lp == nullptr) ||
        n_top < 0 || n_top > VLY_SCORE_MAX_TOP || (n_top > 0 && (!top_id || !top_lp)) || (copy && copy_ld < V) ||
        ((uintptr_t)logits & 3) || ((uintptr_t)target & 3) || ((uintptr_t)target_lp & 3) || ((uintptr_t)lse & 3) ||
        ((uintptr_t)top_id & 3) || ((uintptr_t)top_lp & 3) || ((uintptr_t)copy & 3)) {
        set_error("vly_score_rows: bad args R=%d V=%d ld=%d n_top=%d copy_ld=%d (0 < V <= 262144, ld >= V, 0 < R <= 2^24, "
                  "0 <= n_top <= 20 with top_id / top_lp, target with target_lp, copy_ld >= V, non-NULL logits, 4-byte aligned)",
                  R, V, ld, n_top, copy_ld);
        return -22;
    }
    if (V <= REG_J * ROW_THREADS)
        hipLaunchKernelGGL(score_rows_kernel<true>, dim3(R), dim3(ROW_THREADS), 0, (hipStream_t)stream, logits, ld, V, target,
                           target_lp, lse, n_top, top_id, top_lp, copy, copy_ld);
    else
        hipLaunchKernelGGL(score_rows_kernel<false>, dim3(R), dim3(ROW_THREADS), 0, (hipStream_t)stream, logits, ld, V, target,
                           target_lp, lse, n_top, top_id, top_lp, copy, copy_ld);
    return check_launch("vly_score_rows");
}

extern "C" int vly_score_record(const float* raw, int raw_ld, int V, int R, const float* lse, const int32_t* tok, const int32_t* len_dev,
                                int len_per_row, int len_add, float* lp_table, int table_ld, int n_top, const int32_t* top_id,
                                const float* top_lp, int32_t* top_id_table, float* top_lp_table, void* stream) {
    if (!raw || !lse || !tok || !lp_table || R <= 0 || R > SCORE_MAX_R || V <= 0 || V > SCORE_MAX_V || raw_ld < V || table_ld <= 0 ||
        (len_per_row && !len_dev) || n_top < 0 || n_top > VLY_SCORE_MAX_TOP ||
        (n_top > 0 && (!top_id || !top_lp || !top_id_table || !top_lp_table)) || ((uintptr_t)raw & 3) || ((uintptr_t)lse & 3) ||
        ((uintptr_t)tok & 3) || ((uintptr_t)len_dev & 3) || ((uintptr_t)lp_table & 3) || ((uintptr_t)top_id & 3) ||
        ((uintptr_t)top_lp & 3) || ((uintptr_t)top_id_table & 3) || ((uintptr_t)top_lp_table & 3)) {
        set_error("vly_score_record: bad args R=%d V=%d raw_ld=%d table_ld=%d len_per_row=%d n_top=%d (0 < V <= 262144, raw_ld >= V, "
                  "table_ld > 0, non-NULL raw / lse / tok / lp_table, len_dev with len_per_row, 0 <= n_top <= 20 with the four top "
                  "pointers, 4-byte aligned)", R, V, raw_ld, table_ld, len_per_row, n_top);
        return -22;
    }
    hipLaunchKernelGGL(score_record_kernel, dim3(R), dim3(REC_THREADS), 0, (hipStream_t)stream, raw, raw_ld, V, lse, tok, len_dev,
                       len_per_row, len_add, lp_table, table_ld, n_top, top_id, top_lp, top_id_table, top_lp_table);
    return check_launch("vly_score_record");
}

extern "C" int vly_score_loss(const float* target_lp, const int32_t* target, int M, int V, float* loss, int32_t* count, void* stream) {
    if (!target_lp || !target || !loss || !count || M <= 0 || V <= 0 || ((uintptr_t)target_lp & 3) || ((uintptr_t)target & 3) ||
        ((uintptr_t)loss & 3) || ((uintptr_t)count & 3)) {
        set_error("vly_score_loss: bad args M=%d V=%d (M > 0, V > 0, non-NULL target_lp / target / loss / count, 4-byte aligned)", M, V);
        return -22;
    }
    hipLaunchKernelGGL(score_loss_kernel, dim3(1), dim3(LOSS_THREADS), 0, (hipStream_t)stream, target_lp, target, M, V, loss, count);
    return check_launch("vly_score_loss");
}
