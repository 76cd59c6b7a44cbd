// Beam search on the device (include/valley_hip_beam.h; DESIGN.md "decode: beam search"): the top-K continuations of
// every prompt, the running beams of the next step, and the in-place reorder of the KV cache rows.
//
// Row top-K and merge: beam_rows.inc (shared with logits.hip), here over log_softmax(logits) + the beam's running score.
//
// This unit is compiled into its own library and includes no storage-type header: nothing here depends on bf16 / fp16.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "companion_capi.hpp"
#include "../../include/valley_hip_beam.h"

namespace {

#include "beam_rows.inc"

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

// one 64-thread workgroup per prompt: the nb best of v = score + hit * (-1e9), stable in candidate order
__global__ void __launch_bounds__(64) beam_select_kernel(const float* __restrict__ score, const int32_t* __restrict__ token,
                                                         const int32_t* __restrict__ beam, const uint8_t* __restrict__ hit,
                                                         int nb, int K, int32_t* __restrict__ tok, int32_t* __restrict__ parent,
                                                         float* __restrict__ running) {
    __shared__ uint32_t vk[MAX_K];
    const int b = blockIdx.x, t = threadIdx.x;
    float v = 0.f;
    if (t < K) {
        v = score[b * K + t] + (float)hit[b * K + t] * -1.0e9f;
        vk[t] = okey(v);
    }
    __syncthreads();
    if (t >= K) return;
    const uint32_t k = vk[t];
    int rank = 0;
    for (int j = 0; j < K; ++j) rank += (vk[j] > k || (vk[j] == k && j < t)) ? 1 : 0;
    if (rank < nb) {
        const int o = b * nb + rank;
        tok[o] = token[b * K + t];
        parent[o] = beam[b * K + t];
        running[o] = v;
    }
}

constexpr int RO_THREADS = 256;
constexpr int RO_VECS = 2048;                       // 32 KB of LDS staging: 16-byte vectors
constexpr int RO_MAX_R = 128;

// one workgroup per (head, layer, K | V): row dst[c] <- row src[c] of that slab over [lo, hi), a run of positions at a time
__global__ void __launch_bounds__(RO_THREADS) kv_reorder_kernel(const int64_t* __restrict__ table, int R, int heads, int ctx_max,
                                                                int vpp, const int32_t* __restrict__ parent, int lo,
                                                                const int32_t* __restrict__ pos_dev, int hi_add) {
    __shared__ u32x4 stage[RO_VECS];
    __shared__ int dst[RO_MAX_R], src[RO_MAX_R];
    __shared__ int nch;
    const int tid = threadIdx.x;
    const int h = blockIdx.x, l = blockIdx.y >> 1, which = blockIdx.y & 1;
    int hi = (pos_dev ? pos_dev[0] : 0) + hi_add;
    hi = hi < ctx_max ? hi : ctx_max;
    if (hi <= lo) return;
    if (tid == 0) {
        int n = 0;
        for (int r = 0; r < R; ++r) {
            const int p = parent[r];
            if (p != r && p >= 0 && p < R) { dst[n] = r; src[n] = p; ++n; }
        }
        nch = n;
    }
    __syncthreads();
    const int n = nch;
    if (n == 0) return;
    u32x4* base = (u32x4*)table[2 * l + which];
    const int P = RO_VECS / (n * vpp);                           // positions per run (>= 1: checked on the host)
    for (int p0 = lo; p0 < hi; p0 += P) {
        const int np = hi - p0 < P ? hi - p0 : P;
        const int per = np * vpp, total = n * per;               // a row's run is contiguous: per vectors
        for (int e = tid; e < total; e += RO_THREADS) {
            const int c = e / per, off = e - c * per;
            stage[e] = base[((size_t)src[c] * heads + h) * ctx_max * vpp + (size_t)p0 * vpp + off];
        }
        __syncthreads();                                         // every source vector is in LDS before any row is written
        for (int e = tid; e < total; e += RO_THREADS) {
            const int c = e / per, off = e - c * per;
            base[((size_t)dst[c] * heads + h) * ctx_max * vpp + (size_t)p0 * vpp + off] = stage[e];
        }
        __syncthreads();
    }
}

}  // namespace

VLY_COMPANION_CAPI(beam, VLY_BEAM_ABI_VERSION)

extern "C" size_t vly_beam_scratch_bytes(int B, int nb, int K) { return beam_scratch_bytes(B, nb, K); }

extern "C" int vly_beam_candidates(const float* logits, int ld, int V, int B, int nb, const float* running, int K,
                                   const int32_t* eos, int n_eos, void* scratch, float* score, int32_t* token, int32_t* beam,
                                   uint8_t* hit, void* stream) {
    if (!beam_rows_args_ok(logits, ld, V, B, nb, running, K, eos, n_eos, scratch, score, token, beam, hit)) {
        set_error("vly_beam_candidates: bad args B=%d nb=%d K=%d V=%d ld=%d n_eos=%d (nb <= 16, nb <= K <= 64, K <= V < 2^24, "
                  "scratch 256-byte aligned)", B, nb, K, V, ld, n_eos);
        return -22;
    }
    launch_beam_rows<true>(logits, ld, V, B, nb, running, K, eos, n_eos, scratch, score, token, beam, hit, (hipStream_t)stream);
    return check_launch("vly_beam_candidates");
}

extern "C" int vly_beam_select(const float* score, const int32_t* token, const int32_t* beam, const uint8_t* hit, int B, int nb,
                               int K, int32_t* tok, int32_t* parent, float* running, void* stream) {
    if (!score || !token || !beam || !hit || !tok || !parent || !running || B <= 0 || nb <= 0 || nb > MAX_NB || K < nb ||
        K > MAX_K) {
        set_error("vly_beam_select: bad args B=%d nb=%d K=%d (nb <= 16, nb <= K <= 64)", B, nb, K);
        return -22;
    }
    hipLaunchKernelGGL(beam_select_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, score, token, beam, hit, nb, K, tok, parent,
                       running);
    return check_launch("vly_beam_select");
}

extern "C" int vly_kv_beam_reorder(const int64_t* table, int L, int R, int heads, int ctx_max, int elem_bytes,
                                   const int32_t* parent, int lo, const int32_t* pos_dev, int hi_add, void* stream) {
    if (!table || !parent || L <= 0 || R <= 0 || R > RO_MAX_R || heads <= 0 || heads > 65535 || ctx_max <= 0 ||
        (elem_bytes != 2 && elem_bytes != 4) || R * 128 * elem_bytes > RO_VECS * 16 || lo < 0 || (2 * L) > 65535 ||
        ((uintptr_t)table & 7) || ((uintptr_t)parent & 3) || ((uintptr_t)pos_dev & 3)) {
        set_error("vly_kv_beam_reorder: bad args L=%d R=%d heads=%d ctx_max=%d elem_bytes=%d lo=%d (elem_bytes 2 | 4, "
                  "R * 128 * elem_bytes <= 32768)", L, R, heads, ctx_max, elem_bytes, lo);
        return -22;
    }
    if (!pos_dev && hi_add <= lo) return 0;
    hipLaunchKernelGGL(kv_reorder_kernel, dim3(heads, 2 * L), dim3(RO_THREADS), 0, (hipStream_t)stream, table, R, heads, ctx_max,
                       128 * elem_bytes / 16, parent, lo, pos_dev, hi_add);
    return check_launch("vly_kv_beam_reorder");
}
