// Classifier-free guidance on the device (include/valley_hip_guide.h; DESIGN.md "decode: classifier-free guidance"): the
// logits of a conditional row and of its unconditional partner are combined right behind the lm_head, in front of
// vly_logits_process, and behind the argmax / draw the unconditional row takes its conditional row's token.
//
// vly_guide_apply: one 1024-thread workgroup per row; a workgroup whose row is no valid conditional row returns at once.
// Two row reductions (row_lse of beam_rows.inc over each row: vly_logits_process's log-softmax bits) and one elementwise
// pass; rows up to 32 k wide hold both rows' values in registers (2 x 32 per thread), wider rows read them again from L2.
// Only the conditional row's workgroup writes the conditional row, and nobody writes an unconditional row: no hand-off.
//
// This unit is compiled into its own library and includes no storage-type header: nothing here depends on bf16 / fp16.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "companion_capi.hpp"
#include "../../include/valley_hip_guide.h"

namespace {

#include "beam_rows.inc"

constexpr int FOLLOW_THREADS = 256;

// row r's partner where (r, partner) is a valid pair with r in the role `mine` and the partner in the role `theirs`, else -1
BM_DEVICE int partner_of(const int32_t* __restrict__ rows, int R, int r, int mine, int theirs) {
    if (rows[4 * r] != mine) return -1;
    const int p = rows[4 * r + 1];
    if (p < 0 || p >= R || p == r) return -1;
    return rows[4 * p] == theirs ? p : -1;
}

template <bool REG>
__global__ void __launch_bounds__(ROW_THREADS) guide_kernel(float* __restrict__ logits, int ld, int V, int R,
                                                            const int32_t* __restrict__ rows) {
    __shared__ float red[16];
    const int tid = threadIdx.x, r = blockIdx.x;
    const int u = partner_of(rows, R, r, VLY_GUIDE_COND, VLY_GUIDE_UNCOND);
    if (u < 0) return;                                           // neutral, unconditional or malformed: neither read nor written
    const float scale = __int_as_float(rows[4 * r + 2]), log_beta = __int_as_float(rows[4 * r + 3]);
    float* xc = logits + (size_t)r * ld;
    const float* xu = logits + (size_t)u * ld;

    float cv[REG ? REG_J : 1], uv[REG ? REG_J : 1];
    if constexpr (REG) {
#pragma unroll
        for (int j = 0; j < REG_J; ++j) {
            const int i = j * ROW_THREADS + tid;
            cv[j] = i < V ? xc[i] : __builtin_nanf("");
            uv[j] = i < V ? xu[i] : __builtin_nanf("");
        }
    }
    // f(i, x_c[i], x_u[i]) over the thread's elements i = tid, tid + ROW_THREADS, ... (row_lse's order)
    auto visit = [&](auto&& f) {
        if constexpr (REG) {
#pragma unroll
            for (int j = 0; j < REG_J; ++j) {
                const int i = j * ROW_THREADS + tid;
                if (i < V) f(i, cv[j], uv[j]);
            }
        } else {
            for (int i = tid; i < V; i += ROW_THREADS) f(i, xc[i], xu[i]);
        }
    };
    float m_c, m_u;
    const float lse_c = row_lse([&](auto&& f) { visit([&](int i, float c, float) { f(i, c); }); }, red, m_c);
    const float lse_u = row_lse([&](auto&& f) { visit([&](int i, float, float w) { f(i, w); }); }, red, m_u);
    const bool cut = log_beta > -INFINITY;                       // (false for a NaN as well)
    const float floor_c = (m_c - lse_c) + log_beta;

    visit([&](int i, float c, float w) {
        // three separately rounded operations.  (__fmul_rn is an inlined plain product that carries its header's contraction
        // flag, and the compiler fuses it with the sum behind it into an FMA: plain operators under contract(off) do not)
#pragma clang fp contract(off)
        const float lc = c - lse_c;
        float o;
        if (c != c || c == -INFINITY) {
            o = -INFINITY;
        } else if (w != w || w == -INFINITY || scale == 1.0f) {
            o = lc;                                              // (a scale of 1: HF returns the log-softmax itself)
        } else {
            const float lu = w - lse_u;
            const float d = lc - lu;
            const float p = scale * d;
            o = p + lu;
            if (o != o) o = lc;
        }
        if (cut && lc < floor_c) o = -INFINITY;
        xc[i] = o;
    });
}

__global__ void __launch_bounds__(FOLLOW_THREADS) follow_kernel(int32_t* __restrict__ tok, int R, const int32_t* __restrict__ rows) {
    for (int r = threadIdx.x; r < R; r += FOLLOW_THREADS) {
        const int c = partner_of(rows, R, r, VLY_GUIDE_UNCOND, VLY_GUIDE_COND);
        if (c >= 0) tok[r] = tok[c];
    }
}

}  // namespace

VLY_COMPANION_CAPI(guide, VLY_GUIDE_ABI_VERSION)

extern "C" int vly_guide_apply(float* logits, int ld, int V, int R, const int32_t* rows, void* stream) {
    if (!logits || !rows || R <= 0 || R > 65535 || V <= 0 || V >= (1 << 24) || ld < V || ((uintptr_t)logits & 3) ||
        ((uintptr_t)rows & 3)) {
        set_error("vly_guide_apply: bad args R=%d V=%d ld=%d (0 < V < 2^24, ld >= V, 0 < R <= 65535, non-NULL logits / rows, "
                  "4-byte aligned)", R, V, ld);
        return -22;
    }
    if (V <= REG_J * ROW_THREADS)
        hipLaunchKernelGGL(guide_kernel<true>, dim3(R), dim3(ROW_THREADS), 0, (hipStream_t)stream, logits, ld, V, R, rows);
    else
        hipLaunchKernelGGL(guide_kernel<false>, dim3(R), dim3(ROW_THREADS), 0, (hipStream_t)stream, logits, ld, V, R, rows);
    return check_launch("vly_guide_apply");
}

extern "C" int vly_guide_follow(int32_t* tok, int R, const int32_t* rows, void* stream) {
    if (!tok || !rows || R <= 0 || R > 65535 || ((uintptr_t)tok & 3) || ((uintptr_t)rows & 3)) {
        set_error("vly_guide_follow: bad args R=%d (0 < R <= 65535, non-NULL tok / rows, 4-byte aligned)", R);
        return -22;
    }
    hipLaunchKernelGGL(follow_kernel, dim3(1), dim3(FOLLOW_THREADS), 0, (hipStream_t)stream, tok, R, rows);
    return check_launch("vly_guide_follow");
}
