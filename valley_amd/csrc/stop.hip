// The end of a generation decided on the device (include/valley_hip_stop.h):
// behind the argmax / draw a row finishes on an EOS id or when HF's StopStringCriteria fires on the row's last tokens, and a
// finished row's tokens become its pad id.  The verdict lands in device memory, so the host may replay n steps and look once.
//
// vly_stop_apply: one 64-thread workgroup (one wave) per row.  The ids of the up to 63 tokens in front of the newest one and
// their lengths are fetched first, one per lane (their addresses do not depend on a chain's running length), then every lane
// walks one (string, end overlap) chain over them out of LDS; a chain's only global loads are the valid positions it compares.
//
// This unit is compiled into its own library and includes no storage-type header: it reads and writes int32 only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "companion_capi.hpp"
#include "../../include/valley_hip_stop.h"

namespace {

constexpr int THREADS = 64;

__global__ void __launch_bounds__(THREADS) stop_kernel(int32_t* __restrict__ tok, const int32_t* __restrict__ hist, int ld,
                                                       const int32_t* __restrict__ pos, int per_row, int pos_add,
                                                       const int32_t* __restrict__ rows, int32_t* __restrict__ state,
                                                       const int32_t* __restrict__ tables, int table_words,
                                                       const int32_t* __restrict__ eos, int n_eos) {
    __shared__ int s_row[VLY_STOP_MAX_LEN];                      // table row of the j-th token in front of the newest one
    __shared__ int s_len[VLY_STOP_MAX_LEN];                      // ... and its length
    __shared__ int s_hit;
    const int r = blockIdx.x, lane = threadIdx.x;
    const int flags = rows[4 * r];
    if (!(flags & VLY_STOP_WATCH)) return;
    if (state[2 * r] != 0) {                                     // finished before this token: only the pad rule is left
        if ((flags & VLY_STOP_PAD_AFTER) && lane == 0) tok[r] = rows[4 * r + 2];
        return;
    }
    const long long p = (long long)(pos ? pos[per_row ? r : 0] : 0) + pos_add;
    const int t = tok[r];
    if (lane == 0) s_hit = 0;
    __syncthreads();                                             // the word is cleared before any lane may set it
    bool hit = false;
    for (int i = lane; i < n_eos; i += THREADS) hit |= eos[i] == t;

    // the header describes a table inside [0, table_words), or the string test is off (every value is the workgroup's)
    const int ns = tables[0], mvp = tables[1], mvel = tables[2], mtl = tables[3], T = tables[4], W = tables[5];
    const bool ok = ns >= 1 && ns <= VLY_STOP_MAX_STRINGS && mvp >= 0 && mvel >= 1 && mtl >= 1 && mtl <= VLY_STOP_MAX_LEN &&
                    W >= 1 && W <= VLY_STOP_MAX_WIDTH && (long long)ns * ((long long)mvp + mvel) + 1 == W && T >= 1 &&
                    VLY_STOP_HEADER + (long long)T * W <= table_words;
    if (ok) {
        const int32_t* __restrict__ emb = tables + VLY_STOP_HEADER;
        auto row_of = [&](int id) { return id < 0 || id >= T - 1 ? T - 1 : id; };
        // the tokens in front of the newest one, newest first: indices p, p - 1, ... down to max(begin, 0, p + 2 - mtl)
        int n_prev = 0;
        if (p >= 0 && p < ld) {
            long long lo = rows[4 * r + 1];
            lo = lo < 0 ? 0 : lo;
            lo = lo < p + 2 - mtl ? p + 2 - mtl : lo;
            n_prev = lo <= p ? (int)(p - lo + 1) : 0;            // <= mtl - 1 <= 63
        }
        for (int j = lane; j < n_prev; j += THREADS) {
            const int row = row_of(hist[(size_t)r * ld + (size_t)(p - j)]);
            s_row[j] = row;
            s_len[j] = emb[(size_t)row * W + W - 1];
        }
        __syncthreads();
        const int tr = row_of(t);
        for (int c = lane; c < ns * mvel; c += THREADS) {
            const int s = c / mvel;
            const int target = tables[8 + s];
            int cum = emb[(size_t)tr * W + ns * mvp + c];        // the newest token's end overlap of this chain
            if (cum <= 0) continue;
            bool fired = cum >= target;
            for (int j = 0; j < n_prev && !fired; ++j) {
                const int32_t* __restrict__ vp = emb + (size_t)s_row[j] * W + s * mvp;
                bool match = false;
                for (int q = 0; q < mvp; ++q) match |= vp[q] == cum;
                if (!match) break;
                cum = (int)((unsigned)cum + (unsigned)s_len[j]);
                fired = cum >= target;
            }
            hit |= fired;
        }
    }
    if (hit) atomicOr(&s_hit, 1);
    __syncthreads();
    if (lane == 0 && s_hit) {
        state[2 * r] = 1;
        state[2 * r + 1] = (int)(p + 1);
    }
}

}  // namespace

VLY_COMPANION_CAPI(stop, VLY_STOP_ABI_VERSION)

extern "C" int vly_stop_apply(int32_t* tok, const int32_t* hist, int ld, const int32_t* pos, int per_row, int pos_add,
                              const int32_t* rows, int32_t* state, const int32_t* tables, int table_words, const int32_t* eos,
                              int n_eos, int R, void* stream) {
    if (!tok || !hist || !rows || !state || !tables || R <= 0 || R > 65535 || ld < 1 || table_words < VLY_STOP_HEADER ||
        n_eos < 0 || n_eos > 64 || (n_eos > 0 && !eos) || (per_row && !pos) ||
        (((uintptr_t)tok | (uintptr_t)hist | (uintptr_t)pos | (uintptr_t)rows | (uintptr_t)state | (uintptr_t)tables |
          (uintptr_t)eos) & 3)) {
        set_error("vly_stop_apply: bad args R=%d ld=%d table_words=%d n_eos=%d (0 < R <= 65535, ld >= 1, table_words >= %d, "
                  "0 <= n_eos <= 64 with eos, non-NULL tok / hist / rows / state / tables, pos for per_row, 4-byte aligned)",
                  R, ld, table_words, n_eos, VLY_STOP_HEADER);
        return -22;
    }
    hipLaunchKernelGGL(stop_kernel, dim3(R), dim3(THREADS), 0, (hipStream_t)stream, tok, hist, ld, pos, per_row ? 1 : 0, pos_add,
                       rows, state, tables, table_words, n_eos ? eos : nullptr, n_eos);
    return check_launch("vly_stop_apply");
}
