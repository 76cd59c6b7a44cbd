// Token selection over rows of fp32 logits [M,N] (row stride ld >= N): the greedy argmax of the decode step and seeded
// sampling with temperature, top-k and top-p (vly_argmax with a vly_sample_row per row; DESIGN.md "decode: sampling").
//
// A sampled row follows HF's warper order: s = l / T (IEEE division), top-k keeps s >= the k-th largest s (ties at the
// boundary kept), top-p keeps token t iff the softmax mass of the kept tokens strictly above s_t is < p, and the draw is
// Gumbel-max, argmax over kept i of s_i - log(-log(u_i)) (first index on ties), which samples softmax(filtered s) exactly.
// u_i comes from counter-based Philox4x32-10: key (seed_lo, seed_hi), counter (i >> 2, ctr, 0, 0), word i & 3, so a
// request's stream depends on (seed, ctr, logits) only — not on its batch row, its neighbours or graph vs eager launch.
//
// One 1024-thread workgroup per row.  The top-k value and the top-p threshold are found by radix descent on the
// order-preserving uint32 key of s: four 8-bit digits, each a pass over the row into a 256-bin LDS histogram of counts
// and (top-p) of fixed-point mass exp(s - max) * 2^40 as uint64 — integer sums, so the result does not depend on the
// order in which the atomics land.  Rows up to SMP_REG_N wide are held in registers (32 values per thread); wider rows
// are re-read from global memory (L2-resident) by every pass.
#include "common.hpp"
#include "../../include/valley_hip.h"

namespace {

VLY_DEVICE bool first_max_better(float v, int i, float best, int bi) { return v > best || (v == best && i < bi); }

// block-wide (best value, first index) reduction of 1024 threads; the result is valid in thread 0.  When no thread took an
// element (every value NaN, or nothing selectable) the index is 0, never the 0x7fffffff the threads start from: the token
// goes straight into the next step's embedding gather.
VLY_DEVICE int block_first_max(float best, int bi, float* sv, int* si) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (first_max_better(ov, oi, best, bi)) { best = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w)
            if (first_max_better(sv[w], si[w], best, bi)) { best = sv[w]; bi = si[w]; }
    }
    return bi == 0x7fffffff ? 0 : bi;
}

// first maximal index of one row (torch.argmax tie rule on CPU; NaN is never selected, an all-NaN row gives 0); valid in
// thread 0.  16-byte loads
// issued four at a time (a 256-thread scalar loop spent 39 us per 32 k-wide row on dependent load latency: 0.7 % of a
// 13B decode step).
VLY_DEVICE int argmax_row(const float* __restrict__ r, int N, float* sv, int* si) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
    auto take = [&](float v, int i) {
        if (v > best || (v == best && i < bi)) { best = v; bi = i; }
    };
    const int tid = threadIdx.x;
    if ((((uintptr_t)r) & 15) == 0) {
        const int nv = N >> 2;
        for (int c0 = 0; c0 < nv; c0 += 4096) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * 1024 + tid;
                v[u] = c < nv ? ((const float4*)r)[c] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * 1024 + tid;
                if (c >= nv) continue;                      // an absent slot's -inf must not be taken: its index is not the row's
                const int i = c * 4;
                take(v[u].x, i); take(v[u].y, i + 1); take(v[u].z, i + 2); take(v[u].w, i + 3);
            }
        }
        for (int i = (nv << 2) + tid; i < N; i += 1024) take(r[i], i);
    } else {
        for (int i = tid; i < N; i += 1024) take(r[i], i);
    }
    return block_first_max(best, bi, sv, si);
}

// argmax over rows of fp32 [M,N]; one 1024-thread workgroup per row (the NULL-parameter path of vly_argmax)
__global__ void __launch_bounds__(1024) argmax_kernel(const float* __restrict__ x, int32_t* __restrict__ idx, int N, int ld) {
    __shared__ float sv[16];
    __shared__ int si[16];
    const int bi = argmax_row(x + (size_t)blockIdx.x * ld, N, sv, si);
    if (threadIdx.x == 0) idx[blockIdx.x] = bi;
}

// ---- sampling -------------------------------------------------------------------------------------------------------

constexpr int SMP_GROUPS = 8;                       // register-resident groups of 4 consecutive values per thread
constexpr int SMP_REG_N = SMP_GROUPS * 4 * 1024;    // rows up to 32768 wide stay in registers
constexpr int HCOPIES = 4;                          // histogram copies (wave & 3) to spread the atomics of hot bins

typedef unsigned long long u64;

// order-preserving key of a float; -0 and +0 share a key; NaN (and an absent element) is 0, below every real value
VLY_DEVICE uint32_t okey(float s) {
    if (s != s) return 0u;
    const uint32_t u = __float_as_uint(s + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
VLY_DEVICE float okey_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// Philox4x32-10 (Salmon et al., SC'11; Random123's constants): the four output words of counter (c0, c1, 0, 0), key (k0, k1)
VLY_DEVICE u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1) {
    uint32_t c2 = 0u, c3 = 0u;
#pragma unroll
    for (int rnd = 0; rnd < 10; ++rnd) {
        if (rnd) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    }
    u32x4 o;
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
    return o;
}

// Gumbel noise of one Philox word: u = (2 * (x >> 9) + 1) * 2^-24 lies strictly inside (0, 1) and is exact in fp32
VLY_DEVICE float gumbel(uint32_t x) {
    const float u = (float)(2u * (x >> 9) + 1u) * 0x1p-24f;
    return -logf(-logf(u));
}

struct SampleLds {
    uint32_t cnt[HCOPIES][256];
    u64 mass[HCOPIES][256];
    uint32_t tcnt[256];
    u64 tmass[256];
    uint32_t ukey[16];
    float sv[16];
    int si[16];
    uint32_t digit, status, rem;
    u64 base;
};

template <bool REG>
__global__ void __launch_bounds__(1024) sample_kernel(const float* __restrict__ x, int32_t* __restrict__ idx, int N, int ld,
                                                      const vly_sample_row* __restrict__ rows, const int32_t* __restrict__ ctr,
                                                      int ctr_per_row, int ctr_add) {
    __shared__ SampleLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* r = x + (size_t)blockIdx.x * ld;
    const vly_sample_row P = rows[blockIdx.x];
    const float T = P.temperature;
    if (!(T >= 1e-4f)) {                                            // greedy row: exactly the argmax kernel's answer
        const int bi = argmax_row(r, N, L.sv, L.si);
        if (tid == 0) idx[blockIdx.x] = bi;
        return;
    }
    // element i = 4 g + w of group g, held as the key of s = x / T; absent elements have key 0 (never a candidate)
    uint32_t s[REG ? SMP_GROUPS : 1][4];
    auto load4 = [&](int g, uint32_t (&v)[4]) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int i = 4 * g + w;
            v[w] = i < N ? okey(__fdiv_rn(r[i], T)) : 0u;
        }
    };
    auto visit = [&](auto&& f) {
        if constexpr (REG) {
#pragma unroll
            for (int j = 0; j < SMP_GROUPS; ++j) {
                const int g = j * 1024 + tid;
                if (4 * g < N) f(g, s[j]);
                __builtin_amdgcn_sched_barrier(0);           // one group at a time (interleaved Philox calls spill)
            }
        } else {
            for (int g = tid; 4 * g < N; g += 1024) {
                uint32_t v[4];
                load4(g, v);
                f(g, v);
            }
        }
    };
    if constexpr (REG) {
#pragma unroll
        for (int j = 0; j < SMP_GROUPS; ++j) load4(j * 1024 + tid, s[j]);
    }
    // row maximum of s (as a key)
    uint32_t kmax = 0u;
    visit([&](int, const uint32_t (&v)[4]) {
#pragma unroll
        for (int w = 0; w < 4; ++w) kmax = max(kmax, v[w]);
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o, 64));
    if (lane == 0) L.ukey[wave] = kmax;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 16; ++w) kmax = max(kmax, L.ukey[w]);
    const float m = okey_value(kmax);
    if (kmax == 0u || !isfinite(m)) {                               // no finite score: the greedy answer
        const int bi = argmax_row(r, N, L.sv, L.si);
        if (tid == 0) idx[blockIdx.x] = bi;
        return;
    }

    // one digit level of a radix descent: 256-bin histogram of the elements with key >= lo and (key & mask) == prefix
    // (counts, and with MASS the fixed-point exp(s - m) * 2^40), summed over the copies into tcnt / tmass
    auto histogram = [&](uint32_t lo, uint32_t prefix, uint32_t mask, int shift, bool with_mass) {
        for (int t = tid; t < HCOPIES * 256; t += 1024) {
            (&L.cnt[0][0])[t] = 0u;
            (&L.mass[0][0])[t] = 0ull;
        }
        __syncthreads();
        uint32_t* hc = L.cnt[wave & (HCOPIES - 1)];
        u64* hm = L.mass[wave & (HCOPIES - 1)];
        visit([&](int, const uint32_t (&v)[4]) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t k = v[w];
                if (k >= lo && (k & mask) == prefix) {
                    const int d = (k >> shift) & 255;
                    atomicAdd(&hc[d], 1u);
                    if (with_mass) atomicAdd(&hm[d], (u64)(expf(okey_value(k) - m) * 0x1p40f));
                }
            }
        });
        __syncthreads();
        if (tid < 256) {
            uint32_t c = 0u;
            u64 ms = 0ull;
#pragma unroll
            for (int h = 0; h < HCOPIES; ++h) { c += L.cnt[h][tid]; ms += L.mass[h][tid]; }
            L.tcnt[tid] = c;
            L.tmass[tid] = ms;
        }
        __syncthreads();
    };
    // wave 0: the 256 bins in descending digit order, four per lane (lane l: digits 255-4l .. 252-4l), with the count and
    // mass of every higher digit
    struct Bins { uint32_t c[4]; u64 ms[4]; uint32_t c_above; u64 m_above; uint32_t c_total; u64 m_total; };
    auto scan_bins = [&]() {
        Bins b;
        uint32_t cs = 0u;
        u64 msum = 0ull;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            b.c[q] = L.tcnt[255 - 4 * lane - q];
            b.ms[q] = L.tmass[255 - 4 * lane - q];
            cs += b.c[q];
            msum += b.ms[q];
        }
        uint32_t ci = cs;
        u64 mi = msum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t tc = __shfl_up(ci, o, 64);
            const u64 tm = __shfl_up(mi, o, 64);
            if (lane >= o) { ci += tc; mi += tm; }
        }
        b.c_above = ci - cs;
        b.m_above = mi - msum;
        b.c_total = __shfl(ci, 63, 64);
        b.m_total = __shfl(mi, 63, 64);
        return b;
    };

    uint32_t thr = 1u;                                              // keys >= thr are kept
    const int k = P.top_k;
    if (k > 0 && k < N) {
        // top-k: the k-th largest key, digit by digit
        uint32_t prefix = 0u, mask = 0u, rem = (uint32_t)k;
        bool done = true;
#pragma unroll 1
        for (int lev = 0; lev < 4; ++lev) {
            const int shift = 24 - 8 * lev;
            histogram(1u, prefix, mask, shift, false);
            if (wave == 0) {
                const Bins b = scan_bins();
                if (lev == 0 && rem > b.c_total) {
                    if (lane == 0) L.status = 1u;                   // fewer candidates than k (NaNs): top-k is off
                } else {
                    uint32_t above = b.c_above;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (b.c[q] && above < rem && rem <= above + b.c[q]) {
                            L.digit = 255 - 4 * lane - q;
                            L.rem = rem - above;
                            L.status = 0u;
                        }
                        above += b.c[q];
                    }
                }
            }
            __syncthreads();
            if (L.status) { done = false; break; }
            prefix |= L.digit << shift;
            mask |= 0xffu << shift;
            rem = L.rem;
        }
        if (done) thr = prefix;
    }
    const float p = P.top_p;
    if (p > 0.f && p < 1.f) {
        // top-p: the lowest key whose kept mass strictly above it is < p * Z, digit by digit
        uint32_t prefix = 0u, mask = 0u;
        u64 base = 0ull;
        double pz = 0.0;                                            // p * Z (wave 0)
#pragma unroll 1
        for (int lev = 0; lev < 4; ++lev) {
            const int shift = 24 - 8 * lev;
            histogram(thr, prefix, mask, shift, true);
            if (wave == 0) {
                const Bins b = scan_bins();
                if (lev == 0) pz = (double)p * (double)b.m_total;
                int found = -1;
                u64 fb = 0ull, above = base + b.m_above;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (b.c[q] && (double)above < pz) { found = 255 - 4 * lane - q; fb = above; }
                    above += b.ms[q];
                }
                // the condition holds on an upper set of digits: the lowest one is in the highest lane that found one
                const u64 bal = __ballot(found >= 0);
                if (bal && lane == 63 - __builtin_clzll(bal)) { L.digit = (uint32_t)found; L.base = fb; }
            }
            __syncthreads();
            prefix |= L.digit << shift;
            mask |= 0xffu << shift;
            base = L.base;
        }
        thr = prefix;
    }

    // the draw: Gumbel-max over the kept elements, one Philox call per group of four
    const uint32_t c = (uint32_t)((ctr ? ctr[ctr_per_row ? blockIdx.x : 0] : 0) + ctr_add);
    float best = -INFINITY;
    int bi = 0x7fffffff;
    visit([&](int g, const uint32_t (&v)[4]) {
        bool any = false;
#pragma unroll
        for (int w = 0; w < 4; ++w) any |= v[w] >= thr;
        if (!any) return;
        const u32x4 rnd = philox4x32_10((uint32_t)g, c, P.seed_lo, P.seed_hi);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (v[w] >= thr) {
                const float z = okey_value(v[w]) + gumbel(rnd[w]);
                if (first_max_better(z, 4 * g + w, best, bi)) { best = z; bi = 4 * g + w; }
            }
        }
    });
    bi = block_first_max(best, bi, L.sv, L.si);
    if (tid == 0) idx[blockIdx.x] = bi;
}

}  // namespace

extern "C" int vly_argmax(const float* x, int32_t* idx, int M, int N, int ld, const vly_sample_row* rows, const int32_t* ctr,
                          int ctr_per_row, int ctr_add, void* stream) {
    if (M <= 0 || N <= 0 || ld < N || !x || !idx || ((uintptr_t)rows & 3) || ((uintptr_t)ctr & 3)) {
        vly_set_error("vly_argmax: bad args M=%d N=%d ld=%d", M, N, ld);
        return -22;
    }
    if (!rows)
        hipLaunchKernelGGL(argmax_kernel, dim3(M), dim3(1024), 0, (hipStream_t)stream, x, idx, N, ld);
    else if (N <= SMP_REG_N)
        hipLaunchKernelGGL(sample_kernel<true>, dim3(M), dim3(1024), 0, (hipStream_t)stream, x, idx, N, ld, rows, ctr,
                           ctr_per_row, ctr_add);
    else
        hipLaunchKernelGGL(sample_kernel<false>, dim3(M), dim3(1024), 0, (hipStream_t)stream, x, idx, N, ld, rows, ctr,
                           ctr_per_row, ctr_add);
    return vly_check_launch("vly_argmax");
}
