// The row top-K and per-prompt merge of beam search, shared by libvalley_hip_beam.so (beam.hip: over log_softmax(logits)
// + running) and libvalley_hip_logits.so (logits.hip: over processed scores + running).  Included inside an anonymous
// namespace of a translation unit that has included <hip/hip_runtime.h> and <stdint.h>.
//
// Row top-K: one 1024-thread workgroup per logits row.  The row's accumulated score is turned into an order-preserving
// uint32 key (NaN lowest), held in registers for rows up to 32 k wide, and the K-th largest key is found by radix descent
// over four 8-bit digits (256-bin LDS histograms, the method of sampling.hip).  Ties at the boundary key are resolved to
// the lowest indices by a second descent over the index bits.  The K selected elements are ranked in LDS and written,
// best first, to the scratch; the last workgroup of a prompt (ticket counter, the hand-off of
// vly_decode_attention_merged) merges its nb sorted lists by binary search.

#define BM_DEVICE __device__ __forceinline__

constexpr int MAX_K = 64;
constexpr int MAX_NB = 16;
constexpr int ROW_THREADS = 1024;
constexpr int REG_J = 32;                           // values per thread held in registers: rows up to 32768 wide
constexpr int HCOPIES = 4;                          // histogram copies (wave & 3): spreads the atomics of hot bins

// order-preserving key of a float; -0 and +0 share a key; NaN is 0, below every real value
BM_DEVICE uint32_t okey(float s) {
    if (s != s) return 0u;
    const uint32_t u = __float_as_uint(s + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
BM_DEVICE float okey_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

struct Entry {                                      // one candidate of a row's sorted list in the scratch
    uint32_t key;
    int32_t tok;
};

struct RowLds {
    uint32_t cnt[HCOPIES][256];
    uint32_t tcnt[256];
    float red[16];
    uint32_t ck[MAX_K];
    int32_t ci[MAX_K];
    uint32_t digit, rem, n, last;
    // the merge of the last workgroup of a prompt
    uint32_t mk[MAX_NB * MAX_K];
    int32_t mt[MAX_NB * MAX_K];
};

BM_DEVICE float block_max(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float m = red[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) m = fmaxf(m, red[w]);
    return m;
}

// fixed reduction order (lanes by xor tree, waves in index order): the same bits at every launch
BM_DEVICE float block_sum(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = red[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) s += red[w];
    return s;
}

// the log-sum-exp of a row: m + log(sum exp(x - m)) over its non-NaN values, 0 when the maximum is not finite.  visit_x(f)
// calls f(i, x_i) for the thread's elements i = tid, tid + ROW_THREADS, ... in that order: with the fixed block reductions
// the result has the same bits in every kernel that visits a row this way
// (row_max: the row's maximum over its non-NaN values, -inf for a row without one, for a caller that needs it too)
template <typename VisitX>
BM_DEVICE float row_lse(VisitX&& visit_x, float* red, float& row_max) {
    float m = -INFINITY;
    visit_x([&](int, float v) { m = fmaxf(m, v); });            // (fmaxf ignores NaN)
    m = block_max(m, red);
    row_max = m;
    float s = 0.f;
    if (m > -INFINITY && m < INFINITY)
        visit_x([&](int, float v) { if (v == v) s += expf(v - m); });
    s = block_sum(s, red);
    return (m > -INFINITY && m < INFINITY) ? m + logf(s) : 0.f;
}

template <typename VisitX>
BM_DEVICE float row_lse(VisitX&& visit_x, float* red) {
    float m;
    return row_lse(visit_x, red, m);
}

template <bool REG, bool LSE>
__global__ void __launch_bounds__(ROW_THREADS) beam_rows_kernel(const float* __restrict__ logits, int ld, int V, int nb,
                                                                const float* __restrict__ running, int K,
                                                                const int32_t* __restrict__ eos, int n_eos,
                                                                uint32_t* __restrict__ tickets, Entry* __restrict__ lists,
                                                                float* __restrict__ score, int32_t* __restrict__ token,
                                                                int32_t* __restrict__ beam, uint8_t* __restrict__ hit) {
    __shared__ RowLds L;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = blockIdx.x;
    const float* x = logits + (size_t)r * ld;
    const float run = running[r];

    float xv[REG ? REG_J : 1];
    if constexpr (REG) {
#pragma unroll
        for (int j = 0; j < REG_J; ++j) {
            const int i = j * ROW_THREADS + tid;
            xv[j] = i < V ? x[i] : __builtin_nanf("");
        }
    }
    // f(i, x_i) over the row's elements (NaN stands for an absent element in the register form)
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
    // LSE: acc = (x - lse) + running over the logits; otherwise acc = y + running over scores the caller processed
    // (vly_logits_process's log-softmax mode wrote y = x - lse with the same row_lse: a row it left alone keys the same)
    float lse = 0.f;
    if constexpr (LSE) lse = row_lse(visit_x, L.red);
    auto key_of = [&](float v) { return LSE ? okey((v - lse) + run) : okey(v + run); };

    // ---- radix descent: the K-th largest key ------------------------------------------------------------------------
    uint32_t k_reg[REG ? REG_J : 1];
    if constexpr (REG) {
#pragma unroll
        for (int j = 0; j < REG_J; ++j) k_reg[j] = key_of(xv[j]);
    }
    auto visit = [&](auto&& f) {                                 // f(i, key_i)
        if constexpr (REG) {
#pragma unroll
            for (int j = 0; j < REG_J; ++j) {
                const int i = j * ROW_THREADS + tid;
                if (i < V) f(i, k_reg[j]);
            }
        } else {
            for (int i = tid; i < V; i += ROW_THREADS) f(i, key_of(x[i]));
        }
    };
    // one level: 256-bin histogram of digit(v) over the elements with (v & mask) == prefix, summed into tcnt; then
    // wave 0 finds the digit (searched from 255 down if DESC, from 0 up otherwise) at which the running count reaches rem
    auto level = [&](auto&& value_of, uint32_t prefix, uint32_t mask, int shift, uint32_t rem, bool desc) {
        for (int t = tid; t < HCOPIES * 256; t += ROW_THREADS) (&L.cnt[0][0])[t] = 0u;
        __syncthreads();
        uint32_t* hc = L.cnt[wave & (HCOPIES - 1)];
        visit([&](int i, uint32_t k) {
            const uint32_t v = value_of(i, k);
            if ((v & mask) == prefix) atomicAdd(&hc[(v >> shift) & 255], 1u);
        });
        __syncthreads();
        if (tid < 256) {
            uint32_t c = 0u;
#pragma unroll
            for (int h = 0; h < HCOPIES; ++h) c += L.cnt[h][tid];
            L.tcnt[tid] = c;
        }
        __syncthreads();
        if (wave == 0) {
            // lane l owns four bins in search order: positions 4l .. 4l + 3
            uint32_t c[4], cs = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int pos = 4 * lane + q;
                c[q] = L.tcnt[desc ? 255 - pos : pos];
                cs += c[q];
            }
            uint32_t ci = cs;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = __shfl_up(ci, o, 64);
                if (lane >= o) ci += t;
            }
            uint32_t before = ci - cs;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (c[q] && before < rem && rem <= before + c[q]) {
                    const int pos = 4 * lane + q;
                    L.digit = desc ? 255 - pos : pos;
                    L.rem = rem - before;
                }
                before += c[q];
            }
        }
        __syncthreads();
    };
    const uint32_t Kr = (uint32_t)K;
    uint32_t prefix = 0u, mask = 0u, rem = Kr;
    for (int lev = 0; lev < 4; ++lev) {
        const int shift = 24 - 8 * lev;
        level([](int, uint32_t k) { return k; }, prefix, mask, shift, rem, true);
        prefix |= L.digit << shift;
        mask |= 0xffu << shift;
        rem = L.rem;
    }
    const uint32_t thr = prefix;                                 // the K-th largest key; take `rem` of the keys equal to it
    const uint32_t n_eq = L.tcnt[thr & 255];
    int icut = 0x7fffffff;                                       // ... those with the lowest indices: index <= icut
    if (n_eq > rem) {
        uint32_t ip = 0u, im = 0u, irem = rem;
        for (int lev = 0; lev < 3; ++lev) {                      // indices < 2^24
            const int shift = 16 - 8 * lev;
            level([&](int i, uint32_t k) { return k == thr ? (uint32_t)i : 0xffffffffu; }, ip, im | 0xff000000u, shift, irem,
                  false);
            ip |= L.digit << shift;
            im |= 0xffu << shift;
            irem = L.rem;
        }
        icut = (int)ip;
    }
    // ---- collect the K, rank them, publish the row's sorted list ------------------------------------------------------
    if (tid == 0) L.n = 0u;
    __syncthreads();
    visit([&](int i, uint32_t k) {
        if (k > thr || (k == thr && i <= icut)) {
            const uint32_t slot = atomicAdd(&L.n, 1u);
            if (slot < (uint32_t)MAX_K) { L.ck[slot] = k; L.ci[slot] = i; }
        }
    });
    __syncthreads();
    Entry* mine = lists + (size_t)r * K;
    if (tid < K) {
        const uint32_t k = L.ck[tid];
        const int i = L.ci[tid];
        int rank = 0;
        for (int j = 0; j < K; ++j) rank += (L.ck[j] > k || (L.ck[j] == k && L.ci[j] < i)) ? 1 : 0;
        mine[rank] = Entry{k, i};
    }
    // ---- hand-off: the last workgroup of the prompt merges --------------------------------------------------------------
    __threadfence();
    __syncthreads();
    const int b = r / nb;
    if (tid == 0) {
        const uint32_t t = atomicAdd(&tickets[b], 1u);
        L.last = t == (uint32_t)(nb - 1);
        if (L.last) {
            tickets[b] = 0u;                                     // back at zero for the next launch
            __threadfence();
        }
    }
    __syncthreads();
    if (!L.last) return;
    const int n = nb * K;
    const Entry* pl = lists + (size_t)b * nb * K;
    for (int e = tid; e < n; e += ROW_THREADS) {
        L.mk[e] = __hip_atomic_load(&pl[e].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        L.mt[e] = __hip_atomic_load(&pl[e].tok, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (tid < n) {
        const int jt = tid / K, pos = tid - jt * K;
        const uint32_t k = L.mk[tid];
        // rank = number of better candidates: in its own list the ones before it; in list j the keys above k, and the
        // keys equal to k too when j < jt (same key, lower flat index j * V + t)
        int rank = pos;
        for (int j = 0; j < nb; ++j) {
            if (j == jt) continue;
            const uint32_t* lk = L.mk + j * K;
            const bool ge = j < jt;
            int lo = 0, hi = K;                                  // first position whose key is not better (lists descend)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (ge ? lk[mid] >= k : lk[mid] > k) lo = mid + 1;
                else hi = mid;
            }
            rank += lo;
        }
        if (rank < K) {
            const int o = b * K + rank;
            const int t = L.mt[tid];
            score[o] = okey_value(k);
            token[o] = t;
            beam[o] = b * nb + jt;
            bool h = false;
            for (int e = 0; e < n_eos; ++e) h |= eos[e] == t;
            hit[o] = h ? 1 : 0;
        }
    }
}

size_t lists_offset(int B) { return ((size_t)B * 4 + 255) / 256 * 256; }

size_t beam_scratch_bytes(int B, int nb, int K) {
    if (B <= 0 || nb <= 0 || K <= 0) return 0;
    return lists_offset(B) + (size_t)B * nb * K * sizeof(Entry);
}

bool beam_rows_args_ok(const float* logits, int ld, int V, int B, int nb, const float* running, int K, const int32_t* eos,
                       int n_eos, const void* scratch, const float* score, const int32_t* token, const int32_t* beam,
                       const uint8_t* hit) {
    return logits && running && scratch && score && token && beam && hit && B > 0 && nb > 0 && nb <= MAX_NB && K >= nb &&
           K <= MAX_K && V >= K && V < (1 << 24) && ld >= V && n_eos >= 0 && (n_eos == 0 || eos) &&
           !((uintptr_t)scratch & 255) && !((uintptr_t)logits & 3);
}

// one workgroup per row, then the merge by the last workgroup of each prompt (arguments checked by beam_rows_args_ok)
template <bool LSE>
void launch_beam_rows(const float* logits, int ld, int V, int B, int nb, const float* running, int K, const int32_t* eos,
                      int n_eos, void* scratch, float* score, int32_t* token, int32_t* beam, uint8_t* hit, hipStream_t stream) {
    uint32_t* tickets = (uint32_t*)scratch;
    Entry* lists = (Entry*)((char*)scratch + lists_offset(B));
    if (V <= REG_J * ROW_THREADS)
        hipLaunchKernelGGL((beam_rows_kernel<true, LSE>), dim3(B * nb), dim3(ROW_THREADS), 0, stream, logits, ld, V, nb, running,
                           K, eos, n_eos, tickets, lists, score, token, beam, hit);
    else
        hipLaunchKernelGGL((beam_rows_kernel<false, LSE>), dim3(B * nb), dim3(ROW_THREADS), 0, stream, logits, ld, V, nb, running,
                           K, eos, n_eos, tickets, lists, score, token, beam, hit);
}
