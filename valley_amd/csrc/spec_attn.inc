// The split attention of a speculative verify step, shared by libvalley_hip_spec.so (spec.hip: ONE position per launch) and
// libvalley_hip_spec_rows.so (spec_rows.hip: one position per sequence).  Included inside the unit's anonymous namespace, behind
// common.hpp.  The two forms differ in where a sequence's position comes from and in what happens at the end of the cache
// (ROWS below); the arithmetic of the query at absolute position P is the same instruction sequence in both, which is what makes
// a row of one library bit for bit the row of the other.

typedef __attribute__((ext_vector_type(2))) _Float16 sp_f16x2;
typedef __attribute__((ext_vector_type(2))) __bf16 sp_bf16x2;

template <int DT> VLY_DEVICE float t_h2f(uint16_t v) {
    if constexpr (DT == 1) return (float)__builtin_bit_cast(_Float16, v);
    else return __uint_as_float(((uint32_t)v) << 16);
}
template <int DT> VLY_DEVICE float t_lo(uint32_t w) {
    if constexpr (DT == 1) return (float)__builtin_bit_cast(sp_f16x2, w)[0];
    else return __uint_as_float(w << 16);
}
template <int DT> VLY_DEVICE float t_hi(uint32_t w) {
    if constexpr (DT == 1) return (float)__builtin_bit_cast(sp_f16x2, w)[1];
    else return __uint_as_float(w & 0xffff0000u);
}
template <int DT> VLY_DEVICE uint32_t t_pack2(float lo, float hi) {
    const vly_f32x2 v = {lo, hi};
    if constexpr (DT == 1) return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, sp_f16x2));
    else return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, sp_bf16x2));
}

constexpr float LOG2E = 1.4426950408889634f;
constexpr float NEG_BIG = -1.0e30f;
constexpr int SPLITS = 4;                                        // = VLY_SPEC_SPLITS = VLY_SPEC_ROWS_SPLITS
constexpr int PART = 132;                                        // = VLY_SPEC_PARTIAL = VLY_SPEC_ROWS_PARTIAL

// x + x[lane ^ 1], then + [lane ^ 2]: the four lanes of a quad end with the same bits ((a0 + a1) + (a2 + a3), commutative adds)
VLY_DEVICE float quad_sum(float v) {
    v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0xb1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
    v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x4e, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
    return v;
}

// grid (heads, B, SPLITS), 256 threads.  Per 64-key block: thread t holds a quarter (32 dims) of K row t >> 2 for the scores and
// 8 dims of V rows (t >> 4) + 16 u, u < 4, for P.V; the next block of the split is requested before the current one is used.
// Per query: running max m, sum l (replicated in every thread) and the thread's 8 x (its 4 keys) share of P.V; at the end the
// sixteen key groups are added in LDS in a fixed order and (m, l, o[128]) is published for the merge.
//
// ROWS = false (vly_spec_attention): past = the host's value, or past_dev[0] clamped to [0, ctx_max - S]; kv_len = past + S.
// ROWS = true (vly_spec_rows_attention): past = past_dev[b] clamped to [0, ctx_max - 1]; kv_len = min(past + S, ctx_max).  A
// query whose position past + i lies behind the cache is DEAD: it is computed as a query at the cache's last position (finite,
// ignored by the caller), so no key index, table column or cache row behind ctx_max is ever formed.
template <int S, int DT, bool ROWS>
__global__ void __launch_bounds__(256) spec_attn_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ kc,
                                                        const uint16_t* __restrict__ vc, const uint8_t* __restrict__ key_valid,
                                                        int kv_stride, uint16_t* __restrict__ out, int heads, int past,
                                                        const int32_t* __restrict__ past_dev, int ctx_max,
                                                        float* __restrict__ partials, unsigned* __restrict__ arrivals) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float qs[S][128];
    __shared__ float sc[S][64];
    __shared__ float red[2][S][4];
    __shared__ __attribute__((aligned(16))) float acc_s[16][128];
    __shared__ int last_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x, b = blockIdx.y, sp = blockIdx.z;
    const int Hq = heads * 128;
    if constexpr (ROWS) past = max(0, min(past_dev[b], ctx_max - 1));
    else if (past_dev) past = max(0, min(past_dev[0], ctx_max - S));
    const int kv_len = ROWS ? min(past + S, ctx_max) : past + S; // <= ctx_max: every row index below is clamped to kv_len - 1
    // the position of query i (uniform): past + i, a dead row's brought back to the last row there is
    auto qpos = [&](int i) { return ROWS ? min(past + i, kv_len - 1) : past + i; };
    const int nblk = (kv_len + 63) >> 6;
    const uint16_t* kbase = kc + ((size_t)b * heads + h) * ctx_max * 128;
    const uint16_t* vbase = vc + ((size_t)b * heads + h) * ctx_max * 128;
    const uint8_t* kvld = key_valid ? key_valid + (size_t)b * kv_stride : nullptr;

    for (int e = tid; e < S * 128; e += 256) {
        const int i = e >> 7, d = e & 127;
        qs[i][d] = t_h2f<DT>(qkv[((size_t)b * S + i) * 3 * Hq + h * 128 + d]) * (0.08838834764831845f * LOG2E);
    }

    const int kr = tid >> 2, qd = tid & 3;                       // score role: key row of the block, quarter of its dims
    const int kg = tid >> 4, dc = tid & 15;                      // P.V role: key group, 8-dim chunk
    u32x4 kk[4], vv[4], kn[4], vn[4];
    uint8_t kval = 1, kvaln = 1;
    auto request = [&](int c, u32x4 (&k4)[4], u32x4 (&v4)[4], uint8_t& valid) {
        const int jk = min(c * 64 + kr, kv_len - 1);
        const u32x4* kp = (const u32x4*)(kbase + (size_t)jk * 128 + 32 * qd);
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) k4[cc] = kp[cc];
        valid = kvld ? kvld[jk] : (uint8_t)1;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jv = min(c * 64 + kg + 16 * u, kv_len - 1);
            v4[u] = *(const u32x4*)(vbase + (size_t)jv * 128 + 8 * dc);
        }
    };
    if (sp < nblk) request(sp, kk, vv, kval);

    float m_run[S], l_run[S], o[S][8];
#pragma unroll
    for (int i = 0; i < S; ++i) {
        m_run[i] = NEG_BIG;
        l_run[i] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[i][e] = 0.f;
    }
    __syncthreads();

#pragma unroll 1
    for (int c = sp; c < nblk; c += SPLITS) {
        if (c + SPLITS < nblk) request(c + SPLITS, kn, vn, kvaln);
        const int c0 = c * 64, jk = c0 + kr;
        // rows from kv_len on (clamped loads of the newest row) count as zero: never 0 x stale data
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (c0 + kg + 16 * u >= kv_len) vv[u] = u32x4{0u, 0u, 0u, 0u};
        float s[S], alpha[S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
            s[i] = NEG_BIG;
            if (c0 <= qpos(i)) {                                 // (uniform) the block holds keys of this query's past
                float a = 0.f;
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    const f32x4 q0 = *(const f32x4*)(&qs[i][32 * qd + 8 * cc]), q1 = *(const f32x4*)(&qs[i][32 * qd + 8 * cc + 4]);
                    a = __builtin_fmaf(t_lo<DT>(kk[cc][0]), q0[0], a); a = __builtin_fmaf(t_hi<DT>(kk[cc][0]), q0[1], a);
                    a = __builtin_fmaf(t_lo<DT>(kk[cc][1]), q0[2], a); a = __builtin_fmaf(t_hi<DT>(kk[cc][1]), q0[3], a);
                    a = __builtin_fmaf(t_lo<DT>(kk[cc][2]), q1[0], a); a = __builtin_fmaf(t_hi<DT>(kk[cc][2]), q1[1], a);
                    a = __builtin_fmaf(t_lo<DT>(kk[cc][3]), q1[2], a); a = __builtin_fmaf(t_hi<DT>(kk[cc][3]), q1[3], a);
                }
                a = quad_sum(a);
                if (jk <= qpos(i) && kval) s[i] = a;             // a select: a NaN score of a masked key is dropped
                const float mc = wave_max(s[i]);
                if (lane == 0) red[0][i][wave] = mc;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < S; ++i) {
            if (c0 <= qpos(i)) {
                const float mc = fmaxf(fmaxf(red[0][i][0], red[0][i][1]), fmaxf(red[0][i][2], red[0][i][3]));
                const float m_new = fmaxf(m_run[i], mc);
                alpha[i] = __builtin_amdgcn_exp2f(m_run[i] - m_new);
                const float p = s[i] > 0.5f * NEG_BIG ? __builtin_amdgcn_exp2f(s[i] - m_new) : 0.f;   // masked keys never count
                m_run[i] = m_new;
                if (qd == 0) sc[i][kr] = p;
                const float lc = wave_sum(qd == 0 ? p : 0.f);
                if (lane == 0) red[1][i][wave] = lc;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < S; ++i) {
            if (c0 <= qpos(i)) {
                const float lc = ((red[1][i][0] + red[1][i][1]) + red[1][i][2]) + red[1][i][3];
                l_run[i] = l_run[i] * alpha[i] + lc;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[i][e] *= alpha[i];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float pj = sc[i][kg + 16 * u];
                    o[i][0] = __builtin_fmaf(pj, t_lo<DT>(vv[u][0]), o[i][0]); o[i][1] = __builtin_fmaf(pj, t_hi<DT>(vv[u][0]), o[i][1]);
                    o[i][2] = __builtin_fmaf(pj, t_lo<DT>(vv[u][1]), o[i][2]); o[i][3] = __builtin_fmaf(pj, t_hi<DT>(vv[u][1]), o[i][3]);
                    o[i][4] = __builtin_fmaf(pj, t_lo<DT>(vv[u][2]), o[i][4]); o[i][5] = __builtin_fmaf(pj, t_hi<DT>(vv[u][2]), o[i][5]);
                    o[i][6] = __builtin_fmaf(pj, t_lo<DT>(vv[u][3]), o[i][6]); o[i][7] = __builtin_fmaf(pj, t_hi<DT>(vv[u][3]), o[i][7]);
                }
            }
        }
        // (no barrier here: the next block writes red[0] before its first barrier, sc / red[1] behind it, and every read of
        // them above lies before this thread's next arrival at that barrier)
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) { kk[cc] = kn[cc]; vv[cc] = vn[cc]; }
        kval = kvaln;
    }

    // ---- publish (m, l, o[128]) per query: write-through stores, as split_publish (attention.hip)
#pragma unroll
    for (int i = 0; i < S; ++i) {
        float* part = partials + ((((size_t)b * heads + h) * S + i) * SPLITS + sp) * PART;
        __syncthreads();                                         // acc_s: the previous query's sums have been read
#pragma unroll
        for (int e = 0; e < 8; ++e) acc_s[kg][8 * dc + e] = o[i][e];
        __syncthreads();
        if (tid < 128) {
            float t = 0.f;
#pragma unroll
            for (int k2 = 0; k2 < 16; ++k2) t += acc_s[k2][tid];
            __hip_atomic_store(part + 4 + tid, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (tid < 132) {
            __hip_atomic_store(part + tid - 128, tid == 128 ? m_run[i] : tid == 129 ? l_run[i] : 0.f, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
    }

    // ---- the last of the head's four workgroups to get here merges (split_merge_if_last's ticket, in its fenced form): the
    // partials are drained and released before the ticket, acquired behind it; nobody waits for anybody
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned* ctr = arrivals + (size_t)b * heads + h;
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_s = t == SPLITS - 1;
        if (t == SPLITS - 1) {
            __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
    }
    __syncthreads();
    if (!last_s || tid >= 32 * S) return;
    // 32 lanes x 4 dims per query, split_merge_if_last's arithmetic in split order
    const int i = tid >> 5, ln = tid & 31;
    const float* hb = partials + (((size_t)b * heads + h) * S + i) * (SPLITS * PART);
    float ms[SPLITS], ls[SPLITS], os[SPLITS][4];
#pragma unroll
    for (int q = 0; q < SPLITS; ++q) {
        ms[q] = __hip_atomic_load(hb + q * PART, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ls[q] = __hip_atomic_load(hb + q * PART + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int r = 0; r < 4; ++r) os[q][r] = __hip_atomic_load(hb + q * PART + 4 + 4 * ln + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    float mx = ms[0];
#pragma unroll
    for (int q = 1; q < SPLITS; ++q) mx = fmaxf(mx, ms[q]);
    float L = 0.f, O[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < SPLITS; ++q) {
        const float w = exp2f(ms[q] - mx);
        L = __builtin_fmaf(ls[q], w, L);
#pragma unroll
        for (int r = 0; r < 4; ++r) O[r] = __builtin_fmaf(os[q][r], w, O[r]);
    }
    u32x2 pk;
    pk[0] = t_pack2<DT>(O[0] / L, O[1] / L);
    pk[1] = t_pack2<DT>(O[2] / L, O[3] / L);
    *(u32x2*)(out + ((size_t)b * S + i) * Hq + h * 128 + 4 * ln) = pk;
}
