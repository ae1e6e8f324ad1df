// ann_search_body.inc -- the body of the graph search kernels (kernels_ann.hip), included once per tail:
//   R3DM_ANN_KNN 0   ann_search_kernel<NQ, ROWS>(P): the two best pool entries and the ratio test
//   R3DM_ANN_KNN 1   ann_search_knn_kernel<NQ, ROWS>(P, k): the first min(L, k) pool entries, ascending, -1 / +inf behind them; the pool
//                    holds k + P entries (P.pool_cap), as KGraphImpl::search sizes it
// One text, so that the two kernels cannot drift apart; an include rather than a shared function, so that the 2-NN kernels keep the
// machine code they were profiled with (a body function taking the parameter block loses the address spaces of its pointers).
    extern __shared__ __attribute__((aligned(16))) unsigned char ann_smem[];
    const uint32_t pair = blockIdx.x / P.qb_per_pair;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t q = (blockIdx.x % P.qb_per_pair) * 4 + wave;
    const uint2 pr = P.pairs[pair];
    const ImgDev* __restrict__ Ip = P.imgs + pr.x;
    const ImgDev* __restrict__ Jp = P.imgs + pr.y;
    const uint32_t nI = Ip->n, nJ = Jp->n, dim = Ip->dim, g4 = dim >> 2;
    if (q >= nJ) return;                                          // whole wave; no workgroup barrier below
    uint32_t* flags = (uint32_t*)ann_smem + (size_t)wave * P.flag_words;
    for (uint32_t w = lane; w < P.flag_words; w += 64) flags[w] = 0u;

    const uint32_t sub = lane & 3u, grp = lane >> 2;
    const uint32_t g_lo = sub * NQ;
    const float* __restrict__ rowsI = Ip->rows;
    const uint16_t* __restrict__ rows16 = Ip->ann_rows16;
    const uint8_t* __restrict__ rows8 = Ip->ann_rows8;
    [[maybe_unused]] const float* __restrict__ normsI = Ip->norms;
    const uint32_t* __restrict__ adj = Ip->ann_adj;
    const uint32_t* __restrict__ deg = Ip->ann_deg;

    f32x4 qv[ROWS == 3 ? 1 : NQ];
    [[maybe_unused]] uint32_t q8[ROWS == 3 ? NQ : 1];
    [[maybe_unused]] uint32_t qq_part = 0;                  // ||q||^2 (summed over the four lanes of the group below)
    if constexpr (ROWS == 3) {
        static_assert(ROWS != 3 || NQ % 4 == 0, "byte rows are read 16 elements at a time");
        const u32x4* src = (const u32x4*)(Jp->ann_rows8 + (size_t)q * dim) + (g_lo >> 2);
#pragma unroll
        for (int g4i = 0; g4i < NQ / 4; ++g4i) {
            const u32x4 w = (g_lo + 4 * g4i < g4) ? src[g4i] : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 4; ++k) { q8[4 * g4i + k] = w[k]; qq_part = __builtin_amdgcn_udot4(w[k], w[k], qq_part, false); }
        }
        qq_part += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)qq_part, 0xB1, 0xF, 0xF, true);
        qq_part += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)qq_part, 0x4E, 0xF, 0xF, true);
    } else {
        const f32x4* src = (const f32x4*)(Jp->rows + (size_t)q * dim);
#pragma unroll
        for (int g = 0; g < NQ; ++g) qv[g] = (g_lo + g < g4) ? src[g_lo + g] : f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // pool: one entry per lane, ascending distance, `L` valid entries, at most `cap` = K + P
    float pdist = R3DM_INF; uint32_t pid = kNone, pm = 0, pM = 0; bool pflag = false;
    uint32_t L = 0;
    const uint32_t cap = P.pool_cap, S = P.S;
    const uint2 vid = P.pair_ids[pair];
    uint32_t comps = 0;

    uint32_t e_id = 0, e_m = 0, end_m = 0;
    uint32_t seed_round = 0;
    const uint32_t n_seed_rounds = (P.P + 15) / 16;
    for (;;) {
        // ---- the 16 candidates of this step: start rows first, then neighbours of the best open pool entry
        uint32_t cid = kNone;
        bool valid;
        if (seed_round < n_seed_rounds) {
            const uint32_t s = seed_round * 16 + grp;
            valid = s < P.P;
            if (valid) {
                const uint32_t lo = (uint32_t)(((uint64_t)s * nI) / P.P), hi = (uint32_t)(((uint64_t)(s + 1) * nI) / P.P);
                const uint64_t r = ann_rng_u64(P.seed ^ 0x6b67726170680000ULL, vid.x, vid.y, q, s);
                cid = lo + (uint32_t)(((r >> 32) * (uint64_t)(hi - lo)) >> 32);
            }
            ++seed_round;
        } else {
            const unsigned long long open = __ballot(pflag && lane < L);
            if (open == 0ull) break;
            const uint32_t k = (uint32_t)__builtin_ctzll(open);
            e_id = (uint32_t)__builtin_amdgcn_readlane((int)pid, (int)k);
            e_m = (uint32_t)__builtin_amdgcn_readlane((int)pm, (int)k);
            const uint32_t e_M = (uint32_t)__builtin_amdgcn_readlane((int)pM, (int)k);
            end_m = e_m + S;
            const bool done = end_m > e_M;
            if (done) end_m = e_M;
            if (lane == k) { pm = end_m; if (done) pflag = false; }
            valid = (grp < S) && (e_m + grp < end_m);
            if (valid) cid = adj[(size_t)e_id * kAnnDeg + e_m + grp];
        }
        bool fresh = false;
        if (valid) fresh = ((flags[cid >> 5] >> (cid & 31u)) & 1u) == 0u;
        if (fresh && sub == 0) atomicOr(&flags[cid >> 5], 1u << (cid & 31u));

        // ---- distance of the group's candidate in the reference's summation order
        float r = 0.0f;
        uint32_t cdeg = 0;
        if constexpr (ROWS == 3) {
            if (fresh) {
                const u32x4* a8 = (const u32x4*)(rows8 + (size_t)cid * dim) + (g_lo >> 2);
                const float aa_f = normsI[cid];                                // ||a||^2 from the staging statistics (an integer)
                uint32_t aq = 0;
#pragma unroll
                for (int g4i = 0; g4i < NQ / 4; ++g4i) {
                    if (g_lo + 4 * g4i < g4) {
                        const u32x4 w = a8[g4i];
#pragma unroll
                        for (int k = 0; k < 4; ++k) aq = __builtin_amdgcn_udot4(w[k], q8[4 * g4i + k], aq, false);
                    }
                }
                cdeg = deg[cid];
                aq += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)aq, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
                aq += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)aq, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]: all four lanes hold a.q
                r = (float)((uint32_t)aa_f + qq_part - 2u * aq);                    // sum of (a - q)^2 >= 0, below 2^24
            }
        } else
        if (fresh) {
            float gs[NQ];
            if constexpr (ROWS == 2) {
                static_assert(NQ % 4 == 0, "u8 rows are read 16 elements (four groups) at a time");
                const u32x4* a8 = (const u32x4*)(rows8 + (size_t)cid * dim) + (g_lo >> 2);
#pragma unroll
                for (int g4i = 0; g4i < NQ / 4; ++g4i) {
                    if (g_lo + 4 * g4i < g4) {                                 // dim % 16 == 0: groups come in fours
                        const u32x4 w = a8[g4i];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const f32x4 v = {(float)(w[k] & 0xFFu), (float)((w[k] >> 8) & 0xFFu), (float)((w[k] >> 16) & 0xFFu), (float)(w[k] >> 24)};
                            gs[4 * g4i + k] = group_sq(v, qv[4 * g4i + k]);
                        }
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) gs[4 * g4i + k] = 0.0f;
                    }
                }
            } else if constexpr (ROWS == 1) {
                static_assert(NQ % 2 == 0, "bf16 rows are read 8 elements (two groups) at a time");
                const u32x4* a16 = (const u32x4*)(rows16 + (size_t)cid * dim) + (g_lo >> 1);
#pragma unroll
                for (int g2 = 0; g2 < NQ / 2; ++g2) {
                    if (g_lo + 2 * g2 < g4) {                                  // dim % 8 == 0: groups come in pairs
                        const u32x4 w = a16[g2];
                        const f32x4 lo4 = {__uint_as_float(w[0] << 16), __uint_as_float(w[0] & 0xFFFF0000u), __uint_as_float(w[1] << 16), __uint_as_float(w[1] & 0xFFFF0000u)};
                        const f32x4 hi4 = {__uint_as_float(w[2] << 16), __uint_as_float(w[2] & 0xFFFF0000u), __uint_as_float(w[3] << 16), __uint_as_float(w[3] & 0xFFFF0000u)};
                        gs[2 * g2] = group_sq(lo4, qv[2 * g2]); gs[2 * g2 + 1] = group_sq(hi4, qv[2 * g2 + 1]);
                    } else { gs[2 * g2] = 0.0f; gs[2 * g2 + 1] = 0.0f; }
                }
            } else {
                const f32x4* a = (const f32x4*)(rowsI + (size_t)cid * dim) + g_lo;
#pragma unroll
                for (int g = 0; g < NQ; ++g) gs[g] = (g_lo + g < g4) ? group_sq(a[g], qv[g]) : 0.0f;
            }
            cdeg = deg[cid];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                float t = r;
#pragma unroll
                for (int g = 0; g < NQ; ++g) t = ((uint32_t)(s * NQ + g) < g4) ? t + gs[g] : t;
                r = (sub == (uint32_t)s) ? t : r;
                const float prev = __shfl_up(r, 1);
                if (sub == (uint32_t)s + 1u) r = prev;
            }
        }
        // ---- sequential sorted inserts, candidate order = adjacency order (UpdateKnnList semantics)
        // A full pool rejects every candidate at or beyond its last entry, and that entry only moves down while the step's
        // candidates are inserted: those are dropped here, before the one-at-a-time loop (most of them, once the pool has settled)
        const unsigned long long evaluated = __ballot(fresh && sub == 3u);
        comps += (uint32_t)__builtin_popcountll(evaluated);
        const float worst = (L >= cap) ? __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(pdist), (int)(cap - 1u))) : R3DM_INF;
        unsigned long long todo = __ballot(fresh && sub == 3u && (r < worst || L < cap));
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            const float cd = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(r), src));
            const uint32_t ci = (uint32_t)__builtin_amdgcn_readlane((int)cid, src);
            const uint32_t cM = (uint32_t)__builtin_amdgcn_readlane((int)cdeg, src);
            const uint32_t rk = (uint32_t)__builtin_popcountll(__ballot(lane < L && pdist <= cd));
            if (rk >= cap) continue;
            const float sd = __shfl_up(pdist, 1);
            const uint32_t si = (uint32_t)__shfl_up((int)pid, 1);
            const uint32_t sm = (uint32_t)__shfl_up((int)pm, 1);
            const uint32_t sM = (uint32_t)__shfl_up((int)pM, 1);
            const int sf = __shfl_up((int)pflag, 1);
            if (lane > rk) { pdist = sd; pid = si; pm = sm; pM = sM; pflag = sf != 0; }
            if (lane == rk) { pdist = cd; pid = ci; pm = 0; pM = cM; pflag = true; }
            if (L < cap) ++L;
        }
    }

#if R3DM_ANN_KNN
    // ---- results: the pool is the answer (KGraphImpl::search copies its first K entries out, kgraph.cpp:540-551)
    {
        const size_t o = (size_t)pair * P.q_stride + q;
        if (lane < k) {
            P.knn_idx[o * k + lane] = lane < L ? (int32_t)pid : -1;
            P.knn_dist[o * k + lane] = lane < L ? pdist : R3DM_INF;
        }
        if (lane == 0) { P.nn_idx[o] = kNone; atomicAdd(P.n_comps, (unsigned long long)comps); }
    }
#else
    // ---- results: the two best pool entries; distance-ratio test (squared metric: R = ratio^2)
    const float d0 = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(pdist), 0));
    const float d1 = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(pdist), 1));
    const uint32_t i0 = (uint32_t)__builtin_amdgcn_readlane((int)pid, 0);
    const uint32_t i1 = (uint32_t)__builtin_amdgcn_readlane((int)pid, 1);
    if (lane == 0) {
        const size_t o = (size_t)pair * P.q_stride + q;
        const bool two = L >= 2;
        P.nn_idx[o] = (two && d0 < P.ratio_R * d1) ? i0 : kNone;
        if (P.knn_idx) {
            P.knn_idx[2 * o] = L >= 1 ? (int32_t)i0 : -1; P.knn_idx[2 * o + 1] = two ? (int32_t)i1 : -1;
            P.knn_dist[2 * o] = L >= 1 ? d0 : R3DM_INF;   P.knn_dist[2 * o + 1] = two ? d1 : R3DM_INF;
        }
        atomicAdd(P.n_comps, (unsigned long long)comps);
    }
#endif
