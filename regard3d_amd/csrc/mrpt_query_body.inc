// mrpt_query_body.inc -- the body of the MRPT query kernels (kernels_mrpt.hip), included once per tail:
//   R3DM_MRPT_KNN 0   mrpt_query_kernel(P): Mrpt::query(q, 2, votes) with the adapter's retry, the ratio test
//   R3DM_MRPT_KNN 1   mrpt_query_knn_kernel(P, k): Mrpt::query(q, k, votes); the election is the same, the retry asks for k elected
//                     rows instead of two, the re-rank keeps the k nearest by (distance, row)
// One text for both kernels; an include rather than a shared function, so that the 2-NN kernel keeps its machine code.
    extern __shared__ __attribute__((aligned(16))) unsigned char mr_smem[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const MrptQueryJob job = P.jobs[blockIdx.y];
    const uint32_t qi = blockIdx.x * P.waves + wave;
    if (qi >= job.nq) return;                                                 // (no workgroup barrier below)
    const MrptView ix = job.ix;
    const uint32_t n = ix.n, dim = ix.dim, depth = ix.depth, n_trees = ix.n_trees, n_pool = n_trees * depth;
    unsigned char* base = mr_smem + (size_t)wave * P.per_wave;
    float* pq = reinterpret_cast<float*>(base);
    uint32_t* leaf = reinterpret_cast<uint32_t*>(base + P.pool_pad * 4u);
    uint32_t* cnt = leaf + 256;                                               // (n_trees <= 255)
    uint32_t* elected = cnt + 2;
    uint32_t* votes = elected + P.elected_cap;
    const uint32_t vote_words = (P.max_n + 3u) / 4u;
    const float* q = job.query + (size_t)qi * dim;
    const size_t o = (size_t)job.out_base + qi;

    // project: output j = lane, lane + 64, ...; RT [dim][n_pool]: the lanes read consecutive j
    for (uint32_t j = lane; j < n_pool; j += 64u) {
        float acc = 0.0f;
        for (uint32_t c = 0; c < dim; ++c) { const float tt = ix.RT[(size_t)c * n_pool + j] * q[c]; acc = acc + tt; }
        pq[j] = acc;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // route: a lane per tree
    const uint32_t n_nodes_all = (1u << depth) - 1u;
    for (uint32_t t = lane; t < n_trees; t += 64u) {
        uint32_t node = 0;
        for (uint32_t d = 0; d < depth; ++d) {
            const float sp = ix.splits[(size_t)t * n_nodes_all + node];
            node = (pq[t * depth + d] <= sp) ? 2u * node + 1u : 2u * node + 2u;
        }
        leaf[t] = node - n_nodes_all;
    }
#if R3DM_MRPT_KNN
    TopK<R3DM_KNN_MAX> kl;
    uint32_t n_found = 0;
#else
    uint32_t i0 = kNoneM, i1 = kNoneM; float d0 = 0.f, d1 = 0.f;
#endif
    uint32_t need = P.votes;
    for (int attempt = 0; attempt < 2; ++attempt) {
        for (uint32_t w = lane; w < vote_words; w += 64u) votes[w] = 0u;
        if (lane == 0) cnt[0] = 0u;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (uint32_t t = 0; t < n_trees; ++t) {
            const uint32_t lf = leaf[t];
            const uint32_t b = (uint32_t)ix.leaf_first[lf], e = (uint32_t)ix.leaf_first[lf + 1u];
            const int32_t* rows_t = ix.leaves + (size_t)t * n;
            for (uint32_t a = b + lane; a < e; a += 64u) {
                const uint32_t r = (uint32_t)rows_t[a];
                const uint32_t sh = 8u * (r & 3u);
                const uint32_t old = atomicAdd(&votes[r >> 2], 1u << sh);     // a row occurs once per tree: no two lanes of this step share a byte
                if (((old >> sh) & 255u) + 1u == need) { const uint32_t pos = atomicAdd(&cnt[0], 1u); if (pos < P.elected_cap) elected[pos] = r; }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint32_t ne = min(cnt[0], P.elected_cap);
#if R3DM_MRPT_KNN
        // the k nearest of the elected rows by (distance, row): a sorted list per lane, merged across the wavefront after the retry
        topk_init(kl);
        for (uint32_t e = lane; e < ne; e += 64u) {
            const uint32_t r = elected[e];
            topk_push_lex(kl, mr_l2sq(ix.rows + (size_t)r * dim, q, dim), r);
        }
        if (lane == 0) atomicAdd(P.n_comps, (unsigned long long)ne);
        n_found = ne;
        if (ne >= k || need <= 1u) break;                                 // wave-uniform; Mrpt::query leaves -1 behind fewer than k elected rows
        need -= 1u;                                                       // ArrayMatcher_mrpt: "Try again" with votes - 1
#else
        // the two nearest of the elected rows by (distance, row)
        i0 = kNoneM; i1 = kNoneM; d0 = 0.f; d1 = 0.f;
        for (uint32_t k = lane; k < ne; k += 64u) {
            const uint32_t r = elected[k];
            const float d = mr_l2sq(ix.rows + (size_t)r * dim, q, dim);
            if (i0 == kNoneM || d < d0 || (d == d0 && r < i0)) { i1 = i0; d1 = d0; i0 = r; d0 = d; }
            else if (i1 == kNoneM || d < d1 || (d == d1 && r < i1)) { i1 = r; d1 = d; }
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            const uint32_t oi0 = mr_shfl_xor(i0, m), oi1 = mr_shfl_xor(i1, m);
            const float od0 = mr_shfl_xor(d0, m), od1 = mr_shfl_xor(d1, m);
            // merge two sorted pairs (mine, other) -> the two smallest by (d, i)
            uint32_t c_i[4] = {i0, i1, oi0, oi1}; float c_d[4] = {d0, d1, od0, od1};
            uint32_t b0 = kNoneM, b1 = kNoneM; float e0 = 0.f, e1 = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t r = c_i[u]; const float d = c_d[u];
                if (r == kNoneM) continue;
                if (b0 == kNoneM || d < e0 || (d == e0 && r < b0)) { b1 = b0; e1 = e0; b0 = r; e0 = d; }
                else if (b1 == kNoneM || d < e1 || (d == e1 && r < b1)) { b1 = r; e1 = d; }
            }
            i0 = b0; i1 = b1; d0 = e0; d1 = e1;
        }
        if (lane == 0) atomicAdd(P.n_comps, (unsigned long long)ne);
        if ((i0 != kNoneM && i1 != kNoneM) || need <= 1u) break;               // wave-uniform
        need -= 1u;                                                           // ArrayMatcher_mrpt: "Try again" with votes - 1
#endif
    }
#if R3DM_MRPT_KNN
    // a query still short of k rows is dropped (!isValid): k entries of -1 / -1
    const bool ok = n_found >= k;
    topk_wave_select(kl, k, [&](uint32_t j, float d, uint32_t r) {
        if (lane == 0) {
            P.knn_idx[o * k + j] = ok ? (int32_t)r : -1;
            P.knn_dist[o * k + j] = ok ? sqrtf(d) : -1.0f;
        }
    });
    if (lane == 0) P.nn_idx[o] = kNoneM;
#else
    if (lane == 0) {
        const bool two = i0 != kNoneM && i1 != kNoneM;
        const float s0 = two ? sqrtf(d0) : -1.0f, s1 = two ? sqrtf(d1) : -1.0f;
        P.nn_idx[o] = (two && s0 < P.ratio * s1) ? i0 : kNoneM;
        if (P.knn_idx) {
            P.knn_idx[2 * o] = two ? (int32_t)i0 : -1; P.knn_idx[2 * o + 1] = two ? (int32_t)i1 : -1;
            P.knn_dist[2 * o] = s0; P.knn_dist[2 * o + 1] = s1;
        }
    }
#endif
