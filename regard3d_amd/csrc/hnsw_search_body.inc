// hnsw_search_body.inc -- the body of the wavefront-per-query HNSW search kernels (kernels_hnsw.hip), included once per tail:
//   R3DM_HNSW_KNN 0   hnsw_search_kernel<NB, ROW>(P): searchKnn(query, 2) and the ratio test
//   R3DM_HNSW_KNN 1   hnsw_search_knn_kernel<NB, ROW>(P, k): searchKnn(query, k), the k-list
// P.ef is the beam of the whole search, max(ef_, k) as hnswlib widens it (hnswalg.h:765): the two heap tests, the LDS carve-up below
// and the launcher's LDS size all read that one number.  One text for both kernels; an include rather than a shared function, so that
// the 2-NN kernels keep their machine code (a body function taking the parameter block loses the address spaces of its pointers).
    extern __shared__ unsigned char hn_smem[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const HnswSearchJob job = P.jobs[blockIdx.y];
    const uint32_t qi = blockIdx.x * 4 + wave;
    // per-wave LDS: visited bits | top heap (ef + 1) | candidate heap (cand_cap) | dist[64] | ids[64] | todo[64]
    const uint32_t per_wave = P.flag_words * 4 + (P.ef + 1) * 8 + P.cand_cap * 8 + 64 * 4 + 64 * 4 + 64 * 4;
    unsigned char* base = hn_smem + (size_t)wave * per_wave;
    uint32_t* visited = reinterpret_cast<uint32_t*>(base);
    HnPair* top = reinterpret_cast<HnPair*>(base + P.flag_words * 4);
    HnPair* cand = top + (P.ef + 1);
    float* dist = reinterpret_cast<float*>(cand + P.cand_cap);
    int32_t* ids = reinterpret_cast<int32_t*>(dist + 64);
    int32_t* todo = ids + 64;
    if (qi >= job.nq) return;                                            // (no workgroup barrier below)
    const HnswView ix = job.ix;
    const uint32_t dim = ix.dim, M = ix.M, l = lane & 7u;
    const ROW* __restrict__ xrows = sizeof(ROW) == 1 ? reinterpret_cast<const ROW*>(ix.rows8) : reinterpret_cast<const ROW*>(ix.rows);
    const size_t o = (size_t)job.out_base + qi;

    float q[NB];
    hn_load_q<NB>(q, job.query + (size_t)qi * dim, l);
    for (uint32_t w = lane; w < P.flag_words; w += 64) visited[w] = 0;
    unsigned long long evals = 1;

    uint32_t cur = (uint32_t)ix.enter;
    float curdist = hn_hsum8(hn_acc<NB, ROW>(q, xrows + (size_t)cur * dim, l), lane);
    curdist = __shfl(curdist, 0);
    // greedy descent (hnswalg.h:745-768): the list is walked in order, every strictly closer row takes over
    for (int level = ix.maxlevel; level > 0; --level) {
        bool changed = true;
        while (changed) {
            changed = false;
            const int32_t* L = ix.up + ((size_t)ix.up_off[cur] + (uint32_t)(level - 1)) * (1 + M);
            const uint32_t size = (uint32_t)L[0];
            hn_dist_list<NB, ROW>(q, xrows, dim, L + 1, size, dist, lane, [](uint32_t) { return false; });
            HN_SYNC();
            evals += size;
            for (uint32_t j = 0; j < size; ++j) {
                const float d = dist[j];
                if (d < curdist) { curdist = d; cur = (uint32_t)L[1 + j]; changed = true; }
            }
            HN_SYNC();
        }
    }
    // searchBaseLayerST (hnswalg.h:214-280)
    const uint32_t ef = P.ef;
    uint32_t n_top = 0, n_cand = 0;
    bool overflow = false;
    HN_SYNC();
    if (lane == 0) visited[cur >> 5] |= 1u << (cur & 31u);
    hn_push(top, n_top, curdist, cur);
    hn_push(cand, n_cand, -curdist, cur);
    float lower = curdist;
    HN_SYNC();
    while (n_cand) {
        const HnPair c0 = cand[0];
        if ((-c0.d) > lower) break;
        hn_pop(cand, n_cand);
        const int32_t* L = ix.l0 + (size_t)c0.id * (1 + 2 * M);
        const uint32_t size = (uint32_t)L[0];
        HN_SYNC();
        if (lane < size) ids[lane] = L[1 + lane];                       // 2M <= 64 links
        HN_SYNC();
        uint32_t n_walk = size;
        if (P.dense_steps) hn_dist_list<NB, ROW>(q, xrows, dim, ids, size, dist, lane, [&](uint32_t c) { return ((visited[c >> 5] >> (c & 31u)) & 1u) != 0; });
        else n_walk = hn_dist_list_unvisited<NB, ROW>(q, xrows, dim, ids, size, dist, todo, visited, lane);
        HN_SYNC();
        // the walk over the list in link order; links that were visited before the hop are no-ops in hnswlib's loop, so only the others
        // (todo, ascending) are walked -- a row that occurs twice in a list is in todo twice and the second visit finds it marked
        for (uint32_t k = 0; k < n_walk; ++k) {
            const uint32_t j = P.dense_steps ? k : (uint32_t)todo[k];
            const uint32_t c = (uint32_t)ids[j];
            const uint32_t w = visited[c >> 5], bit = 1u << (c & 31u);
            if (w & bit) continue;                                     // seen before this list, or earlier in this list
            visited[c >> 5] = w | bit;
            evals += 1;
            const float d = dist[j];
            if (top[0].d > d || n_top < ef) {
                if (n_cand >= P.cand_cap) { overflow = true; break; }
                hn_push(cand, n_cand, -d, c);
                hn_push(top, n_top, d, c);
                if (n_top > ef) hn_pop(top, n_top);
                lower = top[0].d;
            }
        }
        if (overflow) break;
    }
    if (overflow) {                                                     // the host repeats the query with a larger heap
        if (lane == 0) { atomicAdd(P.n_overflow, 1u); P.nn_idx[o] = kNone - 1u; }
        return;
    }
#if R3DM_HNSW_KNN
    // searchKnn pops the beam down to k (CompareByFirst: the sift order decides between equally distant rows), its `results` queue
    // and ArrayMatcher_hnsw's std::reverse order what is left ascending by (distance, row); rows the search did not find: -1 / +inf
    while (n_top > k) hn_pop(top, n_top);
    HN_SYNC();
    const uint32_t nr = n_top;                                         // <= k <= R3DM_KNN_MAX: a lane per entry
    if (lane < k) {
        if (lane < nr) {
            const HnPair mine = top[lane];
            uint32_t rank = 0;
            for (uint32_t j = 0; j < nr; ++j) {
                const HnPair t = top[j];
                rank += (t.d < mine.d || (t.d == mine.d && t.id < mine.id)) ? 1u : 0u;      // rows are unique: so are the ranks
            }
            P.knn_idx[o * k + rank] = (int32_t)mine.id;
            P.knn_dist[o * k + rank] = mine.d;
        } else {
            P.knn_idx[o * k + lane] = -1;
            P.knn_dist[o * k + lane] = R3DM_INF;
        }
    }
    if (lane == 0) { P.nn_idx[o] = kNone; atomicAdd(P.n_comps, evals); }
#else
    while (n_top > 2) hn_pop(top, n_top);
    // results as ArrayMatcher_hnsw::SearchNeighbours orders them: ascending (distance, row)
    HnPair r0{0.f, kNone}, r1{0.f, kNone};
    const uint32_t nr = n_top;
    if (nr >= 1) { r0 = top[0]; hn_pop(top, n_top); }
    if (nr == 2) {
        r1 = top[0];
        if (r1.d < r0.d || (!(r0.d < r1.d) && r1.id < r0.id)) { const HnPair t = r0; r0 = r1; r1 = t; }
    }
    if (lane == 0) {
        const bool two = nr == 2;
        P.nn_idx[o] = (two && r0.d < P.ratio_R * r1.d) ? r0.id : kNone;
        if (P.knn_idx) {
            P.knn_idx[2 * o] = nr >= 1 ? (int32_t)r0.id : -1; P.knn_idx[2 * o + 1] = two ? (int32_t)r1.id : -1;
            P.knn_dist[2 * o] = nr >= 1 ? r0.d : R3DM_INF;   P.knn_dist[2 * o + 1] = two ? r1.d : R3DM_INF;
        }
        atomicAdd(P.n_comps, evals);
    }
#endif
