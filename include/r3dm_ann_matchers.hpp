// r3dm_ann_matchers.hpp -- the reference's three approximate matcher plugins, served by the GPU library.
//
// ArrayMatcher_r3dm_kgraph / _hnsw / _mrpt have the shape of the reference's ArrayMatcher_kgraph / _hnsw / _mrpt
// (/root/reference/src/utils/matcher_kgraph.h:34-260, matcher_hnsw.h:34-206, matcher_mrpt.h:45-259) and drop into
// `RegionsMatcherT<...>` where those stand (kgraph_match / hnsw_match / mrpt_match, /root/reference/src/R3DComputeMatches.cpp:
// 808-902, 497-593, 423-491; INTEGRATION.md shows the three bodies).  Same stand-in types and R3DM_WITH_OPENMVG switch as
// r3dm_array_matcher.hpp, which serves the exhaustive matcher.
//
// Build() stages the dataset ONCE (r3dm_index_create); the arm's structure -- the K-NN graph, the HNSW graph, the forest -- is built
// on the index by the first SearchNeighbours and kept (r3dm_index_kgraph_knn / _hnsw_knn / _mrpt_knn); every later search uploads its
// query rows only.  Any NN up to R3DM_KNN_MAX (8) is served, as the reference's plugins serve it (`sparams.K = NN`,
// `searchKnn(q, NN)`, `query(q, NN, votes)`): the search itself depends on NN (pool of NN + P entries; beam max(ef, NN); retry when
// fewer than NN rows were elected).  NN > 8 or NN > nbRows: `false`.  A dataset of fewer than 128 rows is answered exactly.
//   ArrayMatcher_r3dm_kgraph   emits NN entries per query, ascending; a pool that ran short leaves (row 0xFFFFFFFF, +inf) behind
//   ArrayMatcher_r3dm_hnsw     emits NN entries per query, ascending by (distance, row); the same for rows the search did not find
//   ArrayMatcher_r3dm_mrpt     emits NN entries for a query with NN elected rows and NOTHING for a dropped one (`if(isValid)`,
//                              matcher_mrpt.h:235-243); distances are square roots.  The reference's autotune mode (autotune_,
//                              targetRecall_, treesMax_: Mrpt::grow_autotune) is NOT served: a matcher constructed with autotune = true
//                              refuses Build and every search.
// Build parameters are read when Build is called and belong to the index from then on (KGraph: index_K; HNSW: M_, efConstruction_;
// MRPT: trees, depth); search parameters are read at every search (search_P / search_S / seed; ef_; votes).
//
// Binary rows: ArrayMatcher_r3dm_kgraph<unsigned char, Metric> with a Hamming metric -- the tag type r3d_amd::HammingMetric, or
// openMVG::matching::Hamming<unsigned char> under R3DM_WITH_OPENMVG -- stages its rows as R3DM_BIN (`dimension` bytes per row: 29..32 or
// 61..64) and searches the Hamming graph index (r3dm_set_kgraph_hamming, switched on in the leased context for the length of the search);
// distances are the Hamming counts.  The reference's plugin is generic in its metric in the same way (matcher_kgraph.h:33-37,60,90).  With
// any other metric unsigned char rows are R3DM_U8 under L2, as before.  The HNSW and MRPT plugins serve no Hamming metric: hnswlib's
// L2Space is hard-wired (matcher_hnsw.h:70), MRPT projects floats.
//
// Thread-safety: as r3dm_array_matcher.hpp -- the reference calls SearchNeighbours from many OpenMP threads; a context drives one HIP
// stream and owns its scratch, so every call leases a context from the process-wide pool of its device and concurrent searches run on
// different streams.  The FIRST search of an index builds the arm's structure under the index's lock: concurrent first searches wait
// for the one that builds, none builds twice.  Build and the destructor must not run beside a search of the same matcher (the
// reference's plugins have the same rule).  The static parameters of ArrayMatcher_r3dm_hnsw are plain ints, as the reference's: set
// them before Build, not beside it.
#pragma once

#include <cstdint>
#include <type_traits>
#include <vector>

#include "r3dm.h"
#include "r3dm_array_matcher.hpp"    // IndMatch / IndMatches / DefaultMetric / R3DM_ARRAY_MATCHER_BASE, the context pool

namespace r3d_amd {

// the Hamming metric of ArrayMatcher_r3dm_kgraph<unsigned char, ...> where OpenMVG's Hamming<unsigned char> is not at hand
struct HammingMetric { using ElementType = unsigned char; using ResultType = unsigned; };

namespace detail {

template <typename Metric> struct is_hamming_metric : std::false_type {};
template <> struct is_hamming_metric<HammingMetric> : std::true_type {};
#ifdef R3DM_WITH_OPENMVG
template <typename T> struct is_hamming_metric<openMVG::matching::Hamming<T>> : std::true_type {};
#endif

// what the three classes share: the staged dataset and the emission of an index search's k-lists
class AnnMatcherCore {
public:
    explicit AnnMatcherCore(int device_id) : pool_(ContextPool::of(device_id)) {}
    ~AnnMatcherCore() { if (index_) r3dm_index_destroy(index_); }
    AnnMatcherCore(const AnnMatcherCore&) = delete;
    AnnMatcherCore& operator=(const AnnMatcherCore&) = delete;

    // binary: unsigned char rows under a Hamming metric -> R3DM_BIN (dimension = bytes per row)
    template <typename Scalar>
    bool build(const Scalar* dataset, int nbRows, int dimension, bool binary = false)
    {
        if (nbRows < 1 || dimension < 1 || !dataset) return false;     // matcher_kgraph.h:126-130
        ContextLease lease(pool_);
        if (!lease.ctx) return false;
        if (index_) { r3dm_index_destroy(index_); index_ = nullptr; }
        const r3dm_dtype dt = sizeof(Scalar) == 1 ? (binary ? R3DM_BIN : R3DM_U8) : R3DM_F32;
        nbRows_ = nbRows;
        return r3dm_index_create(lease.ctx, dataset, static_cast<uint32_t>(nbRows), static_cast<uint32_t>(dimension), dt, &index_) == R3DM_OK;
    }

    // search(ctx, index, idx, dist) -> R3DM_OK: the arm's r3dm_index_*_knn; skip_dropped: a query whose first row is -1 emits nothing
    template <typename DistanceType, class Search>
    bool neighbours(const void* query, int nbQuery, IndMatches* pvec_indices, std::vector<DistanceType>* pvec_distances, size_t NN,
                    bool skip_dropped, Search&& search)
    {
        if (!index_ || !query || nbQuery < 1 || NN < 1 || NN > R3DM_KNN_MAX || NN > static_cast<size_t>(nbRows_)) return false;
        std::vector<int32_t> idx(NN * static_cast<size_t>(nbQuery));
        std::vector<float> dist(NN * static_cast<size_t>(nbQuery));
        {
            ContextLease lease(pool_);                         // one stream + scratch per concurrent search
            if (!lease.ctx) return false;
            if (search(lease.ctx, index_, idx.data(), dist.data()) != R3DM_OK) return false;
        }
        pvec_indices->reserve(pvec_indices->size() + nbQuery * NN);
        pvec_distances->reserve(pvec_distances->size() + nbQuery * NN);
        for (int q = 0; q < nbQuery; ++q) {
            if (skip_dropped && idx[NN * q] < 0) continue;
            for (size_t k = 0; k < NN; ++k) {
                pvec_indices->emplace_back(static_cast<uint32_t>(q), static_cast<uint32_t>(idx[NN * q + k]));
                pvec_distances->emplace_back(static_cast<DistanceType>(dist[NN * q + k]));
            }
        }
        return true;
    }

    uint64_t viewsStaged() const { return pool_.viewsStaged(); }

private:
    ContextPool& pool_;
    r3dm_index* index_ = nullptr;
    int nbRows_ = 0;
};

}  // namespace detail

// ---- ArrayMatcher_kgraph (matcher_kgraph.h): index parameters and search parameters in the constructor
template <typename Scalar = float, typename Metric = DefaultMetric<Scalar>>
class ArrayMatcher_r3dm_kgraph R3DM_ARRAY_MATCHER_BASE(Scalar, Metric) {
public:
    using DistanceType = typename Metric::ResultType;

    // params: r3dm_kgraph_preset(0 fast / 1 medium / 2 precise / other: the reference's default block); pair_i / pair_j key the
    // start-row stream of the searches (the view ids of r3dm_match_pairs_kgraph)
    explicit ArrayMatcher_r3dm_kgraph(const r3dm_kgraph_params& params, uint32_t pair_i = 0, uint32_t pair_j = 1, int device_id = 0)
        : core_(device_id), params_(params), pair_i_(pair_i), pair_j_(pair_j) {}
    explicit ArrayMatcher_r3dm_kgraph(int preset = 3, int device_id = 0) : core_(device_id) { (void)r3dm_kgraph_preset(preset, &params_); }
    virtual ~ArrayMatcher_r3dm_kgraph() = default;
    uint64_t viewsStaged() const { return core_.viewsStaged(); }        // not part of the ArrayMatcher interface (test / diagnostics hook)

    // unsigned char rows under a Hamming metric are binary rows (R3DM_BIN) on the Hamming graph index
    static constexpr bool kHamming = sizeof(Scalar) == 1 && detail::is_hamming_metric<Metric>::value;

    bool Build(const Scalar* dataset, int nbRows, int dimension) R3DM_OVERRIDE { return core_.build(dataset, nbRows, dimension, kHamming); }

    bool SearchNeighbour(const Scalar* query, int* indice, DistanceType* distance) R3DM_OVERRIDE
    {
        IndMatches idx; std::vector<DistanceType> dist;
        if (!SearchNeighbours(query, 1, &idx, &dist, 1) || idx.empty()) return false;
        indice[0] = static_cast<int>(idx[0].j_); distance[0] = dist[0];
        return true;
    }

    bool SearchNeighbours(const Scalar* query, int nbQuery, IndMatches* pvec_indices, std::vector<DistanceType>* pvec_distances, size_t NN) R3DM_OVERRIDE
    {
        return core_.neighbours(query, nbQuery, pvec_indices, pvec_distances, NN, false,
                                [&](r3dm_ctx* c, const r3dm_index* ix, int32_t* idx, float* dist) {
            // (the lease is exclusive: the pooled context serves binary indices for this search only)
            if (kHamming) (void)r3dm_set_kgraph_hamming(c, 1);
            const int rc = r3dm_index_kgraph_knn(c, ix, &params_, query, static_cast<uint32_t>(nbQuery), pair_i_, pair_j_, static_cast<uint32_t>(NN), idx, dist);
            if (kHamming) (void)r3dm_set_kgraph_hamming(c, 0);
            return rc;
        });
    }

private:
    detail::AnnMatcherCore core_;
    r3dm_kgraph_params params_{};
    uint32_t pair_i_ = 0, pair_j_ = 1;
};

// ---- ArrayMatcher_hnsw (matcher_hnsw.h): the reference's static efConstruction_ / ef_ / M_ (set by hnsw_match per preset,
// src/R3DComputeMatches.cpp:533-565; defaults here: the "precise" preset)
template <typename Scalar = float, typename Metric = DefaultMetric<Scalar>>
class ArrayMatcher_r3dm_hnsw R3DM_ARRAY_MATCHER_BASE(Scalar, Metric) {
public:
    using DistanceType = typename Metric::ResultType;

    explicit ArrayMatcher_r3dm_hnsw(int device_id = 0) : core_(device_id) {}
    virtual ~ArrayMatcher_r3dm_hnsw() = default;
    uint64_t viewsStaged() const { return core_.viewsStaged(); }        // not part of the ArrayMatcher interface

    bool Build(const Scalar* dataset, int nbRows, int dimension) R3DM_OVERRIDE
    {
        if (M_ < 2 || efConstruction_ < 0) return false;
        built_.M = static_cast<uint32_t>(M_); built_.ef_construction = static_cast<uint32_t>(efConstruction_); built_.seed = 100;     // hnswalg.h:55
        return core_.build(dataset, nbRows, dimension);
    }

    bool SearchNeighbour(const Scalar* query, int* indice, DistanceType* distance) R3DM_OVERRIDE
    {
        IndMatches idx; std::vector<DistanceType> dist;
        if (!SearchNeighbours(query, 1, &idx, &dist, 1) || idx.empty()) return false;
        indice[0] = static_cast<int>(idx[0].j_); distance[0] = dist[0];
        return true;
    }

    bool SearchNeighbours(const Scalar* query, int nbQuery, IndMatches* pvec_indices, std::vector<DistanceType>* pvec_distances, size_t NN) R3DM_OVERRIDE
    {
        if (ef_ < 1) return false;
        r3dm_hnsw_params hp = built_;                          // (the index was built from M_ / efConstruction_ as Build read them)
        hp.ef = static_cast<uint32_t>(ef_);
        return core_.neighbours(query, nbQuery, pvec_indices, pvec_distances, NN, false,
                                [&](r3dm_ctx* c, const r3dm_index* ix, int32_t* idx, float* dist) {
            return r3dm_index_hnsw_knn(c, ix, &hp, query, static_cast<uint32_t>(nbQuery), static_cast<uint32_t>(NN), idx, dist);
        });
    }

    inline static int efConstruction_ = 100;
    inline static int ef_ = 15;
    inline static int M_ = 19;

private:
    detail::AnnMatcherCore core_;
    r3dm_hnsw_params built_{};
};

// ---- ArrayMatcher_mrpt (matcher_mrpt.h): trees, depth and votes; no autotune
template <typename Scalar = float, typename Metric = DefaultMetric<Scalar>>
class ArrayMatcher_r3dm_mrpt R3DM_ARRAY_MATCHER_BASE(Scalar, Metric) {
public:
    using DistanceType = typename Metric::ResultType;

    // defaults: mrpt_match's (26, 6, 5), src/R3DComputeMatches.cpp:453-455.  autotune = true is refused (see the header comment)
    explicit ArrayMatcher_r3dm_mrpt(int n_trees = 26, int depth = 6, int votes = 5, bool autotune = false, int device_id = 0)
        : core_(device_id), autotune_(autotune)
    {
        (void)r3dm_mrpt_preset(&params_);                      // density and seed of the preset
        params_.n_trees = static_cast<uint32_t>(n_trees); params_.depth = static_cast<uint32_t>(depth); params_.votes = static_cast<uint32_t>(votes);
    }
    virtual ~ArrayMatcher_r3dm_mrpt() = default;
    void setVotes(int votes) { params_.votes = static_cast<uint32_t>(votes); }          // a search parameter: free per search
    uint64_t viewsStaged() const { return core_.viewsStaged(); }        // not part of the ArrayMatcher interface

    bool Build(const Scalar* dataset, int nbRows, int dimension) R3DM_OVERRIDE
    {
        if (autotune_) return false;
        return core_.build(dataset, nbRows, dimension);
    }

    // Mrpt::query(q, 1, votes): the row may be -1 (no elected row), as in the reference
    bool SearchNeighbour(const Scalar* query, int* indice, DistanceType* distance) R3DM_OVERRIDE
    {
        IndMatches idx; std::vector<DistanceType> dist;
        if (!SearchNeighbours(query, 1, &idx, &dist, 1)) return false;
        indice[0] = idx.empty() ? -1 : static_cast<int>(idx[0].j_); distance[0] = idx.empty() ? static_cast<DistanceType>(-1) : dist[0];
        return true;
    }

    bool SearchNeighbours(const Scalar* query, int nbQuery, IndMatches* pvec_indices, std::vector<DistanceType>* pvec_distances, size_t NN) R3DM_OVERRIDE
    {
        if (autotune_) return false;
        return core_.neighbours(query, nbQuery, pvec_indices, pvec_distances, NN, true,
                                [&](r3dm_ctx* c, const r3dm_index* ix, int32_t* idx, float* dist) {
            return r3dm_index_mrpt_knn(c, ix, &params_, query, static_cast<uint32_t>(nbQuery), static_cast<uint32_t>(NN), idx, dist);
        });
    }

private:
    detail::AnnMatcherCore core_;
    r3dm_mrpt_params params_{};
    bool autotune_ = false;
};

}  // namespace r3d_amd
