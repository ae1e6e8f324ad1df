// ann_adapter_main.cpp -- the three approximate matcher plugins (include/r3dm_ann_matchers.hpp) driven the way kgraph_match / hnsw_match
// / mrpt_match drive the reference's: one Build, SearchNeighbours(NN = 2) and (NN = 8), then NN = 8 searches from an OpenMP loop.
//   ann_adapter_main <dataset.f32> <rows> <query.f32> <queries> <dim> <out prefix> <loop count>
// writes <prefix>.<arm>.nn2 / .nn8 (arm = kgraph, hnsw, mrpt) as text rows "query row, dataset row, distance", one per emitted entry,
// and prints per arm
//   <NN = 9 refused> <NN > rows refused> <views staged by the loop> <loop answers all equal>
// and a last line <MRPT autotune refused>.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "r3dm_ann_matchers.hpp"

using r3d_amd::IndMatches;

static bool read_f32(const char* path, size_t count, std::vector<float>& v)
{
    v.resize(count);
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const size_t got = fread(v.data(), sizeof(float), count, f);
    fclose(f);
    return got == count;
}

static bool write_result(const std::string& path, const IndMatches& idx, const std::vector<float>& dist)
{
    FILE* f = fopen(path.c_str(), "w");
    if (!f) return false;
    for (size_t k = 0; k < idx.size(); ++k) fprintf(f, "%u %d %.9g\n", idx[k].i_, (int)idx[k].j_, dist[k]);
    fclose(f);
    return true;
}

// small: the same matcher type over 5 rows (NN = 6 must be refused, NN = 5 served)
template <class Matcher>
static int drive(const char* arm, Matcher& m, Matcher& small, const std::vector<float>& a, int n, const std::vector<float>& b, int nq, int dim,
                 const std::string& prefix, int loops)
{
    if (!m.Build(a.data(), n, dim)) { fprintf(stderr, "%s: Build failed\n", arm); return 4; }
    IndMatches idx; std::vector<float> dist;
    for (size_t NN : {(size_t)2, (size_t)8}) {
        idx.clear(); dist.clear();
        if (!m.SearchNeighbours(b.data(), nq, &idx, &dist, NN) || idx.size() != dist.size()) { fprintf(stderr, "%s: SearchNeighbours(NN = %zu) failed\n", arm, NN); return 5; }
        if (!write_result(prefix + "." + arm + (NN == 2 ? ".nn2" : ".nn8"), idx, dist)) return 6;
    }
    IndMatches first = idx; std::vector<float> first_d = dist;            // the NN = 8 answer
    idx.clear(); dist.clear();
    const bool refused9 = !m.SearchNeighbours(b.data(), nq, &idx, &dist, 9) && idx.empty();
    if (!small.Build(a.data(), 5, dim)) { fprintf(stderr, "%s: Build of 5 rows failed\n", arm); return 4; }
    const bool refused_rows = !small.SearchNeighbours(b.data(), nq, &idx, &dist, 6) && idx.empty() && small.SearchNeighbours(b.data(), nq, &idx, &dist, 5);
    const unsigned long long staged_before = m.viewsStaged();
    int same = 1;
#pragma omp parallel for schedule(dynamic) num_threads(8)
    for (int it = 0; it < loops; ++it) {
        IndMatches li; std::vector<float> ld;
        bool ok = m.SearchNeighbours(b.data(), nq, &li, &ld, 8) && li.size() == first.size();
        for (size_t k = 0; ok && k < li.size(); ++k) ok = li[k].i_ == first[k].i_ && li[k].j_ == first[k].j_ && ld[k] == first_d[k];
        if (!ok) {
#pragma omp atomic write
            same = 0;
        }
    }
    printf("%d %d %llu %d\n", refused9 ? 1 : 0, refused_rows ? 1 : 0, (unsigned long long)m.viewsStaged() - staged_before, same);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 8) { fprintf(stderr, "usage: ann_adapter_main <dataset.f32> <rows> <query.f32> <queries> <dim> <out prefix> <loop count>\n"); return 2; }
    const int n = atoi(argv[2]), nq = atoi(argv[4]), dim = atoi(argv[5]), loops = atoi(argv[7]);
    const std::string prefix = argv[6];
    std::vector<float> a, b;
    if (!read_f32(argv[1], (size_t)n * dim, a) || !read_f32(argv[3], (size_t)nq * dim, b)) { fprintf(stderr, "cannot read the rows\n"); return 3; }
    int rc;
    {
        r3dm_kgraph_params kp;
        r3dm_kgraph_preset(3, &kp);
        r3d_amd::ArrayMatcher_r3dm_kgraph<float> m(kp, 3, 9), small(kp, 3, 9);
        if ((rc = drive("kgraph", m, small, a, n, b, nq, dim, prefix, loops)) != 0) return rc;
    }
    {
        using H = r3d_amd::ArrayMatcher_r3dm_hnsw<float>;
        H::efConstruction_ = 112; H::ef_ = 5; H::M_ = 5;                 // the "fast" preset: NN = 8 widens its beam
        H m, small;
        if ((rc = drive("hnsw", m, small, a, n, b, nq, dim, prefix, loops)) != 0) return rc;
    }
    {
        r3d_amd::ArrayMatcher_r3dm_mrpt<float> m(26, 6, 4), small(26, 6, 4);
        if ((rc = drive("mrpt", m, small, a, n, b, nq, dim, prefix, loops)) != 0) return rc;
        r3d_amd::ArrayMatcher_r3dm_mrpt<float> tuned(26, 6, 5, true);
        IndMatches idx; std::vector<float> dist;
        printf("%d\n", (!tuned.Build(a.data(), n, dim) && !tuned.SearchNeighbours(b.data(), nq, &idx, &dist, 2)) ? 1 : 0);
    }
    return 0;
}
