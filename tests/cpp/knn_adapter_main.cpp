// knn_adapter_main.cpp -- the matcher-plugin slot (include/r3dm_array_matcher.hpp) asked for more than two neighbours, the way a
// host beyond MatchDistanceRatio asks its plugins (second-ratio tests, k-NN voting): SearchNeighbours(NN = 3), (NN = 8), the refused
// counts, and NN = 3 searches from an OpenMP loop against one Build.
//   knn_adapter_main <dataset.f32> <rows> <query.f32> <queries> <dim> <out prefix> <loop count>
// writes <prefix>.nn3 / .nn8 as text rows "query row, then NN x (dataset row, distance)" and prints
//   <NN = 9 refused> <NN > rows refused> <views staged before the loop> <views staged by the loop> <loop answers all equal>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "r3dm_array_matcher.hpp"

using Matcher = r3d_amd::ArrayMatcher_r3dm<float>;

static bool read_f32(const char* path, size_t count, std::vector<float>& v)
{
    v.resize(count);
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const size_t got = fread(v.data(), sizeof(float), count, f);
    fclose(f);
    return got == count;
}

static bool search(Matcher& m, const std::vector<float>& q, int nq, size_t NN, r3d_amd::IndMatches& idx, std::vector<float>& dist)
{
    idx.clear(); dist.clear();
    return m.SearchNeighbours(q.data(), nq, &idx, &dist, NN) && idx.size() == NN * (size_t)nq && dist.size() == idx.size();
}

static bool write_result(const std::string& path, int nq, size_t NN, const r3d_amd::IndMatches& idx, const std::vector<float>& dist)
{
    FILE* f = fopen(path.c_str(), "w");
    if (!f) return false;
    for (int q = 0; q < nq; ++q) {
        fprintf(f, "%u", idx[NN * q].i_);
        for (size_t k = 0; k < NN; ++k) fprintf(f, " %u %.9g", idx[NN * q + k].j_, dist[NN * q + k]);
        fprintf(f, "\n");
    }
    fclose(f);
    return true;
}

int main(int argc, char** argv)
{
    if (argc != 8) { fprintf(stderr, "usage: knn_adapter_main <dataset.f32> <rows> <query.f32> <queries> <dim> <out prefix> <loop count>\n"); return 2; }
    const int n = atoi(argv[2]), nq = atoi(argv[4]), dim = atoi(argv[5]), loops = atoi(argv[7]);
    const std::string prefix = argv[6];
    std::vector<float> a, b;
    if (!read_f32(argv[1], (size_t)n * dim, a) || !read_f32(argv[3], (size_t)nq * dim, b)) { fprintf(stderr, "cannot read the rows\n"); return 3; }

    Matcher m;
    if (!m.Build(a.data(), n, dim)) { fprintf(stderr, "Build failed\n"); return 4; }
    r3d_amd::IndMatches idx; std::vector<float> dist;
    for (size_t NN : {(size_t)3, (size_t)8}) {
        if (!search(m, b, nq, NN, idx, dist)) { fprintf(stderr, "SearchNeighbours(NN = %zu) failed\n", NN); return 5; }
        if (!write_result(prefix + (NN == 3 ? ".nn3" : ".nn8"), nq, NN, idx, dist)) return 6;
    }
    const bool refused9 = !search(m, b, nq, 9, idx, dist);
    Matcher small;
    if (!small.Build(a.data(), 5, dim)) { fprintf(stderr, "Build of 5 rows failed\n"); return 4; }
    const bool refused_rows = !search(small, b, nq, 6, idx, dist) && search(small, b, nq, 5, idx, dist);

    r3d_amd::IndMatches first; std::vector<float> first_d;
    if (!search(m, b, nq, 3, first, first_d)) return 5;
    const unsigned long long staged_before = m.viewsStaged();
    int same = 1;
#pragma omp parallel for schedule(dynamic) num_threads(8)
    for (int it = 0; it < loops; ++it) {
        r3d_amd::IndMatches li; std::vector<float> ld;
        bool ok = search(m, b, nq, 3, li, ld);
        for (size_t k = 0; ok && k < li.size(); ++k) ok = li[k].i_ == first[k].i_ && li[k].j_ == first[k].j_ && ld[k] == first_d[k];
        if (!ok) {
#pragma omp atomic write
            same = 0;
        }
    }
    printf("%d %d %llu %llu %d\n", refused9 ? 1 : 0, refused_rows ? 1 : 0, staged_before, (unsigned long long)m.viewsStaged() - staged_before, same);
    return 0;
}
