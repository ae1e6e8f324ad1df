// knn_narrow_adapter_main.cpp -- the matcher-plugin slot (include/r3dm_array_matcher.hpp) asked for more than two neighbours with
// setKnnNarrowTiles(true): ArrayMatcher_r3dm<float> and ArrayMatcher_r3dm<unsigned char>, SearchNeighbours(NN = 3) and (NN = 8),
// then NN = 3 searches from an OpenMP loop against one Build, and the same search with the switch off.
//   knn_narrow_adapter_main <f32|u8> <dataset file> <rows> <query file> <queries> <dim> <out prefix> <loop count>
// writes <prefix>.nn3 / .nn8 as text rows "query row, then NN x (dataset row, distance)" and prints
//   <views staged by the loop> <loop answers all equal> <the switch-off answer equals the switch-on answer>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "r3dm_array_matcher.hpp"

template <typename T>
static bool read_rows(const char* path, size_t count, std::vector<T>& v)
{
    v.resize(count);
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const size_t got = fread(v.data(), sizeof(T), count, f);
    fclose(f);
    return got == count;
}

template <typename M, typename T>
static bool search(M& m, const std::vector<T>& q, int nq, size_t NN, r3d_amd::IndMatches& idx, std::vector<float>& dist)
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

static bool same_answer(const r3d_amd::IndMatches& a, const std::vector<float>& da, const r3d_amd::IndMatches& b, const std::vector<float>& db)
{
    bool ok = a.size() == b.size() && da.size() == db.size();
    for (size_t k = 0; ok && k < a.size(); ++k) ok = a[k].i_ == b[k].i_ && a[k].j_ == b[k].j_ && da[k] == db[k];
    return ok;
}

template <typename T>
static int run(char** argv)
{
    using Matcher = r3d_amd::ArrayMatcher_r3dm<T>;
    const int n = atoi(argv[3]), nq = atoi(argv[5]), dim = atoi(argv[6]), loops = atoi(argv[8]);
    const std::string prefix = argv[7];
    std::vector<T> a, b;
    if (!read_rows(argv[2], (size_t)n * dim, a) || !read_rows(argv[4], (size_t)nq * dim, b)) { fprintf(stderr, "cannot read the rows\n"); return 3; }

    Matcher m;
    m.setKnnNarrowTiles(true);
    if (!m.Build(a.data(), n, dim)) { fprintf(stderr, "Build failed\n"); return 4; }
    r3d_amd::IndMatches idx; std::vector<float> dist;
    for (size_t NN : {(size_t)3, (size_t)8}) {
        if (!search(m, b, nq, NN, idx, dist)) { fprintf(stderr, "SearchNeighbours(NN = %zu) failed\n", NN); return 5; }
        if (!write_result(prefix + (NN == 3 ? ".nn3" : ".nn8"), nq, NN, idx, dist)) return 6;
    }
    r3d_amd::IndMatches first; std::vector<float> first_d;
    if (!search(m, b, nq, 3, first, first_d)) return 5;
    const unsigned long long staged_before = m.viewsStaged();
    int same = 1;
#pragma omp parallel for schedule(dynamic) num_threads(8)
    for (int it = 0; it < loops; ++it) {
        r3d_amd::IndMatches li; std::vector<float> ld;
        if (!(search(m, b, nq, 3, li, ld) && same_answer(li, ld, first, first_d))) {
#pragma omp atomic write
            same = 0;
        }
    }
    const unsigned long long staged_loop = m.viewsStaged() - staged_before;
    m.setKnnNarrowTiles(false);
    const bool off_same = search(m, b, nq, 3, idx, dist) && same_answer(idx, dist, first, first_d);
    printf("%llu %d %d\n", staged_loop, same, off_same ? 1 : 0);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 9 || (strcmp(argv[1], "f32") != 0 && strcmp(argv[1], "u8") != 0)) {
        fprintf(stderr, "usage: knn_narrow_adapter_main <f32|u8> <dataset file> <rows> <query file> <queries> <dim> <out prefix> <loop count>\n");
        return 2;
    }
    return strcmp(argv[1], "u8") == 0 ? run<unsigned char>(argv) : run<float>(argv);
}
