// mldb_kgraph_main.cpp -- binary rows on the graph matcher the way a C++ host reaches them.
//   mldb_kgraph_main plugin <rows.u8> <n rows> <bytes> <queries.u8> <n queries> <out prefix>
//       ArrayMatcher_r3dm_kgraph<unsigned char, r3d_amd::HammingMetric>: Build, then SearchNeighbours with NN = 1, 2, 5 ->
//       <out prefix>.h<NN>.bin (per entry: query u32, row u32, distance f32); the same rows under the default metric with NN = 2 ->
//       <out prefix>.l2.bin
//   mldb_kgraph_main stage <matches dir> <n views> <width> <height> <gray.f32> <dist ratio> <matchingAlgorithm> <as requested 0|1>
//       R3DComputeMatches with setRegionsType(R3DM_BIN, 61) from pixels, no filter; prints "<putative pairs> <exhaustive 0|1>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "r3d_compute_matches.hpp"
#include "r3dm_ann_matchers.hpp"

static bool read_all(const char* path, void* dst, size_t bytes)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    const bool ok = fread(dst, 1, bytes, f) == bytes;
    fclose(f);
    return ok;
}

template <class Matcher, class Dist>
static int search_to_file(Matcher& m, const unsigned char* q, int nq, size_t NN, const std::string& path)
{
    r3d_amd::IndMatches idx; std::vector<Dist> dist;
    if (!m.SearchNeighbours(q, nq, &idx, &dist, NN)) return 5;
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return 6;
    for (size_t k = 0; k < idx.size(); ++k) {
        const uint32_t rec[2] = {idx[k].i_, idx[k].j_};
        const float d = (float)dist[k];
        fwrite(rec, 4, 2, f); fwrite(&d, 4, 1, f);
    }
    fclose(f);
    return 0;
}

static int run_plugin(char** a)
{
    const int n = atoi(a[3]), nbytes = atoi(a[4]), nq = atoi(a[6]);
    std::vector<unsigned char> rows((size_t)n * nbytes), q((size_t)nq * nbytes);
    if (!read_all(a[2], rows.data(), rows.size()) || !read_all(a[5], q.data(), q.size())) return 3;
    const std::string out = a[7];
    {
        r3d_amd::ArrayMatcher_r3dm_kgraph<unsigned char, r3d_amd::HammingMetric> m(3);
        static_assert(std::is_same<decltype(m)::DistanceType, unsigned>::value, "Hamming distances are counts");
        if (!m.Build(rows.data(), n, nbytes)) return 4;
        for (size_t NN : {1u, 2u, 5u}) {
            const int rc = search_to_file<decltype(m), unsigned>(m, q.data(), nq, NN, out + ".h" + std::to_string(NN) + ".bin");
            if (rc) return rc;
        }
    }
    r3d_amd::ArrayMatcher_r3dm_kgraph<unsigned char> l2(3);             // the default metric: byte VALUES under L2, as before
    if (nbytes % 4) return 0;                                          // (L2 rows come in fours)
    if (!l2.Build(rows.data(), n, nbytes)) return 7;
    return search_to_file<decltype(l2), float>(l2, q.data(), nq, 2, out + ".l2.bin");
}

static int run_stage(char** a)
{
    const uint32_t n = (uint32_t)atoi(a[3]), w = (uint32_t)atoi(a[4]), h = (uint32_t)atoi(a[5]);
    std::vector<float> gray((size_t)n * w * h);
    if (!read_all(a[6], gray.data(), gray.size() * 4)) return 3;
    r3d_amd::R3DComputeMatches stage(0);
    std::vector<r3d_amd::View> views(n);
    for (uint32_t k = 0; k < n; ++k) {
        char name[32];
        snprintf(name, sizeof(name), "img%03u", k);
        views[k].id_view = k; views[k].ui_width = w; views[k].ui_height = h; views[k].basename = name;
        views[k].gray = gray.data() + (size_t)k * w * h;
    }
    stage.addViews(views);
    stage.setRegionsType(R3DM_BIN, 61);
    stage.setFeaturesConcurrency(2, 2);
    stage.setApproximateArmsPolicy(atoi(a[9]) ? r3d_amd::R3DComputeMatches::kArmsAsRequested : r3d_amd::R3DComputeMatches::kArmsFastest);
    r3d_amd::R3DFParams params;
    params.keypointDetectorList_ = {"Fast-AKAZE"};
    params.threshold_ = 0.001f;
    params.distRatio_ = (float)atof(a[7]);
    params.computeFundalmentalMatrix_ = false;
    params.computeEssentialMatrix_ = false;
    params.computeHomographyMatrix_ = false;
    r3d_amd::R3DProjectPaths paths;
    paths.relativeMatchesPath_ = a[2];
    if (!stage.computeMatches(params, false, paths, 1, atoi(a[8]))) {
        fprintf(stderr, "computeMatches: %s\n", stage.errorMessage().c_str());
        return 4;
    }
    printf("%zu %d\n", stage.getStatistics().putativeMatches_.size(), stage.lastMatchWasExhaustive() ? 1 : 0);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 8 && !strcmp(argv[1], "plugin")) return run_plugin(argv);
    if (argc == 10 && !strcmp(argv[1], "stage")) return run_stage(argv);
    fprintf(stderr, "usage: mldb_kgraph_main plugin <rows.u8> <n> <bytes> <queries.u8> <nq> <out prefix>\n"
                    "       mldb_kgraph_main stage <matches dir> <n views> <width> <height> <gray.f32> <dist ratio> <matchingAlgorithm> <as requested 0|1>\n");
    return 2;
}
