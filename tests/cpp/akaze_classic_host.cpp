// akaze_classic_host.cpp -- the C++ facades with Regard3D's default detector list {"AKAZE"} (classic A-KAZE), as a host would call them.
// Used by tests/test_gpu_akaze_classic_stage.py.
//   features <gray.f32> <w> <h> <out.txt>          Regard3DFeatures::detectAndExtract with {"AKAZE"}: one "x y scale orientation desc..." line
//                                                  per feature; {"MSER"} and detectKeypoints("TBMR") must throw by name (else exit 9)
//   stage <dir> <w> <h> <gray.f32...>              R3DComputeMatches::computeMatches from pixels with {"AKAZE"}, F filter only
//   refuse <dir> <w> <h> <gray.f32>                {"MSER"} and {"AKAZE", "TBMR"} are refused by name (exit 0 when both are)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "r3d_compute_matches.hpp"
#include "regard3d_features.hpp"

using r3d_amd::Regard3DFeatures;

static std::vector<float> read_f32(const char* path, size_t n)
{
    std::vector<float> v(n);
    FILE* f = fopen(path, "rb");
    if (!f || fread(v.data(), 4, n, f) != n) { fprintf(stderr, "cannot read %s\n", path); exit(3); }
    fclose(f);
    return v;
}

static bool run_stage(const std::string& dir, int w, int h, const std::vector<std::vector<float>>& imgs, const std::vector<std::string>& detectors,
                      std::string& err)
{
    r3d_amd::R3DComputeMatches stage(0);
    std::vector<r3d_amd::View> views(imgs.size());
    for (size_t k = 0; k < imgs.size(); ++k) {
        char name[32];
        snprintf(name, sizeof(name), "img%03zu", k);
        views[k].id_view = (uint32_t)k; views[k].ui_width = (uint32_t)w; views[k].ui_height = (uint32_t)h; views[k].basename = name;
        views[k].gray = imgs[k].data();
    }
    stage.addViews(views);
    r3d_amd::R3DFParams params;
    params.keypointDetectorList_ = detectors;
    params.threshold_ = 0.001f;
    params.distRatio_ = 0.6f;
    params.computeFundalmentalMatrix_ = true;
    params.computeEssentialMatrix_ = false;
    params.computeHomographyMatrix_ = false;
    r3d_amd::R3DProjectPaths paths;
    paths.relativeMatchesPath_ = dir;
    const bool ok = stage.computeMatches(params, false, paths, 1, r3d_amd::R3DComputeMatches::kMatchingAlgorithmGPU);
    err = stage.errorMessage();
    return ok;
}

int main(int argc, char** argv)
{
    if (argc < 5) { fprintf(stderr, "usage: akaze_classic_host features|stage|refuse ...\n"); return 2; }
    const int w = atoi(argv[3]), h = atoi(argv[4]);
    if (!strcmp(argv[1], "features") && argc == 6) {
        const std::vector<float> img = read_f32(argv[2], (size_t)w * h);
        Regard3DFeatures::FeatsR3D feats; Regard3DFeatures::DescsR3D descs;
        try {
            Regard3DFeatures::R3DFParams params;
            params.keypointDetectorList_ = {"AKAZE"};
            params.threshold_ = 0.001f;
            if (!Regard3DFeatures::isDetectorServed("AKAZE")) return 8;
            Regard3DFeatures::detectAndExtract(r3d_amd::ImageViewF(img.data(), w, h), feats, descs, params);
        } catch (const std::exception& e) { fprintf(stderr, "detectAndExtract failed: %s\n", e.what()); return 7; }
        int refused = 0;
        try {
            Regard3DFeatures::R3DFParams params; params.keypointDetectorList_ = {"MSER"};
            Regard3DFeatures::FeatsR3D f2; Regard3DFeatures::DescsR3D d2;
            Regard3DFeatures::detectAndExtract(r3d_amd::ImageViewF(img.data(), w, h), f2, d2, params);
        } catch (const std::runtime_error& e) { refused += strstr(e.what(), "\"MSER\"") != nullptr; }
        try {
            std::vector<r3d_amd::KeyPointR3D> kp;
            Regard3DFeatures::detectKeypoints(r3d_amd::ImageViewF(img.data(), w, h), kp, "TBMR", Regard3DFeatures::R3DFParams());
        } catch (const std::runtime_error& e) { refused += strstr(e.what(), "\"TBMR\"") != nullptr; }
        if (refused != 2) return 9;
        FILE* o = fopen(argv[5], "w");
        for (size_t k = 0; k < feats.size(); ++k) {
            fprintf(o, "%.9g %.9g %.9g %.9g", feats[k].x, feats[k].y, feats[k].scale, feats[k].orientation);
            for (float v : descs[k]) fprintf(o, " %.9g", v);
            fprintf(o, "\n");
        }
        fclose(o);
        printf("%zu\n", feats.size());
        return 0;
    }
    if (!strcmp(argv[1], "stage") && argc >= 6) {
        std::vector<std::vector<float>> imgs;
        for (int k = 5; k < argc; ++k) imgs.push_back(read_f32(argv[k], (size_t)w * h));
        std::string err;
        if (!run_stage(argv[2], w, h, imgs, {"AKAZE"}, err)) { fprintf(stderr, "computeMatches failed: %s\n", err.c_str()); return 7; }
        return 0;
    }
    if (!strcmp(argv[1], "refuse") && argc == 6) {
        const std::vector<std::vector<float>> imgs{read_f32(argv[5], (size_t)w * h)};
        std::string e1, e2;
        const bool ok1 = run_stage(argv[2], w, h, imgs, {"MSER"}, e1);
        const bool ok2 = run_stage(argv[2], w, h, imgs, {"AKAZE", "TBMR"}, e2);
        fprintf(stderr, "%s\n%s\n", e1.c_str(), e2.c_str());
        return (!ok1 && !ok2 && e1.find("\"MSER\"") != std::string::npos && e2.find("\"TBMR\"") != std::string::npos) ? 0 : 9;
    }
    return 2;
}
