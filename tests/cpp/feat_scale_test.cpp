// feat_scale_test.cpp -- the .feat reader of the facade (regard3d_amd/csrc/feat_text.hpp) keeps the scale column as written: reads the
// file named on the command line and prints "n", then one line "x y scale" per feature with the three floats' bit patterns in hex.
// g++ -O2 -std=c++17 tests/cpp/feat_scale_test.cpp -o feat_scale_test && ./feat_scale_test file.feat
#include "../../regard3d_amd/csrc/feat_text.hpp"
#include <cstdint>
#include <cstring>

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    std::vector<float> xy, scale, xy_only;
    if (!r3dm_feat::load_feat(argv[1], xy, &scale) || !r3dm_feat::load_feat(argv[1], xy_only)) return 1;
    if (xy != xy_only || xy.size() != 2 * scale.size()) return 3;       // the positions do not depend on whether the scales are asked for
    std::printf("%zu\n", scale.size());
    for (size_t k = 0; k < scale.size(); ++k) {
        uint32_t b[3];
        std::memcpy(&b[0], &xy[2 * k], 4); std::memcpy(&b[1], &xy[2 * k + 1], 4); std::memcpy(&b[2], &scale[k], 4);
        std::printf("%08x %08x %08x\n", b[0], b[1], b[2]);
    }
    return 0;
}
