// Prints the table of regard3d_amd/csrc/descriptor_arms.hpp for tests/test_descriptor_arms.py: host only, the header alone.
// g++ -std=c++17 -I. tests/cpp/descriptor_arms_test.cpp -o descriptor_arms_test && ./descriptor_arms_test
//   arm <id> <name> <tag> <macro> <dtype> <dim> <row_bytes> <border_mult> <level_planes> <the float bits of ak_smax>
// and, for the lookups the caller asks for (arguments `id <n>` and `type <dtype>,<dim>`):
//   by_id <id> <found>        by_type <dtype> <dim> <id or none>
#include "regard3d_amd/csrc/descriptor_arms.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char** argv)
{
    for (const DescriptorArm& a : kDescriptorArms) {
        const float smax = ak_smax(a);
        uint32_t bits;
        memcpy(&bits, &smax, 4);
        printf("arm %d %s %s %s %d %u %u %g %d %08x\n", a.id, a.name, a.tag, a.macro, (int)a.dtype, a.dim, a.row_bytes, a.border_mult, (int)a.level_planes, bits);
        if (descriptor_arm_by_id(a.id) != &a || descriptor_arm_by_type(a.dtype, a.dim) != &a || ak_smax(a.border_mult) != smax) return 1;   // the lookups round-trip
    }
    for (int i = 1; i + 1 < argc; i += 2) {           // the arguments come in pairs: id <n>, or type <dtype>,<dim>
        if (!strcmp(argv[i], "id")) printf("by_id %d %d\n", atoi(argv[i + 1]), descriptor_arm_by_id(atoi(argv[i + 1])) ? 1 : 0);
        else if (!strcmp(argv[i], "type")) {
            int dtype = 0; unsigned dim = 0;
            if (sscanf(argv[i + 1], "%d,%u", &dtype, &dim) != 2) return 2;
            const DescriptorArm* a = descriptor_arm_by_type(dtype, dim);
            if (a) printf("by_type %d %u %d\n", dtype, dim, a->id); else printf("by_type %d %u none\n", dtype, dim);
        } else return 2;
    }
    return 0;
}
