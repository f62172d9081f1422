// mip_args_host.cpp -- TEST TOOL ONLY.  The argument rule of csky_build_mips / csky_build_mips_device (csrc/mip_args.h) compiled with g++, which is
// what keeps the header free of HIP, so that tests/test_bake_reference.py can ask the DEVICE form about level counts no GPU is ever handed.
//   mip_args_host DEVICE N CH LEVELS [N CH LEVELS ...]  -> one line per triple: 1 accepted, 0 refused   (DEVICE: 0 host rule, 1 device rule)
#include <cstdio>
#include <cstdlib>
#include "../../godot-volumetric-cloud-demo-v2_amd/csrc/mip_args.h"

int main(int argc, char** argv) {
    if (argc < 5 || (argc - 2) % 3) { fprintf(stderr, "usage: mip_args_host DEVICE N CH LEVELS [N CH LEVELS ...]\n"); return 2; }
    static const unsigned char vol = 0;                       // only compared with NULL
    for (int i = 2; i + 2 < argc; i += 3) printf("%d\n", (int)csky::mip_args_ok(&vol, atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[1]) != 0));
    return 0;
}
