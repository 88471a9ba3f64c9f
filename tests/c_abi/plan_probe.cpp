// Prints the pass plan the host planner (prysm_amd/csrc/planner.cpp) makes for
// one merkleHash, so that a test can assert which kernels its shape reaches:
//   plan_probe n item_len aligned16
//   -> "small S ws W" and one line per pass:
//      "pass I leaf L wave W sp S ni N nwg G nfast F nlock K c1 C levels V"
// Built host-only with g++ by tests/test_gpu_ws_contract.py (no HIP).
#include <cstdio>
#include <cstdlib>

#include "planner.hpp"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const uint64_t n = std::strtoull(argv[1], nullptr, 10);
    const uint32_t il = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    const bool aligned = std::atoi(argv[3]) != 0;
    mk::Plan p;
    if (mk::make_plan(n, il, false, 0, false, aligned, p) != MK_OK) {
        std::printf("error %s\n", mk::last_error());
        return 1;
    }
    std::printf("small %d ws %llu\n", p.small ? 1 : 0, (unsigned long long)(p.small ? 0 : mk::plan_ws_bytes(p)));
    for (size_t i = 0; i < p.passes.size(); ++i) {
        const mk::Pass& ps = p.passes[i];
        std::printf("pass %zu leaf %d wave %d sp %d ni %u nwg %llu nfast %llu nlock %llu c1 %llu levels %u\n", i,
                    ps.leaf ? 1 : 0, ps.wave ? 1 : 0, ps.sp ? 1 : 0, ps.ni, (unsigned long long)ps.nwg,
                    (unsigned long long)ps.nfast, (unsigned long long)ps.nlock, (unsigned long long)ps.a.c1,
                    ps.a.levels);
    }
    return 0;
}
