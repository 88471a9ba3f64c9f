// Host check of the sparse round 0 (prysm_amd/csrc/keccak_sparse.hpp): the
// header's instruction sequence, compiled for the host over a plain C++ ops
// policy, against a textbook Keccak-f round on the zero-extended 25-lane
// input, for random fills of the live lanes, both forms.  Built with
// -fsanitize=address,undefined by tests/test_sparse_round_host.py.  This
// covers the lane map the two policies share; the device policy's own
// instruction wrappers (AsmOps in keccak_dev.hpp: ax2, ax3s, ...) run only
// on the GPU and are covered by the root tests there.
//   sparse_round_host <seed> <cases>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "keccak_sparse.hpp"

namespace {

struct State {
    uint32_t lo[25];
    uint32_t hi[25];
};

struct HostOps {
    static uint32_t x2(uint32_t a, uint32_t b) { return a ^ b; }
    static uint32_t x3(uint32_t a, uint32_t b, uint32_t c) { return a ^ b ^ c; }
    static uint32_t xk(uint32_t a, uint32_t k) { return a ^ k; }
    static uint32_t x3k(uint32_t a, uint32_t b, uint32_t k) { return a ^ b ^ k; }
    static uint32_t chi(uint32_t a, uint32_t b, uint32_t c) { return a ^ (~b & c); }
    template <int N>
    static void rot(uint32_t lo, uint32_t hi, uint32_t& olo, uint32_t& ohi) {
        const uint64_t v = ((uint64_t)hi << 32) | lo;
        const uint64_t r = N ? (v << N) | (v >> (64 - N)) : v;
        olo = (uint32_t)r;
        ohi = (uint32_t)(r >> 32);
    }
    static void bar_theta() { ++bars; }
    static void bar_chi() { ++bars; }
    static int bars;
};
int HostOps::bars = 0;

uint64_t rotl(uint64_t v, int n) { return n ? (v << n) | (v >> (64 - n)) : v; }

// one Keccak-f[1600] round as in FIPS 202 §3.2, A[x + 5y]
void round_ref(uint64_t (&a)[25], uint64_t rc) {
    static const int r[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
    uint64_t c[5], b[25];
    for (int x = 0; x < 5; ++x) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
    for (int i = 0; i < 25; ++i) a[i] ^= c[(i % 5 + 4) % 5] ^ rotl(c[(i % 5 + 1) % 5], 1);
    for (int x = 0; x < 5; ++x)
        for (int y = 0; y < 5; ++y) b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl(a[x + 5 * y], r[x + 5 * y]);
    for (int y = 0; y < 5; ++y)
        for (int x = 0; x < 5; ++x) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
    a[0] ^= rc;
}

uint64_t sm_state;
uint64_t splitmix() {
    uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// live lanes [0, nlive) filled (every 16th case all-zero or all-ones), the rest poisoned in `s` and zero in `a`
void fill(int nlive, long k, State& s, uint64_t (&a)[25]) {
    for (int i = 0; i < 25; ++i) {
        uint64_t v = splitmix();
        if (k % 16 == 0) v = 0;
        if (k % 16 == 1) v = ~0ull;
        a[i] = i < nlive ? v : 0;
        s.lo[i] = i < nlive ? (uint32_t)v : 0xDEADBEEFu;  // must not be read
        s.hi[i] = i < nlive ? (uint32_t)(v >> 32) : 0xFEEDFACEu;
    }
}

bool same(const State& s, const uint64_t (&a)[25]) {
    for (int i = 0; i < 25; ++i)
        if ((((uint64_t)s.hi[i] << 32) | s.lo[i]) != a[i]) return false;
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    sm_state = argc > 1 ? strtoull(argv[1], nullptr, 0) : 1;
    const long cases = argc > 2 ? atol(argv[2]) : 10000;
    const uint64_t rc = 0x0000000000000001ull;
    for (long k = 0; k < cases; ++k) {
        State s;
        uint64_t a[25];
        fill(8, k, s, a);
        a[8] = 0x01;  // the pad byte after 64 B of message
        a[16] = 0x8000000000000000ull;
        round_ref(a, rc);
        mk::sparse::round0_node<HostOps>(s, (uint32_t)rc, (uint32_t)(rc >> 32));
        if (!same(s, a)) {
            fprintf(stderr, "round0_node differs at case %ld\n", k);
            return 1;
        }
        fill(17, k, s, a);
        round_ref(a, rc);
        mk::sparse::round0_block17<HostOps>(s, (uint32_t)rc, (uint32_t)(rc >> 32));
        if (!same(s, a)) {
            fprintf(stderr, "round0_block17 differs at case %ld\n", k);
            return 1;
        }
    }
    if (HostOps::bars != 4 * cases) {  // two barrier positions per round, as round_asm<true>
        fprintf(stderr, "%d barrier positions in %ld rounds, expected %ld\n", HostOps::bars, 2 * cases, 4 * cases);
        return 1;
    }
    fprintf(stderr, "%ld cases clean (both forms)\n", cases);
    return 0;
}
