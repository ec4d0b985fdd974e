// Host check of the hoisted Philox call (pathfinder.jl_amd/csrc/pfmi_common.h): pf_philox_draw_invariants + pf_philox_block_product +
// pf_philox4x32_hoisted<PF_NORMAL_ROUNDS> against pf_philox4x32<PF_NORMAL_ROUNDS>(n, g, 0, 0, k0, k1), word for word.  No HIP call, no GPU.
// Built and run by tests/test_philox_hoist_host.py; prints "ok <tuples>" and returns 0, or the first mismatch and 1.
#include <cstdint>
#include <cstdio>
#include "pfmi_common.h"

static unsigned long long checked = 0;

static bool same(uint32_t n, uint32_t g, uint32_t k0, uint32_t k1) {
    uint32_t a[4], b[4];
    pf_philox4x32<PF_NORMAL_ROUNDS>(n, g, 0u, 0u, k0, k1, a);
    const pf_philox_inv v = pf_philox_draw_invariants(n, k0, k1);
    pf_philox4x32_hoisted<PF_NORMAL_ROUNDS>(v, pf_philox_block_product(g, k0), k0, k1, b);
    ++checked;
    if (a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3]) return true;
    printf("mismatch at n=%08x g=%08x k0=%08x k1=%08x: %08x %08x %08x %08x != %08x %08x %08x %08x\n", n, g, k0, k1, a[0], a[1], a[2], a[3],
           b[0], b[1], b[2], b[3]);
    return false;
}

// the hoisted form with three rounds is the words after round 3 themselves: a second, independent look at the split
static bool same3(uint32_t n, uint32_t g, uint32_t k0, uint32_t k1) {
    uint32_t a[4], b[4];
    pf_philox4x32<3>(n, g, 0u, 0u, k0, k1, a);
    pf_philox4x32_hoisted<3>(pf_philox_draw_invariants(n, k0, k1), pf_philox_block_product(g, k0), k0, k1, b);
    return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3];
}

static uint64_t splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main() {
    const uint32_t edge[5] = {0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
    const uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    for (uint32_t n : edge) for (uint32_t g : edge) for (uint32_t k0 : edge) for (uint32_t k1 : edge)
        if (!same(n, g, k0, k1) || !same3(n, g, k0, k1)) return 1;
    // keys for which k + j W wraps at round j + 1: k = -(j W) - 1, -(j W), -(j W) + 1 for every j the rounds use
    for (uint32_t j = 1; j < (uint32_t)PF_NORMAL_ROUNDS; ++j)
        for (int e0 = -1; e0 <= 1; ++e0) for (int e1 = -1; e1 <= 1; ++e1) for (uint32_t n : edge) for (uint32_t g : edge) {
            const uint32_t k0 = 0u - j * W0 + (uint32_t)e0, k1 = 0u - j * W1 + (uint32_t)e1;
            if (!same(n, g, k0, k1) || !same3(n, g, k0, k1)) return 1;
        }
    uint64_t s = 20240607ull;
    for (int i = 0; i < 100000; ++i) {
        const uint64_t a = splitmix(s), b = splitmix(s);
        if (!same((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32))) return 1;
        // the scan's own range as well: small draw and row-group indices under a random key
        if (!same((uint32_t)a & 0xFFFu, (uint32_t)(a >> 32) & 0x3FFu, (uint32_t)b, (uint32_t)(b >> 32))) return 1;
    }
    printf("ok %llu\n", checked);
    return 0;
}
