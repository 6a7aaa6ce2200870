// oracle/philox_fixture.cpp -- TEST INFRASTRUCTURE.  Prints the known-answer table tests/golden/philox4x32_10.json from an implementation of
// Philox4x32-10 that is not this project's: ATen's at::Philox4_32 (torch/include/ATen/core/PhiloxRNGEngine.h), compiled host-only.
// at::Philox4_32(seed, subsequence, offset) holds key = {seed lo, seed hi} and counter = {offset lo, offset hi, subsequence lo, subsequence hi};
// its first four outputs are the four words of Philox4x32-10(key, counter).  Build and run: `make -C oracle philox-fixture` (needs torch's headers;
// no test compiles anything: tests read the committed table only).
#include <ATen/core/PhiloxRNGEngine.h>
#include <cstdint>
#include <cstdio>

struct KC { uint32_t k[2], c[4]; };

int main() {
    const uint32_t F = 0xFFFFFFFFu, TAG = 0x5A4D504Cu;      // TAG: word 3 of the sampler's counters
    KC t[64]; int n = 0;
    auto add = [&](uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) { t[n++] = KC{{k0, k1}, {c0, c1, c2, c3}}; };
    add(0, 0, 0, 0, 0, 0);                                   // all-zero
    add(F, F, F, F, F, F);                                   // all-ones
    add(0xA4093822u, 0x299F31D0u, 0x243F6A88u, 0x85A308D3u, 0x13198A2Eu, 0x03707344u);      // Random123's kat_vectors "pi" row
    add(0, 0, F, F, F, F); add(F, F, 0, 0, 0, 0);
    for (int b = 0; b < 4; b++) add(0, 0, b == 0, b == 1, b == 2, b == 3);                   // one counter word set at a time
    add(1, 0, 0, 0, 0, 0); add(0, 1, 0, 0, 0, 0);
    // the sampler's shape: key = a 64-bit seed, counter = {call lo, call hi, lane, TAG (+ attempt)}; call counters below, at and above 2^32
    const uint64_t seeds[4] = {0, 5, 77, 0x9E3779B97F4A7C15ull};
    const uint64_t calls[6] = {0, 1, 0xFFFFFFFFull, 0x100000000ull, 0x100000001ull, 0xFEDCBA9876543210ull};
    const uint32_t lanes[3] = {0, 63, 1023};
    for (int s = 0; s < 4; s++) for (int c = 0; c < 6; c++) {
        const uint32_t lane = lanes[(s + c) % 3];
        add((uint32_t)seeds[s], (uint32_t)(seeds[s] >> 32), (uint32_t)calls[c], (uint32_t)(calls[c] >> 32), lane, TAG + (uint32_t)((s * 6 + c) % 3));
    }
    std::printf("{\"source\": \"at::Philox4_32, ATen/core/PhiloxRNGEngine.h\", \"rows\": [\n");
    for (int i = 0; i < n; i++) {
        at::Philox4_32 g(((uint64_t)t[i].k[1] << 32) | t[i].k[0], ((uint64_t)t[i].c[3] << 32) | t[i].c[2], ((uint64_t)t[i].c[1] << 32) | t[i].c[0]);
        uint32_t o[4]; for (int j = 0; j < 4; j++) o[j] = g();
        std::printf("  {\"key\": [%u, %u], \"counter\": [%u, %u, %u, %u], \"out\": [%u, %u, %u, %u]}%s\n", t[i].k[0], t[i].k[1], t[i].c[0], t[i].c[1], t[i].c[2],
                    t[i].c[3], o[0], o[1], o[2], o[3], i + 1 < n ? "," : "");
    }
    std::printf("]}\n");
    return 0;
}
