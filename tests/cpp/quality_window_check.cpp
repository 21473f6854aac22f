// CPU run of the frame-quality arithmetic the device runs (x266_amd/csrc/x266_quality.hpp: the sums of four packed samples, the sums of a
// 4x4 block, the window's Q30 value), as plain C++.  The program builds a fixed list of 8x8 sample windows itself -- the windows whose values
// include/x266hip.h states, seeded noise against independent noise and against its inverse, flat windows one level apart, a smooth window
// lightly distorted -- takes each through the header the way quality_kernels.hip does (a dword per block row, four rows to a block, four blocks
// to a window) and prints the samples, the four sums, the squared error, cn and q.  tests/test_quality_window.py holds every printed value
// against tests/_quality_ref.py.
// Test infrastructure; built and run by tests/test_quality_window.py (g++, plain and with sanitizers; no GPU, no HIP).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "x266_quality.hpp"

using namespace x266;

static int g_windows = 0, g_failures = 0;

static uint64_t mix(uint64_t &state)                                        // SplitMix64
{
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static uint32_t row_word(const uint8_t *row)                                // four samples as the device loads them: little-endian
{
    uint32_t w;
    std::memcpy(&w, row, 4);
    return w;
}

static void window(const char *name, const uint8_t a[64], const uint8_t b[64])
{
    QualitySums win = {0, 0, 0};
    for (int by = 0; by < 2; ++by)
        for (int bx = 0; bx < 2; ++bx) {
            QualitySums block = {0, 0, 0};
            for (int r = 0; r < 4; ++r) block = quality_add4(block, row_word(a + (4 * by + r) * 8 + 4 * bx), row_word(b + (4 * by + r) * 8 + 4 * bx));
            win = win + block;
        }
    const uint32_t s1 = win.s & 0xFFFFu, s2 = win.s >> 16;
    int64_t cn = 0;
    const int64_t q = quality_window_q(s1, s2, win.ss, win.ab, &cn);
    if (q != quality_window_q(win)) ++g_failures, std::printf("FAIL %s: the packed form gives another q\n", name);
    uint32_t direct = 0;
    for (int i = 0; i < 64; ++i) direct += (uint32_t)(((int)a[i] - (int)b[i]) * ((int)a[i] - (int)b[i]));
    if (direct != quality_sse(win)) ++g_failures, std::printf("FAIL %s: sse %u, sample by sample %u\n", name, quality_sse(win), direct);
    std::printf("window %s a=", name);
    for (int i = 0; i < 64; ++i) std::printf("%02x", a[i]);
    std::printf(" b=");
    for (int i = 0; i < 64; ++i) std::printf("%02x", b[i]);
    std::printf(" s1=%u s2=%u ss=%u s12=%u sse=%u cn=%lld q=%lld\n", s1, s2, win.ss, win.ab, quality_sse(win), (long long)cn, (long long)q);
    ++g_windows;
}

int main()
{
    uint8_t a[64], b[64];
    char name[64];
    std::memset(a, 77, 64);
    window("identical_flat", a, a);
    std::memset(a, 0, 64);
    std::memset(b, 255, 64);
    window("zeros_against_255", a, b);
    window("255_against_zeros", b, a);
    for (int i = 0; i < 64; ++i) a[i] = (uint8_t)(255 * (((i & 7) + (i >> 3)) & 1)), b[i] = (uint8_t)(255 - a[i]);
    window("checkerboard_against_inverse", a, b);
    uint64_t state = 0x266;
    for (int n = 0; n < 24; ++n) {
        for (int i = 0; i < 64; ++i) a[i] = (uint8_t)mix(state), b[i] = (uint8_t)mix(state);
        std::snprintf(name, sizeof name, "noise_%d", n);
        window(name, a, b);
        std::snprintf(name, sizeof name, "noise_%d_identical", n);
        window(name, a, a);
        for (int i = 0; i < 64; ++i) b[i] = (uint8_t)(255 - a[i]);
        std::snprintf(name, sizeof name, "noise_%d_inverse", n);
        window(name, a, b);
    }
    for (int level : {0, 1, 16, 127, 128, 254}) {                            // flat windows one level apart, both ways
        std::memset(a, level, 64);
        std::memset(b, level + 1, 64);
        std::snprintf(name, sizeof name, "flat_%d_plus_1", level);
        window(name, a, b);
        std::snprintf(name, sizeof name, "flat_%d_minus_1", level + 1);
        window(name, b, a);
    }
    for (int n = 0; n < 8; ++n) {                                            // a ramp with a little noise, distorted by +-3 and clipped
        for (int i = 0; i < 64; ++i) {
            const int v = 30 * n + 3 * (i & 7) + 2 * (i >> 3) + (int)(mix(state) % 5), d = v + (int)(mix(state) % 7) - 3;
            a[i] = (uint8_t)(v > 255 ? 255 : v);
            b[i] = (uint8_t)(d < 0 ? 0 : d > 255 ? 255 : d);
        }
        std::snprintf(name, sizeof name, "distorted_%d", n);
        window(name, a, b);
    }
    std::printf("windows %d\n", g_windows);
    if (g_failures) {
        std::printf("%d checks FAILED\n", g_failures);
        return 1;
    }
    std::printf("the window arithmetic holds (%d windows)\n", g_windows);
    return 0;
}
