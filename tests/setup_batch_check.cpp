// Host check of the two arguments the batched sample set-up of the one-sided lane machine rests on (csrc/hip/render_device.h:
// lane_camera_batched; csrc/hip/device_trace.h: sample_setup / primary_from_setup). Stand-alone; built and run by test_setup_batch_host.py.
//
// 1. csrc/pcg_jump.h: pcg_jump2(inc) is the state of a PCG32 stream after its seeding and two draws, for the extremes of the stream index
//    and a large random set. The generator is restated here from its definition (state' = state * M + inc; the seeding steps, adds a
//    constant and steps again), not taken from the header under test.
// 2. On a power-of-two film the camera block passes sx = p + r to sample_primary, p = pixel coordinate (an offset ray's may be -1 or the
//    film size), r = a draw, m * 2^-32. floor(sx) == p and sx - floor(sx) == r bit for bit, so all five rays of a sample hand the pixel
//    filter the same numbers. For r in {0, 1, 2^31, 2^32 - 1} * 2^-32 and random r, p from -1 to the film size, film sizes 2^4 .. 2^15.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "../gradient-based-path-tracing_amd/csrc/pcg_jump.h"

namespace {

constexpr uint64_t M = 6364136223846793005ULL, K = 0x31e241f862a1fb5eULL;
struct Rng { uint64_t state, inc; };
void step(Rng &r) { r.state = r.state * M + (r.inc | 1); }
Rng seeded(uint64_t stream) {
    Rng r{0, (stream << 1) | 1};
    step(r); r.state += K; step(r);
    return r;
}
// a draw as the kernels form it (device_math.h: pcg_real): 32 bits into the mantissa of [1, 2), minus 1
double real_from_bits(uint32_t m) {
    const uint64_t u = ((uint64_t)m << 20) | 0x3ff0000000000000ULL;
    double d;
    std::memcpy(&d, &u, sizeof d);
    return d - 1.0;
}
bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

}  // namespace

int main() {
    // the constants as derived by hand once (A = (M + 1)(M^2 + 1), B = K * M^3 mod 2^64)
    static_assert(gd::kPcgJump2A == 0xcbb5f646404a560cULL, "jump multiplier");
    static_assert(gd::kPcgJump2B == 0x4c36be7be4e240f6ULL, "jump increment");
    static_assert(gd::kPcgMult == M && gd::kPcgSeedAdd == K, "generator constants");
    std::mt19937_64 gen(20240611);
    unsigned long long streams = 0;
    auto check_stream = [&](uint64_t stream) {
        Rng r = seeded(stream);
        step(r); step(r);
        const uint64_t inc = gd::pcg_stream_inc(stream);
        if (inc != r.inc || gd::pcg_jump2(inc) != r.state) {
            std::printf("stream %llu: jump %llx, stepped %llx\n", (unsigned long long)stream, (unsigned long long)gd::pcg_jump2(inc), (unsigned long long)r.state);
            return false;
        }
        streams++;
        return true;
    };
    const uint64_t extremes[] = {0, 1, 2, (1ULL << 31) - 1, 1ULL << 31, 1ULL << 32, (1ULL << 62), (1ULL << 63) - 1, 1ULL << 63, ~0ULL - 1, ~0ULL};
    for (uint64_t s : extremes) if (!check_stream(s)) return 1;
    for (int i = 0; i < 200000; i++) if (!check_stream(gen())) return 1;
    for (int i = 0; i < 200000; i++) if (!check_stream(gen() >> 24)) return 1;       // the sizes that occur: pixel index * spp + s

    unsigned long long pairs = 0;
    for (int log2 = 4; log2 <= 15; log2++) {
        const int size = 1 << log2;
        for (int p = -1; p <= size; p++) {
            uint32_t ms[4 + 12] = {0u, 1u, 1u << 31, 0xFFFFFFFFu};
            for (int i = 4; i < 16; i++) ms[i] = (uint32_t)gen();
            for (uint32_t m : ms) {
                const double r = real_from_bits(m);
                if (!same_bits(r, (double)m * 0x1p-32)) { std::printf("draw %u is not m * 2^-32\n", m); return 1; }
                const double sx = p + r;                 // (x + ox) + rx, int + double as in lane_camera
                const double fx = std::floor(sx);
                if (!same_bits(fx, (double)p) || !same_bits(sx - fx, r)) {
                    std::printf("film %d, p %d, m %u: floor %.17g, remainder %.17g, draw %.17g\n", size, p, m, fx, sx - fx, r);
                    return 1;
                }
                pairs++;
            }
        }
    }
    std::printf("setup_batch_check ok: %llu streams, %llu (pixel, draw) pairs\n", streams, pairs);
    return 0;
}
