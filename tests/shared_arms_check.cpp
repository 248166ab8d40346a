// Host check of the arguments the shared arms of the lane machine's step rest on (csrc/hip/render_device.h: lane_consume, acc_step;
// csrc/pcg_jump.h). Stand-alone; built and run by test_shared_arms_host.py.
//
// 1. One set of draws. An offset lane's bounce-1 numbers are the three draws behind its stream's seeding and the two sub-pixel draws.
//    Form A seeds the stream and steps twice (what lane_consume did), form B starts from pcg_jump2 (what it does now); both then make
//    three draws. Same three doubles, same end state, for the extremes of the stream index, the largest base + s a 2^15-square film at
//    4096 spp forms, and 400 000 random streams. The generator is restated here from its definition, not taken from the header under test.
// 2. One division per step. acc_step forms num / (prob * spp) with num = w for an offset and 1.0 for a sample that ends without
//    offsets, where acc_no_offsets wrote 1.0 / (prob * spp); and radiance * inv_spp with inv_spp = 1.0 / spp formed once, where
//    operator/(D3, double) forms 1.0 / spp at every call. For prob over the denormals and 1e-300 .. 1e300 and spp = 1 .. 4096 the bits
//    are equal. (The numerator and the operands go through volatiles: nothing is folded at compile time.)
// 3. contrib - (+0) is contrib bit for bit (zeros of both signs, denormals, infinities; a NaN stays a NaN), which lets a sample without
//    offsets take the offsets' expression with cX = 0; and the component an offset k adds to is {1, 3, 2, 4}[k].
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "../gradient-based-path-tracing_amd/csrc/pcg_jump.h"

namespace {

constexpr uint64_t M = 6364136223846793005ULL, K = 0x31e241f862a1fb5eULL;
struct Rng { uint64_t state, inc; };
uint32_t next(Rng &r) {      // PCG32 XSH-RR
    const uint64_t old = r.state;
    r.state = old * M + (r.inc | 1);
    const uint32_t xorshifted = (uint32_t)(((old >> 18u) ^ old) >> 27u);
    const uint32_t rot = (uint32_t)(old >> 59u);
    return (xorshifted >> rot) | (xorshifted << ((0u - rot) & 31u));
}
Rng seeded(uint64_t stream) {
    Rng r{0, (stream << 1) | 1};
    next(r); r.state += K; next(r);
    return r;
}
double real(Rng &r) {        // 32 bits into the mantissa of [1, 2), minus 1
    const uint64_t u = ((uint64_t)next(r) << 20) | 0x3ff0000000000000ULL;
    double d;
    std::memcpy(&d, &u, sizeof d);
    return d - 1.0;
}
uint64_t bits(double a) { uint64_t u; std::memcpy(&u, &a, sizeof u); return u; }
bool same_bits(double a, double b) { return bits(a) == bits(b); }

}  // namespace

int main() {
    std::mt19937_64 gen(20240917);
    // ---- 1 ----
    unsigned long long streams = 0;
    auto check_stream = [&](uint64_t stream) {
        Rng a = seeded(stream);
        next(a); next(a);
        const double a0 = real(a), a1 = real(a), a2 = real(a);
        Rng b;
        b.inc = gd::pcg_stream_inc(stream);
        b.state = gd::pcg_jump2(b.inc);
        const double b0 = real(b), b1 = real(b), b2 = real(b);
        if (!same_bits(a0, b0) || !same_bits(a1, b1) || !same_bits(a2, b2) || a.state != b.state || a.inc != b.inc) {
            std::printf("stream %llu: stepped (%.17g %.17g %.17g, %llx), jumped (%.17g %.17g %.17g, %llx)\n", (unsigned long long)stream, a0, a1, a2,
                        (unsigned long long)a.state, b0, b1, b2, (unsigned long long)b.state);
            return false;
        }
        streams++;
        return true;
    };
    // the largest base + s: pixel (2^15 - 1, 2^15 - 1) of a 2^15-square film, 4096 streams per pixel, the last of them
    const uint64_t side = 1ULL << 15, spp_max = 4096;
    const uint64_t largest = ((side - 1) * side + (side - 1)) * spp_max + (spp_max - 1);
    static_assert(((1ULL << 15) - 1) * (1ULL << 15) + ((1ULL << 15) - 1) == (1ULL << 30) - 1, "last pixel index");
    const uint64_t extremes[] = {0, 1, 2, 1ULL << 32, (1ULL << 32) - 1, 1ULL << 63, (1ULL << 63) - 1, ~0ULL, largest, largest - 1, largest + 1};
    for (uint64_t s : extremes) if (!check_stream(s)) return 1;
    for (int i = 0; i < 200000; i++) if (!check_stream(gen())) return 1;
    for (int i = 0; i < 200000; i++) if (!check_stream(gen() % (largest + 1))) return 1;       // the sizes that occur

    // ---- 2 ----
    unsigned long long quotients = 0;
    volatile double one = 1.0;
    const double denorm_min = std::numeric_limits<double>::denorm_min(), dbl_min = std::numeric_limits<double>::min();
    std::uniform_real_distribution<double> mant(1.0, 2.0);
    auto check_prob = [&](double prob_in, int spp_in) {
        volatile double prob = prob_in, spp = (double)spp_in;
        const double as_written = 1.0 / (prob * spp);           // acc_no_offsets
        const double num = one;
        const double shared = num / (prob * spp);               // acc_step with num = 1.0
        if (!same_bits(as_written, shared)) { std::printf("prob %.17g spp %d: 1.0 / x = %.17g, num / x = %.17g\n", prob_in, spp_in, as_written, shared); return false; }
        quotients++;
        return true;
    };
    auto check_radiance = [&](double r_in, int spp_in) {
        volatile double r = r_in, spp = (double)spp_in;
        const double inv_here = 1.0 / spp;                      // operator/(D3, double): double inv = 1.0 / s; a.x * inv
        const double as_written = r * inv_here;
        volatile double inv_spp = 1.0 / (double)spp_in;         // formed once per launch
        const double shared = r * inv_spp;
        if (!same_bits(as_written, shared)) { std::printf("radiance %.17g spp %d: %.17g against %.17g\n", r_in, spp_in, as_written, shared); return false; }
        quotients++;
        return true;
    };
    for (int spp = 1; spp <= 4096; spp++) {
        const double fixed[] = {denorm_min, 3 * denorm_min, dbl_min / 2, dbl_min, 1e-300, 1e-100, 1e-10, 0.5, 1.0, 1.0 / 3, 1e10, 1e100, 1e300,
                                std::numeric_limits<double>::max(), 0.0, std::numeric_limits<double>::infinity()};
        for (double p : fixed) if (!check_prob(p, spp) || !check_radiance(p, spp) || !check_radiance(-p, spp)) return 1;
        for (int i = 0; i < 24; i++) {
            const int e = (int)(gen() % 2098) - 1074;           // 2^-1074 .. 2^1023: the denormals included
            const double p = std::ldexp(mant(gen), e);
            if (!check_prob(p, spp) || !check_radiance(p, spp)) return 1;
        }
    }

    // ---- 3 ----
    const double specials[] = {0.0, -0.0, denorm_min, -denorm_min, dbl_min, 1.0, -1.0, 1e300, -1e300, std::numeric_limits<double>::infinity(),
                               -std::numeric_limits<double>::infinity()};
    volatile double zero = 0.0;
    for (double c : specials) {
        volatile double v = c;
        const double d = v - zero;
        if (!same_bits(d, c)) { std::printf("%.17g - 0 = %.17g: other bits\n", c, d); return 1; }
    }
    for (int i = 0; i < 100000; i++) {
        uint64_t u = gen();
        double c;
        std::memcpy(&c, &u, sizeof c);
        volatile double v = c;
        const double d = v - zero;
        if (std::isnan(c) ? !std::isnan(d) : !same_bits(d, c)) { std::printf("%llx - 0: other bits\n", (unsigned long long)u); return 1; }
    }
    const int component[4] = {1, 3, 2, 4};                      // acc_offset: k = 0 dx0, 1 dx1, 2 dy0, 3 dy1
    for (int k = 0; k < 4; k++)
        if (1 + ((k & 1) << 1) + (k >> 1) != component[k]) { std::printf("offset %d adds to component %d\n", k, 1 + ((k & 1) << 1) + (k >> 1)); return 1; }

    std::printf("shared_arms_check ok: %llu streams, %llu quotients\n", streams, quotients);
    return 0;
}
