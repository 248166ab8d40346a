// pcg_jump.h — the state of a PCG32 stream behind its seeding and two draws, in one multiply-add (no HIP dependency: device_math.h
// includes it for the kernels, tests/setup_batch_check.cpp on the host).
//
// A step is state' = state * M + inc (mod 2^64). pcg_init (device_math.h, src/pcg.h) starts from 0, steps, adds K and steps again:
//   after the seeding   inc * (M + 1) + K * M
//   one draw later      inc * (M + 1) * M + K * M^2 + inc
//   two draws later     inc * ((M + 1) * M^2 + M + 1) + K * M^3  =  inc * (M + 1)(M^2 + 1) + K * M^3
// so the state is affine in inc. A lane that receives the two draws' results from elsewhere (render_device.h: sample_setup made them) gets
// the state it would have had from pcg_jump2 instead of three steps and two output permutations.
#pragma once
#include <stdint.h>

namespace gd {

constexpr uint64_t kPcgMult = 6364136223846793005ULL;       // src/pcg.h:21
constexpr uint64_t kPcgSeedAdd = 0x31e241f862a1fb5eULL;     // what pcg_init adds between its two steps
constexpr uint64_t kPcgJump2A = (kPcgMult + 1u) * (kPcgMult * kPcgMult + 1u);
constexpr uint64_t kPcgJump2B = kPcgSeedAdd * kPcgMult * kPcgMult * kPcgMult;

// inc of stream `stream`, as pcg_init forms it
constexpr uint64_t pcg_stream_inc(uint64_t stream) { return (stream << 1u) | 1u; }
// state of the stream with that inc after pcg_init and two pcg_next
constexpr uint64_t pcg_jump2(uint64_t inc) { return inc * kPcgJump2A + kPcgJump2B; }

} // namespace gd
