// init_genrand(19650218) (_randommodule.c), the starting array of
// init_by_array: the same for every seed, so it is a constant table read
// through the scalar cache instead of a per-step multiply chain.
// Plain C++ (no HIP): hz_device.hpp places it in constant memory, and
// tests/initgen_driver.cpp checks it on the host.
//
// The seeding loops read it a group or two of eight ahead of the row they are
// at, so it carries kInitGenPad more words (copies of the last: never used)
// and a read-ahead needs no clamp: a group of eight is one scalar load.  The
// groups start at rows 1 mod 8, so `lead` puts row 1 on a 64-byte boundary.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace hz {

constexpr int kInitGenRows = 624, kInitGenPad = 16;
struct InitGen {
  alignas(64) uint32_t lead[15];
  uint32_t v[kInitGenRows + kInitGenPad];
};
constexpr InitGen make_init_gen() {
  InitGen g{};
  uint32_t x = 19650218u;
  g.v[0] = x;
  for (int i = 1; i < kInitGenRows; i++) {
    x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)i;
    g.v[i] = x;
  }
  for (int i = kInitGenRows; i < kInitGenRows + kInitGenPad; i++) g.v[i] = x;
  return g;
}
static_assert(offsetof(InitGen, v) % 64 == 60, "row 1 of the table on a 64-byte boundary");

}  // namespace hz
