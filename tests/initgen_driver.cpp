// Prints the seeding table of csrc/hz_initgen.hpp (plain C++: no GPU, no
// HIP) for tests/test_initgen_cpu.py: the offset of row 0 in the struct, the
// row and padding counts, then every word of v, one per line.
#include <cstdio>

#include "../harmonies-alphazero_amd/csrc/hz_initgen.hpp"

int main() {
  static constexpr hz::InitGen g = hz::make_init_gen();
  std::printf("%zu %zu %d %d\n", offsetof(hz::InitGen, v), alignof(hz::InitGen), hz::kInitGenRows, hz::kInitGenPad);
  for (int i = 0; i < hz::kInitGenRows + hz::kInitGenPad; i++) std::printf("%u\n", g.v[i]);
  return 0;
}
