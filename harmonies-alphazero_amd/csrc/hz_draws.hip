// hz_draws.hip — the stateless draw kernels of self-play: root noise, the
// playout-cap coin, the root Gumbels and the leaf-symmetry keys, each keyed by (seed, global board id,
// move).  None takes a handle.
#include "hz_mcts.hpp"

#include "../../include/hz_abi.h"

using namespace hz;
using namespace hz_host;
using namespace hz_tree;

namespace {

// ------------------------------------------------------------- root noise
// The self-play root noise of get_best_action_and_pi (MCTS.py:314-316:
// np.random.dirichlet([alpha] * L) over the L legal moves) and the tau = 1
// uniform of its move choice (MCTS.py:411, np.random.choice), drawn from a
// counter-based generator keyed by (seed, global board id, move) instead of
// the process-global np.random: every board's draws are the same whatever
// the batch it sits in or the number of GPUs.  One wave per
// board; lane c draws child c's Gamma(alpha) (and c + 64's): Marsaglia-Tsang
// for alpha + 1 with a standard normal from Box-Muller, times U^(1/alpha)
// for alpha < 1.  The live children's sum is a fixed butterfly over the
// wave, so the result does not depend on anything but the key.
struct NoiseStream {
  uint64_t key, ctr;
  __device__ double uniform() {  // (0, 1], 53 bits
    uint64_t z = mix64(key + 0x9E3779B97F4A7C15ULL * ++ctr);
    return ((double)(z >> 11) + 1.0) * 0x1.0p-53;
  }
};

__device__ double gamma_draw(NoiseStream &s, double alpha) {
  const double a = alpha < 1.0 ? alpha + 1.0 : alpha;
  const double d = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
  double g;
  for (;;) {
    double x, v;
    do {
      double u1 = s.uniform(), u2 = s.uniform();
      x = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
      v = 1.0 + c * x;
    } while (v <= 0.0);
    v = v * v * v;
    double u = s.uniform();
    if (u < 1.0 - 0.0331 * x * x * x * x || log(u) < 0.5 * x * x + d * (1.0 - v + log(v))) {
      g = d * v;
      break;
    }
  }
  if (alpha < 1.0) g *= pow(s.uniform(), 1.0 / alpha);
  return g;
}

// The key of board b's draws at `move`: every draw kernel's, the per-board-move forms' too.
__device__ __forceinline__ uint64_t draw_key(uint64_t seed, uint64_t board_base, int b, uint64_t move) {
  return mix64(mix64(mix64(seed ^ 0x6A09E667F3BCC908ULL) ^ (board_base + (uint64_t)b)) ^ move);
}

// Board b's noise row and uniform under `key` (one wave): k_root_noise's and k_root_noise_at's body.
__device__ __forceinline__ void root_noise_row(const int32_t *__restrict__ count, int b, int lane, uint64_t key,
                                               double alpha, double *__restrict__ noise, double *__restrict__ u) {
  const int nl = count ? min(max(count[b], 0), kMaxChildren) : 0;
  double g[2];
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int c = lane + kWave * k;
    NoiseStream s{mix64(key ^ (0xD1B54A32D192ED03ULL * (uint64_t)(c + 1))), 0};
    g[k] = c < nl ? gamma_draw(s, alpha) : 0.0;
    sum += g[k];
  }
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) sum += __shfl_xor(sum, off);
  const double inv = sum > 0.0 ? 1.0 / sum : 0.0;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int c = lane + kWave * k;
    if (c < kMaxChildren) noise[(size_t)b * kMaxChildren + c] = g[k] * inv;
  }
  if (lane == 0 && u) {
    NoiseStream s{mix64(key ^ 0x5851F42D4C957F2DULL), 0};
    u[b] = s.uniform() - 0x1.0p-53;  // [0, 1)
  }
}

__global__ void __launch_bounds__(kWave) k_root_noise(const int32_t *__restrict__ count, int n, uint64_t seed,
                                                      uint64_t board_base, uint64_t move, double alpha,
                                                      double *__restrict__ noise, double *__restrict__ u) {
  const int b = blockIdx.x;
  root_noise_row(count, b, threadIdx.x, draw_key(seed, board_base, b, move), alpha, noise, u);
}

// The per-board-move form (hz_root_noise_at): board b's row at move[b], where
// mask[b] == 1; every other row of noise and u keeps what it holds.
__global__ void __launch_bounds__(kWave) k_root_noise_at(const int32_t *__restrict__ count, int n, uint64_t seed,
                                                         uint64_t board_base, const uint64_t *__restrict__ move,
                                                         const uint8_t *__restrict__ mask, double alpha,
                                                         double *__restrict__ noise, double *__restrict__ u) {
  const int b = blockIdx.x;
  if (mask[b] != 1) return;  // (wave-uniform)
  root_noise_row(count, b, threadIdx.x, draw_key(seed, board_base, b, move[b]), alpha, noise, u);
}

// One uniform in (0, 1] per board (hz_playout_coin: the coin of playout-cap
// randomization, no reference counterpart), from k_root_noise's generator and
// board key under a salt of its own: neither the noise nor the move-choice
// uniform moves by a bit.
__device__ __forceinline__ double coin_of(uint64_t key) {
  NoiseStream s{mix64(key ^ 0x94D049BB133111EBULL), 0};
  return s.uniform();
}
__global__ void __launch_bounds__(256) k_playout_coin(int n, uint64_t seed, uint64_t board_base, uint64_t move,
                                                      double *__restrict__ coin) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  coin[b] = coin_of(draw_key(seed, board_base, b, move));
}

// The per-board-move form (hz_playout_coin_at): board b's coin at move[b],
// where mask[b] == 1; every other entry keeps what it holds.
__global__ void __launch_bounds__(256) k_playout_coin_at(int n, uint64_t seed, uint64_t board_base,
                                                         const uint64_t *__restrict__ move,
                                                         const uint8_t *__restrict__ mask, double *__restrict__ coin) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n || mask[b] != 1) return;
  coin[b] = coin_of(draw_key(seed, board_base, b, move[b]));
}

// One standard Gumbel per board and legal rank (hz_root_gumbel; no reference
// counterpart): g = -log(-log u), u = (k + 1/2) 2^-52 for a 52-bit k, so u
// lies strictly inside (0, 1) and g is finite; from k_root_noise's generator
// and board key under a salt of its own (the noise, the move-choice uniform
// and the coin keep their bits).
__global__ void __launch_bounds__(kWave) k_root_gumbel(int n, uint64_t seed, uint64_t board_base, uint64_t move,
                                                       double *__restrict__ out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= n) return;
  const uint64_t key = mix64(mix64(mix64(seed ^ 0x6A09E667F3BCC908ULL) ^ (board_base + (uint64_t)b)) ^ move);
  for (int c = lane; c < kMaxChildren; c += kWave) {
    const uint64_t z = mix64(mix64(key ^ (0xA0761D6478BD642FULL * (uint64_t)(c + 1))) + 0x9E3779B97F4A7C15ULL);
    const double u = ((double)(z >> 12) + 0.5) * 0x1.0p-52;
    out[(size_t)b * kMaxChildren + c] = -log(-log(u));
  }
}

// One 64-bit key per board (hz_leaf_sym_keys: the key leaf_sym_of mixes with a
// leaf's node id; no reference counterpart): k_root_noise's board key under a
// salt of its own, so the noise, the move-choice uniform, the coin and the
// Gumbels keep their bits.
__global__ void __launch_bounds__(256) k_leaf_sym_keys(int n, uint64_t seed, uint64_t board_base, uint64_t move,
                                                       uint64_t *__restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  const uint64_t key = mix64(mix64(mix64(seed ^ 0x6A09E667F3BCC908ULL) ^ (board_base + (uint64_t)b)) ^ move);
  out[b] = mix64(key ^ 0xC2B2AE3D27D4EB4FULL);
}

}  // namespace

extern "C" {

int hz_root_noise(const int32_t *count, int32_t n, uint64_t seed, uint64_t board_base, uint64_t move, double alpha,
                  double *noise, double *u, void *stream) {
  if (n < 0 || !count || !noise || !(alpha > 0.0)) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_root_noise, dim3(n), dim3(kWave), 0, (hipStream_t)stream, count, n, seed, board_base, move,
                     alpha, noise, u);
  return launch_err();
}

int hz_playout_coin(int32_t n, uint64_t seed, uint64_t board_base, uint64_t move, double *coin, void *stream) {
  if (n < 0 || !coin) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_playout_coin, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, seed, board_base,
                     move, coin);
  return launch_err();
}

int hz_root_noise_at(const int32_t *count, int32_t n, uint64_t seed, uint64_t board_base, const uint64_t *move,
                     const uint8_t *mask, double alpha, double *noise, double *u, void *stream) {
  if (n < 0 || !count || !move || !mask || !noise || !(alpha > 0.0)) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_root_noise_at, dim3(n), dim3(kWave), 0, (hipStream_t)stream, count, n, seed, board_base, move,
                     mask, alpha, noise, u);
  return launch_err();
}

int hz_playout_coin_at(int32_t n, uint64_t seed, uint64_t board_base, const uint64_t *move, const uint8_t *mask,
                       double *coin, void *stream) {
  if (n < 0 || !move || !mask || !coin) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_playout_coin_at, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, seed, board_base,
                     move, mask, coin);
  return launch_err();
}

int hz_root_gumbel(int32_t n, uint64_t seed, uint64_t board_base, uint64_t move, double *out, void *stream) {
  if (n < 0 || !out) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_root_gumbel, dim3(n), dim3(kWave), 0, (hipStream_t)stream, n, seed, board_base, move, out);
  return launch_err();
}

int hz_leaf_sym_keys(int32_t n, uint64_t seed, uint64_t board_base, uint64_t move, uint64_t *out, void *stream) {
  if (n < 0 || !out) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_leaf_sym_keys, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, seed, board_base,
                     move, out);
  return launch_err();
}

}  // extern "C"
