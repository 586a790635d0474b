// hz_train.hip — the training side's kernels over packed records: the record
// transform under a board symmetry (hz_sym_records) and one training batch
// (board, glob, pi, z) per launch, each item under a symmetry of its own
// (hz_train_batch).  The rule is in include/hz_abi.h ("board symmetries"),
// the cell permutation in hz_sym.hpp, the encoder in hz_encode.hpp.  A
// translation unit of its own: the env's and the search's objects do not
// change with it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/hz_abi.h"
#include "hz_device.hpp"
#include "hz_encode.hpp"
#include "hz_host.hpp"

using namespace hz;
using namespace hz_host;

namespace {

// ------------------------------------------------ records and symmetries
// A packed training record (hzamd.distributed): 42 u64 words = the six state
// words | 143 u16 slots (visit counts, or the quantised improved policy) |
// int8 z | int8 player.  Records are 8-byte aligned.
constexpr int kRecWords = 42, kRecTail = kRecWords - 6;
constexpr int kRecWaves = 4;  // records per 256-thread block

// out[j] = rec[j] under sym[j] & 3, one wave per record: lane w holds word
// w, the tail words go through the wave's LDS row so that each lane can
// gather the four slots of its output word (slot a of the image is slot
// sym_action(a) of the source: the map is an involution).  The whole record
// is in registers and LDS before the first store, so out may be rec.
__global__ void __launch_bounds__(64 * kRecWaves) k_sym_records(const uint64_t *rec, long m,
                                                                const uint8_t *__restrict__ sym, uint64_t *out) {
  __shared__ uint64_t stail[kRecWaves][kRecTail];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long j = (long)blockIdx.x * kRecWaves + w;
  if (j >= m) return;  // (the whole wave)
  const int g = sym ? sym[j] & 3 : 0;
  uint64_t word = 0;
  if (lane < kRecWords) word = rec[j * kRecWords + lane];
  if (lane >= 6 && lane < kRecWords) stail[w][lane - 6] = word;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane < 4) {
    word = sym_plane(word, g);
  } else if (lane >= 6 && lane < kRecWords) {
    const uint16_t *slot = reinterpret_cast<const uint16_t *>(stail[w]);
    const int a0 = 4 * (lane - 6);
    word = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int a = a0 + k;  // slot 143 is the z and player bytes
      word |= (uint64_t)slot[a < kActions ? sym_action(a, g) : a] << (16 * k);
    }
  }
  if (lane < kRecWords) out[j * kRecWords + lane] = word;
}

// One training batch from packed records: the wave that encodes the pair of
// items (j0, j0 + 1) also writes their policy targets (slot / slot sum: an
// exact integer sum, one f64 divide per slot, as hzamd.distributed.pi_of)
// and outcomes.  Rows of pi are 572 B: per-lane f32 stores, coalesced.
__global__ void __launch_bounds__(256) k_train_batch(const uint64_t *__restrict__ rec,
                                                     const int32_t *__restrict__ idx,
                                                     const uint8_t *__restrict__ sym, int m,
                                                     float *__restrict__ board, float *__restrict__ glob,
                                                     float *__restrict__ pi, float *__restrict__ z) {
  __shared__ uint64_t smask[kEncWaves][76];
  __shared__ float sval[kEncWaves][76];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long j0 = 2 * ((long)blockIdx.x * kEncWaves + w);
  encode_pair<true, true>(rec, 1, kRecWords, idx, m, board, glob, lane, j0, smask[w], sval[w], sym);
#pragma unroll
  for (int r = 0; r < 2; r++) {
    const long j = j0 + r;
    if (j >= m) break;  // (the whole wave)
    const long bi = idx ? (long)idx[j] : j;
    const int g = sym ? sym[j] & 3 : 0;
    const uint16_t *slot = bi >= 0 ? reinterpret_cast<const uint16_t *>(rec + bi * kRecWords + 6) : nullptr;
    int v[3], sum = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int a = lane + 64 * k;
      v[k] = slot && a < kActions ? (int)slot[sym_action(a, g)] : 0;
      sum += v[k];  // at most 143 * 65535
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int a = lane + 64 * k;
      if (a < kActions) pi[j * kActions + a] = sum > 0 ? (float)((double)v[k] / (double)sum) : 0.f;
    }
    if (lane == 0) z[j] = slot ? (float)(int8_t)reinterpret_cast<const uint8_t *>(slot)[2 * kActions] : 0.f;
  }
}

}  // namespace

extern "C" {

int hz_sym_records(const int64_t *rec, int64_t m, const uint8_t *sym, int64_t *out, void *stream) {
  const int64_t blocks = (m + kRecWaves - 1) / kRecWaves;
  if (m < 0 || blocks > 0x7fffffffll) return -1;
  if (m == 0) return 0;  // (an empty tensor's pointer may be NULL)
  if (!rec || !out) return -1;
  hipLaunchKernelGGL(k_sym_records, dim3((unsigned)blocks), dim3(64 * kRecWaves), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint64_t *>(rec), (long)m, sym, reinterpret_cast<uint64_t *>(out));
  return launch_err();
}

int hz_train_batch(const int64_t *rec, const int32_t *idx, const uint8_t *sym, int32_t m, float *board, float *glob,
                   float *pi, float *z, void *stream) {
  if (!rec || m < 0 || !board || !glob || !pi || !z) return -1;
  if (m == 0) return 0;
  const long pairs = ((long)m + 1) / 2;
  hipLaunchKernelGGL(k_train_batch, dim3((unsigned)((pairs + kEncWaves - 1) / kEncWaves)), dim3(256), 0,
                     (hipStream_t)stream, reinterpret_cast<const uint64_t *>(rec), idx, sym, m, board, glob, pi, z);
  return launch_err();
}

}  // extern "C"
