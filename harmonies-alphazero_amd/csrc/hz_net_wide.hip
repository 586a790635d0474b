// The folded network at other widths (hzamd/infer.py): the x6 conv for
// cin, cout in {32, 64, .., 256} and the fused head for other head shapes.
//
// hz_net.hip's kernels are cut for 128 filters (model.py:277-394 with
// cnn_filters = 128); the reference's model_config takes any cnn_filters,
// value_head_hidden_dim and head filter counts (its test_model_config is
// 32 / 64 / 2 + 1).  The kernels here have k_conv3x3_x6's arithmetic with
// the channel counts as arguments:
//     every fp32 operand split exactly into three bf16 pieces (split4, the
//     same roundings), v_mfma_f32_16x16x32_bf16 accumulating in fp32, and per
//     output element one chain: chunks of 32 input channels ascending, taps
//     0..8, pa 0..Ord, pb 0..Ord - pa; then relu((acc + bias) + res).
// A tap off the 5x7 board reads a zero region (its MFMAs add exact zeros), so
// at cin = cout = 128 the result equals hz_conv3x3_x6_bias_act's and
// hz_conv3x3_xn_bias_act's bit for bit (those skip some of the zero taps).
//
// Two workgroup forms of 4 waves each, the same chain per row in both:
//   1 state  = 35 rows as 3 row blocks of 16; wave = 32 output channels
//              (grid.y covers cout in tiles of 128),
//   8 states = 280 rows as 18 row blocks; wave = (row half, 32 output
//              channels) with 9 x 2 accumulator tiles, so each B fragment
//              read from L2 feeds 280 rows instead of 35 (grid.y covers cout
//              in tiles of 64; a wave whose channels lie past cout stages and
//              waits at the barriers but issues no MFMA).
// Staging as k_conv3x3_x6: a chunk of 32 channels is split on the way into
// LDS, 224 B per cell (3 planes of 64 B + 32 B), double-buffered: 8 states
// take 2 x (62,720 + 512) = 126,464 B of the 160 KB.  No workgroup waits on
// another; every loop bound is a function of the arguments.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/hz_abi.h"
#include "hz_host.hpp"

using namespace hz_host;

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_v;
typedef __attribute__((ext_vector_type(2))) float f32x2_v;

constexpr int kCell = 224;     // bytes per staged cell (k_conv3x3_x6's kX6Cell)
constexpr int kZeroB = 512;    // bytes of zeros behind a chunk's cells
constexpr int kBoardC = 38;    // encoder board channels (stem input)

__device__ __forceinline__ uint32_t bf16_pair(float a, float b) {
  const f32x2_v f = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2_v));
}
__device__ __forceinline__ float bf16_lo(uint32_t p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t p) { return __uint_as_float(p & 0xffff0000u); }

// the three bf16 planes of four consecutive channels (hz_net.hip's split4:
// round to nearest even at each step, h + m + l == v exactly)
__device__ __forceinline__ void split4(const f32x4 v, uint2 &h, uint2 &m, uint2 &l) {
  const uint32_t h01 = bf16_pair(v[0], v[1]), h23 = bf16_pair(v[2], v[3]);
  const float r0 = v[0] - bf16_lo(h01), r1 = v[1] - bf16_hi(h01);
  const float r2 = v[2] - bf16_lo(h23), r3 = v[3] - bf16_hi(h23);
  const uint32_t m01 = bf16_pair(r0, r1), m23 = bf16_pair(r2, r3);
  const float s0 = r0 - bf16_lo(m01), s1 = r1 - bf16_hi(m01);
  const float s2 = r2 - bf16_lo(m23), s3 = r3 - bf16_hi(m23);
  h = make_uint2(h01, h23);
  m = make_uint2(m01, m23);
  l = make_uint2(bf16_pair(s0, s1), bf16_pair(s2, s3));
}

// CS states per workgroup (8 or 1).  Stem: x is the encoder's NCHW board
// [B][38][5][7], staged as two chunks (channels >= 38 are zeros; channel 37
// is split like any other value); else an NHWC [B][5][7][cin] activation.
// out, res: NHWC [B][5][7][cout].  wp: bf16 planes [tap][cin/32][plane][cout][32].
// Ord: the piece products kept are those with pa + pb <= Ord.
template <int CS, bool Stem, int Ord>
__global__ void __launch_bounds__(256)
    k_conv3x3_x6g(const float *__restrict__ x, const bf16x8 *__restrict__ wp, const float *__restrict__ bias,
                  const float *__restrict__ res, float *__restrict__ out, int32_t cin, int32_t cout, int32_t batch,
                  const int32_t *__restrict__ live) {
  static_assert(CS == 8 || CS == 1, "8 or 1 states per workgroup");
  constexpr int kRowsT = CS * 35;                 // output rows of the group
  constexpr int kRG = CS == 8 ? 2 : 1;            // row groups of waves
  constexpr int kCW = 4 / kRG;                    // waves across the output channels, 32 each
  constexpr int kRBT = CS == 8 ? 9 : 3;           // row blocks of 16 per wave
  constexpr int kStg = (kRowsT * 8 + 255) / 256;  // float4 staged per thread per chunk
  constexpr int kZero = (kRowsT * kCell + 255) / 256 * 256;  // zero region: 256-B aligned
  constexpr int kBufT = kZero + kZeroB;
  static_assert(kRG * kRBT * 16 >= kRowsT, "row blocks cover the rows");
  extern __shared__ float4 lds4[];
  char *lds = (char *)lds4;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, kg = lane >> 4, rg = w / kCW, cw = w % kCW;
  const int s0 = blockIdx.x * CS;
  if (live) batch = *live < batch ? *live : batch;  // rows past the live count are neither read nor written
  if (s0 >= batch) return;
  const int ns = batch - s0 < CS ? batch - s0 : CS;
  const int nq = Stem ? 2 : cin / 32;

  if (t < 2 * kZeroB / 16) {  // both buffers' zero regions
    const int b = t / (kZeroB / 16), k = t - b * (kZeroB / 16);
    *(float4 *)(lds + b * kBufT + kZero + 16 * k) = make_float4(0.f, 0.f, 0.f, 0.f);
  }

  // staging: float4 f of a chunk = (row f >> 3, channels 4 (f & 7) ..); the
  // states past the last live one restage that one (computed, not stored)
  f32x4 stg[kStg];
  int grow[kStg], gpart[kStg], ldst[kStg];
#pragma unroll
  for (int it = 0; it < kStg; it++) {
    int f = it * 256 + t;
    f = f < kRowsT * 8 ? f : kRowsT * 8 - 1;
    const int sc = f >> 3, part = f & 7, s = sc / 35, cell = sc - 35 * s;
    if constexpr (Stem)
      grow[it] = (s0 + (s < ns ? s : ns - 1)) * (kBoardC * 35) + cell;  // + channel * 35
    else
      grow[it] = (s0 + (s < ns ? s : ns - 1)) * 35 + cell;              // x row
    gpart[it] = 4 * part;
    ldst[it] = sc * kCell + 8 * part;
  }
  auto load = [&](int q) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < kStg; it++) {
      if constexpr (Stem) {
        const int c0 = 32 * q + gpart[it];
#pragma unroll
        for (int j = 0; j < 4; j++) stg[it][j] = c0 + j < kBoardC ? x[(size_t)grow[it] + (c0 + j) * 35] : 0.f;
      } else {
        stg[it] = *(const f32x4 *)(x + (size_t)grow[it] * cin + 32 * q + gpart[it]);
      }
    }
  };
  auto store = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < kStg; it++) {
      uint2 h, m, l;
      split4(stg[it], h, m, l);
      char *d = lds + buf * kBufT + ldst[it];
      *(uint2 *)d = h;
      if constexpr (Ord >= 1) *(uint2 *)(d + 64) = m;
      if constexpr (Ord >= 2) *(uint2 *)(d + 128) = l;
    }
  };

  // A fragment of row block rb: the lane's row (rg * kRBT + rb) * 16 + (lane & 15)
  // (clamped: the rows past the group's are not stored), 16 B at K slice kg
  int cbase[kRBT];
  uint32_t valid[kRBT];
#pragma unroll
  for (int rb = 0; rb < kRBT; rb++) {
    int r = (rg * kRBT + rb) * 16 + (lane & 15);
    r = r < kRowsT ? r : kRowsT - 1;
    const int cell = r % 35, ch = cell / 7, cwc = cell - 7 * ch;
    cbase[rb] = r * kCell + 16 * kg;
    uint32_t v = 0;
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
      const int hh = ch + tap / 3 - 1, ww = cwc + tap % 3 - 1;
      v |= (uint32_t)(hh >= 0 && hh < 5 && ww >= 0 && ww < 7) << tap;
    }
    valid[rb] = v;
  }
  // the neighbour's cell or, off the board, the zero region at the same
  // offset mod 256 (at most 255 + 2 planes + 16 B < kZeroB)
  auto aoff = [&](int rb, int tap) -> int {
    const int a = cbase[rb] + ((tap / 3 - 1) * 7 + (tap % 3 - 1)) * kCell;
    return (valid[rb] >> tap) & 1 ? a : kZero + (a & 255);
  };

  f32x4 acc[kRBT][2];
#pragma unroll
  for (int rb = 0; rb < kRBT; rb++) acc[rb][0] = acc[rb][1] = (f32x4){};

  // this wave's 32 output channels; a wave past cout only stages
  const int cob = ((int)blockIdx.y * kCW + cw) * 32;
  const bool active = cob < cout;
  // B fragment of (chunk q, tap), plane p, column block cb:
  // wp[(((tap * nq + q) * 3 + p) * cout + cob + 16 cb + (lane & 15)) * 4 + kg]
  const bf16x8 *wl = wp + (size_t)(cob + (lane & 15)) * 4 + kg;
  auto bload = [&](int q, int tap, int p, int cb) -> bf16x8 {
    return wl[(size_t)((tap * nq + q) * 3 + p) * cout * 4 + 64 * cb];
  };

  load(0);
  store(0);
  __syncthreads();

  bf16x8 b[3][2], bn[3][2];  // this K-step's B fragments, the next step's
  if (active) {
#pragma unroll
    for (int p = 0; p <= Ord; p++)
#pragma unroll
      for (int cb = 0; cb < 2; cb++) b[p][cb] = bload(0, 0, p, cb);
  }

  for (int q = 0; q < nq; q++) {
    const char *lb = lds + (q & 1) * kBufT;
    const bool more = q + 1 < nq;
    if (more) load(q + 1);
    if (active) {
      // A fragments a step (tap, pa) ahead of their MFMAs: with one wave per
      // SIMD nothing else covers the LDS latency
      bf16x8 a[2][kRBT];
#pragma unroll
      for (int rb = 0; rb < kRBT; rb++) a[0][rb] = *(const bf16x8 *)(lb + aoff(rb, 0));
#pragma unroll
      for (int tap = 0; tap < 9; tap++) {
        const int qn = tap < 8 ? q : (more ? q + 1 : q), tn = tap < 8 ? tap + 1 : (more ? 0 : 8);
#pragma unroll
        for (int p = 0; p <= Ord; p++)
#pragma unroll
          for (int cb = 0; cb < 2; cb++) bn[p][cb] = bload(qn, tn, p, cb);
#pragma unroll
        for (int pa = 0; pa <= Ord; pa++) {
          constexpr int kSteps = 9 * (Ord + 1);
          const int st = tap * (Ord + 1) + pa, cur = st & 1;
          if (st + 1 < kSteps) {
            const int tap1 = (st + 1) / (Ord + 1), pa1 = (st + 1) % (Ord + 1);
#pragma unroll
            for (int rb = 0; rb < kRBT; rb++) a[cur ^ 1][rb] = *(const bf16x8 *)(lb + aoff(rb, tap1) + 64 * pa1);
          }
#pragma unroll
          for (int pb = 0; pb <= Ord - pa; pb++)
#pragma unroll
            for (int rb = 0; rb < kRBT; rb++)
#pragma unroll
              for (int cb = 0; cb < 2; cb++)
                acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[cur][rb], b[pb][cb], acc[rb][cb], 0, 0, 0);
        }
#pragma unroll
        for (int p = 0; p <= Ord; p++)
#pragma unroll
          for (int cb = 0; cb < 2; cb++) b[p][cb] = bn[p][cb];
      }
    }
    // the other buffer was last read for chunk q - 1, before the barrier
    // that ended iteration q - 1
    if (more) {
      store((q + 1) & 1);
      __syncthreads();
    }
  }
  if (!active) return;

  // epilogue: accumulator register j of a lane is row 4 kg + j, column lane & 15
  const int nrow = ns * 35;
#pragma unroll
  for (int cb = 0; cb < 2; cb++) {
    const int co = cob + 16 * cb + (lane & 15);
    const float bc = bias[co];
#pragma unroll
    for (int rb = 0; rb < kRBT; rb++) {
      const int rbase = (rg * kRBT + rb) * 16 + 4 * kg;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (rbase + j < nrow) {
          const size_t o = ((size_t)s0 * 35 + rbase + j) * cout + co;
          float v = acc[rb][cb][j] + bc;
          if (res) v = v + res[o];
          out[o] = v > 0.f ? v : 0.f;
        }
      }
    }
  }
}

template <int CS, bool Stem, int Ord>
int launch_g(const float *x, const void *wpack6, const float *bias, const float *res, float *out, int32_t cin,
             int32_t cout, int32_t batch, const int32_t *live, void *stream) {
  const size_t lds = 2 * (size_t)((CS * 35 * kCell + 255) / 256 * 256 + kZeroB);
  if (lds_opt_in<k_conv3x3_x6g<CS, Stem, Ord>>(lds)) return 1;
  const int tile = CS == 8 ? 64 : 128;  // output channels per workgroup
  hipLaunchKernelGGL((k_conv3x3_x6g<CS, Stem, Ord>), dim3((batch + CS - 1) / CS, (cout + tile - 1) / tile), dim3(256),
                     lds, (hipStream_t)stream, x, (const bf16x8 *)wpack6, bias, res, out, cin, cout, batch, live);
  return launch_err() ? 1 : 0;
}

// spg = 0: batches up to this many rows run one state per workgroup.  The
// two forms' measured predict times cross at ~2,890 rows for 64 filters and
// ~420 for 256, and not up to 4,096 for 32 (tools/width_bench.py,
// profiles/r12): the one-state form re-reads the conv's whole pack per state,
// which costs more the wider the conv.  The default is the power law through
// the two measured crossings, in cin * cout (7,550 rows at 32 x 32; the
// widths between are interpolated, not measured).  HZ_X6G_SMALL_MAX
// overrides it for every width (A/B measurements).
int32_t g_small_max(int32_t cin, int32_t cout) {
  static const int32_t v = env_int("HZ_X6G_SMALL_MAX", -1);
  if (v >= 0) return v;
  return (int32_t)(2887.0 * pow(4096.0 / ((double)cin * cout), 0.6935));
}

bool width_ok(int32_t c) { return c >= 32 && c <= 256 && c % 32 == 0; }

template <bool Stem, int Ord>
int launch_g_spg(const float *x, const void *wpack6, const float *bias, const float *res, float *out, int32_t cin,
                 int32_t cout, int32_t batch, const int32_t *live, int32_t spg, void *stream) {
  if (spg == 0) spg = batch <= g_small_max(cin, cout) ? 1 : 8;
  return spg == 1 ? launch_g<1, Stem, Ord>(x, wpack6, bias, res, out, cin, cout, batch, live, stream)
                  : launch_g<8, Stem, Ord>(x, wpack6, bias, res, out, cin, cout, batch, live, stream);
}

}  // namespace

extern "C" int hz_conv3x3_x6g_bias_act(const float *x, const void *wpack6, const float *bias, const float *res,
                                       float *out, int32_t cin, int32_t cout, int32_t batch, const int32_t *live,
                                       int32_t products, int32_t spg, void *stream) {
  if (!x || !wpack6 || !bias || !out || batch < 0 || !width_ok(cin) || !width_ok(cout)) return -1;
  if (products != 6 && products != 3 && products != 1) return -1;
  if (spg != 0 && spg != 1 && spg != 8) return -1;
  if (((uintptr_t)x | (uintptr_t)wpack6 | (uintptr_t)out | (uintptr_t)res) & 15) return -1;
  if (batch == 0) return 0;
  if (products == 6) return launch_g_spg<false, 2>(x, wpack6, bias, res, out, cin, cout, batch, live, spg, stream);
  if (products == 3) return launch_g_spg<false, 1>(x, wpack6, bias, res, out, cin, cout, batch, live, spg, stream);
  return launch_g_spg<false, 0>(x, wpack6, bias, res, out, cin, cout, batch, live, spg, stream);
}

extern "C" int hz_stem3x3_x6g_bias_act(const float *board, const void *wpack6, const float *bias, float *out,
                                       int32_t cout, int32_t batch, const int32_t *live, int32_t spg, void *stream) {
  if (!board || !wpack6 || !bias || !out || batch < 0 || !width_ok(cout)) return -1;
  if (spg != 0 && spg != 1 && spg != 8) return -1;
  if (((uintptr_t)wpack6 | (uintptr_t)out) & 15) return -1;
  if (batch == 0) return 0;
  return launch_g_spg<true, 2>(board, wpack6, bias, nullptr, out, 64, cout, batch, live, spg, stream);
}

// ---- the whole head for other shapes ----------------------------------------
//
// model.py:336-355 with BN folded, one 256-thread workgroup per state, fp32
// FMAs; every sum runs in one order whatever the batch:
//   1x1 convs: channels ascending, + bias, ReLU -> pcat (pf * 35 in NCHW
//     flatten order || 42 globals), vcat (vf * 35 || 42 globals);
//   logits[a] = sum over k ascending of pcat[k] * wpT[k][a], + bp[a];
//   hidden[u] = relu(sum over k ascending of vcat[k] * w1T[k][u], + b1[u]);
//   value = tanh(tree sum of hidden[u] * w2[u] + b2): thread t takes
//     u = t, t + 256, .. ascending, then the fixed halving tree below;
//   probs = softmax(logits) through the same tree (max, then sum).
namespace {

constexpr int kHCells = 35, kHGlob = 42, kHAct = 143;
constexpr int kHMaxF = 4, kHMaxCh = 256, kHMaxHidden = 1024;

template <bool Max>
__device__ __forceinline__ float tree256(float v, float *red, int t) {
  red[t] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s >= 1; s >>= 1) {
    if (t < s) red[t] = Max ? fmaxf(red[t], red[t + s]) : red[t] + red[t + s];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(256)
    k_heads_fc_g(const float *__restrict__ x, const float *__restrict__ glob, const float *__restrict__ hw,
                 const float *__restrict__ hb, const float *__restrict__ wpT, const float *__restrict__ bp,
                 const float *__restrict__ w1T, const float *__restrict__ b1, const float *__restrict__ w2,
                 const float *__restrict__ b2, float *__restrict__ logits, float *__restrict__ probs,
                 float *__restrict__ value, int32_t ch, int32_t pf, int32_t vf, int32_t hidden, int32_t batch,
                 const int32_t *__restrict__ live) {
  __shared__ float xs[kHCells * (kHMaxCh + 1)];  // the state's activation, rows padded by one float (banks)
  __shared__ float hws[2 * kHMaxF * kHMaxCh];
  __shared__ float pcat[kHMaxF * kHCells + kHGlob], vcat[kHMaxF * kHCells + kHGlob];
  __shared__ float lg[kHAct], red[256];
  const int t = threadIdx.x, s = blockIdx.x;
  if (live) batch = *live < batch ? *live : batch;
  if (s >= batch) return;
  const int nf = pf + vf, np = pf * kHCells + kHGlob, nv = vf * kHCells + kHGlob;
  const float *xr = x + (size_t)s * kHCells * ch;
  for (int i = t; i < kHCells * ch; i += 256) xs[(i / ch) * (ch + 1) + i % ch] = xr[i];
  for (int i = t; i < nf * ch; i += 256) hws[i] = hw[i];
  if (t < kHGlob) pcat[pf * kHCells + t] = vcat[vf * kHCells + t] = glob[(size_t)s * kHGlob + t];
  __syncthreads();
  for (int o = t; o < nf * kHCells; o += 256) {
    const int f = o / kHCells, cell = o - f * kHCells;
    const float *xc = xs + cell * (ch + 1), *wc = hws + f * ch;
    float a = 0.f;
    for (int c = 0; c < ch; c++) a = fmaf(xc[c], wc[c], a);
    a = a + hb[f];
    a = a > 0.f ? a : 0.f;
    if (f < pf)
      pcat[o] = a;
    else
      vcat[o - pf * kHCells] = a;
  }
  __syncthreads();
  if (t < kHAct) {
    float a = 0.f;
    for (int k = 0; k < np; k++) a = fmaf(pcat[k], wpT[k * kHAct + t], a);
    a = a + bp[t];
    lg[t] = a;
    if (logits) logits[(size_t)s * kHAct + t] = a;
  }
  float part = 0.f;
  for (int u = t; u < hidden; u += 256) {
    float a = 0.f;
    for (int k = 0; k < nv; k++) a = fmaf(vcat[k], w1T[(size_t)k * hidden + u], a);
    a = a + b1[u];
    a = a > 0.f ? a : 0.f;
    part = fmaf(a, w2[u], part);
  }
  const float vsum = tree256<false>(part, red, t);  // (its first barrier also publishes lg)
  if (t == 0) value[s] = tanhf(vsum + b2[0]);
  if (probs) {
    const float l = t < kHAct ? lg[t] : -INFINITY;
    const float mx = tree256<true>(l, red, t);
    const float e = t < kHAct ? expf(l - mx) : 0.f;
    const float sum = tree256<false>(e, red, t);
    if (t < kHAct) probs[(size_t)s * kHAct + t] = e / sum;
  }
}

}  // namespace

extern "C" int hz_heads_fc_g(const float *x, const float *glob, const float *hw, const float *hb, const float *wpT,
                             const float *bp, const float *w1T, const float *b1, const float *w2, const float *b2,
                             float *logits, float *probs, float *value, int32_t ch, int32_t pf, int32_t vf,
                             int32_t hidden, int32_t batch, const int32_t *live, void *stream) {
  if (!x || !glob || !hw || !hb || !wpT || !bp || !w1T || !b1 || !w2 || !b2 || !value || batch < 0) return -1;
  if (!width_ok(ch) || pf < 1 || pf > kHMaxF || vf < 1 || vf > kHMaxF || hidden < 1 || hidden > kHMaxHidden)
    return -1;
  if (batch == 0) return 0;
  hipLaunchKernelGGL(k_heads_fc_g, dim3(batch), dim3(256), 0, (hipStream_t)stream, x, glob, hw, hb, wpT, bp, w1T, b1,
                     w2, b2, logits, probs, value, ch, pf, vf, hidden, batch, live);
  return launch_err() ? 1 : 0;
}
