// hz_chance.hpp — what hz_play's two pipelines and hz_rollout share: the
// prepared pile script and the draw source that replays it, the turn-pair
// step, the script-building draws, and the row movers between HBM and LDS.
// Part of hz_env.hip's translation unit (included by it alone, after its
// diagnostic macros and block constants).
#pragma once

namespace {

// ------------------------------------------------------------ chance-ahead
// The piles a game draws do not depend on its moves: only a turn end draws
// (one pile: a turn takes exactly one of the five), the bag changes only by
// draws, and the stream only by draws.  So a board's whole chance sequence
// for an episode is fixed by its seed.  The preparing blocks of one hz_play
// launch (on CUs the playing blocks leave idle) seed the stream of each
// board's next episode and run its first kAheadDraws pile draws on the
// initial bag: they store the piles (9 bits each, packed), the stream
// cursor after each draw, and the stream.  The next launch plays such a
// board from the pile script; a game that needs more draws continues on the
// stored stream (slot, global memory) from the cursor after the last
// scripted draw.
constexpr int kAheadDraws = 24;             // 5 opening + 19 turn ends (rule games: at most 23)
constexpr int kAheadWords = (9 * kAheadDraws + 63) / 64;  // 4 u64: the piles, 9 bits each

// the rule hashes of an episode's first kRulePlies plies (rule games end by
// ply 72), computed by draw2's otherwise idle waves 1-3 and read by the
// playing wave a turn pair ahead; plies past them are hashed in place
constexpr int kRulePlies = 80;

// wait-error bits (hz_env_set_error_word): a bounded wait gave up
constexpr int32_t kWaitErrSeedRows = 1;  // k_rollout's seed stage: wave 0's pass-2 row progress
constexpr int32_t kWaitErrP2Twist = 2;   // k_play2's twist wave: P2c's progress
constexpr int kSpinLimitDefault = 1 << 22;
__device__ __forceinline__ void wait_failed(int32_t *err, int32_t bit) {
  if (err) __hip_atomic_fetch_or(err, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A board's prepared pile script in registers: up to kAheadDraws piles of 9
// bits, entry i at bit 9 i of the 256-bit value q3:q2:q1:q0 as run_script
// (below) and k_play2's draw stages pack it.  A shift queue, the next entry
// always in the low 9 bits: a select over the four words would become a
// dynamic index into a scratch copy.
struct PileScript {
  uint64_t q0, q1, q2, q3; // the rest of the script, next entry in the low 9 bits
  int d;                   // script entries consumed
  int nd;                  // script length (<= kAheadDraws)

  // the next script entry, unconditionally (the caller checked d < nd)
  __device__ __forceinline__ uint32_t pop() {
    uint32_t p9 = (uint32_t)q0 & 0x1FFu;
    q0 = (q0 >> 9) | (q1 << 55);
    q1 = (q1 >> 9) | (q2 << 55);
    q2 = (q2 >> 9) | (q3 << 55);
    q3 >>= 9;
    d++;
    return p9;
  }
  // the same by the lanes with `want` only, 0x1FF for the others: no branch,
  // for a wave whose wanting lanes all have an entry left
  __device__ __forceinline__ uint32_t pop_if(bool want) {
    uint32_t p9 = want ? (uint32_t)q0 & 0x1FFu : 0x1FFu;
    uint64_t n0 = (q0 >> 9) | (q1 << 55), n1 = (q1 >> 9) | (q2 << 55), n2 = (q2 >> 9) | (q3 << 55);
    q0 = want ? n0 : q0;
    q1 = want ? n1 : q1;
    q2 = want ? n2 : q2;
    q3 = want ? q3 >> 9 : q3;
    d += want ? 1 : 0;
    return p9;
  }
  // reset_state from a script of >= 5 entries: its first five are the
  // opening piles (a full bag always fills them), 45 bits laid out as the
  // piles word
  __device__ __forceinline__ void scripted_reset(State &s) {
    s.pl[0] = s.pl[1] = s.pl[2] = s.pl[3] = 0;
    uint64_t open = q0 & ((1ull << 45) - 1);
    s.piles = open | (5ull << 45);
    uint64_t misc = 0x1FF;  // empty hand, player 0, choose_pile
#pragma unroll
    for (int t = 0; t < 6; t++) misc = set_bits(misc, 11 + 5 * t, 5, (uint64_t)initial_count(t));
#pragma unroll
    for (int i = 0; i < 5; i++) apply_pile_fast(misc, (uint32_t)(open >> (9 * i)) & 0x1FFu);
    s.misc = misc;
    q0 = (q0 >> 45) | (q1 << 19);
    q1 = (q1 >> 45) | (q2 << 19);
    q2 = (q2 >> 45) | (q3 << 19);
    q3 >>= 45;
    d = 5;
  }
};

// run script entries [from, to) of a board's chance sequence on its LDS
// stream, recording packed piles and the cursor after each draw at
// cur[(i + 1) * cs] (a rolled loop: one copy of the sampling code, so the
// instruction cache holds it; the script word is picked by selects, not by
// a dynamic index).  StopOnTwist: end before a draw that twisted (the rows
// past the staged ones are not in LDS).  Returns the entries completed.
template <bool StopOnTwist = false>
__device__ __forceinline__ int run_script(StreamDraw<LdsMT> &d, uint64_t &bag, uint64_t q[kAheadWords],
                                          int32_t *__restrict__ cur, size_t cs, int from, int to) {
  static_assert(kAheadWords == 4, "script words");
  uint64_t q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
  int i = from;
#pragma unroll 1
  for (; i < to; i++) {
    uint32_t p9 = d(bag);
    if (StopOnTwist && d.m.tw != kAheadTwist) break;
    apply_pile_fast(bag, p9);  // 0x1FF: no tiles
    // the script's layout: entry i at bit 9 i of the 256-bit value
    // q3:q2:q1:q0 (PileScript pops 9 bits at a time from its low end)
    int bit = 9 * i, wd = bit >> 6, off = bit & 63;
    uint64_t lo = (uint64_t)p9 << off;
    uint64_t hi = off > 55 ? (uint64_t)p9 >> (64 - off) : 0ull;
    q0 |= wd == 0 ? lo : 0ull;
    q1 |= wd == 1 ? lo : wd == 0 ? hi : 0ull;
    q2 |= wd == 2 ? lo : wd == 1 ? hi : 0ull;
    q3 |= wd == 3 ? lo : wd == 2 ? hi : 0ull;
    cur[(size_t)(i + 1) * cs] = d.m.cursor();
  }
  q[0] = q0; q[1] = q1; q[2] = q2; q[3] = q3;
  return i;
}

__device__ __forceinline__ uint64_t initial_bag() {
  uint64_t bag = 0;
#pragma unroll
  for (int t = 0; t < 6; t++) bag = set_bits(bag, 11 + 5 * t, 5, (uint64_t)initial_count(t));
  return bag;
}

__device__ __forceinline__ uint64_t episode_seed(uint64_t seed_base, int b, int e) {
  return seed_base + (uint64_t)b + ((uint64_t)e << 32);
}

// The draws that do not come from the script (boards not prepared ahead, and
// a script's rare overrun) live out of line: one copy of the sampling code
// instead of one per refill site keeps the ply loop's code small.  State
// goes in and out by value so the caller's copy stays in registers.
struct SlowDrawOut {
  uint32_t p9;
  int mpos, mtw, gpos, gtw;
};

__device__ __noinline__ SlowDrawOut play_draw_slow(uint64_t misc, int lane, int mpos, int mtw, int scripted,
                                                    uint32_t *gw, int gcursor) {
  SlowDrawOut o;
  uint32_t p9;
  if (scripted) {
    MT gm(gw, gcursor);
    o.p9 = draw_pile(misc, gm, p9) ? p9 : 0x1FFu;
    o.mpos = mpos;
    o.mtw = mtw;
    o.gpos = gm.pos;
    o.gtw = gm.tw;
  } else {
    LdsMT m(lane, mpos | (mtw << 16));
    m.prefetch();
    o.p9 = draw_pile(misc, m, p9) ? p9 : 0x1FFu;
    o.mpos = m.pos;
    o.mtw = m.tw;
    o.gpos = gcursor & 0xFFFF;
    o.gtw = gcursor >> 16;
  }
  return o;
}

// k_rollout's draw source: the pile script of a board prepared ahead, then
// its slot stream; the LDS stream of every other board
struct PlayDraw : PileScript {
  LdsMT m;                 // stream in LDS (boards not prepared ahead, auto-reset games)
  bool scripted;           // replaying the prepared pile script
  bool fell;               // script exhausted: drawing from the slot stream
  MT gm;                   // slot stream (valid once fell)
  const int32_t *cur_tail; // cursor after the last scripted draw (global)

  __device__ __forceinline__ uint32_t operator()(uint64_t misc) { return take(misc, true); }

  // one draw per lane, any source
  __device__ __forceinline__ uint32_t draw_one(uint64_t misc) {
    if (scripted && d < nd) return pop();
    if (scripted && !fell) {
      gm = MT(gm.w, *cur_tail);
      fell = true;
    }
    SlowDrawOut o = play_draw_slow(misc, m.lane, m.pos, m.tw, scripted, gm.w, gm.cursor());
    m.pos = o.mpos;
    m.tw = o.mtw;
    gm.pos = o.gpos;
    gm.tw = o.gtw;
    return o.p9;
  }

  // both refills of a turn pair come from the script: two entries left (a
  // script holds <= 24 draws, so the bag still has >= 48 tiles and every
  // turn end refills exactly one pile)
  __device__ __forceinline__ bool pair_pops() const { return scripted && d + 2 <= nd; }

  // a draw by the lanes with `want` (0x1FF for the others): while every such
  // lane replays its script (wave-uniform test) a plain masked pop, else the
  // general per-lane path
  __device__ __forceinline__ uint32_t take(uint64_t misc, bool want) {
    bool fast = scripted && d < nd;
    if (__all(!want || fast)) return pop_if(want);
    uint32_t p9 = 0x1FFu;
    if (want) p9 = draw_one(misc);
    return p9;
  }
};

// a pair of whole turns (eight plies) on the rule hashes h; returns the plies
// played: 8, or 4 when the first turn ended the game
template <class Draw>
__device__ __forceinline__ int play_pair(State &s, Draw &draw, const uint32_t (&h)[8]) {
  int done = 4;
  if (__all(draw.pair_pops())) {  // the refills are plain pops
    play_turn_h<0, Draw, true>(s, draw, h[0], h[1], h[2], h[3]);
    if (phase_of(s.misc) != PH_OVER) {
      play_turn_h<1, Draw, true>(s, draw, h[4], h[5], h[6], h[7]);
      done = 8;
    }
  } else {
    play_turn_h<0>(s, draw, h[0], h[1], h[2], h[3]);
    if (phase_of(s.misc) != PH_OVER) {
      play_turn_h<1>(s, draw, h[4], h[5], h[6], h[7]);
      done = 8;
    }
  }
  return done;
}

// Copy the streams of boards set in `mask` between HBM (one contiguous span
// of nb x 624 words, board-major) and LDS ([624][65]); 16 B per thread-load,
// eight loads in flight per thread.
__device__ __forceinline__ void stage_mt(uint32_t *__restrict__ g, int nb, int tid, uint64_t mask, bool to_lds) {
  uint32_t *lds = hz_lds;
  constexpr int U = 8;
  int total4 = nb * (kMT / 4);
  for (int q0 = 0; q0 < total4; q0 += kStageThreads * U) {
    uint4 v[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      int q = q0 + u * kStageThreads + tid;
      int o = q * 4, bl = o / kMT, i = o - bl * kMT;
      if (q < total4 && ((mask >> bl) & 1)) {
        if (to_lds) {
          v[u] = reinterpret_cast<const uint4 *>(g)[q];
        } else {
          v[u].x = lds[i * kLdsStride + bl];
          v[u].y = lds[(i + 1) * kLdsStride + bl];
          v[u].z = lds[(i + 2) * kLdsStride + bl];
          v[u].w = lds[(i + 3) * kLdsStride + bl];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      int q = q0 + u * kStageThreads + tid;
      int o = q * 4, bl = o / kMT, i = o - bl * kMT;
      if (q < total4 && ((mask >> bl) & 1)) {
        if (to_lds) {
          lds[i * kLdsStride + bl] = v[u].x;
          lds[(i + 1) * kLdsStride + bl] = v[u].y;
          lds[(i + 2) * kLdsStride + bl] = v[u].z;
          lds[(i + 3) * kLdsStride + bl] = v[u].w;
        } else {
          reinterpret_cast<uint4 *>(g)[q] = v[u];
        }
      }
    }
  }
}

// rows [r0, r1) of the block's 64 boards, word-major HBM -> LDS [row][65];
// 16 B per thread-load, eight in flight (conflict-free LDS writes: a wave
// covers four rows, whose banks are shifted by one)
__device__ __forceinline__ void stage_rows(const uint32_t *__restrict__ slot, size_t nrow, int b0, int r0, int r1,
                                           int tid) {
  constexpr int U = 8;
  int total = (r1 - r0) * 16;
  for (int q0 = 0; q0 < total; q0 += kStageThreads * U) {
    uint4 v[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      int q = q0 + u * kStageThreads + tid;
      q = q < total ? q : total - 1;
      v[u] = *reinterpret_cast<const uint4 *>(slot + (size_t)(r0 + (q >> 4)) * nrow + b0 + (q & 15) * 4);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      int q = q0 + u * kStageThreads + tid;
      if (q < total) {
        uint32_t *d = hz_lds + (r0 + (q >> 4)) * kLdsStride + (q & 15) * 4;
        d[0] = v[u].x;
        d[1] = v[u].y;
        d[2] = v[u].z;
        d[3] = v[u].w;
      }
    }
  }
}

// all rows of the boards in `mask`, LDS -> word-major HBM (coalesced rows)
__device__ __forceinline__ void unstage_rows(uint32_t *__restrict__ slot, size_t nrow, int b0, int tid,
                                             uint64_t mask) {
  int lane = tid & 63;
  if (!((mask >> lane) & 1)) return;
  for (int r = tid >> 6; r < kMT; r += kStageThreads / 64)
    slot[(size_t)r * nrow + b0 + lane] = hz_lds[r * kLdsStride + lane];
}

// Rows [0, kAheadTwist) of the block's 64 boards from a slot holding the
// streams as seeded, word-major HBM -> LDS [row][65], written as the next
// generation's: row i from rows i, i + 1 and i + 397 of the slot (all still
// old), read straight from HBM (16 B per load, 12 in flight per thread), so
// the twist needs no LDS round trip and no barrier.
__device__ __forceinline__ void stage_rows_twisted(const uint32_t *__restrict__ slot, size_t nrow, int b0, int tid) {
  constexpr int U = 4;
  constexpr int total = kAheadTwist * 16;
  for (int q0 = 0; q0 < total; q0 += kStageThreads * U) {
    uint4 c[U], c1[U], f[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      int q = q0 + u * kStageThreads + tid;
      q = q < total ? q : total - 1;
      const uint32_t *p = slot + b0 + (q & 15) * 4;
      int r = q >> 4;
      c[u] = *reinterpret_cast<const uint4 *>(p + (size_t)r * nrow);
      c1[u] = *reinterpret_cast<const uint4 *>(p + (size_t)(r + 1) * nrow);
      f[u] = *reinterpret_cast<const uint4 *>(p + (size_t)(r + 397) * nrow);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      int q = q0 + u * kStageThreads + tid;
      if (q < total) {
        uint32_t *d = hz_lds + (q >> 4) * kLdsStride + (q & 15) * 4;
        d[0] = twist_word(c[u].x, c1[u].x, f[u].x);
        d[1] = twist_word(c[u].y, c1[u].y, f[u].y);
        d[2] = twist_word(c[u].z, c1[u].z, f[u].z);
        d[3] = twist_word(c[u].w, c1[u].w, f[u].w);
      }
    }
  }
}


}  // namespace
