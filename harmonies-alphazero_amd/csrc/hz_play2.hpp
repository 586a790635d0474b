// hz_play2.hpp — k_play2, hz_play's second pipeline, and the kernel that
// rebuilds a board's own stream after it.  Part of hz_env.hip's translation
// unit (included by it alone, after hz_chance.hpp and hz_rollout.hpp; P2Draw,
// P2Mid and the kP2* stage counts sit with struct hz_env, which is sized by
// them).
#pragma once

namespace {

// ============================================================= pipeline 2
// hz_play's second pipeline (hz_env_set_pipeline(e, 2)).  Each of
// k_rollout's roles runs one serial per-board chain of ~60 k cycles (a whole
// game, a whole seeding, 16 pile draws), and a launch lasts as long as its
// longest chain.  Here every board's episode is cut into fifteen stages of
// about 20 k cycles, one per consecutive hz_play call, and one launch runs
// all fifteen at once, each on a different episode of the board (ep = the
// episode counter the previous call left, p2_ep; stage s works on episode
// ep + 14 - s).  The wave of each stage outside the seed and play blocks is
// kP2Wave's (HZ_P2_WAVES); by default:
//   s = 0  P1    seeding pass 1, all 624 steps, in     draw-Y blocks, wave 2
//                registers: only its last word leaves
//   s = 1  P2a   pass 2, steps 2-208: stores the      seed blocks, wave 0
//                twist parts of rows 2-161
//   s = 2  P2b   pass 2, steps 209-432: stores rows   seed blocks, wave 1
//                393-432
//   s = 3  P2c   pass 2, steps 433-624, rows 433-560  seed blocks, wave 2
//                kept in LDS; rows 0-159 of the next  (twist: wave 3)
//                generation twisted
//          (each of s = 0..3 then computes its rows of the episode's 80 rule
//          hashes, kP2HashCut, from the seed it holds, behind its chain)
//   s = 4  D1    pile draws [dcut0 = 0, dcut1), from  draw-X blocks, wave 0
//                slot rows [L, L + 96), L = 3 dcut & ~3
//   s = 5  D2    draws [dcut1, dcut2)                 draw-X blocks, wave 1
//   s = 6  D3    draws [dcut2, dcut3)                 draw-Y blocks, wave 0
//   s = 7  D4    draws [dcut3, dcut4)                 draw-Y blocks, wave 1
//   s = 8  D5    draws [dcut4, dcut5)                 draw-X blocks, wave 2
//   s = 9  D6    draws [dcut5, 24)                    draw-X blocks, wave 3
//   s = 10 playA plies [0, cut0)                      draw-Y blocks, wave 3
//   s = 11 playB plies [cut0, cut1)                   play blocks, wave 3
//   s = 12 playC plies [cut1, cut2)                   play blocks, wave 2
//   s = 13 playD plies [cut2, cut3)                   play blocks, wave 1
//   s = 14 playE the rest, final scoring, the board's play blocks, wave 0
//                state, cursor and counters
// (-DHZ_P2_NDRAW=5: fourteen stages, draw-X wave 3 idle.)
// Pass 1 never reaches memory: a pass-1 word is a function of the board's key
// and the constant kInitGen table, so P1 hands on only what pass 2's last
// step needs (row 1's word after the 624th step), and each pass-2 stage
// recomputes pass 1 over its own rows next to its pass-2 chain (a second,
// independent recurrence of four VALU operations per step), started from
// pass 1's word at the row before its range: one step from the constants for
// P2a, handed on with pass 2's value for P2b and P2c.
// An episode's stream lives in one slot of a ring of kP2Stream from P2a to
// playE; stage s >= 1 of call c uses slot (c - s) mod kP2Stream.  A slot
// holds what the stages read and no more: the next generation's rows below
// kP2Twist (the draw stages' windows, a play stage past its script) and, on
// the way there, the twist's inputs (the parts of those rows, the old
// generation's rows 397 .. kP2bEnd - 1).  Nothing else of pass 2 reaches
// memory.  A game that would read past row kP2Twist is played again from
// scratch by playE, and the board's own stream, when another entry point
// needs it, is rebuilt from the episode's seed (k_mt_materialize2).  A
// stage uses an input only when its tag names the stage's episode, so a wrong
// prediction costs time, never results: the stages skip the board and playE
// plays its whole game from scratch (seeding and drawing in LDS, like
// k_rollout's unprepared boards).  The episode's rule hashes live in a ring
// entry that goes with the slot (same index; P1, which has no slot, writes
// the entry P2a adopts in the next call) and have no tag of their own: every
// seeding stage stores its hash rows before its tag, and each tests the
// previous stage's tag (P2a P1's, P2b P2a's, P2c P2b's), so a slot tagged
// "seeded for e" has all of e's rows, and the last draw stage's script tag,
// the one a play stage tests, is given only on such a slot.  An entry is next
// written by P1 one call after the last play stage read it.
// The results are k_rollout's: the board ends
// the call with episode ep's final state, cursor and counters, and
// games_done / steps_done count that game (its first plies ran in the four
// calls before, in playA to playD).  In steady state a call does every stage
// once per board: one game's worth of work per board per call.
#ifndef HZ_P2_ST_WT
// 1: the hand-off stores (hashes, cursors, scripts, mid-game states) write-
// through too (global_store ... sc1): 17.0 G against 18.3 G with them plain
// (profiles/r05/p2_writethrough), so plain by default
#define HZ_P2_ST_WT 0
#endif
#ifndef HZ_P2_AUX
// cache policy of the seeding stages' and the twist's stream-slot stores
// (~24 MB per 4096-board launch): 16 = sc1, write-through, the line dropped
// from the XCD's L2 (the next call's stages read them, from the MALL), so
// the kernel's end finds no dirty slot lines to write back: 14.1 vs 15.8 us
// per launch against plain stores (0), 15.5 with nt (2)
// (profiles/r05/p2_writethrough; A/B builds -DHZ_P2_AUX=0 / 2)
#define HZ_P2_AUX 16
#endif
#ifndef HZ_P2_STATIC_WIN
#define HZ_P2_STATIC_WIN 1
#endif
constexpr bool kP2StaticWin = HZ_P2_STATIC_WIN;

constexpr int kP2Win = 96;        // rows a draw stage stages, from row (3 dcut[stage]) & ~3 (p2_draw_stage)
constexpr int kP2WinRows = kP2Win + 24;  // LDS rows per window (a scan reads up to 23 rows past its cursor)
#ifndef HZ_P2_DCUT
// the draw stages' first draws (run time: HZ_P2_DCUTS).  Later draws take
// longer, so the early stages take more of them: with four stages of six, D3
// ran 13.8 us against D1's 10.5, and the cuts became 0, 7, 13, 18
// (profiles/r05/p2_dcut); five stages: profiles/r07, and profiles/r09 since
// the first stage loads its window in its first round trip and takes a sixth
// draw from the last.  Six stages: profiles/r22 (every scanned set passes
// tests/test_p2_windows6_cpu.py first).
#if HZ_P2_NDRAW == 6
#define HZ_P2_DCUT 0, 5, 9, 13, 17, 20
#elif HZ_P2_NDRAW == 5
#define HZ_P2_DCUT 0, 6, 11, 15, 19
#elif HZ_P2_NDRAW == 4
#define HZ_P2_DCUT 0, 7, 13, 18
#endif
#endif
constexpr int kP2DCut[kP2Draw] = {HZ_P2_DCUT};
// A draw stage's window holds kP2Win rows from row (3 dcut[stage]) & ~3.
// Seven draws (the most a stage ever had) use at most ~60 words (eight
// consecutive draws: 67 over 20,000 seeds), which leaves room for the
// cursors' spread at the stage's start: over 1,000,000 simulated streams
// with the default cuts no stage's last draw ended past its window
// (tests/test_p2_windows_cpu.py).  A draw that does is discarded and redone
// by a later stage: time, never results.
constexpr int kP2StageDraws = 7;
#ifndef HZ_P2_PCUT
// the play stages' ply boundaries (run time: HZ_P2_CUTS5; four stages:
// HZ_P2_CUTS).  Multiples of 8: a stage that starts inside a turn pair plays
// single plies up to the next pair, and every such setting measured slower
// (profiles/r07/cuts_scan.json).
#if HZ_P2_NPLAY == 5
#define HZ_P2_PCUT 16, 32, 48, 64
#elif HZ_P2_NPLAY == 4
#define HZ_P2_PCUT 24, 40, 56
#endif
#endif
constexpr int kP2PCut[kP2Play - 1] = {HZ_P2_PCUT};
// what each wave of a draw-X (first four) and a draw-Y block runs: a draw
// stage (0 .. kP2Draw - 1), P1, play stage 0, or nothing.  (The rule hashes
// had a wave of their own, draw-X wave 3, until the seeding stages took them:
// kP2HashCut.)
// (A play wave brings the ply loop's ~50 KB of code into its CU pair's
// instruction cache next to the draw code.)
enum { kWvP1 = 8, kWvPlay = 10, kWvIdle = 15 };
#ifndef HZ_P2_WAVES
#if HZ_P2_NDRAW == 6 && HZ_P2_NPLAY == 5
#define HZ_P2_WAVES 0, 1, 4, 5, 2, 3, 8, 10
#elif HZ_P2_NDRAW == 6
#define HZ_P2_WAVES 0, 1, 4, 5, 2, 3, 8, 15
#elif HZ_P2_NDRAW == 5 && HZ_P2_NPLAY == 5
#define HZ_P2_WAVES 0, 1, 4, 15, 2, 3, 8, 10
#elif HZ_P2_NDRAW == 5
#define HZ_P2_WAVES 0, 1, 4, 15, 2, 3, 8, 15
#elif HZ_P2_NPLAY == 5
#define HZ_P2_WAVES 0, 1, 8, 15, 2, 3, 10, 15
#else
#define HZ_P2_WAVES 0, 1, 8, 15, 2, 3, 15, 15
#endif
#endif
constexpr int kP2Wave[8] = {HZ_P2_WAVES};
constexpr int p2_wave_count(int code) {
  int c = 0;
  for (int k = 0; k < 8; k++) c += kP2Wave[k] == code;
  return c;
}
constexpr bool p2_waves_ok() {
  for (int d = 0; d < 6; d++)
    if (p2_wave_count(d) != (d < kP2Draw ? 1 : 0)) return false;
  return p2_wave_count(kWvP1) == 1 && p2_wave_count(kWvPlay) == (kP2Play == 5 ? 1 : 0);
}
#ifndef HZ_P2_HSPLIT
// The rule hashes' split over the seeding stages: the first rows of P2a's,
// P2b's and P2c's ranges (A/B builds).  P1 computes rows [0, first), P2a
// [first, second), P2b [second, third), P2c the rest, each behind its chain's
// last step; a range may be empty.  A hash is ~137 cycles.  By the stamps of
// profiles/r19 P1, P2b and P2c end 7.2-7.5 k cycles before the launch and P2a
// 4.6 k, with the twist (which follows P2c and is left alone) between, so P1,
// P2b and P2c share the rows and P2a takes none (profiles/r22).
#define HZ_P2_HSPLIT 24, 24, 52
#endif
constexpr int kP2HashSplit[3] = {HZ_P2_HSPLIT};
// seeding stage s (0 P1 .. 3 P2c) computes hash rows [kP2HashCut[s], kP2HashCut[s + 1])
constexpr int kP2HashCut[5] = {0, kP2HashSplit[0], kP2HashSplit[1], kP2HashSplit[2], kRulePlies};
static_assert(0 <= kP2HashCut[1] && kP2HashCut[1] <= kP2HashCut[2] && kP2HashCut[2] <= kP2HashCut[3] &&
                  kP2HashCut[3] <= kRulePlies,
              "HZ_P2_HSPLIT: non-decreasing rows within the table");
static_assert(p2_waves_ok(), "HZ_P2_WAVES: every stage outside the seed and play blocks on exactly one wave");
constexpr int kP2MinPlies = 96;   // hz_play max_plies from which pipeline 2 applies (rule games end by ply 80)
#ifdef HZ_DIAG
constexpr int kP2Stamps = 48;  // stamp slots per board in k_play2 (tools/p2_roles.py)
#define P2_PHASE(slot, t0)                                                                                       \
  do {                                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
    if (g_stamps && b < a.n) g_stamps[(size_t)b * kP2Stamps + (slot)] = __builtin_amdgcn_s_memtime() - (t0); \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
  } while (0)
// a value in hand before the next stamp (an opening's arguments, a load's
// result): the stamp then says when it arrived
#define P2_USE_V(x) asm volatile("" ::"v"(x))
#define P2_USE_S(x) asm volatile("" ::"s"(x))
#else
#define P2_PHASE(slot, t0) \
  do {                     \
  } while (0)
#define P2_USE_V(x) \
  do {              \
  } while (0)
#define P2_USE_S(x) \
  do {              \
  } while (0)
#endif
static_assert(4 * kP2WinRows * kWinStride * 4 <= (int)kResetLds, "a window per wave of a draw block");

// What a stage's opening needs of the kernel's arguments is one contiguous
// record per stage, indexed by the wave's stage: a wave fetches it with
// scalar loads issued together and waits once (p2_draw_args, p2_play_args),
// where an argument block indexed field by field (s_tag[4 + stage], then
// x_r[stage - 1], ...) cost a scalar round trip per field, each between two
// vector ones.  launch_play2 fills them.
struct P2DrawArgs {          // draw stage k
  const uint32_t *slot;      // its stream slot, its tag and its cursor table
  const int32_t *stag;
  int32_t *cur;
  P2Draw in, out;            // the previous draw stage's script (k = 0: any valid one, read and discarded) and this one's
  int d0, d1;                // draws [d0, d1)
};
struct P2PlayArgs {          // play stage st
  const int32_t *ep;         // the episode counter the stage's episode follows from: ep_in, the last stage the board's own
  int ep_off;                // episode = ep[b] + ep_off
  int g0;                    // the ply it expects to start at: cut[st - 1], 0 for the first
  int g_end;                 // its last ply's end: min(cut[st], max_plies), max_plies for the last
  int fell_lim;              // slot rows it may draw from (HZ_P2_FELL_LIMIT; at most kP2Twist)
  const int32_t *ptag, *pk;  // the last draw stage's script: tag and draws done (written st + 1 calls before)
  const uint64_t *q;         // [4][nrow] the script: the draw stage's (st = 0), else what the previous play stage left of it
  const uint32_t *h;         // [kRulePlies][nrow] the slot's rule hashes (the episode's whenever ptag names it)
  uint32_t *slot;            // the stream slot and its cursor table
  const int32_t *cur;
  P2Mid in, out;             // the previous play stage's state (st = 0: any valid one, read and discarded) and this one's
};
struct P2Args {
  uint64_t *st;
  uint32_t *mt;
  int32_t *pos, *ply, *episode;
  uint64_t *seed;
  int n, max_plies;
  uint64_t seed_base;
  long nrow;
  int32_t *games_done, *steps_done, *mt_src;
  int32_t *win_tag;           // [nrow] PlyWin's tags: the last play stage sets its board's to none
  const int32_t *ep_in;
  int32_t *ep_out;
  P2DrawArgs dr[kP2Draw];
  P2PlayArgs pp[kP2Play];
  uint32_t *s_mt[kP2SDraw];   // the stream slots of the pass-2 stages this call ([0], P1: none)
  int32_t *s_tag[kP2SDraw];   // [nrow] episode * 8 + 3 P2a / 4 P2b / 5 seeded, rows 0-223 twisted
  // what wave k of a seed block reads before its barrier, k = 0 P2a, 1 P2b, 2 P2c (and the twist)
  const int32_t *seed_tag[3]; // [nrow] the tag it decides by: P1's (episode * 8 + 2), s_tag[2], s_tag[3]
  const uint32_t *seed_h[3];  // the hand-off: [nrow] P1 -> P2a: pass 1's row-1 word after its 624th step; [4][nrow]
                              // P2a -> P2b and P2b -> P2c: pass 2's last value, pass 1's row-1 word, row 2's final
                              // word, pass 1's word of the stage's last row
  int s_idx_last;             // the last play stage's slot index (materialize: mt_src = 2 + index)
  uint32_t *p1h_w;            // [nrow] P1's hand-off as written this call, and its tag
  int32_t *p1t_w;
  uint32_t *p2h_w;            // [4][nrow] P2a's
  uint32_t *p3h_w;            // [4][nrow] P2b's
  uint32_t *s_h[kP2SDraw];        // [kRulePlies][nrow] the rule hashes' entry of seeding stage s (P1's: the one P2a uses next call)
  int32_t *err;                   // the env's wait-error word
  int spin;                       // spin bound of the twist wave's waits
};

// PlayDraw for the prepared stages: the pile script in registers, then (a
// script shorter than the game needs) the episode's stream slot in HBM: its
// next-generation rows below fell_lim (at most kP2Twist, all a slot
// holds).  A game that would draw past them is lost(): the stage voids its
// hand-off and the last play stage plays the board's game from scratch.
struct PlayDraw2 : PileScript {
  bool fell;
  MTR gm;                  // valid once fell
  const int32_t *cur_nd;   // the slot's cursor after the last scripted draw (read when the script runs out)
  __device__ __forceinline__ bool pair_pops() const { return d + 2 <= nd; }
  __device__ __forceinline__ bool lost() const { return fell && gm.over(); }
  __device__ __forceinline__ uint32_t draw_one(uint64_t misc) {
    if (d < nd) return pop();
    if (!fell) {
      gm = MTR(gm.w, gm.stride, *cur_nd, gm.lim);
      fell = true;
    }
    uint32_t p9;
    return draw_pile(misc, gm, p9) ? p9 : 0x1FFu;
  }
  __device__ __forceinline__ uint32_t operator()(uint64_t misc) { return take(misc, true); }
  __device__ __forceinline__ uint32_t take(uint64_t misc, bool want) {
    if (__all(!want || d < nd)) return pop_if(want);
    return want ? draw_one(misc) : 0x1FFu;
  }
};

// the rule policy's plies [g, g_end) of one board (k_rollout's ply loop, no
// reset, no recording): turn pairs while the wave allows, single plies
// otherwise; hashes from a pipeline slot when `hs` (row stride nr) holds the
// episode's, else computed.  h0 (if not null): the slot's rows [h0_g, h0_g + 8)
// of this board, h0_g wave-uniform, loaded by the caller with its opening;
// they serve as the first pair read ahead when every lane has the slot's
// hashes.  Returns the plies played.
template <class Draw>
__device__ __forceinline__ int p2_plies(State &s, Draw &draw, int g, int g_end, uint64_t rkey, const uint32_t *hs,
                                        size_t nr, const uint32_t *h0 = nullptr, int h0_g = -1) {
  const int g0 = g;
  auto hash = [&](int ply) -> uint32_t { return hs && ply < kRulePlies ? hs[(size_t)ply * nr] : rule_h32(rkey, ply); };
  // the next turn pair's hashes, read one pair ahead (a slot's are in HBM).
  // Wave-uniform choices: a per-lane select would evaluate both sides, i.e.
  // compute all eight hashes and issue their loads every pair.
  const bool all_hs = __all(hs != nullptr);
  uint32_t hn[8];
  int hn_g = -1;  // (wave-uniform)
  if (h0 && all_hs) {
#pragma unroll
    for (int j = 0; j < 8; j++) hn[j] = h0[j];
    hn_g = h0_g;
  }
  while (g < g_end) {
    if (phase_of(s.misc) == PH_OVER) break;
    if (__all(g + 8 <= g_end && turn_pair_safe(s))) {
      uint32_t h[8];
      if (__all(hn_g == g)) {
#pragma unroll
        for (int j = 0; j < 8; j++) h[j] = hn[j];
      } else if (all_hs && __all(g + 8 <= kRulePlies)) {
#pragma unroll
        for (int j = 0; j < 8; j++) h[j] = hs[(size_t)(g + j) * nr];
      } else {
#pragma unroll
        for (int j = 0; j < 8; j++) h[j] = hash(g + j);
      }
      if (all_hs && __all(g + 16 <= g_end && g + 16 <= kRulePlies)) {
#pragma unroll
        for (int j = 0; j < 8; j++) hn[j] = hs[(size_t)(g + 8 + j) * nr];
        hn_g = __builtin_amdgcn_readfirstlane(g + 8);
      }
      g += play_pair(s, draw, h);
      continue;
    }
    const int a = rule_action(s, hash(g));
    if (a < 0) break;  // stuck board (unreachable from HarmoniesGameState())
    step_trusted<true>(s, a, draw);
    g++;
  }
  return g - g0;
}

__device__ __forceinline__ int p2_wait(int *flag, int need, int limit, int32_t *err) {
  int v = __hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
  // every publisher reaches kMT + 1 (or kMT rows); the bound only guards
  // against a hang should that ever change, and giving up is reported (the
  // caller goes on with rows that may not be final: the host raises)
  for (int spin = 0; v < need && spin < limit; spin++) {
    __builtin_amdgcn_s_sleep(1);
    v = __hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  if (v < need) {
    wait_failed(err, kWaitErrP2Twist);
    v = kMT + 1;  // no further waits this launch
  }
  return v;
}
__device__ __forceinline__ void p2_publish(int *flag, int v) {
  asm volatile("" ::: "memory");
  __hip_atomic_store(flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// the slot's columns of boards [b0, b0 + 64) as a buffer (rows of nr words)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t p2_slot_rsrc(uint32_t *slot, int b0, size_t nr) {
  const uint64_t base = (uint64_t)(slot + b0);
  uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)base), hi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
  const int bytes = __builtin_amdgcn_readfirstlane((int)((size_t)kMT * nr * 4 - (size_t)b0 * 4));
  return __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)hi << 32) | lo), 0, bytes, 0x00020000);
}
#ifndef HZ_P2_LDNT
#define HZ_P2_LDNT 0  // 1: the stages' 16-B slot reads (staging, windows, the twist's rows) non-temporal (A/B builds)
#endif
__device__ __forceinline__ uint4 p2_ld4(const uint32_t *p) {
  if constexpr (HZ_P2_LDNT) {
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const v4u v = __builtin_nontemporal_load((const v4u *)p);
    return make_uint4(v[0], v[1], v[2], v[3]);
  }
  return *reinterpret_cast<const uint4 *>(p);
}
// An opening's load of a lane's element of a wave-uniform array: `off` is the
// lane's byte offset (32 bits), so the address is the array's scalar
// registers plus one vector register shared by the batch's loads, with no
// vector address arithmetic (and none of its waits) between them.
// (The arrays are in global memory, and the load says so: behind p2_row's
// statement the compiler no longer knows, and a flat load's wait is for every
// load that is out.)
template <class T>
__device__ __forceinline__ T p2_at(const T *base, uint32_t off) {
  typedef __attribute__((address_space(1))) const char GlobalByte;
  typedef __attribute__((address_space(1))) const T GlobalT;
  return *(GlobalT *)((GlobalByte *)base + off);
}
// a row of such an array, its address kept in scalar registers (the compiler
// otherwise adds the lane's offset first and the rows to that, in vector
// registers, between the loads)
template <class T>
__device__ __forceinline__ const T *p2_row(const T *base, size_t row_words) {
  const T *p = base + row_words;
  asm volatile("" : "+s"(p));
  return p;
}
// The order of an opening, for the compiler: no load crosses a fence, and
// p2_fence_use(x) is the first use of a loaded x, so whatever depends on x
// comes after the loads issued before it.
__device__ __forceinline__ void p2_fence() { asm volatile("" ::: "memory"); }
__device__ __forceinline__ void p2_fence_use(int &x) { asm volatile("" : "+v"(x)::"memory"); }
// a store read by another stage in a later call only: write-through (sc1)
// like the slot stores (HZ_P2_AUX), so the kernel's end has no dirty lines
// of it to write back
template <class T>
__device__ __forceinline__ void p2_st(T *p, T v) {
  if constexpr (HZ_P2_AUX == 16 && HZ_P2_ST_WT) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}
// (the stream slots' stores: written by one stage, read by another in the
// next call, never by this one: HZ_P2_AUX write-through (sc1) leaves no
// dirty lines in the XCD's L2 for the end of the kernel to write back)
// One step of init_by_array's pass 1 at row i: q is row i - 1's pass-1 word,
// t kInitGen's word of row i; odd rows take key word kA, even ones kB.
__device__ __forceinline__ uint32_t p1_step(uint32_t t, uint32_t q, bool odd, uint32_t kA, uint32_t kB) {
  return (t ^ ((q ^ (q >> 30)) * 1664525U)) + (odd ? kA : kB);
}
// pass 1's row-1 word (its first step, from init_genrand's mt[0])
__device__ __forceinline__ uint32_t p1_row1(uint32_t kA, uint32_t kB) {
  return p1_step(kInitGen.v[1], 19650218u, true, kA, kB);
}
__device__ __forceinline__ void p2_keys(uint64_t seed, uint32_t &kA, uint32_t &kB) {
  const uint32_t key0 = (uint32_t)seed, key1 = (uint32_t)(seed >> 32);
  kA = key0;
  kB = key1 ? key1 + 1u : key0;
}

// Seeding stage S's rows of the episode's rule hashes (kP2HashCut), from the
// seed the stage holds, into the entry that goes with its slot.  Called
// behind the stage's chain (its last step and last progress publish, so no
// wave waits for it) and before the stage stores its tag: a slot tagged
// seeded then has all 80 rows.  The fence keeps the compiler from spreading
// the multiplies into the chain's last steps.  Plain stores (p2_st): written
// through (sc1) like the slot stores they measured 0.9 % slower (profiles/r22).
template <int S>
__device__ __forceinline__ void p2_hash_rows(const P2Args &a, int b, uint64_t seed) {
  constexpr int J0 = kP2HashCut[S], J1 = kP2HashCut[S + 1];
  if constexpr (J0 < J1) {
    __builtin_amdgcn_sched_barrier(0);
    const size_t nr = (size_t)a.nrow;
    const uint64_t rk = rule_key(seed);
    uint32_t *h = a.s_h[S] + (size_t)J0 * nr + b;
#pragma unroll 1
    for (int j = J0; j < J1; j++, h += nr) p2_st(h, rule_h32(rk, j));
    __builtin_amdgcn_sched_barrier(0);
  }
}

// P1: all of init_by_array's pass 1 in registers (624 steps of four
// dependent VALU operations).  No stream slot and no LDS: what leaves is row
// 1's word after the 624th step (the only pass-1 word pass 2 cannot recompute
// from a neighbour: it closes the ring) and the episode tag.
// The wave is alone on its SIMD, so every instruction it issues, scalar ones
// included, costs an issue slot: the loop is kept to the chain plus one
// scalar load and one wait per eight steps.  The table words come a group of
// eight ahead, in two register sets that alternate (a trip is sixteen steps),
// so no set is copied; the padded table needs no clamp, so a group is one
// s_load_dwordx8 from the loop's one table address.
// The loads and their waits are written out: the compiler moves a plain
// table read to wherever it likes (both groups' loads to the top of the trip,
// or each next to its first use, where every group then waits a scalar-cache
// round trip: 12 us for the stage instead of 8) and copies the words between
// the sets.  Scalar loads return out of order, so a wait is for all that are
// out: a group's wait comes before the next group's load is issued, behind
// the eight steps that ran meanwhile.
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
// rows [1 + off / 4 + Imm / 4, + 8) of the table (tab: row 1's address)
template <int Imm>
__device__ __forceinline__ u32x8 p1_load8(const uint32_t *tab, uint32_t off) {
  u32x8 t;
  asm volatile("s_load_dwordx8 %0, %1, %2 offset:%3" : "=&s"(t) : "s"(tab), "s"(off), "n"(Imm));
  return t;
}
__device__ __forceinline__ void p1_arrived(u32x8 &t) { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(t)); }
__device__ __forceinline__ uint32_t p1_steps8(const u32x8 &t, uint32_t prev, uint32_t kA, uint32_t kB) {
#pragma unroll
  for (int u = 0; u < 8; u++) prev = p1_step(t[u], prev, !(u & 1), kA, kB);  // (groups start at odd rows)
  return prev;
}
__device__ __forceinline__ void p2_p1(const P2Args &a, int b) {
  const int e = a.ep_in[b] + kP2Last;
  const uint64_t seed = episode_seed(a.seed_base, b, e);
  uint32_t kA, kB;
  p2_keys(seed, kA, kB);
  uint32_t prev = 19650218u;
  const uint32_t *tab = kInitGen.v + 1;
  static_assert(38 * 16 + 1 == 609 && 617 + 8 <= kMT + kInitGenPad, "the last group's read (rows 617-624) within the table's padding");
  u32x8 ta = p1_load8<0>(tab, 0), tb;
  p1_arrived(ta);
#pragma unroll 1
  for (uint32_t off = 0; off < 38 * 64; off += 64) {  // steps 1..608, sixteen per trip
    tb = p1_load8<32>(tab, off);
    __builtin_amdgcn_sched_barrier(0);
    prev = p1_steps8(ta, prev, kA, kB);
    __builtin_amdgcn_sched_barrier(0);
    p1_arrived(tb);
    ta = p1_load8<64>(tab, off);
    __builtin_amdgcn_sched_barrier(0);
    prev = p1_steps8(tb, prev, kA, kB);
    __builtin_amdgcn_sched_barrier(0);
    p1_arrived(ta);
  }
  tb = p1_load8<0>(tab, (617 - 1) * 4);  // (its eighth word is padding)
  prev = p1_steps8(ta, prev, kA, kB);  // steps 609..616
  p1_arrived(tb);
#pragma unroll
  for (int u = 0; u < 7; u++) prev = p1_step(tb[u], prev, !(u & 1), kA, kB);  // steps 617..623
  // mt[0] = mt[623]; the 624th step at i = 1 (key j = 623 % keylen -> kB)
  a.p1h_w[b] = p1_step(p1_row1(kA, kB), prev, false, kA, kB);
  p2_hash_rows<0>(a, b, seed);  // (before the tag: P2a, which tests it, vouches for these rows)
  a.p1t_w[b] = e * 8 + 2;
}

// Pass 2 in three stages, P2a (steps 2-208), P2b (209-432) and P2c
// (433-623 and the last step at i = 1), in one seed block (three different
// episodes).  Every step reads the row's pass-1 word.  The stages once read
// them from the stream slot (staged into LDS first: an HBM round trip per
// step is far too slow); now each recomputes pass 1 over its own rows, a
// group of eight ahead of its pass-2 chain, so the two recurrences are
// independent instruction streams and interleave.  A word that a later
// stage reads goes to the slot with a buffer store (the row offset a scalar:
// no address arithmetic in the chain); the others are not stored at all
// (HZ_P2_LEAN, kP2None).  The chain is cut into thirds rather than made
// cheaper per step.
#ifndef HZ_P2_BEND
// P2b's end (A/B builds: 225 + 8 k).  The twist follows P2c's progress and
// ends ~1.5 us after it (its last stores' write-through), so P2c gets the
// fewest rows: the rows r + 397 below this row the twist holds in registers
// from the start (kTwHbm, P2b's of the call before, from HBM), the rest it
// reads from P2c's LDS rows as they appear.
#define HZ_P2_BEND 433
#endif
#ifndef HZ_P2_AEND
#define HZ_P2_AEND 209  // P2a's end (A/B builds: 209 - 8 k)
#endif
#ifndef HZ_P2_LEAN
// 1: pass 2 stores only the rows a later stage reads.  The old generation's
// rows 225-396 (P2b) and P2c's rows in HBM had two readers, materialize and a
// play stage twisting past row kAheadTwist; the first now rebuilds a stream
// from its seed and the second is gone (MTR), so 0 is only the A/B build that
// still issues the stores.
#define HZ_P2_LEAN 1
#endif
#ifndef HZ_P2_TWIST
// The next-generation rows a slot gets, [0, kP2Twist): the twist makes no
// more, P2a and P2b store no twist part past them, and P2c keeps in LDS only
// the far rows below kP2Twist + 397.  The draw stages' windows end at row 152
// with the default cuts, and of 26,214,400 rule games (boards 0-4095, episodes
// 0-6399: tools/p2_fell_count.py) the longest read 134 words; a game that
// would read past row kP2Twist is played again from scratch (PlayDraw2), so
// the value decides time, never results.  A multiple of 8, at most
// kAheadTwist (which it was).
#define HZ_P2_TWIST 160
#endif
constexpr int kP2Twist = HZ_P2_TWIST;
constexpr int kP2Ahead = 0 | (kP2Twist << 16);  // a slot's cursor before its first draw
static_assert(kP2Twist % 8 == 0 && kP2Twist >= 64 && kP2Twist <= kAheadTwist, "the slot's twisted rows");
constexpr int kP2PartEnd = HZ_P2_LEAN ? kP2Twist + 1 : kAheadTwist + 1;  // steps [3, kP2PartEnd) store the previous row's twist part
constexpr int p2_up8(int from, int x) { return x <= from ? from : from + 8 * ((x - from + 7) / 8); }
constexpr int p2_min(int a, int b) { return a < b ? a : b; }
constexpr int kP2aEnd = HZ_P2_AEND, kP2bEnd = HZ_P2_BEND;
static_assert(kP2bEnd > 399 && kP2bEnd + 64 < kMT && (kP2bEnd - kAheadTwist - 1) % 8 == 0, "P2b's final steps in groups of eight; rows 397, 398 P2b's");
static_assert(kP2aEnd > 11 && kP2aEnd <= kAheadTwist - 7 && (kAheadTwist + 1 - kP2aEnd) % 8 == 0, "P2b's part steps in groups of eight");
// P2b's final steps [kAheadTwist + 1, kP2bDrop) store nothing: whole groups
// below row 397, the first row the twist reads as a far row (the group that
// holds row 397 stores its rows from 393 on)
constexpr int kP2bDrop = HZ_P2_LEAN ? kAheadTwist + 1 + 8 * ((397 - kAheadTwist - 1) / 8) : kAheadTwist + 1;
// pass 1 a group ahead of pass 2, at row g
struct P2Ahead {
  uint32_t cur[8];  // pass 1's words of rows [g, g + 8)
  uint32_t iv[8];   // kInitGen's words of rows [g + 8, g + 16)
  uint32_t last;    // pass 1's word of the last row pass 2 has consumed (the next stage starts from it)
};
// The table's address as a pass-2 stage holds it: in one scalar register
// pair from the stage's start, its groups' loads at immediate offsets (the
// compiler, knowing the address, makes it again from the program counter for
// every group: three scalar instructions each).
typedef __attribute__((address_space(4))) const uint32_t ConstWord;
__device__ __forceinline__ ConstWord *p2_table() {
  ConstWord *t = (ConstWord *)kInitGen.v;
  asm volatile("" : "+s"(t));
  return t;
}
// q: pass 1's word of row G - 1
template <int G>
__device__ __forceinline__ void p2_ahead_init(ConstWord *tab, P2Ahead &h, uint32_t q, uint32_t kA, uint32_t kB) {
#pragma unroll
  for (int u = 0; u < 8; u++) {
    q = p1_step(tab[G + u], q, (G + u) & 1, kA, kB);
    h.cur[u] = q;
  }
#pragma unroll
  for (int u = 0; u < 8; u++) h.iv[u] = tab[G + 8 + u];
  h.last = q;
}
// twist_word(cur, next, far) = far ^ twist_part(cur, next): the part of row
// r's next-generation word that rows r and r + 1 decide.  Four operations:
// the select of cur's top bit into next (v_bfi_b32), the shift, next's low
// bit spread (v_bfe_i32), and "and, xor" in one v_bitop3_b32.  (The select
// is written out: from every source form of it the compiler makes v_and_b32
// and v_and_or_b32.)
__device__ __forceinline__ uint32_t twist_part(uint32_t cur, uint32_t next) {
  uint32_t y;  // (cur & 0x80000000) | (next & 0x7fffffff)
  asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(y) : "s"(0x7fffffffU), "v"(next), "v"(cur));
  return (y >> 1) ^ ((next & 1U) ? 0x9908b0dfU : 0U);
}
// What a pass-2 step stores: its final word to its row (kP2Final), the same
// and to the row in LDS (kP2Keep), the previous row's twist part (kP2Part:
// rows 2 .. kP2Twist - 1, which only the twist reads), the row in LDS only (kP2KeepLds,
// P2c: the twist reads its rows there), or nothing (kP2None: rows no stage
// reads; the loop then has no store, no row offset and no use of vo[])
enum { kP2Final = 0, kP2Keep = 1, kP2Part = 2, kP2KeepLds = 3, kP2None = 4 };
constexpr bool p2_mode_lds(int m) { return m == kP2Keep || m == kP2KeepLds; }
constexpr bool p2_mode_hbm(int m) { return m == kP2Final || m == kP2Keep || m == kP2Part; }
// A stage's store addresses, made once: the slot's buffer, the byte offsets
// of the lane's column in eight consecutive rows (a store's voffset; the
// group's first row is its scalar offset: one scalar instruction per group of
// eight stores, none per store), and the lane's LDS byte address.
typedef __attribute__((address_space(3))) uint32_t LdsWord;
struct P2Out {
  __amdgpu_buffer_rsrc_t rs;
  int row_bytes;
  int vo[8];
  uint32_t lds;
  __device__ __forceinline__ P2Out(__amdgpu_buffer_rsrc_t r, int rb, int lane) : rs(r), row_bytes(rb) {
#pragma unroll
    for (int u = 0; u < 8; u++) {
      vo[u] = lane * 4 + u * rb;
      asm volatile("" : "+v"(vo[u]));  // (kept: not made again at every store)
    }
    lds = (uint32_t)(uintptr_t)(LdsWord *)(hz_lds + lane);
  }
  // word v to column `lane` of row g + u (g wave-uniform, soff = g * row_bytes)
  __device__ __forceinline__ void put(uint32_t v, int soff, int u) const {
    __builtin_amdgcn_raw_buffer_store_b32(v, rs, vo[u], soff, HZ_P2_AUX);
  }
};
// steps [G0, G1) of pass 2 (G1 - G0 a multiple of 8; h at row G0 on entry, at
// G1 on return), while pass 1 runs over the next group's rows (past the
// stage's last row its words are unused); stores to the slot as Mode says,
// with kP2Keep publishing progress every 8 steps.  kP2Keep's LDS rows: one
// address per group, the group's rows at immediate offsets.
template <int G0, int G1, int Mode>
__device__ __forceinline__ void p2_span(ConstWord *tab, const P2Out &o, uint32_t &prev, P2Ahead &h, uint32_t kA, uint32_t kB, int *prog) {
  constexpr bool KeepLds = p2_mode_lds(Mode), Hbm = p2_mode_hbm(Mode);
  static_assert((G1 - G0) % 8 == 0, "groups of eight");
  static_assert(G1 + 15 < kMT + kInitGenPad, "the table's read-ahead within its padding");
  constexpr int S = kLdsStride;
  uint32_t lg = o.lds + G0 * S * 4;
#pragma unroll 2
  for (int g = G0; g < G1; g += 8) {
    uint32_t ivn[8], nx[8];
#pragma unroll
    for (int u = 0; u < 8; u++) ivn[u] = tab[g + 16 + u];
    const uint32_t kneg = __builtin_amdgcn_readfirstlane(0u - (uint32_t)g);
    [[maybe_unused]] int soff = 0;
    if constexpr (Hbm) soff = __builtin_amdgcn_readfirstlane((Mode == kP2Part ? g - 1 : g) * o.row_bytes);
    if (KeepLds) asm volatile("" : "+v"(lg));  // (one register for the group, not an address per row)
    uint32_t q = h.cur[7];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      // (cur ^ p) - (g + u) as one v_xad_u32 with the offset in an SGPR
      const uint32_t p = (prev ^ (prev >> 30)) * 1566083941U;
      uint32_t v;
      asm("v_xad_u32 %0, %1, %2, %3" : "=v"(v) : "v"(p), "v"(h.cur[u]), "s"(kneg - (uint32_t)u));
      if constexpr (Hbm) o.put(Mode == kP2Part ? twist_part(prev, v) : v, soff, u);
      if (KeepLds) *(LdsWord *)(uintptr_t)(lg + u * S * 4) = v;
      prev = v;
      // pass 1, row g + 8 + u (the parity of G0 + u: g - G0 is a multiple of 8)
      q = p1_step(h.iv[u], q, (G0 + u) & 1, kA, kB);
      nx[u] = q;
    }
    if (KeepLds) {
      p2_publish(prog, g + 8);  // rows [G0, g + 8) final in LDS
      lg += 8 * S * 4;
    }
    h.last = h.cur[7];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      h.cur[u] = nx[u];
      h.iv[u] = ivn[u];
    }
  }
}
// the last steps [G, G1) one by one (fewer than eight: h holds their pass-1 words)
template <int G, int G1, int Mode>
__device__ __forceinline__ void p2_tail(const P2Out &o, int lane, uint32_t &prev, P2Ahead &h) {
  static_assert(G1 - G >= 1 && G1 - G <= 8, "within the group ahead");
  [[maybe_unused]] const int soff = __builtin_amdgcn_readfirstlane((Mode == kP2Part ? G - 1 : G) * o.row_bytes);
#pragma unroll
  for (int i = G; i < G1; i++) {
    const uint32_t v = (h.cur[i - G] ^ ((prev ^ (prev >> 30)) * 1566083941U)) - (uint32_t)i;
    if constexpr (p2_mode_hbm(Mode)) o.put(Mode == kP2Part ? twist_part(prev, v) : v, soff, i - G);
    if (p2_mode_lds(Mode)) hz_lds[i * kLdsStride + lane] = v;
    prev = v;
  }
  h.last = h.cur[G1 - G - 1];
}

// P2a (seed blocks, wave 0): the seed blocks' P2a episode, whose pass 1
// completed in the previous call; P2b (wave 1) the next older; P2c (wave 2,
// with wave 3's twist) the one before.  Each hands (prev, pass 1's row-1
// word, row 2's final word, pass 1's word of its last row) to the next.
// Rows 2 .. kP2Twist - 1 of the slot are read
// only by the twist, which needs from each row r only its twist part
// (rows r and r + 1's words): P2a and P2b store that instead of the final
// word (one step late, when row r + 1 is known), so the twist is one xor
// per word with the far row.  (e, ok, hw: the board's episode, whether the
// stage's input is this episode's, and the hand-off's words, read by every
// wave of the block before its barrier, so before P2c rewrites its tag.)
template <int K>  // 0 P2a, 1 P2b, 2 P2c
__device__ __forceinline__ void p2_third(const P2Args &a, int b0, int lane, int e, bool ok, const uint32_t (&hw)[4],
                                         int *s_prog) {
  const int b = b0 + lane;
  const bool act = b < a.n;
  const size_t nr = (size_t)a.nrow;
  // (P2a's slot is a fresh one: whatever tag an older episode left on it goes)
  if (K == 0 && act && !ok) a.s_tag[1][b] = -1;
  if (!__any(ok)) {
    if (K == 2) p2_publish(s_prog, kMT + 1);  // (the twist wave's waits end: nothing to twist)
    return;
  }
  uint32_t *slot = a.s_mt[1 + K];
  const uint64_t seed = episode_seed(a.seed_base, b, e);
  uint32_t kA, kB;
  p2_keys(seed, kA, kB);
  uint32_t prev, first1, row2, q;
  if (K == 0) {
    first1 = act ? hw[0] : 0u;
    prev = first1;
    q = p1_row1(kA, kB);
  } else {
    prev = act ? hw[0] : 0u;
    first1 = act ? hw[1] : 0u;
    row2 = act ? hw[2] : 0u;
    q = act ? hw[3] : 0u;
  }
  const __amdgpu_buffer_rsrc_t rs = p2_slot_rsrc(slot, b0, nr);
  const int row_bytes = __builtin_amdgcn_readfirstlane((int)(nr * 4));
  const P2Out o(rs, row_bytes, lane);
  ConstWord *tab = p2_table();
  P2Ahead h;
  if constexpr (K == 0) {  // step 2: row 2's final word, handed on (row 1's part needs row 1, P2c's last step)
    q = p1_step(kInitGen.v[2], q, false, kA, kB);
    row2 = (q ^ ((prev ^ (prev >> 30)) * 1566083941U)) - 2U;
    prev = row2;
    p2_ahead_init<3>(tab, h, q, kA, kB);
    constexpr int G = 3 + 8 * ((kP2aEnd - 3) / 8), Gp = p2_min(G, p2_up8(3, kP2PartEnd));
    p2_span<3, Gp, kP2Part>(tab, o, prev, h, kA, kB, s_prog);  // parts of rows 2 .. (whole groups: a few past kP2Twist)
    p2_span<Gp, G, kP2None>(tab, o, prev, h, kA, kB, s_prog);
    p2_tail<G, kP2aEnd, (G < kP2PartEnd ? kP2Part : kP2None)>(o, lane, prev, h);
  } else if constexpr (K == 1) {
    p2_ahead_init<kP2aEnd>(tab, h, q, kA, kB);
    constexpr int E1 = kAheadTwist + 1, Pb = p2_min(E1, p2_up8(kP2aEnd, kP2PartEnd));
    p2_span<kP2aEnd, Pb, kP2Part>(tab, o, prev, h, kA, kB, s_prog);  // the parts P2a left to do, if any
    p2_span<Pb, E1, kP2None>(tab, o, prev, h, kA, kB, s_prog);
    if constexpr (!HZ_P2_LEAN)  // row 224's final word
      __builtin_amdgcn_raw_buffer_store_b32(prev, rs, lane * 4, kAheadTwist * row_bytes, HZ_P2_AUX);
    p2_span<E1, kP2bDrop, kP2None>(tab, o, prev, h, kA, kB, s_prog);
    p2_span<kP2bDrop, kP2bEnd, kP2Final>(tab, o, prev, h, kA, kB, s_prog);
  } else {
    // rows 0 and 1 of the next generation are P2c's own last words: their
    // far rows (397, 398: P2b's) loaded now, used after the chain
    const uint32_t f0 = act ? slot[(size_t)397 * nr + b] : 0u, f1 = act ? slot[(size_t)398 * nr + b] : 0u;
    p2_ahead_init<kP2bEnd>(tab, h, q, kA, kB);
    constexpr int G = kP2bEnd + 8 * ((kMT - kP2bEnd) / 8);
    constexpr int Keep = HZ_P2_LEAN ? kP2KeepLds : kP2Keep;
    // (the twist's far rows end below row kP2Twist + 397: the steps past them are the bare chain)
    constexpr int Kc = HZ_P2_LEAN ? p2_min(G, p2_up8(kP2bEnd, kP2Twist + 397)) : G;
    p2_span<kP2bEnd, Kc, Keep>(tab, o, prev, h, kA, kB, s_prog);
    p2_span<Kc, G, kP2None>(tab, o, prev, h, kA, kB, s_prog);
    p2_tail<G, kMT, (Kc == G ? Keep : kP2None)>(o, lane, prev, h);
    p2_publish(s_prog, kMT);
    const uint32_t row1 = (first1 ^ ((prev ^ (prev >> 30)) * 1566083941U)) - 1U;  // the last step, at i = 1
    // mt[0] = 0x80000000 after init_by_array; row 1's next row is row 2
    __builtin_amdgcn_raw_buffer_store_b32(f0 ^ twist_part(0x80000000u, row1), rs, lane * 4, 0, HZ_P2_AUX);
    __builtin_amdgcn_raw_buffer_store_b32(f1 ^ twist_part(row1, row2), rs, lane * 4, row_bytes, HZ_P2_AUX);
  }
  if (K < 2) {
    if (ok) {
      uint32_t *ho = K == 0 ? a.p2h_w : a.p3h_w;
      ho[b] = prev;
      ho[nr + b] = first1;
      ho[2 * nr + b] = row2;
      ho[3 * nr + b] = h.last;
      p2_hash_rows<1 + K>(a, b, seed);
      a.s_tag[1 + K][b] = e * 8 + 3 + K;
    }
  } else if (ok) {
    p2_hash_rows<3>(a, b, seed);
    a.s_tag[3][b] = e * 8 + 5;  // seeded: the earlier stages' tags named e, so all of e's hash rows are in
  }
}

// The twist (seed blocks, wave 3): rows [0, kP2Twist) of the next
// generation into P2c's slot (the stream at cursor kP2Ahead): row r's new
// word is the far row r + 397 (P2b's below row kP2bEnd, from HBM; P2c's from
// LDS) xor row r's twist part, which P2a and P2b left in the slot (rows
// 2-223).  Lane: four boards, rows grp + 4 i, grp = lane / 16, so iteration
// i needs P2c's rows up to 4 i + 400 (from iteration 9 on: the rows below
// kP2bEnd are in registers) and follows P2c's progress (s_prog),
// two iterations per publish of P2c's; rows 0 and 1 (from row 1, P2c's last
// step, and row 2's final word) are P2c's own.  All its loads precede its
// stores.  (Before the parts, the wave shuffled each row's
// successor in from the next lane group and ran at ~350 cycles per
// iteration, ending ~8 k cycles after P2c: profiles/r04/p2/.)
#ifndef HZ_P2_TWGO
#define HZ_P2_TWGO 64  // rows of P2c the twist waits for before its loads (A/B builds; < 0: none)
#endif
constexpr int kTwGo = HZ_P2_TWGO;
constexpr int kTwIters = kP2Twist / 4;
constexpr int kTwHbm = (kP2bEnd - 397 + 3) / 4;  // iterations whose rows r + 397 are P2b's (HBM)
__device__ __forceinline__ uint4 xor4(const uint4 &a, const uint4 &b) {
  return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w);
}
__device__ __forceinline__ void p2_twist(const P2Args &a, int b0, int lane, bool any, int *s_prog) {
  if (!any) return;
  const size_t nr = (size_t)a.nrow;
  uint32_t *slot = a.s_mt[3];
  const int grp = lane >> 4, c4 = (lane & 15) * 4;
  uint32_t *col = slot + b0 + c4;
  auto row = [&](int r) { return p2_ld4(col + (size_t)r * nr); };
  const __amdgpu_buffer_rsrc_t rs = p2_slot_rsrc(slot, b0, nr);
  const int row_bytes = __builtin_amdgcn_readfirstlane((int)(nr * 4));
  auto store = [&](int r, const uint4 &v) {
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    // (r = grp + 4 i differs across the lane groups: per-lane voffset, no soffset)
    __builtin_amdgcn_raw_buffer_store_b128(v4u{v.x, v.y, v.z, v.w}, rs, c4 * 4 + r * row_bytes, 0, HZ_P2_AUX);
  };
  [[maybe_unused]] const int b = b0 + lane;  // (P2_PHASE's board)
  HZ_DIAG_T0(tz);
  // (the wave has ~16 k cycles of slack: its 4 MB of loads wait until P2c is
  // 64 rows in, out of the launch's opening burst, where every other
  // stage's inputs arrive)
  int have = kTwGo >= 0 ? p2_wait(s_prog, kP2bEnd + kTwGo, a.spin, a.err) : 0;
  P2_PHASE(35, tz);
  uint4 pt[kTwIters], fh[kTwHbm];
#pragma unroll
  for (int i = 0; i < kTwIters; i++) {
    const int r = grp + 4 * i;
    pt[i] = r >= 2 ? row(r) : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < kTwHbm; i++) {
    const int r = grp + 4 * i + 397;
    fh[i] = r < kP2bEnd ? row(r) : make_uint4(0, 0, 0, 0);
  }
  auto far = [&](int i) -> uint4 {
    const int r = grp + 4 * i;
    if (i < kTwHbm && r + 397 < kP2bEnd) return fh[i < kTwHbm ? i : 0];
    const uint32_t *d = hz_lds + (r + 397) * kLdsStride + c4;
    return make_uint4(d[0], d[1], d[2], d[3]);
  };
#pragma unroll
  for (int i = 0; i < kTwIters; i += 2) {
    const int need = 4 * (i + 1) + 3 + 397 + 1;  // the pair's far rows final
    if (need > kP2bEnd && have < need) have = p2_wait(s_prog, need, a.spin, a.err);
    const uint4 f0 = far(i), f1 = far(i + 1);
    if (i > 0 || grp >= 2) store(grp + 4 * i, xor4(f0, pt[i]));
    store(grp + 4 * (i + 1), xor4(f1, pt[i + 1]));
    if (i == 0) P2_PHASE(36, tz);
  }
  P2_PHASE(37, tz);
  // (the old generation's rows are not in the slot: k_mt_materialize2 rebuilds a board's stream)
}

// seed blocks: waves 0-2 P2a, P2b, P2c; wave 3 the twist of P2c's episode
__device__ __forceinline__ void p2_seed(const P2Args &a, int blk) {
  __shared__ int s_prog;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b0 = blk * kBlock, b = b0 + lane;
  const bool act = b < a.n;
  if (tid == 0) s_prog = 0;
  // each stage's episode, decision and hand-off (P2c's episode and decision
  // for the twist wave), read before the barrier, so before any wave
  // rewrites a tag.  One round trip: the wave's stage is a scalar, so its
  // tag's and its hand-off's addresses come from the arguments with scalar
  // loads, and the episode counter, the tag and the hand-off's four words
  // are loaded together, from a clamped board index (a lane past n reads
  // board n - 1's, valid memory, and discards them), and compared after.
  // (P2a's hand-off is one word: its four loads are of that word.)
  const int wv = __builtin_amdgcn_readfirstlane(w);
  const int k = wv < 3 ? wv : 2;
  const int32_t *tagp = a.seed_tag[k];
  const uint32_t *hp = a.seed_h[k];
  const int32_t *ep_in = a.ep_in;
  const int n = a.n;
  const size_t hrow = k == 0 ? 0 : (size_t)a.nrow;
  asm volatile("" ::"s"(tagp), "s"(hp), "s"(ep_in), "s"(n), "s"(hrow));  // (one scalar batch: p2_draw_args)
  __builtin_amdgcn_sched_barrier(0);
  const int bc = min(b, n - 1);
  const int hb = wv < 3 ? bc : b0;  // (the twist wave uses no hand-off: one address for the wave)
  const uint32_t *hrp[4];
#pragma unroll
  for (int i = 0; i < 4; i++) hrp[i] = p2_row(hp, i * hrow);
  p2_fence();
  int ep = p2_at(ep_in, (uint32_t)bc * 4u);
  const int tag = p2_at(tagp, (uint32_t)bc * 4u);
  uint32_t hw[4];
#pragma unroll
  for (int i = 0; i < 4; i++) hw[i] = p2_at(hrp[i], (uint32_t)hb * 4u);
  p2_fence_use(ep);
  const int e = act ? ep + kP2Last - 1 - k : 0;
  const bool ok = act && tag == e * 8 + 2 + k;
  __syncthreads();
  if (w == 0) p2_third<0>(a, b0, lane, e, ok, hw, &s_prog);
  else if (w == 1) p2_third<1>(a, b0, lane, e, ok, hw, &s_prog);
  else if (w == 2) p2_third<2>(a, b0, lane, e, ok, hw, &s_prog);
  else p2_twist(a, b0, lane, __any(ok), &s_prog);
}

// a draw stage: draws [d0, d1) of episode e on its stream slot, from an LDS
// window (at `base`) of kP2Win rows starting at the wave's lowest start
// cursor (the wave's 64 boards, staged here); `in` (stage > 0) holds the
// draws so far, `out` gets them plus these; the cursors go to the slot's
// cursor table
// A stage's part of the arguments, and the common ones its opening needs, in
// scalar registers: the loads are issued together and the empty statement,
// which takes every value, waits for them once (scalar loads return out of
// order: one wait for all that are out).  Left to itself the compiler
// fetches each where it is first used, a scalar round trip between two
// vector ones.
__device__ __forceinline__ P2DrawArgs p2_draw_args(const P2Args &a, int stage, int &n, size_t &nr,
                                                   const int32_t *&ep_in) {
  const P2DrawArgs r = a.dr[stage];
  n = a.n;
  nr = (size_t)a.nrow;
  ep_in = a.ep_in;
  asm volatile("" ::"s"(r.slot), "s"(r.stag), "s"(r.cur), "s"(r.in.tag), "s"(r.in.k), "s"(r.in.q), "s"(r.in.bag),
               "s"(r.in.c), "s"(r.out.tag), "s"(r.out.k), "s"(r.out.q), "s"(r.out.bag), "s"(r.out.c), "s"(r.d0),
               "s"(r.d1), "s"(n), "s"(nr), "s"(ep_in));
  __builtin_amdgcn_sched_barrier(0);
  return r;
}
__device__ __forceinline__ P2PlayArgs p2_play_args(const P2Args &a, int st, int &n, size_t &nr, uint64_t &seed_base) {
  const P2PlayArgs r = a.pp[st];
  n = a.n;
  nr = (size_t)a.nrow;
  seed_base = a.seed_base;
  asm volatile("" ::"s"(r.ep), "s"(r.ep_off), "s"(r.g0), "s"(r.g_end), "s"(r.ptag), "s"(r.pk), "s"(r.q), "s"(r.h),
               "s"(r.slot), "s"(r.cur), "s"(r.in.tag), "s"(r.in.st), "s"(r.in.q), "s"(r.in.i),
               "s"(r.out.tag), "s"(r.out.st), "s"(r.out.q), "s"(r.out.i), "s"(n), "s"(nr), "s"(seed_base),
               "s"(r.fell_lim));
  __builtin_amdgcn_sched_barrier(0);
  return r;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ void p2_draw_stage(const P2Args &a, int b0, int lane, int stage, int base) {
  const int b = b0 + lane;
  HZ_DIAG_T0(t0);
  // The opening is one scalar batch and one vector batch.  Scalar: the
  // stage's record and the three common arguments, loaded together and
  // waited for once (p2_draw_args).  Vector: the episode counter, the slot's
  // tag and the previous stage's hand-off (tag, draws, cursor, bag, script),
  // then the window's 24 loads, all issued before the first wait and in that
  // order, so the small ones are back (vmcnt counts in order) while the
  // window is still in flight; the tags are compared after.  No guard: a
  // lane past n reads board n - 1's words (valid memory in every array,
  // whether sized n or nrow) and discards them; D1, which has no previous
  // stage, reads one board's hand-off of D2's input and discards it.
  int n;
  size_t nr;
  const int32_t *ep_in;
  const P2DrawArgs r = p2_draw_args(a, stage, n, nr, ep_in);
  if (stage == 1) P2_PHASE(33, t0);
  const int d0 = r.d0, d1 = r.d1;
  const bool act = b < n;
  const uint32_t *slot = r.slot;
  int32_t *cur = r.cur + b;
  const P2Draw &in = r.in, &out = r.out;
  int k0 = 0, c0 = kP2Ahead;
  uint64_t bag = initial_bag(), q[kAheadWords] = {0, 0, 0, 0};
  // the window: rows [r0, r0 + kP2Win), 16-B loads (four boards of a row per
  // lane), all in flight, and one 16-B LDS store each
  constexpr int U = kP2Win / 4;
  const int c4 = (lane & 15) * 4;
  uint4 v[U];
  auto win_load = [&](int r0) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int r = r0 + 4 * u + (lane >> 4);
      v[u] = p2_ld4(slot + (size_t)r * nr + b0 + c4);
    }
  };
  auto win_store = [&]() {
#pragma unroll
    for (int u = 0; u < U; u++)
      *reinterpret_cast<uint4 *>(hz_lds + base + (4 * u + (lane >> 4)) * kWinStride + c4) = v[u];
  };
  // The window's first row is the stage's first draw's (wave-uniform, from
  // the kernel's arguments): every draw of a script is from a bag of more
  // than 21 tiles, so it consumes at least three words, and a board that has
  // made d0 draws stands at row 3 d0 or later.  So the window's loads go out
  // behind the tags' and the hand-off's, in the same round trip (rows of
  // another episode are never read: !ok).  HZ_P2_STATIC_WIN=0 (A/B builds):
  // from the wave's lowest cursor, known only after the hand-off arrived.
  const int rs = kP2StaticWin ? __builtin_amdgcn_readfirstlane((3 * d0) & ~3) : 0;
  const int bc = min(b, n - 1), bi = stage > 0 ? bc : b0;
  const uint32_t o4 = (uint32_t)bc * 4u, i4 = (uint32_t)bi * 4u, i8 = i4 * 2u;
  const uint64_t *iqr[kAheadWords];
#pragma unroll
  for (int i = 0; i < kAheadWords; i++) iqr[i] = p2_row(in.q, (size_t)i * nr);
  p2_fence();
  int ep = p2_at(ep_in, o4);
  const int stag = p2_at(r.stag, o4);
  const int itag = p2_at(in.tag, i4), ik = p2_at(in.k, i4), ic = p2_at(in.c, i4);
  const uint64_t ibag = p2_at(in.bag, i8);
  uint64_t iq[kAheadWords];
#pragma unroll
  for (int i = 0; i < kAheadWords; i++) iq[i] = p2_at(iqr[i], i8);
  p2_fence();
  if (kP2StaticWin || stage == 0) win_load(rs);
  p2_fence_use(ep);
  if (stage == 1) {
    P2_USE_V(ep);
    P2_PHASE(34, t0);
  }
  const int e = act ? ep + kP2Last - kP2SDraw - stage : 0;
  bool ok = act && stag == e * 8 + 5;
  if (stage > 0) {
    k0 = ik;
    c0 = ic;
    bag = ibag;
#pragma unroll
    for (int i = 0; i < kAheadWords; i++) q[i] = iq[i];
    ok = ok && itag == e * 8 + stage;
  }
  if (stage == 1) {
    P2_USE_V((int)ok);
    P2_PHASE(26, t0);
  }
  bool draws = ok && k0 >= d0 && d0 < d1;
  int r0 = rs;
  if constexpr (kP2StaticWin) {
    draws = draws && (c0 & 0xFFFF) >= r0;  // (always: see above; a board below the window would read outside it)
    win_store();
  } else {
    r0 = wave_min_i(draws ? (c0 & 0xFFFF) : kP2Twist) & ~3;
    if (r0 < kP2Twist) {
      if (stage > 0) win_load(r0);
      win_store();
    }
  }
  P2_PHASE(stage < 5 ? 28 + stage : 43, t0);  // window staged (slot 33 is D2's arguments)
  if (!act) return;
  if (!ok) {
    out.tag[b] = -1;
    return;
  }
  if (stage == 0) cur[0] = kP2Ahead;
  int k = k0, cc = c0;
  if (draws) {  // every earlier draw is done: continue in the window
    const int lim = min(r0 + kP2Win, kP2Twist);
    StreamDraw<WinMT> d{WinMT(base - r0 * kWinStride + lane, c0, lim)};
#pragma unroll 1
    for (int i = d0; i < d1; i++) {
      if (d.m.pos >= lim) break;
      const uint32_t p9 = d(bag);
      // a draw that consumed words past the window is discarded: the next
      // stage (or a play stage, from the stream slot) redoes it from the
      // last cursor kept
      if (d.m.pos > lim) break;
      apply_pile_fast(bag, p9);
      const int bit = 9 * i, wd = bit >> 6, off = bit & 63;
      const uint64_t lo9 = (uint64_t)p9 << off, hi9 = off > 55 ? (uint64_t)p9 >> (64 - off) : 0ull;
      q[0] |= wd == 0 ? lo9 : 0ull;
      q[1] |= wd == 1 ? lo9 : wd == 0 ? hi9 : 0ull;
      q[2] |= wd == 2 ? lo9 : wd == 1 ? hi9 : 0ull;
      q[3] |= wd == 3 ? lo9 : wd == 2 ? hi9 : 0ull;
      cc = d.m.cursor();
      p2_st(&cur[(size_t)(i + 1) * nr], cc);
      k = i + 1;
    }
  }
  p2_st(&out.k[b], k);
  p2_st(&out.c[b], cc);
  p2_st(&out.bag[b], bag);
#pragma unroll
  for (int i = 0; i < kAheadWords; i++) p2_st(&out.q[(size_t)i * nr + b], q[i]);
  p2_st(&out.tag[b], e * 8 + stage + 1);
}

// a wave of a draw-X or draw-Y block that runs no play stage (kP2Wave):
// a draw stage, which stages its own window (the wave's) and reads only it,
// or P1
__device__ __forceinline__ void p2_draw(const P2Args &a, int blk, int code) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b0 = blk * kBlock;
  if (code < kP2Draw) {
    p2_draw_stage(a, b0, lane, code, w * kP2WinRows * kWinStride);
  } else if (code == kWvP1 && b0 + lane < a.n) {
    p2_p1(a, b0 + lane);
  }
}

// a play stage's state after its plies, for the next play stage
__device__ __forceinline__ void p2_mid_put(const P2Mid &m, size_t nr, int b, const State &s, const PlayDraw2 &d, int g,
                                           int e) {
#pragma unroll
  for (int k = 0; k < 4; k++) p2_st(&m.st[(size_t)k * nr + b], s.pl[k]);
  p2_st(&m.st[4 * nr + b], s.piles);
  p2_st(&m.st[5 * nr + b], s.misc);
  p2_st(&m.q[b], d.q0);
  p2_st(&m.q[nr + b], d.q1);
  p2_st(&m.q[2 * nr + b], d.q2);
  p2_st(&m.q[3 * nr + b], d.q3);
  p2_st(&m.i[b], d.d);
  p2_st(&m.i[nr + b], g);
  p2_st(&m.i[2 * nr + b], d.fell ? d.gm.cursor() : -1);
  p2_st(&m.tag[b], e);
}
// (read back by the next play stage's opening, p2_play: m.i is script entries
// used, plies played, the slot stream's cursor if the game fell onto it)

// Play stage st on episode ep + kP2Play - 1 - st (the last stage: the rest of
// episode ep, or all of it).  In a play block (in_block) wave w runs stage
// kP2Play - 1 - w, the last on wave 0 with its LDS fallback; with five stages,
// stage 0 runs on a wave of a draw block (kWvPlay: it needs no LDS and joins
// no barrier).  The stages run one code path (st wave-uniform), so a block's
// waves share one copy of the ply loop in the instruction cache (one inlined
// copy per stage, ~50 KB each, thrashed the cache the two CUs of a pair
// share), and k_play2 calls this from one place.
__device__ __forceinline__ void p2_play(const P2Args &a, int blk, int st, bool in_block) {
  __shared__ uint64_t s_lds_mask;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b0 = blk * kBlock, b = b0 + lane;
  HZ_DIAG_T0(t0);
  const bool last = st == kP2Play - 1;
  // The opening is one scalar batch and one vector batch.  Scalar: the
  // stage's record and n, nrow (p2_play_args).  Vector, all issued before the
  // first wait and used only after it: the episode counter, the script's tag
  // and length, the previous stage's tag, the script,
  // the previous stage's state, and the eight hash rows of the turn pair the
  // stage expects to start with, [g0, g0 + 8) (g0 = the cut before it, an
  // argument; p2_plies takes them as its first pair read ahead, and uses
  // them only if every lane has the slot's hashes and stands at g0).  No
  // guard: a lane past n reads board n - 1's words (valid memory in every
  // array, whether sized n or nrow) and discards them; the first stage,
  // which has no previous one, reads one board's state of the second stage's
  // input and discards it.  The tags are compared after.
  int n;
  size_t nr;
  uint64_t seed_base;
  const P2PlayArgs r = p2_play_args(a, st, n, nr, seed_base);
  const int fell_lim = r.fell_lim;
  if (last) P2_PHASE(38, t0);
  const bool act = b < n;
  const uint64_t actmask = __ballot(act);
  const int nb = n - b0 < kBlock ? n - b0 : kBlock;
  const int bc = min(b, n - 1), bi = st > 0 ? bc : b0;
  const uint32_t c4 = (uint32_t)bc * 4u, c8 = c4 * 2u, i4 = (uint32_t)bi * 4u, i8 = i4 * 2u;
  // (a pair past the hash table, cuts up to 2^20 are accepted, is not loaded early: the rows of ply 0, unused)
  const bool h0_fits = r.g0 + 8 <= kRulePlies;
  const int h0_g = h0_fits ? r.g0 : -1;
  const size_t h0_row = h0_fits ? (size_t)r.g0 : 0;
  const uint64_t *qr[4], *str[6];
  const int32_t *ir[3];
  const uint32_t *hr[8];
#pragma unroll
  for (int k = 0; k < 4; k++) qr[k] = p2_row(r.q, (size_t)k * nr);
#pragma unroll
  for (int k = 0; k < 6; k++) str[k] = p2_row(r.in.st, (size_t)k * nr);
#pragma unroll
  for (int k = 0; k < 3; k++) ir[k] = p2_row(r.in.i, (size_t)k * nr);
#pragma unroll
  for (int j = 0; j < 8; j++) hr[j] = p2_row(r.h, (h0_row + j) * nr);
  p2_fence();
  int ep = p2_at(r.ep, c4);
  const int ptag = p2_at(r.ptag, c4), nd = p2_at(r.pk, c4), itag = p2_at(r.in.tag, i4);
  const int id = p2_at(ir[0], i4), ig = p2_at(ir[1], i4), ifc = p2_at(ir[2], i4);
  uint64_t sq[4], ist[6];
#pragma unroll
  for (int k = 0; k < 4; k++) sq[k] = p2_at(qr[k], c8);
#pragma unroll
  for (int k = 0; k < 6; k++) ist[k] = p2_at(str[k], i8);
  uint32_t h0[8];
#pragma unroll
  for (int j = 0; j < 8; j++) h0[j] = p2_at(hr[j], c4);
  p2_fence_use(ep);
  if (last) {
    P2_USE_V(ep);
    P2_PHASE(39, t0);
  }
  bool lds_used = false;
  if (act) {
    const int e = ep + r.ep_off;
    const P2Mid &mo = r.out;
    uint32_t *slot = r.slot + b;
    const int32_t *cur = r.cur + b;
    const int g_end = r.g_end;
    const uint64_t sd = episode_seed(seed_base, b, e), rk = rule_key(sd);
    const int mtag = st > 0 ? itag : e;
    State s;
    int g = 0;
    PlayDraw2 draw{{sq[0], sq[1], sq[2], sq[3], 0, nd}, false, MTR(slot, (int)nr, 0, fell_lim), cur + (size_t)nd * nr};
    if (st > 0) {  // the previous play stage's state; the draw source continues its script or the slot stream it fell onto
#pragma unroll
      for (int k = 0; k < 4; k++) s.pl[k] = ist[k];
      s.piles = ist[4];
      s.misc = ist[5];
      g = ig;
      draw.d = id;
      draw.fell = ifc >= 0;
      draw.gm = MTR(slot, (int)nr, ifc >= 0 ? ifc : 0, fell_lim);
    }
    bool prep = ptag == e * 8 + kP2Draw && mtag == e;
    // (the script's tag vouches for the hash rows too: it is given only on a slot seeded for e)
    const uint32_t *hs = r.h + b;
    if (last) {
      P2_USE_V((int)prep);
      P2_PHASE(42, t0);
    }
    if (prep) {
      if (st == 0) {
        if (__all(nd >= 5)) draw.scripted_reset(s);
        else reset_state(s, draw);
      }
      P2_PHASE(16 + 2 * st, t0);
      g += p2_plies(s, draw, g, g_end, rk, hs, nr, h0, h0_g);
      P2_PHASE(17 + 2 * st, t0);
      // a game that drew past the slot's rows: its draws since are not the
      // stream's, so the board counts as unprepared from here on
      if (draw.lost()) prep = false;
    }
    if (!last) {
      if (prep) p2_mid_put(mo, nr, b, s, draw, g, e);
      else mo.tag[b] = -1;
    } else {
      int cursor, src;
      if (prep) {
        cursor = draw.fell ? draw.gm.cursor() : cur[(size_t)draw.d * nr];
        src = 2 + a.s_idx_last;
      } else {  // unprepared: the whole game, the stream seeded and drawn in LDS
        mt_seed(hz_lds + lane, kLdsStride, sd);
        PlayDraw fb{{0, 0, 0, 0, 0, 0}, LdsMT(lane, kMTSeeded), false, false, MT(nullptr, 0), nullptr};
        reset_state(s, fb);
        g = p2_plies(s, fb, 0, a.max_plies, rk, nullptr, nr);
        cursor = fb.m.cursor();
        src = -1;
        lds_used = true;
      }
      a.episode[b] = e + 1;
      if (score_pending(s.misc)) finish_game(s);
      P2_PHASE(27, t0);
      store_state(a.st, a.n, b, s);
      a.pos[b] = cursor;
      a.mt_src[b] = src;
      a.win_tag[b] = -1;
      a.ply[b] = g;
      a.seed[b] = sd;
      a.ep_out[b] = e + 1;
      // the game this call completes, as hz_play's other pipeline counts it
      if (a.games_done) a.games_done[b] = phase_of(s.misc) == PH_OVER ? 1 : 0;
      if (a.steps_done) a.steps_done[b] = g;
    }
    if (in_block) P2_PHASE(w, t0);  // the wave's duration: the last stage .. the second
  }
  if (!in_block) return;
  if (w == 0) {
    const uint64_t lm = __ballot(lds_used);
    if (lane == 0) s_lds_mask = lm;
  }
  __syncthreads();
  const uint64_t lds_mask = s_lds_mask & actmask;
  if (lds_mask) stage_mt(a.mt + (size_t)b0 * kMT, nb, tid, lds_mask, false);
}

// one 162 KB-LDS block per CU, so one wave per SIMD: every wave may use the
// whole register file
__global__ void __launch_bounds__(kStageThreads) __attribute__((amdgpu_waves_per_eu(1, 1))) k_play2(P2Args a, int nblk) {
  const int blk = (int)blockIdx.x;
  const int role = blk / nblk;  // 0 play, 1 draw X, 2 draw Y, 3 seed blocks
  const int rb = blk - role * nblk;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int code = role == 1 || role == 2 ? kP2Wave[4 * (role - 1) + wv] : kWvIdle;
  // the wave's play stage, if it runs one
  const int st = role == 0 ? kP2Play - 1 - wv : code == kWvPlay ? 0 : -1;
#ifdef HZ_DIAG
  if (g_role_only >= 0 && g_role_only != role) return;
  const uint64_t t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
#endif
  if (st >= 0) p2_play(a, rb, st, role == 0);
  else if (role == 3) p2_seed(a, rb);
  else if (role != 0) p2_draw(a, rb, code);
#ifdef HZ_DIAG
  {  // wave durations per board, slot 4 role + wave: 0-3 play (the last stage
     // .. the second: stamped in p2_play, before its barrier), 4-7 draw X,
     // 8-11 draw Y (kP2Wave says what each runs), 12-15 seed (P2a, P2b, P2c,
     // twist)
    const int w = threadIdx.x >> 6, bb = rb * kBlock + (threadIdx.x & 63);
    const bool idle = (role == 1 || role == 2) && code == kWvIdle;
    if (g_stamps && role > 0 && !idle && bb < a.n) g_stamps[(size_t)bb * kP2Stamps + 4 * role + w] = __builtin_amdgcn_s_memtime() - t0;
    // the wave's realtime (100 MHz) start and end and its clock cycles, per
    // (role, wave): slot 40 of the block's boards 16 role + 4 w + k
    // (tools/p2_span.py: the launch's span against its waves')
    if (g_stamps && bb < a.n && (threadIdx.x & 63) < 4) {
      const int k = threadIdx.x & 63;
      const uint64_t v = k == 0 ? r0 : k == 1 ? __builtin_amdgcn_s_memrealtime() : k == 2 ? t0 : __builtin_amdgcn_s_memtime();
      g_stamps[(size_t)(rb * kBlock + 16 * role + 4 * w + k) * kP2Stamps + 40] = v;
      // where the wave ran: HW_ID (cu, sh, se in bits 8-14) and XCC_ID
      if (k == 0)
        g_stamps[(size_t)(rb * kBlock + 16 * role + 4 * w) * kP2Stamps + 41] =
            (uint64_t)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((uint64_t)__builtin_amdgcn_s_getreg((15 << 11) | 20) << 32);
    }
  }
#endif
}

// Boards whose stream lives in a pipeline-2 slot (mt_src = 2 + slot).  A slot
// holds only the rows the pipeline reads (the next generation's rows below
// kAheadTwist and a few of the old one), so the board's own stream is rebuilt
// from what the last play stage left: init_by_array of the episode's seed,
// then the twist of the rows below the cursor's tw, bit for bit the state a
// whole slot would hold.  64 boards per block, a lane per board, in LDS, like
// the reset's seeding and at its cost (one seeding per block, tens of
// microseconds for 4096 boards, where the copy it replaces moved 10 MB: no
// timed path runs it; DESIGN section 3, "Round 14").
__global__ void __launch_bounds__(kStageThreads) k_mt_materialize2(uint32_t *__restrict__ mt,
                                                                  const uint64_t *__restrict__ seed,
                                                                  const int32_t *__restrict__ pos,
                                                                  int32_t *__restrict__ mt_src, int n) {
  __shared__ uint64_t s_mask;
  const int tid = threadIdx.x, lane = tid & 63;
  const int b0 = blockIdx.x * kBlock, b = b0 + lane;
  const int nb = n - b0 < kBlock ? n - b0 : kBlock;
  if (tid < 64) {
    const int src = b < n ? mt_src[b] : -1;
    const bool mine = src >= 2 && src < 2 + kP2Stream;
    const uint64_t m = __ballot(mine);
    if (lane == 0) s_mask = m;
    if (mine) {
      mt_seed(hz_lds + lane, kLdsStride, seed[b]);
      LdsMT s(lane, kMTSeeded);
      s.twist_ahead(pos[b] >> 16);
      mt_src[b] = -1;
    }
  }
  __syncthreads();
  const uint64_t mask = s_mask;
  if (mask) stage_mt(mt + (size_t)b0 * kMT, nb, tid, mask, false);
}


}  // namespace
