// hz_env.hip — batched Harmonies env kernels and their C-ABI (include/hz_abi.h).
//
// Every env kernel is lane-per-board: thread b owns board b, loads its 48 B
// SoA record (coalesced: 64 lanes x 8 B per word), runs the rules from
// hz_device.hpp in registers and stores the record back.  The encoder is
// element-parallel instead (it writes 5,488 B per board and is HBM-bound).
//
// This file holds struct hz_env, the diagnostic macros, the per-ply API
// kernels, the materialize / import kernels and the C-ABI with its launchers;
// the fused pipelines live in hz_chance.hpp, hz_rollout.hpp and hz_play2.hpp,
// included below into this one translation unit.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/hz_abi.h"
#include "hz_device.hpp"
#include "hz_encode.hpp"
#include "hz_host.hpp"

using namespace hz;
using namespace hz_host;

// pipeline-2 hand-offs (k_play2), per board, rows of nrow
struct P2Draw {   // a draw stage's output: the pile script so far
  int32_t *tag;   // [nrow] episode * 8 + draw stages done
  int32_t *k;     // [nrow] draws done
  uint64_t *q;    // [4][nrow] the script: draw i at bits 9 i ..
  uint64_t *bag;  // [nrow] bag fields (misc layout) after those draws
  int32_t *c;     // [nrow] stream cursor after those draws
};
struct P2Mid {    // a play stage's end state, for the next play stage
  int32_t *tag;   // [nrow] episode
  uint64_t *st;   // [6][nrow] state
  uint64_t *q;    // [4][nrow] the rest of the script
  int32_t *i;     // [3][nrow] script entries used, plies played, stream cursor if fell (else -1)
};

// pipeline 2's shape (k_play2): one seeding stage for pass 1, three for pass
// 2, kP2Draw draw stages, kP2Play play stages.  (A/B builds: -DHZ_P2_NDRAW=5
// or 4 and / or -DHZ_P2_NPLAY=4 leave the waves of the last stages idle.)
#ifndef HZ_P2_NDRAW
#define HZ_P2_NDRAW 6
#endif
#ifndef HZ_P2_NPLAY
#define HZ_P2_NPLAY 5
#endif
constexpr int kP2Draw = HZ_P2_NDRAW;
constexpr int kP2Play = HZ_P2_NPLAY;
constexpr int kP2SDraw = 4;                    // the first draw stage (after P1, P2a, P2b, P2c)
constexpr int kP2SPlay = kP2SDraw + kP2Draw;   // the first play stage
constexpr int kP2Stages = kP2SPlay + kP2Play;
constexpr int kP2Last = kP2Stages - 1;  // stage s works on episode ep + kP2Last - s
constexpr int kP2Ring = kP2Play + 1;    // the last draw stage's scripts: read by the play stages 1..kP2Play calls later
// stream slots: one per stage from P2a on (P1 runs in registers), plus one:
// the last play stage's slot stays the board's stream
constexpr int kP2Stream = kP2Stages;
static_assert(kP2Draw >= 2 && kP2Draw <= 6 && kP2Play >= 2 && kP2Play <= 5, "stage counts");

// Created by value-initialising new: every field starts zero.  The device
// buffers belong to three owners by lifetime (bufs: hz_env_create; p2_bufs:
// alloc_p2; ar_bufs: alloc_ar), each freed by its release().
struct hz_env {
  DevBufs bufs, p2_bufs, ar_bufs;
  int32_t n;
  uint64_t seed_base;
  hipStream_t stream;
  uint64_t *state;   // [6][n]
  uint32_t *mt;      // [n][624] board-major MT19937 words
  int32_t *pos;      // [n] MT cursor (pos | tw << 16, see hz_device.hpp)
  int32_t *ply;      // [n]
  int32_t *episode;  // [n]
  uint64_t *seed;    // [n]
  // chance-ahead (hz_play): extra blocks of the same launch prepare each
  // board's next episodes (seed, draw1, draw2 stages; see the stages and
  // launch_rollout) while the playing blocks play the current one
  int seed_ahead;            // scripted draws prepared per board (0: off; default kAheadDraws)
  uint32_t *ahead_mt[2];     // [n][624] seeded streams
  int32_t *ahead_tag[2];     // [n] episode each slot holds (-1: none)
  uint64_t *ahead_pile[2];   // [kAheadWords][n] prepared pile scripts
  int32_t *ahead_cur[2];     // [kAheadDraws + 1][n] stream cursor after each scripted draw
  uint32_t *ahead_rule[2];   // [kRulePlies][nrow] rule hashes (top 32 bits) per ply
  int32_t *ep_final[2];      // [n] episode counter after the k_rollout that read the slot
  size_t nrow;               // n rounded up to 64: row stride of the ring slots
  uint32_t *ring_mt[3];      // [624][nrow] word-major streams, three calls / two calls ahead
  int32_t *ring_tag[3];      // [nrow] episode * 4 + stage done
  uint64_t *ring_pile[3];    // [3][nrow] draw1's partial scripts
  int32_t *ring_cur[3];      // [kD1Draws + 1][nrow] cursors
  int32_t *ring_k1[3];       // [nrow] draws draw1 completed
  int calls;                 // hz_play calls (ring and play-slot rotation)
  int primed, slot_valid[2];
  // where board b's current stream lives: -1 = mt (its own), k = ahead_mt[k]
  // (an hz_play board that replayed a prepared episode keeps playing on the
  // prepared copy; it is copied into mt only when something else needs it:
  // materialize(), before any other entry point that reads streams)
  int32_t *mt_src;           // [n]
  int lazy;                  // some board may have mt_src >= 0
  // auto-reset episodes prepared ahead (hz_rollout with auto_reset; see
  // ar_prep_stage): slot s of board b holds one episode's pile script,
  // cursors and stream, tagged with the episode; mt_src = kArSrc + s while a
  // board plays on slot s's stream
  int ar_ahead;              // on unless HZ_AR_AHEAD=0 / hz_env_set_auto_ahead(e, 0)
  uint32_t *ar_mt;           // [kArSlots][n][624]
  int32_t *ar_tag;           // [kArSlots][n] episode held (-1: none)
  uint64_t *ar_pile;         // [kArSlots][kAheadWords][n]
  int32_t *ar_cur;           // [kArSlots][kAheadDraws + 1][n]
  int32_t *ar_ep[2];         // [n] episode counter at the start of an auto-reset call, by call parity
  int ar_calls, ar_primed;
  // per-ply draw windows (k_step / k_ply; see PlyWin): 12 stream words per
  // board saved by the ply before a turn end, tagged with the cursor; every
  // other entry point that can move or rewrite streams sets the tags to
  // none in stream order (its kernel, or touch)
  uint32_t *pw_words;        // [kPlyWin][nrow]
  int32_t *pw_tag;           // [nrow] cursor the words start at (-1: none)
  // pipeline 2 (hz_env_set_pipeline(e, 2); see k_play2): every board's game
  // spread over kP2Stages consecutive hz_play calls, one stage per call
  int pipeline;              // 1: chance-ahead (k_rollout's roles), 2: k_play2
  int calls2, primed2;
  int p2_cut[kP2Play - 1];   // the play stages' ply boundaries (HZ_P2_CUTS5)
  int p2_dcut[kP2Draw + 1];  // the draw stages' first draws (HZ_P2_DCUTS); [0] = 0, [kP2Draw] = kAheadDraws
  int p2_fell_lim;           // slot rows a play stage may draw from past its script (HZ_P2_FELL_LIMIT)
  uint32_t *p2_s[kP2Stream];     // [624][nrow] stream slots
  int32_t *p2_s_tag[kP2Stream];  // [nrow] episode * 8 + 3 P2a / 4 P2b / 5 seeded, rows 0-223 twisted (-1: none)
  int32_t *p2_s_cur[kP2Stream];  // [kAheadDraws + 1][nrow] the slot's cursor before draw 0 and after each draw
  uint32_t *p2_p1h[2];       // [nrow] P1 -> P2a: pass 1's row-1 word after its last step
  int32_t *p2_p1t[2];        // [nrow] its tag: episode * 8 + 2
  uint32_t *p2_p2h[2];       // [4][nrow] P2a -> P2b
  uint32_t *p2_p3h[2];       // [4][nrow] P2b -> P2c
  P2Draw p2_x[kP2Draw - 1][2];   // D1 -> D2 -> ... -> the last draw stage, by call parity
  P2Draw p2_pl[kP2Ring];         // the last draw stage -> every play stage: a ring
  P2Mid p2_m[kP2Play - 1][2];    // play stage st -> st + 1, by call parity
  uint32_t *p2_h[kP2Stream];     // [kRulePlies][nrow] rule hashes: entry k goes with stream slot k (and its tag)
  int32_t *p2_ep[2];         // [nrow] episode counter each board ended the call with
  // a pipeline wave that gives up waiting for its publisher (a bounded spin
  // on an LDS progress counter) ORs a bit into *wait_err (kWaitErr*), so the
  // host raises instead of trusting the call's streams (hz_env_set_error_word)
  int32_t *wait_err_own;     // [1] the handle's own word
  int32_t *wait_err;         // the word the kernels OR into (caller's or own)
  int spin_limit;            // s_sleep rounds before a wait gives up (hz_env_set_spin_limit)
};

#ifdef HZ_DIAG
// diagnostic build only (tools/diag.py): per-lane phase clocks; g_role_only
// >= 0 runs only that k_rollout role (0 draw2, 1 draw1, 2 seed, 3 play)
__device__ uint64_t *g_stamps;
__device__ int g_role_only = -1;
#define HZ_STAMP(slot)                                                    \
  do {                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                    \
    if (g_stamps) g_stamps[(size_t)b * 16 + (slot)] = __builtin_amdgcn_s_memtime(); \
    __builtin_amdgcn_sched_barrier(0);                                    \
  } while (0)
#ifndef HZ_DIAG_ROLES_ONLY
#define HZ_ACC(slot, t0)                                                  \
  do {                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                    \
    uint64_t _t = __builtin_amdgcn_s_memtime();                           \
    acc##slot += _t - (t0);                                               \
    t0 = _t;                                                              \
    __builtin_amdgcn_sched_barrier(0);                                    \
  } while (0)
#else  // role durations only (tools/libhz_roles.so): no stamps inside the ply loop
#define HZ_ACC(slot, t0) \
  do {                   \
  } while (0)
#endif
// phase boundary inside a preparation role: cycles since the role began
#define HZ_PHASE(slot, t0, b)                                                                 \
  do {                                                                                        \
    __builtin_amdgcn_sched_barrier(0);                                                        \
    if (g_stamps) g_stamps[(size_t)(b) * 16 + (slot)] = __builtin_amdgcn_s_memtime() - (t0); \
    __builtin_amdgcn_sched_barrier(0);                                                        \
  } while (0)
// a phase's or a role's start clock
#define HZ_DIAG_T0(name) uint64_t name = __builtin_amdgcn_s_memtime()
// run only the role the tool asked for (g_role_only)
#define HZ_DIAG_ROLE_GATE(role) \
  if (g_role_only >= 0 && g_role_only != (role)) return
#else
#define HZ_STAMP(slot) \
  do {                 \
  } while (0)
#define HZ_PHASE(slot, t0, b) \
  do {                        \
  } while (0)
#define HZ_ACC(slot, t0) \
  do {                   \
  } while (0)
#define HZ_DIAG_T0(name) \
  do {                   \
  } while (0)
#define HZ_DIAG_ROLE_GATE(role) \
  do {                          \
  } while (0)
#endif
// the roles-only build's own stamps and counters (tools/role_alone.py,
// p2_roles.py, ar_passes.py): HZ_PHASE / a statement there, nothing elsewhere
#ifdef HZ_DIAG_ROLES_ONLY
#define HZ_ROLE_PHASE(slot, t0, b) HZ_PHASE(slot, t0, b)
#define HZ_ROLES_ONLY(...) __VA_ARGS__
#else
#define HZ_ROLE_PHASE(slot, t0, b) \
  do {                             \
  } while (0)
#define HZ_ROLES_ONLY(...)
#endif

namespace {

constexpr int kBlock = 64;  // one wave per workgroup: 4096 boards -> 64 waves

inline int grid_for(int n) { return (n + kBlock - 1) / kBlock; }

// The 64-board LDS kernels (k_reset, k_rollout) run 256
// threads per block: wave 0 plays (lane = board), waves 1-3 only help move
// the block's streams between HBM and LDS (one 162 KB block per CU, so the
// extra waves cost no occupancy) and wait at the barriers meanwhile.
constexpr int kStageThreads = 256;
constexpr size_t kResetLds = (size_t)kMT * kLdsStride * sizeof(uint32_t);  // 162,240 B

}  // namespace

// The rest of this translation unit's device code, one file per pipeline
// (each continues the anonymous namespace and uses the macros and constants
// above): the chance machinery both pipelines share, hz_play's first pipeline
// and hz_rollout (k_rollout and its preparing roles), hz_play's second
// pipeline (k_play2).
#include "hz_chance.hpp"
#include "hz_rollout.hpp"
#include "hz_play2.hpp"

namespace {

// ------------------------------------------------------------------ reset
// Lane-per-board with the 64 boards' MT arrays staged in LDS as [624][65]
// words (stride 65: the per-lane seeding writes and the board-major write-out
// reads are both bank-conflict free).  Seeding (two serial 623-step passes)
// and the 15 opening draws run at LDS latency; one coalesced pass then writes
// the block's contiguous 64 x 2,496 B of HBM.
__global__ void __launch_bounds__(kStageThreads) k_reset(uint64_t *__restrict__ st, uint32_t *__restrict__ mt,
                                                  int32_t *__restrict__ pos, int32_t *__restrict__ ply,
                                                  int32_t *__restrict__ episode, uint64_t *__restrict__ seed,
                                                  int n, uint64_t seed_base, const uint8_t *__restrict__ sel,
                                                  const uint64_t *__restrict__ seeds) {
  int tid = threadIdx.x;
  int lane = tid & 63;
  bool w0 = tid < 64;
  int b0 = blockIdx.x * kBlock;
  int b = b0 + lane;
  bool act = b < n && (!sel || sel[b]);
  uint64_t actmask = __ballot(act);  // the same in every wave
  if (w0 && act) {
    uint64_t sd;
    if (seeds) {
      sd = seeds[b];
    } else {
      int e = episode[b];
      sd = episode_seed(seed_base, b, e);
      episode[b] = e + 1;
    }
    HZ_STAMP(0);
    mt_seed(hz_lds + lane, kLdsStride, sd);
    HZ_STAMP(1);
    StreamDraw<LdsMT> d{LdsMT(lane, kMTSeeded)};
    State s;
    reset_state(s, d);
    HZ_STAMP(2);
    store_state(st, n, b, s);
    pos[b] = d.m.cursor();
    ply[b] = 0;
    seed[b] = sd;
  }
  __syncthreads();
  int nb = n - b0 < kBlock ? n - b0 : kBlock;
  if (w0 && act) HZ_STAMP(3);
  stage_mt(mt + (size_t)b0 * kMT, nb, tid, actmask, false);
  if (w0 && act) HZ_STAMP(4);
}

// ------------------------------------------------------------- legal mask
__global__ void __launch_bounds__(kBlock) k_legal(const uint64_t *__restrict__ st, int n,
                                                  uint64_t *__restrict__ mask, int32_t *__restrict__ count) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  State s = load_state(st, n, b);
  uint64_t m[3];
  int c = legal_mask(s, m);
  if (game_done(s.misc)) { m[0] = m[1] = m[2] = 0; c = 0; }
  mask[(size_t)b * 3 + 0] = m[0];
  mask[(size_t)b * 3 + 1] = m[1];
  mask[(size_t)b * 3 + 2] = m[2];
  if (count) count[b] = c;
}

// ---------------------------------------------------- per-ply draw windows
// A turn end draws one pile (harmonies_engine.py:301-329 -> :132-137):
// ~4 stream words, a twist of the generation in place every other time.
// The per-ply kernels (k_step, k_ply) spread that memory work over the turn
// instead of putting it on the turn-ending ply: the ply that makes a turn's
// first placement twists the stream ahead until 12 words past the cursor
// are twisted; the ply that makes the second saves those 12 words in the
// board's slot (word-major, so the turn-ending ply loads them coalesced,
// with its state, in the same round trip), tagged with the cursor.  The
// turn-ending ply draws from the slot when the tag is its cursor (WinGMT's
// window, marked fresh: no load), from memory otherwise.  The words are the
// stream's own, and every other entry point that can move or rewrite a
// stream voids the tags on the device, in stream order: hz_rollout's and
// hz_play's kernels store -1 to the tag of every board they play (with its
// cursor), the others fill every tag with -1 first (touch, below).  A
// captured call does so again at every replay and a replayed ply reads the
// tags current, so results never depend on the slot.
constexpr int kPlyWin = 12;
static_assert(kPlyWin == 12, "WinMT12's window");
struct PlyWin {
  uint32_t *w;   // [kPlyWin][nrow]
  int32_t *tag;  // [nrow]
  long nrow;
};
struct PlyWinIn {  // a board's slot, loaded with its state
  uint32_t q[kPlyWin];
  int32_t tag;
};
__device__ __forceinline__ PlyWinIn win_load(const PlyWin &pw, int b) {
  PlyWinIn in;
#pragma unroll
  for (int j = 0; j < kPlyWin; j++) in.q[j] = pw.w[(size_t)j * pw.nrow + b];
  in.tag = pw.tag[b];
  return in;
}
// the turn-ending ply: draw from the saved words when they are this cursor's
__device__ __forceinline__ void win_take(const PlyWinIn &in, WinMT12 &m, int cursor) {
  if (in.tag == cursor) {
#pragma unroll
    for (int j = 0; j < kPlyWin; j++) m.q[j] = in.q[j];
    m.left = kPlyWin;
    m.fresh = true;
  }
}
// after a successful non-drawing step: twist ahead (a first placement made),
// or save the next 12 words (a second placement made: the next ply ends the
// turn).  m's cursor may move tw only (written back by the caller).
__device__ __forceinline__ void win_prepare(const PlyWin &pw, WinMT12 &m, int b, int phase_after) {
  if (phase_after != PH_P2 && phase_after != PH_P3) return;
  if (m.pos >= kMT) return;  // (a generation's end: the draw's own prefetch handles it)
  while (m.tw < kMT && m.tw < m.pos + kPlyWin) m.tw += twist_block_vec(m.w, m.tw);
  if (phase_after != PH_P3) return;
  if (m.tw - m.pos < kPlyWin) {  // the generation ends inside the window
    pw.tag[b] = -1;
    return;
  }
  const int a = m.pos & ~3, sh = m.pos & 3;
  uint32_t f[kPlyWin + 4];
#pragma unroll
  for (int k = 0; k < kPlyWin / 4 + 1; k++) {
    const int o = a + 4 * k <= kMT - 4 ? a + 4 * k : kMT - 4;
    const uint4 v = *(const uint4 *)(m.w + o);
    f[4 * k] = v.x; f[4 * k + 1] = v.y; f[4 * k + 2] = v.z; f[4 * k + 3] = v.w;
  }
#pragma unroll
  for (int j = 0; j < kPlyWin; j++)
    pw.w[(size_t)j * pw.nrow + b] = sh == 0 ? f[j] : sh == 1 ? f[j + 1] : sh == 2 ? f[j + 2] : f[j + 3];
  pw.tag[b] = m.cursor();
}

// the same masks unpacked to one byte per action (bool [n][143], what
// BatchedEnv.legal_actions() hands a caller): each lane unpacks its board's
// three words into LDS, then the block writes its 64 boards' 9,152
// contiguous bytes with 16-B stores (a byte store per action and lane
// would touch 64 lines per instruction)
__global__ void __launch_bounds__(kBlock) k_legal_bytes(const uint64_t *__restrict__ st, int n,
                                                        uint8_t *__restrict__ out, int32_t *__restrict__ count) {
  __shared__ uint4 s_out[kBlock * kActions / 16];
  const int lane = threadIdx.x, b0 = blockIdx.x * kBlock, b = b0 + lane;
  const int nb = n - b0 < kBlock ? n - b0 : kBlock;
  uint64_t m[3] = {0, 0, 0};
  int c = 0;
  if (b < n) {
    const State s = load_state(st, n, b);
    c = legal_mask(s, m);
    if (game_done(s.misc)) { m[0] = m[1] = m[2] = 0; c = 0; }
    if (count) count[b] = c;
  }
  uint8_t *o = reinterpret_cast<uint8_t *>(s_out) + lane * kActions;
#pragma unroll 8
  for (int a = 0; a < kActions; a++) o[a] = (uint8_t)((m[a >> 6] >> (a & 63)) & 1);
  __syncthreads();
  const int total = nb * kActions;  // bytes of this block's boards
  uint8_t *dst = out + (size_t)b0 * kActions;
  // (out + b0 * 143 is 16-B aligned only when b0 is: 64 * 143 = 9,152 = 572 x 16 keeps it so from an aligned base)
  for (int q = lane; q < total / 16; q += kBlock) reinterpret_cast<uint4 *>(dst)[q] = s_out[q];
  for (int i = total / 16 * 16 + lane; i < total; i += kBlock) dst[i] = reinterpret_cast<const uint8_t *>(s_out)[i];
}

// ------------------------------------------------------------------- step
__global__ void __launch_bounds__(kBlock) k_step(uint64_t *__restrict__ st, uint32_t *__restrict__ mt,
                                                 int32_t *__restrict__ pos, int32_t *__restrict__ ply, int n,
                                                 const int16_t *__restrict__ action, int32_t *__restrict__ status,
                                                 PlyWin pw) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  // every load of the step issued with the action's (one memory round trip;
  // a no-op board's loads go unused)
  const int a = action[b];
  State s = load_state(st, n, b);
  const int c0 = pos[b];
  const PlyWinIn win = win_load(pw, b);
  // (the compiler would sink these loads past the no-op branch: a second
  // round trip; naming them here keeps all of them in the first)
  asm volatile("" ::"v"(s.pl[0]), "v"(s.pl[1]), "v"(s.pl[2]), "v"(s.pl[3]), "v"(s.piles), "v"(s.misc), "v"(c0),
               "v"(win.tag), "v"(win.q[0]), "v"(win.q[1]), "v"(win.q[2]), "v"(win.q[3]), "v"(win.q[4]),
               "v"(win.q[5]), "v"(win.q[6]), "v"(win.q[7]), "v"(win.q[8]), "v"(win.q[9]), "v"(win.q[10]),
               "v"(win.q[11]));
  if (a < 0) {
    if (status) status[b] = ST_NOOP;
    return;
  }
  StreamDraw<WinMT12> d{WinMT12(mt + (size_t)b * kMT, c0)};
  if (phase_of(s.misc) == PH_P3) win_take(win, d.m, c0);
  int r = step_state(s, a, d);
  if (r == ST_OK) {
    store_state(st, n, b, s);
    win_prepare(pw, d.m, b, phase_of(s.misc));
    pos[b] = d.m.cursor();
    ply[b] += 1;
  }
  if (status) status[b] = r;
}

// -------------------------------------------- replenish / end-turn (facade)
__global__ void __launch_bounds__(kBlock) k_turn_op(uint64_t *__restrict__ st, uint32_t *__restrict__ mt,
                                                    int32_t *__restrict__ pos, int n, const uint8_t *__restrict__ sel,
                                                    int op) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n || (sel && !sel[b])) return;
  State s = load_state(st, n, b);
  StreamDraw<MT> d{MT(mt + (size_t)b * kMT, pos[b])};
  if (op == 0) replenish(s, d);
  else end_turn(s, d);
  store_state(st, n, b, s);
  pos[b] = d.m.cursor();
}

// ------------------------------------------------------------------ score
__global__ void __launch_bounds__(kBlock) k_score(const uint64_t *__restrict__ st, int n, int32_t *__restrict__ out,
                                                  int32_t *__restrict__ parts) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  State s = load_state(st, n, b);
  for (int p = 0; p < 2; p++) {
    uint32_t pb[4];
    planes_of(s, p, pb);
    ScoreParts r = score_parts(pb);
    if (out) out[(size_t)b * 2 + p] = r.grass + r.mount + r.field + r.bldg + r.water;
    if (parts) {
      int32_t *o = parts + ((size_t)b * 2 + p) * 5;
      o[0] = r.grass; o[1] = r.mount; o[2] = r.field; o[3] = r.bldg; o[4] = r.water;
    }
  }
}

// ------------------------------------------------------------ rule policy
__global__ void __launch_bounds__(kBlock) k_rule(const uint64_t *__restrict__ seed, const int32_t *__restrict__ ply,
                                                 int n, const uint64_t *__restrict__ mask,
                                                 const int32_t *__restrict__ count, int16_t *__restrict__ action) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  uint64_t m[3] = {mask[(size_t)b * 3], mask[(size_t)b * 3 + 1], mask[(size_t)b * 3 + 2]};
  int L = count ? count[b] : __popcll(m[0]) + __popcll(m[1]) + __popcll(m[2]);
  action[b] = L > 0 ? (int16_t)kth_action(m, rule_pick(seed[b], ply[b], L)) : (int16_t)-1;
}

// ------------------------------------------------ one ply of the surface
// The per-ply API path in one launch: get_legal_moves -> the benchmark's
// rule pick -> apply_move (harmonies_engine.py:145-298) for every board,
// with the three calls' outputs written as hz_legal_mask, hz_rule_actions
// and hz_step write them (bit-identical: the same device functions in the
// same order).  One 48 B state load and store per board instead of two loads
// and a store across three launches.
__global__ void __launch_bounds__(kBlock) k_ply(uint64_t *__restrict__ st, uint32_t *__restrict__ mt,
                                                int32_t *__restrict__ pos, int32_t *__restrict__ ply,
                                                const uint64_t *__restrict__ seed, int n,
                                                uint64_t *__restrict__ mask, int32_t *__restrict__ count,
                                                int16_t *__restrict__ action, int32_t *__restrict__ status,
                                                PlyWin pw) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  State s = load_state(st, n, b);
  const int c0 = pos[b];
  const PlyWinIn win = win_load(pw, b);
  // the rule's inputs loaded with the state: read after the mask stores, they
  // were a second dependent memory round trip on every ply
  const int p = ply[b];
  const uint64_t sd = seed[b];
  StreamDraw<WinMT12> d{WinMT12(mt + (size_t)b * kMT, c0)};
  // a third placement ends the turn, whose refill draws: from the words the
  // previous ply saved (PlyWin), or else the stream's read-ahead window (and
  // the twist it may need) fetched now, under the legal-mask and rule work
  const bool early = phase_of(s.misc) == PH_P3 && !game_done(s.misc);
  if (early) {
    win_take(win, d.m, c0);
    d.m.prefetch();  // (a no-op after win_take)
  }
  uint64_t m[3];
  int c = legal_mask(s, m);
  if (game_done(s.misc)) { m[0] = m[1] = m[2] = 0; c = 0; }
  if (mask) {
    mask[(size_t)b * 3 + 0] = m[0];
    mask[(size_t)b * 3 + 1] = m[1];
    mask[(size_t)b * 3 + 2] = m[2];
  }
  if (count) count[b] = c;
  const int a = c > 0 ? kth_action(m, rule_pick(sd, p, c)) : -1;
  if (action) action[b] = (int16_t)a;
  if (a < 0) {
    // (the early prefetch may have twisted words in place: its cursor, the
    // same stream position, goes back with them)
    if (early) pos[b] = d.m.cursor();
    if (status) status[b] = ST_NOOP;
    return;
  }
  int r = step_state(s, a, d);
  if (r == ST_OK) {
    store_state(st, n, b, s);
    win_prepare(pw, d.m, b, phase_of(s.misc));
    ply[b] = p + 1;
  }
  if (r == ST_OK || early) pos[b] = d.m.cursor();
  if (status) status[b] = r;
}

// ---------------------------------------------------------- greedy agent
// evaluation.py:137-196 choose_move_greedy, one wave per board: lane l scores
// legal moves l, l+64 (canonical ascending order) by applying the placement
// to a register copy and scoring the mover's board; a shuffle reduction keeps
// the first strictly best.  The reference applies every candidate with
// apply_move, whose place_tile_3 turn end refills the piles from the global
// `random`: lane 0 replays those L refills (identical bag and piles for every
// candidate) on the board's stream before the real move is stepped.
struct NoDraw {
  __device__ __forceinline__ uint32_t operator()(uint64_t) { return 0x1FFu; }
};

__global__ void __launch_bounds__(64) k_greedy(const uint64_t *__restrict__ st, uint32_t *__restrict__ mt,
                                               int32_t *__restrict__ pos, int n, const uint8_t *__restrict__ sel,
                                               int16_t *__restrict__ action) {
  int b = blockIdx.x, lane = threadIdx.x;
  if (b >= n) return;
  bool on = !sel || sel[b];
  State s = load_state(st, n, b);
  uint64_t mk[3];
  int L = legal_mask(s, mk);
  if (!on || game_done(s.misc) || L == 0) {
    if (lane == 0) action[b] = -1;
    return;
  }
  int ph = phase_of(s.misc), p = player_of(s.misc);
  int best_sc = -1, best_k = 0x7fffffff;
  for (int k = lane; k < L; k += 64) {
    int sc;
    if (ph == PH_CHOOSE) {
      sc = score_player(s, p);  // choosing a pile leaves the board as it is
    } else {
      State t = s;
      NoDraw nd;
      step_state<true>(t, kth_action(mk, k), nd);
      sc = score_player(t, p);
    }
    if (sc > best_sc) { best_sc = sc; best_k = k; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    int osc = __shfl_xor(best_sc, off), ok = __shfl_xor(best_k, off);
    if (osc > best_sc || (osc == best_sc && ok < best_k)) { best_sc = osc; best_k = ok; }
  }
  if (lane == 0) {
    if (ph == PH_P3) {
      StreamDraw<MT> d{MT(mt + (size_t)b * kMT, pos[b])};
      for (int k = 0; k < L; k++) {
        State t = s;
        replenish(t, d);
      }
      pos[b] = d.m.cursor();
    }
    action[b] = (int16_t)kth_action(mk, best_k);
  }
}

// ---------------------------------------------------------- state transfer
__global__ void __launch_bounds__(kBlock) k_mt_normalize(uint32_t *__restrict__ mt, int32_t *__restrict__ pos,
                                                         int n, int32_t *__restrict__ index) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  MT m(mt + (size_t)b * kMT, pos[b]);
  m.normalize();
  pos[b] = m.cursor();
  if (index) index[b] = m.pos;
}

__global__ void __launch_bounds__(kBlock) k_mt_import(int32_t *__restrict__ pos, int n,
                                                      const int32_t *__restrict__ index) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  pos[b] = index[b] | (kMT << 16);  // CPython states are fully twisted
}

}  // namespace

// ======================================================================= ABI
// boards whose stream lives in a play slot (mt_src >= 0): copy it into the
// board's own stream, one wave per board
__global__ void __launch_bounds__(64) k_mt_materialize(uint32_t *__restrict__ mt, const uint32_t *__restrict__ a0,
                                                      const uint32_t *__restrict__ a1, int32_t *__restrict__ mt_src,
                                                      int n) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int src = mt_src[b];
  if (src < 0 || src > 1) return;  // (pipeline-2 slots: k_mt_materialize2)
  const uint32_t *from = (src ? a1 : a0) + (size_t)b * kMT;
  uint32_t *to = mt + (size_t)b * kMT;
  uint32_t v[(kMT + 63) / 64];
#pragma unroll
  for (int k = 0; k < (kMT + 63) / 64; k++) v[k] = lane + 64 * k < kMT ? from[lane + 64 * k] : 0u;
#pragma unroll
  for (int k = 0; k < (kMT + 63) / 64; k++)
    if (lane + 64 * k < kMT) to[lane + 64 * k] = v[k];
  if (lane == 0) mt_src[b] = -1;
}

// boards whose stream lives in an auto-reset slot (mt_src = kArSrc + slot)
__global__ void __launch_bounds__(64) k_mt_materialize_ar(uint32_t *__restrict__ mt, const uint32_t *__restrict__ ar_mt,
                                                         int32_t *__restrict__ mt_src, int n) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int src = mt_src[b];
  if (src < kArSrc || src >= kArSrc + kArSlots) return;
  const uint32_t *from = ar_mt + ((size_t)(src - kArSrc) * n + b) * kMT;
  uint32_t *to = mt + (size_t)b * kMT;
  uint32_t v[(kMT + 63) / 64];
#pragma unroll
  for (int k = 0; k < (kMT + 63) / 64; k++) v[k] = lane + 64 * k < kMT ? from[lane + 64 * k] : 0u;
#pragma unroll
  for (int k = 0; k < (kMT + 63) / 64; k++)
    if (lane + 64 * k < kMT) to[lane + 64 * k] = v[k];
  if (lane == 0) mt_src[b] = -1;
}

static PlyWin ply_win(hz_env *e) { return PlyWin{e->pw_words, e->pw_tag, (long)e->nrow}; }

// the saved draw windows voided on e's stream (streams_touched, hz_host.hpp):
// 0, or 1 if the fill could not be enqueued
static int touch(hz_env *e) { return streams_touched<HipDev>(e) ? 0 : 1; }

static int materialize(hz_env *e) {
  if (!e->lazy) return 0;  // (a lazy board's PlyWin window was voided by the kernel that moved its stream)
  if (e->ar_mt)
    hipLaunchKernelGGL(k_mt_materialize_ar, dim3(e->n), dim3(64), 0, e->stream, e->mt, e->ar_mt, e->mt_src, e->n);
  hipLaunchKernelGGL(k_mt_materialize, dim3(e->n), dim3(64), 0, e->stream, e->mt, e->ahead_mt[0], e->ahead_mt[1],
                     e->mt_src, e->n);
  if (e->p2_s[0])
    hipLaunchKernelGGL(k_mt_materialize2, dim3(grid_for(e->n)), dim3(kStageThreads), kResetLds, e->stream, e->mt,
                       e->seed, e->pos, e->mt_src, e->n);
  e->lazy = 0;
  return launch_err();
}

// ---------------------------------------------------------- pipeline 2 host
static_assert(sizeof(((hz_env *)0)->p2_s) / sizeof(uint32_t *) == kP2Stream, "slot ring");

// every hand-off tag to "none" (a tag names the episode its slot holds, and a
// slot's contents depend only on (board, episode), so this is never needed
// for correctness; it keeps a fresh pipeline from trusting fresh memory)
static int p2_clear_tags(hz_env *e) {
  const size_t bytes = e->nrow * sizeof(int32_t);
  auto c = [&](int32_t *t) { return hipMemsetAsync(t, 0xff, bytes, e->stream) != hipSuccess; };
  for (int k = 0; k < kP2Stream; k++)
    if (c(e->p2_s_tag[k])) return 1;
  for (int k = 0; k < 2; k++)
    if (c(e->p2_p1t[k])) return 1;
  for (int k = 0; k < kP2Draw - 1; k++)
    if (c(e->p2_x[k][0].tag) || c(e->p2_x[k][1].tag)) return 1;
  for (int k = 0; k < kP2Ring; k++)
    if (c(e->p2_pl[k].tag)) return 1;
  for (int k = 0; k < kP2Play - 1; k++)
    if (c(e->p2_m[k][0].tag) || c(e->p2_m[k][1].tag)) return 1;
  return 0;
}

// allocated on first use: kP2Stream stream slots of 2.5 KB per board plus
// ~5 KB of hand-offs per board (the rule hashes' ring, an entry per slot, is
// most of it)
static int alloc_p2(hz_env *e) {
  if (e->p2_s[0]) return 0;
  const size_t nr = e->nrow;
  DevBufs &o = e->p2_bufs;  // (a request after a failed one does nothing: one check at the end)
  for (int k = 0; k < kP2Stream; k++) {
    o.get(e->p2_s[k], nr * kMT * 4);
    o.get(e->p2_s_tag[k], nr * 4);
    o.get(e->p2_s_cur[k], (kAheadDraws + 1) * nr * 4);
    o.get(e->p2_h[k], kRulePlies * nr * 4);
  }
  auto md = [&](P2Draw &d) {
    o.get(d.tag, nr * 4);
    o.get(d.k, nr * 4);
    o.get(d.q, kAheadWords * nr * 8);
    o.get(d.bag, nr * 8);
    o.get(d.c, nr * 4);
  };
  for (int k = 0; k < kP2Draw - 1; k++) md(e->p2_x[k][0]), md(e->p2_x[k][1]);
  for (int k = 0; k < kP2Ring; k++) {
    md(e->p2_pl[k]);
  }
  for (int k = 0; k < kP2Play - 1; k++)
    for (int j = 0; j < 2; j++) {
      P2Mid &mm = e->p2_m[k][j];
      o.get(mm.tag, nr * 4);
      o.get(mm.st, 6 * nr * 8);
      o.get(mm.q, 4 * nr * 8);
      o.get(mm.i, 3 * nr * 4);
    }
  for (int k = 0; k < 2; k++) {
    o.get(e->p2_p1h[k], nr * 4);
    o.get(e->p2_p1t[k], nr * 4);
    o.get(e->p2_p2h[k], 4 * nr * 4);
    o.get(e->p2_p3h[k], 4 * nr * 4);
    o.get(e->p2_ep[k], nr * 4);
  }
  if (!o.ok || p2_clear_tags(e)) {
    o.release();
    return 1;
  }
  e->primed2 = 0;
  return 0;
}

// one hz_play call of pipeline 2 (k_play2).  Call c uses stream slot
// (c - s) % kP2Stream for stage s >= 1 (P1, stage 0, has none); the draw
// stages' hand-offs, P1 -> P2a -> P2b -> P2c and play stage st -> st + 1 by
// call parity; the last draw stage's script in a ring of kP2Ring (read by
// play stage st st + 1 calls later); the rule hashes in a ring as long as the
// slots', indexed like them (entry (c - s) % kP2Stream for stage s: written by
// the seeding stages, P1 included, each its rows, read by the play stages),
// valid whenever the slot's tag says seeded.  Every slot written by
// call c is read by call c + 1 or later, so launch order on the stream is the
// only synchronisation.
static int launch_play2(hz_env *e, int32_t max_plies, int32_t *games_done, int32_t *steps_done) {
  if (alloc_p2(e)) return 1;  // (k_play2 voids PlyWin's window of every board it finishes; hz_play checked e)
  const int c = e->calls2, r = c & 1, w = r ^ 1;
  if (!e->primed2) {
    if (hipMemcpyAsync(e->p2_ep[w], e->episode, (size_t)e->n * sizeof(int32_t), hipMemcpyDeviceToDevice,
                       e->stream))
      return 1;
    e->primed2 = 1;
  }
  P2Args a{};
  a.st = e->state;
  a.mt = e->mt;
  a.pos = e->pos;
  a.ply = e->ply;
  a.episode = e->episode;
  a.seed = e->seed;
  a.n = e->n;
  a.max_plies = max_plies;
  a.err = e->wait_err;
  a.spin = e->spin_limit;
  a.seed_base = e->seed_base;
  a.nrow = (long)e->nrow;
  a.games_done = games_done;
  a.steps_done = steps_done;
  a.mt_src = e->mt_src;
  a.win_tag = e->pw_tag;
  a.ep_in = e->p2_ep[w];
  a.ep_out = e->p2_ep[r];
  auto sl = [c](int s) { return ((c - s) % kP2Stream + kP2Stream) % kP2Stream; };
  for (int s = 1; s < kP2SDraw; s++) {
    a.s_mt[s] = e->p2_s[sl(s)];
    a.s_tag[s] = e->p2_s_tag[sl(s)];
  }
  for (int s = 0; s < kP2SDraw; s++) a.s_h[s] = e->p2_h[sl(s)];
  a.s_idx_last = sl(kP2Last);
  a.p1h_w = e->p2_p1h[r];
  a.p1t_w = e->p2_p1t[r];
  a.p2h_w = e->p2_p2h[r];
  a.p3h_w = e->p2_p3h[r];
  // what each wave of a seed block decides by and starts from (P2a, P2b, P2c)
  a.seed_tag[0] = e->p2_p1t[w];
  a.seed_tag[1] = a.s_tag[2];
  a.seed_tag[2] = a.s_tag[3];
  a.seed_h[0] = e->p2_p1h[w];
  a.seed_h[1] = e->p2_p2h[w];
  a.seed_h[2] = e->p2_p3h[w];
  // one record per draw stage and per play stage (P2DrawArgs, P2PlayArgs).  A
  // first stage has no previous one: its `in` names the second stage's, valid
  // memory that it reads and discards.
  const int draws = e->seed_ahead;
  for (int k = 0; k < kP2Draw; k++) {
    P2DrawArgs &d = a.dr[k];
    const int s = kP2SDraw + k;
    d.slot = e->p2_s[sl(s)];
    d.stag = e->p2_s_tag[sl(s)];
    d.cur = e->p2_s_cur[sl(s)];
    d.in = e->p2_x[k > 0 ? k - 1 : 0][w];
    d.out = k == kP2Draw - 1 ? e->p2_pl[c % kP2Ring] : e->p2_x[k][r];
    d.d0 = e->p2_dcut[k];
    d.d1 = k == kP2Draw - 1 ? draws : std::min(draws, e->p2_dcut[k + 1]);
  }
  for (int st = 0; st < kP2Play; st++) {
    P2PlayArgs &p = a.pp[st];
    const bool last = st == kP2Play - 1;
    const int s = kP2SPlay + st;
    const int k = (c + kP2Ring - 1 - st) % kP2Ring;  // the script written by call c - 1 - st
    p.ep = last ? e->episode : e->p2_ep[w];
    p.ep_off = last ? 0 : kP2Play - 1 - st;
    p.g0 = st > 0 ? e->p2_cut[st - 1] : 0;
    p.g_end = last ? max_plies : std::min(e->p2_cut[st], max_plies);
    p.fell_lim = e->p2_fell_lim;
    p.ptag = e->p2_pl[k].tag;
    p.pk = e->p2_pl[k].k;
    p.q = st > 0 ? e->p2_m[st - 1][w].q : e->p2_pl[k].q;
    p.h = e->p2_h[sl(s)];
    p.slot = e->p2_s[sl(s)];
    p.cur = e->p2_s_cur[sl(s)];
    p.in = e->p2_m[st > 0 ? st - 1 : 0][w];  // play stage st - 1 -> st, by call parity
    p.out = e->p2_m[last ? 0 : st][r];       // (the last stage writes none)
  }
  const int nblk = grid_for(e->n);
  hipLaunchKernelGGL(k_play2, dim3(4 * nblk), dim3(kStageThreads), kResetLds, e->stream, a, nblk);
  if (int err = launch_err()) return err;
  e->lazy = 1;
  e->calls2 = (c + 1) % (kP2Stream * kP2Ring * 2);  // (a multiple of every ring length: slots, script ring, parity)
  e->primed = 0;  // the other pipeline's episode prediction is stale now
  e->ar_primed = 0;
  return 0;
}

extern "C" {

hz_env *hz_env_create(int32_t n_boards, uint64_t seed_base, void *stream) {
  if (n_boards <= 0) return nullptr;
  if (install_comp_table()) return nullptr;  // scoring's component table (hz_device.hpp)
  // k_reset / k_rollout stage 64 boards' MT words in 158 KiB of LDS
  if (lds_opt_in<k_reset>(kResetLds) || lds_opt_in<k_rollout<false, false>>(kResetLds) ||
      lds_opt_in<k_rollout<false, true>>(kResetLds) || lds_opt_in<k_rollout<true, false>>(kResetLds) ||
      lds_opt_in<k_rollout<true, true>>(kResetLds) || lds_opt_in<k_play2>(kResetLds) ||
      lds_opt_in<k_mt_materialize2>(kResetLds))
    return nullptr;
  hz_env *e = new (std::nothrow) hz_env();
  if (!e) return nullptr;
  e->n = n_boards;
  e->seed_base = seed_base;
  e->stream = (hipStream_t)stream;
  const size_t n = (size_t)n_boards, nr = (n + kBlock - 1) / kBlock * kBlock, i32 = sizeof(int32_t);
  e->nrow = nr;
  DevBufs &o = e->bufs;  // (a request after a failed one does nothing: one check at the end)
  o.get(e->state, n * 6 * sizeof(uint64_t), 0);
  o.get(e->mt, n * 624 * sizeof(uint32_t));
  o.get(e->pos, n * i32, 0);
  o.get(e->ply, n * i32, 0);
  o.get(e->episode, n * i32, 0);
  o.get(e->seed, n * sizeof(uint64_t), 0);
  o.get(e->mt_src, n * i32, 0xff);
  for (int k = 0; k < 2; k++) {
    o.get(e->ahead_mt[k], n * kMT * sizeof(uint32_t));
    o.get(e->ahead_tag[k], n * i32, 0xff);
    o.get(e->ahead_pile[k], n * kAheadWords * sizeof(uint64_t));
    o.get(e->ahead_cur[k], n * (kAheadDraws + 1) * i32);
    o.get(e->ahead_rule[k], nr * kRulePlies * sizeof(uint32_t));
    o.get(e->ep_final[k], n * i32);
  }
  for (int k = 0; k < kRing; k++) {
    o.get(e->ring_mt[k], nr * kMT * sizeof(uint32_t));
    o.get(e->ring_tag[k], nr * i32, 0xff);
    o.get(e->ring_pile[k], nr * 3 * sizeof(uint64_t));
    o.get(e->ring_cur[k], nr * (kD1Draws + 1) * i32);
    o.get(e->ring_k1[k], nr * i32);
  }
  o.get(e->pw_words, nr * kPlyWin * sizeof(uint32_t));
  o.get(e->pw_tag, nr * i32, 0xff);
  o.get(e->wait_err_own, i32, 0);
  e->seed_ahead = kAheadDraws;
  e->ar_ahead = env_pick("HZ_AR_AHEAD", 0, 1);
  // hz_play's pipeline: 2 by default, HZ_PIPELINE=1 for the first (hz_env_set_pipeline)
  e->pipeline = env_pick("HZ_PIPELINE", 1, 2);
  // HZ_P2_CUTS5="a,b,c,d": pipeline 2's play stage boundaries (plies,
  // increasing multiples of 4: whole turns; a stage that starts at player
  // 1's turn plays single plies up to the next turn pair).  HZ_P2_CUTS, the
  // three boundaries of four play stages, is read only by a build with four.
  for (int k = 0; k < kP2Play - 1; k++) e->p2_cut[k] = kP2PCut[k];
  if constexpr (kP2Play == 4) env_cuts("HZ_P2_CUTS", e->p2_cut);
  else if constexpr (kP2Play == 5) env_cuts_n("HZ_P2_CUTS5", e->p2_cut, kP2Play - 1, 4, 1 << 20);
  // HZ_P2_DCUTS="a,b,c,d[,e]": the first draws of draw stages 2..5, or 2..6
  // (increasing, 1..23, the sixth's may be 24: an empty stage; stage 1 starts
  // at draw 0; with four values the sixth stage keeps its default, raised to
  // the fifth's; no stage more than kP2StageDraws draws, else the setting is
  // ignored: env_p2_dcuts)
  for (int k = 0; k < kP2Draw; k++) e->p2_dcut[k] = kP2DCut[k];
  e->p2_dcut[kP2Draw] = kAheadDraws;
  if constexpr (kP2Draw >= 5) env_p2_dcuts("HZ_P2_DCUTS", e->p2_dcut, kP2Draw, kAheadDraws, kP2StageDraws);
  // HZ_P2_FELL_LIMIT: the slot rows a play stage may draw from once its
  // script has run out (a slot holds kP2Twist; a game that needs more is
  // played again from scratch by the last play stage).  Lower values only
  // force that path (tests).
  e->p2_fell_lim = env_clamped("HZ_P2_FELL_LIMIT", kP2Twist, 0, kP2Twist);
  e->wait_err = e->wait_err_own;
  e->spin_limit = kSpinLimitDefault;
  if (!o.ok || hipDeviceSynchronize() != hipSuccess) {
    hz_env_destroy(e);
    return nullptr;
  }
  return e;
}

void hz_env_destroy(hz_env *e) {
  if (!e) return;
  e->p2_bufs.release();
  e->ar_bufs.release();
  e->bufs.release();
  delete e;
}

int32_t hz_env_size(const hz_env *e) { return e ? e->n : -1; }

int hz_env_set_error_word(hz_env *e, int32_t *word) {
  if (!e) return -1;
  e->wait_err = word ? word : e->wait_err_own;
  return 0;
}

int hz_env_set_spin_limit(hz_env *e, int32_t limit) {
  if (!e || limit < 0) return -1;
  e->spin_limit = limit ? limit : kSpinLimitDefault;
  return 0;
}

int hz_env_set_pipeline(hz_env *e, int32_t pipeline) {
  if (!e || (pipeline != 1 && pipeline != 2)) return -1;
  e->pipeline = pipeline;
  e->primed = 0;
  e->primed2 = 0;
  return 0;
}

int hz_env_set_auto_ahead(hz_env *e, int32_t on) {
  if (!e) return -1;
  e->ar_ahead = on ? 1 : 0;
  e->ar_primed = 0;
  return 0;
}

int hz_env_set_stream(hz_env *e, void *stream) {
  if (!e) return -1;
  e->stream = (hipStream_t)stream;
  return 0;
}

uint64_t *hz_env_state_ptr(hz_env *e) { return e ? e->state : nullptr; }
uint32_t *hz_env_mt_ptr(hz_env *e) {  // the streams are made current first (materialize)
  if (!e || materialize(e) || touch(e)) return nullptr;  // the caller may move or rewrite streams (PlyWin)
  return e->mt;
}
int32_t *hz_env_mt_pos_ptr(hz_env *e) {
  if (!e || touch(e)) return nullptr;
  return e->pos;
}
int hz_env_stream_ptrs(hz_env *e, uint32_t **mt, int32_t **mt_pos, int32_t **win_tag) {
  if (!e || !mt || !mt_pos || !win_tag) return -1;
  if (int err = materialize(e)) return err;
  *mt = e->mt;
  *mt_pos = e->pos;
  *win_tag = e->pw_tag;
  return 0;
}
int32_t *hz_env_ply_ptr(hz_env *e) { return e ? e->ply : nullptr; }
uint64_t *hz_env_seed_ptr(hz_env *e) { return e ? e->seed : nullptr; }

int hz_env_set_seed_ahead(hz_env *e, int32_t draws) {
  if (!e || draws < 0) return -1;
  e->seed_ahead = draws > kAheadDraws ? kAheadDraws : draws;
  e->primed = 0;
  e->primed2 = 0;
  if (e->p2_s[0] && p2_clear_tags(e)) return 1;
  // draw1's work depends on the draw count: start the ring afresh
  for (int k = 0; k < kRing; k++)
    if (hipMemsetAsync(e->ring_tag[k], 0xff, e->nrow * sizeof(int32_t), e->stream)) return 1;
  return 0;
}

int hz_reset(hz_env *e, const uint8_t *sel, const uint64_t *seeds) {
  if (!e) return -1;
  if (touch(e)) return 1;  // (may move or rewrite streams: PlyWin)
  if (int err = materialize(e)) return err;  // unselected boards keep their streams
  e->primed = 0;  // episode counters move outside hz_play's plan
  e->primed2 = 0;
  e->ar_primed = 0;
  hipLaunchKernelGGL(k_reset, dim3(grid_for(e->n)), dim3(kStageThreads), kResetLds, e->stream, e->state, e->mt, e->pos,
                     e->ply, e->episode, e->seed, e->n, e->seed_base, sel, seeds);
  return launch_err();
}

int hz_legal_actions(hz_env *e, uint8_t *legal, int32_t *count) {
  if (!e || !legal || ((uintptr_t)legal & 15)) return -1;
  hipLaunchKernelGGL(k_legal_bytes, dim3(grid_for(e->n)), dim3(kBlock), 0, e->stream, e->state, e->n, legal, count);
  return launch_err();
}

int hz_legal_mask(hz_env *e, uint64_t *mask, int32_t *count) {
  if (!e || !mask) return -1;
  hipLaunchKernelGGL(k_legal, dim3(grid_for(e->n)), dim3(kBlock), 0, e->stream, e->state, e->n, mask, count);
  return launch_err();
}

int hz_step(hz_env *e, const int16_t *action, int32_t *status) {
  if (!e || !action) return -1;
  if (int err = materialize(e)) return err;
  hipLaunchKernelGGL(k_step, dim3(grid_for(e->n)), dim3(kBlock), 0, e->stream, e->state, e->mt, e->pos, e->ply,
                     e->n, action, status, ply_win(e));
  return launch_err();
}

int hz_rule_ply(hz_env *e, uint64_t *mask, int32_t *count, int16_t *action, int32_t *status) {
  if (!e) return -1;
  if (int err = materialize(e)) return err;
  hipLaunchKernelGGL(k_ply, dim3(grid_for(e->n)), dim3(kBlock), 0, e->stream, e->state, e->mt, e->pos, e->ply,
                     e->seed, e->n, mask, count, action, status, ply_win(e));
  return launch_err();
}

int hz_score(hz_env *e, int32_t *out, int32_t *out_parts) {
  if (!e || (!out && !out_parts)) return -1;
  hipLaunchKernelGGL(k_score, dim3(grid_for(e->n)), dim3(kBlock), 0, e->stream, e->state, e->n, out, out_parts);
  return launch_err();
}

int hz_encode(hz_env *e, const int32_t *idx, int32_t m, float *board, float *glob) {
  if (!e || m < 0 || (!board && !glob)) return -1;
  if (!idx && m > e->n) return -2;
  if (m == 0) return 0;
  launch_encode(e->state, (long)e->n, 1, idx, m, board, glob, e->stream);
  return launch_err();
}

int hz_rule_actions(hz_env *e, const uint64_t *mask, const int32_t *count, int16_t *action) {
  if (!e || !mask || !action) return -1;
  hipLaunchKernelGGL(k_rule, dim3(grid_for(e->n)), dim3(kBlock), 0, e->stream, e->seed, e->ply, e->n, mask, count,
                     action);
  return launch_err();
}

int hz_greedy_actions(hz_env *e, const uint8_t *sel, int16_t *action) {
  if (!e || !action) return -1;
  if (touch(e)) return 1;  // (may move or rewrite streams: PlyWin)
  if (int err = materialize(e)) return err;
  hipLaunchKernelGGL(k_greedy, dim3(e->n), dim3(64), 0, e->stream, e->state, e->mt, e->pos, e->n, sel, action);
  return launch_err();
}

// auto-reset preparation slots, allocated at the first auto-reset hz_rollout
// (40 MB of streams at 4096 boards)
static int alloc_ar(hz_env *e) {
  if (e->ar_mt) return 0;
  const size_t n = (size_t)e->n;
  DevBufs &o = e->ar_bufs;
  o.get(e->ar_mt, kArSlots * n * kMT * sizeof(uint32_t));
  o.get(e->ar_tag, kArSlots * n * sizeof(int32_t), 0xff, e->stream);
  o.get(e->ar_pile, kArSlots * kAheadWords * n * sizeof(uint64_t));
  o.get(e->ar_cur, kArSlots * (kAheadDraws + 1) * n * sizeof(int32_t));
  o.get(e->ar_ep[0], n * sizeof(int32_t));
  o.get(e->ar_ep[1], n * sizeof(int32_t));
  if (!o.ok) {
    o.release();
    return 1;
  }
  e->ar_primed = 0;
  return 0;
}

// hz_play's chance-ahead pipeline: one launch per call c.  Blocks [0, nblk)
// play from play slot r = c & 1; draw2 blocks [nblk, 2 nblk) fill play slot
// w = r ^ 1 for call c + 1 from ring slot (c + 1) % 3; draw1 blocks
// continue ring slot (c + 2) % 3 for call c + 2; seed blocks refill ring
// slot c % 3 for call c + 3.  Launch order on the stream is the only
// synchronisation: a slot written by call c is read by call c + 1; the
// preparing blocks read ep_final[w], written by call c - 1's playing blocks
// (the episode counter each board ended with).  The prediction (call c + k
// resets to that counter plus k) only decides which boards skip seeding and
// drawing: a board replays a slot only when the slot's tag equals its
// episode counter, so results never depend on it.  Anything else that moves
// episode counters (hz_reset, hz_rollout) makes the next call re-prime
// ep_final from the counters.
static int launch_rollout(hz_env *e, int32_t max_plies, int32_t auto_reset, int reset_first, uint64_t *traj_state,
                          uint64_t *traj_mask, int16_t *traj_action, int32_t *games_done, int32_t *steps_done) {
  if (!e || max_plies < 0) return -1;  // (k_rollout voids PlyWin's window of every board it plays)
  e->primed2 = 0;  // (pipeline 2's episode prediction is stale after this launch)
  // hz_rollout continues the current games on their streams; hz_play starts
  // every board's next game (its old stream is dead)
  if (!reset_first)
    if (int err = materialize(e)) return err;
  uint32_t *ahead_mt = nullptr;
  const int32_t *ahead_tag = nullptr;
  const uint64_t *ahead_pile = nullptr;
  const int32_t *ahead_cur = nullptr;
  const uint32_t *ahead_rule = nullptr;
  int32_t *ep_final = nullptr;
  int nblk = grid_for(e->n), grid = nblk;
  bool pipe = reset_first && e->seed_ahead > 0;
  int r = e->calls & 1, w = r ^ 1;
  int c3 = e->calls % kRing;
  auto ring = [e](int k) {
    return Ring{e->ring_mt[k], e->ring_tag[k], e->ring_pile[k], e->ring_cur[k], e->ring_k1[k], e->wait_err,
                e->spin_limit};
  };
  if (pipe) {
    size_t n = (size_t)e->n;
    if (!e->primed) {
      if (hipMemcpyAsync(e->ep_final[w], e->episode, n * sizeof(int32_t), hipMemcpyDeviceToDevice, e->stream))
        return 1;
      e->slot_valid[r] = 0;
      e->primed = 1;
    }
    if (e->slot_valid[r]) {
      ahead_mt = e->ahead_mt[r];
      ahead_tag = e->ahead_tag[r];
      ahead_pile = e->ahead_pile[r];
      ahead_cur = e->ahead_cur[r];
      ahead_rule = e->ahead_rule[r];
    }
    ep_final = e->ep_final[r];
    grid = 4 * nblk;
  } else {
    e->primed = 0;
  }
  bool rec = traj_state || traj_mask || traj_action;
  // hz_rollout with auto-reset: episodes prepared ahead (ar_prep_stage) by
  // 2 x nblk extra blocks; the playing blocks leave the counters they end
  // with for the next call's preparing blocks (ep_final)
  ArArgs ar{};
  const bool ar_on = auto_reset && !reset_first && !rec && e->ar_ahead;
  if (ar_on) {
    if (alloc_ar(e)) return 1;
    const int ar_r = e->ar_calls & 1;
    if (!e->ar_primed) {
      if (hipMemcpyAsync(e->ar_ep[ar_r], e->episode, (size_t)e->n * sizeof(int32_t), hipMemcpyDeviceToDevice,
                         e->stream))
        return 1;
      e->ar_primed = 1;
    }
    ar = ArArgs{e->ar_mt, e->ar_tag, e->ar_pile, e->ar_cur, e->ar_ep[ar_r], 1};
    ep_final = e->ar_ep[ar_r ^ 1];
    grid = 3 * nblk;
  } else {
    e->ar_primed = 0;  // episode counters move outside the auto-reset plan
  }
  auto kern = auto_reset ? (rec ? k_rollout<true, true> : k_rollout<true, false>)
                         : (rec ? k_rollout<false, true> : k_rollout<false, false>);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kStageThreads), kResetLds, e->stream, e->state, e->mt, e->pos, e->ply,
                     e->episode, e->seed, e->n, e->seed_base, max_plies, auto_reset, reset_first, traj_state,
                     traj_mask, traj_action, games_done, steps_done, ahead_mt, ahead_tag, ahead_pile, ahead_cur,
                     e->seed_ahead, ep_final, nblk, e->ahead_mt[w], e->ahead_tag[w], e->ahead_pile[w],
                     e->ahead_cur[w], e->ep_final[w], ring(c3), ring((c3 + 2) % kRing), ring((c3 + 1) % kRing),
                     (long)e->nrow, ahead_rule, e->ahead_rule[w], e->mt_src, ahead_mt ? r : -1, ar, e->pw_tag);
  int err = launch_err();
  if (err) return err;
  if (ahead_mt) e->lazy = 1;
  if (ar_on) {
    e->lazy = 1;
    e->ar_calls++;
  }
  if (pipe) {
    e->slot_valid[w] = 1;
    e->calls++;
  }
  return 0;
}

int hz_rollout(hz_env *e, int32_t max_plies, int32_t auto_reset, uint64_t *traj_state, uint64_t *traj_mask,
               int16_t *traj_action, int32_t *games_done, int32_t *steps_done) {
  return launch_rollout(e, max_plies, auto_reset, 0, traj_state, traj_mask, traj_action, games_done, steps_done);
}

int hz_play(hz_env *e, int32_t max_plies, int32_t auto_reset, uint64_t *traj_state, uint64_t *traj_mask,
            int16_t *traj_action, int32_t *games_done, int32_t *steps_done) {
  if (e && e->pipeline == 2 && !auto_reset && !traj_state && !traj_mask && !traj_action &&
      max_plies >= kP2MinPlies)
    return launch_play2(e, max_plies, games_done, steps_done);
  return launch_rollout(e, max_plies, auto_reset, 1, traj_state, traj_mask, traj_action, games_done, steps_done);
}

int hz_export_state(hz_env *e, uint64_t *state, uint32_t *mt, int32_t *mt_index) {
  if (!e) return -1;
  size_t n = (size_t)e->n;
  if (state && hipMemcpyAsync(state, e->state, n * 6 * sizeof(uint64_t), hipMemcpyDeviceToDevice, e->stream))
    return 1;
  if (mt || mt_index) {
    if (int err = materialize(e)) return err;
    hipLaunchKernelGGL(k_mt_normalize, dim3(grid_for(e->n)), dim3(kBlock), 0, e->stream, e->mt, e->pos, e->n,
                       mt_index);
    int r = launch_err();
    if (r) return r;
    if (mt && hipMemcpyAsync(mt, e->mt, n * kMT * sizeof(uint32_t), hipMemcpyDeviceToDevice, e->stream)) return 1;
  }
  return 0;
}

int hz_import_state(hz_env *e, const uint64_t *state, const uint32_t *mt, const int32_t *mt_index) {
  if (!e) return -1;
  if (touch(e)) return 1;  // (may move or rewrite streams: PlyWin)
  if ((mt == nullptr) != (mt_index == nullptr)) return -2;
  size_t n = (size_t)e->n;
  if (state && hipMemcpyAsync(e->state, state, n * 6 * sizeof(uint64_t), hipMemcpyDeviceToDevice, e->stream))
    return 1;
  if (mt) {
    if (int err = materialize(e)) return err;  // (then every board's stream is its own)
    if (hipMemcpyAsync(e->mt, mt, n * kMT * sizeof(uint32_t), hipMemcpyDeviceToDevice, e->stream)) return 1;
    hipLaunchKernelGGL(k_mt_import, dim3(grid_for(e->n)), dim3(kBlock), 0, e->stream, e->pos, e->n, mt_index);
    return launch_err();
  }
  return 0;
}

int hz_replenish(hz_env *e, const uint8_t *sel) {
  if (!e) return -1;
  if (touch(e)) return 1;  // (may move or rewrite streams: PlyWin)
  if (int err = materialize(e)) return err;
  hipLaunchKernelGGL(k_turn_op, dim3(grid_for(e->n)), dim3(kBlock), 0, e->stream, e->state, e->mt, e->pos, e->n, sel,
                     0);
  return launch_err();
}

int hz_end_turn(hz_env *e, const uint8_t *sel) {
  if (!e) return -1;
  if (touch(e)) return 1;  // (may move or rewrite streams: PlyWin)
  if (int err = materialize(e)) return err;
  hipLaunchKernelGGL(k_turn_op, dim3(grid_for(e->n)), dim3(kBlock), 0, e->stream, e->state, e->mt, e->pos, e->n, sel,
                     1);
  return launch_err();
}

int hz_encode_states(const uint64_t *states, int64_t word_stride, int64_t item_stride, const int32_t *idx, int32_t m,
                     float *board, float *glob, void *stream) {
  if (!states || m < 0 || (!board && !glob)) return -1;
  if (m == 0) return 0;
  launch_encode(states, (long)word_stride, (long)item_stride, idx, m, board, glob, (hipStream_t)stream);
  return launch_err();
}

const char *hz_version(void) { return "hz 0.1 gfx950"; }

#ifdef HZ_DIAG
int hz_diag_set_stamps(uint64_t *p) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &p, sizeof(p)) == hipSuccess ? 0 : 1;
}
int hz_diag_set_role_only(int r) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_role_only), &r, sizeof(r)) == hipSuccess ? 0 : 1;
}
#endif

}  // extern "C"
