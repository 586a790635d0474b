// hz_rollout.hpp — k_rollout: hz_rollout's kernel and hz_play's first
// pipeline, with the roles that prepare episodes ahead in the same launch
// (seed / draw1 / draw2 for hz_play, ar_prep_stage for auto-reset calls).
// Part of hz_env.hip's translation unit (included by it alone, after
// hz_chance.hpp).
#pragma once

namespace {

// ---------------------------------------------------------------- rollout
// Lane-per-board with the block's 64 MT streams resident in LDS for the
// whole call ([624][65] words, as in k_reset): every draw reads and twists at
// LDS latency instead of paying a scattered HBM round trip per draw.  The
// streams are staged in (or seeded in place when reset_first) and written
// back once.
//
// Chance-ahead preparation: a three-stage pipeline in the blocks of each
// hz_play launch beyond the playing ones (4 x 64 blocks of 162 KB LDS: one
// per CU, every CU of the chip).  Stage k works on each board's episode k
// calls ahead (the episode counter the previous launch left, plus k):
//   seed  (k = 3) blocks [3 nblk, 4 nblk): the stream seeded in LDS and
//     stored as seeded to a word-major ring slot (waves 1-3 store rows while
//     wave 0 still seeds);
//   draw1 (k = 2) blocks [2 nblk, 3 nblk): rows [0, kAheadTwist) staged
//     into LDS twisted on the way in (every source still old: no serial
//     chain), the first kD1Draws pile draws run
//     (a lane stops at a draw that would twist further; the next stage
//     redoes it), the partial script, cursors and draw count written beside
//     the slot;
//   draw2 (k = 1) blocks [nblk, 2 nblk): the whole slot staged and twisted
//     likewise, the remaining draws run, and stream (board-major), script,
//     cursors and tag written to the play slot the next call's playing
//     blocks replay.
// Each ring slot carries one tag per board, episode * 4 + stage done, so a
// stage only continues work its predecessor finished for the same
// episode; otherwise it redoes the earlier stages itself in LDS.  A slot's
// contents depend only on (board, episode), so a matching tag is always
// right, whatever happened between the calls.
constexpr int kD1Draws = 16;
constexpr int kRing = 3;
static_assert(kD1Draws <= kAheadDraws && 9 * kD1Draws <= 192, "draw1's script sits in words 0-2");

// one ring slot: the stream word-major (row r of board b at mt[r * nrow + b],
// nrow = n rounded up to 64, so a wave's row is 256 contiguous bytes), and
// per board the tag, draw1's script, cursors and draw count
struct Ring {
  uint32_t *mt;
  int32_t *tag;   // [nrow] episode * 4 + stage (1 seeded, 2 draw1 done); -1 none
  uint64_t *pile; // [kAheadWords][nrow]
  int32_t *cur;   // [kD1Draws + 1][nrow] cursor before draw 0 and after each draw
  int32_t *k1;    // [nrow] draws draw1 completed
  int32_t *err;   // the env's wait-error word (seed stage)
  int spin;       // spin bound of the seed stage's row wait
};

// a board's stream seeded and pre-twisted in its LDS column (cursor kMTAhead)
__device__ __forceinline__ void seed_in_lds(int lane, uint64_t sd) {
  mt_seed(hz_lds + lane, kLdsStride, sd);
  LdsMT m(lane, kMTSeeded);
  m.twist_ahead(kAheadTwist);
}

// pass-2 progress of the seed stage's wave 0, published to waves 1-3 in
// LDS every 32 rows and at the end of the group loop.  A wave's LDS
// operations execute in order, so a plain store of the counter after the
// rows' stores is seen after them (the empty asm only keeps the compiler
// from reordering; a release fence would wait for every pending LDS read
// of the prefetch); readers load it with acquire.  mt_seed_tab reports
// rows = 10, 18, ..., 618; published: 34, 66, ..., 610, 618.
constexpr int kLastPub = 618;
constexpr int kSeedChunk = (kStageThreads - 64) / 16;  // rows per pass of waves 1-3
constexpr int kOverlapEnd = 2 + (kLastPub - 2) / kSeedChunk * kSeedChunk;
struct SeedProgress {
  int *flag;
  __device__ __forceinline__ void operator()(int rows) const {
    if ((rows & 31) == 2 || rows == kLastPub) {
      asm volatile("" ::: "memory");
      __hip_atomic_store(flag, rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
};

// The seed stage's LDS: init_genrand's table at offset 0 (its reads are
// immediate offsets) and the 64 streams after it as [624][64] (row-major,
// so four boards of a row are one aligned 16-B read): kMT + kMT * 64 words
// = the block's 162,240 B.
constexpr int kSeedStride = 64;
static_assert((kMT * kSeedStride + kMT) * 4 <= (int)kResetLds, "seed stage LDS");

__device__ __forceinline__ void seed_stage(int blk, Ring rs, size_t nrow, const int32_t *__restrict__ ep_final,
                                           int n, uint64_t seed_base) {
  __shared__ int s_rows;  // pass-2 rows [2, s_rows) of every board are final
  int tid = threadIdx.x;
  int lane = tid & 63;
  int b = blk * kBlock + lane;
  bool act = b < n;
  HZ_DIAG_T0(t0);
  int e = act ? ep_final[b] + 3 : 0;
  uint32_t *tab = hz_lds, *rows = hz_lds + kMT;
  for (int i = tid; i < kMT; i += kStageThreads) tab[i] = kInitGen.v[i];
  if (tid == 0) s_rows = 0;
  __syncthreads();
  // Stores: four boards of a row per thread (one 16-B LDS read, one 16-B
  // store; a wave covers four rows), the stream as seeded (the draw stages
  // twist rows [0, kAheadTwist) as they stage them, stage_rows_twisted).  Waves 1-3
  // store rows [2, kOverlapEnd) chunk by chunk as wave 0 publishes its pass-2
  // progress; after the barrier all four waves store the rest (the last
  // rows and rows 0, 1, final last).  Columns past n hold whatever LDS held;
  // the next stages never read them.
  int c4 = (tid & 15) * 4;
  uint32_t *out = rs.mt + (size_t)blk * kBlock + c4;
  auto row4 = [&](int r) { return *reinterpret_cast<const uint4 *>(rows + r * kSeedStride + c4); };
  if (tid < 64) {
    if (act) {
      mt_seed_tab<kSeedStride>(rows + lane, tab, episode_seed(seed_base, b, e), SeedProgress{&s_rows});
      HZ_PHASE(0, t0, b);
    }
  } else {
    int done = 0;
#pragma unroll 1
    for (int r0 = 2; r0 < kOverlapEnd; r0 += kSeedChunk) {
      // wave 0 publishes every row up to kLastPub; the bound only guards
      // against a hang should that ever change, and giving up is reported
      for (int spin = 0; done < r0 + kSeedChunk && spin < rs.spin; spin++) {
        __builtin_amdgcn_s_sleep(1);
        done = __hip_atomic_load(&s_rows, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      if (done < r0 + kSeedChunk) {
        done = r0 + kSeedChunk;  // (one report per chunk at most; the rows stored are then untrusted)
        wait_failed(rs.err, kWaitErrSeedRows);
      }
      int r = r0 + ((tid - 64) >> 4);
      *reinterpret_cast<uint4 *>(out + (size_t)r * nrow) = row4(r);
    }
    if (tid < 128 && act) HZ_ROLE_PHASE(11, t0, b);
  }
  __syncthreads();
  if (tid < 64 && act) HZ_ROLE_PHASE(12, t0, b);
  {  // rows [kOverlapEnd, 624) and 0, 1: 12 rows, one per 16-thread group
    int i = tid >> 4, r = i < kMT - kOverlapEnd ? kOverlapEnd + i : i - (kMT - kOverlapEnd);
    if (r < 2 || r >= kOverlapEnd) *reinterpret_cast<uint4 *>(out + (size_t)r * nrow) = row4(r);
  }
  if (tid < 64 && act) {
    rs.tag[b] = e * 4 + 1;
    HZ_PHASE(1, t0, b);
  }
}

__device__ __forceinline__ void draw1_stage(int blk, Ring r1, size_t nrow, const int32_t *__restrict__ ep_final,
                                            int n, uint64_t seed_base, int draws) {
  int tid = threadIdx.x;
  int lane = tid & 63;
  int b0 = blk * kBlock;
  int b = b0 + lane;
  bool act = b < n;
  HZ_DIAG_T0(t0);
  int e = act ? ep_final[b] + 2 : 0;
  bool seeded = act && r1.tag[b] == e * 4 + 1;
  uint64_t smask = __ballot(seeded), fmask = __ballot(act && !seeded);  // the same in every wave
  // rows [0, kAheadTwist), twisted on the way in
  if (smask) stage_rows_twisted(r1.mt, nrow, b0, tid);
  // boards the seed stage missed: seeded here, their stream (as seeded,
  // like the seed stage's) to the slot, then twisted in place
  if (tid < 64 && act && !seeded) mt_seed(hz_lds + lane, kLdsStride, episode_seed(seed_base, b, e));
  __syncthreads();
  if (fmask) {
    unstage_rows(r1.mt, nrow, b0, tid, fmask);
    __syncthreads();
  }
  if (tid < 64 && act) {
    HZ_PHASE(2, t0, b);
    if (!seeded) {
      LdsMT m(lane, kMTSeeded);
      m.twist_ahead(kAheadTwist);
    }
    StreamDraw<LdsMT> d{LdsMT(lane, kMTAhead)};
    uint64_t bag = initial_bag(), q[kAheadWords] = {};
    int32_t *cur = r1.cur + b;
    cur[0] = kMTAhead;
    int k = draws < kD1Draws ? draws : kD1Draws;
    // only the twisted rows are live: a lane stops before a draw that would
    // twist further (draw2, holding the whole stream, redoes it), so the
    // slot's stream stays as seeded and every cursor's tw is kAheadTwist
    int k1 = run_script<true>(d, bag, q, cur, nrow, 0, k);
#pragma unroll
    for (int w = 0; w < 3; w++) r1.pile[(size_t)w * nrow + b] = q[w];
    r1.k1[b] = k1;
    r1.tag[b] = e * 4 + 2;
    HZ_PHASE(3, t0, b);
  }
}

__device__ __forceinline__ void draw2_stage(int blk, Ring r2, size_t nrow, uint32_t *__restrict__ out_mt,
                                            int32_t *__restrict__ tag, uint64_t *__restrict__ pile,
                                            int32_t *__restrict__ cur, uint32_t *__restrict__ rule,
                                            const int32_t *__restrict__ ep_final, int n, uint64_t seed_base,
                                            int draws) {
  int tid = threadIdx.x;
  int lane = tid & 63;
  int b0 = blk * kBlock;
  int b = b0 + lane;
  bool act = b < n;
  uint64_t actmask = __ballot(act);
  int nb = n - b0 < kBlock ? n - b0 : kBlock;
  HZ_DIAG_T0(t0);
  int e = act ? ep_final[b] + 1 : 0;
  bool ok = act && r2.tag[b] == e * 4 + 2;
  uint64_t okmask = __ballot(ok);
  if (okmask) {  // the slot holds the stream as seeded; draw1's cursors say 224 rows twisted
    stage_rows_twisted(r2.mt, nrow, b0, tid);
    stage_rows(r2.mt, nrow, b0, kAheadTwist, kMT, tid);
  }
  __syncthreads();
  if (tid < 64 && act) HZ_PHASE(4, t0, b);
  if (tid >= 64 && act) {  // waves 1-3, while wave 0 draws: the episode's rule hashes
    uint64_t rk = rule_key(episode_seed(seed_base, b, e));
#pragma unroll 1
    for (int j = (tid >> 6) - 1; j < kRulePlies; j += 3) rule[(size_t)j * nrow + b] = rule_h32(rk, j);
  }
  if (tid < 64 && act) {
    uint64_t bag = initial_bag(), q[kAheadWords] = {};
    int start = 0, c0 = kMTAhead;
    if (ok) {  // continue after draw1's draws
      int k1 = r2.k1[b];
      c0 = r2.cur[(size_t)k1 * nrow + b];
#pragma unroll
      for (int w = 0; w < 3; w++) q[w] = r2.pile[(size_t)w * nrow + b];
      // draw1's cursors over (all loads issued before the stores) and the
      // bag replayed from its script; entries past k1 unused
      int32_t cv[kD1Draws];
#pragma unroll
      for (int i = 0; i < kD1Draws; i++) cv[i] = r2.cur[(size_t)i * nrow + b];
#pragma unroll
      for (int i = 0; i < kD1Draws; i++)
        if (i < k1) cur[(size_t)i * n + b] = cv[i];
#pragma unroll
      for (int i = 0; i < kD1Draws; i++) {
        uint32_t p9 = (uint32_t)(q[(9 * i) >> 6] >> ((9 * i) & 63));
        if ((9 * i & 63) > 55) p9 |= (uint32_t)(q[((9 * i) >> 6) + 1] << (64 - ((9 * i) & 63)));
        apply_pile_fast(bag, i < k1 ? p9 & 0x1FFu : 0x1FFu);
      }
      start = k1;
    } else {
      seed_in_lds(lane, episode_seed(seed_base, b, e));
    }
    cur[(size_t)start * n + b] = c0;
    StreamDraw<LdsMT> d{LdsMT(lane, c0)};
    run_script(d, bag, q, cur + b, n, start, draws);
    HZ_PHASE(14, t0, b);
#pragma unroll
    for (int w = 0; w < kAheadWords; w++) pile[(size_t)w * n + b] = q[w];
    tag[b] = e;
  }
  __syncthreads();
  stage_mt(out_mt + (size_t)b0 * kMT, nb, tid, actmask, false);
}

// ------------------------------------------------- auto-reset chance-ahead
// hz_rollout(auto_reset = 1) plays every board on and on, starting its next
// episode (seed_base + b + (e << 32)) whenever a game ends: about 1.5 game
// ends per board per 96-ply call.  Seeding a stream is a 1,246-step serial
// chain (~60 k cycles); in-kernel, the wave of a board whose game ended had
// to wait for it.  As with hz_play's chance-ahead, a game's chance sequence
// does not depend on its moves, so extra blocks of each auto-reset launch
// prepare every board's episodes e0 + 2 and e0 + 3 (e0 = the board's episode
// counter when the call starts: it starts e0 and at most e0 + 1 in the call
// when it takes prepared ones) into a ring of four slots by episode: the
// stream seeded and pre-twisted, its first kAheadDraws pile draws from the
// initial bag run into a script with the cursor after each draw, the stream
// after them.  A board whose game ends then starts episode e from slot e & 3
// when the slot's tag says e (prepared by an earlier call: this call's blocks
// write slots e0 + 2, e0 + 3, never the ones it reads) and e - e0 < 2: a
// scripted reset, no chain, no wait for the rest of the wave; otherwise it
// seeds in place as before.  A slot is tagged only when none of its draws
// twisted past the pre-twisted rows, so the stream as stored and every cursor
// agree (materialize copies it to the board's own stream after the call).
// The preparation only decides where a board's chance draws come from, never
// what they are: results are the same with it off (hz_env_set_auto_ahead).
constexpr int kArSlots = 4;
constexpr int kArSrc = 16;  // mt_src codes kArSrc + slot (0, 1: pipeline 1; 2..15: pipeline 2)
struct ArArgs {
  uint32_t *mt;          // [kArSlots][n][624]
  int32_t *tag;          // [kArSlots][n]
  uint64_t *pile;        // [kArSlots][kAheadWords][n]
  int32_t *cur;          // [kArSlots][kAheadDraws + 1][n]
  const int32_t *ep_in;  // [n] the counters the previous call ended with (the preparing blocks' e0)
  int on;
};

__device__ __forceinline__ void ar_prep_stage(int blk, int k, const ArArgs &ar, int n, uint64_t seed_base) {
  __shared__ uint64_t s_ar_mask[kArSlots];
  const int tid = threadIdx.x, lane = tid & 63, b0 = blk * kBlock, b = b0 + lane;
  const bool act = b < n;
  const int nb = n - b0 < kBlock ? n - b0 : kBlock;
  const int e = act ? ar.ep_in[b] + 2 + k : 0;
  const int sl = e & (kArSlots - 1);
  const bool need = act && ar.tag[(size_t)sl * n + b] != e;  // (prepared by an earlier call: kept)
  if (tid < 64) {
#pragma unroll
    for (int q = 0; q < kArSlots; q++) {
      const uint64_t m = __ballot(need && sl == q);
      if (lane == 0) s_ar_mask[q] = m;
    }
    if (need) {
      seed_in_lds(lane, episode_seed(seed_base, b, e));
      uint64_t bag = initial_bag(), q[kAheadWords] = {};
      int32_t *cur = ar.cur + (size_t)sl * (kAheadDraws + 1) * n + b;
      cur[0] = kMTAhead;
      StreamDraw<LdsMT> d{LdsMT(lane, kMTAhead)};
      run_script(d, bag, q, cur, n, 0, kAheadDraws);
      // the stored stream matches every cursor only if no draw twisted past
      // the pre-twisted rows (a bag of >= 48 tiles: in practice never)
      const bool clean = d.m.tw == kAheadTwist;
#pragma unroll
      for (int w = 0; w < kAheadWords; w++) ar.pile[((size_t)sl * kAheadWords + w) * n + b] = q[w];
      ar.tag[(size_t)sl * n + b] = clean ? e : -1;
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int q = 0; q < kArSlots; q++) {
    const uint64_t m = s_ar_mask[q];
    if (m) stage_mt(ar.mt + ((size_t)q * n + b0) * kMT, nb, tid, m, false);
  }
}

// AutoReset / Record are template parameters so that the common variant
// (play to the end, no trajectory) has a plain loop: no reset path, no
// record stores, fewer live scalar values across the ply loop.
template <bool AutoReset, bool Record>
__global__ void __launch_bounds__(kStageThreads) k_rollout(uint64_t *__restrict__ st, uint32_t *__restrict__ mt,
                                                    int32_t *__restrict__ pos, int32_t *__restrict__ ply,
                                                    int32_t *__restrict__ episode, uint64_t *__restrict__ seed,
                                                    int n, uint64_t seed_base, int max_plies, int auto_reset,
                                                    int reset_first, uint64_t *__restrict__ traj_state,
                                                    uint64_t *__restrict__ traj_mask,
                                                    int16_t *__restrict__ traj_action, int32_t *__restrict__ games_done,
                                                    int32_t *__restrict__ steps_done,
                                                    uint32_t *__restrict__ ahead_mt,
                                                    const int32_t *__restrict__ ahead_tag,
                                                    const uint64_t *__restrict__ ahead_pile,
                                                    const int32_t *__restrict__ ahead_cur, int ahead_draws,
                                                    int32_t *__restrict__ ep_final, int nblk,
                                                    uint32_t *__restrict__ prep_mt, int32_t *__restrict__ prep_tag,
                                                    uint64_t *__restrict__ prep_pile, int32_t *__restrict__ prep_cur,
                                                    const int32_t *__restrict__ prep_ep, Ring rs, Ring r1,
                                                    Ring r2, long nrow, const uint32_t *__restrict__ ahead_rule,
                                                    uint32_t *__restrict__ prep_rule, int32_t *__restrict__ mt_src,
                                                    int src_slot, ArArgs ar, int32_t *__restrict__ win_tag) {
  HZ_DIAG_T0(role_t0);
  if ((int)blockIdx.x >= nblk) {  // chance-ahead roles (uniform per block)
    int blk = (int)blockIdx.x - nblk;
    int role = blk / nblk;
    blk -= role * nblk;
    if constexpr (AutoReset && !Record) {
      if (ar.on) {  // hz_rollout's auto-reset preparation: episodes e0 + 2 (role 0), e0 + 3 (role 1)
        ar_prep_stage(blk, role, ar, n, seed_base);
        return;
      }
    }
#ifdef HZ_PREP_DELAY
    if (role < 2) __builtin_amdgcn_s_sleep(HZ_PREP_DELAY);
#endif
    HZ_DIAG_ROLE_GATE(role);
    if (role == 0)
      draw2_stage(blk, r2, (size_t)nrow, prep_mt, prep_tag, prep_pile, prep_cur, prep_rule, prep_ep, n, seed_base,
                  ahead_draws);
    else if (role == 1)
      draw1_stage(blk, r1, (size_t)nrow, prep_ep, n, seed_base, ahead_draws);
    else
      seed_stage(blk, rs, (size_t)nrow, prep_ep, n, seed_base);
#ifdef HZ_DIAG
    {  // role durations: slot 6 (draw2 blocks), 15 (draw1), 7 (seed), per board of the block
      int bb = blk * kBlock + (threadIdx.x & 63);
      if (g_stamps && threadIdx.x < 64 && bb < n)
        g_stamps[(size_t)bb * 16 + (role == 0 ? 6 : role == 1 ? 15 : 7)] = __builtin_amdgcn_s_memtime() - role_t0;
    }
#endif
    return;
  }
  HZ_DIAG_ROLE_GATE(3);
  __shared__ uint64_t s_lds_mask;
  int tid = threadIdx.x;
  int lane = tid & 63;
  bool w0 = __builtin_amdgcn_readfirstlane(tid) < 64;  // wave-uniform: wave 0 plays
  int b0 = blockIdx.x * kBlock;
  int b = b0 + lane;
  bool act = b < n;
  uint64_t actmask = __ballot(act);  // the same in every wave
  int nb = n - b0 < kBlock ? n - b0 : kBlock;
  uint32_t *g = mt + (size_t)b0 * kMT;
  // reset_first: a board whose episode was prepared ahead plays its pile
  // script; the others seed their stream in LDS below
  // the script words are read with the tag (one memory round trip); they
  // are used only when the tag matches
  uint64_t pq0 = 0, pq1 = 0, pq2 = 0, pq3 = 0;
  if (reset_first && act && ahead_pile && w0) {
    pq0 = ahead_pile[b];
    pq1 = ahead_pile[(size_t)n + b];
    pq2 = ahead_pile[(size_t)2 * n + b];
    pq3 = ahead_pile[(size_t)3 * n + b];
  }
  int ep0 = act ? episode[b] : 0;
  bool seeded = reset_first && act && ahead_tag && ahead_tag[b] == ep0;
  // the episode's rule hashes into rows [0, kRulePlies) of each seeded
  // lane's LDS column (a seeded lane replays its script and never keeps its
  // stream in LDS), all four waves, issued with the tag loads
  // (16-B loads: four boards of a row per thread; an unseeded lane's column
  // is overwritten by its seeding after the barrier)
  if (reset_first && ahead_rule) {
    constexpr int K = kRulePlies * 16 / kStageThreads;
    static_assert(kRulePlies * 16 % kStageThreads == 0, "hash rows per pass");
    uint4 hv[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
      int q = k * kStageThreads + tid;
      hv[k] = *reinterpret_cast<const uint4 *>(ahead_rule + (size_t)(q >> 4) * nrow + b0 + (q & 15) * 4);
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
      int q = k * kStageThreads + tid;
      uint32_t *d = hz_lds + (q >> 4) * kLdsStride + (q & 15) * 4;
      d[0] = hv[k].x;
      d[1] = hv[k].y;
      d[2] = hv[k].z;
      d[3] = hv[k].w;
    }
  }
  if (!reset_first) stage_mt(g, nb, tid, actmask, true);
  __syncthreads();
  if (w0 && act) HZ_ROLE_PHASE(13, role_t0, b);
  // a board replaying a prepared episode plays on to the end on the
  // prepared stream in ahead_mt (mt_src); it reaches the board's own mt
  // only if something else needs it (materialize)
  if (w0 && act) {
    PlayDraw draw{{0, 0, 0, 0, 0, ahead_draws}, LdsMT(lane, reset_first ? kMTSeeded : pos[b]), seeded, false,
                  MT(ahead_mt ? ahead_mt + (size_t)b * kMT : nullptr, 0),
                  ahead_cur ? ahead_cur + (size_t)ahead_draws * n + b : nullptr};
    if (seeded) {
      draw.q0 = pq0;
      draw.q1 = pq1;
      draw.q2 = pq2;
      draw.q3 = pq3;
    }
    State s;
    int g_ply, games = 0, steps = 0;
    uint64_t sd, rkey;
    // episode e begins: its seed and rule key, the board's counter past it
    auto begin_episode = [&](int e) {
      sd = episode_seed(seed_base, b, e);
      rkey = rule_key(sd);
      episode[b] = e + 1;
      g_ply = 0;
    };
    // where the lane's scripted stream lives: the play slot of a prepared
    // hz_play episode, or an auto-reset slot (set below when one is taken)
    const int32_t *cur_b = ahead_cur ? ahead_cur + b : nullptr;
    int src_b = src_slot;
    if (reset_first) {
      begin_episode(ep0);
      if (!seeded) mt_seed(hz_lds + lane, kLdsStride, sd);
      // HarmoniesGameState(), from the script when the whole wave has one
      if (__all(seeded) && ahead_draws >= 5) draw.scripted_reset(s);
      else reset_state(s, draw);
      HZ_ROLE_PHASE(8, role_t0, b);
    } else {
      s = load_state(st, n, b);
      g_ply = ply[b];
      sd = seed[b];
      rkey = rule_key(sd);
    }
#ifdef HZ_DIAG
    uint64_t t0 = __builtin_amdgcn_s_memtime();
    uint64_t acc8 = 0, acc9 = 0, acc10 = 0, acc11 = 0, acc12 = 0, acc13 = 0;
#endif
    bool lds_used = !seeded;  // the LDS copy of the stream is live
    bool pre = seeded && ahead_rule != nullptr;  // the episode's rule hashes are in LDS
    // Record: the ply's state, legal mask and rule move into trajectory row
    // `row`; returns the move (-1: none)
    [[maybe_unused]] auto record_ply = [&](int row) -> int {
      uint64_t mk[3];
      int L = legal_mask(s, mk);
      if constexpr (!AutoReset) HZ_ACC(9, t0);  // (the plain loop's phase clocks)
      if (traj_state) {
        uint64_t *o = traj_state + (size_t)row * 6 * n + b;
        o[0] = s.pl[0]; o[(size_t)n] = s.pl[1]; o[(size_t)2 * n] = s.pl[2]; o[(size_t)3 * n] = s.pl[3];
        o[(size_t)4 * n] = s.piles; o[(size_t)5 * n] = s.misc;
      }
      if (traj_mask) {
        uint64_t *o = traj_mask + ((size_t)row * n + b) * 3;
        o[0] = mk[0]; o[1] = mk[1]; o[2] = mk[2];
      }
      int a = L ? kth_action(mk, rule_pick_k(rkey, g_ply, L)) : -1;
      if (traj_action) traj_action[(size_t)row * n + b] = (int16_t)a;
      return a;
    };
    if constexpr (AutoReset) {
      // A board whose game ends starts its next episode: seeding its stream
      // is a 1,246-step chain (~60 k cycles) that the whole wave waits for.
      // Each lane counts its own plies (used), and a lane whose game ended
      // waits until no lane of the wave can play on; then every waiting lane
      // seeds together, in one pass, and play resumes.  Every board plays the
      // same plies in the same order as with a reset at its own ply (lanes
      // share nothing), so results are the same; the wave seeds once or
      // twice per launch instead of once per distinct game end.
      int used = 0;
      bool stuck = false;
      HZ_ROLES_ONLY(int n_pass = 0, n_iter = 0;)
      // the next episode seeded in the lane's LDS column, in place
      auto next_episode_in_lds = [&]() {
        if (score_pending(s.misc)) finish_game(s);  // the finished game is scored all the same
        begin_episode(episode[b]);
        mt_seed(hz_lds + lane, kLdsStride, sd);
        draw.m = LdsMT(lane, kMTSeeded);
        draw.scripted = false;
        lds_used = true;
        pre = false;
        reset_state(s, draw);
      };
      while (true) {
        if constexpr (!Record) {
          // a prepared episode (ar_prep_stage): a scripted reset at once, the
          // lane's own, with no seeding pass for the wave to wait for
          if (ar.on && phase_of(s.misc) == PH_OVER && !stuck && used < max_plies) {
            const int e = episode[b];
            const int sl = e & (kArSlots - 1);
            if (e - ep0 < 2 && ar.tag[(size_t)sl * n + b] == e) {
              if (score_pending(s.misc)) finish_game(s);  // the finished game is scored all the same
              const uint64_t *pq = ar.pile + (size_t)sl * kAheadWords * n + b;
              draw.q0 = pq[0];
              draw.q1 = pq[(size_t)n];
              draw.q2 = pq[(size_t)2 * n];
              draw.q3 = pq[(size_t)3 * n];
              draw.scripted = true;
              draw.fell = false;
              draw.d = 0;
              draw.nd = kAheadDraws;
              draw.gm = MT(ar.mt + ((size_t)sl * n + b) * kMT, 0);
              cur_b = ar.cur + (size_t)sl * (kAheadDraws + 1) * n + b;
              draw.cur_tail = cur_b + (size_t)kAheadDraws * n;
              src_b = kArSrc + sl;
              begin_episode(e);
              lds_used = false;
              pre = false;
              draw.scripted_reset(s);
            }
          }
        }
        const bool over = phase_of(s.misc) == PH_OVER;
        const bool can = !over && !stuck && used < max_plies;
        HZ_ROLES_ONLY(n_iter++;)
        if (!__any(can)) {
          const bool want = over && !stuck && used < max_plies;
          if (!__any(want)) break;
          HZ_ROLES_ONLY(n_pass++;)
          if (want) next_episode_in_lds();  // every waiting board's, seeded together
          continue;
        }
        if (!can) continue;
        if constexpr (!Record) {
          // a pair of whole turns at once while every playing board of the
          // wave is at a pair boundary with 8 plies of budget
          if (__all(used + 8 <= max_plies && turn_pair_safe(s))) {
            uint32_t h[8];
            if (__all(pre && g_ply + 8 <= kRulePlies)) {
#pragma unroll
              for (int j = 0; j < 8; j++) h[j] = hz_lds[(g_ply + j) * kLdsStride + lane];
            } else {
#pragma unroll
              for (int j = 0; j < 8; j++) h[j] = rule_h32(rkey, g_ply + j);
            }
            const int done = play_pair(s, draw, h);
            g_ply += done;
            steps += done;
            used += done;
            if (phase_of(s.misc) == PH_OVER) games++;
            continue;
          }
        }
        int a;
        if constexpr (Record) a = record_ply(used);
        else a = rule_action(s, rule_h32(rkey, g_ply));  // legal mask + rule pick, fused
        if (a < 0) {  // stuck board (unreachable from HarmoniesGameState())
          stuck = true;
          continue;
        }
        step_trusted<true>(s, a, draw);
        g_ply++;
        steps++;
        used++;
        if (phase_of(s.misc) == PH_OVER) games++;
      }
#ifdef HZ_DIAG_ROLES_ONLY
      if (g_stamps && lane == 0) {  // the wave's reseeding passes and loop iterations (tools/ar_passes.py)
        g_stamps[(size_t)b * 16 + 11] = n_pass;
        g_stamps[(size_t)b * 16 + 12] = n_iter;
      }
#endif
    } else {
      for (int i = 0; i < max_plies; i++) {
        if (phase_of(s.misc) == PH_OVER) {  // finished (scored, or scoring deferred)
          if (Record && traj_action) {
            for (int j = i; j < max_plies; j++) traj_action[(size_t)j * n + b] = -1;
          }
          break;
        }
        if constexpr (!Record) {
          // a pair of whole turns at once while every board of the wave still
          // playing is at a pair boundary (always, for boards reset together)
          if (__all(i + 8 <= max_plies && turn_pair_safe(s))) {
            uint32_t h[8];
            if (__all(pre && g_ply + 8 <= kRulePlies)) {
#pragma unroll
              for (int j = 0; j < 8; j++) h[j] = hz_lds[(g_ply + j) * kLdsStride + lane];
            } else {
#pragma unroll
              for (int j = 0; j < 8; j++) h[j] = rule_h32(rkey, g_ply + j);
            }
            const int done = play_pair(s, draw, h);
            g_ply += done;
            steps += done;
            i += done - 1;
            if (phase_of(s.misc) == PH_OVER) games++;
            continue;
          }
        }
        int a;
        HZ_ACC(8, t0);
        if constexpr (Record) {
          a = record_ply(i);
        } else {
          a = rule_action(s, rule_h32(rkey, g_ply));  // legal mask + rule pick, fused
          HZ_ACC(9, t0);
        }
        if (a < 0) break;  // stuck board (unreachable from HarmoniesGameState())
        HZ_ACC(10, t0);
        bool te = phase_of(s.misc) == PH_P3;
        step_trusted<true>(s, a, draw);
        if (te) HZ_ACC(12, t0);
        else HZ_ACC(11, t0);
        g_ply++;
        steps++;
        if (phase_of(s.misc) == PH_OVER) games++;
      }
    }
    HZ_ROLE_PHASE(9, role_t0, b);
    // final scoring of the games that ended in this call, the whole wave at once
    if (score_pending(s.misc)) finish_game(s);
    HZ_ROLE_PHASE(10, role_t0, b);
    HZ_ACC(13, t0);
    store_state(st, n, b, s);
    if (lds_used) pos[b] = draw.m.cursor();
    else if (draw.fell) pos[b] = draw.gm.cursor();
    else pos[b] = cur_b[(size_t)draw.d * n];
    mt_src[b] = lds_used ? -1 : src_b;
    win_tag[b] = -1;  // the board's saved draw window (PlyWin): none, its stream has moved
    ply[b] = g_ply;
    seed[b] = sd;
#if defined(HZ_DIAG) && !defined(HZ_DIAG_ROLES_ONLY)
    if (g_stamps) {
      uint64_t *o = g_stamps + (size_t)b * 16;
      o[8] = acc8; o[9] = acc9; o[10] = acc10; o[11] = acc11; o[12] = acc12; o[13] = acc13;
    }
#endif
    if (games_done) games_done[b] = games;
    if (steps_done) steps_done[b] = steps;
    if (ep_final) ep_final[b] = episode[b];
    uint64_t lm = __ballot(lds_used);
    if (lane == 0) s_lds_mask = lm;
  }
  if (w0 && !act && lane == 0 && actmask == 0) s_lds_mask = 0;
  __syncthreads();
  uint64_t lds_mask = s_lds_mask & actmask;
  if (lds_mask) stage_mt(g, nb, tid, lds_mask, false);
  if (threadIdx.x < 64 && act) HZ_PHASE(5, role_t0, b);  // the playing role's duration
}


}  // namespace
