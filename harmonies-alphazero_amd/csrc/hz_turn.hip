// hz_turn.hip — the turn of asynchronous self-play (SelfPlay.play_async): the
// boards whose search is spent record their result, play their move and begin
// their next search inside a sim step, while the other boards' trees, counters,
// budgets and noise rows stay untouched.  include/hz_abi.h states each entry
// point's rule.  A unit of its own: the search kernels' objects (hz_mcts.hip)
// are what they are without it.
#include "hz_mcts.hpp"

#include "../../include/hz_abi.h"

using namespace hz;
using namespace hz_host;
using namespace hz_tree;

struct hz_env;  // defined in hz_env.hip; accessed through the ABI getters

namespace {

constexpr int kThreads = 256;

// ------------------------------------------------------------ masked begin
// hz_mcts.hip's k_begin for the boards whose mask is 1 (the same stores in the
// same order: node 0, key, counts with a new generation, hash entry,
// sims_done = 0, the stuck-root budget 0); a board whose mask is 2 is stopped
// (k_begin's inactive board, and budget 0 under the gate); a board whose mask
// is 0 has nothing written.
__global__ void __launch_bounds__(kWave) k_begin_some(hz_mcts_args m, const uint64_t *__restrict__ game, int n_env,
                                                      const uint8_t *__restrict__ mask) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= m.n) return;
  const int mk = mask[b];
  if (mk == 0) return;
  int32_t *cnt = m.counts + (size_t)b * 4;
  m.sims_done[b] = 0;
  if (m.carry) m.carry[b] = 0;  // a fresh start drops the board's carry
  if (mk != 1) {
    m.leaf[b] = -1;
    m.leaf_gidx[b] = -1;
    cnt[0] = 0;
    cnt[1] = 0;
    if (m.budget) m.budget[b] = 0;
    return;
  }
  State s = load_state(game, n_env, b);
  if (m.budget && !game_done(s.misc)) {
    uint64_t lm[3];
    if (legal_mask(s, lm) == 0) m.budget[b] = 0;  // the stuck-root rule of hz_mcts_set_budget
  }
  const size_t nb = (size_t)b * m.max_nodes;
  store_node(m.node_state + nb * 6, s);
  CKey key = canon_key(s, !m.exact_keys);
  const uint64_t h = key_hash(key);
#pragma unroll
  for (int w = 0; w < 8; w++) m.node_key[nb * 8 + w] = key.w[w];
  m.node_e0[nb] = 0;
  m.node_ne[nb] = 0;
  const int gen = cnt[2] + 1;
  cnt[0] = 1;
  cnt[1] = 0;
  cnt[2] = gen;
  cnt[3] = 0;
  uint64_t *ht = m.ht + (size_t)b * m.hcap;
  ht[h & (uint64_t)(m.hcap - 1)] = ht_entry(gen, 0);
}

// ------------------------------------------------------ masked gate updates
__global__ void __launch_bounds__(kThreads) k_set_gate_some(hz_mcts_args m, const int32_t *__restrict__ budget,
                                                            const uint8_t *__restrict__ noise_bit,
                                                            const uint8_t *__restrict__ mask) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= m.n || mask[b] != 1) return;
  if (budget) m.budget_buf[b] = budget[b];
  if (noise_bit) m.mask_buf[b] = noise_bit[b] ? 1 : 0;
}

// ---------------------------------------------------------- the move choice
// hzamd.mcts.choose_actions for one board from its visits by action id (global
// memory or LDS): int64 cumulative counts; the sampled move is the first
// action whose cumulative count as fp64 exceeds the fp64 product u * total by
// '<' (action 0 when none does, as argmax over no hit gives); the greedy move
// the first action with the most visits; -1 without visits.
__device__ __forceinline__ int choose_from_visits(const int32_t *vis, bool explore, double u) {
  long long total = 0;
  int greedy = 0, most = vis[0];
  for (int a = 0; a < kActions; a++) {
    const int v = vis[a];
    total += (long long)v;
    if (v > most) {
      most = v;
      greedy = a;
    }
  }
  if (total <= 0) return -1;
  if (!explore) return greedy;
  const double target = __dmul_rn(u, (double)total);
  long long cum = 0;
  for (int a = 0; a < kActions; a++) {
    cum += (long long)vis[a];
    if (target < (double)cum) return a;
  }
  return 0;
}

__global__ void __launch_bounds__(kThreads) k_choose_actions(const int32_t *__restrict__ visits, int n,
                                                             const uint8_t *__restrict__ explore,
                                                             const double *__restrict__ u,
                                                             int16_t *__restrict__ action) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  action[b] = (int16_t)choose_from_visits(visits + (size_t)b * kActions, explore[b] != 0, u[b]);
}

// ------------------------------------------------- the turn: choose + record
// One wave per board.  A board turns iff it has moves left and its search is
// spent under the budget gate.  The root's visits by action id are built in
// LDS as hz_mcts_result builds them (an edge range or action outside the
// board's pools reads as no edge), lane 0 chooses, and the wave writes the
// record row at slot mc[b].
struct TurnRec {
  int64_t *states;   // [moves][6][n]
  int32_t *visits;   // [moves][n][143]
  int32_t *game;     // [moves][n]
  uint8_t *full;     // [moves][n], or nullptr
};

__global__ void __launch_bounds__(kWave) k_turn_choose(hz_mcts_args m, const uint64_t *__restrict__ st, int n_env,
                                                       const double *__restrict__ u, const int32_t *__restrict__ ply,
                                                       const int64_t *__restrict__ mc,
                                                       const int64_t *__restrict__ game, int64_t moves, int tau0,
                                                       int testing, int16_t *__restrict__ action,
                                                       uint8_t *__restrict__ turned, TurnRec rec) {
  __shared__ int32_t vis[kActions];
  __shared__ int pick;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t k = mc[b];
  const bool turn = k >= 0 && k < moves && m.sims_done[b] >= m.budget[b];
  if (!turn) {
    if (lane == 0) {
      action[b] = -1;
      turned[b] = 0;
    }
    return;
  }
  for (int a = lane; a < kActions; a += kWave) vis[a] = 0;
  __syncthreads();  // the zeros before the edges' entries (one wave: ordering only)
  const int32_t *cnt = m.counts + (size_t)b * 4;
  const int n_nodes = cnt[0], n_edges = cnt[1];
  int e0 = 0;
  const int ne = checked_counts(m, n_nodes, n_edges) ? checked_edges(m, (size_t)b * m.max_nodes, 0, n_edges, e0) : 0;
  const size_t eb = (size_t)b * m.max_edges + e0;
  for (int i = lane; i < ne; i += kWave) {
    const int a = m.edge_action[eb + i];
    if (a >= 0 && a < kActions) vis[a] = m.edge_n[eb + i];
  }
  __syncthreads();
  if (lane == 0) {
    const int a = choose_from_visits(vis, !testing && ply[b] < tau0, u[b]);
    pick = a;
    action[b] = (int16_t)a;
    turned[b] = 1;
    rec.game[(size_t)k * m.n + b] = (int32_t)game[b];
    if (rec.full) rec.full[(size_t)k * m.n + b] = m.noise_mask[b] ? 1 : 0;
  }
  if (lane < 6) rec.states[((size_t)k * 6 + lane) * m.n + b] = (int64_t)st[(size_t)lane * n_env + b];
  int32_t *row = rec.visits + ((size_t)k * m.n + b) * kActions;
  for (int a = lane; a < kActions; a += kWave) row[a] = vis[a];
}

// ------------------------------------------------------- the turn: after step
// Step (c) of a turn for the boards that turned, from the env's state after
// hz_step: the slot's ended / outcome / plies, the board's game, ply and move
// counters, the reset mask and seed of a board whose game ended, what the
// masked begin is to do with the board (1: begin, 2: stopped), a failed step,
// and the count of running boards.
struct TurnAfter {
  uint8_t *ended;    // [moves][n]
  float *outcome;    // [moves][n]
  int16_t *plies;    // [moves][n]
  uint8_t *sel;      // [n] hz_reset's mask
  uint64_t *seeds;   // [n] hz_reset's seeds
  uint8_t *begin;    // [n] hz_mcts_begin_some's mask (and the draws' and the gate updates')
  uint8_t *bad;      // [n] set where a turned board's step failed (never cleared here)
  int32_t *running;  // [1] boards with moves left
};

__global__ void __launch_bounds__(kThreads) k_turn_after(const uint64_t *__restrict__ st, int n,
                                                         const uint8_t *__restrict__ turned,
                                                         const int32_t *__restrict__ status, int64_t *__restrict__ mc,
                                                         int32_t *__restrict__ ply, int64_t *__restrict__ game,
                                                         int64_t moves, uint64_t seed_base, TurnAfter o) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  if (!turned[b]) {
    o.sel[b] = 0;
    o.begin[b] = 0;
    return;
  }
  const int64_t k = mc[b];
  const uint64_t misc = st[(size_t)5 * n + b];
  const bool over = game_done(misc);
  const int win = winner_code(misc);
  const size_t slot = (size_t)k * n + b;
  o.ended[slot] = over ? 1 : 0;
  o.outcome[slot] = over ? (win == 1 ? 1.0f : (win == 2 ? -1.0f : 0.0f)) : 0.0f;
  const int p = ply[b] + 1;
  o.plies[slot] = (int16_t)p;
  const int64_t g = game[b] + (over ? 1 : 0);
  game[b] = g;
  ply[b] = over ? 0 : p;
  mc[b] = k + 1;
  o.sel[b] = over ? 1 : 0;
  o.seeds[b] = seed_base + (uint64_t)b + ((uint64_t)g << 32);
  const bool more = k + 1 < moves;
  o.begin[b] = more ? 1 : 2;
  if (!more) atomicSub(o.running, 1);
  if (status[b] != 0) o.bad[b] = 1;
}

}  // namespace

extern "C" {

int hz_mcts_begin_some(hz_mcts *m, hz_env *env, const uint8_t *mask) {
  if (!m || !env || !mask || hz_env_size(env) != m->n) return -1;
  hipLaunchKernelGGL(k_begin_some, dim3((m->n + kWave - 1) / kWave), dim3(kWave), 0, m->stream, *m,
                     hz_env_state_ptr(env), m->n, mask);
  return launch_err();
}

int hz_mcts_set_gate_some(hz_mcts *m, const int32_t *budget, const uint8_t *noise_bit, const uint8_t *mask) {
  if (!m || !mask || (budget && !m->budget) || (noise_bit && !m->noise_mask)) return -1;
  if (!budget && !noise_bit) return 0;
  hipLaunchKernelGGL(k_set_gate_some, dim3((m->n + kThreads - 1) / kThreads), dim3(kThreads), 0, m->stream, *m,
                     budget, noise_bit, mask);
  return launch_err();
}

int hz_choose_actions(const int32_t *visits, int32_t n, const uint8_t *explore, const double *u, int16_t *action,
                      void *stream) {
  if (n < 0 || !visits || !explore || !u || !action) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_choose_actions, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream,
                     visits, n, explore, u, action);
  return launch_err();
}

int hz_turn_choose(hz_mcts *m, hz_env *env, const double *u, const int32_t *ply, const int64_t *mc,
                   const int64_t *game, int64_t moves, int32_t turns_until_tau0, int32_t testing, int16_t *action,
                   uint8_t *turned, int64_t *rec_states, int32_t *rec_visits, int32_t *rec_game, uint8_t *rec_full) {
  if (!m || !env || hz_env_size(env) != m->n || !u || !ply || !mc || !game || moves < 0 || !action || !turned ||
      !rec_states || !rec_visits || !rec_game)
    return -1;
  if (!m->budget || (rec_full && !m->noise_mask)) return -1;  // a turn is defined under the budget gate only
  const TurnRec rec{rec_states, rec_visits, rec_game, rec_full};
  hipLaunchKernelGGL(k_turn_choose, dim3(m->n), dim3(kWave), 0, m->stream, *m, hz_env_state_ptr(env), m->n, u, ply, mc,
                     game, moves, turns_until_tau0, testing, action, turned, rec);
  return launch_err();
}

int hz_turn_after(hz_env *env, const uint8_t *turned, const int32_t *status, int64_t *mc, int32_t *ply, int64_t *game,
                  int64_t moves, uint64_t seed_base, uint8_t *rec_ended, float *rec_outcome, int16_t *rec_plies,
                  uint8_t *sel, uint64_t *seeds, uint8_t *begin, uint8_t *bad, int32_t *running, void *stream) {
  if (!env || !turned || !status || !mc || !ply || !game || moves < 0 || !rec_ended || !rec_outcome || !rec_plies ||
      !sel || !seeds || !begin || !bad || !running)
    return -1;
  const int n = hz_env_size(env);
  if (n <= 0) return -1;
  const TurnAfter o{rec_ended, rec_outcome, rec_plies, sel, seeds, begin, bad, running};
  hipLaunchKernelGGL(k_turn_after, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream,
                     hz_env_state_ptr(env), n, turned, status, mc, ply, game, moves, seed_base, o);
  return launch_err();
}

}  // extern "C"
