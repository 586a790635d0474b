// hz_mcts_carry.hip — tree reuse: between two searches a board keeps the
// subtree below the move just played (hz_mcts_advance) and starts its next
// search from it (hz_mcts_begin_carried).
#include "hz_mcts.hpp"

#include "../../include/hz_abi.h"

using namespace hz;
using namespace hz_host;
using namespace hz_tree;

struct hz_env;  // defined in hz_env.hip; accessed through the ABI getters

namespace {

// -------------------------------------------------------------- tree reuse
// hz_mcts_advance / hz_mcts_begin_carried (no reference counterpart: MCTS.py:288
// builds a fresh Node per call; the rule is stated in include/hz_abi.h).  Both
// run between searches, one wave per board, and trust nothing they read from
// the tree: edge ranges and child links are checked against the board's counts
// before use, so every index stays inside the board's slices.
// The wave reads words other lanes of it wrote earlier in the launch.  What
// that rests on: (a) wave_mem_sync() between the phases is a compiler-level
// ordering (no load or store moves across it) and a wave barrier; it is not a
// wait for the stores to complete; (b) every such read-after-write is by the
// same wave, whose requests to one address reach memory in issue order;
// (c) the reads are ld_l2 loads, which go past the CU's L1, so no stale line
// is hit.  A plain load of a word written earlier in the launch must not be
// put behind one of these syncs.  Loads-before-stores within a chunk (a
// lane's destination may be another lane's source) holds by data dependence:
// the stores' values come from the chunk's load instructions, which the wave
// waits for as a whole.
template <class T>
__device__ __forceinline__ T ld_l2(const T *p) {
  return __hip_atomic_load(const_cast<T *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void wave_mem_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ bool state_eq(const uint64_t *ns, const State &s) {
  return ns[0] == s.pl[0] && ns[1] == s.pl[1] && ns[2] == s.pl[2] && ns[3] == s.pl[3] && ns[4] == s.piles &&
         ns[5] == s.misc;
}

// After hz_step applied action[b]: the tree becomes the sub-DAG reachable
// from the played child c (carried), or nothing (dropped).  Steps, each over
// the board's old pools with the wave's lanes as nodes or edges:
//   1. the carry conditions that need no traversal (wave-uniform);
//   2. reach marks from c: the kept expanded nodes form a queue, each node's
//      edges are the lanes; a child is claimed once (atomic exchange on its
//      mark), kept edges are flagged in edge_hint (rebuilt in step 7);
//   3. headroom; then new node ids: c -> 0, the others 1.. in ascending old id;
//   4. edges packed in pool order, in place, ascending (destination <= source;
//      a chunk's loads complete before its stores), children renumbered; the
//      old position keeps the edge's new index (a kept node's new e0);
//   5. nodes moved in place the same way, c first;
//   6. the generation bumped and every kept node entered into the hash table;
//   7. hints rebuilt from the moved nodes; counts, info and the carry flag.
__global__ void __launch_bounds__(kWave) k_advance(hz_mcts_args m, const uint64_t *__restrict__ game, int n_env,
                                                   const int16_t *__restrict__ action,
                                                   const uint8_t *__restrict__ active, int headroom,
                                                   int32_t *__restrict__ info) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int32_t *cnt = m.counts + (size_t)b * 4;
  const size_t nb = (size_t)b * m.max_nodes, eb = (size_t)b * m.max_edges;
  const int nn = cnt[0], nE = cnt[1];
  const int a = action[b];
  const uint64_t below = (1ull << lane) - 1;
  int32_t *mark = m.adv_remap + nb, *queue = m.adv_queue + nb;
  int32_t *hint = m.edge_hint + eb;
  bool ok = (!active || active[b]) && a >= 0 && a < kActions && checked_counts(m, nn, nE);
  int c = -1;
  if (ok) {  // the root's edge for the action, its child
    int e0 = 0;
    const int ne = checked_edges(m, nb, 0, nE, e0);
    const bool hit0 = lane < ne && m.edge_action[eb + e0 + lane] == a;
    const bool hit1 = lane + kWave < ne && m.edge_action[eb + e0 + lane + kWave] == a;
    const uint64_t b0 = __ballot(hit0), b1 = __ballot(hit1);
    const int ei = b0 ? __builtin_ctzll(b0) : b1 ? kWave + __builtin_ctzll(b1) : -1;
    if (ei >= 0) c = m.edge_child[eb + e0 + ei];
    ok = ei >= 0 && c > 0 && c < nn;
  }
  if (ok) {  // not terminal, and the state the env now holds
    const uint64_t *cs = m.node_state + (nb + c) * 6;
    ok = m.node_ne[nb + c] >= 0 && !game_done(cs[5]) && state_eq(cs, load_state(game, n_env, b));
  }
  int kn = 0, ke = 0;
  if (ok) {
    for (int i = lane; i < nn; i += kWave) mark[i] = 0;
    for (int e = lane; e < nE; e += kWave) hint[e] = 0;
    int ce0 = 0;
    const int cne = checked_edges(m, nb, c, nE, ce0);
    wave_mem_sync();
    if (lane == 0) {
      mark[c] = 1;
      queue[0] = c;
    }
    wave_mem_sync();
    kn = 1;
    ke = cne;
    int qh = 0, qt = cne > 0 ? 1 : 0;  // (every claimed node enters the queue at most once: qt <= nn)
    while (qh < qt) {
      const int batch = qt - qh < kWave ? qt - qh : kWave;
      int ve0 = 0, vne = 0;
      if (lane < batch) vne = checked_edges(m, nb, ld_l2(&queue[qh + lane]), nE, ve0);
      for (int j = 0; j < batch; j++) {
        const int e0 = __shfl(ve0, j), ne = __shfl(vne, j);
#pragma unroll
        for (int r = 0; r < 2; r++) {
          const int k = lane + r * kWave;
          bool fresh = false;
          int ch = 0, chne = 0, che0 = 0;
          if (k < ne) {
            hint[e0 + k] = 1;
            ch = m.edge_child[eb + e0 + k];
            if (ch > 0 && ch < nn) fresh = atomicExch(&mark[ch], 1) == 0;
          }
          if (fresh) chne = checked_edges(m, nb, ch, nE, che0);
          const bool grow = fresh && chne > 0;
          const uint64_t fb = __ballot(fresh), gb = __ballot(grow);
          if (grow) queue[qt + __popcll(gb & below)] = ch;
          kn += __popcll(fb);
          qt += __popcll(gb);
          ke += wave_sum_i(grow ? chne : 0);
        }
      }
      qh += batch;
      wave_mem_sync();  // the queue's new entries, before the next batch reads them
    }
    ok = (long long)kn + headroom <= m.max_nodes && (long long)ke + headroom <= m.max_edges;
  }
  if (!ok) {  // dropped (a tree marked above is gone with its counts)
    if (lane == 0) {
      m.carry[b] = 0;
      cnt[0] = 0;
      cnt[1] = 0;
      info[(size_t)b * 3] = 0;
      info[(size_t)b * 3 + 1] = 0;
      info[(size_t)b * 3 + 2] = 0;
    }
    return;
  }
  {  // 3. new ids
    int base = 1;
    for (int i0 = 0; i0 < nn; i0 += kWave) {
      const int i = i0 + lane;
      const bool kept = i < nn && i != c && ld_l2(&mark[i]) != 0;
      const uint64_t kb = __ballot(kept);
      if (i < nn) mark[i] = kept ? base + __popcll(kb & below) : (i == c ? 0 : -1);
      base += __popcll(kb);
    }
  }
  wave_mem_sync();
  {  // 4. edges
    int ebase = 0;
    for (int c0 = 0; c0 < nE; c0 += kWave) {
      const int e = c0 + lane;
      const bool kept = e < nE && ld_l2(&hint[e]) == 1;
      const uint64_t kb = __ballot(kept);
      const int dst = ebase + __popcll(kb & below);  // <= e
      int16_t ea = 0;
      int ech = 0, en = 0;
      double ew = 0.0;
      float ep = 0.f;
      uint8_t epl = 0;
      if (kept) {
        ea = m.edge_action[eb + e];
        ech = m.edge_child[eb + e];
        en = m.edge_n[eb + e];
        ew = m.edge_w[eb + e];
        ep = m.edge_p[eb + e];
        epl = m.edge_player[eb + e];
        ech = ech > 0 && ech < nn ? ld_l2(&mark[ech]) : 0;
      }
      wave_mem_sync();  // the chunk's loads before its stores (a lane's destination may be another's source)
      if (kept) {
        m.edge_action[eb + dst] = ea;
        m.edge_child[eb + dst] = ech;
        m.edge_n[eb + dst] = en;
        m.edge_w[eb + dst] = ew;
        m.edge_p[eb + dst] = ep;
        m.edge_player[eb + dst] = epl;
        hint[e] = dst;
      }
      ebase += __popcll(kb);
    }
  }
  wave_mem_sync();
  // a kept expanded node's new first edge: its old first edge's new index
  auto new_e0 = [&](int ne, int e0) { return ne > 0 && e0 >= 0 && e0 < nE ? ld_l2(&hint[e0]) : 0; };
  {  // 5. nodes: c first (slot 0 held the old root, which no kept node is)
    uint64_t wv = 0;
    if (lane < 6) wv = m.node_state[(nb + c) * 6 + lane];
    else if (lane < 14) wv = m.node_key[(nb + c) * 8 + lane - 6];
    const int cne = m.node_ne[nb + c], ce0 = new_e0(cne, m.node_e0[nb + c]);
    wave_mem_sync();
    if (lane < 6) m.node_state[nb * 6 + lane] = wv;
    else if (lane < 14) m.node_key[nb * 8 + lane - 6] = wv;
    if (lane == 0) {
      m.node_ne[nb] = cne;
      m.node_e0[nb] = ce0;
    }
    wave_mem_sync();
    for (int i0 = 0; i0 < nn; i0 += kWave) {
      const int i = i0 + lane;
      const int dst = i < nn ? ld_l2(&mark[i]) : -1;  // 1 <= dst <= i for a kept node
      uint64_t st[6], ky[8];
      int ne = 0, e0 = 0;
      if (dst > 0) {
#pragma unroll
        for (int w = 0; w < 6; w++) st[w] = ld_l2(&m.node_state[(nb + i) * 6 + w]);
#pragma unroll
        for (int w = 0; w < 8; w++) ky[w] = ld_l2(&m.node_key[(nb + i) * 8 + w]);
        ne = ld_l2(&m.node_ne[nb + i]);
        e0 = new_e0(ne, ld_l2(&m.node_e0[nb + i]));
      }
      wave_mem_sync();
      if (dst > 0) {
#pragma unroll
        for (int w = 0; w < 6; w++) m.node_state[(nb + dst) * 6 + w] = st[w];
#pragma unroll
        for (int w = 0; w < 8; w++) m.node_key[(nb + dst) * 8 + w] = ky[w];
        m.node_ne[nb + dst] = ne;
        m.node_e0[nb + dst] = e0;
      }
    }
  }
  wave_mem_sync();
  const int gen = cnt[2] + 1;
  {  // 6. the hash table of the new generation (hcap >= 2 max_nodes: a free slot is always found)
    uint64_t *ht = m.ht + (size_t)b * m.hcap;
    const uint64_t hmask = (uint64_t)(m.hcap - 1);
    for (int i = lane; i < kn; i += kWave) {
      CKey k;
#pragma unroll
      for (int w = 0; w < 8; w++) k.w[w] = ld_l2(&m.node_key[(nb + i) * 8 + w]);
      uint64_t slot = key_hash(k) & hmask;
      unsigned long long old = ld_l2(&ht[slot]);
      for (;;) {
        while ((int)(old >> 32) == gen) {
          slot = (slot + 1) & hmask;
          old = ld_l2(&ht[slot]);
        }
        const unsigned long long prev =
            atomicCAS((unsigned long long *)&ht[slot], old, (unsigned long long)ht_entry(gen, i));
        if (prev == old) break;
        old = prev;
      }
    }
  }
  // 7. hints from the moved nodes, the new root's visits
  for (int e = lane; e < ke; e += kWave) {
    const int ch = ld_l2(&m.edge_child[eb + e]);
    int cne = 0, ce0 = 0;
    if (ch >= 0 && ch < kn) {
      cne = ld_l2(&m.node_ne[nb + ch]);
      ce0 = ld_l2(&m.node_e0[nb + ch]);
    }
    hint[e] = edge_hint_of(cne > 0 ? ce0 : 0, cne > 0 ? cne : 0, cne < 0);
  }
  int rn = 0;
  {
    const int rne = ld_l2(&m.node_ne[nb]), re0 = ld_l2(&m.node_e0[nb]);
    if (rne > 0 && rne <= kChildSlots && re0 >= 0 && re0 <= ke - rne)
      for (int k = lane; k < rne; k += kWave) rn += ld_l2(&m.edge_n[eb + re0 + k]);
    rn = wave_sum_i(rn);
  }
  if (lane == 0) {
    cnt[0] = kn;
    cnt[1] = ke;
    cnt[2] = gen;
    cnt[3] = 0;
    m.carry[b] = 1;
    info[(size_t)b * 3] = kn;
    info[(size_t)b * 3 + 1] = ke;
    info[(size_t)b * 3 + 2] = rn;
  }
}

// hz_mcts_begin for a handle that advanced: a board whose carry flag is set
// and whose node 0 still is the env's state keeps its tree (limit flag and
// simulation count cleared; a noisy board's expanded root gets the root mix,
// with the expansion's arithmetic); every other active board starts as k_begin
// starts it.  The flag is consumed.  One wave per board; lanes are root edges.
__global__ void __launch_bounds__(kWave) k_begin_carried(hz_mcts_args m, const uint64_t *__restrict__ game, int n_env,
                                                         const uint8_t *__restrict__ active,
                                                         const double *__restrict__ noise, double eps,
                                                         float one_minus_eps, int testing) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int32_t *cnt = m.counts + (size_t)b * 4;
  const size_t nb = (size_t)b * m.max_nodes, eb = (size_t)b * m.max_edges;
  const bool act = !active || active[b];
  const bool flagged = m.carry[b] != 0;
  const int nn = cnt[0], nE = cnt[1];
  wave_mem_sync();  // every lane has read the flag
  if (lane == 0) {
    m.sims_done[b] = 0;
    m.carry[b] = 0;
  }
  if (!act) {
    if (lane == 0) {
      m.leaf[b] = -1;
      m.leaf_gidx[b] = -1;
      cnt[0] = 0;
      cnt[1] = 0;
    }
    return;
  }
  const State s = load_state(game, n_env, b);
  uint64_t mk[3];
  const int nl = legal_mask(s, mk);
  if (m.budget && !game_done(s.misc) && nl == 0 && lane == 0) m.budget[b] = 0;  // a stuck root (k_begin)
  const bool keep = flagged && checked_counts(m, nn, nE) && state_eq(m.node_state + nb * 6, s);
  if (!keep) {
    if (lane == 0) {  // k_begin's fresh tree
      store_node(m.node_state + nb * 6, s);
      const CKey key = canon_key(s, !m.exact_keys);
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
    return;
  }
  if (lane == 0) cnt[3] = 0;
  const bool noisy = !testing && noise && (!m.noise_mask || m.noise_mask[b]);
  int e0 = 0;
  const int ne = checked_edges(m, nb, 0, nE, e0);
  if (!noisy || ne == 0) return;  // (an unexpanded root is mixed where the first simulation expands it)
  for (int k = lane; k < ne; k += kWave) {
    const int a = m.edge_action[eb + e0 + k];
    if (a < 0 || a >= kActions) continue;
    // the action's rank among the root's legal moves (not the edge index: a skipped self-loop child shifts it)
    int i = 0;
#pragma unroll
    for (int w = 0; w < 3; w++) {
      const uint64_t bits = w < (a >> 6) ? mk[w] : (w == (a >> 6) ? mk[w] & ((1ull << (a & 63)) - 1) : 0ull);
      i += __popcll(bits);
    }
    if (i >= kMaxChildren) continue;
    const float p = m.edge_p[eb + e0 + k];
    m.edge_p[eb + e0 + k] = __double2float_rn(
        __dadd_rn((double)__fmul_rn(one_minus_eps, p), __dmul_rn(eps, noise[(size_t)b * kMaxChildren + i])));
  }
}

}  // namespace

extern "C" {

int hz_mcts_advance(hz_mcts *m, hz_env *env, const int16_t *action, const uint8_t *active, int32_t headroom,
                    int32_t *info) {
  if (!m || !env || !action || !info || headroom < 0 || hz_env_size(env) != m->n) return -1;
  if (!m->carry && !request_carry(m->carry_bufs, *m)) {  // first use
    m->carry_bufs.release();
    return 1;
  }
  hipLaunchKernelGGL(k_advance, dim3(m->n), dim3(kWave), 0, m->stream, *m, hz_env_state_ptr(env), m->n, action,
                     active, headroom, info);
  return launch_err();
}

int hz_mcts_begin_carried(hz_mcts *m, hz_env *env, const uint8_t *active, const double *noise, double eps,
                          int32_t testing) {
  if (!m || !env || hz_env_size(env) != m->n) return -1;
  if (m->forced_k > 0.0) return -1;  // (forced playouts start from an empty tree: hz_mcts_set_forced)
  if (!m->carry) return hz_mcts_begin(m, env, active);  // never advanced: nothing to carry
  hipLaunchKernelGGL(k_begin_carried, dim3(m->n), dim3(kWave), 0, m->stream, *m, hz_env_state_ptr(env), m->n, active,
                     noise, eps, (float)(1.0 - eps), testing);
  return launch_err();
}

}  // extern "C"
