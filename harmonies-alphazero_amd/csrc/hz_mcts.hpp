// hz_mcts.hpp — what the units of the tree search share (hz_mcts.hip: the
// simulation; hz_mcts_report.hip: views of a finished tree; hz_mcts_carry.hip:
// tree reuse): the kernels' argument struct, the handle, the request lists of
// the handle's device buffers, the picker of a launch's kernel instantiation,
// and the device helpers more than one unit uses.
//
// Everything above the HIP section compiles with a plain C++17 compiler
// (tests/host_driver.cpp runs the request lists and the picker under ASan + UBSan without a GPU).
#pragma once

#include <cstddef>
#include <cstdint>

typedef struct ihipStream_t *hipStream_t;  // (as <hip/hip_runtime.h> declares it)

// What every tree kernel receives, by value.  The device pointers are owned by
// the handle's buffer groups below; the host-only fields ride along.
struct hz_mcts_args {
  int32_t n, max_nodes, max_edges, hcap, max_depth;
  int32_t exact_keys;
  int32_t dedup_walk;    // hz_mcts_set_dedup_walk (tests): every sibling dedup takes the serial walk
  int32_t gather_mode;   // hz_mcts_set_gather_encode: 0 layered, 1 or -1 (the default) fused
  hipStream_t stream;
  uint64_t *node_state;  // [n][max_nodes][6]
  uint64_t *node_key;    // [n][max_nodes][8] canonical key (a probe compares it whole: no key rebuilt)
  int32_t *node_e0;      // [n][max_nodes]
  int32_t *node_ne;      // [n][max_nodes]
  int16_t *edge_action;  // [n][max_edges]
  int32_t *edge_child;   // [n][max_edges]
  int32_t *edge_n;       // [n][max_edges]
  double *edge_w;        // [n][max_edges]
  float *edge_p;         // [n][max_edges]
  uint8_t *edge_player;  // [n][max_edges]
  // [n][max_edges] the child node's e0 << 8 | terminal << 7 | ne as far as
  // known: ne = 0 means "not expanded when last seen" (select then reads the
  // node itself and repairs the hint), so the walk takes one memory round
  // trip per level (edges + hints) instead of two (node, then its edges)
  int32_t *edge_hint;
  uint64_t *ht;          // [n][hcap]
  int32_t *counts;       // [n][4]: nodes, edges, generation, overflow
  int32_t *path;         // [n][max_depth]
  int32_t *depth;        // [n]
  int32_t *leaf;         // [n]  leaf node of the current simulation, -1 = inactive
  int32_t *leaf_gidx;    // [n]  b*max_nodes + leaf for the encoder, -1 = no eval
  int32_t *slot;         // [n]  row of board b in the gathered leaf batch, -1 = not evaluated
  int32_t *gidx_c;       // [n]  leaf_gidx of the gathered rows, in board order
  int64_t *eval_ctr;     // optional (hz_mcts_set_eval_counter): k_gather adds each simulation's row count
  // rows of the policy / value tensors of the next expand call (hz_mcts_set_row_cap; 0: unchecked): a board whose
  // row is at or past it reads neither, expands and backs up nothing and sets err[0]
  int32_t row_cap;
  int32_t *err;          // [1] device error word (hz_mcts_take_error): bit 0 = a row at or past row_cap
  // per-board simulation budgets (hz_mcts_set_budget): budget == nullptr: no gate; else budget == budget_buf
  int32_t *budget;       // [n] the gate's budgets (the handle's copy), or nullptr
  int32_t *sims_done;    // [n] simulations select_board has given board b in this search (counted under the gate only)
  int32_t *budget_buf;   // [n] owned; fixed address, so a captured simulation stays valid while its contents change
  // per-board root noise (hz_mcts_set_root_noise_mask): nullptr: every board, else noise_mask == mask_buf
  uint8_t *noise_mask;
  uint8_t *mask_buf;     // [n] owned
  // tree reuse (hz_mcts_advance; allocated by its first call, nullptr on a handle that never advanced)
  uint8_t *carry;        // [n] board b's tree is the subtree hz_mcts_advance kept (consumed by the next begin)
  int32_t *adv_remap;    // [n][max_nodes] advance's scratch: reach marks, then old node id -> new id (-1: dropped)
  int32_t *adv_queue;    // [n][max_nodes] advance's scratch: the kept expanded nodes, in discovery order
  // the Gumbel root (hz_mcts_set_gumbel; allocated by its first call): gumbel == nullptr: gate off, else == gumbel_buf
  double *gumbel;        // [n][69] G by legal rank (the handle's copy), or nullptr
  double *gumbel_buf;    // [n][69] owned; fixed address (a captured simulation stays valid while its contents change)
  double *g_score;       // [n][69] G + log P by root edge index, written where node 0's edges are
  float *root_value;     // [n] the network's value of node 0, written where node 0 is expanded
  // [g_considered + 1][g_nroot] considered-visit table: owned, allocated once for the largest table the ABI
  // admits (70 x 32767 int16, 4.6 MB), so its address is fixed for the handle's life like the others'
  int16_t *g_table;
  int32_t g_considered, g_nroot;
  double g_c_visit, g_c_scale;
  // leaf symmetries (hz_mcts_set_leaf_symmetry; allocated by its first call): leaf_key == nullptr: gate off, else == leaf_key_buf
  uint64_t *leaf_key;      // [n] the boards' keys (the handle's copy), or nullptr
  uint64_t *leaf_key_buf;  // [n] owned; fixed address (a captured simulation stays valid while its contents change)
  uint8_t *leaf_g;         // [n] by board: the g of leaf_gidx's leaves, for the per-board encoder (hz_mcts_encode_leaves)
  uint8_t *row_g;          // [n] by gathered row, beside gidx_c: the g of k_gather's rows, for the layered encoder
  // forced playouts at the root (hz_mcts_set_forced; allocated by its first call): forced_k == 0: gate off
  double forced_k;         // KataGo's k; a captured simulation holds it by value
  uint8_t *forced_mask;    // nullptr: every board, else == forced_buf
  uint8_t *forced_buf;     // [n] owned; fixed address (a captured simulation stays valid while its contents change)
  int32_t *forced_cnt;     // [n][2] this search's root selections under the gate, and those the forced rule decided
};

namespace hz_tree {

constexpr int kWave = 64;
constexpr int kMaxChildren = 69;  // measured max legal moves
constexpr int kChildSlots = 128;  // two per lane (loop bound: lanes c and c + 64)
constexpr int32_t kGumbelTableMax = (kMaxChildren + 1) * 32767;  // entries of the largest table hz_mcts_set_gumbel admits

// ------------------------------------------------------ the handle's buffers
// The five groups of a handle's device buffers, each requested whole from its
// own owner (hz_host.hpp's DevBufsT) and freed by that owner's release(): a
// request after a failed one does nothing, so each list ends in one check.  A
// buffer's address is fixed while its group lives (captured simulations bake
// addresses in).  Only the buffers named here are filled: the node and edge
// pools are gigabytes.  a.n, max_nodes, max_edges, hcap and max_depth are set.
// The base group (hz_mcts_create): synchronous fills.
template <class Bufs>
bool request_base(Bufs &o, hz_mcts_args &a) {
  const size_t n = (size_t)a.n, N = n * a.max_nodes, E = n * a.max_edges;
  o.get(a.node_state, N * 6 * sizeof(uint64_t));
  o.get(a.node_key, N * 8 * sizeof(uint64_t));
  o.get(a.node_e0, N * sizeof(int32_t));
  o.get(a.node_ne, N * sizeof(int32_t));
  o.get(a.edge_action, E * sizeof(int16_t));
  o.get(a.edge_child, E * sizeof(int32_t));
  o.get(a.edge_n, E * sizeof(int32_t));
  o.get(a.edge_w, E * sizeof(double));
  o.get(a.edge_p, E * sizeof(float));
  o.get(a.edge_player, E * sizeof(uint8_t));
  o.get(a.edge_hint, E * sizeof(int32_t));
  o.get(a.ht, n * a.hcap * sizeof(uint64_t), 0);
  o.get(a.counts, n * 4 * sizeof(int32_t), 0);
  o.get(a.path, n * a.max_depth * sizeof(int32_t));
  o.get(a.depth, n * sizeof(int32_t), 0);
  o.get(a.leaf, n * sizeof(int32_t), 0xff);
  o.get(a.leaf_gidx, n * sizeof(int32_t), 0xff);
  o.get(a.slot, n * sizeof(int32_t));
  o.get(a.gidx_c, n * sizeof(int32_t));
  o.get(a.err, sizeof(int32_t), 0);
  o.get(a.sims_done, n * sizeof(int32_t), 0);
  o.get(a.budget_buf, n * sizeof(int32_t), 0);
  o.get(a.mask_buf, n * sizeof(uint8_t), 0);
  return o.ok;
}
// Tree reuse (the first hz_mcts_advance): the flags, cleared on the handle's
// stream, and advance's scratch (never a second node pool).
template <class Bufs>
bool request_carry(Bufs &o, hz_mcts_args &a) {
  const size_t n = (size_t)a.n, N = n * a.max_nodes;
  o.get(a.carry, n * sizeof(uint8_t), 0, (void *)a.stream);
  o.get(a.adv_remap, N * sizeof(int32_t));
  o.get(a.adv_queue, N * sizeof(int32_t));
  return o.ok;
}
// The Gumbel root (the first hz_mcts_set_gumbel): every buffer at its final
// size, the table for the largest the ABI admits.
template <class Bufs>
bool request_gumbel(Bufs &o, hz_mcts_args &a) {
  const size_t n = (size_t)a.n;
  o.get(a.gumbel_buf, n * kMaxChildren * sizeof(double));
  o.get(a.g_score, n * kMaxChildren * sizeof(double), 0, (void *)a.stream);
  o.get(a.root_value, n * sizeof(float), 0, (void *)a.stream);
  o.get(a.g_table, (size_t)kGumbelTableMax * sizeof(int16_t));
  return o.ok;
}
// Leaf symmetries (the first hz_mcts_set_leaf_symmetry): the keys and the two
// byte arrays the layered encoders read, cleared on the handle's stream.
template <class Bufs>
bool request_leaf_sym(Bufs &o, hz_mcts_args &a) {
  const size_t n = (size_t)a.n;
  o.get(a.leaf_key_buf, n * sizeof(uint64_t));
  o.get(a.leaf_g, n * sizeof(uint8_t), 0, (void *)a.stream);
  o.get(a.row_g, n * sizeof(uint8_t), 0, (void *)a.stream);
  return o.ok;
}

// Forced playouts (the first hz_mcts_set_forced): the mask and the per-board
// counters, cleared on the handle's stream.
template <class Bufs>
bool request_forced(Bufs &o, hz_mcts_args &a) {
  const size_t n = (size_t)a.n;
  o.get(a.forced_buf, n * sizeof(uint8_t), 0, (void *)a.stream);
  o.get(a.forced_cnt, n * 2 * sizeof(int32_t), 0, (void *)a.stream);
  return o.ok;
}

// ------------------------------------------------------------ the launch form
// The root forms of the walk (select_board's template argument): PUCT, the
// Gumbel root, or PUCT behind the forced-playout rule of hz_mcts_set_forced.
constexpr int kRootPuct = 0, kRootGumbel = 1, kRootForced = 2;
// Which instantiation of a tree kernel a launch takes: the walk's root form
// and whether the leaf-symmetry code is in (with a gate off the kernels carry
// none of its code); root -1: the gates' combination has no instantiation.
struct LaunchForm {
  int root;
  bool sym;
};
// From the handle's gates (gumbel != nullptr, forced_k > 0, leaf_key !=
// nullptr) and whether the launch walks (has a select).  One root form per
// search, so the Gumbel root with forced playouts is refused; the symmetric
// instantiations exist without the Gumbel root only; the forced rule lives in
// the walk, so a launch without one never takes the forced form.
inline LaunchForm pick_form(bool gumbel, bool forced, bool leaf_key, bool walk) {
  if (gumbel && (leaf_key || forced)) return {-1, false};
  if (gumbel) return {kRootGumbel, false};
  return {forced && walk ? kRootForced : kRootPuct, leaf_key};
}
inline LaunchForm pick_form(const hz_mcts_args &a, bool walk) {
  return pick_form(a.gumbel != nullptr, a.forced_k > 0.0, a.leaf_key != nullptr, walk);
}
// launch(FormOf<Root, Sym>{}) for the picked form, so a generic lambda names
// the kernel by decltype(f)::root and ::sym.  Only what pick_form can return
// is instantiated: no symmetric Gumbel form, the forced forms only with Walk.
template <int Root, bool Sym>
struct FormOf {
  static constexpr int root = Root;
  static constexpr bool sym = Sym;
};
template <bool Walk, class Launch>
void with_form(LaunchForm f, Launch &&launch) {
  if (f.root == kRootGumbel) launch(FormOf<kRootGumbel, false>{});
  else if (f.root == kRootPuct && f.sym) launch(FormOf<kRootPuct, true>{});
  else if (f.root == kRootPuct) launch(FormOf<kRootPuct, false>{});
  else if constexpr (Walk) {
    if (f.root == kRootForced && f.sym) launch(FormOf<kRootForced, true>{});
    else if (f.root == kRootForced) launch(FormOf<kRootForced, false>{});
  }
}

}  // namespace hz_tree

// ---------------------------------------------------------------- HIP only
#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "hz_device.hpp"
#include "hz_host.hpp"

// The handle of the ABI: the kernels' arguments (a launch passes *m, of which
// the kernel takes the hz_mcts_args part) and the owners of their buffers.
// Made by new, never moved: the owners keep the addresses of its pointers.
struct hz_mcts : hz_mcts_args {
  hz_host::DevBufs base_bufs, carry_bufs, gumbel_bufs, leaf_sym_bufs, forced_bufs;
};

namespace hz_tree {
using namespace hz;

// ---------------------------------------------------------- device helpers
__device__ __forceinline__ uint64_t ht_entry(int gen, int node) {
  return ((uint64_t)(uint32_t)gen << 32) | (uint32_t)node;
}

__device__ __forceinline__ State load_node(const uint64_t *ns) {
  State s;
#pragma unroll
  for (int k = 0; k < 4; k++) s.pl[k] = ns[k];
  s.piles = ns[4];
  s.misc = ns[5];
  return s;
}

__device__ __forceinline__ void store_node(uint64_t *ns, const State &s) {
#pragma unroll
  for (int k = 0; k < 4; k++) ns[k] = s.pl[k];
  ns[4] = s.piles;
  ns[5] = s.misc;
}

constexpr int kHintNe = 127, kHintTerm = 128;  // edge_hint's fields (edge_hint_of below)
// Wave reductions of the walk: within each row of 16 lanes by DPP moves (a
// VALU operand modifier: quad_perm xor 1, xor 2, then row_ror 4, 8), across
// the four rows by two ds_bpermute rounds (xor 16, 32): 2 LDS-crossbar
// round trips per reduction instead of 6.  Every lane ends with the result.
template <int Ctrl>
__device__ __forceinline__ int dpp_mov(int v) {
  return __builtin_amdgcn_update_dpp(0, v, Ctrl, 0xf, 0xf, false);
}
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppRor4 = 0x124, kDppRor8 = 0x128;
__device__ __forceinline__ int wave_sum_i(int v) {
  v += dpp_mov<kDppXor1>(v);
  v += dpp_mov<kDppXor2>(v);
  v += dpp_mov<kDppRor4>(v);
  v += dpp_mov<kDppRor8>(v);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}
// (value, index): the largest value, the smallest index among equal values
// (MCTS.py:102-121's first strict '>' in insertion order); associative and
// commutative, so the reduction order does not change the result
__device__ __forceinline__ void argmax_take(double ob, int oi, double &best, int &bi) {
  if (ob > best || (ob == best && oi < bi)) {
    best = ob;
    bi = oi;
  }
}
template <int Ctrl>
__device__ __forceinline__ void argmax_dpp(double &best, int &bi) {
  const long long b = __double_as_longlong(best);
  const int lo = dpp_mov<Ctrl>((int)b), hi = dpp_mov<Ctrl>((int)(b >> 32)), oi = dpp_mov<Ctrl>(bi);
  argmax_take(__longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo)), oi, best,
              bi);
}
__device__ __forceinline__ void wave_argmax(double &best, int &bi) {
  argmax_dpp<kDppXor1>(best, bi);
  argmax_dpp<kDppXor2>(best, bi);
  argmax_dpp<kDppRor4>(best, bi);
  argmax_dpp<kDppRor8>(best, bi);
#pragma unroll
  for (int o = 16; o < kWave; o <<= 1) argmax_take(__shfl_xor(best, o), __shfl_xor(bi, o), best, bi);
}
// edge_hint = first edge << 8 | terminal << 7 | edge count: the first edge
// must fit in 24 bits, so hz_mcts_create refuses max_nodes >= kMaxNodesHint
constexpr int32_t kMaxNodesHint = 1 << 24;
__device__ __forceinline__ int32_t edge_hint_of(int e0, int ne, bool term) {
  return (int32_t)((uint32_t)e0 << 8 | (term ? (uint32_t)kHintTerm : 0u) | (uint32_t)ne);
}
// ------------------------------------------------------------ the Gumbel root
// The root rule of hz_mcts_set_gumbel (include/hz_abi.h states it; no
// reference counterpart).  Lane l holds root edges l and l + 64.  The two
// fp64 sums are the xor butterfly: the lane's partial is edge l's term plus
// edge l + 64's (0.0 for an edge that is absent or unvisited), then
// v = v + v[lane ^ off] for off = 1, 2, 4, 8, 16, 32; minima and maxima are
// exact in any order.  These run once per simulation and board, under the
// gate only: plain cross-lane moves, not the walk's DPP forms.
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) v = __dadd_rn(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) v = fmin(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
// G + log P of one root edge: the one place the transcendental is taken (the
// expansion of node 0 stores it in g_score; the select, the result and
// hz_mcts_root_gumbel_scores read that array); -inf where P is 0
__device__ __forceinline__ double gumbel_edge_score(double g, float p) { return __dadd_rn(g, log((double)p)); }
constexpr double kGumbelFloor = -1e9;
// sigma of the lane's two edges from the root's statistics (ne edges, t = sum
// N), the completed-Q mix v_mix and the largest N
__device__ __forceinline__ void gumbel_sigma(const hz_mcts_args &m, int lane, int ne, int t, int n0, int n1, double w0,
                                             double w1, float p0, float p1, double v_root, double &sg0, double &sg1,
                                             double &v_mix, int &max_n) {
  const bool in0 = lane < ne, in1 = lane + kWave < ne;
  const bool vis0 = in0 && n0 > 0, vis1 = in1 && n1 > 0;
  const double q0 = vis0 ? __ddiv_rn(w0, (double)n0) : 0.0, q1 = vis1 ? __ddiv_rn(w1, (double)n1) : 0.0;
  const double sp = wave_sum_d(__dadd_rn(vis0 ? (double)p0 : 0.0, vis1 ? (double)p1 : 0.0));
  const double spq =
      wave_sum_d(__dadd_rn(vis0 ? __dmul_rn((double)p0, q0) : 0.0, vis1 ? __dmul_rn((double)p1, q1) : 0.0));
  const double wq = sp > 0.0 ? __ddiv_rn(spq, sp) : 0.0;
  v_mix = __ddiv_rn(__dadd_rn(v_root, __dmul_rn((double)t, wq)), (double)(t + 1));
  max_n = wave_max_i(max(in0 ? n0 : 0, in1 ? n1 : 0));
  const double c0 = vis0 ? q0 : v_mix, c1 = vis1 ? q1 : v_mix;  // completed Q
  const double mn = wave_min_d(fmin(in0 ? c0 : INFINITY, in1 ? c1 : INFINITY));
  const double mx = wave_max_d(fmax(in0 ? c0 : -INFINITY, in1 ? c1 : -INFINITY));
  const double den = fmax(__dsub_rn(mx, mn), 1e-8);
  const double scale = __dmul_rn(__dadd_rn(m.g_c_visit, (double)max_n), m.g_c_scale);
  sg0 = in0 ? __dmul_rn(scale, __ddiv_rn(__dsub_rn(c0, mn), den)) : 0.0;
  sg1 = in1 ? __dmul_rn(scale, __ddiv_rn(__dsub_rn(c1, mn), den)) : 0.0;
}

// ------------------------------------------------------------ forced playouts
// Root edge e is forced iff N_e > 0 and (double)(N_e N_e) < (k (double)P_e)
// (double)t: an exact integer product against two fp64 products in that order.
__device__ __forceinline__ bool forced_edge(double k, int n, float p, int t) {
  return n > 0 && (double)((long long)n * (long long)n) < __dmul_rn(__dmul_rn(k, (double)p), (double)t);
}

// A node's edge range [e0, e0 + ne) when it lies within the board's n_edges
// edges (two per lane at most), else ne = 0.
__device__ __forceinline__ int checked_edges(const hz_mcts_args &m, size_t nb, int node, int n_edges, int &e0) {
  const int ne = m.node_ne[nb + node];
  e0 = m.node_e0[nb + node];
  return ne > 0 && ne <= kChildSlots && e0 >= 0 && e0 <= n_edges - ne ? ne : 0;
}
__device__ __forceinline__ bool checked_counts(const hz_mcts_args &m, int n_nodes, int n_edges) {
  return n_nodes > 0 && n_nodes <= m.max_nodes && n_edges >= 0 && n_edges <= m.max_edges;
}

}  // namespace hz_tree
#endif  // __HIPCC__
