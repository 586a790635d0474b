// hz_mcts_report.hip — read-only views of a finished tree (hz_mcts.hip builds
// it): the root's visits, the search report, the two Gumbel reports, the
// statistics and the tree export.  No kernel here writes to the tree.
#include "hz_mcts.hpp"

#include "../../include/hz_abi.h"

using namespace hz;
using namespace hz_host;
using namespace hz_tree;

namespace {

// root visit counts by action (MCTS.py:355-376)
__global__ void __launch_bounds__(kWave) k_result(hz_mcts_args m, int32_t *__restrict__ visits) {
  int b = blockIdx.x;
  int lane = threadIdx.x;
  int32_t *out = visits + (size_t)b * kActions;
  for (int a = lane; a < kActions; a += kWave) out[a] = 0;
  __syncthreads();
  if (m.counts[(size_t)b * 4] == 0) return;
  size_t nb = (size_t)b * m.max_nodes, eb = (size_t)b * m.max_edges;
  int ne = m.node_ne[nb], e0 = m.node_e0[nb];
  for (int i = lane; i < ne; i += kWave) out[m.edge_action[eb + e0 + i]] = m.edge_n[eb + e0 + i];
}

// ------------------------------------------------------------ search report
// Read-only views of the tree for the caller (no reference kernel: the
// reference keeps Python objects, MCTS.get_root_edges MCTS.py:268-269).  Both
// kernels trust nothing they read from the tree: a node's edge range is used
// only when it lies inside the board's edge count, a child link only when it
// is below the board's node count; anything else reads as "no edges".

// The root's edges by action id (MCTS.py:355-376 reads N from them; Edge.stats
// MCTS.py:34-39): N, W, Q = W / N as back_fill leaves it (MCTS.py:254; 0 while
// N == 0), P, the child node; value = sum W / sum N, both sums in edge order.
// One wave per board: the edges' lanes note their action's slot in LDS, then
// lanes are actions and every output row is written once, whole.
__global__ void __launch_bounds__(kWave) k_root_edges(hz_mcts_args m, int32_t *__restrict__ n_out, double *__restrict__ w_out,
                                                      double *__restrict__ q_out, float *__restrict__ p_out,
                                                      int32_t *__restrict__ child_out,
                                                      double *__restrict__ value_out) {
  __shared__ int16_t slot[kActions];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int32_t *cnt = m.counts + (size_t)b * 4;
  const size_t nb = (size_t)b * m.max_nodes, eb = (size_t)b * m.max_edges;
  const int n_nodes = cnt[0], n_edges = cnt[1];
  int e0 = 0;
  const int ne = checked_counts(m, n_nodes, n_edges) ? checked_edges(m, nb, 0, n_edges, e0) : 0;
  for (int a = lane; a < kActions; a += kWave) slot[a] = -1;
  __syncthreads();
  int n0 = 0, n1 = 0;
  double w0 = 0.0, w1 = 0.0;
  if (lane < ne) {
    const size_t e = eb + e0 + lane;
    n0 = m.edge_n[e];
    w0 = m.edge_w[e];
    const int a = m.edge_action[e];
    if (a >= 0 && a < kActions) slot[a] = (int16_t)lane;
  }
  if (lane + kWave < ne) {
    const size_t e = eb + e0 + lane + kWave;
    n1 = m.edge_n[e];
    w1 = m.edge_w[e];
    const int a = m.edge_action[e];
    if (a >= 0 && a < kActions) slot[a] = (int16_t)(lane + kWave);
  }
  __syncthreads();
  for (int a = lane; a < kActions; a += kWave) {
    const int i = slot[a];
    int n = 0, child = -1;
    double w = 0.0, q = 0.0;
    float p = 0.f;
    if (i >= 0) {
      const size_t e = eb + e0 + i;
      n = m.edge_n[e];
      w = m.edge_w[e];
      p = m.edge_p[e];
      child = m.edge_child[e];
      q = n ? __ddiv_rn(w, (double)n) : 0.0;
    }
    const size_t o = (size_t)b * kActions + a;
    n_out[o] = n;
    w_out[o] = w;
    q_out[o] = q;
    p_out[o] = p;
    if (child_out) child_out[o] = child;
  }
  if (value_out) {
    const int sn = wave_sum_i(n0 + n1);
    double sw = 0.0;
    for (int i = 0; i < ne; i++) sw = __dadd_rn(sw, __shfl(i < kWave ? w0 : w1, i & (kWave - 1)));
    if (lane == 0) value_out[b] = sn ? __ddiv_rn(sw, (double)sn) : 0.0;
  }
}

// The line the search expects: from the root, the first edge with the most
// visits (the greedy choice of MCTS.py:418-423 applied at every level), until
// a node without edges, an edge without visits or max_len moves.  One wave
// per board, two edges per lane, one (N, index) reduction per level.
__global__ void __launch_bounds__(kWave) k_pv(hz_mcts_args m, int max_len, int16_t *__restrict__ action,
                                              int32_t *__restrict__ visits, double *__restrict__ q,
                                              uint8_t *__restrict__ player, int32_t *__restrict__ len) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int32_t *cnt = m.counts + (size_t)b * 4;
  const size_t nb = (size_t)b * m.max_nodes, eb = (size_t)b * m.max_edges, ob = (size_t)b * max_len;
  const int n_nodes = cnt[0], n_edges = cnt[1];
  int node = 0, d = 0;
  if (checked_counts(m, n_nodes, n_edges)) {
    while (d < max_len && node >= 0 && node < n_nodes) {
      int e0 = 0;
      const int ne = checked_edges(m, nb, node, n_edges, e0);
      if (ne == 0) break;
      double best = -INFINITY;  // a visit count as a double (exact)
      int bi = 0x7fffffff;
      if (lane < ne) {
        best = (double)m.edge_n[eb + e0 + lane];
        bi = lane;
      }
      if (lane + kWave < ne) {
        const double v = (double)m.edge_n[eb + e0 + lane + kWave];
        if (v > best) { best = v; bi = lane + kWave; }
      }
      wave_argmax(best, bi);
      const int nsel = (int)best;
      if (nsel <= 0) break;
      const size_t e = eb + e0 + bi;
      if (lane == 0) {
        action[ob + d] = m.edge_action[e];
        visits[ob + d] = nsel;
        q[ob + d] = __ddiv_rn(m.edge_w[e], (double)nsel);
        player[ob + d] = m.edge_player[e];
      }
      node = m.edge_child[e];
      d++;
    }
  }
  for (int i = d + lane; i < max_len; i += kWave) {
    action[ob + i] = -1;
    visits[ob + i] = 0;
    q[ob + i] = 0.0;
    player[ob + i] = 0;
  }
  if (lane == 0) len[b] = d;
}

// The root's edges for the two Gumbel reports: at most kMaxChildren of them
// (g_score has that many slots per board), inside the board's counts, on a
// board the search began; else none.
__device__ __forceinline__ int gumbel_root_edges(const hz_mcts_args &m, int b, int &e0) {
  const int32_t *cnt = m.counts + (size_t)b * 4;
  const int n_nodes = cnt[0], n_edges = cnt[1];
  e0 = 0;
  const int ne = checked_counts(m, n_nodes, n_edges) ? checked_edges(m, (size_t)b * m.max_nodes, 0, n_edges, e0) : 0;
  return ne <= kMaxChildren ? ne : 0;
}

// hz_mcts_root_gumbel_scores: G + log P by root edge index (0.0 past the root's edges)
__global__ void __launch_bounds__(kWave) k_gumbel_scores(hz_mcts_args m, double *__restrict__ out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int e0;
  const int ne = gumbel_root_edges(m, b, e0);
  for (int i = lane; i < kMaxChildren; i += kWave)
    out[(size_t)b * kMaxChildren + i] = i < ne ? m.g_score[(size_t)b * kMaxChildren + i] : 0.0;
}

// hz_mcts_gumbel_result: after the search, the move (the first edge with the
// largest score among the most visited), the improved policy softmax(log P +
// sigma) over the root's edges by action id (the maximum subtracted first;
// should every prior be 0, the softmax of sigma alone) and v_mix.  A root
// without edges: action -1, a zero row, value 0.
__global__ void __launch_bounds__(kWave) k_gumbel_result(hz_mcts_args m, int16_t *__restrict__ action,
                                                         float *__restrict__ pi, double *__restrict__ value) {
  const int b = blockIdx.x, lane = threadIdx.x;
  float *row = pi + (size_t)b * kActions;
  for (int a = lane; a < kActions; a += kWave) row[a] = 0.f;
  __syncthreads();  // the zeros before the edges' entries (one wave: ordering only)
  int e0;
  const int ne = gumbel_root_edges(m, b, e0);
  if (ne == 0) {
    if (lane == 0) {
      action[b] = -1;
      value[b] = 0.0;
    }
    return;
  }
  const size_t eb = (size_t)b * m.max_edges + e0, gb = (size_t)b * kMaxChildren;
  const bool in0 = lane < ne, in1 = lane + kWave < ne;
  int n0 = 0, n1 = 0, a0 = -1, a1 = -1;
  double w0 = 0.0, w1 = 0.0, gs0 = 0.0, gs1 = 0.0;
  float p0 = 0.f, p1 = 0.f;
  if (in0) {
    n0 = m.edge_n[eb + lane];
    w0 = m.edge_w[eb + lane];
    p0 = m.edge_p[eb + lane];
    a0 = m.edge_action[eb + lane];
    gs0 = m.g_score[gb + lane];
  }
  if (in1) {
    n1 = m.edge_n[eb + lane + kWave];
    w1 = m.edge_w[eb + lane + kWave];
    p1 = m.edge_p[eb + lane + kWave];
    a1 = m.edge_action[eb + lane + kWave];
    gs1 = m.g_score[gb + lane + kWave];
  }
  const int t = wave_sum_i(n0 + n1);
  double sg0, sg1, v_mix;
  int max_n;
  gumbel_sigma(m, lane, ne, t, n0, n1, w0, w1, p0, p1, (double)m.root_value[b], sg0, sg1, v_mix, max_n);
  double best = -INFINITY;
  int bi = 0x7fffffff;
  if (in0 && n0 == max_n) {
    best = fmax(kGumbelFloor, __dadd_rn(gs0, sg0));
    bi = lane;
  }
  if (in1 && n1 == max_n) {
    const double v = fmax(kGumbelFloor, __dadd_rn(gs1, sg1));
    if (v > best) { best = v; bi = lane + kWave; }
  }
  wave_argmax(best, bi);
  const int act = __shfl(bi < kWave ? a0 : a1, bi & (kWave - 1));
  // the improved policy
  double l0 = in0 ? __dadd_rn(log((double)p0), sg0) : -INFINITY, l1 = in1 ? __dadd_rn(log((double)p1), sg1) : -INFINITY;
  double mx = wave_max_d(fmax(l0, l1));
  if (mx == -INFINITY) {
    l0 = in0 ? sg0 : -INFINITY;
    l1 = in1 ? sg1 : -INFINITY;
    mx = wave_max_d(fmax(l0, l1));
  }
  const double x0 = in0 ? exp(__dsub_rn(l0, mx)) : 0.0, x1 = in1 ? exp(__dsub_rn(l1, mx)) : 0.0;
  const double sum = wave_sum_d(__dadd_rn(x0, x1));
  if (in0 && a0 >= 0 && a0 < kActions) row[a0] = (float)__ddiv_rn(x0, sum);
  if (in1 && a1 >= 0 && a1 < kActions) row[a1] = (float)__ddiv_rn(x1, sum);
  if (lane == 0) {
    action[b] = (int16_t)act;
    value[b] = v_mix;
  }
}

// hz_mcts_pruned_visits: policy target pruning (include/hz_abi.h states the
// rule; KataGo's, with the select's own arithmetic).  One wave per board, two
// root edges per lane as in the walk.  The best edge e* (the first with the
// largest N) sets bound = q + U at its own count; every other visited edge
// gives back up to nf = floor(sqrt((k P) t)) visits, one at a time, while
// its q + U at the reduced count stays below the bound, and goes to 0 when
// a reduction leaves it at most one visit.  The lane's loop runs at most
// min(nf, N) <= sqrt(k t) steps.  A board whose bit is clear, or without a
// visit, gets k_result's row; a board without a tree zeros.
__global__ void __launch_bounds__(kWave) k_pruned_visits(hz_mcts_args m, float cpuct, int32_t *__restrict__ visits) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int32_t *out = visits + (size_t)b * kActions;
  for (int a = lane; a < kActions; a += kWave) out[a] = 0;
  __syncthreads();  // the zeros before the edges' entries (one wave: ordering only)
  const int32_t *cnt = m.counts + (size_t)b * 4;
  const int n_nodes = cnt[0], n_edges = cnt[1];
  int e0 = 0;
  const int ne = checked_counts(m, n_nodes, n_edges) ? checked_edges(m, (size_t)b * m.max_nodes, 0, n_edges, e0) : 0;
  if (ne == 0) return;
  const size_t eb = (size_t)b * m.max_edges + e0;
  const bool in0 = lane < ne, in1 = lane + kWave < ne;
  int n0 = 0, n1 = 0, a0 = -1, a1 = -1;
  double w0 = 0.0, w1 = 0.0;
  float p0 = 0.f, p1 = 0.f;
  if (in0) {
    n0 = m.edge_n[eb + lane];
    w0 = m.edge_w[eb + lane];
    p0 = m.edge_p[eb + lane];
    a0 = m.edge_action[eb + lane];
  }
  if (in1) {
    n1 = m.edge_n[eb + lane + kWave];
    w1 = m.edge_w[eb + lane + kWave];
    p1 = m.edge_p[eb + lane + kWave];
    a1 = m.edge_action[eb + lane + kWave];
  }
  const int t = wave_sum_i(n0 + n1);
  const bool on = (!m.forced_mask || m.forced_mask[b]) && t > 0;
  if (on) {
    const double s = __dsqrt_rn(t > 1 ? (double)t : 1.0);
    auto u_of = [&](float p, int x) {
      return __ddiv_rn(__dmul_rn((double)__fmul_rn(cpuct, p), s), (double)(1 + x));
    };
    double best = -INFINITY;  // a visit count as a double (exact)
    int bi = 0x7fffffff;
    if (in0) {
      best = (double)n0;
      bi = lane;
    }
    if (in1 && (double)n1 > best) {
      best = (double)n1;
      bi = lane + kWave;
    }
    wave_argmax(best, bi);
    const int src = bi & (kWave - 1);
    const bool hi = bi >= kWave;
    const int nb = __shfl(hi ? n1 : n0, src);
    const double wb = __shfl(hi ? w1 : w0, src);
    const float pb = __shfl(hi ? p1 : p0, src);
    const double bound = __dadd_rn(nb ? __ddiv_rn(wb, (double)nb) : 0.0, u_of(pb, nb));
    auto prune = [&](int e, int n, double w, float p) {
      if (e == bi || n <= 0) return n;
      const double q = __ddiv_rn(w, (double)n);
      // nf as an int, at most n (a NaN or a negative root gives 0)
      const double rt = floor(__dsqrt_rn(__dmul_rn(__dmul_rn(m.forced_k, (double)p), (double)t)));
      const int lim = rt >= (double)n ? n : (rt > 0.0 ? (int)rt : 0);
      int r = 0;
      for (int j = 1; j <= lim; j++) {
        if (!(__dadd_rn(q, u_of(p, n - j)) < bound)) break;
        r = j;
      }
      const int left = n - r;
      return r > 0 && left <= 1 ? 0 : left;
    };
    n0 = prune(lane, n0, w0, p0);
    n1 = prune(lane + kWave, n1, w1, p1);
  }
  if (in0 && a0 >= 0 && a0 < kActions) out[a0] = n0;
  if (in1 && a1 >= 0 && a1 < kActions) out[a1] = n1;
}

// Sum of every edge's visit count over the board's tree: each simulation
// adds one visit to every edge of its path in back_fill (MCTS.py:220-266),
// so this is the number of edge levels the searches walked (the path-walk
// term of the tree's algorithmic bytes).  Wave per board, one vector atomic.
__global__ void __launch_bounds__(kWave) k_path_edges(hz_mcts_args m, unsigned long long *__restrict__ out) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const int ne = m.counts[(size_t)b * 4 + 1];
  const int32_t *en = m.edge_n + (size_t)b * m.max_edges;
  unsigned long long acc = 0;
  for (int e = lane; e < ne; e += kWave) acc += (unsigned)en[e];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, kWave);
  if (lane == 0 && acc) atomicAdd(out, acc);
}
}  // namespace

extern "C" {

int hz_mcts_result(hz_mcts *m, int32_t *visits) {
  if (!m || !visits) return -1;
  hipLaunchKernelGGL(k_result, dim3(m->n), dim3(kWave), 0, m->stream, *m, visits);
  return launch_err();
}

int hz_mcts_stats(hz_mcts *m, int32_t *counts) {
  if (!m || !counts) return -1;
  return hipMemcpyAsync(counts, m->counts, (size_t)m->n * 4 * sizeof(int32_t), hipMemcpyDeviceToDevice, m->stream)
             ? 1
             : 0;
}

int hz_mcts_root_edges(hz_mcts *m, int32_t *n, double *w, double *q, float *p, int32_t *child, double *value) {
  if (!m || !n || !w || !q || !p) return -1;
  hipLaunchKernelGGL(k_root_edges, dim3(m->n), dim3(kWave), 0, m->stream, *m, n, w, q, p, child, value);
  return launch_err();
}

int hz_mcts_pv(hz_mcts *m, int32_t max_len, int16_t *action, int32_t *visits, double *q, uint8_t *player,
               int32_t *len) {
  if (!m || max_len < 1 || max_len > m->max_depth || !action || !visits || !q || !player || !len) return -1;
  hipLaunchKernelGGL(k_pv, dim3(m->n), dim3(kWave), 0, m->stream, *m, max_len, action, visits, q, player, len);
  return launch_err();
}

int hz_mcts_export_tree(hz_mcts *m, int32_t b, uint64_t *node_state, int32_t *node_e0, int32_t *node_ne,
                        int16_t *edge_action, int32_t *edge_child, int32_t *edge_n, double *edge_w, float *edge_p,
                        uint8_t *edge_player) {
  if (!m || b < 0 || b >= m->n) return -1;
  const size_t nb = (size_t)b * m->max_nodes, eb = (size_t)b * m->max_edges, N = m->max_nodes, E = m->max_edges;
  auto copy = [&](void *dst, const void *src, size_t bytes) {
    return !dst || hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, m->stream) == hipSuccess;
  };
  const bool ok = copy(node_state, m->node_state + nb * 6, N * 6 * sizeof(uint64_t)) &&
                  copy(node_e0, m->node_e0 + nb, N * sizeof(int32_t)) &&
                  copy(node_ne, m->node_ne + nb, N * sizeof(int32_t)) &&
                  copy(edge_action, m->edge_action + eb, E * sizeof(int16_t)) &&
                  copy(edge_child, m->edge_child + eb, E * sizeof(int32_t)) &&
                  copy(edge_n, m->edge_n + eb, E * sizeof(int32_t)) &&
                  copy(edge_w, m->edge_w + eb, E * sizeof(double)) &&
                  copy(edge_p, m->edge_p + eb, E * sizeof(float)) &&
                  copy(edge_player, m->edge_player + eb, E * sizeof(uint8_t));
  return ok ? 0 : 1;
}

int hz_mcts_sims_done(hz_mcts *m, int32_t *out) {
  if (!m || !out) return -1;
  return hipMemcpyAsync(out, m->sims_done, (size_t)m->n * sizeof(int32_t), hipMemcpyDeviceToDevice, m->stream) ? 1
                                                                                                                : 0;
}

int hz_mcts_root_gumbel_scores(hz_mcts *m, double *out) {
  if (!m || !out || !m->gumbel) return -1;
  hipLaunchKernelGGL(k_gumbel_scores, dim3(m->n), dim3(kWave), 0, m->stream, *m, out);
  return launch_err();
}

int hz_mcts_gumbel_result(hz_mcts *m, int16_t *action, float *pi, double *value) {
  if (!m || !action || !pi || !value || !m->gumbel) return -1;
  hipLaunchKernelGGL(k_gumbel_result, dim3(m->n), dim3(kWave), 0, m->stream, *m, action, pi, value);
  return launch_err();
}

int hz_mcts_pruned_visits(hz_mcts *m, float cpuct, int32_t *visits) {
  if (!m || !visits || !(m->forced_k > 0.0)) return -1;
  hipLaunchKernelGGL(k_pruned_visits, dim3(m->n), dim3(kWave), 0, m->stream, *m, cpuct, visits);
  return launch_err();
}

int hz_mcts_forced_counts(hz_mcts *m, int32_t *out) {
  if (!m || !out || !(m->forced_k > 0.0)) return -1;
  return hipMemcpyAsync(out, m->forced_cnt, (size_t)m->n * 2 * sizeof(int32_t), hipMemcpyDeviceToDevice, m->stream)
             ? 1
             : 0;
}

int hz_mcts_path_edges(hz_mcts *m, int64_t *out) {
  if (!m || !out) return -1;
  hipLaunchKernelGGL(k_path_edges, dim3(m->n), dim3(kWave), 0, m->stream, *m, (unsigned long long *)out);
  return launch_err();
}

}  // extern "C"
