"""BatchedMCTS: one PUCT search per board of a BatchedEnv, all boards advancing
in lock-step so that every simulation's leaf evaluations form one PyTorch
batch (the reference evaluates one leaf at a time: MCTS.py:291-352).

    select (HIP) -> gather + encode the leaves that need the network (HIP)
    -> evaluator(board, glob) (PyTorch) -> expand + backup (HIP)

Like the reference, which calls predict only for non-terminal leaves
(MCTS.py:297-341), each simulation's batch holds only the active boards
whose selected leaf is not terminal, gathered on the device: in board order
(hz_mcts_gather_leaves), or, for an evaluator that declares
`row_independent = True` (each output row a function of its input row
alone, whatever its position or the batch size: the folded network, the
stub), in arrival order by the fused expand/backup/select/gather launch.

The evaluator is any callable (board f32[k,38,5,7], glob f32[k,42]) ->
(policy f32[k,143] probabilities, value f32[k]) on the same device, e.g.
`BatchedPredictor(model)` wrapping model.py's AlphaZeroModel the way
ModelManager.predict does (softmax over all 143 logits, model.py:81-110).
An evaluator with `device_rows = True` is instead called as
evaluator(board, glob, rows, count) on the full [n]-row buffers, of which
the first count[0] (a device int32) are live and rows[j] is row j's board:
no host round trip per simulation (BatchedPredictor's HIP kernels take
count as their live-row bound).
"""
import ctypes
from typing import NamedTuple

import torch

from . import _native as nat
from .env import ACTION_SIZE

MAX_CHILDREN = 69
MAX_NODES_END = 1 << 24  # hz_mcts_create refuses max_nodes from here on (an edge id must fit 24 bits)
DEFAULT_MAX_DEPTH = 192
FORCED_K_DEFAULT = 2.0  # KataGo's k (forced playouts), not tuned here
GUMBEL_DEFAULT = {"max_considered": 16, "c_visit": 50.0, "c_scale": 1.0}  # the paper's setting, not tuned here


def considered_visit_table(max_considered, n_root):
    """The Gumbel root's considered-visit table (include/hz_abi.h,
    hz_mcts_set_gumbel): int16 numpy [max_considered + 1, n_root]; row m is the
    paper's sequential-halving sequence for m considered actions and n_root
    root visits (rows 0 and 1: 0, 1, 2, ...)."""
    import math

    import numpy as np
    max_considered, n_root = int(max_considered), int(n_root)
    if max_considered < 1 or not 1 <= n_root <= 32767:
        raise ValueError(f"max_considered {max_considered} below 1 or n_root {n_root} outside 1..32767")
    table = np.zeros((max_considered + 1, n_root), np.int16)
    for m in range(max_considered + 1):
        if m <= 1:
            table[m] = np.arange(n_root)
            continue
        log2m = math.ceil(math.log2(m))
        seq, visits, k = [], [0] * m, m
        while len(seq) < n_root:
            for _ in range(max(1, int(n_root / (log2m * k)))):
                seq.extend(visits[:k])
                for i in range(k):
                    visits[i] += 1
            k = max(2, k // 2)
        table[m] = seq[:n_root]
    return table


class Gate(NamedTuple):  # the handle's gates as _open() last set them (a captured simulation holds them by value)
    budget: bool = False      # the budget gate is on
    root_noise: bool = False  # the root-noise mask is on
    gumbel: tuple = None      # the Gumbel gate's (max_considered, n_root, c_visit, c_scale), or None
    leaf_sym: bool = False    # the leaf-symmetry gate is on
    forced: tuple = None      # the forced gate's (k, mask given), or None


class BatchedMCTS:
    def __init__(self, env, num_simulations, max_nodes=None, max_depth=DEFAULT_MAX_DEPTH, exact_keys=False):
        self.env = env
        self.n = env.n
        self.device = env.device
        self.num_simulations = int(num_simulations)
        self._graph_cache = None  # (key, captured simulation, network) kept by search(graph=True)
        self._capture_stream = None  # this handle's graph-capture stream (own split-tower counter block)
        # the default pools cannot overflow: one expansion of at most 69
        # children per simulation (hz_abi.h, hz_mcts_create)
        default_nodes = 1 + MAX_CHILDREN * self.num_simulations
        self.max_nodes = default_nodes if max_nodes is None else int(max_nodes)
        self.max_depth = int(max_depth)
        if not 2 <= self.max_nodes < MAX_NODES_END:
            raise ValueError(f"max_nodes {self.max_nodes} outside 2..{MAX_NODES_END - 1}")
        if self.max_depth < 1:
            raise ValueError(f"max_depth {self.max_depth} below 1")
        # smaller pools or a shorter path than the defaults: a search may hit
        # a limit (stats()[:, 3] != 0: still a search, of a truncated tree, no
        # longer the reference's); _finish() then counts the flagged boards
        self.bounded = self.max_nodes < default_nodes or self.max_depth < DEFAULT_MAX_DEPTH
        self._report = {}  # output buffers of root_edges / principal_variation / export_tree, made on first use
        L = nat.lib()
        self._h = L.hz_mcts_create(self.n, self.max_nodes, self.max_depth, int(bool(exact_keys)),
                                   nat.stream_ptr(self.device))
        if not self._h:
            raise nat.NativeError("hz_mcts_create failed (out of device memory?)")
        d = self.device
        self.board = torch.zeros(self.n, 38, 5, 7, dtype=torch.float32, device=d)
        self.glob = torch.zeros(self.n, 42, dtype=torch.float32, device=d)
        self.visits = torch.zeros(self.n, ACTION_SIZE, dtype=torch.int32, device=d)
        self.counts = torch.zeros(self.n, 4, dtype=torch.int32, device=d)
        self.rows = torch.zeros(self.n, dtype=torch.int32, device=d)
        self.count = torch.zeros(1, dtype=torch.int32, device=d)
        # the second leaf-count buffer of the fused gather (search(): the
        # launch that consumes one count builds the next batch's in the other)
        self.count_b = torch.zeros(1, dtype=torch.int32, device=d)
        self.eval_rows = torch.zeros(1, dtype=torch.int64, device=d)  # leaves evaluated, last search
        self.eval_rows_total = torch.zeros(1, dtype=torch.int64, device=d)  # ... all searches (one add each)
        # k_gather adds each simulation's gathered row count to it (no extra kernel)
        nat.check(L.hz_mcts_set_eval_counter(self._h, nat.ptr(self.eval_rows)), "hz_mcts_set_eval_counter")
        # count_edges: after each search, its edges (one apply_move per legal
        # child of every expanded leaf, MCTS.py:171-177; the skipped self-loop
        # children of :189-194 are not edges) are added on the device to
        # edges_total (two small launches per search, no host read)
        self.count_edges = False
        # the next simulation's select inside each expand/backup launch (search(); False: separate launches)
        self.fuse_select = True
        # ... and the next leaf batch's gather + encode too (each board that needs the network takes a row and
        # encodes its leaf in that launch; False keeps hz_mcts_gather_leaves' separate launch)
        self.fuse_gather = True
        self.edges_total = torch.zeros(1, dtype=torch.int64, device=d)
        # count_path: after each search, the edge levels its simulations
        # walked (the sum of the tree's edge visit counts, hz_mcts_path_edges)
        # are added on the device to path_total (one small launch per search)
        self.count_path = False
        self.path_total = torch.zeros(1, dtype=torch.int64, device=d)
        # boards whose search hit a limit, all searches (added by _finish() on
        # a bounded handle only: one small device sum per search, no host read)
        self.limit_hits_total = torch.zeros(1, dtype=torch.int64, device=d)
        self._nil_pol = torch.zeros(1, ACTION_SIZE, dtype=torch.float32, device=d)
        self._nil_val = torch.zeros(1, dtype=torch.float32, device=d)
        self._sims_done = torch.zeros(self.n, dtype=torch.int32, device=d)
        # an expand call of this search got fewer policy rows than there are
        # boards: only then can a row lie past them, and _finish() reads the
        # handle's error word (hz_mcts_set_row_cap)
        self._cap_risk = False
        self._gate = Gate()  # as last set by _open()
        self._leaf_sym = torch.zeros(self.n, dtype=torch.uint8, device=d)  # leaf_symmetries()' report
        self._gumbel_tables = {}  # (max_considered, n_root) -> the device table (built once per shape)
        # tree reuse (advance() / search(carry=True)): advance's info rows, and
        # the edges and walked levels the search began with (count_edges and
        # count_path add only what the search itself made)
        self._carry_info = torch.zeros(self.n, 3, dtype=torch.int32, device=d)
        self._edges_base = None
        self._path_base = None

    def close(self):
        if getattr(self, "_h", None):
            torch.cuda.synchronize(self.device)
            nat.lib().hz_mcts_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _sync(self):
        nat.lib().hz_mcts_set_stream(self._h, nat.stream_ptr(self.device))
        self.env._sync_stream()

    # -- the four device stages ----------------------------------------------
    def begin(self, active=None):
        self._sync()
        nat.check(nat.lib().hz_mcts_begin(self._h, self.env.handle, nat.ptr(active)), "hz_mcts_begin")

    def _per_board(self, t, dtype, name):
        t = t.to(device=self.device, dtype=dtype).contiguous()
        if t.shape != (self.n,):
            raise ValueError(f"{name} of shape {tuple(t.shape)}, not ({self.n},)")
        return t

    def _mask(self, mask, name="mask"):
        """A per-board mask of the masked entry points: uint8 [n] on the device."""
        if not torch.is_tensor(mask) or mask.shape != (self.n,):
            raise ValueError(f"{name}: a tensor of one flag per board, shape ({self.n},)")
        return mask.to(device=self.device, dtype=torch.uint8).contiguous()

    def begin_some(self, mask):
        """begin() for the boards whose mask is 1 (hz_mcts_begin_some), with
        nothing written on the boards whose mask is 0: their trees, counts
        and sims_done stay what they are (begin() clears inactive boards and
        zeroes every board's sims_done).  A board whose mask is 2 is stopped:
        no tree, and budget 0 under the gate."""
        self._sync()
        nat.check(nat.lib().hz_mcts_begin_some(self._h, self.env.handle, nat.ptr(self._mask(mask))),
                  "hz_mcts_begin_some")

    def set_gate_some(self, mask, budget=None, root_noise=None):
        """The budget and the root-noise bit of the boards whose mask is 1
        (hz_mcts_set_gate_some), written into the handle's copies in stream
        order; every other board keeps its own.  The gate (the mask) must be
        on: set by the last search(budget=, root_noise=) or _set_gate()."""
        if budget is not None:
            if not self._gate.budget:
                raise ValueError("set_gate_some(budget=) while the budget gate is off")
            budget = self._per_board(budget, torch.int32, "budget")
        if root_noise is not None:
            if not self._gate.root_noise:
                raise ValueError("set_gate_some(root_noise=) while the root-noise mask is off")
            root_noise = self._mask(root_noise, "root_noise")
        nat.check(nat.lib().hz_mcts_set_gate_some(self._h, nat.ptr(budget), nat.ptr(root_noise),
                                                  nat.ptr(self._mask(mask))), "hz_mcts_set_gate_some")

    def begin_carried(self, active=None, noise=None, eps=0.25, testing=True):
        """begin() that keeps the trees advance() carried (hz_mcts_begin_carried):
        a carried board whose node 0 still is the env's state starts from its
        tree, its expanded root's priors mixed with the noise where the board
        is noisy; every other active board starts fresh.  The carry is consumed."""
        self._sync()
        if noise is not None:
            noise = noise.to(device=self.device, dtype=torch.float64).contiguous()
        nat.check(nat.lib().hz_mcts_begin_carried(self._h, self.env.handle, nat.ptr(active), nat.ptr(noise),
                                                  float(eps), int(bool(testing))), "hz_mcts_begin_carried")

    def advance(self, action, active=None, headroom=None):
        """Tree reuse, after env.step(action): each board keeps the subtree
        below the move just played as the start of its next search
        (hz_mcts_advance, whose rule include/hz_abi.h states), or drops its
        tree: an inactive board, a move without a root edge, a terminal child,
        a child whose state is not the env's (a turn end whose draws differ), or
        a kept tree that leaves less than `headroom` free nodes or edges
        (default 69 * num_simulations: the next search cannot hit max_nodes).
        Returns device int32 [n] tensors {"nodes", "edges", "visits"} (kept
        nodes, kept edges, the new root's visits; zeros where dropped): views
        of the handle's own buffer, rewritten by the next call.  The carry is
        taken up by the next search(carry=True) only."""
        self._sync()
        action = self._per_board(action, torch.int16, "action")
        if active is not None:
            active = active.to(device=self.device, dtype=torch.uint8).contiguous()
        headroom = MAX_CHILDREN * self.num_simulations if headroom is None else int(headroom)
        if headroom < 0:
            raise ValueError(f"headroom {headroom} below 0")
        nat.check(nat.lib().hz_mcts_advance(self._h, self.env.handle, nat.ptr(action), nat.ptr(active), headroom,
                                            nat.ptr(self._carry_info)), "hz_mcts_advance")
        info = self._carry_info
        return {"nodes": info[:, 0], "edges": info[:, 1], "visits": info[:, 2]}

    def select(self, cpuct, active=None):
        nat.check(nat.lib().hz_mcts_select(self._h, nat.ptr(active), float(cpuct)), "hz_mcts_select")

    def encode_leaves(self):
        nat.check(nat.lib().hz_mcts_encode_leaves(self._h, nat.ptr(self.board), nat.ptr(self.glob)),
                  "hz_mcts_encode_leaves")
        return self.board, self.glob

    def select_gather(self, cpuct, active=None):
        """select then gather_leaves; one launch when the handle has at most
        32 boards (hz_mcts_select_gather)."""
        nat.check(nat.lib().hz_mcts_select_gather(self._h, nat.ptr(active), float(cpuct), nat.ptr(self.board),
                                                  nat.ptr(self.glob), nat.ptr(self.rows), nat.ptr(self.count)),
                  "hz_mcts_select_gather")
        return self.board, self.glob, self.rows, self.count

    def gather_leaves(self):
        """The leaves that need the network, in board order: (board, glob,
        rows, count) with rows [0, count[0]) live (hz_mcts_gather_leaves)."""
        nat.check(nat.lib().hz_mcts_gather_leaves(self._h, nat.ptr(self.board), nat.ptr(self.glob),
                                                  nat.ptr(self.rows), nat.ptr(self.count)),
                  "hz_mcts_gather_leaves")
        return self.board, self.glob, self.rows, self.count

    def expand_backup(self, policy, value, noise=None, eps=0.25, testing=True, gathered=False):
        policy, value, noise = self._expand_args(policy, value, noise)
        fn = nat.lib().hz_mcts_expand_backup_gathered if gathered else nat.lib().hz_mcts_expand_backup
        nat.check(fn(self._h, self.env.handle, nat.ptr(policy), nat.ptr(value), nat.ptr(noise), float(eps),
                     int(bool(testing))), "hz_mcts_expand_backup")

    def expand_backup_select(self, policy, value, cpuct, active=None, noise=None, eps=0.25, testing=True):
        """expand_backup(gathered=True), then the next simulation's select in
        the same launch (hz_mcts_expand_backup_select)."""
        policy, value, noise = self._expand_args(policy, value, noise)
        nat.check(nat.lib().hz_mcts_expand_backup_select(self._h, self.env.handle, nat.ptr(policy), nat.ptr(value),
                                                         nat.ptr(noise), float(eps), int(bool(testing)),
                                                         nat.ptr(active), float(cpuct)),
                  "hz_mcts_expand_backup_select")

    def expand_backup_select_gather(self, policy, value, cpuct, active, noise, eps, testing, count_out, count_prev,
                                    add_prev):
        """expand_backup_select, then the next leaf batch in the same launch
        (hz_mcts_expand_backup_select_gather): rows in arrival order into
        self.board / self.glob / self.rows, its count into count_out (zero on
        entry); count_prev (this batch's) is zeroed, and first added to the
        eval counter when add_prev."""
        policy, value, noise = self._expand_args(policy, value, noise)
        nat.check(nat.lib().hz_mcts_expand_backup_select_gather(
            self._h, self.env.handle, nat.ptr(policy), nat.ptr(value), nat.ptr(noise), float(eps), int(bool(testing)),
            nat.ptr(active), float(cpuct), nat.ptr(self.board), nat.ptr(self.glob), nat.ptr(self.rows),
            nat.ptr(count_out), nat.ptr(count_prev), int(bool(add_prev))), "hz_mcts_expand_backup_select_gather")

    def _expand_args(self, policy, value, noise):
        """What every expand call passes: float32 policy rows and values (the
        nil row when no leaf needed the network: never read, but not NULL),
        float64 noise, all contiguous; and the row cap set from them."""
        if policy.numel() == 0:
            policy, value = self._nil_pol, self._nil_val
        policy = policy.to(dtype=torch.float32).contiguous()
        value = value.reshape(-1).to(dtype=torch.float32).contiguous()
        if noise is not None:
            noise = noise.to(device=self.device, dtype=torch.float64).contiguous()
        self._set_row_cap(policy, value)
        return policy, value, noise

    def _set_row_cap(self, policy, value):
        """Before every expand call: the kernel may read rows [0, cap) of
        policy and value and no others (hz_mcts_set_row_cap); captured into a
        graph, the cap is the capture's max_rows."""
        cap = min(int(policy.shape[0]), int(value.numel()))
        nat.check(nat.lib().hz_mcts_set_row_cap(self._h, cap), "hz_mcts_set_row_cap")
        if cap < self.n:
            self._cap_risk = True

    def result(self):
        nat.check(nat.lib().hz_mcts_result(self._h, nat.ptr(self.visits)), "hz_mcts_result")
        return self.visits

    def sims_done(self):
        """Device int32 [n]: the simulations each board had in the last search
        under a budget (hz_mcts_sims_done): min(budget, sims) where it was
        searched, 0 on boards left out, on stuck roots and in a search
        without a budget.  The handle's own tensor, rewritten by the next call."""
        nat.check(nat.lib().hz_mcts_sims_done(self._h, nat.ptr(self._sims_done)), "hz_mcts_sims_done")
        return self._sims_done

    def _set_gumbel(self, gumbel, total, max_considered, c_visit, c_scale):
        """The Gumbel gate of the search about to begin (gumbel None: off),
        copied into the handle in stream order; returns the gate's settings
        (what a captured simulation holds of it) or None."""
        L = nat.lib()
        if gumbel is None:
            nat.check(L.hz_mcts_set_gumbel(self._h, None, None, 0, 0, 0.0, 0.0), "hz_mcts_set_gumbel")
            return None
        gumbel = gumbel.to(device=self.device, dtype=torch.float64).contiguous()
        if gumbel.shape != (self.n, MAX_CHILDREN):
            raise ValueError(f"gumbel of shape {tuple(gumbel.shape)}, not ({self.n}, {MAX_CHILDREN})")
        mc = GUMBEL_DEFAULT["max_considered"] if max_considered is None else int(max_considered)
        cv = GUMBEL_DEFAULT["c_visit"] if c_visit is None else float(c_visit)
        cs = GUMBEL_DEFAULT["c_scale"] if c_scale is None else float(c_scale)
        if not 1 <= mc <= MAX_CHILDREN or not cv >= 0.0 or not cs >= 0.0:
            raise ValueError(f"max_considered {mc} outside 1..{MAX_CHILDREN}, or a negative c_visit / c_scale")
        n_root = max(1, int(total) - 1)  # simulation 1 expands the root and visits no edge
        table = self._gumbel_tables.get((mc, n_root))
        if table is None:
            if len(self._gumbel_tables) >= 8:
                self._gumbel_tables.clear()
            table = self._gumbel_tables[(mc, n_root)] = torch.from_numpy(
                considered_visit_table(mc, n_root)).to(self.device)
        nat.check(L.hz_mcts_set_gumbel(self._h, nat.ptr(gumbel), nat.ptr(table), mc, n_root, cv, cs),
                  "hz_mcts_set_gumbel")
        return (mc, n_root, cv, cs)

    def gumbel_result(self):
        """After search(root="gumbel") (hz_mcts_gumbel_result): device tensors
        action int16 [n] (the move of the first edge with the largest score
        among the most visited; -1 for a root without edges), pi f32 [n, 143]
        (the improved policy softmax(log P + sigma) over the root's edges, a
        zero row where there are none) and value f64 [n] (v_mix, from the
        root mover's side).  The handle's own tensors, rewritten by the next call."""
        if self._gate.gumbel is None:
            raise ValueError("gumbel_result() after a search without root='gumbel'")
        r = self._report.get("gumbel")
        if r is None:
            z = self._zeros
            r = self._report["gumbel"] = {"action": z(torch.int16, self.n), "pi": z(torch.float32, self.n, ACTION_SIZE),
                                          "value": z(torch.float64, self.n)}
        nat.check(nat.lib().hz_mcts_gumbel_result(self._h, nat.ptr(r["action"]), nat.ptr(r["pi"]),
                                                  nat.ptr(r["value"])), "hz_mcts_gumbel_result")
        return dict(r)

    def root_gumbel_scores(self):
        """After search(root="gumbel"): device f64 [n, 69], G + log P per root
        edge in edge order (hz_mcts_root_gumbel_scores: the values the root's
        select used; -inf where P is 0, 0.0 past the root's edges)."""
        if self._gate.gumbel is None:
            raise ValueError("root_gumbel_scores() after a search without root='gumbel'")
        r = self._report.get("gumbel_scores")
        if r is None:
            r = self._report["gumbel_scores"] = self._zeros(torch.float64, self.n, MAX_CHILDREN)
        nat.check(nat.lib().hz_mcts_root_gumbel_scores(self._h, nat.ptr(r)), "hz_mcts_root_gumbel_scores")
        return r

    def _set_leaf_symmetry(self, keys):
        """The leaf-symmetry gate of the search about to begin (keys None:
        off), copied into the handle in stream order; returns whether it is on."""
        L = nat.lib()
        if keys is None:
            nat.check(L.hz_mcts_set_leaf_symmetry(self._h, None), "hz_mcts_set_leaf_symmetry")
            return False
        if not torch.is_tensor(keys) or keys.dtype not in (torch.int64, torch.uint64):
            raise ValueError("leaf_symmetry: an int64 / uint64 tensor of one key per board (NoiseSource.leaf_symmetry)")
        keys = self._per_board(keys, keys.dtype, "leaf_symmetry")
        nat.check(L.hz_mcts_set_leaf_symmetry(self._h, nat.ptr(keys)), "hz_mcts_set_leaf_symmetry")
        return True

    def leaf_symmetries(self):
        """Device uint8 [n]: the symmetry g each board's current leaf is
        evaluated under (hz_mcts_leaf_symmetry): 0 for a board without a leaf
        to evaluate, and everywhere after a search without leaf_symmetry=.
        The handle's own tensor, rewritten by the next call."""
        nat.check(nat.lib().hz_mcts_leaf_symmetry(self._h, nat.ptr(self._leaf_sym)), "hz_mcts_leaf_symmetry")
        return self._leaf_sym

    def _set_forced(self, forced, forced_k):
        """The forced-playout gate of the search about to begin (forced None
        or False: off), the mask copied into the handle in stream order;
        returns (the gate's k, whether a mask was given), which is what a
        captured simulation holds of it by value, or None."""
        L = nat.lib()
        if forced is None or forced is False:
            nat.check(L.hz_mcts_set_forced(self._h, None, 0.0), "hz_mcts_set_forced")
            return None
        k = FORCED_K_DEFAULT if forced_k is None else float(forced_k)
        if not k > 0.0:
            raise ValueError(f"forced_k {forced_k!r}: not above 0")
        mask = None
        if forced is not True:
            if not torch.is_tensor(forced) or forced.dtype not in (torch.bool, torch.uint8):
                raise ValueError("forced: True, or a bool / uint8 tensor of one flag per board")
            mask = self._per_board(forced, torch.uint8, "forced")
        nat.check(L.hz_mcts_set_forced(self._h, nat.ptr(mask), k), "hz_mcts_set_forced")
        return k, mask is not None

    def pruned_visits(self, cpuct):
        """After search(forced=) (hz_mcts_pruned_visits): device int32 [n, 143],
        the root's visits with the visits that were only forced taken back
        (policy target pruning, whose rule include/hz_abi.h states; cpuct: the
        search's).  A board whose forced bit was clear has its result() row, a
        board without a tree zeros.  The handle's own tensor, rewritten by the
        next call."""
        if self._gate.forced is None:
            raise ValueError("pruned_visits() after a search without forced=")
        r = self._report.get("pruned")
        if r is None:
            r = self._report["pruned"] = self._zeros(torch.int32, self.n, ACTION_SIZE)
        nat.check(nat.lib().hz_mcts_pruned_visits(self._h, float(cpuct), nat.ptr(r)), "hz_mcts_pruned_visits")
        return r

    def forced_counts(self):
        """After search(forced=) (hz_mcts_forced_counts): device int32 [n, 2],
        per board the root selections of the search under the gate and those
        the forced rule decided.  The handle's own tensor."""
        if self._gate.forced is None:
            raise ValueError("forced_counts() after a search without forced=")
        r = self._report.get("forced_counts")
        if r is None:
            r = self._report["forced_counts"] = self._zeros(torch.int32, self.n, 2)
        nat.check(nat.lib().hz_mcts_forced_counts(self._h, nat.ptr(r)), "hz_mcts_forced_counts")
        return r

    def _set_gate(self, budget, root_noise):
        """The budget gate and the root-noise mask of the search about to begin (None: off), in stream order."""
        L = nat.lib()
        if budget is not None:
            budget = self._per_board(budget, torch.int32, "budget")
        if root_noise is not None:
            root_noise = self._per_board(root_noise, torch.uint8, "root_noise")
        nat.check(L.hz_mcts_set_budget(self._h, nat.ptr(budget)), "hz_mcts_set_budget")
        nat.check(L.hz_mcts_set_root_noise_mask(self._h, nat.ptr(root_noise)), "hz_mcts_set_root_noise_mask")
        self._gate = self._gate._replace(budget=budget is not None, root_noise=root_noise is not None)

    def stats(self):
        nat.check(nat.lib().hz_mcts_stats(self._h, nat.ptr(self.counts)), "hz_mcts_stats")
        return self.counts

    def limit_flags(self):
        """Device int32 [n]: nonzero where the board's last search hit a limit
        (1: an expansion did not fit max_nodes, or a walk reached max_depth;
        2: a leaf with more than 69 legal moves) -- stats()[:, 3], no host
        read.  A board with 0 searched exactly as an unbounded search would.
        hz_mcts_begin clears the flag of the boards it starts; a board left
        out of the last search (stats()[:, 0] == 0) keeps its earlier flag."""
        return self.stats()[:, 3]

    # -- the search report (read-only views of the trees) ---------------------
    def _zeros(self, dtype, *shape):
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def root_edges(self, value=True):
        """The root's edge statistics by action id (hz_mcts_root_edges; the
        reference's MCTS.get_root_edges, MCTS.py:268-269): device tensors n
        int32 [n, 143], w f64, q f64 (W / N; 0 while N == 0), p f32 (the prior
        after the root mix), child int32 (-1: no such edge) and, with value,
        value f64 [n] = sum W / sum N from the root mover's side.  One launch,
        no host read; the tensors are the handle's own, rewritten by the next
        call."""
        r = self._report.get("root")
        if r is None:
            z = self._zeros
            A = ACTION_SIZE
            r = self._report["root"] = {
                "n": z(torch.int32, self.n, A), "w": z(torch.float64, self.n, A), "q": z(torch.float64, self.n, A),
                "p": z(torch.float32, self.n, A), "child": z(torch.int32, self.n, A), "value": z(torch.float64, self.n)}
        nat.check(nat.lib().hz_mcts_root_edges(self._h, nat.ptr(r["n"]), nat.ptr(r["w"]), nat.ptr(r["q"]),
                                               nat.ptr(r["p"]), nat.ptr(r["child"]),
                                               nat.ptr(r["value"]) if value else None), "hz_mcts_root_edges")
        return dict(r) if value else {k: v for k, v in r.items() if k != "value"}

    def principal_variation(self, max_len=16):
        """The line each board's search expects (hz_mcts_pv): at every node
        the first edge with the most visits, until a node without edges, an
        edge without visits or max_len moves (1 <= max_len <= max_depth).
        Device tensors action int16 [n, max_len] (-1 past the end), visits
        int32, q f64 (the edge's W / N), player uint8 (the edge's mover) and
        len int32 [n]; the handle's own, rewritten by the next call with the
        same max_len."""
        max_len = int(max_len)
        if not 1 <= max_len <= self.max_depth:
            raise ValueError(f"max_len {max_len} outside 1..{self.max_depth}")
        r = self._report.get(("pv", max_len))
        if r is None:
            z = self._zeros
            r = self._report[("pv", max_len)] = {
                "action": z(torch.int16, self.n, max_len), "visits": z(torch.int32, self.n, max_len),
                "q": z(torch.float64, self.n, max_len), "player": z(torch.uint8, self.n, max_len),
                "len": z(torch.int32, self.n)}
        nat.check(nat.lib().hz_mcts_pv(self._h, max_len, nat.ptr(r["action"]), nat.ptr(r["visits"]), nat.ptr(r["q"]),
                                       nat.ptr(r["player"]), nat.ptr(r["len"])), "hz_mcts_pv")
        return dict(r)

    def export_tree(self, b):
        """Board b's tree as CPU numpy arrays (hz_mcts_export_tree), trimmed
        to its node and edge counts: state uint64 [nodes, 6], e0 / ne int32
        [nodes] (a node's first edge and edge count; ne -1: terminal, 0: not
        expanded), and per edge action int16, child int32, n int32, w f64,
        p f32, player uint8.  The debugging view: it waits for the device."""
        b = int(b)
        if not 0 <= b < self.n:
            raise IndexError(f"board {b} outside 0..{self.n - 1}")
        r = self._report.get("tree")
        if r is None:
            z = self._zeros
            m = self.max_nodes
            r = self._report["tree"] = {
                "state": z(torch.int64, m, 6), "e0": z(torch.int32, m), "ne": z(torch.int32, m),
                "action": z(torch.int16, m), "child": z(torch.int32, m), "n": z(torch.int32, m),
                "w": z(torch.float64, m), "p": z(torch.float32, m), "player": z(torch.uint8, m)}
        nat.check(nat.lib().hz_mcts_export_tree(self._h, b, *(nat.ptr(r[k]) for k in (
            "state", "e0", "ne", "action", "child", "n", "w", "p", "player"))), "hz_mcts_export_tree")
        nodes, edges = (int(x) for x in self.stats()[b, :2].tolist())
        out = {k: r[k][:nodes].cpu().numpy() for k in ("state", "e0", "ne")}
        out["state"] = out["state"].view("uint64")
        out.update({k: r[k][:edges].cpu().numpy() for k in ("action", "child", "n", "w", "p", "player")})
        return out

    # -- one full search per board -------------------------------------------
    def _step(self, evaluator, device_rows, cpuct, active, noise, eps, testing, max_rows=None):
        """One simulation as launches of its own (with a device-row evaluator: no host round trip)."""
        board, glob, rows, count = self.select_gather(cpuct, active)  # (adds count to eval_rows)
        policy, value = self._evaluate(evaluator, device_rows, board, glob, rows, count, max_rows)
        self.expand_backup(policy, value, noise, eps, testing, gathered=True)

    def _capture_step(self, evaluator, cpuct, active, eps, testing, max_rows=None):
        """One simulation captured as a HIP graph (select, gather + encode,
        the evaluator's kernels, expand + backup): replaying it costs one
        launch instead of ~60.  Noise is passed as NULL: the kernel reads it
        only when it expands the root, which the first (eager) simulation does
        (hz_mcts.hip k_expand_backup: noisy = leaf == 0 && !testing && noise).

        Replay constraint: the graph bakes in the split tower's counter block
        of its capture stream, and capture streams come from PyTorch's stream
        pool, so two handles may share one block.  Replays of captured
        simulations must therefore run one at a time (search() replays on the
        caller's stream, in order); replaying two handles' graphs
        concurrently on different streams would corrupt the hand-off
        counters."""
        g = torch.cuda.CUDAGraph()
        if self._capture_stream is None:
            self._capture_stream = torch.cuda.Stream(self.device)
        # the split tower's counter block for this stream, zeroed now: created
        # inside the capture, its zero-fill would be a graph node replayed
        # with every simulation (hzamd.infer._split_sync)
        from .infer import _split_sync
        _split_sync(self.device, self._capture_stream)
        try:
            with torch.cuda.graph(g, stream=self._capture_stream):
                self._sync()  # the handles launch on the capture stream
                self._step(evaluator, True, cpuct, active, None, eps, testing, max_rows)
        finally:
            self._sync()  # back on the caller's stream, captured or not
        return g

    def search(self, evaluator, cpuct, active=None, noise=None, eps=0.25, testing=True, sims=None,
               gather=True, graph=False, max_rows=None, budget=None, root_noise=None, tail=None, carry=False,
               root=None, gumbel=None, max_considered=None, c_visit=None, c_scale=None, leaf_symmetry=None,
               forced=None, forced_k=None):
        """get_best_action_and_pi's simulation loop (MCTS.py:288-352) for every
        active board; returns root visit counts int32 [n, 143].

        gather (default): each simulation evaluates only the leaves that need
        the network (module docstring); `eval_rows` counts them on the device.
        gather=False evaluates one row per board (terminal leaves and inactive
        boards included, their results unused), as before.

        graph: simulations 2.. replay one captured HIP graph, for small,
        launch-bound batches (the arena's few dozen boards); taken only with
        a device-row evaluator that declares `capturable = True` (no host
        reads, no allocations outside PyTorch's allocator), as
        BatchedPredictor does for the folded network; otherwise ignored.

        max_rows (host int, device-row evaluators): an upper bound on the
        leaves a simulation can gather (e.g. the number of active boards);
        the evaluator then gets the first max_rows rows of the buffers, so
        its kernels are sized (and the small-batch conv form chosen) by it.
        A bound below a simulation's leaves is an error, not a read past the
        evaluator's outputs: NativeError at the end of the search.

        budget (int32 [n], optional): board b gets min(budget[b], sims)
        simulations (hz_mcts_set_budget) and is, bit for bit, the search of
        that many; sims_done() has the counts.  None: no gate (a handle
        reused after a budgeted search searches in full).
        root_noise (bool / uint8 [n], optional): the root mix only where set;
        a board with 0 searches as testing=True does.

        tail = (s0, k) (host ints, device-row evaluators): the caller's promise
        that from simulation s0 on (counted from 0) at most k leaves are live,
        e.g. once every board of a smaller budget is spent; from there the
        evaluator gets the first min(max_rows, k) rows.  With graph=True the
        tail is a second captured simulation.  A broken promise raises like a
        wrong max_rows.

        carry: start from the trees the last advance() kept (begin_carried)
        instead of empty ones; `sims` (or the budgets) count the new
        simulations, the visits returned include the carried ones.  The
        simulations themselves are the same launches in every search form.

        root="gumbel" with gumbel=G (f64 [n, 69], one Gumbel per board and
        legal rank: NoiseSource.gumbel): the root's choice is sequential
        halving over the top max_considered actions by G + log P (+ sigma of
        the completed Q, constants c_visit and c_scale; hz_mcts_set_gumbel
        states the rule), for a search of `sims` simulations; below the root
        the search is PUCT as always.  gumbel_result() then has the move, the
        improved policy and v_mix; the visits returned are the search's.  In
        every search form; not with noise=, root_noise=, budget=, tail= or
        carry=True (ValueError).  A search without root= clears the gate.

        leaf_symmetry=keys (int64 / uint64 [n] on the device, one key per
        board: NoiseSource.leaf_symmetry): every leaf is evaluated under one
        of the board's four symmetries, g a function of the board's key and
        the leaf's node id (hz_mcts_set_leaf_symmetry states the rule): the
        network sees the leaf's image and the expansion reads the priors back
        through g; the walk, the children, the draws and the backup are what
        they are without it.  In every search form, with active=, budget=,
        root_noise=, tail= and max_rows=; not with root="gumbel" or
        carry=True (ValueError).  A search without it clears the gate.

        forced=True, or a bool / uint8 [n] mask, with forced_k=k (default 2,
        KataGo's): forced playouts at the root of the boards whose flag is
        set (hz_mcts_set_forced states the rule): a root child that has been
        visited is owed sqrt(k P sum N) visits and is chosen ahead of PUCT
        until it has them; everything else is the search it is without it.
        pruned_visits(cpuct) then has the visits with the merely forced ones
        taken back; the visits returned are the raw ones.  In every search
        form, with active=, budget=, root_noise=, tail=, max_rows= and
        leaf_symmetry=; not with root="gumbel" or carry=True (ValueError).  A
        search without it clears the gate."""
        total = self.num_simulations if sims is None else int(sims)
        if active is not None:
            active = active.to(device=self.device, dtype=torch.uint8).contiguous()
        self._open(total, budget, root_noise, noise, tail, carry, root, gumbel, max_considered, c_visit, c_scale,
                   leaf_symmetry, forced, forced_k)
        if carry:
            self.begin_carried(active, noise, eps, testing)
            if self.count_edges:
                self._edges_base = self.stats()[:, 1].sum(dtype=torch.int64)
            if self.count_path:  # the carried trees' edge visits: levels earlier searches walked
                self._path_base = torch.zeros(1, dtype=torch.int64, device=self.device)
                nat.check(nat.lib().hz_mcts_path_edges(self._h, nat.ptr(self._path_base)), "hz_mcts_path_edges")
        else:
            self.begin(active)
        device_rows = bool(getattr(evaluator, "device_rows", False))
        s0, tail_rows = total, max_rows
        if tail is not None and device_rows:
            s0 = max(0, int(tail[0]))
            tail_rows = max(1, min(self.n if max_rows is None else int(max_rows), int(tail[1])))
        run = (evaluator, cpuct, active, noise, eps, testing, total, max_rows, s0, tail_rows)
        if graph and gather and device_rows and getattr(evaluator, "capturable", False) and total > 1:
            self._run_graph(*run)
        elif gather and total > 1 and self.n > 32 and self.fuse_select:
            self._run_fused(*run, device_rows)
        else:
            self._run_layered(*run, device_rows, gather)
        return self._finish()

    def _open(self, total, budget=None, root_noise=None, noise=None, tail=None, carry=False, root=None, gumbel=None,
              max_considered=None, c_visit=None, c_scale=None, leaf_symmetry=None, forced=None, forced_k=None):
        """Opens a search of `total` simulations, closed by _finish(): ValueError for a combination of search()'s
        arguments that does not exist, every gate set or cleared in stream order, the per-search counters reset."""
        if forced is False:
            forced = None
        if forced is not None and (root == "gumbel" or carry):
            raise ValueError("forced= does not combine with root='gumbel' or carry=True")
        if forced is None and forced_k is not None:
            raise ValueError("forced_k= goes with forced=")
        if leaf_symmetry is not None and (root == "gumbel" or carry):
            raise ValueError("leaf_symmetry= does not combine with root='gumbel' or carry=True")
        if root not in (None, "gumbel"):
            raise ValueError(f"root {root!r}: not None or 'gumbel'")
        if root is None and (gumbel is not None or max_considered is not None or c_visit is not None or
                             c_scale is not None):
            raise ValueError("gumbel=, max_considered=, c_visit= and c_scale= go with root='gumbel'")
        if root == "gumbel":
            if gumbel is None:
                raise ValueError("root='gumbel' needs gumbel= (NoiseSource.gumbel)")
            if noise is not None or root_noise is not None or budget is not None or tail is not None or carry:
                raise ValueError("root='gumbel' does not combine with noise=, root_noise=, budget=, tail= or carry=True")
        self._sync()
        self._gate = self._gate._replace(gumbel=self._set_gumbel(gumbel, total, max_considered, c_visit, c_scale),
                                         leaf_sym=self._set_leaf_symmetry(leaf_symmetry),
                                         forced=self._set_forced(forced, forced_k))
        self._set_gate(budget, root_noise)
        self._edges_base = self._path_base = None
        self.eval_rows.zero_()
        self._cap_risk = False

    def _run_graph(self, evaluator, cpuct, active, noise, eps, testing, total, max_rows, s0, tail_rows):
        """The first simulation eager, the others replays of one captured simulation (two with a tail)."""
        self._step(evaluator, True, cpuct, active, noise, eps, testing, max_rows if s0 > 0 else tail_rows)
        # an evaluator with a graph_key (the network object and its weight generation) lets the captured
        # simulation be kept for the next search with the same settings (the drop-in's one search per move);
        # only without an `active` mask, whose tensor the graph would bake in
        gk = getattr(evaluator, "graph_key", None)
        # (a capture holds the handle by value: whether each gate and each mask, the forced gate's too, are on,
        # and each step's row cap, belong to the key)
        head = min(max(s0 - 1, 0), total - 1)  # replays before the tail (simulation 0 ran eagerly)
        steps = ((max_rows, head), (tail_rows, total - 1 - head))
        key = None if gk is None or active is not None else (
            id(gk[0]), gk[1], float(cpuct), float(eps), bool(testing), self._gate)
        cached = self._graph_cache
        if key is None or cached is None or cached[0] != key:
            cached = self._graph_cache = None
        graphs = {} if cached is None else cached[1]
        wanted = {rows for rows, times in steps if times}
        if len(wanted | set(graphs)) > 4:  # (row bounds that change from search to search: keep a few)
            for rows in set(graphs) - wanted:
                del graphs[rows]
        for rows, times in steps:
            if times and rows not in graphs:
                graphs[rows] = self._capture_step(evaluator, cpuct, active, eps, testing, rows)
        if key is not None and cached is None:
            self._graph_cache = (key, graphs, gk[0])  # holds the network: its id stays unique
        for rows, times in steps:
            if times and rows is not None and rows < self.n:
                self._cap_risk = True  # (a cached capture: no expand call of this search set it)
            for _ in range(times):
                graphs[rows].replay()

    def _run_fused(self, evaluator, cpuct, active, noise, eps, testing, total, max_rows, s0, tail_rows, device_rows):
        """The next simulation's select rides in each expand/backup launch (and, fuse_gather, the gather + encode
        of its leaf batch: the two count buffers alternate, each zeroed by the launch after the one that filled
        it, so both are zero between searches)."""
        # rows in arrival order only for an evaluator that opts in: one
        # that maps rows to boards by position, or whose results depend on
        # a row's place in the batch, keeps the board-order gather
        fuse_gather = self.fuse_gather and bool(getattr(evaluator, "row_independent", False))
        if fuse_gather:
            self.count_b.zero_()  # (defensive: a search cut short may have left it set)
        board, glob, rows, count = self.select_gather(cpuct, active)
        bufs, cur = (self.count, self.count_b), 0
        for s in range(total):
            policy, value = self._evaluate(evaluator, device_rows, board, glob, rows, count,
                                           max_rows if s < s0 else tail_rows)
            if s + 1 < total:
                if fuse_gather:
                    self.expand_backup_select_gather(policy, value, cpuct, active, noise, eps, testing,
                                                     bufs[cur ^ 1], bufs[cur], add_prev=s > 0)
                    cur ^= 1
                    count = bufs[cur]
                else:
                    self.expand_backup_select(policy, value, cpuct, active, noise, eps, testing)
                    board, glob, rows, count = self.gather_leaves()
            else:
                self.expand_backup(policy, value, noise, eps, testing, gathered=True)
        if fuse_gather:  # the last batch's count: no gather call added it
            self.eval_rows += count
            count.zero_()

    def _run_layered(self, evaluator, cpuct, active, noise, eps, testing, total, max_rows, s0, tail_rows, device_rows,
                     gather):
        """Every simulation its own launches; gather=False: one row per board."""
        for s in range(total):
            if not gather:
                self.select(cpuct, active)
                board, glob = self.encode_leaves()
                policy, value = evaluator(board, glob)
                self.eval_rows += self.n
                self.expand_backup(policy, value, noise, eps, testing)
                continue
            self._step(evaluator, device_rows, cpuct, active, noise, eps, testing, max_rows if s < s0 else tail_rows)

    def _evaluate(self, evaluator, device_rows, board, glob, rows, count, max_rows):
        if device_rows:
            if max_rows is not None:  # the live rows are a prefix of at most max_rows
                board, glob = board[:max_rows], glob[:max_rows]
            return evaluator(board, glob, rows, count)
        k = int(count.item())  # one host read per simulation
        if k:
            return evaluator(board[:k], glob[:k])
        return self._nil_pol, self._nil_val

    def _finish(self, trees=True):
        """Closes what _open() opened: root visits of the search just run, after making sure no leaf evaluation of
        it went through a timed-out split-tower hand-off (whose NaN priors would have steered PUCT silently):
        NativeError if one did; and, where an expand call had fewer rows than boards, that no board's row lay past
        them (the handle's error word: one read per search).  trees=False (play_async, whose trees are not one
        search's): no counter read from the trees, no visits."""
        from .infer import check_split_timeouts
        self.eval_rows_total += self.eval_rows
        if trees and self.count_edges:
            self.edges_total += self.stats()[:, 1].sum(dtype=torch.int64)
            if self._edges_base is not None:  # a carried search: only the edges it created
                self.edges_total -= self._edges_base
        if trees and self.bounded:
            c = self.stats()  # (a board left out of this search has no nodes and keeps its last flag)
            self.limit_hits_total += ((c[:, 3] != 0) & (c[:, 0] > 0)).sum(dtype=torch.int64)
        if trees and self.count_path:
            nat.check(nat.lib().hz_mcts_path_edges(self._h, nat.ptr(self.path_total)), "hz_mcts_path_edges")
            if self._path_base is not None:  # a carried search: only the levels it walked
                self.path_total -= self._path_base
        visits = self.result() if trees else None
        if self._cap_risk:
            self._cap_risk = False
            word = ctypes.c_int32(0)
            nat.check(nat.lib().hz_mcts_take_error(self._h, ctypes.byref(word)), "hz_mcts_take_error")
            if word.value:  # (cleared by the call: the next search starts clean)
                raise nat.NativeError("leaf batch larger than the evaluator's rows")
        check_split_timeouts(self.device)
        return visits


def choose_actions(visits, explore, u):
    """Move choice of get_best_action_and_pi (MCTS.py:394-423) from root visit
    counts (edges are in ascending action order, as the search inserts them):
    explore[b] -> sample proportional to N with the uniform u[b] (first action
    whose cumulative count exceeds u * total); else the first action with the
    most visits.  Returns int64 [n] (-1 when a board has no visits)."""
    v = visits.to(torch.int64)
    total = v.sum(1)
    greedy = torch.argmax(v, dim=1)
    cum = v.cumsum(1)
    target = u.to(torch.float64) * total.to(torch.float64)
    sampled = torch.argmax((target.unsqueeze(1) < cum.to(torch.float64)).to(torch.int32), dim=1)
    act = torch.where(explore.to(torch.bool), sampled, greedy)
    return torch.where(total > 0, act, torch.full_like(act, -1))


def choose_actions_native(visits, explore, u):
    """choose_actions in one launch (hz_choose_actions: the rule the turn of
    SelfPlay.play_async applies to its trees): int16 [n] on the device."""
    n = visits.shape[0]
    d = visits.device
    if visits.shape != (n, ACTION_SIZE):
        raise ValueError(f"visits of shape {tuple(visits.shape)}, not (n, {ACTION_SIZE})")
    visits = visits.to(torch.int32).contiguous()
    explore = explore.to(device=d, dtype=torch.uint8).contiguous()
    u = u.to(device=d, dtype=torch.float64).contiguous()
    if explore.shape != (n,) or u.shape != (n,):
        raise ValueError("explore and u: one entry per board")
    act = torch.empty(n, dtype=torch.int16, device=d)
    nat.check(nat.lib().hz_choose_actions(nat.ptr(visits), n, nat.ptr(explore), nat.ptr(u), nat.ptr(act),
                                          nat.stream_ptr(d)), "hz_choose_actions")
    return act


def pi_from_visits(visits):
    """pi_target = N / sum(N) in float64, stored as float32 by the trainer
    (MCTS.py:378-381, trainer.py:531)."""
    v = visits.to(torch.float64)
    tot = v.sum(1, keepdim=True)
    return torch.where(tot > 0, v / tot.clamp_min(1), torch.zeros_like(v)).to(torch.float32)


class BatchedPredictor:
    """ModelManager.predict (model.py:81-110) for a whole batch: eval mode,
    no grad, softmax over all 143 logits (illegal moves are not masked).
    Called by BatchedMCTS with the device row count (device_rows): the
    folded net's HIP kernels compute only the live rows.
    tower: the folded net's tower mode (FoldedNet.TOWER_MFMA; None: HZ_TOWER,
    else "x6")."""

    device_rows = True

    def __init__(self, model, dtype=None, fold=True, tower=None):
        self.model = model
        self.dtype = dtype
        # eval-mode BatchNorm folded into the convs (hzamd.infer): same fp32
        # arithmetic up to rounding, ~3x faster on MI355X at batch 4096
        self.fast = None
        if fold and hasattr(model, "residual_blocks"):
            from .infer import FoldedNet
            self.fast = FoldedNet(model, tower=tower)
        # the folded fp32 path is HIP kernels + PyTorch ops only: it can be
        # captured in a HIP graph (BatchedMCTS.search(graph=True))
        self.capturable = self.fast is not None and (dtype is None or dtype == torch.float32)
        # the folded kernels compute every row on its own, in one summation
        # order whatever the batch (test_predict_rows_do_not_depend_on_batch_size);
        # the PyTorch/MIOpen path makes no such promise, nor do the unfused
        # head's F.linear layers (FoldedNet.row_independent)
        self.row_independent = self.capturable and self.fast.row_independent

    def refresh(self):
        """Re-fold after the model's weights changed."""
        if self.fast is not None:
            self.fast.refresh()

    @torch.no_grad()
    def __call__(self, board, glob, rows=None, count=None):
        self.model.eval()
        low = self.dtype is not None and self.dtype != torch.float32
        # the folded net's HIP kernels are fp32-only; autocast runs the source
        # net (on every row: it has no live-row bound)
        if low:
            with torch.autocast(device_type="cuda", dtype=self.dtype):
                logits, value = self.model(board, glob)
        elif self.fast is not None:
            return self.fast.predict(board, glob, live=count)
        else:
            logits, value = self.model(board, glob)
        return torch.softmax(logits.float(), dim=1), value.float().reshape(-1)


def _stub_key(board, glob):
    """The integer key K both stub evaluators hash (int64 [k])."""
    n0 = torch.round(board[:, 0:18].double().sum((1, 2, 3))).long()
    n1 = torch.round(board[:, 18:36].double().sum((1, 2, 3))).long()
    cp = torch.round(board[:, 36].amax((1, 2))).long()
    ph3 = torch.round(board[:, 37].amax((1, 2)) * 3.0).long()
    pc = torch.round(glob[:, 0:36].double() * 3.0).long()
    w = (pc * torch.arange(1, 37, device=board.device, dtype=torch.int64)).sum(1)
    return (n0 * 73 + n1 * 151 + ph3 * 7 + cp * 3 + w * 13) % (1 << 31)


def stub_evaluator(board, glob):
    """Deterministic integer-valued evaluator used by the parity tests; the
    same formula as tests/golden/make_golden.py:stub_predict_np, so the GPU
    search and the reference search see identical priors and values."""
    K = _stub_key(board, glob)
    a = torch.arange(ACTION_SIZE, device=board.device, dtype=torch.int64)
    h = (a.unsqueeze(0) * 2654435761 + K.unsqueeze(1) * 40503) % (1 << 32)
    pol = ((h >> 22) + 1).to(torch.float32) / 1024.0
    val = ((K % 255) - 127).to(torch.float64) / 128.0
    return pol, val.to(torch.float32)


stub_evaluator.row_independent = True  # a function of each row alone


def dense_stub_evaluator(board, glob):
    """The second parity evaluator (tests/golden/make_golden.py:
    dense_stub_predict_np): where the stub's priors are k/1024 and its values
    k/128, so that the search arithmetic is exact in any precision, these
    priors have full 24-bit significands over twenty binades, in ladders of
    three actions one fp32 ulp apart, one triple in 32 exactly zero, and the
    values are signed 24-bit integers times 2^-23, three in four of them
    within eight ulps of +-1.  Integers converted and
    scaled by powers of two only: the same bits in NumPy, C and torch."""
    K = _stub_key(board, glob)
    a = torch.arange(ACTION_SIZE, device=board.device, dtype=torch.int64)
    r = a % 3
    hg = ((a - r).unsqueeze(0) * 2654435761 + K.unsqueeze(1) * 40503) % (1 << 32)
    low = hg & 31
    mant = (1 << 23) + ((hg >> 9) & ~3) + r.unsqueeze(0)
    # 2^-(24+s) from its fp32 bit pattern (exponent field 127 - 24 - s): device
    # integer ops only, so the evaluator can be captured in a HIP graph
    scale = ((103 - low % 20) << 23).to(torch.int32).view(torch.float32)
    pol = mant.to(torch.float32) * scale
    pol = torch.where(low == 31, torch.zeros_like(pol), pol)
    hv = (K * 2246822519) % (1 << 32)
    j = (hv >> 4) & 7
    sat = torch.where((hv & 8) != 0, j - (1 << 23), (1 << 23) - 1 - j)
    vi = torch.where((hv & 7) < 6, sat, (hv >> 8) - (1 << 23))
    return pol, vi.to(torch.float32) * (2.0 ** -23)


dense_stub_evaluator.row_independent = True
