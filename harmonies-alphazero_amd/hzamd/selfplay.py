"""Batched self-play: `self_play_worker` (trainer.py:434-541) for n boards at
once on one GPU.

Per ply, for every board still playing: record the state and the player to
move, run get_best_action_and_pi's search (BatchedMCTS, one PyTorch leaf
batch per simulation), choose the move (tau = 1 sampling for the first
`turns_until_tau0` plies unless testing, else the first most-visited move),
apply it (HIP step, chance draws from the board's CPython stream).  When a
board's game ends its examples get z = outcome from the recorded player's
perspective (trainer.py:517-538).

Records stay on the device in compact form: state words int64 [T, 6, n],
player int8 [T, n], visit counts int32 [T, n, 143], valid bool [T, n].
`examples()` turns them into the reference's example tuples
(board f32[38,5,7], glob f32[42], pi f32[143], z f32[1]).

Playout-cap randomization (no reference counterpart; config keys
`playout_cap_p` and `playout_cap_fast`, both absent by default): each move a
coin per board (NoiseSource.coin) decides whether the board is searched in
full (`num_simulations`, root noise; probability p) or fast
(`playout_cap_fast` simulations, no noise) through BatchedMCTS.search's
per-board budgets; the move is chosen as always, the records gain `full`,
and only the full moves become training records.

Tree reuse (no reference counterpart; config key `tree_reuse`, absent by
default): after each step the search handle keeps the subtree below the move
just played (BatchedMCTS.advance, whose rule include/hz_abi.h states) and the
next move's search starts from it.  "add" runs `num_simulations` new
simulations on top; "topup" gives board b
clamp(num_simulations - carried visits, tree_reuse_min_sims, num_simulations)
through the per-board budgets.  Visit counts and pi include the carried
visits; the records gain `carried`.

The Gumbel root (no reference counterpart; config key `root_policy`:
"gumbel", absent by default, with `gumbel_max_considered`, `gumbel_c_visit`,
`gumbel_c_scale`): the root of every search is sequential halving over the
top-m actions by Gumbel + log prior (BatchedMCTS.search(root="gumbel"), whose
rule include/hz_abi.h states) instead of PUCT with Dirichlet noise; the move
is the search's own at every ply, and the visit slots of the records hold the
improved policy as rint(pi' * 65535), so pi = N / sum N rebuilds it.

Leaf symmetries (no reference counterpart; config key `leaf_symmetry`:
"random", absent by default): every leaf of every search is evaluated under
one of the board's four symmetries, drawn per board and node from the move's
key (NoiseSource.leaf_symmetry, BatchedMCTS.search(leaf_symmetry=), whose rule
include/hz_abi.h states).  With playout caps; not with tree_reuse or
root_policy "gumbel".

Forced playouts and policy target pruning (no reference counterpart; config
key `forced_playouts`: KataGo's k, absent by default, with `prune_targets`,
default True): on the boards searched in full (every active board without
playout caps) a visited root child is owed sqrt(k P sum N) visits
(BatchedMCTS.search(forced=), whose rule include/hz_abi.h states); the move
is chosen from the raw visits (kept in `last_visits`), and the visits move()
returns and the records hold are the pruned ones
(BatchedMCTS.pruned_visits).  Off while `testing`; with playout caps and
leaf symmetries; not with tree_reuse or root_policy "gumbel".

The asynchronous schedule (no reference counterpart; SelfPlay.play_async,
and `schedule="async"` with `moves_per_board` in iteration() and the
trainer's self-play config, absent by default): play_steady without the
barrier between moves.  Every board keeps a move counter of its own, and a
board whose search is spent records, moves and begins its next search inside
the sim step (the turn: include/hz_abi.h), so boards with different budgets
never leave a sim step with idle rows; the records are play_steady's bit for
bit.  With playout caps on or off and `testing`; not with tree_reuse,
root_policy "gumbel", leaf_symmetry, forced_playouts or keep_root_value.
"""
import torch

from . import _native as nat
from .env import BatchedEnv
from .mcts import MAX_CHILDREN, BatchedMCTS, choose_actions, pi_from_visits

MCTS_DEFAULT = {  # config.py:53-65 (the self-play config)
    "num_simulations": 400, "cpuct": 2, "dirichlet_alpha": 0.4, "dirichlet_epsilon": 0.25,
    "fpu_value": 0.25, "turns_until_tau0": 15, "action_size": 143, "testing": False,
}


def topup_budgets(carried, num_simulations, min_sims):
    """The "topup" rule of tree reuse for one move: budget int32 [n] =
    clamp(num_simulations - carried visits, min_sims, num_simulations)."""
    left = int(num_simulations) - carried.to(torch.int64)
    return left.clamp(min(int(min_sims), int(num_simulations)), int(num_simulations)).to(torch.int32)


def playout_budgets(coin, p, full_sims, fast_sims):
    """The playout-cap rule for one move: (budget int32 [n], full bool [n])
    from the boards' coins in (0, 1] (NoiseSource.coin).  A board is full iff
    its coin is below p (a coin equal to p is not), and every board is at
    p >= 1; full boards get full_sims simulations, the others fast_sims."""
    full = coin < float(p) if float(p) < 1.0 else torch.ones_like(coin, dtype=torch.bool)
    budget = torch.where(full, int(full_sims), int(fast_sims)).to(torch.int32)
    return budget, full


def check_schedule(schedule, moves_per_board):
    """The self-play schedule keys (SelfPlay.iteration, Trainer's
    self_play_config): schedule None (a game per board, the barrier schedule)
    takes no moves_per_board; "async" (SelfPlay.play_async) needs a positive
    integer.  Returns moves_per_board as an int, or None."""
    if schedule not in (None, "async"):
        raise ValueError(f"schedule {schedule!r}: not None or 'async'")
    if schedule is None:
        if moves_per_board is not None:
            raise ValueError("moves_per_board goes with schedule 'async'")
        return None
    if isinstance(moves_per_board, bool) or not isinstance(moves_per_board, int) or moves_per_board < 1:
        raise ValueError(f"schedule 'async' needs moves_per_board, a positive integer, not {moves_per_board!r}")
    return moves_per_board


class NoiseSource:
    """Root Dirichlet noise (MCTS.py:314-316) and the tau=1 uniforms, drawn on
    the device by hz_root_noise from a counter-based generator keyed by
    (seed, global board id = board_base + b, move counter): a board's draws
    are the same whatever batch it sits in and whatever the GPU count."""

    def __init__(self, board_base, device, seed=0):
        self.board_base = int(board_base)
        self.seed = int(seed)
        self.device = torch.device(device)

    def draw(self, step, counts, alpha):
        n = counts.numel()
        counts = counts.to(device=self.device, dtype=torch.int32).contiguous()
        noise = torch.empty(n, MAX_CHILDREN, dtype=torch.float64, device=self.device)
        u = torch.empty(n, dtype=torch.float64, device=self.device)
        nat.check(nat.lib().hz_root_noise(nat.ptr(counts), n, self.seed & (2**64 - 1),
                                          self.board_base & (2**64 - 1), int(step) & (2**64 - 1), float(alpha),
                                          nat.ptr(noise), nat.ptr(u), nat.stream_ptr(self.device)),
                  "hz_root_noise")
        return noise, u

    def coin(self, step, n):
        """One uniform in (0, 1] per board under the same key (hz_playout_coin),
        f64 [n] on the device: move `step`'s coin for playout-cap
        randomization; the noise and u of draw() do not depend on it."""
        coin = torch.empty(n, dtype=torch.float64, device=self.device)
        nat.check(nat.lib().hz_playout_coin(n, self.seed & (2**64 - 1), self.board_base & (2**64 - 1),
                                            int(step) & (2**64 - 1), nat.ptr(coin), nat.stream_ptr(self.device)),
                  "hz_playout_coin")
        return coin

    def _at_args(self, moves, mask, n):
        if not torch.is_tensor(moves) or moves.dtype not in (torch.int64, torch.uint64) or moves.shape != (n,):
            raise ValueError("moves: an int64 / uint64 tensor of one move counter per board")
        if not torch.is_tensor(mask) or mask.shape != (n,):
            raise ValueError("mask: one flag per board")
        return (moves.to(device=self.device).contiguous(),
                mask.to(device=self.device, dtype=torch.uint8).contiguous())

    def draw_at(self, moves, counts, alpha, mask, noise_out, u_out):
        """The per-board-counter form of draw() (hz_root_noise_at): where
        mask[b] == 1, row b of noise_out (f64 [n, 69]) and u_out[b] (f64 [n])
        get the bits draw(moves[b], ...) gives board b; every other row keeps
        what it holds.  moves: int64 / uint64 [n] on the device."""
        n = counts.numel()
        moves, mask = self._at_args(moves, mask, n)
        counts = counts.to(device=self.device, dtype=torch.int32).contiguous()
        for t, shape, name in ((noise_out, (n, MAX_CHILDREN), "noise_out"), (u_out, (n,), "u_out")):
            if (not torch.is_tensor(t) or t.dtype != torch.float64 or tuple(t.shape) != shape or
                    not t.is_contiguous() or t.device.type != self.device.type):
                raise ValueError(f"{name}: a contiguous float64 tensor of shape {shape} on {self.device}")
        nat.check(nat.lib().hz_root_noise_at(nat.ptr(counts), n, self.seed & (2**64 - 1),
                                             self.board_base & (2**64 - 1), nat.ptr(moves), nat.ptr(mask),
                                             float(alpha), nat.ptr(noise_out), nat.ptr(u_out),
                                             nat.stream_ptr(self.device)), "hz_root_noise_at")

    def coin_at(self, moves, mask, coin_out):
        """The per-board-counter form of coin() (hz_playout_coin_at): where
        mask[b] == 1, coin_out[b] (f64 [n]) gets board b's coin of move
        moves[b]; every other entry keeps what it holds."""
        n = coin_out.numel()
        moves, mask = self._at_args(moves, mask, n)
        if coin_out.dtype != torch.float64 or coin_out.dim() != 1 or not coin_out.is_contiguous() or \
                coin_out.device.type != self.device.type:
            raise ValueError(f"coin_out: a contiguous float64 tensor of shape ({n},) on {self.device}")
        nat.check(nat.lib().hz_playout_coin_at(n, self.seed & (2**64 - 1), self.board_base & (2**64 - 1),
                                               nat.ptr(moves), nat.ptr(mask), nat.ptr(coin_out),
                                               nat.stream_ptr(self.device)), "hz_playout_coin_at")

    def gumbel(self, step, n):
        """One standard Gumbel per board and legal rank under the same key
        (hz_root_gumbel), f64 [n, 69] on the device: move `step`'s draws for
        BatchedMCTS.search(root="gumbel"); draw() and coin() do not depend on it."""
        g = torch.empty(n, MAX_CHILDREN, dtype=torch.float64, device=self.device)
        nat.check(nat.lib().hz_root_gumbel(n, self.seed & (2**64 - 1), self.board_base & (2**64 - 1),
                                           int(step) & (2**64 - 1), nat.ptr(g), nat.stream_ptr(self.device)),
                  "hz_root_gumbel")
        return g

    def leaf_symmetry(self, step, n):
        """One 64-bit key per board under the same key (hz_leaf_sym_keys),
        int64 [n] on the device: move `step`'s keys for
        BatchedMCTS.search(leaf_symmetry=); draw(), coin() and gumbel() do not
        depend on it."""
        keys = torch.empty(n, dtype=torch.int64, device=self.device)
        nat.check(nat.lib().hz_leaf_sym_keys(n, self.seed & (2**64 - 1), self.board_base & (2**64 - 1),
                                             int(step) & (2**64 - 1), nat.ptr(keys), nat.stream_ptr(self.device)),
                  "hz_leaf_sym_keys")
        return keys


class SelfPlay:
    def __init__(self, n_boards, evaluator, mcts_config=None, seed_base=0, device="cuda", max_plies=200,
                 env=None, exact_keys=False, keep_root_value=False):
        self.cfg = dict(MCTS_DEFAULT, **(mcts_config or {}))
        self.device = torch.device(device)
        self.env = env or BatchedEnv(n_boards, seed_base=seed_base, device=self.device)
        self.n = self.env.n
        self.evaluator = evaluator
        # tree reuse: on when the key is given; the pools get room for a carried tree
        # next to a whole search (a kept tree that leaves less is dropped, so no search overflows)
        self.tree_reuse = self.cfg.get("tree_reuse")
        if self.tree_reuse not in (None, "add", "topup"):
            raise ValueError(f"tree_reuse {self.tree_reuse!r}: not 'add' or 'topup'")
        self.reuse_min_sims = int(self.cfg.get("tree_reuse_min_sims", 1))
        pool = float(self.cfg.get("tree_reuse_pool", 2.0))
        if self.tree_reuse and (pool < 1.0 or self.reuse_min_sims < 0):
            raise ValueError("tree_reuse_pool below 1 or a negative tree_reuse_min_sims")
        if self.tree_reuse and (self.cfg.get("playout_cap_p") is not None or
                                self.cfg.get("playout_cap_fast") is not None):
            raise ValueError("tree_reuse and playout caps do not combine")
        # the Gumbel root: on when root_policy is "gumbel" (absent: PUCT with Dirichlet noise, as always)
        policy = self.cfg.get("root_policy")
        if policy not in (None, "puct", "gumbel"):
            raise ValueError(f"root_policy {policy!r}: not 'puct' or 'gumbel'")
        self.gumbel = None
        if policy == "gumbel":
            if self.tree_reuse or self.cfg.get("playout_cap_p") is not None or \
                    self.cfg.get("playout_cap_fast") is not None:
                raise ValueError("root_policy 'gumbel' does not combine with playout caps or tree_reuse")
            self.gumbel = {"max_considered": self.cfg.get("gumbel_max_considered"),
                           "c_visit": self.cfg.get("gumbel_c_visit"), "c_scale": self.cfg.get("gumbel_c_scale")}
        # leaf symmetries: on when leaf_symmetry is "random" (absent: every leaf in the orientation it was played in)
        self.leaf_symmetry = self.cfg.get("leaf_symmetry")
        if self.leaf_symmetry not in (None, "random"):
            raise ValueError(f"leaf_symmetry {self.leaf_symmetry!r}: not 'random'")
        if self.leaf_symmetry and (self.tree_reuse or policy == "gumbel"):
            raise ValueError("leaf_symmetry does not combine with tree_reuse or root_policy 'gumbel'")
        # forced playouts: on when forced_playouts (k) is given; the records then hold the pruned visits
        fk = self.cfg.get("forced_playouts")
        self.forced_k = None
        if fk is not None:
            if isinstance(fk, bool) or not isinstance(fk, (int, float)) or not float(fk) > 0.0:
                raise ValueError(f"forced_playouts {fk!r}: not a number above 0 (KataGo's k)")
            if self.tree_reuse or policy == "gumbel":
                raise ValueError("forced_playouts does not combine with tree_reuse or root_policy 'gumbel'")
            self.forced_k = float(fk)
        prune = self.cfg.get("prune_targets")
        if prune is not None and not isinstance(prune, bool):
            raise ValueError(f"prune_targets {prune!r}: not True or False")
        if prune and self.forced_k is None:
            raise ValueError("prune_targets goes with forced_playouts")
        self.prune_targets = self.forced_k is not None and prune is not False
        self.last_visits = None  # int32 [n, 143] of the last move(): the raw visits the move was chosen from
        self.last_gumbel = None  # gumbel_result() of the last move(), with the Gumbel root
        max_nodes = int(pool * (1 + MAX_CHILDREN * self.cfg["num_simulations"])) if self.tree_reuse else None
        self.mcts = BatchedMCTS(self.env, self.cfg["num_simulations"], max_nodes=max_nodes, exact_keys=exact_keys)
        self._carried = None  # (state words after the last step, the visits advance() kept), with tree reuse
        self.last_carried = None  # int32 [n] of the last move(): the root visits its search started with
        self.max_plies = int(max_plies)
        self.noise = NoiseSource(seed_base, self.device)
        self.keep_noise = False
        # keep_root_value: each move() also takes the searches' root value
        # (BatchedMCTS.root_edges()["value"]: sum W / sum N over the root's
        # edges, from the root mover's side; one more launch, no host read)
        # into last_root_value, and play() / play_steady() record it
        self.keep_root_value = bool(keep_root_value)
        self.last_root_value = None  # f64 [n] of the last move() (the search handle's buffer), when kept
        self.noise_log = []
        self.step_counter = 0
        # move() holds the host back only after its search is queued: the
        # previous move's step status and active-board count come back
        # through a pinned buffer and an event recorded after that step
        self._n_active = self.n  # an upper bound on the active boards (sizes the network's launches) ...
        self._n_active_epoch = -1  # ... while the env's epoch (no game started since) is this
        self._flags = torch.zeros(3, dtype=torch.int64, pin_memory=self.device.type == "cuda")
        self._flags_ev = None
        self._bad_dev = None
        # playout caps: on when both keys are given
        p, fast = self.cfg.get("playout_cap_p"), self.cfg.get("playout_cap_fast")
        if (p is None) != (fast is None):
            raise ValueError("playout_cap_p and playout_cap_fast go together")
        self.playout_cap = None if p is None else (float(p), int(fast))
        if self.playout_cap and not (0.0 <= self.playout_cap[0] <= 1.0 and self.playout_cap[1] >= 0):
            raise ValueError(f"playout cap {self.playout_cap}: p outside 0..1 or a negative fast budget")
        self.last_full = None  # bool [n] of the last move(): searched in full
        # full boards of coming moves by move counter, an upper bound each (the
        # coin of move k + 2 is drawn at move k and its count rides in _flags)
        self._full_bound = {}
        self._flags_full_step = None

    def move(self, ply, done=None, _bound=None):
        """One ply for every board that is still playing: search, choose,
        step.  Returns (state words before the move, visits, active mask).

        A step failure of this move is reported by the next move() or by
        check_steps(): a caller that stops after a move must end with
        check_steps().  `done` (optional) is the caller's finished-board mask;
        the network's launches are then sized for every board, since the
        active-board bound kept from the last step holds only for the env's
        own done() (play() passes its bound for the mask it computed)."""
        env, n, d, cfg = self.env, self.n, self.device, self.cfg
        testing = bool(cfg.get("testing", False))
        if done is None:
            done = env.done()
            bound = self._active_bound()  # done() only shrinks the active set between resets
        else:
            bound = n if _bound is None else int(_bound)
        active = ~done
        st = env.export_state()
        if self.gumbel is not None:
            return self._gumbel_move(st, active, bound)
        _, count = env.legal_mask()
        noise, u = self.noise.draw(self.step_counter, count, cfg["dirichlet_alpha"])
        self.step_counter += 1
        # the leaf batch holds at most one row per active board: size the
        # network's launches by that (late in the games most boards are done);
        # an upper bound from an earlier move, so no host read waits here
        step = self.step_counter - 1  # this move's counter
        budget = full = tail = None
        if self.playout_cap:
            p, fast = self.playout_cap
            budget, full = playout_budgets(self.noise.coin(step, n), p, cfg["num_simulations"], fast)
            # once the fast boards are spent only full boards have leaves
            k = self._full_bound.pop(step, None)
            if k is not None and fast < cfg["num_simulations"]:
                tail = (fast, k)
            self.last_full = full
        if self.tree_reuse:
            # the visits carried into this search: the last advance()'s, where the
            # board still is in the state that step left (the handle makes the same
            # check: a reset or import in between starts the board fresh)
            if self._carried is None:
                carried = torch.zeros(n, dtype=torch.int32, device=d)
            else:
                same = (st == self._carried[0]).all(0) & active
                carried = torch.where(same, self._carried[1], torch.zeros_like(self._carried[1]))
            self.last_carried = carried
            if self.tree_reuse == "topup":
                budget = topup_budgets(carried, cfg["num_simulations"], self.reuse_min_sims)
        keys = self.noise.leaf_symmetry(step, n) if self.leaf_symmetry else None
        # forced playouts: the boards searched in full (every searched board without caps); off while testing
        forced = None
        if self.forced_k is not None and not testing:
            forced = full if full is not None else True
        v = self.mcts.search(self.evaluator, cfg["cpuct"], active=active, noise=noise,
                             eps=cfg["dirichlet_epsilon"], testing=testing, max_rows=max(1, bound),
                             budget=budget, root_noise=full, tail=tail, carry=self.tree_reuse is not None,
                             leaf_symmetry=keys, forced=forced, forced_k=self.forced_k if forced is not None else None)
        self.last_visits = v
        if self.keep_root_value:
            self.last_root_value = self.mcts.root_edges()["value"]
        self.check_steps()  # the previous move's step, done long before this search runs
        if torch.is_tensor(ply):
            explore = (ply < cfg["turns_until_tau0"]) & (not testing)
        else:
            explore = torch.full((n,), (not testing) and ply < cfg["turns_until_tau0"], dtype=torch.bool, device=d)
        act = choose_actions(v, explore, u)
        if self.keep_noise:
            self.noise_log.append((noise.clone(), u.clone(), act.clone()))
        self._step(act, active, step)
        if forced is not None and self.prune_targets:  # the move came from the raw visits; the records get the pruned
            v = self.mcts.pruned_visits(cfg["cpuct"])
        return st, v, active

    def _gumbel_move(self, st, active, bound):
        """move() with the Gumbel root (root_policy "gumbel"): no Dirichlet
        noise, the move is the search's own at every ply (the tau switch does
        not apply), and the visit slots of the records hold the improved
        policy as rint(pi' * 65535), so pi = N / sum N rebuilds pi' to within
        the quantisation.  keep_root_value records the search's v_mix.  An
        active board whose root has no edges (stuck) gets the search's -1, as
        zero visits give it under PUCT: env.step reports the no-op and the next
        check_steps() raises for that board, under either root policy."""
        cfg = self.cfg
        step = self.step_counter
        g = self.noise.gumbel(step, self.n)
        self.step_counter += 1
        self.mcts.search(self.evaluator, cfg["cpuct"], active=active, testing=True, max_rows=max(1, bound),
                         root="gumbel", gumbel=g, **self.gumbel)
        res = self.last_gumbel = self.mcts.gumbel_result()
        if self.keep_root_value:
            self.last_root_value = res["value"]
        self.check_steps()  # the previous move's step, done long before this search runs
        act = res["action"].to(torch.int64)
        v = torch.round(res["pi"].to(torch.float64) * 65535.0).to(torch.int32)
        if self.keep_noise:
            self.noise_log.append((g.clone(), None, act.clone()))
        self._step(act, active, step)
        return st, v, active

    def _step(self, act, active, step):
        """The chosen moves applied; the step's status queued for the next move()."""
        env, n, d = self.env, self.n, self.device
        act = torch.where(active, act, torch.full_like(act, -1)).to(torch.int16)
        status = env.step(act)
        if self.tree_reuse:
            self._carried = (env.export_state(), self.mcts.advance(act, active)["visits"].clone())
        bad = active & (status != 0)
        # read back by the next move (or check_steps()) after its search is queued
        # (with playout caps: the full boards of the move after next, whose
        # coin depends on (seed, board, move) alone; the next move's search is
        # queued before these flags are read)
        flags = [bad.sum(dtype=torch.int64), (~env.done()).sum(dtype=torch.int64)]
        if self.playout_cap:
            flags.append(playout_budgets(self.noise.coin(step + 2, n), self.playout_cap[0], 1, 0)[1]
                         .sum(dtype=torch.int64))
            self._flags_full_step = step + 2
        self._flags[:len(flags)].copy_(torch.stack(flags), non_blocking=True)
        self._flags_ev = torch.cuda.Event() if d.type == "cuda" else None
        if self._flags_ev is not None:
            self._flags_ev.record()
        self._bad_dev = bad
        self._flags_epoch = env.epoch

    def _active_bound(self):
        return self._n_active if self.env.epoch == self._n_active_epoch else self.n

    def check_steps(self):
        """Raise RuntimeError if the last move's env step failed on a board
        (waits for that step only); updates the active-board bound."""
        if self._bad_dev is None:
            return
        if self._flags_ev is not None:
            self._flags_ev.synchronize()
        nbad, nact, nfull = (int(x) for x in self._flags.tolist())
        bad, self._bad_dev = self._bad_dev, None
        if self.playout_cap:
            self._full_bound = {self._flags_full_step: nfull}
        self._n_active, self._n_active_epoch = nact, self._flags_epoch
        if nbad:
            raise RuntimeError(f"self-play step failed on boards {torch.nonzero(bad).flatten().tolist()[:8]}")

    def play(self, reset=True):
        """Play one game on every board; returns the device records."""
        env, n, d = self.env, self.n, self.device
        if reset:
            env.reset()
        T = self.max_plies
        states = torch.zeros(T, 6, n, dtype=torch.int64, device=d)
        players = torch.zeros(T, n, dtype=torch.int8, device=d)
        visits = torch.zeros(T, n, 143, dtype=torch.int32, device=d)
        valid = torch.zeros(T, n, dtype=torch.bool, device=d)
        root_value = torch.zeros(T, n, dtype=torch.float64, device=d) if self.keep_root_value else None
        full = torch.zeros(T, n, dtype=torch.bool, device=d) if self.playout_cap else None
        carried = torch.zeros(T, n, dtype=torch.int32, device=d) if self.tree_reuse else None
        done = env.done()
        ply = 0
        while ply < T:
            n_active = int((~done).sum())  # (one host read per ply: the loop stops exactly)
            if n_active == 0:
                break
            self._n_active, self._n_active_epoch = n_active, env.epoch
            st, v, active = self.move(ply, done, _bound=n_active)
            states[ply] = st
            players[ply] = ((st[5] >> 41) & 1).to(torch.int8)
            valid[ply] = active
            visits[ply] = v
            if root_value is not None:
                root_value[ply] = self.last_root_value
            if full is not None:
                full[ply] = self.last_full
            if carried is not None:
                carried[ply] = self.last_carried
            done = env.done()
            ply += 1
        self.check_steps()
        final = env.export_state()
        rec = {"states": states[:ply], "players": players[:ply], "visits": visits[:ply],
               "valid": valid[:ply], "final": final, "plies": ply}
        if root_value is not None:
            rec["root_value"] = root_value[:ply]  # f64 [T, n], from the recorded player's side
        if full is not None:
            rec["full"] = full[:ply]  # bool [T, n]: the move was searched in full (playout caps)
        if carried is not None:
            rec["carried"] = carried[:ply]  # int32 [T, n]: the root visits the search started with (tree reuse)
        return rec

    def play_steady(self, moves, reset=True, progress=None):
        """Continuous self-play: the reference's self_play_worker
        (trainer.py:434-541) run game after game on every board, `moves`
        moves in all.  A board whose game ended at a move starts its next
        game before the following move (HarmoniesGameState() after
        random.seed(seed_base + b + (k << 32)) for its k-th game, k = 0, 1,
        ... per board: the seeds hz_rollout(auto_reset=1) uses), so every
        board searches at every move and no leaf batch shrinks while games
        end.  Each move's records keep the board's game index; z comes from
        that game's outcome once it has ended (games still running at the
        end give no examples; compact_steady()).  progress(move) is called
        after each move (host side only)."""
        env, n, d = self.env, self.n, self.device
        bidx = torch.arange(n, device=d, dtype=torch.int64)
        base = int(self.env.seed_base)
        game = torch.zeros(n, dtype=torch.int64, device=d)
        ply = torch.zeros(n, dtype=torch.int64, device=d)
        if reset:
            env.reset(seeds=base + bidx)
        M = int(moves)
        states = torch.zeros(M, 6, n, dtype=torch.int64, device=d)
        visits = torch.zeros(M, n, 143, dtype=torch.int32, device=d)
        games = torch.zeros(M, n, dtype=torch.int32, device=d)
        ended = torch.zeros(M, n, dtype=torch.bool, device=d)
        outcome = torch.zeros(M, n, dtype=torch.float32, device=d)
        plies = torch.zeros(M, n, dtype=torch.int16, device=d)
        none = torch.zeros(n, dtype=torch.bool, device=d)
        root_value = torch.zeros(M, n, dtype=torch.float64, device=d) if self.keep_root_value else None
        full = torch.zeros(M, n, dtype=torch.bool, device=d) if self.playout_cap else None
        carried = torch.zeros(M, n, dtype=torch.int32, device=d) if self.tree_reuse else None
        for m in range(M):
            self._n_active, self._n_active_epoch = n, env.epoch
            st, v, _ = self.move(ply, none, _bound=n)
            states[m] = st
            visits[m] = v
            if root_value is not None:
                root_value[m] = self.last_root_value
            if full is not None:
                full[m] = self.last_full
            if carried is not None:
                carried[m] = self.last_carried
            games[m] = game.to(torch.int32)
            fin = env.export_state()
            over = env.done()
            ended[m] = over
            outcome[m] = torch.where(over, self.outcomes(fin), torch.zeros_like(outcome[m]))
            plies[m] = (ply + 1).to(torch.int16)
            # the boards whose game just ended start their next one (a
            # selected-board reset: nothing moves where over is false)
            game = game + over.to(torch.int64)
            ply = torch.where(over, torch.zeros_like(ply), ply + 1)
            env.reset(sel=over, seeds=base + bidx + (game << 32))
            if progress is not None:
                progress(m)
        self.check_steps()
        players = ((states[:, 5] >> 41) & 1).to(torch.int8)
        rec = {"states": states, "visits": visits, "players": players, "game": games, "ended": ended,
               "outcome": outcome, "plies": plies, "moves": M}
        if root_value is not None:
            rec["root_value"] = root_value  # f64 [M, n], from the recorded player's side
        if full is not None:
            rec["full"] = full  # bool [M, n]: the move was searched in full (playout caps)
        if carried is not None:
            rec["carried"] = carried  # int32 [M, n]: the root visits the search started with (tree reuse)
        return rec

    ASYNC_LAG = 2  # sim steps queued past the one whose running-board count the host waits for

    def _async_unsupported(self):
        """The configuration keys play_async does not take yet (each needs one
        more masked per-board draw, or the carried begin)."""
        off = []
        if self.tree_reuse:
            off.append("tree_reuse")
        if self.gumbel is not None:
            off.append("root_policy 'gumbel'")
        if self.leaf_symmetry:
            off.append("leaf_symmetry")
        if self.forced_k is not None:
            off.append("forced_playouts")
        if self.keep_root_value:
            off.append("keep_root_value")
        return off

    def play_async(self, moves, reset=True, sim_steps=None):
        """play_steady(moves) without the barrier between moves: every board
        keeps a move counter of its own, and a board whose search is spent
        records its result, plays its move and begins its next search inside
        the sim step, while the other boards carry on with theirs; every sim
        step then has one live row per board, whatever the boards' budgets
        (playout caps).  Board b's k-th move is searched, chosen, recorded and
        played exactly as play_steady does at its move k (the draws' keys, the
        budget rule, the tau rule by the board's own ply, the game seeds), so
        the records are play_steady's bit for bit, for a row_independent
        evaluator.

        One sim step is select + gather + encode, the evaluator, expand +
        backup, then the turn (hz_turn_choose, hz_step, hz_turn_after,
        hz_reset on the ended games, the turned boards' draws and gate
        updates, hz_mcts_begin_some): the layered form, in which a turned
        board's new root is evaluated in the very next step.  The host reads
        nothing per sim step: the count of running boards comes back through
        a pinned ring ASYNC_LAG steps late, so up to ASYNC_LAG empty steps are
        queued after the last board has stopped.

        The run ends when every board has made `moves` moves, or after
        sim_steps sim steps if given; the boards have then made different
        numbers of moves.  Returns play_steady's dict plus `moves_done` int32
        [n] (records past moves_done[b] are zero and invalid) and `sim_steps`
        (the steps up to the last turn); compact_steady() takes it as it is.
        A failed env step on a searched board raises RuntimeError at the end
        of the run, as check_steps() does.  The draws' move counter
        (step_counter) advances by `moves`, as play_steady's does, cut or not.

        PUCT root with Dirichlet noise, `testing`, playout caps on or off;
        tree_reuse, root_policy "gumbel", leaf_symmetry, forced_playouts and
        keep_root_value raise ValueError."""
        off = self._async_unsupported()
        if off:
            raise ValueError(f"play_async does not take {', '.join(off)}")
        M = int(moves)
        limit = None if sim_steps is None else int(sim_steps)
        if M < 0 or (limit is not None and limit < 0):
            raise ValueError("play_async: negative moves or sim_steps")
        env, n, d, cfg, mcts, L = self.env, self.n, self.device, self.cfg, self.mcts, nat.lib()
        testing = bool(cfg.get("testing", False))
        nsims, cpuct, eps = int(cfg["num_simulations"]), cfg["cpuct"], cfg["dirichlet_epsilon"]
        alpha, tau0 = cfg["dirichlet_alpha"], int(cfg["turns_until_tau0"])
        base = int(env.seed_base)
        self.check_steps()  # (an earlier move()'s step)
        if reset:
            env.reset(seeds=base + torch.arange(n, device=d, dtype=torch.int64))

        def z(dtype, *shape, fill=0):
            return torch.full(shape, fill, dtype=dtype, device=d)

        rec = {"states": z(torch.int64, M, 6, n), "visits": z(torch.int32, M, n, 143), "game": z(torch.int32, M, n),
               "ended": z(torch.bool, M, n), "outcome": z(torch.float32, M, n), "plies": z(torch.int16, M, n)}
        full = z(torch.bool, M, n) if self.playout_cap else None
        mc, ply, game = z(torch.int64, n), z(torch.int32, n), z(torch.int64, n)
        running = z(torch.int32, 1, fill=n if M else 0)
        act, turned, bad = z(torch.int16, n, fill=-1), z(torch.uint8, n), z(torch.uint8, n)
        sel, seeds = z(torch.uint8, n), z(torch.int64, n)
        begin = z(torch.uint8, n, fill=1 if M else 2)  # the first searches: every board's
        noise, u, coin = z(torch.float64, n, MAX_CHILDREN), z(torch.float64, n), z(torch.float64, n, fill=1.0)
        budget_all = z(torch.int32, n, fill=nsims)
        step0 = self.step_counter
        mcts._open(nsims, budget_all, z(torch.uint8, n, fill=1))  # the budget gate and the root-noise mask on
        device_rows = bool(getattr(self.evaluator, "device_rows", False))

        def begin_turned():
            """Step (d): the searches of the boards `begin` names, at their own move counters."""
            _, count = env.legal_mask()
            mv = mc + step0 if step0 else mc
            if self.playout_cap:
                p, fast = self.playout_cap
                self.noise.coin_at(mv, begin, coin)
                budget, is_full = playout_budgets(coin, p, nsims, fast)
                mcts.set_gate_some(begin, budget=budget, root_noise=is_full)
            else:  # (the stuck-root rule may have zeroed the board's last budget)
                mcts.set_gate_some(begin, budget=budget_all)
            self.noise.draw_at(mv, count, alpha, begin, noise, u)
            mcts.begin_some(begin)

        def sim_step():
            board, glob, rows, count = mcts.select_gather(cpuct)
            if device_rows:
                policy, value = self.evaluator(board, glob, rows, count)
            else:  # every row, the stale ones past count included (unused): no host read of count
                policy, value = self.evaluator(board, glob)
            mcts.expand_backup(policy, value, noise, eps, testing, gathered=True)
            nat.check(L.hz_turn_choose(mcts._h, env.handle, nat.ptr(u), nat.ptr(ply), nat.ptr(mc), nat.ptr(game), M,
                                       tau0, int(testing), nat.ptr(act), nat.ptr(turned), nat.ptr(rec["states"]),
                                       nat.ptr(rec["visits"]), nat.ptr(rec["game"]), nat.ptr(full)), "hz_turn_choose")
            status = env.step(act)
            nat.check(L.hz_turn_after(env.handle, nat.ptr(turned), nat.ptr(status), nat.ptr(mc), nat.ptr(ply),
                                      nat.ptr(game), M, base & (2**64 - 1), nat.ptr(rec["ended"]),
                                      nat.ptr(rec["outcome"]), nat.ptr(rec["plies"]), nat.ptr(sel), nat.ptr(seeds),
                                      nat.ptr(begin), nat.ptr(bad), nat.ptr(running), nat.stream_ptr(d)),
                      "hz_turn_after")
            env.reset(sel=sel, seeds=seeds)
            begin_turned()

        begin_turned()
        ring = torch.zeros(self.ASYNC_LAG + 2, dtype=torch.int32, pin_memory=True)
        pending = []  # (sim steps run, ring slot, event), oldest first
        done_at = 0 if M == 0 else None

        def landed(keep):
            """Wait for the counts queued more than `keep` steps ago; the step count at which no board ran."""
            while len(pending) > keep:
                at, slot, ev = pending.pop(0)
                ev.synchronize()
                if int(ring[slot]) == 0:
                    return at
            return None

        steps = 0
        while done_at is None and (limit is None or steps < limit):
            sim_step()
            steps += 1
            slot = steps % ring.numel()
            ring[slot:slot + 1].copy_(running, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            pending.append((steps, slot, ev))
            done_at = landed(self.ASYNC_LAG)
        if done_at is None:
            done_at = landed(0)
        self.step_counter = step0 + M
        mcts._finish(trees=False)
        nbad = torch.nonzero(bad).flatten().tolist()  # (the run's one wait for the device)
        if nbad:
            raise RuntimeError(f"self-play step failed on boards {nbad[:8]}")
        rec["players"] = ((rec["states"][:, 5] >> 41) & 1).to(torch.int8)
        rec["moves"] = M
        if full is not None:
            rec["full"] = full
        rec["moves_done"] = mc.to(torch.int32)
        rec["sim_steps"] = steps if done_at is None else done_at
        return rec

    def _full_only(self, rec, full_only):
        """The records' full-search mask when only those become training
        records (the default with playout caps on), else None."""
        if full_only is None:
            full_only = self.playout_cap is not None
        return rec["full"] if full_only and "full" in rec else None

    def compact_steady(self, rec, full_only=None):
        """play_steady's records of the games that ended inside the run, in
        (move, board) order: as compact() (states, visits, pi, z from the
        recorded player's side, player, board), plus each record's game
        index, and per ended game its length (`lengths`: plies); with
        keep_root_value also q f32 [M], as compact().  full_only (default:
        playout caps on): only the moves searched in full give records."""
        M, n, d = rec["moves"], self.n, self.device
        game = rec["game"].to(torch.int64)                         # [M, n]
        K = int(game.max().item()) + 1 if M else 1
        key = game * n + torch.arange(n, device=d).unsqueeze(0)    # (game, board)
        res = torch.zeros(K * n, dtype=torch.float32, device=d)
        has = torch.zeros(K * n, dtype=torch.bool, device=d)
        em = rec["ended"]
        res[key[em]] = rec["outcome"][em]
        has[key[em]] = True
        mask = has[key]                                            # records of ended games
        if "moves_done" in rec:  # play_async cut short by sim_steps: the slots a board did not reach are no records
            mask = mask & (torch.arange(M, device=d).unsqueeze(1) < rec["moves_done"].unsqueeze(0))
        full = self._full_only(rec, full_only)
        if full is not None:
            mask = mask & full
        player = rec["players"].to(torch.float32)
        out = res[key]
        z = torch.where(player == 0, out, -out)
        states = rec["states"].permute(0, 2, 1)[mask]
        visits = rec["visits"][mask]
        board_id = torch.arange(n, device=d).expand(M, n)[mask].to(torch.int32)
        comp = {"states": states.contiguous(), "visits": visits, "pi": pi_from_visits(visits),
                "z": z[mask].contiguous(), "player": rec["players"][mask], "board": board_id,
                "game": game[mask].to(torch.int32), "lengths": rec["plies"][em].to(torch.int64)}
        if "root_value" in rec:
            comp["q"] = rec["root_value"][mask].to(torch.float32)
        return comp

    @staticmethod
    def outcomes(final):
        """get_game_outcome per board (+1 P0 won, -1 P1 won, 0 draw)."""
        win = (final[5] >> 46) & 3
        return torch.where(win == 1, 1, torch.where(win == 2, -1, 0)).to(torch.float32)

    def compact(self, rec, full_only=None):
        """Flatten the valid records: states int64 [M, 6], visits int32
        [M, 143], pi f32 [M, 143], z f32 [M] (trainer.py:517-538), player
        int8 [M], board id int32 [M]; from records kept with keep_root_value
        also q f32 [M], the search's root value from the recorded player's
        side like z (the recorded player is the root's mover).  full_only
        (default: playout caps on): only the moves searched in full give
        records (rec["full"])."""
        out = self.outcomes(rec["final"])                       # [n]
        T = rec["plies"]
        mask = rec["valid"]                                      # [T, n]
        full = self._full_only(rec, full_only)
        if full is not None:
            mask = mask & full
        player = rec["players"].to(torch.float32)
        z = torch.where(player == 0, out.unsqueeze(0), -out.unsqueeze(0))  # 0 stays 0 for draws
        states = rec["states"].permute(0, 2, 1)[mask]            # [M, 6]
        visits = rec["visits"][mask]
        pi = pi_from_visits(visits)                              # [M, 143]
        board_id = torch.arange(self.n, device=self.device).expand(T, self.n)[mask].to(torch.int32)
        comp = {"states": states.contiguous(), "visits": visits, "pi": pi, "z": z[mask].contiguous(),
                "player": rec["players"][mask], "board": board_id}
        if "root_value" in rec:
            comp["q"] = rec["root_value"][mask].to(torch.float32)
        return comp

    def iteration(self, buffer=None, group=None, timings=None, schedule=None, moves_per_board=None):
        """One self-play phase: every board plays a game; with torch.distributed
        initialised the packed records of all ranks are all-gathered (RCCL)
        into `buffer` (a distributed.ReplayBuffer) on every rank, in rank
        order.  timings (a dict, optional) gets "play_s" and "exchange_s"
        (device-synchronised; the exchange starts after a barrier).
        schedule="async" with moves_per_board=K: the phase is play_async(K) and
        compact_steady() instead (the games that ended inside the run)."""
        from . import distributed as hd
        import time
        import torch.distributed as dist
        moves_per_board = check_schedule(schedule, moves_per_board)
        t0 = time.perf_counter()
        if schedule == "async":
            rec = self.play_async(moves_per_board)
            comp = self.compact_steady(rec)
        else:
            rec = self.play()
            comp = self.compact(rec)
        packed = hd.pack_records(comp["states"], comp["visits"], comp["z"], comp["player"])
        distributed = dist.is_available() and dist.is_initialized()
        if timings is not None:
            torch.cuda.synchronize(self.device)
            timings["play_s"] = time.perf_counter() - t0
            timings["own_records"] = packed
            if distributed:
                dist.barrier(group)
        t1 = time.perf_counter()
        out = hd.all_gather_records(packed, group) if distributed else packed
        if buffer is not None:
            buffer.extend(out)
        if timings is not None:
            torch.cuda.synchronize(self.device)
            timings["exchange_s"] = time.perf_counter() - t1
        return out, rec

    def examples(self, compact):
        """The reference's replay-buffer tuples (trainer.py:529-538), on CPU."""
        board, glob = encode_states(compact["states"])
        b, g, p, z = board.cpu(), glob.cpu(), compact["pi"].cpu(), compact["z"].cpu()
        return [(b[i], g[i], p[i], z[i:i + 1]) for i in range(b.shape[0])]


def encode_states(states):
    """create_state_tensors for an int64 [M, 6] array of state words."""
    m = states.shape[0]
    dev = states.device
    board = torch.empty(m, 38, 5, 7, dtype=torch.float32, device=dev)
    glob = torch.empty(m, 42, dtype=torch.float32, device=dev)
    if m:
        st = states.contiguous()
        nat.check(nat.lib().hz_encode_states(nat.ptr(st), 1, 6, None, m, nat.ptr(board), nat.ptr(glob),
                                             nat.stream_ptr(dev)), "hz_encode_states")
    return board, glob
