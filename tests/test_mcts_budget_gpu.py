"""Per-board simulation budgets, the per-board root-noise mask, the row cap of
the evaluator's outputs and search()'s tail promise (include/hz_abi.h:
hz_mcts_set_budget, hz_mcts_sims_done, hz_mcts_set_root_noise_mask,
hz_mcts_set_row_cap).

The rule under test: a board with budget k and mask bit r is, bit for bit,
oracle.mcts_search(sims=min(k, sims), testing=not r): visits, node and edge
counts, limit flag and the board's next MT word.  The boards are mid-game
positions a few dozen rule plies in (turn-end expansions, which draw from the
board's stream, occur), 32 simulations, the stub and the dense stub.  n = 24
takes the one-launch select for up to 32 boards; n = 72 takes the 16-board
workgroups of the gathering expand launch, the last of them half empty."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
from hzamd.state import pack_ref, unpack_ref, words_to_array

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SIMS, CPUCT, EPS, BASE = 32, 2.0, 0.25, 7300
CYCLE = (0, 1, 2, 7, 31, 32, 40)
SIZES = (24, 72)


def budgets_for(n):
    b = np.array([CYCLE[(j + 3) % len(CYCLE)] for j in range(n)], np.int32)
    b[0], b[15], b[16], b[n - 1] = 0, 40, 0, 40   # the ends of the budget range on the edges of the launch shapes
    assert set(b.tolist()) == set(CYCLE)
    return b


def mask_for(n):
    m = (np.arange(n) % 3 != 1).astype(np.uint8)
    m[0], m[n - 1] = 0, 1
    return m


@functools.lru_cache(maxsize=None)
def position(n):
    """n mid-game boards (24 to 40 rule plies in): state words, streams, the
    root noise rows.  Played once per size; every test imports a copy."""
    from hzamd.env import BatchedEnv
    from hzamd.selfplay import NoiseSource
    env = BatchedEnv(n, seed_base=BASE, device=DEV)
    env.reset()
    plies = 24 + (torch.arange(n, device=DEV) * 5) % 17
    for p in range(41):
        mask, count = env.legal_mask()
        act = env.rule_actions(mask, count)
        env.step(torch.where(plies > p, act, torch.full_like(act, -1)))
    st, mt, idx = (t.cpu().numpy().copy() for t in env.export_state(with_mt=True))
    _, count = env.legal_mask()
    noise, _ = NoiseSource(BASE, DEV).draw(0, count, 0.4)
    noise = noise.cpu().numpy().copy()
    env.close()
    assert not any(oracle.is_game_over(unpack_ref(st[:, b])) for b in range(n))
    for a in (st, mt, idx, noise):
        a.setflags(write=False)
    return st, mt, idx, noise


def load(env, n, words=None):
    st, mt, idx, _ = position(n)
    env.import_state(torch.from_numpy(np.array(st if words is None else words)), torch.from_numpy(np.array(mt)),
                     torch.from_numpy(np.array(idx)))


def make_env(n, words=None):
    from hzamd.env import BatchedEnv
    env = BatchedEnv(n, seed_base=BASE, device=DEV)
    load(env, n, words)
    return env


def stream(n, b):
    _, mt, idx, _ = position(n)
    return oracle.mt_from_words(mt[b].view(np.uint32), idx[b])


def oracle_board(n, b, k, noisy, evaluator, state=None):
    """(visits, nodes, edges, flag, next MT word) of board b searched by the
    oracle with k simulations.  tau0 = 0 keeps the oracle's move choice greedy
    (no draw); a root left without edges (k = 0, a stuck root) makes it fall
    back to random.choice, one draw after the search: the stream the search
    left is then the untouched one."""
    st, _, _, noise = position(n)
    s = unpack_ref(st[:, b]) if state is None else state
    m = stream(n, b)
    _, visits, nn, ne, flag, _ = oracle.mcts_search(s, m, k, CPUCT, eps=EPS, testing=not noisy, tau0=0, ply=0,
                                                    noise=noise[b], evaluator=evaluator, with_limits=True)
    if ne == 0:
        assert k == 0 or not oracle.legal(s).any()
        m = stream(n, b)
    return visits.copy(), nn, ne, flag, oracle.mt_next32(m)


@functools.lru_cache(maxsize=None)
def reference(n, evaluator, masked=False, budgeted=True):
    bud = budgets_for(n) if budgeted else np.full(n, SIMS, np.int32)
    mask = mask_for(n) if masked else np.ones(n, np.uint8)
    rows = [oracle_board(n, b, min(int(bud[b]), SIMS), bool(mask[b]), evaluator) for b in range(n)]
    if budgeted:
        before = [oracle.mt_next32(stream(n, b)) for b in range(n)]
        assert sum(r[4] != w for r, w in zip(rows, before)) >= 3   # turn-end expansions drew from the streams
    return rows


class Rows:
    """A stub on the device-row protocol (device ops only: capturable)."""
    device_rows = True
    capturable = True
    row_independent = True

    def __init__(self, evaluator, cached=False):
        from hzamd.mcts import dense_stub_evaluator, stub_evaluator
        self.fn = dense_stub_evaluator if evaluator else stub_evaluator
        if cached:
            self.graph_key = (self, 0)

    def __call__(self, board, glob, rows=None, count=None):
        return self.fn(board, glob)


class InAlloc:
    """The stub over the handle's whole n-row buffers, returning the first k
    rows as views (k: the rows it was given, or a fixed number): whatever an
    expand launch reads at a row below n lies inside an allocation."""
    device_rows = True
    row_independent = True

    def __init__(self, mcts, k=None):
        self.mcts, self.k = mcts, k

    def __call__(self, board, glob, rows=None, count=None):
        from hzamd.mcts import stub_evaluator
        pol, val = stub_evaluator(self.mcts.board, self.mcts.glob)
        k = board.shape[0] if self.k is None else self.k
        assert pol.shape[0] == self.mcts.n and pol.is_contiguous() and pol.dtype == torch.float32
        return pol[:k], val[:k]


FORMS = {
    "gathered": {"fuse_select": False},          # select, gather, expand: separate launches
    "plain": {"gather": False},                  # one row per board
    "fused_select": {"fuse_gather": False},      # (n > 32) the next select inside the expand launch
    "fused_gather": {},                          # (n > 32) ... and the next leaf batch
    "graph": {"graph": True},                    # replayed capture, with an active mask
}


def run(mcts, env, n, form, evaluator=0, ev=None, active=None, **kw):
    from hzamd.mcts import dense_stub_evaluator, stub_evaluator
    opts = dict(FORMS[form])
    mcts.fuse_select, mcts.fuse_gather = opts.pop("fuse_select", True), opts.pop("fuse_gather", True)
    if ev is None:
        ev = Rows(evaluator) if opts.get("graph") else (dense_stub_evaluator if evaluator else stub_evaluator)
    noise = torch.from_numpy(np.array(position(n)[3]))
    visits = mcts.search(ev, CPUCT, active=active, noise=noise, eps=EPS, testing=False, **opts, **kw)
    counts = mcts.stats().cpu().numpy().copy()
    _, mt, idx = env.export_state(with_mt=True)
    mt, idx = mt.cpu().numpy().view(np.uint32), idx.cpu().numpy()
    nxt = [oracle.mt_next32(oracle.mt_from_words(mt[b], idx[b])) for b in range(n)]
    return {"visits": visits.cpu().numpy().copy(), "counts": counts, "next": nxt,
            "done": mcts.sims_done().cpu().numpy().copy(), "eval_rows": int(mcts.eval_rows.item())}


def check(res, n, rows, active=None):
    for b in range(n):
        if active is not None and not active[b]:
            want = (np.zeros(143, np.int32), 0, 0, None, oracle.mt_next32(stream(n, b)))
        else:
            want = rows[b]
        assert (res["visits"][b] == want[0]).all(), b
        assert tuple(res["counts"][b, :2]) == want[1:3], (b, res["counts"][b], want[1:3])
        assert want[3] is None or res["counts"][b, 3] == want[3], b
        assert res["next"][b] == want[4], b


def same(a, b):
    return ((a["visits"] == b["visits"]).all() and (a["counts"][:, (0, 1, 3)] == b["counts"][:, (0, 1, 3)]).all()
            and a["next"] == b["next"])


@pytest.mark.parametrize("evaluator", [0, 1])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n", SIZES)
def test_budgeted_boards_match_oracle(n, form, evaluator):
    """Every board against the oracle's search of min(budget, 32) simulations,
    in every form of search(); under the graph two boards are inactive."""
    from hzamd.mcts import BatchedMCTS
    env = make_env(n)
    mcts = BatchedMCTS(env, SIMS)
    bud = budgets_for(n)
    active = None
    if form == "graph":
        active = np.ones(n, bool)
        active[[3, n - 2]] = False
    res = run(mcts, env, n, form, evaluator, budget=torch.from_numpy(bud),
              active=None if active is None else torch.from_numpy(active).to(DEV))
    check(res, n, reference(n, evaluator), active)
    want = np.minimum(bud, SIMS) * (1 if active is None else active)
    assert (res["done"] == want).all(), (res["done"], want)
    assert (res["visits"].sum(1) == np.maximum(want - 1, 0)).all()   # the root's expansion backs nothing up
    if form != "plain":
        assert 0 < res["eval_rows"] <= int(want.sum())
    mcts.close()
    env.close()


@pytest.mark.parametrize("n,form", [(24, "gathered"), (72, "fused_gather"), (72, "graph")])
def test_sims_done_inactive_and_stuck(n, form):
    """sims_done(): min(budget, 32) on searched boards, 0 on inactive and
    stuck boards (a stuck root: no legal move, game not over; its tree is the
    root alone under any budget); eval_rows is at most its sum."""
    from hzamd.mcts import BatchedMCTS
    stuck, off = (5, n - 1), (6, 16)
    words = np.array(position(n)[0])
    stuck_ref = {b: oracle.stuck_state(BASE + b)[0] for b in stuck}
    for b in stuck:
        words[:, b] = words_to_array([pack_ref(stuck_ref[b])])[0]
    env = make_env(n, words)   # the streams stay
    mcts = BatchedMCTS(env, SIMS)
    bud = budgets_for(n)
    bud[list(stuck)] = (7, 40)
    active = np.ones(n, bool)
    active[list(off)] = False
    res = run(mcts, env, n, form, budget=torch.from_numpy(bud), active=torch.from_numpy(active).to(DEV))
    rows = list(reference(n, 0))
    for b in stuck:
        rows[b] = oracle_board(n, b, min(int(bud[b]), SIMS), True, 0, state=stuck_ref[b])
        assert rows[b][1:4] == (1, 0, 0) and rows[b][0].sum() == 0
    check(res, n, rows, active)
    want = np.minimum(bud, SIMS) * active
    want[list(stuck)] = 0
    assert (res["done"] == want).all(), (res["done"], want)
    assert 0 < res["eval_rows"] <= int(res["done"].sum())
    mcts.close()
    env.close()


@pytest.mark.parametrize("n,form", [(24, "gathered"), (72, "fused_gather"), (72, "fused_select"), (24, "graph")])
def test_mixed_root_noise_mask(n, form):
    """root_noise per board: a board with 0 is the oracle's testing=True
    search, a board with 1 the oracle's search with the board's noise row;
    with budgets, and without them (the mask alone)."""
    from hzamd.mcts import BatchedMCTS
    env = make_env(n)
    mcts = BatchedMCTS(env, SIMS)
    mask = torch.from_numpy(mask_for(n))
    res = run(mcts, env, n, form, budget=torch.from_numpy(budgets_for(n)), root_noise=mask)
    check(res, n, reference(n, 0, masked=True))
    load(env, n)
    res = run(mcts, env, n, form, root_noise=mask.bool())
    check(res, n, reference(n, 0, masked=True, budgeted=False))
    assert (res["done"] == 0).all()   # no gate: nothing counted
    plain = reference(n, 0, budgeted=False)
    differ = [b for b in range(n) if (reference(n, 0, masked=True, budgeted=False)[b][0] != plain[b][0]).any()]
    assert differ and all(mask_for(n)[b] == 0 for b in differ)   # the noise matters, and only where it was masked
    mcts.close()
    env.close()


@pytest.mark.parametrize("n,form", [(24, "gathered"), (72, "fused_gather"), (72, "fused_select"), (72, "plain")])
def test_gate_off_is_bit_identical(n, form):
    """The handle before any budget call, budget=None after a budgeted search
    and budget=full(32) give the same visits, stats and MT words: the
    unbudgeted oracle's."""
    from hzamd.mcts import BatchedMCTS
    env = make_env(n)
    mcts = BatchedMCTS(env, SIMS)
    first = run(mcts, env, n, form)
    check(first, n, reference(n, 0, budgeted=False))
    assert (first["done"] == 0).all()
    load(env, n)
    cut = run(mcts, env, n, form, budget=torch.from_numpy(budgets_for(n)))
    assert not same(cut, first)
    load(env, n)
    again = run(mcts, env, n, form, budget=None)
    assert same(again, first) and again["eval_rows"] == first["eval_rows"]
    load(env, n)
    full = run(mcts, env, n, form, budget=torch.full((n,), SIMS, dtype=torch.int32))
    assert same(full, first) and full["eval_rows"] == first["eval_rows"]
    assert (full["done"] == SIMS).all()
    mcts.close()
    env.close()


@pytest.mark.parametrize("n", SIZES)
def test_full_search_after_budgeted_with_graph_cache(n):
    """graph=True with a cacheable evaluator: full, budgeted, full again on
    one handle.  The gate's state is part of the cache key (a capture holds
    the handle by value), so the third search is the first's bits and the
    budgeted one the oracle's."""
    from hzamd.mcts import BatchedMCTS
    env = make_env(n)
    mcts = BatchedMCTS(env, SIMS)
    ev = Rows(0, cached=True)
    first = run(mcts, env, n, "graph", ev=ev)
    check(first, n, reference(n, 0, budgeted=False))
    key0 = mcts._graph_cache[0]
    load(env, n)
    cut = run(mcts, env, n, "graph", ev=ev, budget=torch.from_numpy(budgets_for(n)))
    check(cut, n, reference(n, 0))
    assert mcts._graph_cache[0] != key0
    g_cut = mcts._graph_cache[1]
    load(env, n)
    cut2 = run(mcts, env, n, "graph", ev=ev, budget=torch.from_numpy(budgets_for(n)[::-1].copy()))
    assert mcts._graph_cache[1] is g_cut   # other budgets, the same capture: the buffers keep their addresses
    assert (cut2["done"] == np.minimum(budgets_for(n)[::-1], SIMS)).all()
    load(env, n)
    again = run(mcts, env, n, "graph", ev=ev)
    assert mcts._graph_cache[0] == key0
    assert same(again, first) and (again["done"] == 0).all()
    mcts.close()
    env.close()


@pytest.mark.parametrize("n,form", [(24, "gathered"), (72, "gathered"), (72, "fused_select"), (72, "fused_gather"),
                                    (72, "plain")])
def test_row_cap_guard(n, form):
    """An evaluator whose outputs have fewer rows than the leaf batch: the
    search raises NativeError instead of reading past them (the outputs are
    views of n-row tensors, so even a failed guard would stay inside an
    allocation), and the next search on the handle is clean."""
    from hzamd import _native as nat
    from hzamd.mcts import BatchedMCTS
    env = make_env(n)
    mcts = BatchedMCTS(env, SIMS)
    short = InAlloc(mcts, k=n // 3)   # every board is live in simulation 1: n rows
    if form == "plain":
        short.device_rows = False
    with pytest.raises(nat.NativeError, match="leaf batch larger than the evaluator's rows"):
        run(mcts, env, n, form, ev=short)
    word = ctypes.c_int32(-1)
    assert nat.lib().hz_mcts_take_error(mcts._h, ctypes.byref(word)) == 0 and word.value == 0   # cleared
    load(env, n)
    res = run(mcts, env, n, form)
    check(res, n, reference(n, 0, budgeted=False))
    # enough rows: the same evaluator passes, and is the stub
    load(env, n)
    ok = InAlloc(mcts, k=n)
    if form == "plain":
        ok.device_rows = False
    assert same(run(mcts, env, n, form, ev=ok), res)
    mcts.close()
    env.close()


@pytest.mark.parametrize("n,form", [(72, "fused_gather"), (72, "gathered"), (24, "graph")])
def test_tail_promise(n, form):
    """tail=(s0, k): with a true bound (the boards whose budget exceeds s0)
    the bits of the search without it, the evaluator called with k rows from
    simulation s0 on; with a false one NativeError."""
    from hzamd import _native as nat
    from hzamd.mcts import BatchedMCTS
    env = make_env(n)
    mcts = BatchedMCTS(env, SIMS)
    s0 = 8
    bud = np.where(np.arange(n) % 4 == 1, SIMS, s0).astype(np.int32)
    k = int((bud > s0).sum())
    seen = []

    class Ev(InAlloc):
        capturable = True

        def __call__(self, board, glob, rows=None, count=None):
            seen.append(board.shape[0])
            return super().__call__(board, glob, rows, count)

    plain = run(mcts, env, n, form, ev=Ev(mcts), budget=torch.from_numpy(bud))
    rows = [oracle_board(n, b, int(bud[b]), True, 0) for b in range(n)]
    check(plain, n, rows)
    load(env, n)
    del seen[:]
    cut = run(mcts, env, n, form, ev=Ev(mcts), budget=torch.from_numpy(bud), tail=(s0, k), max_rows=n)
    assert same(cut, plain) and cut["eval_rows"] == plain["eval_rows"]
    if form == "graph":
        assert sorted(set(seen)) == [k, n]   # the eager simulation and two captures
    else:
        assert seen == [n] * s0 + [k] * (SIMS - s0)
    load(env, n)
    with pytest.raises(nat.NativeError, match="leaf batch larger than the evaluator's rows"):
        run(mcts, env, n, form, ev=Ev(mcts), budget=torch.from_numpy(bud), tail=(s0 - 2, k), max_rows=n)
    load(env, n)
    assert same(run(mcts, env, n, form, ev=Ev(mcts), budget=torch.from_numpy(bud)), plain)
    mcts.close()
    env.close()


def test_entry_point_argument_checks():
    from hzamd import _native as nat
    from hzamd.env import BatchedEnv
    from hzamd.mcts import BatchedMCTS
    L = nat.lib()
    buf = torch.zeros(8, dtype=torch.int32, device=DEV)
    assert L.hz_mcts_set_budget(None, nat.ptr(buf)) == -1
    assert L.hz_mcts_sims_done(None, nat.ptr(buf)) == -1
    assert L.hz_mcts_set_root_noise_mask(None, nat.ptr(buf)) == -1
    assert L.hz_mcts_set_row_cap(None, 1) == -1
    assert L.hz_mcts_take_error(None, None) == -1
    env = BatchedEnv(8, seed_base=1, device=DEV)
    env.reset()
    mcts = BatchedMCTS(env, 4)
    assert L.hz_mcts_sims_done(mcts._h, None) == -1
    assert L.hz_mcts_take_error(mcts._h, None) == -1
    assert L.hz_mcts_set_row_cap(mcts._h, -1) == -1
    assert L.hz_mcts_set_budget(mcts._h, None) == 0 and L.hz_mcts_set_root_noise_mask(mcts._h, None) == 0   # off
    with pytest.raises(ValueError):
        mcts.search(None, 2.0, budget=torch.zeros(7, dtype=torch.int32))
    with pytest.raises(ValueError):
        mcts.search(None, 2.0, root_noise=torch.zeros(9, dtype=torch.bool))
    assert (mcts.sims_done() == 0).all()
    mcts.close()
    env.close()
