"""The search's caller-chosen limits (hz_mcts_create's max_nodes and
max_depth, include/hz_abi.h) against the C oracle given the same limits
(or_mcts_cfg.max_nodes / max_depth): an expansion that does not fit is refused
whole and a walk at max_depth stops on an expanded node, either sets
counts[b][3], and a board without the flag is bit for bit the unbounded
search.  Board b's pools are followed directly by board b + 1's, so an
expansion let through one entry too far would rewrite its neighbour's root or
first edges: every batch here orders its boards so that a board that hits the
limit is followed by one that does not and is compared with the fixture.

The rows are mcts.npz's (32 sims, cpuct 2, testing, eps 0.25) group;
tests/test_oracle_golden.py::test_mcts_limits_fixture_conditions pins what
they must offer (needs around max_nodes = 500, deepest paths around 2)."""
import functools
import os

import numpy as np
import pytest
import torch

import oracle
from conftest import GOLDEN
from hzamd.state import pack_ref, words_to_array

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GROUP = (32, 2.0, 1, 0.25)
M = 500   # max_nodes: 8 of the group's 13 rows fit (one exactly: 492 nodes, 500 edges), 5 do not (508 just over)
# smaller pools, where refusals come early enough to change the rest of the search (the five rows refused at 500
# lose only their last expansions: visits and stream as unbounded): at 250 ten rows are refused, two with another
# next MT word than the fixture's (a refused place_tile_3 leaf's draws, kept) and two with other visits; at 140
# twelve, six and three (test_oracle_golden.py::test_mcts_limits_fixture_conditions)
M_EARLY = (250, 140)
# place_tile_3 roots with 2 or 3 legal moves: at max_nodes = need - 1 the root's own expansion never fits
ROOT_REFUSED = ((3, 2, 8), (4, 3, 64), (4, 3, 32))   # (nodes, edges, sims) of the fixture rows
D = 2     # max_depth: the group's deepest paths are 3 3 4 4 2 3 4 2 3 2 3 1 3: 4 rows at or under it, 9 above


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(GOLDEN, "mcts.npz"))


def need(k):
    f = fixture()
    return max(int(f["n_nodes"][k]), int(f["n_edges"][k]))


@functools.lru_cache(maxsize=None)
def oracle_row(k, max_nodes=0, max_depth=0):
    """(action, visits, nodes, edges, flag, deepest path, next MT word) of
    fixture row k under the oracle with these limits (0: none); computed once."""
    f = fixture()
    m = oracle.mt_seed(int(f["mt_seed"][k]))
    r = oracle.mcts_search(
        f["state"][k], m, int(f["sims"][k]), float(f["cpuct"][k]), eps=float(f["eps"][k]),
        testing=bool(f["testing"][k]), tau0=int(f["tau0"][k]), ply=int(f["ply"][k]),
        u=float(f["u"][k]), noise=f["noise"][k], max_nodes=max_nodes, max_depth=max_depth, with_limits=True)
    r[1].setflags(write=False)
    return r + (oracle.mt_next32(m),)


def root_refused_next(k):
    """The next MT word after a search whose root expansion (a place_tile_3
    root) is refused in every simulation: each attempt replays every legal
    child's turn-end draws and keeps them.  Replayed here with or_step."""
    f = fixture()
    m = oracle.mt_seed(int(f["mt_seed"][k]))
    legal = np.flatnonzero(oracle.legal(f["state"][k]))
    for _ in range(int(f["sims"][k])):
        for a in legal:
            assert oracle.step(f["state"][k], int(a), m)[0] == 0
    return oracle.mt_next32(m)


def fits(k, max_nodes=0, max_depth=0):
    return (not max_nodes or need(k) <= max_nodes) and (not max_depth or oracle_row(k)[5] <= max_depth)


def group_order(max_nodes=0, max_depth=0):
    """The group's rows, every row that hits a limit directly followed by one
    that does not, ending on one that does not."""
    f = fixture()
    rows = [k for k in range(len(f["sims"]))
            if (int(f["sims"][k]), float(f["cpuct"][k]), int(f["testing"][k]), float(f["eps"][k])) == GROUP]
    assert len(rows) == 13
    ok = [k for k in rows if fits(k, max_nodes, max_depth)]
    cut = [k for k in rows if not fits(k, max_nodes, max_depth)]
    assert ok and cut
    order = []
    while cut:
        # fitting rows between the refused ones while they last (nine cut rows
        # under max_depth 2 share four fitting ones: then the cut rows stand
        # together, the batch still ending on a fitting row)
        if len(ok) > 1:
            order.append(ok.pop(0))
        order.append(cut.pop(0))
    order += ok
    assert fits(order[-1], max_nodes, max_depth)
    return order


def load_env(env, ks):
    f = fixture()
    words = words_to_array([pack_ref(v) for v in f["state"][ks]])
    mts = np.zeros((len(ks), 624), np.uint32)
    idx = np.zeros(len(ks), np.int32)
    for i, k in enumerate(ks):
        mts[i], idx[i] = oracle.mt_seed(int(f["mt_seed"][k])).words()
    env.import_state(torch.from_numpy(np.ascontiguousarray(words.T)),
                     torch.from_numpy(mts.view(np.int32)), torch.from_numpy(idx))


def make_env(ks):
    from hzamd.env import BatchedEnv
    env = BatchedEnv(len(ks), device=DEV)
    load_env(env, ks)
    return env


class _StubRows:
    """The stub on the device-row protocol (no host read per simulation;
    PyTorch device ops only, so a simulation can be captured)."""
    device_rows = True
    capturable = True
    row_independent = True

    def __call__(self, board, glob, rows=None, count=None):
        from hzamd.mcts import stub_evaluator
        return stub_evaluator(board, glob)


# search() forms: (copies of each row in the batch, settings)
FORMS = {
    "small_batch": (1, {}),
    "separate": (9, {"fuse_select": False}),
    "fused_select": (9, {"fuse_gather": False}),
    "fused_select_gather": (9, {}),
    "graph": (1, {"graph": True}),
}


def search(mcts, env, ks, form, active=None):
    """One search() of rows ks in this form: visits, chosen actions, counts
    [n, 4] and each board's next MT word."""
    from hzamd.mcts import choose_actions, stub_evaluator
    f = fixture()
    opts = dict(FORMS[form][1])
    mcts.fuse_select, mcts.fuse_gather = opts.pop("fuse_select", True), opts.pop("fuse_gather", True)
    ev = _StubRows() if opts.get("graph") else stub_evaluator
    sims, cpuct, testing, eps = (f[key][ks[0]] for key in ("sims", "cpuct", "testing", "eps"))
    assert all((f["sims"][k], f["cpuct"][k], f["testing"][k], f["eps"][k]) == (sims, cpuct, testing, eps) for k in ks)
    assert mcts.num_simulations == sims
    noise = torch.from_numpy(np.ascontiguousarray(f["noise"][ks][:, :69]))
    visits = mcts.search(ev, float(cpuct), active=active, noise=noise, eps=float(eps), testing=bool(testing), **opts)
    explore = torch.tensor([(not testing) and f["ply"][k] < f["tau0"][k] for k in ks])
    u = torch.tensor([f["u"][k] for k in ks], dtype=torch.float64)
    act = choose_actions(visits.cpu(), explore, u).numpy()
    counts = mcts.stats().cpu().numpy().copy()
    _, mt, mti = env.export_state(with_mt=True)
    mt, mti = mt.cpu().numpy().view(np.uint32), mti.cpu().numpy()
    nxt = [oracle.mt_next32(oracle.mt_from_words(mt[j], mti[j])) for j in range(len(ks))]
    return {"visits": visits.cpu().numpy().copy(), "action": act, "counts": counts, "next": nxt}


def check_board(res, j, k, max_nodes=0, max_depth=0):
    """Board j (fixture row k) against the oracle under the same limits, and,
    where the row hits neither, against the fixture itself."""
    f = fixture()
    a, visits, nn, ne, flag, _, nxt = oracle_row(k, max_nodes, max_depth)
    if visits.sum() == 0 and flag:
        # the root itself refused: no visits, so choose_actions gives -1 where
        # the oracle (like the reference) falls back to random.choice, which
        # draws once more from the stream; up to there the streams agree
        assert (nn, ne) == (1, 0) and f["state"][k][73] == 3
        a, nxt = -1, root_refused_next(k)
    got = (res["visits"][j], res["action"][j], tuple(res["counts"][j, :2]), res["counts"][j, 3] != 0, res["next"][j])
    tag = (j, k, need(k), got[2:], (nn, ne, flag, nxt))
    assert (got[0] == visits).all(), tag
    assert got[1:] == (a, (nn, ne), bool(flag), nxt), tag
    ok = fits(k, max_nodes, max_depth)
    assert bool(flag) == (not ok), tag
    if ok:
        assert (got[0] == f["visits"][k]).all() and got[1] == f["action"][k], tag
        assert got[2] == (f["n_nodes"][k], f["n_edges"][k]) and got[4] == f["next_word"][k], tag


def check_copies(res, ks, per):
    for j in range(per, len(ks)):
        assert ks[j] == ks[j - per]
        for key in ("visits", "counts"):
            assert (res[key][j] == res[key][j - per]).all(), (key, j)
        assert res["action"][j] == res["action"][j - per] and res["next"][j] == res["next"][j - per], j


@pytest.mark.parametrize("form", list(FORMS))
def test_refused_expansions_match_bounded_oracle(form):
    """max_nodes 500 on the group, in every form of search() that instantiates
    the expansion or select_board separately: boards that fit are the
    fixture's, boards that do not are the bounded oracle's (visits, move,
    counts, flag, next MT word), copies of a row agree, and the handle's
    limit_hits_total counts the flagged boards."""
    from hzamd.mcts import BatchedMCTS
    copies = FORMS[form][0]
    order = group_order(max_nodes=M)
    ks = order * copies
    assert (len(ks) > 32) == (copies > 1) and len(ks) <= 117
    env = make_env(ks)
    mcts = BatchedMCTS(env, GROUP[0], max_nodes=M)
    assert mcts.bounded
    res = search(mcts, env, ks, form)
    for j, k in enumerate(ks):
        check_board(res, j, k, max_nodes=M)
    check_copies(res, ks, len(order))
    assert (res["counts"][:, :2] <= M).all()
    assert (mcts.limit_flags().cpu().numpy() == res["counts"][:, 3]).all()
    assert int(mcts.limit_hits_total.item()) == 5 * copies == int((res["counts"][:, 3] != 0).sum())
    mcts.close()
    env.close()


@pytest.mark.parametrize("form", ["small_batch", "fused_select_gather", "graph"])
@pytest.mark.parametrize("cap", M_EARLY)
def test_early_refusals_change_stream_and_visits_as_the_oracle_says(form, cap):
    """max_nodes 250 and 140 on the group: expansions are refused early, among
    them place_tile_3 leaves, whose chance draws are kept and made again when
    the leaf is selected again, and leaves that later, smaller expansions
    overtake.  The boards' next MT words and visits then differ from the
    fixture's (asserted here on what the device gave) and equal the bounded
    oracle's.  A kernel that dropped or deferred the stream write-back of a
    refused expansion, or did not draw again, fails here."""
    from hzamd.mcts import BatchedMCTS
    f = fixture()
    copies = FORMS[form][0]
    order = group_order(max_nodes=cap)
    ks = order * copies
    env = make_env(ks)
    mcts = BatchedMCTS(env, GROUP[0], max_nodes=cap)
    res = search(mcts, env, ks, form)
    for j, k in enumerate(ks):
        check_board(res, j, k, max_nodes=cap)
    check_copies(res, ks, len(order))
    assert (res["counts"][:, :2] <= cap).all()
    flagged = [j for j, k in enumerate(order) if res["counts"][j, 3] != 0]
    other_word = [j for j in flagged if res["next"][j] != f["next_word"][order[j]]]
    other_visits = [j for j in flagged if (res["visits"][j] != f["visits"][order[j]]).any()]
    assert len(flagged) >= 10 and len(other_word) >= 2 and len(other_visits) >= 2, (flagged, other_word, other_visits)
    assert (res["visits"][flagged].sum(1) == GROUP[0] - 1).all()   # refused leaves were backed up all the same
    assert int(mcts.limit_hits_total.item()) == len(flagged) * copies
    mcts.close()
    env.close()


def test_root_expansion_that_never_fits():
    """One board per handle, the three place_tile_3 roots with 2 or 3 legal
    moves at max_nodes = need - 1: every simulation tries the root's expansion
    again and is refused, so the search ends with the root alone, no edges, no
    visits, no move and the flag set, and the stream has the draws of every
    attempt: sims rounds over the legal children (another next word than the
    fixture's, where the root was expanded once)."""
    from hzamd.mcts import BatchedMCTS
    f = fixture()
    for shape in ROOT_REFUSED:
        ks = [k for k in range(len(f["sims"])) if (f["n_nodes"][k], f["n_edges"][k], f["sims"][k]) == shape]
        assert len(ks) == 1, shape
        k = ks[0]
        cap = need(k) - 1
        env = make_env(ks)
        mcts = BatchedMCTS(env, int(f["sims"][k]), max_nodes=cap)
        res = search(mcts, env, ks, "small_batch")
        check_board(res, 0, k, max_nodes=cap)
        assert res["visits"][0].sum() == 0 and res["action"][0] == -1 and tuple(res["counts"][0, :2]) == (1, 0), shape
        assert res["counts"][0, 3] == 1 and res["next"][0] == root_refused_next(k) != f["next_word"][k], shape
        assert mcts.root_edges()["n"].sum().item() == 0 and mcts.principal_variation(1)["len"].sum().item() == 0
        assert int(mcts.limit_hits_total.item()) == 1
        mcts.close()
        env.close()


def test_exact_fit_and_one_short():
    """One board per handle (its pools end the allocation), four rows of
    different need -- the 8-simulation row with 267 nodes and 339 edges, where
    only the edge pool binds; one where only the node pool binds (94 / 93); the
    group's exact fit (492 / 500) and its largest-but-one (614 / 741):
    max_nodes == need is the fixture row with flag 0, need - 1 the bounded
    oracle's search with the flag set."""
    from hzamd.mcts import BatchedMCTS
    f = fixture()
    want = [(267, 339, 8), (94, 93, 8), (492, 500, 32), (614, 741, 32)]
    for shape in want:
        ks = [k for k in range(len(f["sims"])) if (f["n_nodes"][k], f["n_edges"][k], f["sims"][k]) == shape]
        assert len(ks) == 1, shape
        k = ks[0]
        for cap in (need(k), need(k) - 1):
            env = make_env(ks)
            mcts = BatchedMCTS(env, int(f["sims"][k]), max_nodes=cap)
            res = search(mcts, env, ks, "small_batch")
            check_board(res, 0, k, max_nodes=cap)
            assert (res["counts"][0, 3] != 0) == (cap < need(k)) and (res["counts"][0, :2] <= cap).all(), (shape, cap)
            mcts.close()
            env.close()


@pytest.mark.parametrize("form", ["small_batch", "fused_select_gather"])
def test_depth_limit_matches_bounded_oracle(form):
    """max_depth 2 with the default pools: rows whose deepest path is at most 2
    are the fixture's with flag 0, the others the oracle's under max_depth 2
    with the flag set; in small_batch form then max_depth 1 as well."""
    from hzamd.mcts import BatchedMCTS
    copies = FORMS[form][0]
    for depth in (D, 1) if form == "small_batch" else (D,):
        order = group_order(max_depth=depth)
        ks = order * copies
        env = make_env(ks)
        mcts = BatchedMCTS(env, GROUP[0], max_depth=depth)
        assert mcts.bounded
        res = search(mcts, env, ks, form)
        for j, k in enumerate(ks):
            check_board(res, j, k, max_depth=depth)
        check_copies(res, ks, len(order))
        flagged = sum(not fits(k, max_depth=depth) for k in ks)
        assert flagged >= 3 * copies and int(mcts.limit_hits_total.item()) == flagged
        mcts.close()
        env.close()


def test_both_limits_under_a_replayed_graph_with_an_active_mask():
    """max_nodes 500 and max_depth 2 together, simulations 2.. one replayed
    graph, every third board left out: those have no visits, counts (0, 0) and
    an untouched stream; the rest are the oracle's under both limits.  Sixteen
    boards (three fitting rows twice), so that all five rows over 500 are
    searched and each is directly followed by a searched, compared board."""
    from hzamd.mcts import BatchedMCTS
    f = fixture()
    order = group_order(max_nodes=M)
    ok = [k for k in order if fits(k, max_nodes=M)]
    over = [k for k in order if not fits(k, max_nodes=M)]
    ok = ok + ok[:3]
    active = torch.ones(16, dtype=torch.uint8)
    active[2::3] = 0                       # 2, 5, 8, 11, 14
    ks = [over.pop(0) if j % 3 == 0 and j < 15 else ok.pop(0) for j in range(16)]   # over 500 at 0, 3, 6, 9, 12
    assert not over and not ok and fits(ks[-1], max_nodes=M) and active[-1]
    assert all(active[j] and active[j + 1] and fits(ks[j + 1], max_nodes=M)
               for j in range(16) if not fits(ks[j], max_nodes=M))
    env = make_env(ks)
    mcts = BatchedMCTS(env, GROUP[0], max_nodes=M, max_depth=D)
    res = search(mcts, env, ks, "graph", active=active.to(DEV))
    hit = 0
    for j, k in enumerate(ks):
        if not active[j]:
            assert res["visits"][j].sum() == 0 and tuple(res["counts"][j, :2]) == (0, 0), j
            assert res["next"][j] == oracle.mt_next32(oracle.mt_seed(int(f["mt_seed"][k]))), j
        else:
            check_board(res, j, k, max_nodes=M, max_depth=D)
            hit += not fits(k, M, D)
    assert 3 <= hit < int(active.sum()) and int(mcts.limit_hits_total.item()) == hit
    mcts.close()
    env.close()


def test_report_stays_in_bounds_on_flagged_boards():
    """After the small_batch search under max_nodes 500: root_edges' n is the
    visits, principal_variation(16) is at most 16 long and starts with the
    most-visited root action, and export_tree's arrays are exactly the counts
    long, child ids inside the tree, the root's slice summing to the visits."""
    from hzamd.mcts import BatchedMCTS
    ks = group_order(max_nodes=M)
    env = make_env(ks)
    mcts = BatchedMCTS(env, GROUP[0], max_nodes=M)
    res = search(mcts, env, ks, "small_batch")
    assert (res["counts"][:, 3] != 0).sum() == 5
    root_n = mcts.root_edges()["n"].cpu().numpy()
    assert (root_n == res["visits"]).all()
    pv = {key: v.cpu().numpy() for key, v in mcts.principal_variation(16).items()}
    for b, k in enumerate(ks):
        nn, ne = (int(x) for x in res["counts"][b, :2])
        assert 1 <= pv["len"][b] <= 16 and pv["action"][b, 0] == np.argmax(res["visits"][b]), b
        assert (pv["action"][b, pv["len"][b]:] == -1).all(), b
        t = mcts.export_tree(b)
        assert [len(t[key]) for key in ("state", "e0", "ne")] == [nn] * 3, b
        assert [len(t[key]) for key in ("action", "child", "n", "w", "p", "player")] == [ne] * 6, b
        assert t["child"].min() >= 0 and t["child"].max() < nn, b
        grown = t["ne"] > 0
        assert (t["e0"][grown] >= 0).all() and (t["e0"][grown] + t["ne"][grown] <= ne).all(), b
        e0, n0 = int(t["e0"][0]), int(t["ne"][0])
        by_action = np.zeros(143, np.int32)
        by_action[t["action"][e0:e0 + n0]] = t["n"][e0:e0 + n0]
        assert (by_action == res["visits"][b]).all() and by_action.sum() == GROUP[0] - 1, b
    mcts.close()
    env.close()


def test_flag_is_per_search():
    """A second search on the same handle, from positions that all fit: every
    flag is 0 and the results are the fixture's (the hash table's generation
    tags hide what the refused search left behind); limit_hits_total keeps the
    first search's count.  hz_mcts_begin clears the flag of the boards it
    starts: a board left out of a search keeps its last one."""
    from hzamd.mcts import BatchedMCTS
    ks = group_order(max_nodes=M)
    env = make_env(ks)
    mcts = BatchedMCTS(env, GROUP[0], max_nodes=M)
    res = search(mcts, env, ks, "small_batch")
    assert (res["counts"][:, 3] != 0).sum() == 5
    ok = [k for k in ks if fits(k, max_nodes=M)]
    again = (ok + ok[::-1])[:len(ks)]   # other rows than before on most boards, all of them fitting
    load_env(env, again)
    res = search(mcts, env, again, "small_batch")
    assert (res["counts"][:, 3] == 0).all()
    for j, k in enumerate(again):
        check_board(res, j, k, max_nodes=M)
    assert int(mcts.limit_hits_total.item()) == 5
    # ... and only for the boards a search starts: one left out keeps its last
    # flag next to counts (0, 0), and limit_hits_total does not count it again
    load_env(env, ks)
    res = search(mcts, env, ks, "small_batch")
    assert res["counts"][1, 3] == 1 and int(mcts.limit_hits_total.item()) == 10
    active = torch.ones(len(ks), dtype=torch.uint8)
    active[1] = 0
    load_env(env, again)
    res = search(mcts, env, again, "small_batch", active=active.to(DEV))
    assert tuple(res["counts"][1, :2]) == (0, 0) and res["counts"][1, 3] == 1 and res["visits"][1].sum() == 0
    assert (np.delete(res["counts"][:, 3], 1) == 0).all()
    assert int(mcts.limit_hits_total.item()) == 10
    mcts.close()
    env.close()


def test_limits_out_of_range_are_refused():
    """max_nodes of 1 or 1 << 24 and max_depth of 0 raise ValueError naming the
    argument (hz_mcts_create itself returns no handle for them), as does a
    principal variation longer than a small max_depth; a handle with the
    default sizes is not bounded and counts nothing."""
    import hzamd._native as nat
    from hzamd.mcts import BatchedMCTS
    ks = group_order(max_nodes=M)[:2]
    env = make_env(ks)
    for kw, name in (({"max_nodes": 1}, "max_nodes"), ({"max_nodes": 1 << 24}, "max_nodes"),
                     ({"max_depth": 0}, "max_depth")):
        with pytest.raises(ValueError, match=name):
            BatchedMCTS(env, 8, **kw)
    for nodes, depth in ((1, 192), (1 << 24, 192), (500, 0)):
        assert not nat.lib().hz_mcts_create(2, nodes, depth, 0, nat.stream_ptr(torch.device(DEV)))
    mcts = BatchedMCTS(env, 8, max_nodes=2, max_depth=3)
    assert mcts.bounded
    with pytest.raises(ValueError, match="max_len"):
        mcts.principal_variation(4)
    mcts.close()
    for kw in ({}, {"max_nodes": 1 + 69 * 8}, {"max_nodes": 1000, "max_depth": 500}):
        mcts = BatchedMCTS(env, 8, **kw)
        assert not mcts.bounded and int(mcts.limit_hits_total.item()) == 0
        mcts.close()
    env.close()
