"""Board symmetries on the CPU (hzamd.symmetry): the group derived from the hex
geometry, the rule-automorphism identities against the C oracle on every ply
of six rule-played games, the record transform in its torch form, and the
training sources' index arithmetic and configuration key.  No GPU calls."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
from hzamd import distributed as hd
from hzamd import symmetry as sym
from hzamd.state import SORTED_COORDS, pack_ref, unpack_ref, words_to_array

CELL_BITS = ((1 << 23) - 1) | (((1 << 23) - 1) << 32)


# ---- the group, from the geometry ------------------------------------------------
def hex_symmetries():
    """The 12 symmetries of the hex lattice about the origin as maps of axial
    coordinates: the six rotations of the cube coordinate (x, y, z) =
    (q, -q - r, r), each with and without the reflection that swaps x and y."""
    def rot60(x, y, z):
        return -z, -x, -y
    maps = []
    for k in range(6):
        for mirror in (False, True):
            def f(q, r, k=k, mirror=mirror):
                x, y, z = q, -q - r, r
                if mirror:
                    x, y = y, x
                for _ in range(k):
                    x, y, z = rot60(x, y, z)
                return x, z
            maps.append(f)
    return maps


@functools.lru_cache(maxsize=None)
def board_automorphisms():
    """Cell permutations of the symmetries that map the board to itself."""
    cell = {c: i for i, c in enumerate(SORTED_COORDS)}
    perms = set()
    for f in hex_symmetries():
        img = [f(q, r) for q, r in SORTED_COORDS]
        if set(img) == set(SORTED_COORDS):
            perms.add(tuple(cell[c] for c in img))
    return perms


def test_board_coordinates_are_the_reference_board():
    import constants
    assert sorted(tuple(h) for h in constants.VALID_HEXES) == SORTED_COORDS
    assert len(set(f(2, -1) + f(1, 3) for f in hex_symmetries())) == 12


def test_group_is_derived_from_geometry():
    autos = board_automorphisms()
    assert len(autos) == 4 == sym.N_SYM
    assert set(tuple(p) for p in sym.CELL_PERM) == autos
    # the issue's labelling: g = 0 the identity, 1 the half turn, 2 and 3 the
    # reflections (q + r, -r) and (-q - r, r)
    cell = {c: i for i, c in enumerate(SORTED_COORDS)}
    for g, f in enumerate((lambda q, r: (q, r), lambda q, r: (-q, -r), lambda q, r: (q + r, -r),
                           lambda q, r: (-q - r, r))):
        assert tuple(cell[f(q, r)] for q, r in SORTED_COORDS) == tuple(sym.CELL_PERM[g])
    assert all(sym.CELL_PERM[1][c] == 22 - c for c in range(23))
    for a in range(4):
        for b in range(4):
            assert sym.compose(a, b) == a ^ b
            ab = tuple(sym.CELL_PERM[a][sym.CELL_PERM[b][c]] for c in range(23))
            assert ab == tuple(sym.CELL_PERM[a ^ b])
        assert all(sym.CELL_PERM[a][sym.CELL_PERM[a][c]] == c for c in range(23))       # an involution
        assert all(sym.ACTION_PERM[a][sym.ACTION_PERM[a][x]] == x for x in range(143))
        assert list(sym.ACTION_PERM[a][:5]) == [0, 1, 2, 3, 4]
        assert sorted(sym.ACTION_PERM[a]) == list(range(143))
        for x in range(5, 143):
            t, c = divmod(x - 5, 23)
            assert sym.ACTION_PERM[a][x] == 5 + 23 * t + sym.CELL_PERM[a][c] == sym.transform_action(x, a)


# ---- the games -------------------------------------------------------------------
def copy_stream(m):
    return oracle.MT.from_buffer_copy(bytes(m))


def stream_words(m):
    w, i = m.words()
    return w.tobytes(), i


@functools.lru_cache(maxsize=None)
def rule_games():
    """Six games: oracle.mt_seed(1000 + k), rule pick oracle.rule(k, ply).
    Every ply's state, the finals included: (states [382, 78], action per
    state or -1 at a final, the stream before and after the step)."""
    states, actions, before, after = [], [], [], []
    for k in range(6):
        m = oracle.mt_seed(1000 + k)
        s = oracle.reset(m)
        ply = 0
        while not oracle.is_game_over(s):
            mask = oracle.legal(s)
            L = int(mask.sum())
            a = int(np.flatnonzero(mask)[((oracle.rule(k, ply) >> 32) * L) >> 32])
            states.append(s)
            actions.append(a)
            before.append(copy_stream(m))
            r, s = oracle.step(s, a, m)
            assert r == 0
            after.append(copy_stream(m))
            ply += 1
        states.append(s)
        actions.append(-1)
        before.append(copy_stream(m))
        after.append(None)
    return np.stack(states), actions, before, after


def words_of(states78):
    """REFSTATE rows -> int64 [n, 6] torch tensor."""
    return torch.from_numpy(words_to_array([pack_ref(v) for v in states78]))


def refs_of(words):
    return np.stack([unpack_ref(w) for w in words.numpy()])


def spatial_map(board, g):
    """board [38, 5, 7] with each valid cell's column moved to the cell's
    image under g (tensor position x = q + 3, y = r + 2)."""
    out = np.zeros_like(board)
    for q, r in SORTED_COORDS:
        x, y = q + 3, r + 2
        x2, y2 = [(x, y), (6 - x, 4 - y), (x + y - 2, 4 - y), (8 - x - y, y)][g]
        out[:, y2, x2] = board[:, y, x]
    return out


def test_rule_games_cover_the_conditions():
    states, actions, _, _ = rule_games()
    assert len(states) == 382
    assert set(states[:, :46].reshape(-1).tolist()) == set(range(13))     # all 13 stack codes
    assert set(states[:, 73].tolist()) == {0, 1, 2, 3, 4}                 # every phase
    assert set(states[:, 72].tolist()) == {0, 1}                          # both movers
    assert sum(a < 0 for a in actions) == 6


@pytest.mark.parametrize("g", [1, 2, 3])
def test_rule_automorphism_against_oracle(g):
    """legal(g s) = g legal(s); step(g s, g a) on a copy of the stream =
    g step(s, a) with the same stream left behind (pile refills, final scores
    and winner included); encode(g s) = the spatially mapped encode(s)."""
    states, actions, before, after = rule_games()
    gstates = refs_of(sym.transform_states(words_of(states), g))
    nxt = {i: oracle.step(states[i], actions[i], copy_stream(before[i]))[1]
           for i in range(len(states)) if actions[i] >= 0}
    order = sorted(nxt)
    gnext = dict(zip(order, refs_of(sym.transform_states(words_of([nxt[i] for i in order]), g))))
    ap = np.array(sym.ACTION_PERM[g])
    valid = np.zeros((5, 7), bool)
    for q, r in SORTED_COORDS:
        valid[r + 2, q + 3] = True
    for i, s in enumerate(states):
        gs = gstates[i]
        assert (gs[46:] == s[46:]).all()                                  # piles, hand, bag, flags, scores
        want = np.zeros(143, np.uint8)
        want[ap] = oracle.legal(s)
        assert (oracle.legal(gs) == want).all(), (g, i)
        b, gl = oracle.encode(s)
        gb, ggl = oracle.encode(gs)
        assert (b[:, ~valid] == 0).all()
        assert (gb == spatial_map(b, g)).all() and (ggl == gl).all(), (g, i)
        if actions[i] < 0:
            continue
        m = copy_stream(before[i])
        r, got = oracle.step(gs, sym.transform_action(actions[i], g), m)
        assert r == 0 and (got == gnext[i]).all(), (g, i)
        assert stream_words(m) == stream_words(after[i]), (g, i)


def test_transform_states_g0_and_per_item():
    states, _, _, _ = rule_games()
    w = words_of(states[::7])
    assert torch.equal(sym.transform_states(w, 0), w)
    gs = torch.arange(w.shape[0]) % 4
    mixed = sym.transform_states(w, gs)
    for g in range(4):
        assert torch.equal(mixed[gs == g], sym.transform_states(w, g)[gs == g])
        assert torch.equal(sym.transform_states(sym.transform_states(w, g), g), w)


# ---- records ---------------------------------------------------------------------
def make_records(n=96, seed=5):
    """Records over game states with random u16 slots, z cycling, both players."""
    states, _, _, _ = rule_games()
    gen = torch.Generator().manual_seed(seed)
    w = words_of(states[torch.randperm(len(states), generator=gen)[:n].numpy()])
    visits = torch.randint(0, 65536, (n, 143), generator=gen, dtype=torch.int32)
    visits[torch.rand(n, 143, generator=gen) < 0.5] = 0
    z = (torch.arange(n) % 3 - 1).to(torch.float32)
    player = (torch.arange(n) // 3 % 2).to(torch.int8)
    return w, visits, z, player


def test_transform_records_cpu():
    w, visits, z, player = make_records()
    rec = hd.pack_records(w, visits, z, player)
    for g in range(4):
        got = sym.transform_records(rec, g)
        want = hd.pack_records(sym.transform_states(w, g), sym.transform_visits(visits, g), z, player)
        assert torch.equal(got, want)
        assert torch.equal(sym.transform_records(got, g), rec)            # an involution
        _, v2, z2, p2 = hd.unpack_records(got)
        assert torch.equal(z2, z) and torch.equal(p2, player)
        for a in (0, 4, 5, 77, 142):                                      # the entry of a moves to g a
            assert torch.equal(v2[:, sym.ACTION_PERM[g][a]], visits[:, a])
    assert torch.equal(sym.transform_records(rec, 0), rec)
    gs = torch.arange(rec.shape[0]) % 4
    mixed = sym.transform_records(rec, gs)
    for g in range(4):
        assert torch.equal(mixed[gs == g], sym.transform_records(rec, g)[gs == g])
    assert torch.equal(sym.transform_records(rec, gs.to(torch.uint8)), mixed)
    assert torch.equal(sym.transform_records(rec[:0], 2), rec[:0])


def test_bits_outside_the_cell_sets_survive():
    w, visits, z, player = make_records(n=24)
    gen = torch.Generator().manual_seed(9)
    junk = torch.randint(-2 ** 62, 2 ** 62, (24, 4), generator=gen, dtype=torch.int64) & ~CELL_BITS
    junk[0] = ~CELL_BITS                                                  # all of them, the sign bit too
    w2 = w.clone()
    w2[:, :4] |= junk
    rec = hd.pack_records(w2, visits, z, player)
    for g in range(4):
        got = sym.transform_records(rec, g)
        assert torch.equal(got[:, :4] & ~CELL_BITS, junk)
        assert torch.equal(got[:, :4] & CELL_BITS, sym.transform_states(w, g)[:, :4] & CELL_BITS)
        assert torch.equal(got[:, 4:6], rec[:, 4:6])


# ---- sources and the configuration key ---------------------------------------------
def test_sym_record_source_lengths_and_modes():
    from hzamd.train import SymRecordSource
    rec = torch.zeros(10, 42, dtype=torch.int64)
    assert len(SymRecordSource(rec, "random")) == 10
    assert len(SymRecordSource(rec, "all")) == 40
    with pytest.raises(ValueError):
        SymRecordSource(rec, "none")


def test_all_mode_index_arithmetic(monkeypatch):
    """Item i of mode "all" is record i >> 2 under symmetry i & 3."""
    import hzamd.train as ht
    seen = {}

    def fake(records, idx, sym=None):
        seen.update(idx=idx.clone(), sym=sym.clone())
        return ()
    monkeypatch.setattr(ht, "train_batch", fake)
    src = ht.SymRecordSource(torch.zeros(10, 42, dtype=torch.int64), "all")
    i = torch.tensor([0, 1, 2, 3, 4, 39, 17, 22])
    src.batch(i)
    assert seen["idx"].tolist() == [0, 0, 0, 0, 1, 9, 4, 5]
    assert seen["sym"].tolist() == [0, 1, 2, 3, 0, 3, 1, 2] and seen["sym"].dtype == torch.uint8
    assert torch.equal(src.last_sym, seen["sym"])
    # every (record, symmetry) pair exactly once over the whole range
    src.batch(torch.arange(40))
    pairs = set(zip(seen["idx"].tolist(), seen["sym"].tolist()))
    assert pairs == {(r, g) for r in range(10) for g in range(4)}


def test_random_mode_draws_per_item(monkeypatch):
    import hzamd.train as ht
    monkeypatch.setattr(ht, "train_batch", lambda records, idx, sym=None: (idx, sym))
    rec = torch.zeros(300, 42, dtype=torch.int64)
    a = ht.SymRecordSource(rec, "random", generator=torch.Generator().manual_seed(4))
    b = ht.SymRecordSource(rec, "random", generator=torch.Generator().manual_seed(4))
    idx = torch.arange(256)
    ia, sa = a.batch(idx)
    _, sb = b.batch(idx)
    assert torch.equal(ia, idx) and torch.equal(sa, sb) and torch.equal(a.last_sym, sa)
    assert sa.dtype == torch.uint8 and set(sa.tolist()) == {0, 1, 2, 3}
    assert not torch.equal(a.batch(idx)[1], sa)                           # a fresh draw per batch


def _trainer(tmp_path, training_extra):
    from hzamd.manager import ModelManager
    from hzamd.trainer import Trainer
    from test_manager_cpu import MODEL_CFG, TRAIN_CFG
    cfg = {"replay_buffer_size": 100, "checkpoint_folder": str(tmp_path / "ck"),
           "replay_buffer_folder": str(tmp_path / "buf"), "epochs_per_iter": 1}
    tc = dict(TRAIN_CFG, **training_extra)
    return Trainer(ModelManager(MODEL_CFG, tc), {}, cfg, tc, log=lambda *_: None)


def test_symmetry_config_key(tmp_path, monkeypatch):
    import hzamd.trainer as htr
    with pytest.raises(ValueError):
        _trainer(tmp_path, {"symmetry": "bogus"})
    calls = []
    monkeypatch.setattr(htr, "training_phase", lambda mgr, source, epochs, bs: calls.append(source))

    def boom(*a, **k):
        raise AssertionError("SymRecordSource built without the key")
    for extra in ({}, {"symmetry": "none"}):
        tr = _trainer(tmp_path, extra)
        monkeypatch.setattr(htr, "SymRecordSource", boom)
        monkeypatch.setattr(htr, "featurize", lambda rec: ("featurized", rec.shape[0]))
        tr.replay_buffer.extend(torch.zeros(7, 42, dtype=torch.int64))
        tr.execute_training_phase()
        assert calls.pop() == ("featurized", 7)
    for mode in ("random", "all"):
        tr = _trainer(tmp_path, {"symmetry": mode})
        monkeypatch.setattr(htr, "SymRecordSource", lambda rec, m: ("sym", rec.shape[0], m))
        monkeypatch.setattr(htr, "featurize", boom)
        tr.replay_buffer.extend(torch.zeros(5, 42, dtype=torch.int64))
        tr.execute_training_phase()
        assert calls.pop() == ("sym", 5, mode)
