"""Board symmetries on the GPU: hz_sym_records against the CPU record
transform, hz_train_batch against the per-batch path it replaces
(RecordSource.batch) and against its defining identity, the symmetric record
sources, one training phase, and a launch inside a captured graph.  All
comparisons are bit for bit."""
import functools

import numpy as np
import pytest
import torch

import oracle
from hzamd import _native as nat
from hzamd import distributed as hd
from hzamd import symmetry as sym
from hzamd.train import RecordSource, SymRecordSource, TensorSource, featurize, train_batch, training_phase
from test_symmetry_cpu import rule_games, words_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL_I = -0x0123456789ABCDEF
SENTINEL_F = -7.25


@functools.lru_cache(maxsize=None)
def fixture():
    """~400 records: the 382 game states and a stuck state (repeated to fill),
    random u16 slots with rows of all zeros, a single 65535 and all 143 set,
    z cycling through -1, 0, 1, both player bytes.  Returns the CPU records,
    their four CPU images and the device copy."""
    states, _, _, _ = rule_games()
    stuck, _ = oracle.stuck_state(77)
    rows = list(states) + [stuck] * 17
    n = len(rows)
    assert n == 399
    gen = torch.Generator().manual_seed(2024)
    visits = torch.randint(0, 65536, (n, 143), generator=gen, dtype=torch.int32)
    visits[torch.rand(n, 143, generator=gen) < 0.6] = 0
    visits[::50] = 0                                   # rows of all zeros (0, 50, ..)
    visits[1] = 0
    visits[1, 97] = 65535                              # a single full slot
    visits[2] = torch.randint(1, 65536, (143,), generator=gen, dtype=torch.int32)   # all 143 set
    visits[3] = 65535                                  # the largest sum
    visits[382] = 0                                    # the stuck state, once with no visits
    z = (torch.arange(n) % 3 - 1).to(torch.float32)
    player = (torch.arange(n) // 3 % 2).to(torch.int8)
    rec = hd.pack_records(words_of(rows), visits, z, player)
    images = [sym.transform_records(rec, g) for g in range(4)]
    return rec, images, rec.to(DEV)


def per_item_syms(n, seed=1):
    g = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    g[:4] = torch.tensor([0, 1, 2, 3], dtype=torch.uint8)[:n]
    return g


def raw_sym_records(rec_dev, m, symt, in_place):
    """hz_sym_records over the first m records into a buffer with one extra
    sentinel record, which must come back untouched."""
    buf = torch.full((m + 1, 42), SENTINEL_I, dtype=torch.int64, device=DEV)
    src = rec_dev[:m].contiguous()
    if in_place:
        buf[:m] = src
        src = buf
    rc = nat.lib().hz_sym_records(nat.ptr(src), m, nat.ptr(symt), nat.ptr(buf), nat.stream_ptr(DEV))
    assert rc == 0
    out = buf.cpu()
    assert (out[m] == SENTINEL_I).all()
    return out[:m]


@pytest.mark.parametrize("m", [0, 1, 2, 3, 63, 64, 65, 383])
def test_sym_records_equals_cpu_transform(m):
    rec, images, rec_dev = fixture()
    gs = per_item_syms(m)
    mixed = torch.stack([images[int(g)][j] for j, g in enumerate(gs)]) if m else rec[:0]
    for in_place in (False, True):
        assert torch.equal(raw_sym_records(rec_dev, m, None, in_place), rec[:m])          # NULL: a copy
        for g in range(4):
            symt = torch.full((m,), g, dtype=torch.uint8, device=DEV)
            assert torch.equal(raw_sym_records(rec_dev, m, symt, in_place), images[g][:m]), (g, in_place)
        # only the two low bits of a symmetry byte count
        noisy = (gs | 0xFC).to(DEV)
        assert torch.equal(raw_sym_records(rec_dev, m, gs.to(DEV), in_place), mixed)
        assert torch.equal(raw_sym_records(rec_dev, m, noisy, in_place), mixed)
    # the Python surface, out of place and in place
    assert torch.equal(sym.transform_records(rec_dev[:m], gs).cpu(), mixed)
    own = rec_dev[:m].clone()
    assert sym.transform_records(own, 3, out=own) is own and torch.equal(own.cpu(), images[3][:m])


def test_sym_records_rejects_bad_arguments():
    _, _, rec_dev = fixture()
    L = nat.lib()
    assert L.hz_sym_records(None, 1, None, nat.ptr(rec_dev), None) < 0
    assert L.hz_sym_records(nat.ptr(rec_dev), 1, None, None, None) < 0
    assert L.hz_sym_records(nat.ptr(rec_dev), -1, None, nat.ptr(rec_dev), None) < 0
    b = torch.empty(1, 38, 5, 7, device=DEV)
    assert L.hz_train_batch(nat.ptr(rec_dev), None, None, -1, nat.ptr(b), nat.ptr(b), nat.ptr(b), nat.ptr(b), None) < 0
    assert L.hz_train_batch(nat.ptr(rec_dev), None, None, 1, nat.ptr(b), nat.ptr(b), None, nat.ptr(b), None) < 0
    assert L.hz_train_batch(nat.ptr(rec_dev), None, None, 0, nat.ptr(b), nat.ptr(b), nat.ptr(b), nat.ptr(b), None) == 0


def raw_train_batch(rec_dev, idx, symt, m):
    """hz_train_batch into outputs that each carry one sentinel row after the
    last; returns (board, glob, pi, z[m, 1])."""
    shapes = ((38, 5, 7), (42,), (143,), (1,))
    outs = [torch.full((m + 1,) + s, SENTINEL_F, dtype=torch.float32, device=DEV) for s in shapes]
    rc = nat.lib().hz_train_batch(nat.ptr(rec_dev), nat.ptr(idx), nat.ptr(symt), m, *[nat.ptr(o) for o in outs],
                                  nat.stream_ptr(DEV))
    assert rc == 0
    for o in outs:
        assert (o[m] == SENTINEL_F).all()
    return tuple(o[:m] for o in outs)


def same(a, b):
    """Bit equality of two tuples of float tensors."""
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))
                                    for x, y in zip(a, b))


def index_cases(m, n):
    gen = torch.Generator().manual_seed(m)
    asc = torch.sort(torch.randperm(n, generator=gen)[:m]).values
    rep = torch.randint(0, min(n, 5), (m,), generator=gen)
    holes = torch.randperm(n, generator=gen)[:m]
    holes[::3] = -1
    if m > 1:
        holes[m - 1] = -1                              # the last item of the batch a hole
    return {"ascending": asc, "reversed": asc.flip(0), "repeats": rep, "holes": holes}


@pytest.mark.parametrize("m", [1, 2, 3, 7, 8, 9, 64, 65, 129])
def test_train_batch_identity_equals_record_source(m):
    """g = 0 (sym NULL, and sym all zero) against RecordSource.batch, all four
    outputs; m crosses the pair, block and wave edges of the encode kernel."""
    rec, _, rec_dev = fixture()
    n = rec.shape[0]
    parent = RecordSource(rec_dev)
    zeros = torch.zeros(m, dtype=torch.uint8, device=DEV)
    for name, idx in index_cases(m, n).items():
        live = (idx >= 0).to(DEV)
        want = parent.batch(idx.clamp_min(0).to(DEV))
        want = tuple(torch.where(live.reshape(-1, *[1] * (w.dim() - 1)), w, torch.zeros_like(w)) for w in want)
        i32 = idx.to(torch.int32).to(DEV)
        assert same(raw_train_batch(rec_dev, i32, None, m), want), name
        assert same(raw_train_batch(rec_dev, i32, zeros, m), want), name
        assert same(train_batch(rec_dev, idx.to(DEV)), want), name     # the wrapper takes int64 indices
    want = parent.batch(torch.arange(m, device=DEV))
    assert same(raw_train_batch(rec_dev, None, None, m), want)         # idx NULL: records 0..m-1
    assert same(train_batch(rec_dev[:m], None), want)
    pi = want[2]
    assert ((pi.sum(1) - 1).abs() < 1e-5).logical_or(pi.sum(1) == 0).all()


def test_train_batch_special_rows():
    """The rows the divide can go wrong on: no visits (zeros, no NaN), one
    full slot (exactly 1), all slots at 65535 (the largest integer sum)."""
    rec, _, rec_dev = fixture()
    _, _, pi, z = raw_train_batch(rec_dev, None, None, 4)
    pi = pi.cpu()
    assert (pi[0] == 0).all()
    assert pi[1, 97] == 1 and pi[1].sum() == 1
    assert (pi[3] == np.float32(1 / 143)).all()
    assert z.reshape(-1).tolist() == [-1.0, 0.0, 1.0, -1.0]


def test_train_batch_defining_identity():
    """hz_train_batch(rec, idx, g) = hz_train_batch(transform_records(rec[idx], g), NULL, 0), device against
    device, for per-item g over all four values; board and glob also equal
    hz_encode_states of transform_states."""
    from hzamd.selfplay import encode_states
    rec, _, rec_dev = fixture()
    n = rec.shape[0]
    for m in (5, 130, n):
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(m))[:m].to(DEV)
        gs = per_item_syms(m, seed=m).to(DEV)
        assert set(gs.tolist()) == {0, 1, 2, 3}
        got = raw_train_batch(rec_dev, idx.to(torch.int32), gs, m)
        sel = rec_dev.index_select(0, idx)
        moved = sym.transform_records(sel, gs)
        assert same(got, raw_train_batch(moved, None, None, m))
        assert same(got, RecordSource(moved).batch(torch.arange(m, device=DEV)))
        assert same(got[:2], encode_states(sym.transform_states(sel[:, :6].contiguous(), gs)))
        assert not same(got[:1], raw_train_batch(rec_dev, idx.to(torch.int32), None, m)[:1])
    # holes stay zero under any symmetry
    idx = torch.tensor([3, -1, 7, -1, -1], dtype=torch.int32, device=DEV)
    got = raw_train_batch(rec_dev, idx, torch.tensor([1, 2, 3, 0, 1], dtype=torch.uint8, device=DEV), 5)
    for o in got:
        assert (o[1] == 0).all() and (o[3:] == 0).all()


def test_all_mode_equals_featurized_images():
    rec, _, rec_dev = fixture()
    n = rec.shape[0]
    src = SymRecordSource(rec_dev, "all")
    assert len(src) == 4 * n
    i4 = torch.arange(4 * n, device=DEV)
    rec4 = sym.transform_records(rec_dev.index_select(0, i4 >> 2), i4 & 3)
    ref = featurize(rec4)
    assert isinstance(ref, TensorSource) and len(ref) == 4 * n
    perm = torch.randperm(4 * n, generator=torch.Generator().manual_seed(8)).to(DEV)
    for s in range(0, 4 * n, 500):
        i = perm[s:s + 500]
        assert same(src.batch(i), ref.batch(i))
        assert torch.equal(src.last_sym, (i & 3).to(torch.uint8))


def test_random_mode_is_seeded_and_covers_the_group():
    rec, _, rec_dev = fixture()
    idx = torch.randperm(rec.shape[0], generator=torch.Generator().manual_seed(6))[:256].to(DEV)
    runs = []
    for _ in range(2):
        src = SymRecordSource(rec_dev, "random", generator=torch.Generator(device=DEV).manual_seed(31))
        assert len(src) == rec.shape[0]
        first = src.batch(idx)
        s1 = src.last_sym
        assert s1.dtype == torch.uint8 and s1.device.type == "cuda" and s1.shape == (256,)
        assert same(first, train_batch(rec_dev, idx, s1))
        second = src.batch(idx)
        runs.append((first, s1, second, src.last_sym))
    a, b = runs
    assert torch.equal(a[1], b[1]) and torch.equal(a[3], b[3]) and same(a[0], b[0]) and same(a[2], b[2])
    assert not torch.equal(a[1], a[3])                                 # a fresh draw per batch
    assert set(a[1].tolist()) == {0, 1, 2, 3}                          # all four within 256 draws


def test_training_phase_over_all_images():
    from hzamd.manager import ModelManager
    from test_manager_cpu import MODEL_CFG, TRAIN_CFG
    _, _, rec_dev = fixture()
    torch.manual_seed(0)
    mgr = ModelManager(MODEL_CFG, dict(TRAIN_CFG, device=DEV))
    res = training_phase(mgr, SymRecordSource(rec_dev[100:164], "all"), epochs=1, batch_size=32,
                         generator=torch.Generator(device=DEV).manual_seed(1), graph=False)
    assert res["batches"] == 8
    assert all(np.isfinite(res[k]) for k in ("loss", "policy_loss", "value_loss"))


def test_train_batch_inside_a_captured_graph():
    """One hz_train_batch launch captured on a side stream and replayed over
    changed idx and sym contents: the kernel reads its arguments from memory
    and keeps no host state.  The graph is a single chain."""
    rec, _, rec_dev = fixture()
    m = 33
    idx = torch.arange(m, dtype=torch.int32, device=DEV)
    gs = torch.zeros(m, dtype=torch.uint8, device=DEV)
    train_batch(rec_dev, idx, gs)                                      # (library loaded before the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = train_batch(rec_dev, idx, gs)
    torch.cuda.current_stream(DEV).wait_stream(side)
    for k in (1, 2):
        gen = torch.Generator().manual_seed(40 + k)
        new_idx = torch.randperm(rec.shape[0], generator=gen)[:m].to(torch.int32)
        new_idx[5 * k] = -1
        new_g = per_item_syms(m, seed=50 + k)
        idx.copy_(new_idx)
        gs.copy_(new_g)
        graph.replay()
        torch.cuda.synchronize()
        got = tuple(o.clone() for o in out)
        assert same(got, train_batch(rec_dev, idx.clone(), gs.clone())), k
        assert (got[0][5 * k] == 0).all() and (got[2][5 * k] == 0).all()
    assert not same(got[:1], (train_batch(rec_dev, torch.arange(m, device=DEV))[0],))
