"""The network kernels at depths and value-head widths other than 128x8x256.

FoldedNet sends every 128-filter network to the HIP kernels, whatever its
num_res_blocks (R) and value_head_hidden_dim (H); the kernels' indexing
depends on the number of tower convs (2 R): the resident and split towers'
bias tables, weight stream, hand-off parity and last-conv epilogue, the
one-launch tower's pointer arrays, and the dispatch's limits (a resident pack
up to 64 convs, the one-launch tower up to 16 blocks, the fused head at H =
256 only).  Every other GPU test builds the default net, so each of these has
otherwise run at one depth.  Here:

1. the whole forward at six shapes against the unfolded float64 network,
   with the kernel wrappers FoldedNet went through counted;
2. a row's result bit-identical through every kernel form, at every depth;
3. the tower entry points on slices of a 32-block net's weights, against the
   chain of layered one-state convs, bit for bit, and their refusals;
4. a graph-replayed search on a 3-block, hidden-64 net.
"""
import collections
import functools

import pytest
import torch

from hzamd._native import NativeError, lib
from hzamd.infer import (FoldedNet, SPLIT_TIMEOUT_WORD, _conv3x3_x6_act, _conv3x3_xn_act, _resblock_x6, _stem_x6_act,
                         _tower_blocks_x6, _tower_resident, _tower_split, split_max_batch)
from hzamd.mcts import BatchedPredictor
from hzamd.net import HarmoniesNet
from test_infer_cpu import NET_SHAPES, _randomise_bn

pytestmark = pytest.mark.gpu

CL = torch.channels_last
ROWS64 = 33                # rows with a float64 reference
ROWS = 803                 # 100 eight-state groups and 3 rows: the large-batch forms
TOL = 1e-4                 # the project's bound on logits, value and probabilities against float64

TOWER_FORMS = ("_tower_split", "_tower_resident", "_tower_blocks_x6", "_resblock_x6", "_conv3x3_x6_act",
               "_conv3x3_xn_act", "_conv3x3_act")
HEAD_FORMS = ("_heads_fc", "_heads")

Case = collections.namedtuple("Case", "net fnet board glob l64 v64 l32 v32")


def _case(R, H=256):
    return _build_case(R, H)


@functools.lru_cache(maxsize=None)
def _build_case(R, H):
    """The R-block net with value-head width H and random BatchNorm
    statistics, folded on the GPU; 803 encoder-like rows; the unfolded
    network's outputs for the first 33 of them in float64 and in fp32, on
    the CPU.  Computed once per shape and never modified."""
    g = torch.Generator().manual_seed(100 + R)
    torch.manual_seed(R)
    net = HarmoniesNet(dict(num_res_blocks=R, value_head_hidden_dim=H)).eval()
    _randomise_bn(net, g)
    board = (torch.rand(ROWS64, 38, 5, 7, generator=g) > 0.8).float()
    glob = torch.rand(ROWS64, 42, generator=g)
    more = (torch.rand(ROWS - ROWS64, 38, 5, 7, generator=g) > 0.8).float()
    more[:, 37] = torch.randint(0, 3, (ROWS - ROWS64, 1, 1), generator=g).float() / 3.0
    board = torch.cat((board, more))
    glob = torch.cat((glob, torch.rand(ROWS - ROWS64, 42, generator=g)))
    with torch.no_grad():
        l64, v64 = net.double()(board[:ROWS64].double(), glob[:ROWS64].double())
        net.float()
        l32, v32 = net(board[:ROWS64], glob[:ROWS64])
    fnet = FoldedNet(net.to("cuda"))
    return Case(net, fnet, board.cuda(), glob.cuda(), l64, v64, l32, v32)


@pytest.fixture
def calls(monkeypatch):
    """Counts the kernel wrappers FoldedNet._run goes through (a refused
    launch, which returns None, is not counted) and keeps what each returned
    last (.last)."""
    import hzamd.infer as inf
    seen = collections.Counter()
    seen.last = {}

    def spy(name, fn):
        def wrapped(*a, **k):
            r = fn(*a, **k)
            if r is not None:
                seen[name] += 1
                seen.last[name] = r
            return r
        return wrapped

    for name in TOWER_FORMS + HEAD_FORMS:
        monkeypatch.setattr(inf, name, spy(name, getattr(inf, name)))
    return seen


def _taken(calls):
    """(tower wrappers, head wrappers) called since the last look, with counts."""
    got = tuple({n: calls[n] for n in names if calls[n]} for names in (TOWER_FORMS, HEAD_FORMS))
    calls.clear()
    return got


def _small_tower(R, B, device):
    """The tower form of a batch of at most 896 rows at the default limits."""
    if R == 0:
        return {}
    if R > 32:
        return {"_resblock_x6": R}       # no resident pack: one launch per block, whatever the batch
    if B <= split_max_batch(device):   # 32 where the device holds every split launch
        return {"_tower_split": 1}
    return {"_tower_resident": 1}


def _rows(c, n):
    return c.board[:n].contiguous(), c.glob[:n].contiguous()


@pytest.mark.parametrize("R,H", NET_SHAPES)
def test_forward_matches_fp64_at_other_shapes(R, H, calls):
    """FoldedNet.forward and .predict at (R, H) as whole batches of 1, 11 and
    33 rows (the split tower with one row block per workgroup, with three,
    and the resident tower; R = 33 the per-block launches, R = 0 no tower)
    against the unfolded float64 network on the CPU: logits, value and
    probabilities within 1e-4, the bound the fp32 CPU network is held to as
    well.  The folded net's packs and the wrappers each run went through are
    asserted, so no shape can pass through the MIOpen fallback.

    Largest deviations from float64 measured on an MI355X over the three
    batches (the fp32 CPU network's in brackets; largest |logit| 2.9):

        (R, H)      logits              value               probabilities
        (0, 256)    1.3e-7 (2.3e-7)     3.6e-8 (2.6e-8)     2.2e-9
        (1, 256)    1.2e-7 (1.7e-7)     3.2e-8 (3.1e-8)     1.8e-9
        (3, 64)     2.2e-7 (2.2e-7)     4.0e-8 (6.7e-8)     3.0e-9
        (20, 512)   9.5e-7 (9.5e-7)     1.1e-7 (4.3e-8)     1.8e-8
        (32, 256)   3.1e-7 (2.2e-7)     1.1e-7 (1.3e-7)     3.2e-9
        (33, 256)   1.8e-6 (1.6e-6)     2.9e-7 (1.6e-7)     8.8e-8"""
    c = _case(R, H)
    fnet = c.fnet
    assert (c.l32.double() - c.l64).abs().max().item() <= TOL
    assert (c.v32.double() - c.v64).abs().max().item() <= TOL
    assert len(fnet.blocks) == R and fnet.vfc1[0].shape[0] == H
    assert fnet.stem_packed is not None and fnet.heads is not None
    assert (fnet.packed is not None) == (R >= 1)
    assert (fnet.resident is not None) == (1 <= R <= 32)
    assert (fnet.fc is not None) == (H == 256)
    if fnet.resident is not None:
        assert fnet.resident[0].shape[0] == 2 * R and fnet.resident[1].shape == (2 * R, 128)
    head = {"_heads_fc": 1} if H == 256 else {"_heads": 1}
    p64 = torch.softmax(c.l64, 1)
    worst = [0.0, 0.0, 0.0]
    for B in (1, 11, ROWS64):
        board, glob = _rows(c, B)
        want = _small_tower(R, B, board.device)
        lo, v = fnet(board, glob)
        assert _taken(calls) == (want, head), (R, B)
        pr, pv = fnet.predict(board, glob)
        assert _taken(calls) == (want, head), (R, B)
        assert lo.shape == (B, 143) and v.shape == (B, 1) and pr.shape == (B, 143) and pv.shape == (B,)
        dl = (lo.cpu().double() - c.l64[:B]).abs().max().item()
        dv = (v.cpu().double() - c.v64[:B]).abs().max().item()
        dp = (pr.cpu().double() - p64[:B]).abs().max().item()
        dpv = (pv.cpu().double() - c.v64[:B].reshape(-1)).abs().max().item()
        print(f"shape R={R} H={H} B={B}: logits {dl:.3g} value {dv:.3g} probabilities {dp:.3g} "
              f"predict's value {dpv:.3g}")
        worst = [max(a, b) for a, b in zip(worst, (dl, max(dv, dpv), dp))]
        assert dl <= TOL and dv <= TOL and dp <= TOL and dpv <= TOL, (R, H, B, dl, dv, dp, dpv)
    print(f"shape R={R} H={H} worst: logits {worst[0]:.3g} value {worst[1]:.3g} probabilities {worst[2]:.3g}; "
          f"fp32 CPU: logits {(c.l32.double() - c.l64).abs().max().item():.3g} "
          f"value {(c.v32.double() - c.v64).abs().max().item():.3g}; max |logit| {c.l64.abs().max().item():.3g}")


def _observe(fnet, calls, board, glob, live=None):
    """predict's and forward's results for a batch, and the tower form taken.
    With the fused head (H = 256) every stage is a HIP kernel: priors, value
    and logits.  Otherwise the HIP part ends at hz_heads' output (each
    head's flattened 1x1 conv || globals), which is what is compared: the
    linear layers behind it are PyTorch's, whose GEMM is chosen by the batch
    size (FoldedNet.row_independent is False there; the final outputs are
    held to float64 at every batch by test_forward_matches_fp64_at_other_shapes)."""
    p, v = fnet.predict(board, glob, live=live)
    tower, _ = _taken(calls)
    first = None if fnet.fc is not None else calls.last["_heads"]
    lo, lv = fnet(board, glob, live=live)
    assert _taken(calls)[0] == tower
    if fnet.fc is not None:
        return tower, (p, v, lo, lv)
    return tower, first + calls.last["_heads"]


def _same(got, want, k):
    return len(got) == len(want) and all(torch.equal(g[:k], w[:k]) for g, w in zip(got, want))


@pytest.mark.parametrize("R,H", [(1, 256), (3, 256), (3, 64), (20, 256), (20, 512), (32, 256), (33, 256)])
def test_rows_do_not_depend_on_kernel_form_at_any_depth(R, H, calls):
    """test_predict_rows_do_not_depend_on_batch_size at other depths: the
    same rows in batches of 1, 11, 33 and 803 give the same bits (see
    _observe for what is compared at H = 64 and 512).  803 rows run twice: at
    the default limits (the resident tower up to 32 blocks, which serves up
    to 896 rows; 33 launches of the fused block at R = 33) and with the
    resident tower limited to the split tower's 32 rows, where the batch
    takes hz_tower_x6_blocks (R = 1, 3: nblk = 1, 3) or one fused block per
    launch (R = 20, 32, 33).  Then each form with a live-row bound inside a
    workgroup (798 = 99 x 8 + 6 of 803; 6 of 11; 29 of 33)."""
    c = _case(R, H)
    fnet = c.fnet
    assert fnet.resident_max == 896 and fnet.split_max == 32 and fnet.tower_loop == 1
    assert fnet.row_independent == (H == 256)
    dev = c.board.device
    tower, full = _observe(fnet, calls, c.board, c.glob)
    assert tower == ({"_tower_resident": 1} if R <= 32 else {"_resblock_x6": R})
    assert all(bool(torch.isfinite(t).all()) for t in full)
    p_full = fnet.predict(c.board, c.glob)[0]
    assert float(p_full.max()) > 2.0 / 143  # the rows are told apart: not a dead tower's uniform prior
    calls.clear()
    k = ROWS - 5
    live = torch.tensor([k], dtype=torch.int32, device="cuda")
    try:
        fnet.resident_max = 32
        tower, big = _observe(fnet, calls, c.board, c.glob)
        tower_live, big_live = _observe(fnet, calls, c.board, c.glob, live)
    finally:
        fnet.resident_max = 896
    assert tower == tower_live == ({"_tower_blocks_x6": 1} if R <= 16 else {"_resblock_x6": R})
    assert _same(big, full, ROWS), "803 rows, large-batch forms"
    assert _same(big_live, full, k), "803 rows, large-batch forms, live rows"
    assert _same(_observe(fnet, calls, c.board, c.glob, live)[1], full, k)  # the resident tower (R = 33: per block)
    for s, k in ((1, 1), (11, 6), (ROWS64, 29)):
        board, glob = _rows(c, s)
        tower, got = _observe(fnet, calls, board, glob)
        assert tower == _small_tower(R, s, dev), (R, s)
        assert _same(got, full, s), (R, s)
        live = torch.tensor([k], dtype=torch.int32, device="cuda")
        tower, got = _observe(fnet, calls, board, glob, live)
        assert tower == _small_tower(R, s, dev), (R, s)
        assert _same(got, full, k), (R, s, k)


@pytest.mark.parametrize("R,H", NET_SHAPES)
def test_predictor_claims_row_independence_only_with_the_fused_head(R, H):
    """BatchedPredictor.row_independent (BatchedMCTS.search then gathers the
    leaf batch in arrival order) holds where every stage is a HIP kernel; at
    H = 64 and 512 the linear layers are PyTorch's and a row's value was seen
    to differ in its last bits between a batch of 1 and of 803 rows."""
    pred = BatchedPredictor(_case(R, H).net)
    assert pred.capturable and pred.row_independent == (H == 256)


# ---- kernel level: slices of the 32-block net's resident pack ----------------

def _pack32():
    """(allw [64], allb [64][128]) of the 32-block net."""
    return _case(32).fnet.resident


def _tower_input(n, tail=2):
    """The 32-block net's stem output for n rows (realistic magnitudes: the
    tests assert that the activations stay alive and finite over 64 convs),
    as the prefix of a buffer whose tail is NaN."""
    c = _case(32)
    x = _stem_x6_act(c.board[:n].contiguous(), c.fnet.stem_packed, c.fnet.stem[1])
    buf = torch.full((n + tail, 128, 5, 7), float("nan"), device="cuda").contiguous(memory_format=CL)
    buf[:n] = x
    return buf[:n]


def _chain(x, allw, allb, products=6, live=None):
    """The layered one-state convs, block by block (the towers' definition)."""
    for i in range(0, allw.shape[0], 2):
        if products == 6:
            y = _conv3x3_x6_act(x, allw[i], allb[i], None, live)
            x = _conv3x3_x6_act(y, allw[i + 1], allb[i + 1], x, live)
        else:
            y = _conv3x3_xn_act(x, allw[i], allb[i], None, live, products)
            x = _conv3x3_xn_act(y, allw[i + 1], allb[i + 1], x, live, products)
    return x


def _stream():
    return torch.cuda.current_stream().cuda_stream


SENTINEL = 7.25


def _resident_into(x, allw, allb, nconv, live=None):
    """hz_tower_x6_resident with nconv given apart from the tensors' sizes,
    into the prefix of a buffer whose other rows hold a sentinel -> (rc, the
    whole buffer)."""
    B = x.shape[0]
    out = torch.full((B + 2, 128, 5, 7), SENTINEL, device="cuda").contiguous(memory_format=CL)
    rc = lib().hz_tower_x6_resident(x.data_ptr(), allw.data_ptr(), allb.data_ptr(), out.data_ptr(), nconv, B,
                                    live.data_ptr() if live is not None else None, _stream())
    return rc, out


@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("nconv", [2, 6, 40, 64])
def test_resident_tower_x6_at_other_depths(nconv, batch):
    """hz_tower_x6_resident over the first nconv convs == the chain of
    layered one-state x6 convs, bit for bit, with and without a live bound;
    the input's NaN tail is not read and the output rows past the batch keep
    their sentinel; with a further, all-NaN conv (and bias row) behind the
    last one the result is the same: the weight stream's read-ahead past the
    last conv is clamped and feeds nothing."""
    allw, allb = _pack32()
    w, b = allw[:nconv], allb[:nconv]
    assert w.is_contiguous() and b.is_contiguous()
    x = _tower_input(batch)
    want = _chain(x, w, b)
    assert bool(torch.isfinite(want).all()) and float(want.max()) > 0
    if nconv > 2:  # the depths differ: a tower that stopped early or ran on would show
        assert not torch.equal(want, _chain(x, allw[:nconv - 2], allb[:nconv - 2]))
    got = _tower_resident(x, w, b)
    assert torch.equal(got, want)
    rc, out = _resident_into(x, w, b, nconv)
    assert rc == 0 and torch.equal(out[:batch], want) and bool((out[batch:] == SENTINEL).all())
    k = (batch + 1) // 2
    live = torch.tensor([k], dtype=torch.int32, device="cuda")
    rc, out = _resident_into(x, w, b, nconv, live)
    assert rc == 0 and torch.equal(out[:k], want[:k]) and bool((out[batch:] == SENTINEL).all())
    wn = torch.cat((w, torch.full_like(allw[:1], float("nan")))).contiguous()
    bn = torch.cat((b, torch.full_like(allb[:1], float("nan")))).contiguous()
    assert wn.shape[0] == nconv + 1 and bool(torch.isnan(wn[nconv].float()).all())
    rc, out = _resident_into(x, wn, bn, nconv)
    assert rc == 0 and torch.equal(out[:batch], want) and bool((out[batch:] == SENTINEL).all())


@pytest.mark.parametrize("products", [3, 1])
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("nconv", [2, 6, 64])
def test_resident_tower_xn_at_other_depths(nconv, batch, products):
    """hz_tower_xn_resident (3 or 1 piece products: the forms whose last conv
    the compiler peels, with the hand-written final wait) == the layered
    hz_conv3x3_xn_bias_act chain, bit for bit, with and without a live bound."""
    allw, allb = _pack32()
    w, b = allw[:nconv], allb[:nconv]
    x = _tower_input(batch)
    want = _chain(x, w, b, products)
    assert bool(torch.isfinite(want).all()) and float(want.max()) > 0
    assert not torch.equal(want, _chain(x, w, b))  # not the x6 tower
    assert torch.equal(_tower_resident(x, w, b, None, products), want)
    k = (batch + 1) // 2
    live = torch.tensor([k], dtype=torch.int32, device="cuda")
    assert torch.equal(_tower_resident(x, w, b, live, products)[:k], want[:k])


def test_split_tower_at_other_depths_back_to_back():
    """hz_tower_x6_split over 64, 2, 6 and 64 convs, back to back on one
    counter block, at 1, 10, 11 and 32 states (one row block per workgroup
    up to 10, three above) == hz_tower_x6_resident bit for bit; after every
    launch no hand-off has timed out and every counter is zero again (a
    counter left by one depth would release the next depth's waits early or
    never); one case with a live bound.  Batches above the device's
    split_max_batch are left out and counted; batch 1 always runs."""
    allw, allb = _pack32()
    cap = split_max_batch(torch.device("cuda", torch.cuda.current_device()))
    ran, skipped = [], 0
    for nconv in (64, 2, 6, 64):
        w, b = allw[:nconv], allb[:nconv]
        for batch in (1, 10, 11, 32):
            if batch > cap:
                skipped += 1
                continue
            x = _tower_input(batch)
            want = _tower_resident(x, w, b)
            sync = []
            got = _tower_split(x, w, b, sync_out=sync)
            assert got is not None, (nconv, batch)
            torch.cuda.synchronize()
            assert int(sync[0][SPLIT_TIMEOUT_WORD]) == 0 and not sync[0].any(), (nconv, batch)
            assert torch.equal(got, want), (nconv, batch)
            ran.append((nconv, batch))
            if (nconv, batch) in ((6, 11), (64, 1)):
                k = (batch + 1) // 2
                live = torch.tensor([k], dtype=torch.int32, device="cuda")
                got = _tower_split(x, w, b, live, sync_out=sync)
                torch.cuda.synchronize()
                assert int(sync[1][SPLIT_TIMEOUT_WORD]) == 0 and not sync[1].any(), (nconv, batch)
                assert torch.equal(got[:k], want[:k]), (nconv, batch)
    print(f"split tower: {len(ran)} launches compared, {skipped} left out (split_max_batch {cap})")
    assert cap >= 1 and all((n, 1) in ran for n in (64, 2, 6))
    assert len(ran) + skipped == 16


@pytest.mark.parametrize("batch", [769, 803])
@pytest.mark.parametrize("nblk", [1, 3, 16])
def test_one_launch_tower_at_other_depths(nblk, batch):
    """hz_tower_x6_blocks over the first nblk blocks == nblk
    hz_resblock_x6_bias_act launches, bit for bit, with both row tables; the
    input (NaN behind its last row) is left unchanged."""
    c = _case(32)
    fnet = c.fnet
    x = _tower_input(batch, tail=9)
    x0 = x.clone()
    assert lib().hz_resblock_x6_fused(batch) == 1
    try:
        for table in (0, 1):
            assert lib().hz_resblock_x6_set_table(table) == 0
            ref = x
            for ((_, b1), (_, b2)), (p1, p2) in list(zip(fnet.blocks, fnet.packed))[:nblk]:
                ref = _resblock_x6(ref, p1, b1, p2, b2)
            tw = _tower_blocks_x6(x, fnet._tw_ptrs, nblk)
            assert tw is not None and torch.equal(tw, ref), table
            assert bool(torch.isfinite(tw).all()) and float(tw.max()) > 0
            assert torch.equal(x, x0)
    finally:
        lib().hz_resblock_x6_set_table(1)
    if nblk > 1:
        assert not torch.equal(tw, _tower_blocks_x6(x, fnet._tw_ptrs, nblk - 1))


@pytest.mark.parametrize("nconv", [0, 1, 3, 66])
def test_tower_entry_points_refuse_other_conv_counts(nconv):
    """An odd conv count, fewer than 2 or more than 64 convs: the resident
    (x6, x3, x1) and split entry points return -1 with nothing enqueued (the
    output keeps its sentinel) and the wrappers raise NativeError."""
    allw, allb = _pack32()
    allw66 = torch.cat((allw, allw[:2])).contiguous()
    allb66 = torch.cat((allb, allb[:2])).contiguous()
    w, b = allw66[:nconv], allb66[:nconv]
    B = 2
    x = _tower_input(B)
    out = torch.full_like(x, SENTINEL, memory_format=CL)
    xch = torch.zeros(2 * B * 35 * 128, device="cuda")
    sync = torch.zeros(33 * 32, dtype=torch.int32, device="cuda")
    L, s = lib(), _stream()
    # the tensors hold 66 convs: a launch that went ahead would stay inside them
    assert L.hz_tower_x6_resident(x.data_ptr(), allw66.data_ptr(), allb66.data_ptr(), out.data_ptr(), nconv, B,
                                  None, s) == -1
    for products in (6, 3, 1):
        assert L.hz_tower_xn_resident(x.data_ptr(), allw66.data_ptr(), allb66.data_ptr(), out.data_ptr(), nconv, B,
                                      None, products, s) == -1
    assert L.hz_tower_x6_split(x.data_ptr(), allw66.data_ptr(), allb66.data_ptr(), out.data_ptr(), xch.data_ptr(),
                               sync.data_ptr(), nconv, B, None, s) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and not sync.any()
    for products in (6, 3, 1):
        with pytest.raises(NativeError, match=r"\(-1\)"):
            _tower_resident(x, w, b, None, products)
    with pytest.raises(NativeError, match=r"\(-1\)"):
        _tower_split(x, w, b)


@pytest.mark.parametrize("nblk", [0, 17])
def test_one_launch_tower_refuses_other_block_counts(nblk):
    """hz_tower_x6_blocks takes 1 to 16 blocks: -1 otherwise, nothing
    enqueued, and the wrapper raises NativeError (it returns None only for a
    batch the per-block path serves)."""
    fnet = _case(32).fnet
    x = _tower_input(ROWS, tail=1)
    assert lib().hz_resblock_x6_fused(ROWS) == 1
    out = torch.full_like(x, SENTINEL, memory_format=CL)
    tmp = torch.full_like(x, SENTINEL, memory_format=CL)
    w1, b1, w2, b2 = fnet._tw_ptrs  # 32 pointers each
    assert lib().hz_tower_x6_blocks(x.data_ptr(), w1, b1, w2, b2, nblk, out.data_ptr(), tmp.data_ptr(), ROWS, None,
                                    _stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((tmp == SENTINEL).all())
    with pytest.raises(NativeError, match=r"\(-1\)"):
        _tower_blocks_x6(x, fnet._tw_ptrs, nblk)


def test_search_graph_replay_equals_eager_on_a_3_block_net(calls):
    """test_search_graph_replay_equals_eager on a 3-block, hidden-64 net (8
    boards, 6 simulations): the captured simulation bakes in the split
    tower's counter block; it replays to the eager search's visit counts
    with 6 convs per launch and the unfused head's linear layers captured."""
    from hzamd.env import BatchedEnv
    from hzamd.mcts import BatchedMCTS
    pred = BatchedPredictor(_case(3, 64).net)
    assert pred.capturable and pred.fast.resident[0].shape[0] == 6 and pred.fast.fc is None
    import hzamd.infer as inf
    n = 8
    out = []
    for graph in (False, True):
        env = BatchedEnv(n, seed_base=77, device="cuda:0")
        env.reset()
        mcts = BatchedMCTS(env, 6)
        out.append(mcts.search(pred, 2.0, graph=graph).clone().cpu())
        inf.check_split_timeouts()
        mcts.close()
        env.close()
        assert calls["_tower_split"] > 0 and calls["_heads"] > 0
        assert not any(calls[f] for f in TOWER_FORMS if f != "_tower_split") and not calls["_heads_fc"]
        calls.clear()
    assert int(out[0].sum()) == n * (6 - 1)  # the first simulation expands the root
    assert torch.equal(out[0], out[1])
