"""Networks of other filter counts and head shapes on the HIP path.

FoldedNet sends a network with cnn_filters F in {32, 64, .., 256} other than
128 (bf16 tower modes) through csrc/hz_net_wide.hip: the width-generic stem
and conv (hz_stem3x3_x6g_bias_act, hz_conv3x3_x6g_bias_act: one- and
eight-state workgroup forms with identical bits) and the generic fused head
(hz_heads_fc_g).  Here:

1. the whole forward at six shapes against the unfolded float64 network, the
   wrappers it went through spied on;
2. a row's result bit-identical in any batch, either form, under a live bound;
3. the conv at cin = cout = 128 against the 128-wide kernels, bit for bit;
4. the conv and the stem at other widths against float64 with a derived bound;
5. the head's logits against float64 with a derived bound;
6. the entry points' refusals;
7. a graph-replayed search and the self-play split invariance on TINY.
"""
import collections
import functools

import pytest
import torch
import torch.nn.functional as F

from hzamd._native import NativeError, lib
from hzamd.infer import (FoldedNet, _conv3x3_x6_act, _conv3x3_x6g_act, _conv3x3_xn_act, _heads_fc_g, _stem_x6g_act,
                         pack_conv3x3_x6, pack_stem_x6g)
from hzamd.mcts import BatchedPredictor
from hzamd.net import TINY, HarmoniesNet
from test_infer_cpu import _randomise_bn

pytestmark = pytest.mark.gpu

CL = torch.channels_last
ROWS64 = 33     # rows with a float64 reference
ROWS = 300      # 37 eight-state groups and 4 rows
TOL = 1e-4      # the project's bound on logits, value and probabilities against float64
U = 2.0 ** -24  # fp32 unit roundoff
SENTINEL = 7.25

# (cnn_filters, num_res_blocks, value_head_hidden_dim, policy filters, value filters)
SHAPES = [(32, 1, 64, 2, 1), (64, 3, 256, 2, 1), (96, 2, 128, 1, 1), (256, 2, 512, 4, 3), (64, 0, 256, 2, 1),
          (32, 33, 64, 2, 1)]
NEW_FORMS = ("_stem_x6g_act", "_conv3x3_x6g_act", "_heads_fc_g")
OLD_FORMS = ("_tower_split", "_tower_resident", "_tower_blocks_x6", "_resblock_x6", "_conv3x3_x6_act",
             "_conv3x3_xn_act", "_conv3x3_act", "_heads_fc", "_heads", "_stem_x6_act", "_stem_act", "_bias_act")

Case = collections.namedtuple("Case", "net fnet board glob l64 v64 l32 v32")


def _cfg(shape):
    f, r, h, pf, vf = shape
    return dict(cnn_filters=f, num_res_blocks=r, value_head_hidden_dim=h, policy_head_conv_filters=pf,
                value_head_conv_filters=vf)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """The network of `shape` with random BatchNorm statistics, folded on the
    GPU; 300 encoder-like rows (0/1 planes, channel 37 in {0, 1/3, 2/3},
    uniform globals); the unfolded network's outputs for the first 33 in
    float64 and fp32 on the CPU.  Computed once per shape, never modified."""
    g = torch.Generator().manual_seed(200 + shape[0] + shape[1])
    torch.manual_seed(shape[0] + shape[1])
    net = HarmoniesNet(_cfg(shape)).eval()
    _randomise_bn(net, g)
    board = (torch.rand(ROWS, 38, 5, 7, generator=g) > 0.8).float()
    board[:, 37] = torch.randint(0, 3, (ROWS, 1, 1), generator=g).float() / 3.0
    glob = torch.rand(ROWS, 42, generator=g)
    with torch.no_grad():
        l64, v64 = net.double()(board[:ROWS64].double(), glob[:ROWS64].double())
        net.float()
        l32, v32 = net(board[:ROWS64], glob[:ROWS64])
    fnet = FoldedNet(net.to("cuda"))
    return Case(net, fnet, board.cuda(), glob.cuda(), l64, v64, l32, v32)


@pytest.fixture
def calls(monkeypatch):
    """Counts the kernel wrappers FoldedNet._run goes through, the 128-wide
    ones and F.conv2d / F.linear (as seen from hzamd.infer) included."""
    import hzamd.infer as inf
    seen = collections.Counter()

    def spy(name, fn):
        def wrapped(*a, **k):
            seen[name] += 1
            return fn(*a, **k)
        return wrapped

    for name in NEW_FORMS + OLD_FORMS:
        monkeypatch.setattr(inf, name, spy(name, getattr(inf, name)))
    for name in ("conv2d", "linear"):
        monkeypatch.setattr(inf.F, name, spy("F." + name, getattr(inf.F, name)))
    return seen


def _taken(calls):
    got = dict(calls)
    calls.clear()
    return got


def _expected(shape):
    return {"_stem_x6g_act": 1, "_heads_fc_g": 1, **({"_conv3x3_x6g_act": 2 * shape[1]} if shape[1] else {})}


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_matches_fp64_at_other_widths(shape, calls):
    """FoldedNet.forward and .predict as whole batches of 1, 11 and 33 rows
    against the unfolded float64 network on the CPU: logits, value and
    probabilities within 1e-4 (the fp32 CPU network is held to the same
    bound first).  Only the width-generic stem, conv and head wrappers ran:
    none of the 128-wide wrappers, no F.conv2d, no F.linear.  No two of the
    33 rows have equal logits (a dead tower would give every row the same).

    Largest deviations from float64 over the three batches, measured on an
    MI355X (the fp32 CPU network's in brackets):

        (F, R, H, pf, vf)      logits              value               probabilities
        (32, 1, 64, 2, 1)      2.2e-7 (2.9e-7)     2.4e-8 (2.4e-8)     3.3e-9
        (64, 3, 256, 2, 1)     2.3e-7 (2.2e-7)     6.8e-8 (7.7e-8)     3.1e-9
        (96, 2, 128, 1, 1)     2.1e-7 (2.1e-7)     3.7e-8 (4.4e-8)     2.3e-9
        (256, 2, 512, 4, 3)    1.2e-7 (1.2e-7)     3.7e-8 (3.6e-8)     1.7e-9
        (64, 0, 256, 2, 1)     1.5e-7 (2.1e-7)     3.2e-8 (3.4e-8)     2.2e-9
        (32, 33, 64, 2, 1)     7.3e-7 (5.9e-7)     4.9e-8 (4.4e-8)     1.0e-8"""
    c = _case(shape)
    fnet = c.fnet
    assert (c.l32.double() - c.l64).abs().max().item() <= TOL
    assert (c.v32.double() - c.v64).abs().max().item() <= TOL
    assert fnet.wide is not None and fnet.wide["dims"] == (shape[3], shape[4], shape[2])
    assert len(fnet.blocks) == shape[1] and fnet.stem[0].shape[0] == shape[0]
    p64 = torch.softmax(c.l64, 1)
    worst = [0.0, 0.0, 0.0]
    calls.clear()
    for B in (1, 11, ROWS64):
        board, glob = c.board[:B].contiguous(), c.glob[:B].contiguous()
        lo, v = fnet(board, glob)
        assert _taken(calls) == _expected(shape), (shape, B)
        pr, pv = fnet.predict(board, glob)
        assert _taken(calls) == _expected(shape), (shape, B)
        assert lo.shape == (B, 143) and v.shape == (B, 1) and pr.shape == (B, 143) and pv.shape == (B,)
        dl = (lo.cpu().double() - c.l64[:B]).abs().max().item()
        dv = (v.cpu().double() - c.v64[:B]).abs().max().item()
        dp = (pr.cpu().double() - p64[:B]).abs().max().item()
        dpv = (pv.cpu().double() - c.v64[:B].reshape(-1)).abs().max().item()
        print(f"shape {shape} B={B}: logits {dl:.3g} value {dv:.3g} probabilities {dp:.3g} predict's value {dpv:.3g}")
        worst = [max(a, b) for a, b in zip(worst, (dl, max(dv, dpv), dp))]
        assert dl <= TOL and dv <= TOL and dp <= TOL and dpv <= TOL, (shape, B, dl, dv, dp, dpv)
    print(f"shape {shape} worst: logits {worst[0]:.3g} value {worst[1]:.3g} probabilities {worst[2]:.3g}; "
          f"fp32 CPU: logits {(c.l32.double() - c.l64).abs().max().item():.3g} "
          f"value {(c.v32.double() - c.v64).abs().max().item():.3g}; max prior {p64.max().item():.3g}")
    rows = lo.cpu()
    assert all(not torch.equal(rows[i], rows[j]) for i in range(ROWS64) for j in range(i))


def _observe(fnet, board, glob, live=None):
    p, v = fnet.predict(board, glob, live=live)
    lo, lv = fnet(board, glob, live=live)
    return p, v, lo, lv


def _same(got, want, k):
    return len(got) == len(want) and all(torch.equal(g[:k], w[:k]) for g, w in zip(got, want))


@pytest.mark.parametrize("shape", SHAPES)
def test_rows_do_not_depend_on_batch_form_or_live(shape, calls):
    """The same rows in batches of 1, 11, 33 and 300, with the convs' form
    forced to one state per workgroup, to eight, and chosen by the batch,
    give the same bits for priors, value and logits; so do the rows below a
    live bound that falls inside an eight-state group (294 of 300, 6 of 11).
    FoldedNet and BatchedPredictor claim row independence."""
    c = _case(shape)
    calls.clear()
    fnet = c.fnet
    assert fnet.row_independent and fnet.wide_spg == 0
    pred = BatchedPredictor(c.net)
    assert pred.capturable and pred.row_independent
    try:
        fnet.wide_spg = 1
        full = _observe(fnet, c.board, c.glob)
        assert all(bool(torch.isfinite(t).all()) for t in full)
        for spg in (1, 8, 0):
            fnet.wide_spg = spg
            for n, k in ((1, 1), (11, 6), (ROWS64, 29), (ROWS, 294)):
                board, glob = c.board[:n].contiguous(), c.glob[:n].contiguous()
                assert _same(_observe(fnet, board, glob), full, n), (shape, spg, n)
                live = torch.tensor([k], dtype=torch.int32, device="cuda")
                assert _same(_observe(fnet, board, glob, live), full, k), (shape, spg, n, k)
    finally:
        fnet.wide_spg = 0
    assert not any(calls[n] for n in OLD_FORMS + ("F.conv2d", "F.linear"))


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("spg", [1, 8])
def test_rows_past_live_stay_untouched(spg):
    """Kernel level, 64 filters: with live = 6 of 11 rows the stem, the conv
    and the head write rows 0..5 as the unbounded call does and leave every
    other row of a sentinel-filled output as it was."""
    c = _case(SHAPES[1])
    fnet, wd = c.fnet, c.fnet.wide
    B, k, L = 11, 6, lib()
    live = torch.tensor([k], dtype=torch.int32, device="cuda")
    board = c.board[:B].contiguous()
    want = _stem_x6g_act(board, wd["stem"], fnet.stem[1], None, spg)
    out = torch.full((B + 2, 64, 5, 7), SENTINEL, device="cuda").contiguous(memory_format=CL)
    assert L.hz_stem3x3_x6g_bias_act(board.data_ptr(), wd["stem"].data_ptr(), fnet.stem[1].data_ptr(), out.data_ptr(),
                                     64, B, live.data_ptr(), spg, _stream()) == 0
    assert torch.equal(out[:k], want[:k]) and bool((out[k:] == SENTINEL).all())
    (_, b1), _ = fnet.blocks[0]
    p1 = wd["blocks"][0][0]
    want2 = _conv3x3_x6g_act(want, p1, b1, want, None, 6, spg)
    out.fill_(SENTINEL)
    assert L.hz_conv3x3_x6g_bias_act(want.data_ptr(), p1.data_ptr(), b1.data_ptr(), want.data_ptr(), out.data_ptr(),
                                     64, 64, B, live.data_ptr(), 6, spg, _stream()) == 0
    assert torch.equal(out[:k], want2[:k]) and bool((out[k:] == SENTINEL).all())
    glob = c.glob[:B].contiguous()
    lo0, pr0, v0 = _heads_fc_g(want2, glob, wd["hw"], wd["hb"], wd["fc"], wd["dims"], logits=True, probs=True)
    lo = torch.full((B + 2, 143), SENTINEL, device="cuda")
    pr, v = lo.clone(), torch.full((B + 2,), SENTINEL, device="cuda")
    assert L.hz_heads_fc_g(want2.data_ptr(), glob.data_ptr(), wd["hw"].data_ptr(), wd["hb"].data_ptr(),
                           *(t.data_ptr() for t in wd["fc"]), lo.data_ptr(), pr.data_ptr(), v.data_ptr(), 64,
                           *wd["dims"], B, live.data_ptr(), _stream()) == 0
    for got, ref in ((lo, lo0), (pr, pr0), (v, v0)):
        assert torch.equal(got[:k], ref[:k]) and bool((got[k:] == SENTINEL).all())


# ---- the conv at 128 against the 128-wide kernels -----------------------------

@pytest.mark.parametrize("batch", [1, 5, 19])
@pytest.mark.parametrize("products", [6, 3, 1])
def test_conv_at_128_equals_the_128_wide_kernels(products, batch):
    """hz_conv3x3_x6g_bias_act(cin = cout = 128) == hz_conv3x3_x6_bias_act
    (products 6) and hz_conv3x3_xn_bias_act (3, 1) bit for bit, in both
    workgroup forms, with and without the residual, on the 32-block net's
    stem output; the input's NaN tail is not read."""
    from test_net_shapes_gpu import _pack32, _tower_input
    allw, allb = _pack32()
    w, b = allw[0], allb[0]
    x = _tower_input(batch)
    for res in (None, x):
        if products == 6:
            want = _conv3x3_x6_act(x, w, b, res)
        else:
            want = _conv3x3_xn_act(x, w, b, res, None, products)
        assert bool(torch.isfinite(want).all()) and float(want.max()) > 0
        for spg in (1, 8):
            got = _conv3x3_x6g_act(x, w, b, res, None, products, spg)
            assert torch.equal(got, want), (products, batch, spg, res is not None)


# ---- the conv and the stem against float64 ------------------------------------

def _conv_bound(x, w, b, res, cin):
    """|err| <= (9 cin + 8) 2^-24 (sum |x||w| + |b| + |res|) per element: an
    fp32 sum of that many terms in any order, plus the dropped piece products."""
    s = F.conv2d(x.abs(), w.abs(), None, padding=1) + b.abs().view(1, -1, 1, 1)
    if res is not None:
        s = s + res.abs()
    return (9 * cin + 8) * U * s


@pytest.mark.parametrize("batch", [1, 9])
@pytest.mark.parametrize("cin,cout", [(32, 32), (64, 64), (96, 96), (256, 256), (64, 32), (32, 256)])
def test_conv_matches_fp64_at_other_widths(cin, cout, batch):
    """hz_conv3x3_x6g_bias_act (six products, both forms, with the residual)
    against torch's float64 relu(conv2d + bias + res) on the CPU, element by
    element within (9 cin + 8) 2^-24 (sum |x||w| + |b| + |res|); the two
    forms agree bit for bit; outputs finite and not all zero."""
    g = torch.Generator().manual_seed(cin * 1000 + cout + batch)
    x = torch.randn(batch, cin, 5, 7, generator=g).relu()
    w = torch.randn(cout, cin, 3, 3, generator=g) / (3.0 * cin ** 0.5)
    b = torch.randn(cout, generator=g) * 0.1
    res = torch.randn(batch, cout, 5, 7, generator=g).relu()
    want = (F.conv2d(x.double(), w.double(), b.double(), padding=1) + res.double()).relu()
    bound = _conv_bound(x.double(), w.double(), b.double(), res.double(), cin)
    xg = x.cuda().contiguous(memory_format=CL)
    rg = res.cuda().contiguous(memory_format=CL)
    pk, bg = pack_conv3x3_x6(w).cuda(), b.cuda()
    got = [_conv3x3_x6g_act(xg, pk, bg, rg, None, 6, spg) for spg in (1, 8)]
    assert torch.equal(got[0], got[1])
    out = got[0].cpu().double()
    assert bool(torch.isfinite(out).all()) and float(out.max()) > 0
    err = (out - want).abs()
    print(f"conv {cin}->{cout} B={batch}: max err {err.max().item():.3g}, max err/bound {(err / bound).max().item():.3g}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("batch", [1, 9])
@pytest.mark.parametrize("cout", [32, 64, 96, 256])
def test_stem_matches_fp64_at_other_widths(cout, batch):
    """hz_stem3x3_x6g_bias_act on encoder-like boards (channel 37 in
    {0, 1/3, 2/3}) against float64 with the same bound at 38 channels."""
    g = torch.Generator().manual_seed(cout + batch)
    board = (torch.rand(batch, 38, 5, 7, generator=g) > 0.8).float()
    board[:, 37] = torch.randint(0, 3, (batch, 1, 1), generator=g).float() / 3.0
    w = torch.randn(cout, 38, 3, 3, generator=g) / (3.0 * 38 ** 0.5)
    b = torch.randn(cout, generator=g) * 0.1
    want = F.conv2d(board.double(), w.double(), b.double(), padding=1).relu()
    bound = _conv_bound(board.double(), w.double(), b.double(), None, 38)
    pk, bg = pack_stem_x6g(w).cuda(), b.cuda()
    got = [_stem_x6g_act(board.cuda(), pk, bg, None, spg) for spg in (1, 8)]
    assert torch.equal(got[0], got[1])
    assert got[0].is_contiguous(memory_format=CL)
    out = got[0].cpu().double()
    assert bool(torch.isfinite(out).all()) and float(out.max()) > 0
    err = (out - want).abs()
    print(f"stem 38->{cout} B={batch}: max err {err.max().item():.3g}, max err/bound {(err / bound).max().item():.3g}")
    assert bool((err <= bound).all())


# ---- the head -------------------------------------------------------------------

def _gamma(n):
    return n * U / (1 - n * U)


@pytest.mark.parametrize("ch,pf,vf,hidden", [(32, 2, 1, 64), (64, 2, 1, 256), (96, 1, 1, 128), (256, 4, 3, 512)])
def test_head_logits_match_fp64(ch, pf, vf, hidden):
    """hz_heads_fc_g's logits against float64: the 1x1 conv is an fp32 sum of
    ch products and the bias (error e1 <= gamma(ch + 1) (sum |x||hw| + |hb|)
    per element of pcat, ReLU not increasing it), the linear layer a sum of
    np = 35 pf + 42 products and the bias over the computed pcat:
    |err| <= sum_k |wp[a][k]| e1[k] + gamma(np + 1) (sum_k (|pcat[k]| + e1[k]) |wp[a][k]| + |bp[a]|)."""
    g = torch.Generator().manual_seed(ch + hidden)
    B, np_, nv = 5, 35 * pf + 42, 35 * vf + 42
    x = torch.randn(B, ch, 5, 7, generator=g).relu()
    glob = torch.rand(B, 42, generator=g)
    hw = torch.randn(pf + vf, ch, generator=g) / ch ** 0.5
    hb = torch.randn(pf + vf, generator=g) * 0.1
    wp = torch.randn(143, np_, generator=g) / np_ ** 0.5
    bp = torch.randn(143, generator=g) * 0.1
    w1 = torch.randn(hidden, nv, generator=g) / nv ** 0.5
    b1 = torch.randn(hidden, generator=g) * 0.1
    w2 = torch.randn(hidden, generator=g) / hidden ** 0.5
    b2 = torch.randn(1, generator=g) * 0.1
    d = torch.float64
    pre = F.conv2d(x.to(d), hw[:pf].to(d).view(pf, ch, 1, 1), hb[:pf].to(d))
    e1 = _gamma(ch + 1) * (F.conv2d(x.to(d), hw[:pf].to(d).abs().view(pf, ch, 1, 1)) + hb[:pf].to(d).abs().view(1, -1, 1, 1))
    pcat = torch.cat((pre.relu().flatten(1), glob.to(d)), 1)
    e1 = torch.cat((e1.flatten(1), torch.zeros(B, 42, dtype=d)), 1)
    want = F.linear(pcat, wp.to(d), bp.to(d))
    bound = e1 @ wp.to(d).abs().t() + _gamma(np_ + 1) * ((pcat + e1) @ wp.to(d).abs().t() + bp.to(d).abs())
    fc = tuple(t.cuda().contiguous() for t in (wp.t(), bp, w1.t(), b1, w2, b2))
    lo, pr, v = _heads_fc_g(x.cuda().contiguous(memory_format=CL), glob.cuda(), hw.cuda(), hb.cuda(), fc,
                            (pf, vf, hidden), logits=True, probs=True)
    err = (lo.cpu().double() - want).abs()
    print(f"head ch={ch} pf={pf} vf={vf} hidden={hidden}: max err {err.max().item():.3g}, "
          f"max err/bound {(err / bound).max().item():.3g}")
    assert bool(torch.isfinite(lo).all()) and float(lo.abs().max()) > 0
    assert bool((err <= bound).all())
    assert bool(torch.isfinite(pr).all()) and bool(torch.isfinite(v).all()) and bool((v.abs() <= 1).all())


# ---- refusals -------------------------------------------------------------------

@pytest.mark.parametrize("cin,cout,products,spg", [(48, 32, 6, 0), (288, 32, 6, 0), (32, 0, 6, 0), (32, 32, 2, 0),
                                                   (32, 32, 6, 4)])
def test_conv_entry_point_refuses(cin, cout, products, spg):
    """cin = 48 or 288, cout = 0, products = 2, spg = 4: -1 with nothing
    enqueued (the output keeps its sentinel), and the wrapper raises."""
    B, co = 2, max(cout, 32)
    x = torch.rand(B, cin, 5, 7, device="cuda").contiguous(memory_format=CL)
    wp = torch.zeros(27 * cin * cout + 8, dtype=torch.bfloat16, device="cuda")  # (cout = 0: still a valid pointer)
    b = torch.zeros(co, device="cuda")
    out = torch.full((B, co, 5, 7), SENTINEL, device="cuda").contiguous(memory_format=CL)
    assert lib().hz_conv3x3_x6g_bias_act(x.data_ptr(), wp.data_ptr(), b.data_ptr(), None, out.data_ptr(), cin, cout, B,
                                         None, products, spg, _stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    if cout:
        with pytest.raises(NativeError, match=r"\(-1\)"):
            _conv3x3_x6g_act(x, wp[:27 * cin * cout], b[:cout], None, None, products, spg)


@pytest.mark.parametrize("cout,spg", [(48, 0), (0, 0), (288, 0), (32, 4)])
def test_stem_entry_point_refuses(cout, spg):
    """The stem with cout = 48, 0 or 288, or spg = 4: -1, nothing enqueued; the wrapper raises."""
    B, co = 2, max(cout, 32)
    board = torch.rand(B, 38, 5, 7, device="cuda")
    wp = torch.zeros(27 * 64 * co, dtype=torch.bfloat16, device="cuda")
    b = torch.zeros(co, device="cuda")
    out = torch.full((B, co, 5, 7), SENTINEL, device="cuda").contiguous(memory_format=CL)
    assert lib().hz_stem3x3_x6g_bias_act(board.data_ptr(), wp.data_ptr(), b.data_ptr(), out.data_ptr(), cout, B, None,
                                         spg, _stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    if cout:
        with pytest.raises(NativeError, match=r"\(-1\)"):
            _stem_x6g_act(board, wp, b, None, spg)


@pytest.mark.parametrize("pf,hidden", [(5, 64), (2, 1025)])
def test_head_entry_point_refuses(pf, hidden):
    """pf = 5, hidden = 1025: -1, the outputs keep their sentinel, the wrapper raises."""
    B, ch, vf = 2, 32, 1
    x = torch.rand(B, ch, 5, 7, device="cuda").contiguous(memory_format=CL)
    glob = torch.rand(B, 42, device="cuda")
    hw, hb = torch.zeros(pf + vf, ch, device="cuda"), torch.zeros(pf + vf, device="cuda")
    fc = (torch.zeros(35 * pf + 42, 143, device="cuda"), torch.zeros(143, device="cuda"),
          torch.zeros(35 * vf + 42, hidden, device="cuda"), torch.zeros(hidden, device="cuda"),
          torch.zeros(hidden, device="cuda"), torch.zeros(1, device="cuda"))
    lo = torch.full((B, 143), SENTINEL, device="cuda")
    v = torch.full((B,), SENTINEL, device="cuda")
    assert lib().hz_heads_fc_g(x.data_ptr(), glob.data_ptr(), hw.data_ptr(), hb.data_ptr(),
                               *(t.data_ptr() for t in fc), lo.data_ptr(), None, v.data_ptr(), ch, pf, vf, hidden, B,
                               None, _stream()) == -1
    torch.cuda.synchronize()
    assert bool((lo == SENTINEL).all()) and bool((v == SENTINEL).all())
    with pytest.raises(NativeError, match=r"\(-1\)"):
        _heads_fc_g(x, glob, hw, hb, fc, (pf, vf, hidden))


def test_other_widths_keep_the_fallback():
    """48 filters (not a multiple of 32), and 128 filters with three policy
    filters, stay on the MIOpen / PyTorch path and claim no row independence;
    so does a 64-filter net with tower="f32" or native_conv=False."""
    for cfg in (dict(cnn_filters=48, num_res_blocks=1), dict(policy_head_conv_filters=3, num_res_blocks=1)):
        fnet = FoldedNet(HarmoniesNet(cfg).eval().cuda())
        assert fnet.wide is None and not fnet.row_independent
    net = HarmoniesNet(dict(cnn_filters=64, num_res_blocks=1)).eval().cuda()
    assert FoldedNet(net).wide is not None
    for kw in (dict(tower="f32"), dict(native_conv=False)):
        fnet = FoldedNet(net, **kw)
        assert fnet.wide is None and not fnet.row_independent


# ---- search level, on TINY ---------------------------------------------------------

def test_search_graph_replay_equals_eager_on_tiny(calls):
    """test_search_graph_replay_equals_eager's recipe (8 boards, 6
    simulations) with the TINY predictor: the captured simulation replays to
    the eager search's visit counts through the width-generic kernels only."""
    from hzamd.env import BatchedEnv
    from hzamd.mcts import BatchedMCTS
    torch.manual_seed(0)
    pred = BatchedPredictor(HarmoniesNet(TINY).eval().cuda())
    assert pred.capturable and pred.row_independent and pred.fast.wide is not None
    n = 8
    out = []
    for graph in (False, True):
        calls.clear()
        env = BatchedEnv(n, seed_base=77, device="cuda:0")
        env.reset()
        mcts = BatchedMCTS(env, 6)
        out.append(mcts.search(pred, 2.0, graph=graph).clone().cpu())
        mcts.close()
        env.close()
        assert all(calls[f] > 0 for f in NEW_FORMS)
        assert not any(calls[f] for f in OLD_FORMS + ("F.conv2d", "F.linear"))
    assert int(out[0].sum()) == n * (6 - 1)  # the first simulation expands the root
    assert torch.equal(out[0], out[1])


def test_selfplay_split_invariant_on_tiny():
    """test_selfplay_split_invariant's recipe with the TINY predictor: 2 x 24
    boards give the same states, visit counts, validity and final states,
    board by board, as 1 x 48."""
    from hzamd.selfplay import SelfPlay
    cfg = {"num_simulations": 6, "cpuct": 2.0, "testing": False, "turns_until_tau0": 15}
    torch.manual_seed(0)
    ev = BatchedPredictor(HarmoniesNet(TINY).to("cuda:0").eval())
    assert ev.row_independent
    recs = [SelfPlay(n, ev, cfg, seed_base=base, device="cuda:0").play() for n, base in ((48, 700), (24, 700), (24, 724))]
    whole, parts = recs[0], recs[1:]
    for k, part in enumerate(parts):
        sl = slice(24 * k, 24 * k + 24)
        T = part["plies"]
        assert torch.equal(part["valid"], whole["valid"][:T, sl]) and not whole["valid"][T:, sl].any()
        assert torch.equal(part["states"], whole["states"][:T, :, sl])
        assert torch.equal(part["visits"], whole["visits"][:T, sl])
        assert torch.equal(part["final"], whole["final"][:, sl])
