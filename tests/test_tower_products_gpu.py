"""The reduced tower modes on the GPU: hz_conv3x3_xn_bias_act and
hz_tower_xn_resident keeping 3 (hh, hm, mh) or 1 (hh) of the six bf16 piece
products, through every kernel form (layered: 1 and 13 rows tiny, 300 small,
803 eight-state with a partly filled last group; resident: 1, 5, 64 rows),
and FoldedNet / BatchedPredictor / BatchedMCTS on top of them.

The bit-for-bit tests rest on the kernels issuing the kept products in the x6
kernels' order (tap by tap, pa outer, pb inner): a product the x6 kernel adds
as an exact zero can then be left out without changing a bit."""
import pytest
import torch

from hzamd._native import lib
from hzamd.infer import (FoldedNet, _conv3x3_x6_act, _conv3x3_xn_act, _heads_fc, _stem_x6_act, _tower_resident,
                         emulate_conv3x3, emulate_folded, pack_conv3x3_x6, split3_bf16)
from hzamd.mcts import BatchedPredictor
from hzamd.net import HarmoniesNet
from test_infer_cpu import _randomise_bn, torch_epilogue

pytestmark = pytest.mark.gpu

CL = torch.channels_last
LAYERED = [1, 13, 300, 803]
RESIDENT = [1, 5, 64]


def dev(t):
    return t.cuda().contiguous(memory_format=CL) if t.dim() == 4 and t.shape[1:] == (128, 5, 7) else t.cuda()


def pack(w):
    return pack_conv3x3_x6(w).cuda()


def xn(x, wp, b, r, k, live=None):
    return _conv3x3_xn_act(dev(x), wp, b.cuda(), dev(r) if r is not None else None, live, k)


def x6(x, wp, b, r):
    return _conv3x3_x6_act(dev(x), wp, b.cuda(), dev(r) if r is not None else None)


def bf(v):
    return v.bfloat16().float()


def t16(v):
    """v truncated to 16 significant bits: its split is exactly (h, m, 0)."""
    return (v.contiguous().view(torch.int32) & -256).view(torch.float32)


def data(batch, res, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 2 * batch + res)
    x = torch.randn(batch, 128, 5, 7, generator=g)
    w = torch.randn(128, 128, 3, 3, generator=g) * 0.03
    b = torch.randn(128, generator=g) * 0.1
    r = torch.randn(batch, 128, 5, 7, generator=g) if res else None
    return x, w, b, r


def with_low_piece(v16, g):
    """v16 (16 significant bits) plus a small d that lands in the third bf16
    piece only: d is zeroed wherever it would change the first two pieces."""
    d = v16.abs() * 2.0 ** -18 * (torch.rand(v16.shape, generator=g) - 0.5)
    v = v16 + d
    keep = (split3_bf16(v)[:2] == split3_bf16(v16)[:2]).all(0)
    v = torch.where(keep, v, v16)
    assert ((v != v16).float().mean().item()) > 0.5, "most elements keep d != 0"
    assert bool((split3_bf16(v)[:2] == split3_bf16(v16)[:2]).all())
    return v


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("batch", LAYERED)
def test_x1_is_x6_on_rounded_operands(batch, res):
    """x1 == x6 on bf16-rounded x and w, bit for bit: x6's other five
    products then add exact zeros in the same accumulation order."""
    x, w, b, r = data(batch, res, 1)
    got = xn(x, pack(w), b, r, 1)
    assert torch.equal(got, x6(bf(x), pack(bf(w)), b, r))
    assert not torch.equal(got, x6(x, pack(w), b, r))


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("batch", LAYERED)
def test_x3_computes_hm_and_mh(batch, res):
    """Operands of 16 significant bits split as (h, m, 0): against a
    bf16-valued other operand x6 has only the products x3 keeps."""
    x, w, b, r = data(batch, res, 2)
    for v in (t16(w), t16(x)):
        s = split3_bf16(v)
        assert bool((s[2] == 0).all()) and bool((s[1] != 0).any())
        assert torch.equal(s[0].double() + s[1].double(), v.double())
    wp = pack(t16(w))
    assert torch.equal(xn(bf(x), wp, b, r, 3), x6(bf(x), wp, b, r))
    wp = pack(bf(w))
    assert torch.equal(xn(t16(x), wp, b, r, 3), x6(t16(x), wp, b, r))
    # ... and the m pieces matter: dropping them (x1) changes the result
    assert not torch.equal(xn(t16(x), wp, b, r, 3), xn(t16(x), wp, b, r, 1))


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("batch", LAYERED)
def test_x3_drops_hl_and_lh(batch, res):
    """An operand with a third piece against a bf16-valued one: x3 gives what
    x6 gives without that piece, and not what x6 gives with it."""
    x, w, b, r = data(batch, res, 3)
    g = torch.Generator().manual_seed(batch)
    w16, x16 = t16(w), t16(x)
    wl, xl = with_low_piece(w16, g), with_low_piece(x16, g)
    got = xn(bf(x), pack(wl), b, r, 3)
    assert torch.equal(got, x6(bf(x), pack(w16), b, r))
    assert not torch.equal(got, x6(bf(x), pack(wl), b, r))
    wp = pack(bf(w))
    got = xn(xl, wp, b, r, 3)
    assert torch.equal(got, x6(x16, wp, b, r))
    assert not torch.equal(got, x6(xl, wp, b, r))


def _epilogue64(y, b, r):
    y = y + b.double().view(1, -1, 1, 1)
    if r is not None:
        y = y + r.double()
    return y.relu()


@pytest.mark.parametrize("res", [False, True])
def test_general_data_against_the_definition(res):
    """Real-valued data (test_conv3x3_x6_fp32_accuracy_vs_fp64's, n = 300):
    each mode is its emulation up to the x6 kernel's own fp32 accumulation
    error (2 e6 + 1e-7), and x3 is farther than that from the six-product
    emulation (a mode that kept all six would not be).  On unscaled x that
    gap measured 1.52e-5 on the GPU against a bound of 9.5e-6 (e6 4.7e-6):
    less than a factor 2, so x is scaled by 64 (exact: a power of two), as
    the feature's specification provides for this case (scaled: 9.76e-4
    against 5.9e-4; |xn - emu_k| 1.9e-4 for x3, 1.5e-4 for x1)."""
    n = 300
    g = torch.Generator().manual_seed(21)
    x = torch.randn(n, 128, 5, 7, generator=g).relu() * 64.0
    w = torch.randn(128, 128, 3, 3, generator=g) * 0.03
    b = torch.randn(128, generator=g) * 0.1
    r = torch.randn(n, 128, 5, 7, generator=g) if res else None
    want = _epilogue64(torch.nn.functional.conv2d(x.double(), w.double(), None, padding=1), b, r)
    wp = pack(w)
    e6 = (x6(x, wp, b, r).cpu().double() - want).abs().max().item()
    bound = 2 * e6 + 1e-7
    emu6 = _epilogue64(emulate_conv3x3(x, w, 6), b, r)
    for k in (3, 1):
        got = xn(x, wp, b, r, k).cpu().double()
        ek = (got - _epilogue64(emulate_conv3x3(x, w, k), b, r)).abs().max().item()
        gap = (got - emu6).abs().max().item()
        print(f"res={res} products={k}: |xn - emu_k| {ek:.3e}  |xn - emu_6| {gap:.3e}  bound {bound:.3e}")
        assert ek <= bound, (k, ek, bound)
        if k == 3:
            assert gap > bound, (gap, bound)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("batch", LAYERED)
def test_integer_data_exact(batch, res, k):
    """test_conv3x3_exact_on_integer_data's inputs are bf16 values: every
    mode equals the fp64 conv exactly (layout, tap and channel order)."""
    g = torch.Generator().manual_seed(batch * 2 + res)
    x = torch.randint(-3, 4, (batch, 128, 5, 7), generator=g).float()
    w = torch.randint(-2, 3, (128, 128, 3, 3), generator=g).float()
    b = torch.randint(-50, 50, (128,), generator=g).float()
    r = torch.randint(-20, 20, (batch, 128, 5, 7), generator=g).float() if res else None
    want = _epilogue64(torch.nn.functional.conv2d(x.double(), w.double(), None, padding=1), b, r).float()
    assert torch.equal(xn(x, pack(w), b, r, k).cpu(), want)


@pytest.mark.parametrize("k", [1, 3])
def test_layered_forms_agree(k):
    """A row's output does not depend on the form that computed it: rows
    [:m] of an eight-state run equal the tiny and small forms' runs."""
    x, w, b, r = data(1100, True, 6)
    x, r, wp = dev(x.relu()), dev(r), pack(w)
    full = xn(x, wp, b, r, k)
    for m in (1, 30, 767):
        assert torch.equal(xn(x[:m], wp, b, r[:m], k), full[:m]), m


def _tower4(batch, seed):
    g = torch.Generator().manual_seed(seed)
    x = dev(torch.randn(batch, 128, 5, 7, generator=g).relu())
    ws = [torch.randn(128, 128, 3, 3, generator=g) * 0.03 for _ in range(4)]
    allw = torch.stack([pack_conv3x3_x6(w) for w in ws]).cuda().contiguous()
    allb = (torch.randn(4, 128, generator=g) * 0.1).cuda().contiguous()
    return x, allw, allb


def _chain(x, allw, allb, k, live=None):
    for i in range(0, allw.shape[0], 2):
        y = _conv3x3_xn_act(x, allw[i], allb[i], None, live, k)
        x = _conv3x3_xn_act(y, allw[i + 1], allb[i + 1], x, live, k)
    return x


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("batch", RESIDENT)
def test_resident_tower_equals_layered_chain(batch, k):
    x, allw, allb = _tower4(batch, 60 + batch)
    got = _tower_resident(x, allw, allb, None, k)
    assert torch.equal(got, _chain(x, allw, allb, k))
    assert not torch.equal(got, _tower_resident(x, allw, allb))  # not the x6 tower
    live = torch.tensor([batch // 2], dtype=torch.int32, device="cuda")
    part = _tower_resident(x, allw, allb, live, k)
    assert torch.equal(part[:batch // 2], got[:batch // 2])


@pytest.mark.parametrize("k", [1, 3])
def test_live_rows(k):
    """A live-row bound (0, one row, a group and a row, 64 groups and five
    rows) leaves the live rows those of the unbounded run."""
    x, w, b, r = data(803, True, 7)
    x, r, wp = dev(x), dev(r), pack(w)
    full = xn(x, wp, b, r, k)
    for live in (0, 1, 9, 517):
        lv = torch.tensor([live], dtype=torch.int32, device="cuda")
        assert torch.equal(xn(x, wp, b, r, k, lv)[:live], full[:live]), live


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("batch", [1, 7, 15, 29, 300])
def test_nothing_read_past_the_inputs(batch, k):
    """The input is the prefix of a buffer whose tail is NaN
    (test_kernels_read_nothing_past_their_inputs): finite outputs."""
    g = torch.Generator(device="cuda").manual_seed(batch)
    x = torch.full((batch + 2, 128, 5, 7), float("nan"), device="cuda").contiguous(memory_format=CL)
    x[:batch] = torch.randn(batch, 128, 5, 7, device="cuda", generator=g)
    w = pack_conv3x3_x6(torch.randn(128, 128, 3, 3, device="cuda", generator=g) * 0.03)
    b = torch.randn(128, device="cuda", generator=g) * 0.1
    assert bool(torch.isfinite(_conv3x3_xn_act(x[:batch], w, b, x[:batch], None, k)).all())
    allw = torch.stack([w, w]).contiguous()
    allb = torch.stack([b, b]).contiguous()
    assert bool(torch.isfinite(_tower_resident(x[:batch], allw, allb, None, k)).all())


def test_products_argument_is_checked():
    x, allw, allb = _tower4(2, 9)
    out = torch.full_like(x, 7.0)
    s = torch.cuda.current_stream().cuda_stream
    L = lib()
    for p in (0, 2, 7):
        assert L.hz_conv3x3_xn_bias_act(x.data_ptr(), allw[0].data_ptr(), allb[0].data_ptr(), None, out.data_ptr(),
                                        2, None, p, s) == -1
        assert L.hz_tower_xn_resident(x.data_ptr(), allw.data_ptr(), allb.data_ptr(), out.data_ptr(), 4, 2, None,
                                      p, s) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was enqueued
    # 6 is the x6 entry point itself
    assert L.hz_conv3x3_xn_bias_act(x.data_ptr(), allw[0].data_ptr(), allb[0].data_ptr(), None, out.data_ptr(), 2,
                                    None, 6, s) == 0
    assert torch.equal(out, _conv3x3_x6_act(x, allw[0], allb[0]))
    assert torch.equal(_tower_resident(x, allw, allb, None, 6), _tower_resident(x, allw, allb))


@pytest.fixture(scope="module")
def whole_net():
    """The default 128x8 net with random BatchNorm statistics, 803
    encoder-like boards, the unfolded float64 network's outputs and the
    float64 emulation of the x1 network (CPU, computed once)."""
    g = torch.Generator().manual_seed(11)
    torch.manual_seed(1)
    net = HarmoniesNet().eval()
    _randomise_bn(net, g)
    n = 803
    board = (torch.rand(n, 38, 5, 7, generator=g) > 0.8).float()
    glob = torch.rand(n, 42, generator=g)
    with torch.no_grad():
        l64, v64 = net.double()(board.double(), glob.double())
        net.float()
    cpu = FoldedNet(net, torch_epilogue, tower="x6")
    le, ve = emulate_folded(cpu, board, glob, 1)
    emu1 = ((le - l64).abs().max().item(), (ve - v64).abs().max().item())
    return net.cuda(), board.cuda(), glob.cuda(), l64, v64, emu1


@pytest.mark.parametrize("rows", [64, 803])
@pytest.mark.parametrize("mode", ["x3", "x1"])
def test_whole_net(whole_net, mode, rows):
    """FoldedNet(tower=mode), through the resident tower (both batches are
    within resident_max) and through the layered convs (resident_max = 0),
    is the layer primitives chained by hand (bit for bit); x3 within
    the project's 1e-4 of the unfolded float64 network; x1 within twice its
    float64 emulation's deviation (803 rows) + 1e-4 (a bf16 rounding flip of
    an activation, caused by an fp32-level difference, is one bf16 ulp: the
    size of the rounding the mode makes anyway)."""
    net, board, glob, l64, v64, emu1 = whole_net
    board, glob, l64, v64 = board[:rows], glob[:rows], l64[:rows], v64[:rows]
    fnet = FoldedNet(net, tower=mode)
    k = fnet.products
    assert k == {"x3": 3, "x1": 1}[mode] and fnet.resident is not None
    assert fnet.split_max < rows <= fnet.resident_max  # the resident tower's batches
    lo, v = fnet(board, glob)
    layered = FoldedNet(net, tower=mode)
    layered.resident_max = 0  # the same rows through two hz_conv3x3_xn_bias_act per block
    l3, v3 = layered(board, glob)
    assert torch.equal(l3, lo) and torch.equal(v3, v)
    x = _stem_x6_act(board, fnet.stem_packed, fnet.stem[1])
    x = _chain(x, *fnet.resident, k)
    lh, _, vh = _heads_fc(x, glob, *fnet.heads, fnet.fc, logits=True, probs=False)
    assert torch.equal(lo, lh) and torch.equal(v, vh.unsqueeze(1))
    assert not torch.equal(lo, FoldedNet(net, tower="x6")(board, glob)[0])
    dl = (lo.cpu().double() - l64).abs().max().item()
    dv = (v.cpu().double() - v64).abs().max().item()
    print(f"{mode} rows={rows}: logits {dl:.3e} value {dv:.3e} (x1 emulation {emu1[0]:.3e} {emu1[1]:.3e})")
    if mode == "x3":
        assert dl <= 1e-4 and dv <= 1e-4, (dl, dv)
    else:
        assert dl <= 2 * emu1[0] + 1e-4 and dv <= 2 * emu1[1] + 1e-4, (dl, dv, emu1)
    live = torch.tensor([rows - 3], dtype=torch.int32, device="cuda")
    l2, v2 = fnet(board, glob, live=live)
    assert torch.equal(l2[:rows - 3], lo[:rows - 3]) and torch.equal(v2[:rows - 3], v[:rows - 3])


def test_predictor_and_mode_switch(whole_net):
    net, board, glob = whole_net[:3]
    board, glob = board[:64], glob[:64]
    pred = BatchedPredictor(net, tower="x3")
    assert pred.fast.tower == "x3" and pred.capturable and pred.row_independent
    p, v = pred(board, glob)
    fnet = FoldedNet(net, tower="x3")
    p0, v0 = fnet.predict(board, glob)
    assert torch.equal(p, p0) and torch.equal(v, v0)
    # a switch re-packs nothing and bumps the generation
    gen, packed = fnet.generation, fnet.resident[0]
    fnet.set_tower("x1")
    assert fnet.generation == gen + 1 and fnet.resident[0] is packed
    assert torch.equal(fnet.predict(board, glob)[0], FoldedNet(net, tower="x1").predict(board, glob)[0])
    fnet.set_tower("x6")
    assert torch.equal(fnet.predict(board, glob)[0], FoldedNet(net, tower="x6").predict(board, glob)[0])


def test_search_graph_replay_equals_eager():
    """48 boards, 8 simulations with the x3 predictor: the captured
    simulation replays to the eager search's visit counts."""
    from hzamd.env import BatchedEnv
    from hzamd.mcts import BatchedMCTS
    torch.manual_seed(0)
    pred = BatchedPredictor(HarmoniesNet().eval().cuda(), tower="x3")
    n = 48
    out = []
    for graph in (False, True):
        env = BatchedEnv(n, seed_base=77, device="cuda:0")
        env.reset()
        mcts = BatchedMCTS(env, 8)
        out.append(mcts.search(pred, 2.0, graph=graph).clone().cpu())
        mcts.close()
        env.close()
    assert int(out[0].sum()) > 0
    assert torch.equal(out[0], out[1])
