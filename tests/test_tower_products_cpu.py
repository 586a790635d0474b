"""The reduced tower modes' arithmetic definition (hzamd.infer.emulate_conv3x3,
emulate_folded: float64 on the CPU) against its error bounds, and the mode
plumbing (FoldedNet(tower=...), HZ_TOWER, ModelManager.set_inference_tower).

Bounds: bf16 round-to-nearest gives |a - a_h| <= 2^-9 |a| and
|a_l| = |a - a_h - a_m| <= 2^-18 |a|, so |a_m| <= 2^-9 (1 + 2^-9) |a|.
The three products leave
  a b - (hh + hm + mh) = a_l b + (a_h + a_m) b_l + a_m b_m,
at most (2^-18 + (1 + 2^-18) 2^-18 + 2^-18 (1 + 2^-9)^2) |a b|
<= 3 * 2^-18 * 1.01 |a b|; the one product leaves
  a b - hh = (a - a_h) b + a_h (b - b_h),
at most (2^-9 + (1 + 2^-9) 2^-9) |a b| = (2^-8 + 2^-18) |a b|
<= (2^-8 + 2^-16) |a b|.  Summed over a conv's terms that is the factor
times S = conv2d(|x|, |w|).  All six products drop only m l, l m, l l:
<= (2 * 2^-27 + 2^-36) (1 + 2^-8) < 2^-26."""
import pytest
import torch
import torch.nn.functional as F

from hzamd.infer import FoldedNet, emulate_conv3x3, emulate_folded
from hzamd.net import HarmoniesNet
from test_infer_cpu import _randomise_bn, torch_epilogue


@pytest.fixture(scope="module")
def conv_data():
    g = torch.Generator().manual_seed(21)
    x = torch.randn(64, 128, 5, 7, generator=g).relu()
    w = torch.randn(128, 128, 3, 3, generator=g) * 0.03
    want = F.conv2d(x.double(), w.double(), None, padding=1)
    S = F.conv2d(x.double().abs(), w.double().abs(), None, padding=1)
    return x, w, want, S


def test_emulated_six_products_are_the_fp64_conv(conv_data):
    x, w, want, S = conv_data
    err = (emulate_conv3x3(x, w, 6) - want).abs()
    assert bool((err <= 2.0 ** -26 * S).all()), (err / S).max().item()


@pytest.mark.parametrize("products,bound", [(3, 3 * 2.0 ** -18 * 1.01), (1, 2.0 ** -8 + 2.0 ** -16)])
def test_emulated_reduced_products_within_worst_case(conv_data, products, bound):
    x, w, want, S = conv_data
    got = emulate_conv3x3(x, w, products)
    assert got.dtype == torch.float64
    err = (got - want).abs()
    print(f"products={products}: max err / S = 2^{torch.log2((err / S).max()).item():.2f}")
    assert bool((err <= bound * S).all()), (err / S).max().item()
    # and the mode is not a more accurate one in disguise
    assert (err / S).max().item() > (2.0 ** -26 if products == 3 else 2.0 ** -17)


@pytest.fixture(scope="module")
def net_data():
    g = torch.Generator().manual_seed(11)
    torch.manual_seed(1)
    net = HarmoniesNet().eval()
    _randomise_bn(net, g)
    n = 64
    board = (torch.rand(n, 38, 5, 7, generator=g) > 0.8).float()
    glob = torch.rand(n, 42, generator=g)
    fnet = FoldedNet(net, torch_epilogue, tower="x6")
    with torch.no_grad():
        l64, v64 = net.double()(board.double(), glob.double())
        net.float()
    return fnet, board, glob, l64, v64


def test_emulate_folded_six_products_is_the_fp64_network(net_data):
    fnet, board, glob, l64, v64 = net_data
    lo, v = emulate_folded(fnet, board, glob, 6)
    assert lo.dtype == torch.float64 and lo.shape == l64.shape and v.shape == v64.shape
    dl, dv = (lo - l64).abs().max().item(), (v - v64).abs().max().item()
    print(f"products=6: logits {dl:.2e} value {dv:.2e}")
    assert dl <= 1e-7 and dv <= 1e-7, (dl, dv)


def test_emulate_folded_three_products_within_project_bound(net_data):
    fnet, board, glob, l64, v64 = net_data
    lo, v = emulate_folded(fnet, board, glob, 3)
    dl, dv = (lo - l64).abs().max().item(), (v - v64).abs().max().item()
    print(f"products=3: logits {dl:.2e} value {dv:.2e}")
    assert dl <= 1e-4 and dv <= 1e-4, (dl, dv)
    assert dl > 1e-7  # not the six-product network


def test_unknown_tower_raises():
    net = HarmoniesNet().eval()
    with pytest.raises(ValueError, match="x3"):
        FoldedNet(net, torch_epilogue, tower="bogus")
    assert FoldedNet.TOWER_MFMA == ("x6", "x3", "x1", "f32")


def test_hz_tower_selects_the_default_mode(monkeypatch):
    net = HarmoniesNet().eval()
    monkeypatch.delenv("HZ_TOWER", raising=False)
    assert FoldedNet(net, torch_epilogue).tower == "x6"
    monkeypatch.setenv("HZ_TOWER", "x3")
    f = FoldedNet(net, torch_epilogue)
    assert f.tower == "x3" and f.products == 3
    assert FoldedNet(net, torch_epilogue, tower="x1").tower == "x1"  # an argument wins
    monkeypatch.setenv("HZ_TOWER", "bogus")
    with pytest.raises(ValueError):
        FoldedNet(net, torch_epilogue)


def test_set_tower_among_x_modes_refolds_nothing():
    net = HarmoniesNet().eval()
    f = FoldedNet(net, torch_epilogue, tower="x6")
    w0, gen = f.stem[0], f.generation
    f.set_tower("x3")
    assert f.tower == "x3" and f.stem[0] is w0 and f.generation == gen + 1
    f.set_tower("x3")
    assert f.generation == gen + 1
    with pytest.raises(ValueError):
        f.set_tower("x2")


def test_manager_set_inference_tower_on_cpu():
    from hzamd.manager import ModelManager
    from test_manager_cpu import MODEL_CFG, TRAIN_CFG
    mm = ModelManager(MODEL_CFG, TRAIN_CFG)
    assert mm.inference_tower is None
    before = {k: v.clone() for k, v in mm.model.state_dict().items()}
    versions = [p._version for p in mm.model.parameters()]
    mm.set_inference_tower("x3")
    assert mm.inference_tower == "x3"
    assert versions == [p._version for p in mm.model.parameters()]
    assert all(torch.equal(v, before[k]) for k, v in mm.model.state_dict().items())
    with pytest.raises(ValueError):
        mm.set_inference_tower("bogus")
    assert mm.inference_tower == "x3"
    assert ModelManager(MODEL_CFG, dict(TRAIN_CFG, inference_tower="x1")).inference_tower == "x1"
