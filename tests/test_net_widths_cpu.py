"""The width-generic conv's weight packs and FoldedNet's dispatch for other
filter counts, as far as they go without a GPU (tests/test_net_widths_gpu.py
runs the kernels)."""
import pytest
import torch

from hzamd._native import exported_symbols
from hzamd.infer import WIDE_FILTERS, FoldedNet, pack_conv3x3_x6, pack_stem_x6g, split3_bf16
from hzamd.net import TINY, HarmoniesNet
from test_infer_cpu import torch_epilogue


def _unpack(p):
    """[tap][ci/32][plane][co][32] bf16 -> (sum of the planes in float64
    [co][ci][3][3], the planes [3][co][ci][3][3])."""
    taps, nq, planes, co, k = p.shape
    assert (taps, planes, k) == (9, 3, 32) and p.dtype == torch.bfloat16
    pl = p.permute(2, 3, 1, 4, 0).reshape(3, co, nq * 32, 3, 3)
    return pl.double().sum(0), pl


@pytest.mark.parametrize("co,ci", [(32, 32), (256, 64)])
def test_generalised_pack_reconstructs_the_weight(co, ci):
    """pack_conv3x3_x6 at other widths: element [tap][q][plane][co][k] is
    plane `plane` of w[co][32 q + k][tap], so h + m + l summed over the
    planes gives the weight back exactly."""
    g = torch.Generator().manual_seed(co + ci)
    w = torch.randn(co, ci, 3, 3, generator=g) * torch.logspace(-6, 2, ci, base=2.0).view(1, -1, 1, 1)
    p = pack_conv3x3_x6(w)
    assert p.shape == (9, ci // 32, 3, co, 32) and p.is_contiguous()
    total, planes = _unpack(p)
    assert torch.equal(total, w.double())
    assert torch.equal(planes, split3_bf16(w))
    assert bool(planes[1].any()) and bool(planes[2].any())


def test_stem_pack_pads_the_channels_to_64():
    """pack_stem_x6g (64 filters): channels 0-37 reconstruct the weight
    exactly, channels 38-63 are zeros in every plane."""
    g = torch.Generator().manual_seed(5)
    w = torch.randn(64, 38, 3, 3, generator=g)
    p = pack_stem_x6g(w)
    assert p.shape == (9, 2, 3, 64, 32)
    total, planes = _unpack(p)
    assert torch.equal(total[:, :38], w.double())
    assert not planes[:, :, 38:].any()


def test_pack_at_128_is_the_present_layout_byte_for_byte():
    """At (128, 128) the pack equals the layout k_conv3x3_x6 has always read,
    restated index by index: B fragment of (tap, chunk q, plane p, channel
    co) holds w_p[co][32 q .. 32 q + 31][tap]."""
    g = torch.Generator().manual_seed(7)
    w = torch.randn(128, 128, 3, 3, generator=g)
    pl = split3_bf16(w)  # [3][co][ci][3][3]
    want = torch.empty(9, 4, 3, 128, 32, dtype=torch.bfloat16)
    for tap in range(9):
        for q in range(4):
            want[tap, q] = pl[:, :, 32 * q:32 * q + 32, tap // 3, tap % 3]
    got = pack_conv3x3_x6(w)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert got.view(torch.int16).numpy().tobytes() == want.view(torch.int16).numpy().tobytes()


def test_torch_path_claims_no_row_independence_at_other_widths():
    """FoldedNet(..., torch_epilogue) packs nothing for the HIP path and
    claims no row independence, at 32, 64 and 256 filters as at 128."""
    for cfg in (TINY, dict(cnn_filters=64, num_res_blocks=1), dict(cnn_filters=256, num_res_blocks=1), None):
        f = FoldedNet(HarmoniesNet(cfg).eval(), torch_epilogue)
        assert f.wide is None and not f.row_independent


def test_dispatch_by_width_and_mode():
    """Which networks take the width-generic kernels: F in {32, .., 256}
    except 128, bf16 tower modes, head filters 1..4; not 48 filters, not
    tower="f32", not native_conv=False, and never a 128-filter network."""
    assert WIDE_FILTERS == (32, 64, 96, 128, 160, 192, 224, 256)
    tiny = HarmoniesNet(TINY).eval()
    for tower in ("x6", "x3", "x1"):
        f = FoldedNet(tiny, tower=tower)
        assert f.wide is not None and f.row_independent and f.wide["dims"] == (2, 1, 64)
        assert f.wide["stem"].shape == (9, 2, 3, 32, 32) and f.wide["blocks"][0][0].shape == (9, 1, 3, 32, 32)
    f = FoldedNet(tiny)
    gen = f.generation
    f.set_tower("x3")
    assert f.wide is not None and f.generation == gen + 1
    f.set_tower("f32")
    assert f.wide is None and not f.row_independent
    assert FoldedNet(tiny, native_conv=False).wide is None
    assert FoldedNet(HarmoniesNet(dict(cnn_filters=48, num_res_blocks=1)).eval()).wide is None
    assert FoldedNet(HarmoniesNet(dict(num_res_blocks=1)).eval()).wide is None
    assert FoldedNet(HarmoniesNet(dict(num_res_blocks=1, policy_head_conv_filters=3)).eval()).wide is None
    assert FoldedNet(HarmoniesNet(dict(cnn_filters=64, num_res_blocks=0, value_head_conv_filters=5)).eval()).wide is None
    wide = FoldedNet(HarmoniesNet(dict(cnn_filters=256, num_res_blocks=2, value_head_hidden_dim=512,
                                       policy_head_conv_filters=4, value_head_conv_filters=3)).eval()).wide
    assert wide["dims"] == (4, 3, 512) and wide["hw"].shape == (7, 256) and wide["fc"][0].shape == (182, 143)


def test_new_entry_points_are_bound():
    assert {"hz_conv3x3_x6g_bias_act", "hz_stem3x3_x6g_bias_act", "hz_heads_fc_g"} <= set(exported_symbols())
