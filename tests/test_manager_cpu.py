"""hzamd.manager.ModelManager against the reference ModelManager
(model.py): train_step losses and updated weights from the same initial
weights and batch (tests/golden/train.npz, captured from the reference on
CPU; fp32, atol 1e-6), the reference-written checkpoint loaded with the
safe loader (tests/golden/ref_ckpt_tiny.pth.tar), the forced LR reset on
load (model.py:198-236), and our own save -> load round trip."""
import functools
import os

import numpy as np
import torch

from conftest import GOLDEN
from hzamd.manager import ModelManager

MODEL_CFG = {"input_channels": 38, "cnn_filters": 32, "board_size": (5, 7), "action_size": 143,
             "global_feature_size": 42, "value_head_hidden_dim": 64, "num_res_blocks": 1,
             "policy_head_conv_filters": 2, "value_head_conv_filters": 1}           # config.py test_model_config
TRAIN_CFG = {"device": "cpu", "optimizer_type": "Adam", "learning_rate": 0.001, "weight_decay": 0.0,
             "value_loss_weight": 1.0, "policy_loss_weight": 1.0, "batch_size": 4, "momentum": 0.9,
             "use_scheduler": True, "scheduler_type": "StepLR", "scheduler_step_size": 30,
             "scheduler_gamma": 0.5, "force_lr_reset_on_load": False, "new_forced_lr": 0.000125}


def fixture():
    return np.load(os.path.join(GOLDEN, "train.npz"))


def state(f, prefix):
    return {k[len(prefix):]: torch.from_numpy(f[k]) for k in f.files if k.startswith(prefix)}


TAU = 1e-7            # gradients below it may round to either sign in fp32 (measured fp32-vs-float64: 1.5e-7)
AMBIGUOUS_CAP = 0.01  # largest share of elements the loose bound may cover


@functools.lru_cache(maxsize=None)
def float64_reference():
    """The fixture's three train steps recomputed in float64 (the same
    ModelManager from init/, model.double(), a fresh Adam at the same lr) and
    every floating element of the state dict put into one of three classes by
    the float64 gradients g_1..g_3 of its parameter element:
      dead       g_t == 0 exactly at all three steps (Adam leaves it alone),
      kept       at every step |g_t| >= TAU (its sign is the same in any fp32
                 run) or g_t == 0 exactly (a unit that a ReLU switched off for
                 the whole batch at that step: zero in fp32 too), not dead,
      ambiguous  the rest (an fp32 run may take either sign: ~lr per step).
    (Requiring |g_t| >= TAU at all three steps of a kept element would leave
    1.52 % ambiguous here, over the cap: 687 elements have an exact zero at
    one or two steps.  They are held to the tight bound instead.)
    Buffers (BatchNorm running statistics) count as kept, but for a
    running_mean channel whose convolution's bias element is ambiguous: the
    batch mean contains that bias, so the channel inherits its class (the
    reference's own fp32 run is 1.9e-4 from float64 there, 2.8e-7 elsewhere).
    Returns (final float64 state dict, {key: bool mask} of the dead or kept
    elements, the number of dead ones)."""
    f = fixture()
    mm = ModelManager(MODEL_CFG, TRAIN_CFG)
    mm.model.load_state_dict(state(f, "init/"))
    mm.model.double()
    mm.optimizer = torch.optim.Adam(mm.model.parameters(), lr=TRAIN_CFG["learning_rate"])
    batch = [torch.from_numpy(f[k]).double() for k in ("board", "glob", "pi", "z")]
    clear, gmax = {}, {}
    for _ in range(3):
        mm.train_step_async(*batch)
        for k, p in mm.model.named_parameters():
            g = p.grad.detach().abs()
            ok = (g == 0) | (g >= TAU)
            clear[k] = ok if k not in clear else clear[k] & ok
            gmax[k] = g.clone() if k not in gmax else torch.maximum(gmax[k], g)
    final = {k: v.detach().clone() for k, v in mm.model.state_dict().items()}
    sure = {k: clear[k] if k in clear else torch.ones_like(v, dtype=torch.bool)
            for k, v in final.items() if v.is_floating_point()}
    for k in sure:
        if k.endswith(".running_mean") or k == "running_mean":
            mod, _, _ = k.rpartition(".")
            head, _, leaf = mod.rpartition(".")
            bias = (head + "." if head else "") + leaf.replace("bn", "conv") + ".bias"
            sure[k] = sure[bias].clone()  # (every BatchNorm here follows a convolution with a bias: KeyError otherwise)
    dead = sum(int((gmax[k] == 0).sum()) for k in gmax)
    return final, sure, dead


def float64_distances(weights):
    """|weights - float64 reference| of a state dict's floating elements:
    (the dead or kept elements', the ambiguous elements'), each 1-D float64."""
    final, sure, _ = float64_reference()
    d = {k: (weights[k].detach().cpu().double() - final[k]).abs() for k in sure}
    return (torch.cat([d[k][sure[k]] for k in sure]), torch.cat([d[k][~sure[k]] for k in sure]))


def train_step_bounds():
    """(reference deviation, n dead, n dead or kept, n ambiguous): the largest
    distance of the reference's own fp32 run (final/) from the float64 weights
    over the dead or kept elements, and the class sizes."""
    d_sure, d_amb = float64_distances(state(fixture(), "final/"))
    return float(d_sure.max()), float64_reference()[2], d_sure.numel(), d_amb.numel()


def test_train_step_classes_and_fixture_against_float64():
    """The conditions of the GPU train-step bound (test_trainer_gpu.py),
    checked without a GPU: at most 1 % of the elements are ambiguous, some
    are dead, the reference's fp32 deviation from float64 is so small that 8
    times it stays more than 100 times below one wrong-sign Adam step (2 lr),
    the fixture meets the bound with factor 1 (by construction) and 6 lr on
    its ambiguous elements, and this CPU's fp32 run of the three steps, one
    more fp32 run with its own summation order (it depends on the CPU and the
    thread count), meets the GPU test's bound: 8 times the reference
    deviation plus 1e-7, and 6 lr (three steps of opposite sign) on the
    ambiguous elements.  Measured: dead
    1,007, kept 49,968, ambiguous 208 (0.41 %: 109 parameter elements, 99
    running means) of 51,183; reference deviation 2.75e-7; this CPU's fp32
    run 2.75e-7 and, on the ambiguous elements, 1.59 lr."""
    lr = TRAIN_CFG["learning_rate"]
    ref_dev, n_dead, n_sure, n_amb = train_step_bounds()
    n = n_sure + n_amb
    print(f"dead {n_dead} kept {n_sure - n_dead} ambiguous {n_amb} of {n}; reference deviation {ref_dev:.3g}")
    assert n_amb <= AMBIGUOUS_CAP * n and 0 < n_dead < n_sure
    assert 0 < ref_dev and 8 * ref_dev + 1e-7 <= 2 * lr / 100
    f = fixture()
    fix_sure, fix_amb = float64_distances(state(f, "final/"))
    assert float(fix_sure.max()) <= ref_dev + 1e-7 and float(fix_amb.max()) <= 6 * lr * 1.01
    mm = ModelManager(MODEL_CFG, TRAIN_CFG)
    mm.model.load_state_dict(state(f, "init/"))
    batch = [torch.from_numpy(f[k]) for k in ("board", "glob", "pi", "z")]
    for _ in range(3):
        mm.train_step(*batch)
    d_sure, d_amb = float64_distances(mm.model.state_dict())
    print(f"fp32 on this CPU: dead or kept max {float(d_sure.max()):.3g}, ambiguous max {float(d_amb.max()):.3g}")
    assert float(d_sure.max()) <= 8 * ref_dev + 1e-7
    assert float(d_amb.max()) <= 6 * lr * 1.01


def test_train_step_matches_reference():
    f = fixture()
    mm = ModelManager(MODEL_CFG, TRAIN_CFG)
    mm.model.load_state_dict(state(f, "init/"))
    b, g, pi, z = (torch.from_numpy(f[k]) for k in ("board", "glob", "pi", "z"))
    losses = np.array([mm.train_step(b, g, pi, z) for _ in range(3)])
    assert np.abs(losses - f["losses"]).max() <= 1e-6
    # atol 1e-6 on every element whose float64 gradient is clear of zero at each
    # step (float64_reference: all but 0.41 %); an ambiguous one (a conv bias
    # feeding a BatchNorm, that BatchNorm's running mean, ...) takes either
    # sign per step depending on this CPU's summation order and thread count:
    # within 6 lr, three steps of opposite sign
    _, sure, _ = float64_reference()
    lr = TRAIN_CFG["learning_rate"]
    for k, v in state(f, "final/").items():
        d = (mm.model.state_dict()[k] - v).abs()
        if k not in sure:
            assert torch.equal(mm.model.state_dict()[k], v), k
            continue
        assert d[sure[k]].numel() == 0 or d[sure[k]].max().item() <= 1e-6, k
        assert d[~sure[k]].numel() == 0 or d[~sure[k]].max().item() <= 6 * lr * 1.01, k


def test_load_reference_checkpoint():
    f = fixture()
    mm = ModelManager(MODEL_CFG, TRAIN_CFG)
    ok, it = mm.load_checkpoint(folder=GOLDEN, filename="ref_ckpt_tiny.pth.tar")
    assert ok and it == 7
    for k, v in state(f, "final/").items():
        assert torch.equal(mm.model.state_dict()[k], v), k
    assert mm.get_current_lr() == 0.001
    assert len(mm.optimizer.state) == len(list(mm.model.parameters()))


def test_forced_lr_reset_on_load():
    mm = ModelManager(MODEL_CFG, dict(TRAIN_CFG, force_lr_reset_on_load=True))
    ok, it = mm.load_checkpoint(folder=GOLDEN, filename="ref_ckpt_tiny.pth.tar")
    assert ok and it == 7
    assert mm.optimizer.param_groups[0]["lr"] == 0.000125
    # StepLR(last_epoch=7 - 7 % 30 = 0) steps once in its constructor, as in the reference
    assert mm.scheduler.last_epoch == 1 and mm.get_current_lr() == 0.000125


def test_capturable_checkpoint_trains_on_cpu(tmp_path):
    """A checkpoint whose Adam groups say capturable=True (a GPU manager's
    optimizer state) loads into a CPU manager that can still train: the
    flag is set for the loading device and the step counters move to the
    host; our own files are written with capturable=False."""
    torch.manual_seed(4)
    a = ModelManager(MODEL_CFG, TRAIN_CFG)
    b, g = torch.rand(4, 38, 5, 7), torch.rand(4, 42)
    pi = torch.softmax(torch.rand(4, 143), 1)
    a.train_step(b, g, pi, torch.zeros(4, 1))
    a.save_checkpoint(folder=tmp_path, filename="a.pth.tar", iteration=1)
    ck = torch.load(tmp_path / "a.pth.tar", weights_only=True)
    assert all(not gr.get("capturable", False) for gr in ck["optimizer_state_dict"]["param_groups"])
    for gr in ck["optimizer_state_dict"]["param_groups"]:
        gr["capturable"] = True                      # as a GPU-written file of round 2 had it
    torch.save(ck, tmp_path / "gpu.pth.tar")
    c = ModelManager(MODEL_CFG, TRAIN_CFG)
    assert c.load_checkpoint(folder=tmp_path, filename="gpu.pth.tar") == (True, 1)
    assert all(gr["capturable"] is False for gr in c.optimizer.param_groups)
    loss = c.train_step(b, g, pi, torch.zeros(4, 1))
    a.train_step(b, g, pi, torch.zeros(4, 1))
    for k, v in a.model.state_dict().items():
        assert torch.equal(c.model.state_dict()[k], v), k
    assert np.isfinite(loss).all()


def test_checkpoint_round_trip(tmp_path):
    torch.manual_seed(3)
    a = ModelManager(MODEL_CFG, TRAIN_CFG)
    b, g = torch.rand(4, 38, 5, 7), torch.rand(4, 42)
    pi = torch.softmax(torch.rand(4, 143), 1)
    a.train_step(b, g, pi, torch.zeros(4, 1))
    a.step_scheduler()
    a.save_checkpoint(folder=tmp_path, filename="x.pth.tar", iteration=3)
    ck = torch.load(tmp_path / "x.pth.tar", weights_only=True)
    assert set(ck) == {"model_config", "training_config", "model_state_dict", "optimizer_state_dict",
                       "scheduler_state_dict", "iteration"}
    c = ModelManager(MODEL_CFG, TRAIN_CFG)
    assert c.load_checkpoint(folder=tmp_path, filename="x.pth.tar") == (True, 3)
    for k, v in a.model.state_dict().items():
        assert torch.equal(c.model.state_dict()[k], v)
    assert c.scheduler.last_epoch == 1
    assert c.load_checkpoint(folder=tmp_path, filename="missing.pth.tar") == (False, 0)
    p0, v0 = a.predict(b[0], g[0])
    p1, v1 = c.predict(b[0], g[0])
    assert p0.shape == (143,) and np.array_equal(p0, p1) and v0 == v1


def test_head_filters_in_config_are_ignored_like_the_reference():
    """The reference's ModelManager never passes the head conv filter counts
    to AlphaZeroModel (model.py:20-29), so its heads are always 2 / 1 filters
    (model.py:287-288): a config naming other counts builds the same network
    and state dict."""
    mm = ModelManager(dict(MODEL_CFG, policy_head_conv_filters=4, value_head_conv_filters=3), TRAIN_CFG)
    ref = ModelManager(MODEL_CFG, TRAIN_CFG)
    a, b = mm.model.state_dict(), ref.model.state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a)
    assert a["policy_conv.weight"].shape[0] == 2 and a["value_conv.weight"].shape[0] == 1
