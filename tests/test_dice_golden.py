"""mmseg's DiceLoss and loss lists on the CPU: heads.dice_loss against tests/golden/g22_dice.npz (written by
tests/golden/make_dice_fixture.py from the reference's own dice_loss.py, loss and autograd gradient, float64); heads._loss_specs
parses a dict, a list and None and raises on what is not built; all four heads take a [CrossEntropyLoss, DiceLoss] list; a tiny SegNet
emits every loss name, sums equal names and keeps the single cross-entropy configuration bit for bit; one training step runs with the
list."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_dice.npz")
CE_DICE = [dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0), dict(type="DiceLoss", loss_weight=3.0)]


def _cases():
    z = np.load(GOLDEN)
    names = ["".join(chr(int(c)) for c in row).strip() for row in z["cases"]]
    return z, names


def test_fixture_holds_the_cases_of_the_issue():
    z, names = _cases()
    assert {f"{k}_c{C}" for k in ("plain", "cw", "smooth") for C in (2, 3, 5)} <= set(names)
    assert {"lw3_c3", "allign_c2", "allign_c5", "ign1_c3", "exp1_c3"} <= set(names)
    assert all(z[k].dtype == np.float64 for k in z.files)                                  # numbers only
    for n in names:
        C = int(n.rsplit("_c", 1)[1])
        assert z[f"{n}/logit"].shape == z[f"{n}/grad"].shape == (2, C, 12, 20) and z[f"{n}/label"].shape == (2, 12, 20)
    assert float(z["smooth_c3/args"][0]) == 0.5 and float(z["lw3_c3/args"][2]) == 3.0
    assert float(z["ign1_c3/args"][3]) == 1.0 and float(z["exp1_c3/args"][1]) == 1.0
    assert bool((z["allign_c2/label"] == 255).all())


def test_dice_loss_matches_the_reference_loss_and_gradient():
    from ppnet_amd import heads
    z, names = _cases()
    for n in names:
        x = torch.tensor(z[f"{n}/logit"], requires_grad=True)
        lab = torch.tensor(z[f"{n}/label"]).long()
        smooth, exponent, lw, ignore = (float(v) for v in z[f"{n}/args"])
        cw = tuple(z[f"{n}/class_weight"]) or None
        loss = heads.dice_loss(x, lab, smooth, int(exponent), cw, lw, int(ignore))
        grad, = torch.autograd.grad(loss, x)
        want, wgrad = float(z[f"{n}/loss"]), torch.tensor(z[f"{n}/grad"])
        assert abs(float(loss.detach()) - want) <= 1e-12 * abs(want), (n, float(loss.detach()), want)
        assert float((grad - wgrad).abs().max()) <= 1e-12 * float(wgrad.abs().max()), n
    # uint8 labels and float32 logits go through the same function
    x32 = torch.tensor(z["cw_c3/logit"]).float()
    l32 = heads.dice_loss(x32, torch.tensor(z["cw_c3/label"]).to(torch.uint8), class_weight=tuple(z["cw_c3/class_weight"]))
    assert l32.dtype == torch.float32 and float(l32) == pytest.approx(float(z["cw_c3/loss"]), rel=1e-5)


def test_loss_specs_parse_dict_list_and_none():
    from ppnet_amd.heads import _loss_specs, _single_ce
    ce = dict(type="CrossEntropyLoss", loss_name="loss_ce", loss_weight=1.0, class_weight=None)
    assert _loss_specs(None, 3) == (ce,) and _single_ce(None)
    assert _loss_specs(dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.4, class_weight=[1, 2, 3]), 3) == (
        dict(ce, loss_weight=0.4, class_weight=(1.0, 2.0, 3.0)),)
    assert _loss_specs(dict(loss_weight=0.4), 3) == (dict(ce, loss_weight=0.4),) and _single_ce(dict(loss_weight=0.4))
    dice = dict(type="DiceLoss", loss_name="loss_dice", loss_weight=1.0, class_weight=None, smooth=1.0, exponent=2, ignore_index=255)
    assert _loss_specs(dict(type="DiceLoss"), 3) == (dice,) and not _single_ce(dict(type="DiceLoss"))
    specs = _loss_specs([dict(type="CrossEntropyLoss", loss_name="loss_a", class_weight=[1, 2]),
                         dict(type="DiceLoss", loss_weight=3, smooth=0.5, exponent=1, ignore_index=1, class_weight=(0.5, 2), loss_name="loss_a")], 2)
    assert specs == (dict(ce, loss_name="loss_a", class_weight=(1.0, 2.0)),
                     dict(dice, loss_name="loss_a", loss_weight=3.0, smooth=0.5, exponent=1, ignore_index=1, class_weight=(0.5, 2.0)))
    assert _loss_specs(tuple(CE_DICE), 2) == _loss_specs(CE_DICE, 2) and not _single_ce(CE_DICE)


@pytest.mark.parametrize("bad", [
    dict(type="LovaszLoss"), dict(type="FocalLoss"), [dict(type="CrossEntropyLoss"), dict(type="LovaszLoss")],
    dict(type="DiceLoss", class_weight="weights.npy"), [dict(type="CrossEntropyLoss", class_weight="weights.npy")],
    dict(type="DiceLoss", reduction="sum"), [dict(type="CrossEntropyLoss", reduction="none"), dict(type="DiceLoss")],
    dict(type="DiceLoss", use_sigmoid=True), [dict(type="CrossEntropyLoss", use_sigmoid=True)],
    [dict(type="CrossEntropyLoss"), dict(type="CrossEntropyLoss", use_sigmoid=True)]], ids=str)
def test_loss_specs_reject_what_is_not_built(bad):
    from ppnet_amd.heads import FCNHead, _loss_specs
    with pytest.raises(NotImplementedError):
        _loss_specs(bad, 2)
    with pytest.raises(NotImplementedError):
        FCNHead(8, 8, 2, 1, loss_decode=bad)


def test_loss_specs_reject_malformed_entries():
    from ppnet_amd.heads import _loss_specs
    with pytest.raises(ValueError):
        _loss_specs(dict(type="DiceLoss", class_weight=[1, 2, 3]), 2)
    with pytest.raises(TypeError):
        _loss_specs([], 2)
    with pytest.raises(TypeError):
        _loss_specs("DiceLoss", 2)


def test_all_four_heads_construct_with_a_list():
    from ppnet_amd.heads import FCNHead, SETRUPHead, UPerHead, UPerPUPHead, _loss_specs
    cw_list = [dict(type="DiceLoss"), dict(type="CrossEntropyLoss", class_weight=[1.0, 2.0], loss_weight=0.4)]
    heads = [SETRUPHead(in_channels=8, channels=8, num_classes=2, loss_decode=cw_list),
             UPerHead(in_channels=(8, 8, 8, 8), channels=8, num_classes=2, loss_decode=cw_list),
             UPerPUPHead(in_channels=(8, 8, 8, 8), channels=8, num_classes=2, loss_decode=cw_list),
             FCNHead(8, 8, 2, 1, loss_decode=cw_list)]                                   # (raised AttributeError on a list before)
    for h in heads:
        assert h.loss_specs == _loss_specs(cw_list, 2) and not h.loss_single_ce
        assert h.class_weight == (1.0, 2.0) and h.sampler is None                         # the first cross-entropy entry's
    assert heads[3].loss_weight == 1.0                                                    # every entry carries its own
    single = FCNHead(8, 8, 2, 1, loss_decode=dict(type="CrossEntropyLoss", loss_weight=0.4, class_weight=[1.0, 3.0]))
    assert single.loss_weight == 0.4 and single.loss_single_ce and single.class_weight == (1.0, 3.0)
    assert FCNHead(8, 8, 2, 1).loss_weight == 1.0 and FCNHead(8, 8, 2, 1).loss_single_ce
    dice_only = FCNHead(8, 8, 2, 1, loss_decode=dict(type="DiceLoss", loss_weight=0.4, class_weight=[1.0, 3.0]))
    assert dice_only.loss_weight == 1.0 and dice_only.class_weight is None and dice_only.loss_specs[0]["loss_weight"] == 0.4


def _tiny_cfg(decode_loss=None, aux_loss=None, classes=3):
    cfg = dict(backbone=dict(type="SwinTransformer", embed_dims=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), drop_path_rate=0.0),
               decode_head=dict(type="UPerHead", in_channels=[32, 64, 128, 256], channels=16, num_classes=classes, dropout_ratio=0.0),
               auxiliary_head=dict(type="FCNHead", in_channels=128, in_index=2, channels=16, num_convs=1, concat_input=False,
                                   num_classes=classes, dropout_ratio=0.0))
    if decode_loss is not None:
        cfg["decode_head"]["loss_decode"] = decode_loss
    if aux_loss is not None:
        cfg["auxiliary_head"]["loss_decode"] = aux_loss
    return cfg


@pytest.fixture(scope="module")
def tiny_inputs():
    g = torch.Generator().manual_seed(5)
    img = torch.randn(2, 3, 64, 64, generator=g)
    gt = torch.randint(0, 3, (2, 64, 64), generator=g).to(torch.uint8)
    gt[torch.rand(2, 64, 64, generator=g) < 0.1] = 255
    return img, gt


def _net(cfg):
    from ppnet_amd.segnet import SegNet
    torch.manual_seed(0)
    return SegNet.from_config(cfg).train()


def test_tiny_segnet_emits_every_loss_name(tiny_inputs):
    from ppnet_amd import fused, heads
    img, gt = tiny_inputs
    calls = (dict(fused.LOSS_CALLS), dict(fused.DICE_CALLS))
    m = _net(_tiny_cfg(CE_DICE, CE_DICE))
    losses = m(img=img, img_metas=[{}, {}], gt_semantic_seg=gt.unsqueeze(1))
    assert list(losses) == ["decode.loss_ce", "decode.loss_dice", "decode.acc_seg", "aux.loss_ce", "aux.loss_dice", "aux.acc_seg"]
    assert [v.requires_grad for v in losses.values()] == [True, True, False, True, True, False]
    # each entry is its own function of the head's logits: the list changes no value of the cross-entropy entry
    feats = m.backbone(img)
    for name, head in (("decode", m.decode_head), ("aux", m.auxiliary_head)):
        lo = head(feats)
        ce, acc = heads.resized_decode_losses(lo, gt, 1.0)
        full = F.interpolate(lo.float(), (64, 64), mode="bilinear", align_corners=False)
        assert torch.equal(losses[f"{name}.loss_ce"], ce) and torch.equal(losses[f"{name}.acc_seg"], acc)
        assert torch.equal(losses[f"{name}.loss_dice"], heads.dice_loss(full, gt, loss_weight=3.0))
        assert float(losses[f"{name}.loss_dice"].detach()) == pytest.approx(3.0 * float(heads.dice_loss(full, gt.long()).detach()), rel=1e-6)
    sum(v for k, v in losses.items() if "loss" in k).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0 for p in m.decode_head.parameters())
    assert (dict(fused.LOSS_CALLS), dict(fused.DICE_CALLS)) == calls                       # CPU tensors: no launch


def test_equal_loss_names_add_and_dice_alone_gives_the_accuracy(tiny_inputs):
    from ppnet_amd import heads
    img, gt = tiny_inputs
    same = [dict(type="CrossEntropyLoss", loss_name="loss_sum", loss_weight=0.5),
            dict(type="DiceLoss", loss_name="loss_sum", loss_weight=2.0, smooth=0.5, class_weight=[1.0, 2.0, 0.5])]
    m = _net(_tiny_cfg(same, dict(type="DiceLoss", loss_weight=0.4)))
    losses = m.forward_train(img, None, gt)
    assert list(losses) == ["decode.loss_sum", "decode.acc_seg", "aux.loss_dice", "aux.acc_seg"]
    feats = m.backbone(img)
    lo = m.decode_head(feats)
    full = F.interpolate(lo.float(), (64, 64), mode="bilinear", align_corners=False)
    ce, acc = heads.resized_decode_losses(lo, gt, 0.5)
    want = ce + heads.dice_loss(full, gt, 0.5, 2, (1.0, 2.0, 0.5), 2.0)
    assert torch.equal(losses["decode.loss_sum"], want) and torch.equal(losses["decode.acc_seg"], acc)
    lo = m.auxiliary_head(feats)
    full = F.interpolate(lo.float(), (64, 64), mode="bilinear", align_corners=False)
    assert torch.equal(losses["aux.loss_dice"], heads.dice_loss(full, gt, loss_weight=0.4))
    assert float(losses["aux.acc_seg"]) == float((full.argmax(1) == gt).float().sum() * (100.0 / gt.numel()))


def test_single_cross_entropy_config_is_bit_equal_to_resized_decode_losses(tiny_inputs):
    from ppnet_amd import heads
    img, gt = tiny_inputs
    # loss_weight on the decode head's single dict stays unread, the auxiliary head's is applied, as before
    m = _net(_tiny_cfg(dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.7, class_weight=[1.0, 2.0, 0.5]),
                       dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.4)))
    losses = m.forward_train(img, None, gt)
    assert list(losses) == ["decode.loss_ce", "decode.acc_seg", "aux.loss_ce", "aux.acc_seg"]
    feats = m.backbone(img)
    d = heads.resized_decode_losses(m.decode_head(feats), gt, 1.0, class_weight=(1.0, 2.0, 0.5), sampler=None)
    a = heads.resized_decode_losses(m.auxiliary_head(feats), gt, 0.4)
    assert torch.equal(losses["decode.loss_ce"], d[0]) and torch.equal(losses["decode.acc_seg"], d[1])
    assert torch.equal(losses["aux.loss_ce"], a[0]) and torch.equal(losses["aux.acc_seg"], a[1])
    plain = _net(_tiny_cfg()).forward_train(img, None, gt)
    assert list(plain) == list(losses)


def test_one_cpu_training_step_with_the_list_changes_the_weights(tiny_inputs):
    from ppnet_amd import train
    img, gt = tiny_inputs
    net = _net(_tiny_cfg(CE_DICE, CE_DICE))
    before = [p.detach().clone() for p in net.parameters()]
    trainer = train.segnet_trainer(net)
    opt = train.segnet_optimizer(trainer, lr=0.01)
    loss = train.segnet_train_step(trainer, opt, 0, 10, img, gt, schedule=dict(warmup_iters=0))
    with torch.no_grad():
        parts = net.train().forward_train(img, None, gt)
    assert torch.isfinite(loss) and float(loss) > 0 and {"decode.loss_dice", "aux.loss_dice"} <= set(parts)
    changed = sum(not torch.equal(b, p.detach()) for b, p in zip(before, net.parameters()))
    assert changed >= len(before) // 2, (changed, len(before))
    ce_only = _net(_tiny_cfg())
    t2 = train.segnet_trainer(ce_only)
    l2 = train.segnet_train_step(t2, train.segnet_optimizer(t2, lr=0.01), 0, 10, img, gt, schedule=dict(warmup_iters=0))
    assert float(loss) > float(l2)                                                         # the Dice terms are in the sum
