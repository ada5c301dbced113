"""train.segnet_adamw: the parameter groups of SegNet/configs/dinats/dinats_base.py:25-29 — AdamW(lr 6e-5, betas (0.9, 0.999), weight
decay 0.01) with decay 0 for every parameter whose name contains 'rpb' or 'norm'."""
import pytest

torch = pytest.importorskip("torch")


def _tiny():
    from ppnet_amd.segnet import SegNet
    return SegNet(backbone=dict(type="DiNAT_s", embed_dim=32, depths=[1, 2, 1, 1], num_heads=[1, 2, 4, 8], mlp_ratio=2.0),
                  decode_head=dict(in_channels=256, channels=32, num_convs=2, up_scale=2, num_classes=2, kernel_size=3),
                  auxiliary_head=dict(type="FCNHead", in_channels=128, in_index=2, channels=16, num_convs=1, concat_input=False, num_classes=2))


def test_every_trainable_parameter_is_in_exactly_one_group_with_the_configs_decay():
    from ppnet_amd import train
    net = _tiny()
    frozen = net.backbone.norm0.weight
    frozen.requires_grad_(False)
    opt = train.segnet_adamw(net)
    assert isinstance(opt, torch.optim.AdamW) and len(opt.param_groups) == 2
    where = {}
    for gi, g in enumerate(opt.param_groups):
        assert g["lr"] == g["base_lr"] == 6e-5 and tuple(g["betas"]) == (0.9, 0.999)
        for p in g["params"]:
            assert id(p) not in where
            where[id(p)] = gi
    names = dict(net.named_parameters())
    assert {id(p) for p in names.values() if p.requires_grad} == set(where) and id(frozen) not in where
    seen = {"rpb": 0, "norm": 0, "rest": 0}
    for name, p in names.items():
        if not p.requires_grad:
            continue
        decay = opt.param_groups[where[id(p)]]["weight_decay"]
        if "rpb" in name or "norm" in name:
            assert decay == 0.0, name
            seen["rpb" if "rpb" in name else "norm"] += 1
        else:
            assert decay == 0.01, name
            seen["rest"] += 1
    assert min(seen.values()) > 0
    for name in ("backbone.layers.1.blocks.0.attn.rpb", "backbone.layers.0.downsample.norm.weight", "backbone.patch_embed.norm.bias",
                 "backbone.layers.1.blocks.1.norm2.weight", "backbone.norm3.bias"):
        assert opt.param_groups[where[id(names[name])]]["weight_decay"] == 0.0, name
    for name in ("backbone.layers.0.downsample.reduction.weight", "backbone.layers.1.blocks.0.attn.qkv.bias", "backbone.patch_embed.proj.weight",
                 "decode_head.conv_seg.weight"):
        assert opt.param_groups[where[id(names[name])]]["weight_decay"] == 0.01, name


def test_arguments_and_schedule():
    from ppnet_amd import train
    net = _tiny()
    opt = train.segnet_adamw(net, lr=1e-3, betas=(0.8, 0.9), weight_decay=0.1, no_decay=("bias",))
    for g in opt.param_groups:
        assert g["lr"] == 1e-3 and tuple(g["betas"]) == (0.8, 0.9) and g["weight_decay"] in (0.1, 0.0)
    names = dict(net.named_parameters())
    by_id = {id(p): g["weight_decay"] for g in opt.param_groups for p in g["params"]}
    assert all(by_id[id(p)] == (0.0 if "bias" in n else 0.1) for n, p in names.items())
    train.segnet_set_lr(opt, 750, 8000)                                      # the config's warm-up poly schedule reads base_lr
    assert all(g["lr"] == pytest.approx(train.mmseg_poly_lr(1e-3, 750, 8000)) for g in opt.param_groups)
    assert len(train.segnet_adamw(net, no_decay=()).param_groups) == 1      # an empty group is left out
