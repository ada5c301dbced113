"""The reference's SegNet model configs (SegNet/configs/**) as the `model = dict(...)` that SegNet.from_config takes, each merged
with its `_base_` files the way mmcv's Config does.  Data only: this module imports nothing."""


NAT_BASE_UPER = dict(   # SegNet/configs/nat/upernet_nat_base.py:6-34 (the default config of SegNet/test.py:29-32)
    backbone=dict(embed_dim=128, mlp_ratio=2.0, depths=[3, 4, 18, 5], num_heads=[4, 8, 16, 32], kernel_size=7,
                  layer_scale=1e-5),
    decode_head=dict(type="UPerHead", in_channels=[128, 256, 512, 1024], in_index=[0, 1, 2, 3], pool_scales=(1, 2, 3, 6),
                     channels=64, num_classes=2))

DINAT_BASE = dict(   # SegNet/configs/dinat/dinat_base.py:5-24 over _base_/models/dinat.py:3-46
    backbone=dict(embed_dim=128, mlp_ratio=2.0, depths=[3, 4, 18, 5], num_heads=[4, 8, 16, 32], kernel_size=7,
                  layer_scale=1e-5,
                  dilations=[[1, 16, 1], [1, 4, 1, 8], [1, 2, 1, 3, 1, 4, 1, 2, 1, 3, 1, 4, 1, 2, 1, 3, 1, 4], [1, 2, 1, 2, 1]]),
    decode_head=dict(in_channels=1024, channels=512, num_convs=4, up_scale=2, num_classes=2, kernel_size=3))

# DiNAT-L + SETR-UP, the reference's largest model: residual streams of 192 / 384 / 768 / 1536 channels, dilations up to 20.  It sets no
# `layer_scale` (dinat_large.py:7-18; the base file has none either), so the layers have no LayerScale.  `pretrained` (an ImageNet-22k
# checkpoint path on the authors' machine, dinat_large.py:16) is left out: load one with DiNAT.init_weights or load_state_dict.
DINAT_LARGE = dict(   # SegNet/configs/dinat/dinat_large.py:5-24 over _base_/models/dinat.py:3-46
    type="EncoderDecoder", pretrained=None,
    backbone=dict(   # _base_/models/dinat.py:6-22 with dinat_large.py:7-18
        type="DiNAT", embed_dim=192, mlp_ratio=2.0, depths=[3, 4, 18, 5], num_heads=[6, 12, 24, 48], drop_path_rate=0.3, kernel_size=7,
        dilations=[[1, 20, 1], [1, 5, 1, 10], [1, 2, 1, 3, 1, 4, 1, 5, 1, 2, 1, 3, 1, 4, 1, 5, 1, 5], [1, 2, 1, 2, 1]],
        out_indices=(0, 1, 2, 3), qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, in_patch_size=4, frozen_stages=-1),
    decode_head=dict(   # _base_/models/dinat.py:23-43 with dinat_large.py:19-23
        type="SETRUPHead", norm_layer=dict(type="LN", eps=1e-6, requires_grad=True), num_convs=4, up_scale=2, kernel_size=3,
        init_cfg=[dict(type="Constant", val=1.0, bias=0, layer="LayerNorm"), dict(type="Normal", std=0.01, override=dict(name="conv_seg"))],
        in_channels=1536, channels=512, in_index=-1, num_classes=2, norm_cfg=dict(type="SyncBN", requires_grad=True), align_corners=False,
        loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0)),
    train_cfg=dict(), test_cfg=dict(mode="whole"))

# NAT-Mini + UPerHead: streams of 64 / 128 / 256 / 512 channels, mlp_ratio 3 (hidden widths 192 / 384 / 768 / 1536).  `pretrained` (a
# checkpoint path on the authors' machine, upernet_nat_mini.py:16) is left out.
NAT_MINI_UPER = dict(   # SegNet/configs/nat/upernet_nat_mini.py:6-34 over _base_/models/nat.py:3-37
    type="EncoderDecoder", pretrained=None,
    backbone=dict(   # _base_/models/nat.py:6-21 with upernet_nat_mini.py:7-17
        type="NAT", embed_dim=64, mlp_ratio=3.0, depths=[3, 4, 6, 5], num_heads=[2, 4, 8, 16], drop_path_rate=0.2, kernel_size=7,
        out_indices=(0, 1, 2, 3), qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, in_patch_size=4, frozen_stages=-1,
        layer_scale=1e-5),
    decode_head=dict(   # upernet_nat_mini.py:18-29
        type="UPerHead", in_channels=[64, 128, 256, 512], in_index=[0, 1, 2, 3], pool_scales=(1, 2, 3, 6), channels=64, dropout_ratio=0.1,
        num_classes=2, norm_cfg=dict(type="SyncBN", requires_grad=True), align_corners=False,
        loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0)),
    # _base_/models/nat.py:22-34 with upernet_nat_mini.py:30-33: in_channels 512 on in_index 2, although level 2 of NAT-Mini has 256
    # channels — kept as the reference merges it (the override is upernet_nat_base.py's, where level 2 has 512; the auxiliary head runs
    # in training only, which this config cannot do as written)
    auxiliary_head=dict(type="FCNHead", in_channels=512, in_index=2, channels=256, num_convs=1, concat_input=False, dropout_ratio=0.1,
                        num_classes=2, norm_cfg=dict(type="SyncBN", requires_grad=True), align_corners=False,
                        loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.4)),
    train_cfg=dict(), test_cfg=dict(mode="whole"))

# Swin-B: SegNet/configs/_base_/models/swin.py:1-57 merged with configs/swin/swin_base.py:5-37 (SETR-UP) and
# configs/swin/upernet_swin_base.py:5-38 (UPerHead + FCN auxiliary head).  `pretrained` (an ImageNet checkpoint path on the
# authors' machine, swin_base.py:14) is left out: load a checkpoint with SwinTransformer.init_weights or load_state_dict.
_SWIN_BASE_BACKBONE = dict(   # _base_/models/swin.py:7-32 with swin_base.py:7-15
    type="SwinTransformer", pretrain_img_size=224, in_channels=3, embed_dims=128, patch_size=4, window_size=7, mlp_ratio=4,
    depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32), strides=(4, 2, 2, 2), out_indices=(0, 1, 2, 3), qkv_bias=True, qk_scale=None,
    patch_norm=True, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.3, use_abs_pos_embed=False, act_cfg=dict(type="GELU"),
    norm_cfg=dict(type="LN"), with_cp=False, frozen_stages=-1, init_cfg=None)
_SWIN_NORM_CFG = dict(type="SyncBN", requires_grad=True)

SWIN_BASE_SETRUP = dict(
    type="EncoderDecoder", pretrained=None, backbone=dict(_SWIN_BASE_BACKBONE),
    decode_head=dict(   # swin_base.py:16-35
        type="SETRUPHead", norm_layer=dict(type="LN", eps=1e-6, requires_grad=True), num_convs=4, up_scale=2, kernel_size=3,
        init_cfg=[dict(type="Constant", val=1.0, bias=0, layer="LayerNorm"), dict(type="Normal", std=0.01, override=dict(name="conv_seg"))],
        in_channels=1024, channels=512, in_index=-1, num_classes=2, norm_cfg=_SWIN_NORM_CFG, align_corners=False,
        loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0)),
    # _base_/models/swin.py:33-45 as swin_base.py leaves it: in_channels 256 and 19 classes, although level 2 of Swin-B has 512
    # channels — kept as the reference merges it (the auxiliary head only runs in training, which this config cannot do as written)
    auxiliary_head=dict(type="FCNHead", in_channels=256, in_index=2, channels=256, num_convs=1, concat_input=False, dropout_ratio=0.1,
                        num_classes=19, norm_cfg=_SWIN_NORM_CFG, align_corners=False,
                        loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.4)),
    train_cfg=dict(), test_cfg=dict(mode="whole"))

SWIN_BASE_UPER = dict(
    type="EncoderDecoder", pretrained=None, backbone=dict(_SWIN_BASE_BACKBONE),
    decode_head=dict(   # upernet_swin_base.py:17-29
        type="UPerHead", in_channels=[128, 256, 512, 1024], in_index=[0, 1, 2, 3], pool_scales=(1, 2, 3, 6), channels=512,
        dropout_ratio=0.1, num_classes=2, norm_cfg=_SWIN_NORM_CFG, align_corners=False,
        loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0)),
    auxiliary_head=dict(   # _base_/models/swin.py:33-45 with upernet_swin_base.py:30-33
        type="FCNHead", in_channels=512, in_index=2, channels=256, num_convs=1, concat_input=False, dropout_ratio=0.1, num_classes=2,
        norm_cfg=_SWIN_NORM_CFG, align_corners=False, loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.4)),
    train_cfg=dict(), test_cfg=dict(mode="whole"))

# The dense configs: UPerPUPHead (mmseg/decode_heads/uper_pup_head.py) on NAT-B and Swin-B.  `pretrained` (checkpoint paths on the
# authors' machine, dense_nat_base.py:16, dense_swin_base.py:14) is left out, as in the SWIN_BASE_* dicts.
_UPERPUP_AUX = dict(   # the base models' FCNHead (_base_/models/nat.py:22-34, swin.py:32-44) with in_channels=512, num_classes=2
    # (dense_nat_base.py:31-34, dense_swin_base.py:30-33)
    type="FCNHead", in_channels=512, in_index=2, channels=256, num_convs=1, concat_input=False, dropout_ratio=0.1, num_classes=2,
    norm_cfg=_SWIN_NORM_CFG, align_corners=False, loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.4))

NAT_BASE_UPERPUP = dict(   # SegNet/configs/nat/dense_nat_base.py:5-35 over _base_/models/nat.py:1-37
    type="EncoderDecoder", pretrained=None,
    backbone=dict(   # nat.py:6-21 with dense_nat_base.py:7-17
        type="NAT", embed_dim=128, mlp_ratio=2.0, depths=[3, 4, 18, 5], num_heads=[4, 8, 16, 32], drop_path_rate=0.5, kernel_size=7,
        out_indices=(0, 1, 2, 3), qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, in_patch_size=4, frozen_stages=-1,
        layer_scale=1e-5),
    decode_head=dict(   # dense_nat_base.py:18-30
        type="UPerPUPHead", in_channels=[128, 256, 512, 1024], in_index=[0, 1, 2, 3], num_convs=(1, 2, 3, 4), pool_scales=(1, 2, 3, 6),
        channels=256, dropout_ratio=0.1, num_classes=2, norm_cfg=_SWIN_NORM_CFG, align_corners=False,
        loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0)),
    auxiliary_head=dict(_UPERPUP_AUX),
    train_cfg=dict(), test_cfg=dict(mode="whole"))

SWIN_BASE_UPERPUP = dict(   # SegNet/configs/swin/dense_swin_base.py:5-34 over _base_/models/swin.py:1-47
    type="EncoderDecoder", pretrained=None, backbone=dict(_SWIN_BASE_BACKBONE),   # dense_swin_base.py:7-16 = swin_base.py:7-15
    decode_head=dict(   # dense_swin_base.py:17-29
        type="UPerPUPHead", in_channels=[128, 256, 512, 1024], in_index=[0, 1, 2, 3], num_convs=(2, 3, 4, 5), pool_scales=(1, 2, 3, 6),
        channels=256, dropout_ratio=0.1, num_classes=2, norm_cfg=_SWIN_NORM_CFG, align_corners=False,
        loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0)),
    auxiliary_head=dict(_UPERPUP_AUX),
    train_cfg=dict(), test_cfg=dict(mode="whole"))

# ViT-B/16 + SETR-UP: configs/vit/vit_base.py:1-30 names '../_base_/models/setr.py' (line 2), which the reference tree lacks; the
# base model file that exists, _base_/models/vit.py:1-43, is that SETR model (EncoderDecoder + VisionTransformer + SETRUPHead with
# the in_channels=768 of vit_base.py:26).  It cannot build alone (embed_dims=1024 with 12 heads, line 11-13), so it is merged here
# with vit_base.py's overrides (lines 5-29): embed 768, 12 layers, 12 heads of 64, no cls token, patch 16.  `pretrained` (an
# ImageNet checkpoint path on the authors' machine, vit_base.py:16) is left out: load one with VisionTransformer.init_weights.
VIT_BASE_SETRUP = dict(
    type="EncoderDecoder", pretrained=None,
    backbone=dict(   # _base_/models/vit.py:6-17 with vit_base.py:7-16
        type="VisionTransformer", img_size=224, patch_size=16, in_channels=3, embed_dims=768, num_layers=12, num_heads=12,
        drop_rate=0.0, norm_cfg=dict(type="LN", eps=1e-6, requires_grad=True), with_cls_token=False),
    decode_head=dict(   # _base_/models/vit.py:18-39 with vit_base.py:18-22
        type="SETRUPHead", norm_layer=dict(type="LN", eps=1e-6, requires_grad=True), num_convs=4, up_scale=2, kernel_size=3,
        init_cfg=[dict(type="Constant", val=1.0, bias=0, layer="LayerNorm"), dict(type="Normal", std=0.01, override=dict(name="conv_seg"))],
        in_channels=768, channels=512, in_index=-1, num_classes=2, norm_cfg=dict(type="SyncBN", requires_grad=True), align_corners=False,
        loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0)),
    train_cfg=dict(), test_cfg=dict(mode="whole"))

# DiNAT_s-B + SETR-UP: configs/dinats/dinats_base.py:1-22 names '../_base_/models/dinats.py' (line 2), which the reference tree lacks,
# so this is a RECONSTRUCTION, as VIT_BASE_SETRUP is.  Backbone: the constructor defaults of the class itself (SegNet/dinats.py:207-228:
# patch 4, mlp_ratio 4, qkv_bias, patch_norm, out_indices 0-3, no frozen stage) with dinats_base.py's overrides (lines 6-17).  Head: the
# config's decode-head overrides (lines 18-22: in_channels 1024, num_convs 4, up_scale 2, num_classes 2) are exactly dinat_base.py's
# (configs/dinat/dinat_base.py:20-24), so the SETR-UP head they override is taken to be that config's base,
# _base_/models/dinat.py:23-43.  `pretrained` (an ImageNet checkpoint path on the authors' machine, dinats_base.py:14) is left out: load
# one with DiNAT_s.init_weights.  The config trains with AdamW (lines 25-29): train.segnet_adamw.
DINATS_BASE_SETRUP = dict(
    type="EncoderDecoder", pretrained=None,
    backbone=dict(   # dinats.py:207-228 with dinats_base.py:6-17
        type="DiNAT_s", pretrain_img_size=224, patch_size=4, in_chans=3, embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32],
        kernel_size=7, dilations=[[1, 16], [1, 8], [1, 2, 1, 3, 1, 4, 1, 2, 1, 3, 1, 4, 1, 2, 1, 3, 1, 4], [1, 2]], mlp_ratio=4.0,
        qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.3, patch_norm=True, out_indices=(0, 1, 2, 3),
        frozen_stages=-1),
    decode_head=dict(   # _base_/models/dinat.py:23-43 with dinats_base.py:18-22
        type="SETRUPHead", norm_layer=dict(type="LN", eps=1e-6, requires_grad=True), num_convs=4, up_scale=2, kernel_size=3,
        init_cfg=[dict(type="Constant", val=1.0, bias=0, layer="LayerNorm"), dict(type="Normal", std=0.01, override=dict(name="conv_seg"))],
        in_channels=1024, channels=512, in_index=-1, num_classes=2, norm_cfg=dict(type="SyncBN", requires_grad=True), align_corners=False,
        loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=1.0)),
    train_cfg=dict(), test_cfg=dict(mode="whole"))
