"""CPU-side checks of ppn_resize_ce_workspace / ppn_resize_ce_fwd / ppn_resize_ce_bwd (csrc/resize_ce.hip): header, library and
bindings carry the three entry points at ABI 111 with the agreed argument names; the workspace size follows the header's formula;
every bad argument is refused with PPN_E_INVALID before any HIP call (the pointers below are never dereferenced); the source is in
the Makefile's SRCS, cross-compiles with the Makefile's flags for gfx950 and no kernel of it uses scratch; and on the CPU
SegNet.forward_train is the library composition bit for bit (the kernel branch cannot be entered without a GPU)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ppnet_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
E_INVALID = -1
ONE = C.c_void_p(0x1000)                                       # 16-byte aligned, never dereferenced on these paths
NAMES = ("ppn_resize_ce_workspace", "ppn_resize_ce_fwd", "ppn_resize_ce_bwd")
FWD_PIXELS = 1024                                              # the header: one float32 sum and one int32 count per 1024 pixels


def _args(decl):
    code = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    return [a.split()[-1].lstrip("*") for a in code.split(",")]


def test_header_library_and_bindings_carry_the_entry_points_at_abi_111():
    from ppnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "ppnet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert int(re.search(r"#define\s+PPN_ABI_VERSION\s+(\d+)", header).group(1)) == 111
    assert _lib.ABI_VERSION == 111 and _lib.lib.ppn_version() == 111
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.EXPORTS and hasattr(_lib.lib, n), n
    version_comment = re.search(r"/\* ABI version of this header.*?\*/", header, re.S).group(0)
    assert all(n in version_comment for n in NAMES)                        # the sentence saying that they joined at 111
    assert _args(re.search(r"int64_t\s+ppn_resize_ce_workspace\s*\((.*?)\)\s*;", code, re.S).group(1)) == ["B", "H", "W"]
    assert _args(re.search(r"int\s+ppn_resize_ce_fwd\s*\((.*?)\)\s*;", code, re.S).group(1)) == [
        "logit", "label", "lse", "loss", "correct", "workspace", "workspace_floats", "B", "C", "h", "w", "H", "W", "ignore_index",
        "logit_dtype", "label_dtype", "stream"]
    assert _args(re.search(r"int\s+ppn_resize_ce_bwd\s*\((.*?)\)\s*;", code, re.S).group(1)) == [
        "logit", "label", "lse", "grad_out", "dlogit", "B", "C", "h", "w", "H", "W", "ignore_index", "logit_dtype", "label_dtype", "stream"]
    assert len(_lib.lib.ppn_resize_ce_fwd.argtypes) == 17 and len(_lib.lib.ppn_resize_ce_bwd.argtypes) == 15
    assert _lib.lib.ppn_resize_ce_workspace.restype is C.c_int64
    # the definitions in capi.hip have the header's lists
    capi = open(os.path.join(CSRC, "capi.hip")).read()
    for n, k in (("ppn_resize_ce_fwd", 17), ("ppn_resize_ce_bwd", 15), ("ppn_resize_ce_workspace", 3)):
        assert len(_args(re.search(r"\b%s\s*\((.*?)\)\s*\{" % n, capi, re.S).group(1))) == k, n


def test_workspace_size():
    from ppnet_amd import _lib
    w = _lib.lib.ppn_resize_ce_workspace
    for B, H, W in ((1, 1, 1), (1, 5, 3), (1, 32, 32), (1, 1, 1025), (2, 128, 128), (8, 512, 512), (3, 1000, 999), (1, 1023, 1), (1, 1024, 1)):
        assert w(B, H, W) == 2 * -(-(B * H * W) // FWD_PIXELS), (B, H, W)
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4, -1, 4), (4, 4, -1)):
        assert w(*bad) < 0, bad
    assert w(1, 1 << 16, 1 << 15) < 0 and w(2, 1 << 15, 1 << 15) < 0 and w(1 << 11, 1 << 10, 1 << 10) < 0    # exactly 2^31 pixels
    assert w(1 << 20, 1 << 20, 1 << 20) < 0 and w(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1) < 0                 # far past 64 bits' comfort
    assert w(1, 2 ** 31 - 1, 1) == 2 * (1 << 21) and w(2 ** 31 - 1, 1, 1) > 0 and w(1, 1, 2 ** 31 - 1) > 0    # just below


def _caller(f, ok):
    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    return call


@pytest.mark.parametrize("logit_dtype", [0, 1])
@pytest.mark.parametrize("label_dtype", [0, 1])
def test_fwd_rejects_bad_arguments_without_gpu(logit_dtype, label_dtype):
    from ppnet_amd import _lib
    need = _lib.lib.ppn_resize_ce_workspace(2, 64, 48)
    assert need == 2 * 6
    #                                        logit label lse loss correct ws  ws_floats B  C  h   w   H   W   ignore ldt          labdt        stream
    call = _caller(_lib.lib.ppn_resize_ce_fwd, [ONE, ONE, ONE, ONE, ONE, ONE, need, 2, 3, 16, 12, 64, 48, 255, logit_dtype, label_dtype, None])
    for i in (0, 1, 3, 4, 5):                                              # every pointer but lse
        assert call(**{f"a{i}": None}) == E_INVALID, i
    for i, off in ((0, 8), (0, 2), (2, 4), (2, 8), (5, 4), (5, 8)):        # 16-byte alignment of logit, lse, workspace
        assert call(**{f"a{i}": C.c_void_p(0x1000 + off)}) == E_INVALID, (i, off)
    assert call(a3=C.c_void_p(0x1002)) == E_INVALID                        # loss: a float
    assert call(a4=C.c_void_p(0x1004)) == E_INVALID                        # correct: an int64
    if label_dtype == 1:
        assert call(a1=C.c_void_p(0x1004)) == E_INVALID                    # int64 labels
    for i in range(7, 13):                                                 # B, C, h, w, H, W
        assert call(**{f"a{i}": 0}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID, i
        assert call(**{f"a{i}": 0, "a6": 1 << 62}) == E_INVALID, i
    for i in (14, 15):
        assert call(**{f"a{i}": 2}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID, i
    assert call(a6=need - 1) == E_INVALID and call(a6=0) == E_INVALID and call(a6=-1) == E_INVALID
    huge = 1 << 62
    assert call(a7=1, a11=1 << 16, a12=1 << 15, a6=huge) == E_INVALID      # B H W = 2^31
    assert call(a7=1 << 11, a11=1 << 10, a12=1 << 10, a6=huge) == E_INVALID
    assert call(a7=2 ** 31 - 1, a11=2 ** 31 - 1, a12=2 ** 31 - 1, a6=huge) == E_INVALID
    assert call(a7=1, a8=1 << 11, a9=1 << 10, a10=1 << 10, a6=huge) == E_INVALID        # B C h w = 2^31
    assert call(a8=2 ** 31 - 1, a9=2 ** 31 - 1, a10=2 ** 31 - 1, a6=huge) == E_INVALID


@pytest.mark.parametrize("logit_dtype", [0, 1])
@pytest.mark.parametrize("label_dtype", [0, 1])
def test_bwd_rejects_bad_arguments_without_gpu(logit_dtype, label_dtype):
    from ppnet_amd import _lib
    #                                        logit label lse grad dlogit B  C  h   w   H   W   ignore ldt          labdt        stream
    call = _caller(_lib.lib.ppn_resize_ce_bwd, [ONE, ONE, ONE, ONE, ONE, 2, 3, 16, 12, 64, 48, 255, logit_dtype, label_dtype, None])
    for i in range(5):                                                     # each pointer, lse included
        assert call(**{f"a{i}": None}) == E_INVALID, i
    for i, off in ((0, 8), (0, 2), (2, 4), (2, 8), (4, 8), (4, 2)):        # 16-byte alignment of logit, lse, dlogit
        assert call(**{f"a{i}": C.c_void_p(0x1000 + off)}) == E_INVALID, (i, off)
    assert call(a3=C.c_void_p(0x1002)) == E_INVALID                        # grad_out: a float
    if label_dtype == 1:
        assert call(a1=C.c_void_p(0x1004)) == E_INVALID
    for i in range(5, 11):                                                 # B, C, h, w, H, W
        assert call(**{f"a{i}": 0}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID, i
    for i in (12, 13):
        assert call(**{f"a{i}": 2}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID, i
    assert call(a5=1, a9=1 << 16, a10=1 << 15) == E_INVALID                # B H W = 2^31
    assert call(a5=1 << 11, a9=1 << 10, a10=1 << 10) == E_INVALID
    assert call(a5=1, a6=1 << 11, a7=1 << 10, a8=1 << 10) == E_INVALID     # B C h w = 2^31
    assert call(a6=2 ** 31 - 1, a7=2 ** 31 - 1, a8=2 ** 31 - 1) == E_INVALID
    # x16: a wave per dlogit element, so 2^25 elements are a launch of 2^31 work-items
    assert call(a5=1, a6=2, a7=1 << 12, a8=1 << 12, a9=1 << 16, a10=1 << 14) == E_INVALID


def test_resize_ce_source_is_built_and_uses_no_scratch(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not present")
    out = tmp_path / "resize_ce.s"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "resize_ce.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    flags = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize --cuda-device-only -S".split()
    for fl in flags[:-2]:
        assert fl.replace("gfx950", "$(ARCH)") in mk, fl                            # the Makefile's own flags
    subprocess.run([HIPCC, *flags, os.path.join(CSRC, "resize_ce.hip"), "-o", str(out)], check=True, cwd=CSRC, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    asm = out.read_text()
    scratch = dict(re.findall(r"\.amdhsa_kernel (\S+).*?; ScratchSize: (\d+)", asm, re.S))
    # forward per (logit type, label type); the final sum; backward per (logit type, label type, lanes per output: 1, 8, 64)
    assert sum("resize_ce_fwd_kernel" in k for k in scratch) == 4, scratch
    assert sum("resize_ce_final_kernel" in k for k in scratch) == 1, scratch
    assert sum("resize_ce_bwd_kernel" in k for k in scratch) == 12, scratch
    assert len(scratch) == 17 and all("resize_ce_" in k for k in scratch), scratch
    assert all(int(v) == 0 for v in scratch.values()), scratch


def test_cpu_forward_train_is_the_library_composition_bit_for_bit(monkeypatch):
    """Without a GPU the kernel branch cannot be entered: a tiny SegNet's losses and every parameter gradient equal the run with
    PPNET_LIBRARY_LOSS=1 and the run with forward_train's earlier two lines patched in, and no launch is counted."""
    torch = pytest.importorskip("torch")
    import torch.nn as nn
    import torch.nn.functional as F
    from ppnet_amd import fused, heads, segnet
    from ppnet_amd.segnet import SegNet, decode_losses
    assert segnet.resized_decode_losses is heads.resized_decode_losses and segnet.decode_losses is heads.decode_losses
    cfg = dict(backbone=dict(type="SwinTransformer", embed_dims=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), drop_path_rate=0.1),
               decode_head=dict(type="UPerPUPHead", in_channels=[32, 64, 128, 256], channels=16, num_convs=(1, 2, 3, 4), num_classes=3),
               auxiliary_head=dict(type="FCNHead", in_channels=128, in_index=2, channels=16, num_convs=1, concat_input=False, num_classes=3,
                                   loss_decode=dict(loss_weight=0.4)))
    torch.manual_seed(0)
    m = SegNet.from_config(cfg).train()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    img = torch.randn(2, 3, 64, 64)
    gt8 = torch.randint(0, 3, (2, 1, 64, 64)).to(torch.uint8)
    gt8[0, 0, :5] = 255
    calls = dict(fused.LOSS_CALLS)

    def run(gt):
        m.load_state_dict(sd)                                                      # BatchNorm's running statistics back too
        m.zero_grad(set_to_none=True)
        torch.manual_seed(3)                                                       # dropout, stochastic depth
        losses = m(img=img, img_metas=[{}, {}], gt_semantic_seg=gt)
        assert list(losses) == ["decode.loss_ce", "decode.acc_seg", "aux.loss_ce", "aux.acc_seg"]
        assert [v.requires_grad for v in losses.values()] == [True, False, True, False]
        (losses["decode.loss_ce"] + losses["aux.loss_ce"]).backward()
        return [v.detach().clone() for v in losses.values()] + [p.grad.clone() for p in m.parameters() if p.grad is not None]
    a = run(gt8)
    a64 = run(gt8.long())
    monkeypatch.setenv("PPNET_LIBRARY_LOSS", "1")
    b = run(gt8)
    monkeypatch.delenv("PPNET_LIBRARY_LOSS")

    def forward_train_before(self, img, img_metas, gt_semantic_seg, **kwargs):     # the method before the kernel branch
        feats = self.backbone(img)
        gt = gt_semantic_seg.squeeze(1).long() if gt_semantic_seg.dim() == 4 else gt_semantic_seg.long()
        losses = {}
        hs = [("decode", self.decode_head, 1.0)] + [(f"aux_{i}" if isinstance(self.auxiliary_head, nn.ModuleList) else "aux", h, h.loss_weight)
                                                    for i, h in enumerate(self._aux_heads())]
        for name, head, w in hs:
            logit = F.interpolate(head(feats).float(), gt.shape[-2:], mode="bilinear", align_corners=head.align_corners)
            losses[f"{name}.loss_ce"], losses[f"{name}.acc_seg"] = decode_losses(logit, gt, w)
        return losses
    monkeypatch.setattr(SegNet, "forward_train", forward_train_before)
    c = run(gt8)
    assert len(a) == len(a64) == len(b) == len(c) > 4 + 20
    for u, u64, v, w in zip(a, a64, b, c):
        assert torch.equal(u, v) and torch.equal(u, w) and torch.equal(u, u64)
    assert float(a[0]) > 0 and float(a[2]) > 0 and 0 <= float(a[1]) <= 100
    assert fused.LOSS_CALLS == calls == {"fwd": calls["fwd"], "bwd": calls["bwd"]}


def test_resize_cross_entropy_refuses_cpu_tensors():
    torch = pytest.importorskip("torch")
    from ppnet_amd import fused
    assert fused.LOSS_CALLS.keys() == {"fwd", "bwd"}
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        fused.resize_cross_entropy(torch.randn(1, 2, 4, 4, requires_grad=True), torch.zeros(1, 8, 8, dtype=torch.uint8))
    # and the heads' entry takes the library composition there, with the same values as decode_losses on the resized logits
    import torch.nn.functional as F
    from ppnet_amd.heads import decode_losses, resized_decode_losses
    lg, gt = torch.randn(2, 3, 4, 5), torch.randint(0, 3, (2, 9, 7))
    got = resized_decode_losses(lg, gt, 0.4)
    ref = decode_losses(F.interpolate(lg, (9, 7), mode="bilinear", align_corners=False), gt, 0.4)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
