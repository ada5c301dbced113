"""GenNet's AESwin (ppnet_amd.gennet.AESwin) on the GPU: the real model (dim 192) on the window-attention kernels, the fixture model
(dim 24, head dims 4 / 2 / 1: every attention on the torch composition) against the reference's recorded outputs, one training
step, and PPNet with AESwin as its GenNet.

The kernel path's bound is measured, not fixed: the same forward with PPNET_LIBRARY_WMSA=1 (every attention on the library
composition) gives the error of everything that is not the attention — the convolutions' and GEMMs' own — and the kernel path
must stay within 2 x that floor: a correct attention adds error at float32 rounding level, far below it."""
import copy

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda"
R = 128


@pytest.fixture(scope="module")
def real_model():
    """(AESwin(1, 1, 128, 192) in eval mode, a {0, 1} input of batch 2, the unprepared module's float64 CPU output)."""
    from ppnet_amd.gennet import AESwin
    torch.manual_seed(0)
    m = AESwin(1, 1, R, 192).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("relative_position_bias_table"):
                p.normal_(0.0, 0.5)
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 1.5)
                mod.weight.uniform_(0.8, 1.2)
                mod.bias.uniform_(-0.1, 0.1)
    x = (torch.rand(2, 1, R, R) > 0.5).float()
    with torch.no_grad():
        want = copy.deepcopy(m).double()(x.double())
    return m, x, want


def _forward(model, x, monkeypatch, library):
    from ppnet_amd import swin
    if library:
        monkeypatch.setenv("PPNET_LIBRARY_WMSA", "1")
    else:
        monkeypatch.delenv("PPNET_LIBRARY_WMSA", raising=False)
    swin.CALLS.update(kernel=0, torch=0)
    with torch.no_grad():
        y = model(x)
    torch.cuda.synchronize()
    monkeypatch.delenv("PPNET_LIBRARY_WMSA", raising=False)
    return y, dict(swin.CALLS)


def test_real_model_float32_on_the_kernels(real_model, monkeypatch, capsys):
    m, x, want = real_model
    p = copy.deepcopy(m).prepare_inference().to(DEV)
    xg = x.to(DEV).contiguous(memory_format=torch.channels_last)
    y, calls = _forward(p, xg, monkeypatch, False)
    assert calls == {"kernel": 14, "torch": 0}                          # every block's attention on a HIP kernel
    ylib, calls = _forward(p, xg, monkeypatch, True)
    assert calls == {"kernel": 0, "torch": 14}
    rng = (want.max() - want.min()).item()
    err = (y.double().cpu() - want).abs().max().item()
    floor = (ylib.double().cpu() - want).abs().max().item()
    with capsys.disabled():
        print(f"\nAESwin dim 192 float32 vs float64: kernel path {err:.3e}, library-attention floor {floor:.3e}, output range {rng:.3e}")
    assert y.shape == want.shape and rng > 0
    assert err <= 2 * floor, (err, floor)


def test_real_model_bfloat16_on_the_kernels(real_model, monkeypatch, capsys):
    m, x, _ = real_model
    p32 = copy.deepcopy(m).prepare_inference().to(DEV)
    xg = x.to(DEV).contiguous(memory_format=torch.channels_last)
    y32, _ = _forward(p32, xg, monkeypatch, False)
    p16 = copy.deepcopy(m).prepare_inference().to(DEV).to(torch.bfloat16)
    x16 = xg.to(torch.bfloat16)
    y, calls = _forward(p16, x16, monkeypatch, False)
    assert calls == {"kernel": 14, "torch": 0}
    ylib, calls = _forward(p16, x16, monkeypatch, True)
    assert calls == {"kernel": 0, "torch": 14}
    err = (y.float() - y32).abs().max().item()
    floor = (ylib.float() - y32).abs().max().item()
    with capsys.disabled():
        print(f"\nAESwin dim 192 bfloat16 vs float32: kernel path {err:.3e}, library-attention floor {floor:.3e}, "
              f"output range {(y32.max() - y32.min()).item():.3e}")
    assert y.dtype == torch.bfloat16 and bool(torch.isfinite(y.float()).all())
    assert err <= 2 * floor, (err, floor)


@pytest.mark.parametrize("prepared", [False, True])
def test_fixture_model_matches_reference(golden_dir, prepared):
    """dim 24: head dims 4 / 2 / 1 have no kernel, so all 14 attentions are the composition on the GPU; the bound is the AE-ViT GPU
    golden test's (float32 on the libraries)."""
    from ppnet_amd import swin
    from tests.test_aeswin_golden import load_fixture_model
    m, g = load_fixture_model(golden_dir, R, torch.float32)
    m = (m.prepare_inference() if prepared else m).to(DEV)
    for res in (128, 112):
        x = torch.from_numpy(g[f"x{res}"]).float().to(DEV)
        swin.CALLS.update(kernel=0, torch=0)
        with torch.no_grad():
            got = m(x.contiguous(memory_format=torch.channels_last) if prepared else x).float().cpu().numpy()
        assert swin.CALLS == {"kernel": 0, "torch": 14}
        y = g[f"y{res}"]
        assert got.shape == y.shape and np.abs(got - y).max() < 1e-3 * max(1.0, np.abs(y).max())


def test_one_training_step():
    from ppnet_amd import train
    from ppnet_amd.gennet import AESwin
    torch.manual_seed(1)
    m = AESwin(1, 1, 112, 24).to(DEV)
    opt = train.gennet_optimizer(m)
    space = (torch.rand(2, 112, 112, device=DEV) > 0.5).to(torch.uint8)
    path = (torch.rand(2, 112, 112, device=DEV) * 255).to(torch.uint8)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    loss = train.gennet_train_step(m, opt, None, space, path)
    assert bool(torch.isfinite(loss))
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    assert any(not torch.equal(before[n], p.detach()) for n, p in m.named_parameters())


@pytest.fixture()
def tunable_state():
    """PPNet() switches PyTorch's TunableOp on for the process (its read-only GEMM table); put it back, so that the library GEMMs of
    the tests that run after this file are picked as they were without it."""
    import torch.cuda.tunable as tn
    was = tn.is_enabled()
    yield
    tn.enable(was)


def test_ppnet_runs_with_aeswin(tunable_state):
    """PPNet(128, gennet=AESwin(1, 1, 128, 192)) as with AE-ViT: heat maps and plans for 4 generated problems."""
    from ppnet_amd import edage
    from ppnet_amd.gennet import AESwin
    from ppnet_amd.ppnet import PPNet
    from ppnet_amd.segnet import SegNet
    dev = torch.device("cuda:0")
    P, Q, K = 4, 1, 20
    torch.manual_seed(0)
    tiny = SegNet(backbone=dict(type="NAT", embed_dim=32, mlp_ratio=2.0, depths=[1, 1], num_heads=[1, 2], kernel_size=7, out_indices=(0, 1)),
                  decode_head=dict(type="SETRUPHead", in_channels=64, channels=64, in_index=1, num_classes=2, num_convs=1, up_scale=2, kernel_size=3))
    model = PPNet(R, segnet=tiny.eval(), gennet=AESwin(1, 1, R, 192).eval()).to(dev).eval()
    pb, mb = edage.PathsBatch(P, R, 50, 3, dev), edage.MapsBatch(P * Q, R, K, dev)
    out = model.generate_and_plan(pb, mb, Q, 0, 0, seed=9, obstacles_size=5, obstacles_num=K)
    torch.cuda.synchronize()
    heat = out["heat"]
    assert heat.shape == (P * Q, R, R) and heat.dtype == torch.uint8
    assert all(int(h.max()) == 255 and int(h.min()) == 0 for h in heat)   # per-sample min-max of a non-constant map
    assert torch.equal(model.heatmap(out["mask"]), heat)
    res = out["result"]
    assert res["ok"].shape[0] == P * Q and res["waypoints"].shape[0] == P * Q and res["success"].shape[0] == P * Q
