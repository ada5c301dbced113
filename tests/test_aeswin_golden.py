"""Pins ppnet_amd.gennet.AESwin (own module, reference key names) against outputs of the reference's GenNet/networks/ae_swin.py
captured in tests/golden/g25_aeswin.npz (tests/golden/make_aeswin_fixture.py).  CPU: the same PyTorch runs both, in float64 here,
so differences are reassociation only; the bounds are the AE-ViT golden test's (tests/test_gennet_golden.py: 2e-5 x max(1, max|y|)
for the module, 5e-5 x for the BatchNorm-folded one)."""
import copy
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_fixture_model(golden_dir, R=128, dtype=torch.float64):
    """(AESwin(1, 1, R, 24) in eval mode with the fixture's weights, the archive).  Shared with tests/test_gpu_aeswin.py."""
    from ppnet_amd.gennet import AESwin
    g = np.load(os.path.join(golden_dir, "g25_aeswin.npz"))
    m = AESwin(1, 1, R, 24).eval()
    keys = [str(k) for k in g["keys"]]
    assert list(m.state_dict().keys()) == keys and len(keys) == 247      # the reference's entries, in its order
    sd = {k: torch.from_numpy(g["w/" + k].astype(np.int64) if k.endswith("relative_position_index") else g["w/" + k]) for k in keys}
    m.load_state_dict(sd, strict=True)
    return m.to(dtype), g


@pytest.fixture(scope="module")
def model64(golden_dir):
    return load_fixture_model(golden_dir)


def _close(got, want, rel):
    err = np.abs(got - want).max()
    assert got.shape == want.shape and err < rel * max(1.0, np.abs(want).max()), err


def test_state_dict_is_the_references(model64):
    m, g = model64
    assert sum(p.numel() for p in m.parameters()) == 259705
    from ppnet_amd import swin
    for w, s in ((7, 0), (14, 1)):
        assert torch.equal(m.swin[s].blocks[0].attn.relative_position_index, swin._relative_index(w))
    assert [b.attn.shift for st in m.swin for b in st.blocks] == [0, 3, 0, 7, 0, 0, 7, 0, 7, 0, 7, 0, 0, 3]
    rates = [b.drop_path_rate for st in m.swin for b in st.blocks]
    assert rates[0] == 0.0 and abs(rates[-1] - 0.1) < 1e-7 and all(b > a for a, b in zip(rates, rates[1:]))
    assert m.swin[0].blocks[0].norm1.eps == 1e-5 and len(m.enc_conv) == len(m.dec_conv) == 1


@pytest.mark.parametrize("R", [128, 112])
def test_cpu_float64_matches_reference(model64, R):
    """R = 128: token grids 64 / 32 / 16, every stage padded; R = 112: 56 / 28 / 14, none padded (one window with four regions in
    the middle stage's shifted blocks)."""
    m, g = model64
    with torch.no_grad():
        got = m(torch.from_numpy(g[f"x{R}"]).double()).numpy()
    _close(got, g[f"y{R}"].astype(np.float64), 2e-5)


def test_block_matches_reference(model64):
    m, g = model64
    x = torch.from_numpy(g["blk_in"]).double().view(1, 32, 32, 24)
    with torch.no_grad():
        got, _ = m.swin[1].blocks[1](x)
    _close(got.reshape(1024, 24).numpy(), g["blk_out"].astype(np.float64), 2e-5)


@pytest.mark.parametrize("R", [128, 112])
def test_prepared_cpu_matches_reference(model64, R):
    m, g = model64
    f = copy.deepcopy(m).prepare_inference()
    assert not any(isinstance(mod, torch.nn.BatchNorm2d) for mod in f.modules())      # the four inside the Swin stages included
    with torch.no_grad():
        got = f(torch.from_numpy(g[f"x{R}"]).double()).numpy()
    _close(got, g[f"y{R}"].astype(np.float64), 5e-5)


def test_dropin_module_path(monkeypatch):
    import ppnet_amd.gennet as G
    monkeypatch.syspath_prepend(os.path.join(ROOT, "ppnet_amd", "dropin"))
    names = ("networks", "networks.ae_swin")
    for n in names:
        sys.modules.pop(n, None)
    try:
        from networks.ae_swin import AESwin            # the reference's own module path
        assert AESwin is G.AESwin
    finally:
        for n in names:
            sys.modules.pop(n, None)


def test_train_mode_backward_is_finite(golden_dir):
    m, g = load_fixture_model(golden_dir, 112, torch.float32)
    m.train()
    torch.manual_seed(0)
    y = m(torch.from_numpy(g["x112"]).float() / 255.0)
    assert y.shape == (2, 1, 112, 112)
    y.square().mean().backward()
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
