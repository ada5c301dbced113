"""gennet.s2_from_adjoint — the torch form of the stride-2 stages' training kernels (csrc/gennet_s2_train.hip): one adjoint pair D / U and
one reduction W, with the weight as stored — against F.conv2d(.., 2, 1) / F.conv_transpose2d(.., 2, 1, 1) and autograd in float64 on the
CPU, for both layer types at C = 24.  Bound: 1e-12 x each output's maximum (N(0, 1) data: about 4e-14 absolute was measured)."""
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F                                               # noqa: E402

C = 24
SHAPES = [(1, 1, 1), (1, 2, 2), (2, 3, 5), (1, 1, 7), (1, 8, 1), (2, 6, 4), (1, 9, 10), (2, 16, 16)]      # (B, H, W) of the conv input


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_s2_from_adjoint_is_the_layer_and_its_autograd(shape, transposed):
    from ppnet_amd import gennet
    B, H, W = shape
    g = torch.Generator().manual_seed(1000 * H + 10 * W + B + int(transposed))
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(C, C, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(x, w, b, 2, 1, 1) if transposed else F.conv2d(x, w, b, 2, 1)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    want = (y.detach() - b.detach().view(1, C, 1, 1),) + torch.autograd.grad(y, [x, w, b], dy)
    got = gennet.s2_from_adjoint(x.detach(), dy, w.detach(), transposed)
    assert len(got) == 4
    for name, a, r in zip(("forward", "dx", "dw", "dbias"), got, want):
        assert a.shape == r.shape and a.dtype == torch.float64, name
        assert (a - r).abs().max().item() <= 1e-12 * r.abs().max().item(), (name, shape, transposed)


def test_s2_from_adjoint_works_in_the_inputs_dtype():
    from ppnet_amd import gennet
    g = torch.Generator().manual_seed(3)
    x, dy, w = torch.randn(2, C, 5, 6, generator=g), torch.randn(2, C, 3, 3, generator=g), torch.randn(C, C, 3, 3, generator=g)
    out = gennet.s2_from_adjoint(x, dy, w, False)
    assert all(t.dtype == torch.float32 for t in out) and out[0].shape == dy.shape and out[1].shape == x.shape
    ref = gennet.s2_from_adjoint(x.double(), dy.double(), w.double(), False)
    assert all((a.double() - r).abs().max().item() <= 1e-4 * r.abs().max().item() for a, r in zip(out, ref))
