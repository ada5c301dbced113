"""CPU-side checks of the training pair of the residual + LayerNorm kernel (csrc/residual_ln_bwd.hip): the three entries are exported
and bound, their argument checks answer before any HIP call, the workspace size behaves, and the torch forms that CPU tensors (and
PPNET_LIBRARY_NORM=1) take are pinned: fused.residual_layer_norm(..., scale=s) against x + s * gamma * a -> F.layer_norm in values
and gradients, and a seeded training-mode NATLayer against the formula it had before the scale argument existed."""
import ctypes as C
import os

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

NEW = ("ppn_residual_layernorm_train_fwd", "ppn_residual_layernorm_bwd_workspace", "ppn_residual_layernorm_bwd")
WIDTHS = (8, 24, 64, 128, 256, 512, 1024)
PPN_E_INVALID, PPN_E_UNSUPPORTED = -1, -3


def test_entries_are_exported_and_bound():
    from ppnet_amd import _lib
    for name in NEW:
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib, name).argtypes is not None
    assert _lib.lib.ppn_residual_layernorm_bwd_workspace.restype is C.c_int64
    assert _lib.PPN_E_UNSUPPORTED == PPN_E_UNSUPPORTED
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ppnet_hip.h")).read()
    assert all(name in header for name in NEW)


def _bwd(L, **kw):
    """ppn_residual_layernorm_bwd on never-dereferenced pointers; keyword arguments replace the valid defaults."""
    one = C.c_void_p(0x1000)
    a = dict(gy=one, gx=one, xn=one, a=one, gamma=one, scale=None, w=one, stats=one, dx=one, da=one, dgamma=one, dw=one, dbeta=one, workspace=one,
             workspace_floats=None, rows=105, rows_per_image=35, C=128, dtype=0)
    a.update(kw)
    if a["workspace_floats"] is None:
        a["workspace_floats"] = max(L.ppn_residual_layernorm_bwd_workspace(a["rows"], a["C"]), 1 << 20)
    return L.ppn_residual_layernorm_bwd(a["gy"], a["gx"], a["xn"], a["a"], a["gamma"], a["scale"], a["w"], a["stats"], a["dx"], a["da"], a["dgamma"],
                                        a["dw"], a["dbeta"], a["workspace"], a["workspace_floats"], a["rows"], a["rows_per_image"], a["C"], a["dtype"],
                                        None)


def test_backward_rejects_bad_arguments_without_gpu():
    from ppnet_amd import _lib
    L = _lib.lib
    one = C.c_void_p(0x1000)
    assert _bwd(L, xn=None) == PPN_E_INVALID
    assert _bwd(L, rows=0) == PPN_E_INVALID
    assert _bwd(L, dtype=2) == PPN_E_INVALID
    assert _bwd(L, C=768) == PPN_E_UNSUPPORTED
    assert _bwd(L, C=12) == PPN_E_UNSUPPORTED
    need = L.ppn_residual_layernorm_bwd_workspace(105, 128)
    assert _bwd(L, workspace_floats=need - 1) == PPN_E_INVALID
    assert _bwd(L, scale=one, rows_per_image=34) == PPN_E_INVALID          # 105 % 34
    assert _bwd(L, gy=None, gx=None) == PPN_E_INVALID                      # no gradient at all
    assert _bwd(L, workspace=None) == PPN_E_INVALID
    assert _bwd(L, gy=None) == PPN_E_INVALID                               # dw / dbeta without the LayerNorm's gradient
    assert _bwd(L, a=None) == PPN_E_INVALID                                # dgamma without a


def test_forward_rejects_bad_arguments_without_gpu():
    from ppnet_amd import _lib
    L = _lib.lib
    one = C.c_void_p(0x1000)

    def fwd(x=one, a=one, gamma=one, scale=None, w=one, b=one, x_out=one, y_out=one, stats=one, rows=105, rpi=35, Cw=128, dtype=0):
        return L.ppn_residual_layernorm_train_fwd(x, a, gamma, scale, w, b, x_out, y_out, stats, rows, rpi, Cw, 1e-5, dtype, None)
    assert fwd(x=None) == PPN_E_INVALID
    assert fwd(rows=0) == PPN_E_INVALID
    assert fwd(dtype=2) == PPN_E_INVALID
    assert fwd(x_out=None) == PPN_E_INVALID                                # a residual with nowhere to go
    assert fwd(a=None, y_out=None) == PPN_E_INVALID                        # a plain LayerNorm with nowhere to go
    assert fwd(stats=None) == PPN_E_INVALID
    assert fwd(w=None) == PPN_E_INVALID
    assert fwd(scale=one, rpi=34) == PPN_E_INVALID
    assert fwd(Cw=768) == PPN_E_UNSUPPORTED
    assert fwd(Cw=12) == PPN_E_UNSUPPORTED


def test_workspace_is_positive_and_does_not_shrink():
    from ppnet_amd import _lib
    ws = _lib.lib.ppn_residual_layernorm_bwd_workspace
    for Cw in WIDTHS:
        sizes = [ws(rows, Cw) for rows in (1, 3, 4, 5, 16, 17, 105, 256, 257, 4096, 4097, 16384, 16385, 262144, 262145, 10 ** 6, 10 ** 8)]
        assert sizes[0] > 0 and sizes[0] % (3 * Cw) == 0
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), (Cw, sizes)
        assert sizes[-1] == sizes[-2]                                        # the workgroup cap: the partials stop growing
    assert ws(0, 128) < 0 and ws(105, 768) < 0 and ws(105, 12) < 0


@pytest.mark.parametrize("with_gamma", [True, False], ids=["gamma", "no_gamma"])
@pytest.mark.parametrize("with_ln", [True, False], ids=["ln", "no_ln"])
def test_cpu_tensors_take_the_torch_form(with_gamma, with_ln):
    """float64, so that the two association orders of s * gamma * a agree to 1e-12."""
    from ppnet_amd import fused
    g = torch.Generator().manual_seed(3)
    B, H, W, Cw = 3, 2, 5, 16
    x, a = (torch.randn(B, H, W, Cw, generator=g, dtype=torch.float64) for _ in range(2))
    gamma = torch.rand(Cw, generator=g, dtype=torch.float64) + 0.5 if with_gamma else None
    ln = torch.nn.LayerNorm(Cw).double() if with_ln else None
    if ln is not None:
        with torch.no_grad():
            ln.weight.copy_(torch.randn(Cw, generator=g, dtype=torch.float64))
            ln.bias.copy_(torch.randn(Cw, generator=g, dtype=torch.float64))
    s = torch.tensor([1 / 0.75, 0.0, 1 / 0.75], dtype=torch.float32)
    gxw, gyw = (torch.randn(B, H, W, Cw, generator=g, dtype=torch.float64) for _ in range(2))
    calls = dict(fused.NORM_CALLS)

    def run(ours):
        leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (x, a, gamma)]
        xl, al, gl = leaves
        if ln is not None:
            ln.zero_grad(set_to_none=True)
        if ours:
            xn, y = fused.residual_layer_norm(xl, al, gl, ln, scale=s)
        else:
            sd = s.double()[:, None, None, None]
            xn = xl + (sd * gl * al if gl is not None else sd * al)
            y = F.layer_norm(xn, (Cw,), ln.weight, ln.bias, ln.eps) if ln is not None else None
        assert (y is None) == (ln is None)
        loss = (xn * gxw).sum() + ((y * gyw).sum() if y is not None else 0.0)
        loss.backward()
        grads = [t.grad for t in leaves if t is not None] + ([ln.weight.grad.clone(), ln.bias.grad.clone()] if ln is not None else [])
        return [xn.detach()] + ([y.detach()] if y is not None else []) + grads
    for got, want in zip(run(True), run(False)):
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    assert fused.NORM_CALLS == calls                                         # no kernel on CPU tensors


def test_seeded_training_natlayer_keeps_its_drop_path_formula():
    """NATLayer with drop_path 0.5 in training mode on the CPU: the output of a seeded call equals x + gamma * drop_path(f(.)) — the
    composition before the mask became residual_layer_norm's scale — bit for bit from the same seed (same draws, same order), and
    x + drop_path(gamma * f(.)), the reference's association, to rounding."""
    from ppnet_amd.dense import drop_path
    from ppnet_amd.nat import NATLayer

    class Mix(torch.nn.Module):                                              # stands in for the GPU-only neighbourhood attention
        def __init__(self, dim):
            super().__init__()
            self.proj = torch.nn.Linear(dim, dim)

        def forward(self, x, real_hw=None):
            return self.proj(x)
    torch.manual_seed(0)
    layer = NATLayer(16, 2, kernel_size=7, dilation=1, mlp_ratio=2.0, drop_path=0.5, layer_scale=0.3)
    layer.attn = Mix(16)
    layer.train()
    nxt = torch.nn.LayerNorm(16)
    x = torch.randn(6, 3, 4, 16, requires_grad=True)
    torch.manual_seed(123)
    x2, y2 = layer(x, None, nxt)
    torch.manual_seed(123)
    t = x + layer.gamma1 * drop_path(layer.attn(layer.norm1(x)), 0.5, True)
    want = t + layer.gamma2 * drop_path(layer.mlp(layer.norm2(t)), 0.5, True)
    assert torch.equal(x2, want) and torch.equal(y2, nxt(want))
    torch.manual_seed(123)
    t = x + drop_path(layer.gamma1 * layer.attn(layer.norm1(x)), 0.5, True)
    ref = t + drop_path(layer.gamma2 * layer.mlp(layer.norm2(t)), 0.5, True)
    torch.testing.assert_close(x2, ref, rtol=1e-6, atol=1e-6)
    # eval mode and rate 0 pass no scale
    assert layer.eval()._drop_scale(x) is None
    layer.train().drop_path_rate = 0.0
    assert layer._drop_scale(x) is None
