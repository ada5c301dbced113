"""The decode heads' up-sampling backward kernels (csrc/upsample_bwd.hip: ppn_upsample2x_nhwc_bwd, ppn_upsample2x_concat_nhwc_bwd,
ppn_resize_concat_nhwc_bwd), their autograd Functions (ppnet_amd/fused.py) and the heads that train on them, on the GPU.

1. the x2 kernel against the definition: float64 CPU autograd of F.interpolate(F.relu(x) if relu else x, scale_factor=2, bilinear).
   The x2 weights (0.25, 0.75, 1) and their products are exact in float32, so only the 16-term float32 sum rounds: with S the
   transpose applied to |dy|, |got - ref| <= 2^-19 S in float32 (16 terms x 2^-24, a factor 2) and <= 2^-8 |ref| + 2^-19 S in
   bfloat16 (one rounding of the result);
2. every dx element is written and nothing else (dx a view into a NaN-filled buffer);
3. two calls give the same bits, all three entries;
4. the concat backward equals, bit for bit, the x2 backward on contiguous copies of the channel slices;
5. the general resize backward is the transpose of the forward kernel: W from one-hot images through fused.resize_concat, expected
   W^T dy in float64, |got - ref| <= (n + 2) 2^-23 (|W|^T |dy|) with n the most outputs one input pixel gathers (every product and
   every partial sum rounds once: n + n_x + n_y + 1 roundings of 2^-24 at most, n_x n_y = n) — bfloat16 adds 2^-8 |ref| — and
   within twice that of the library's float32 CUDA backward of F.interpolate + torch.cat, which differs in summation order only;
6. autograd wiring: the Functions are recorded, their outputs equal the no_grad call's bits, PPNET_LIBRARY_UPSAMPLE=1 records the
   library composition;
7. one training step of a tiny SegNet per head (SETR-UP, UPerHead, UPerPUPHead), with the size gate open and as shipped: the expected
   Functions are recorded, the losses equal the PPNET_LIBRARY_UPSAMPLE=1 path's and a float64 CPU run's, every parameter receives a
   finite gradient — and EVERY up-sampling call of the step is checked where it ran: its inputs, its output, the gradient that
   arrived at its output and the gradients it handed to its inputs are captured in the step itself, and those gradients are held
   against the float64 definition of that call with the derived bounds of 1. and 5.  This replaces a comparison of whole-network
   parameter gradients with the library path's (at most twice its distance to a float64 run): both distances sit at float32's
   rounding noise (1e-6 to 1e-5 of a gradient), a training step is not bit-reproducible from run to run, and the ratio of two noise
   samples decides nothing — it failed by a few percent in about one run of three, for this change and without it.  The captured
   form is deterministic (the kernels are bitwise reproducible), has a derived bound, and checks the gradients the step really
   used."""
import copy
import ctypes

import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_resize_ce import _definition, _model_run, tiny_model  # noqa: E402,F401  (tiny_model: its module-scoped fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = torch.nn.functional
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]


ZERO_GATE = {torch.float32: 0, torch.bfloat16: 0}


@pytest.fixture
def open_gate(monkeypatch):
    """fused.UPSAMPLE_RECORD_MIN is the size from which the single-operator forms record their kernels (a measured routing choice,
    DESIGN.md section 21); the tests' tensors are far below it.  Tests that ask for this fixture run those forms with the gate
    open; test_size_gate and the heads' "shipped" cases run the shipped gate."""
    from ppnet_amd import fused
    monkeypatch.setattr(fused, "UPSAMPLE_RECORD_MIN", dict(ZERO_GATE))


def _randn(shape, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def _up2_ref(x_nhwc, dy_nhwc, relu):
    """(dx, S) in float64 on the CPU, NHWC: autograd of the definition with dy, and of the plain operator with |dy|."""
    xd = x_nhwc.double().cpu().permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.interpolate(F.relu(xd) if relu else xd, scale_factor=2, mode="bilinear", align_corners=False)
    dx, = torch.autograd.grad(y, xd, dy_nhwc.double().cpu().permute(0, 3, 1, 2))
    z = torch.zeros_like(xd).requires_grad_(True)
    s, = torch.autograd.grad(F.interpolate(z, scale_factor=2, mode="bilinear", align_corners=False), z, dy_nhwc.double().cpu().permute(0, 3, 1, 2).abs())
    return dx.permute(0, 2, 3, 1), s.permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------ 1. the x2 kernel
# (B, H, W, C): both borders on one pixel; one axis degenerate (twice); 24 channels = 3 channel groups; odd sizes and a batch
# stride; (W + 1) C / 8 = 328 > 256; and ceil(W / 2) C / 8 = 264: more than one 256-thread piece of this kernel's 2 x 2 block rows
UP2_SHAPES = [(1, 1, 1, 8), (2, 1, 2, 8), (2, 2, 1, 8), (2, 2, 3, 24), (2, 5, 7, 16), (1, 3, 40, 64), (1, 2, 66, 64)]


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", UP2_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_up2x_bwd_against_the_definition(shape, dtype, relu):
    from ppnet_amd import fused
    B, H, W, C = shape
    x = _randn((B, H, W, C), 11 + H * W, dtype)                              # about half negative
    x.view(-1)[::5] = 0                                                     # exact zeros: the gradient there is 0
    dy = _randn((B, 2 * H, 2 * W, C), 12 + H * W, dtype)
    got = fused._upsample2x_bwd(dy.to(DEV), x.to(DEV) if relu else None)
    torch.cuda.synchronize()
    assert got.shape == (B, H, W, C) and got.dtype == dtype
    ref, S = _up2_ref(x, dy, relu)
    err = (got.double().cpu() - ref).abs()
    bound = 2.0 ** -19 * S + (2.0 ** -8 * ref.abs() if dtype == torch.bfloat16 else 0.0)
    assert bool((err <= bound).all()), (float(err.max()), float((err - bound).max()))
    if relu:
        assert bool((got.cpu()[x <= 0] == 0).all())
    if shape == (1, 1, 1, 8) and not relu and dtype == torch.float32:       # dx = the sum of the four dy
        assert torch.allclose(got.cpu().view(-1), dy.sum(dim=(1, 2)).view(-1), rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------------------------------------ 2. written exactly once
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_up2x_bwd_writes_every_element_and_nothing_else(dtype, relu):
    from ppnet_amd import _lib as L
    B, H, W, C = 2, 5, 7, 16
    n, guard = B * H * W * C, 4 * W * C
    buf = torch.full((guard + n + guard,), float("nan"), dtype=dtype, device=DEV)
    dx = buf[guard:guard + n].view(B, H, W, C)
    x = _randn((B, H, W, C), 21, dtype).to(DEV)
    dy = _randn((B, 2 * H, 2 * W, C), 22, dtype).to(DEV)
    rc = L.lib.ppn_upsample2x_nhwc_bwd(ctypes.c_void_p(dy.data_ptr()), ctypes.c_void_p(x.data_ptr() if relu else None), ctypes.c_void_p(dx.data_ptr()),
                                       B, H, W, C, 0 if dtype == torch.float32 else 1, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isfinite(dx).all())
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all())


# ------------------------------------------------------------------------------------------------ 3. / 4. reproducible; concat = slices
def _cl(t):
    return t.to(DEV).permute(0, 3, 1, 2)                                    # NHWC on the host -> a channels_last [B,C,H,W] device tensor


def _concat_grads(levels, dout):
    from ppnet_amd import fused
    xs = [t.detach().requires_grad_(True) for t in levels]
    return torch.autograd.grad(fused.upsample2x_concat(xs), xs, dout)


def _resize_grads(levels, dout):
    from ppnet_amd import fused
    xs = [t.detach().requires_grad_(True) for t in levels]
    return torch.autograd.grad(fused.resize_concat(xs), xs, dout)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bitwise_reproducible(dtype):
    from ppnet_amd import fused
    x, dy = _randn((2, 5, 7, 16), 31, dtype).to(DEV), _randn((2, 10, 14, 16), 32, dtype).to(DEV)
    for xx in (None, x):
        assert torch.equal(fused._upsample2x_bwd(dy, xx), fused._upsample2x_bwd(dy, xx))
    levels = [_cl(_randn((2, 3, 5, c), 33 + c, dtype)) for c in (8, 24, 16)]
    dout = _cl(_randn((2, 6, 10, 48), 34, dtype))
    assert all(torch.equal(a, b) for a, b in zip(_concat_grads(levels, dout), _concat_grads(levels, dout)))
    levels = [_cl(_randn((2, h, w, 8), 35 + h, dtype)) for h, w in ((7, 7), (1, 1), (2, 2), (3, 3), (6, 6))]
    dout = _cl(_randn((2, 7, 7, 40), 36, dtype))
    assert all(torch.equal(a, b) for a, b in zip(_resize_grads(levels, dout), _resize_grads(levels, dout)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_concat_bwd_bit_equal_to_the_x2_bwd_of_its_slices(dtype):
    from ppnet_amd import fused
    ch = [8, 24, 16]
    levels = [_cl(_randn((2, 3, 5, c), 41 + c, dtype)) for c in ch]
    dout_nhwc = _randn((2, 6, 10, sum(ch)), 42, dtype).to(DEV)
    got = _concat_grads(levels, dout_nhwc.permute(0, 3, 1, 2))
    off = 0
    for g, c in zip(got, ch):
        want = fused._upsample2x_bwd(dout_nhwc[..., off:off + c].contiguous(), None)
        assert g.shape == (2, c, 3, 5) and g.permute(0, 2, 3, 1).is_contiguous()
        assert torch.equal(g.permute(0, 2, 3, 1), want)
        off += c
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. the general resize backward
RESIZE_SETS = {"pyramid7": ((7, 7), [(1, 1), (2, 2), (3, 3), (6, 6)]),     # the pyramid at R = 224: non-integer ratios
               "fpn12x8": ((12, 8), [(6, 4), (3, 2), (2, 1)]),             # the FPN's x2 / x4 / x6 on a non-square grid
               "same6x5": ((6, 5), [(6, 5), (3, 3)])}                      # a level of level 0's size: a bit-exact copy
_W_CACHE = {}


def _weights(H0, W0, h, w):
    """The forward kernel's float32 weight matrix [H0 W0, h w] of one level, as float64 on the CPU: one-hot images through
    fused.resize_concat (a batch of h w images, 8 channels)."""
    key = (H0, W0, h, w)
    if key not in _W_CACHE:
        from ppnet_amd import fused
        eye = torch.eye(h * w, device=DEV).view(h * w, h, w, 1).expand(h * w, h, w, 8).contiguous()
        with torch.no_grad():
            out = fused.resize_concat([torch.zeros(h * w, 8, H0, W0, device=DEV), eye.permute(0, 3, 1, 2)])
        _W_CACHE[key] = out[:, 8].reshape(h * w, H0 * W0).t().double().cpu()                # [output pixel, input pixel]
    return _W_CACHE[key]


def _forward_weights(name):
    (H0, W0), small = RESIZE_SETS[name]
    return [_weights(H0, W0, h, w) for h, w in small]


def _resize_ref(Wm, dy_nhwc, h, w):
    """(W^T dy, the bound (n + 2) 2^-23 |W|^T |dy|) in float64 for one level's channel slice dy [B,H0,W0,C] (CPU)."""
    B, C = dy_nhwc.shape[0], dy_nhwc.shape[3]
    dy = dy_nhwc.double().reshape(B, -1, C)
    ref = torch.einsum("oi,boc->bic", Wm, dy).view(B, h, w, C)
    S = torch.einsum("oi,boc->bic", Wm.abs(), dy.abs()).view(B, h, w, C)
    return ref, (int((Wm != 0).sum(dim=0).max()) + 2) * 2.0 ** -23 * S


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(RESIZE_SETS))
def test_resize_concat_bwd_is_the_transpose_of_the_forward_kernel(name, dtype):
    (H0, W0), small = RESIZE_SETS[name]
    mats = _forward_weights(name)
    B, sizes = 2, [(H0, W0)] + small
    levels = [_cl(_randn((B, h, w, 8), 51 + 7 * h + w, dtype)) for h, w in sizes]
    dout_nhwc = _randn((B, H0, W0, 8 * len(sizes)), 52, dtype)
    got = _resize_grads(levels, _cl(dout_nhwc))
    torch.cuda.synchronize()
    assert torch.equal(got[0].permute(0, 2, 3, 1).cpu(), dout_nhwc[..., :8])                # level 0: its slice, bit for bit
    lib_x = [t.detach().float().requires_grad_(True) for t in levels]
    lib_out = torch.cat([lib_x[0]] + [F.interpolate(t, size=(H0, W0), mode="bilinear", align_corners=False) for t in lib_x[1:]], dim=1)
    lib = torch.autograd.grad(lib_out, lib_x, _cl(dout_nhwc).float())
    for l, ((h, w), Wm) in enumerate(zip(small, mats), start=1):
        dy = dout_nhwc[..., 8 * l:8 * l + 8].double().reshape(B, H0 * W0, 8)
        g = got[l].permute(0, 2, 3, 1)
        assert g.shape == (B, h, w, 8) and g.dtype == dtype
        if (h, w) == (H0, W0):
            assert torch.equal(g.cpu(), dout_nhwc[..., 8 * l:8 * l + 8])
            continue
        ref = torch.einsum("oi,boc->bic", Wm, dy).view(B, h, w, 8)
        S = torch.einsum("oi,boc->bic", Wm.abs(), dy.abs()).view(B, h, w, 8)
        n = int((Wm != 0).sum(dim=0).max())
        bound = (n + 2) * 2.0 ** -23 * S
        err = (g.double().cpu() - ref).abs()
        full = bound + (2.0 ** -8 * ref.abs() if dtype == torch.bfloat16 else 0.0)
        assert bool((err <= full).all()), (name, (h, w), n, float(err.max()), float((err - full).max()))
        if dtype == torch.float32:
            dlib = (g.double().cpu() - lib[l].permute(0, 2, 3, 1).double().cpu()).abs()
            assert bool((dlib <= 2.0 * bound).all()), (name, (h, w), float(dlib.max()), float((dlib - 2.0 * bound).max()))


# ------------------------------------------------------------------------------------------------ 6. autograd wiring
def _wiring_cases(dtype):
    from ppnet_amd import fused
    x = _cl(_randn((2, 3, 5, 16), 61, dtype))
    fine = _cl(_randn((2, 6, 10, 16), 62, dtype))
    lv2 = [_cl(_randn((2, 3, 5, c), 63 + c, dtype)) for c in (8, 16)]
    lvr = [_cl(_randn((2, h, w, 8), 64 + h, dtype)) for h, w in ((6, 5), (3, 2), (1, 1))]
    return [("_Upsample2xFunction", lambda t: fused.upsample2x_nhwc(t[0], False), [x]),
            ("_Upsample2xFunction", lambda t: fused.upsample2x_nhwc(t[0], True), [x]),
            ("_Upsample2xAddFunction", lambda t: fused.upsample2x_add(t[0], t[1]), [fine, x]),
            ("_Upsample2xConcatFunction", lambda t: fused.upsample2x_concat(t), lv2),
            ("_ResizeConcatFunction", lambda t: fused.resize_concat(t), lvr)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_autograd_records_the_kernels(dtype, monkeypatch, open_gate):
    ours = ("_Upsample2xFunction", "_Upsample2xAddFunction", "_Upsample2xConcatFunction", "_ResizeConcatFunction")
    for fn_name, call, tensors in _wiring_cases(dtype):
        xs = [t.detach().requires_grad_(True) for t in tensors]
        y = call(xs)
        assert type(y.grad_fn).__name__ == fn_name + "Backward", (fn_name, y.grad_fn)
        with torch.no_grad():
            plain = call(xs)
        assert plain.grad_fn is None and torch.equal(y.detach(), plain)
        grads = torch.autograd.grad(y, xs, torch.ones_like(y))
        assert all(g.shape == t.shape and g.dtype == t.dtype and bool(torch.isfinite(g).all()) for g, t in zip(grads, xs))
        monkeypatch.setenv("PPNET_LIBRARY_UPSAMPLE", "1")
        lib = call(xs)
        with torch.no_grad():
            assert torch.equal(call(xs), plain)                                        # inference is untouched by the knob
        monkeypatch.delenv("PPNET_LIBRARY_UPSAMPLE")
        assert lib.grad_fn is not None and not any(o in type(lib.grad_fn).__name__ for o in ours), (fn_name, lib.grad_fn)
        tol = 1e-5 if dtype == torch.float32 else 2.0 ** -6
        assert bool(((lib.detach().float() - plain.float()).abs() <= tol * plain.float().abs().clamp(min=1.0)).all())
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_size_gate(dtype):
    """With the shipped gate the single-operator forms record their kernels from UPSAMPLE_RECORD_MIN output elements and the library
    composition below; upsample2x_concat and resize_concat have no gate."""
    from ppnet_amd import fused
    need = fused.UPSAMPLE_RECORD_MIN[dtype]
    assert need == {torch.float32: 1 << 23, torch.bfloat16: (1 << 20) + 1}[dtype]
    W = -(-need // (4 * 4 * 64 * 64))                                       # [4, 64, 64, W] -> 4 x as many output elements >= need
    big = torch.zeros(4, 64, W, 64, dtype=dtype, device=DEV).permute(0, 3, 1, 2).requires_grad_(True)
    small = torch.zeros(4, 64, W - 1, 64, dtype=dtype, device=DEV).permute(0, 3, 1, 2).requires_grad_(True)
    assert 4 * big.numel() >= need > 4 * small.numel()
    assert type(fused.upsample2x_nhwc(big, True).grad_fn).__name__ == "_Upsample2xFunctionBackward"
    assert type(fused.upsample2x_nhwc(small, True).grad_fn).__name__ != "_Upsample2xFunctionBackward"
    h = -(-need // (4 * 2 * 64 * 64))                                       # fine [4, 2h, 64, 64] NHWC: 32768 h elements
    for hh, name_is in ((h, True), (h - 1, False)):
        fine = torch.zeros(4, 2 * hh, 64, 64, dtype=dtype, device=DEV).permute(0, 3, 1, 2).requires_grad_(True)
        coarse = torch.zeros(4, hh, 32, 64, dtype=dtype, device=DEV).permute(0, 3, 1, 2).requires_grad_(True)
        assert (fine.numel() >= need) == name_is
        assert (type(fused.upsample2x_add(fine, coarse).grad_fn).__name__ == "_Upsample2xAddFunctionBackward") == name_is
    tiny = [torch.zeros(1, 8, 2, 2, dtype=dtype, device=DEV).requires_grad_(True) for _ in range(2)]
    assert type(fused.upsample2x_concat(tiny).grad_fn).__name__ == "_Upsample2xConcatFunctionBackward"
    assert type(fused.resize_concat(tiny).grad_fn).__name__ == "_ResizeConcatFunctionBackward"


def test_upsample2x_add_passes_the_gradient_through_to_fine(open_gate):
    from ppnet_amd import fused
    fine = _cl(_randn((2, 6, 10, 16), 71, torch.float32)).requires_grad_(True)
    coarse = _cl(_randn((2, 3, 5, 16), 72, torch.float32)).requires_grad_(True)
    g = _cl(_randn((2, 6, 10, 16), 73, torch.float32))
    d_fine, d_coarse = torch.autograd.grad(fused.upsample2x_add(fine, coarse), [fine, coarse], g)
    assert torch.equal(d_fine, g)
    assert torch.equal(d_coarse.permute(0, 2, 3, 1), fused._upsample2x_bwd(g.permute(0, 2, 3, 1).contiguous(), None))
    with torch.no_grad():                                                               # the in-place form's bits
        assert torch.equal(fused.upsample2x_add(fine, coarse), fused.upsample2x_add_(fine.detach().clone(memory_format=torch.preserve_format), coarse))


# ------------------------------------------------------------------------------------------------ 7. the heads, end to end
def _uper_cfg(head):
    """tests/test_gpu_resize_ce.py's tiny DiNAT backbone and FCN auxiliary head (stochastic depth and dropout at 0) under the small
    UPerHead / UPerPUPHead of tests/test_uperpup_golden.py (16 channels, chains 1-2-3-4)."""
    from tests.test_gpu_resize_ce import TINY_AUX, TINY_SEG
    # pool scales (1, 2): the last level of a 64 x 64 image is 2 x 2, and the kernel takes no pooled map larger than it
    heads = {"UPerHead": dict(type="UPerHead", in_channels=[32, 64, 128, 256], channels=16, num_classes=2, dropout_ratio=0.0, pool_scales=(1, 2)),
             "UPerPUPHead": dict(type="UPerPUPHead", in_channels=[32, 64, 128, 256], channels=16, num_convs=(1, 2, 3, 4), num_classes=2,
                                 dropout_ratio=0.0, pool_scales=(1, 2))}
    return dict(backbone=dict(TINY_SEG["backbone"]), decode_head=heads[head], auxiliary_head=dict(TINY_AUX))


_UPER_MODELS = {}


def _uper_model(head):
    """(the float32 network on the CPU, image, labels, the float64 CPU losses and gradients), built once per head; the CPU run takes
    the float64 definition of the neighbourhood attention, as tests/test_gpu_resize_ce.py's tiny_model does."""
    if head not in _UPER_MODELS:
        from oracle import segnet_ref as SR
        from ppnet_amd import na
        from ppnet_amd.segnet import SegNet, randomize_neutral_parameters
        torch.manual_seed(5)
        net = randomize_neutral_parameters(SegNet(**_uper_cfg(head)), seed=6).train()
        g = torch.Generator().manual_seed(7)
        img = torch.randn(4, 3, 64, 64, generator=g)                        # 4 images: the 1 x 1 pooled map's BatchNorm sees 4 values
        gt = torch.randint(0, 2, (4, 64, 64), generator=g).to(torch.uint8)
        gt[torch.rand(4, 64, 64, generator=g) < 0.1] = 255
        own = na.NeighborhoodAttention2D.forward

        def forward(self, x, real_hw=None):
            if x.is_cuda:
                return own(self, x, real_hw)
            return SR.na_fp64(x, self.qkv.weight, self.qkv.bias, self.rpb, self.proj.weight, self.proj.bias, self.num_heads, 7, self.dilation)
        na.NeighborhoodAttention2D.forward = forward
        try:
            ref = _model_run(copy.deepcopy(net).double(), img.double(), gt, forward=_definition)
        finally:
            na.NeighborhoodAttention2D.forward = own
        _UPER_MODELS[head] = (net, img, gt, ref)
    return _UPER_MODELS[head]


def _recorded(losses):
    """Names of the autograd nodes behind the losses."""
    seen, names, todo = set(), set(), [v.grad_fn for v in losses.values() if v.grad_fn is not None]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.add(type(f).__name__)
        todo.extend(n for n, _ in f.next_functions)
    return names


EXPECT_NODES = {"SETRUPHead": {"_Upsample2xFunctionBackward"},
                "UPerHead": {"_Upsample2xAddFunctionBackward", "_ResizeConcatFunctionBackward"},
                "UPerPUPHead": {"_Upsample2xAddFunctionBackward", "_ResizeConcatFunctionBackward", "_Upsample2xFunctionBackward",
                                "_Upsample2xConcatFunctionBackward"}}
OURS = set().union(*EXPECT_NODES.values())


def _nhwc_cpu(t):
    return t.detach().permute(0, 2, 3, 1).cpu()


def _capture(monkeypatch):
    """Wraps the four public up-sampling entries of ppnet_amd.fused: every call made while autograd records is logged with its
    inputs, its output, the gradient arriving at the output and the gradient the call hands to each input.  The inputs go in
    through a view of their own, so that a tensor with other consumers reports this call's share alone."""
    from ppnet_amd import fused
    log, real = [], {}

    def wrap(name, split):
        real[name] = getattr(fused, name)

        def entry(*args):
            tensors, rest = split(*args)
            if not fused.recording(*tensors):
                return real[name](*args)
            views = [t.view_as(t) for t in tensors]
            e = dict(name=name, rest=rest, inputs=[t.detach() for t in tensors], gin=[None] * len(views), gout=None)
            for i, v in enumerate(views):
                assert v.requires_grad
                v.register_hook(lambda g, i=i, e=e: e["gin"].__setitem__(i, g.detach()))
            y = real[name](views[0], *rest) if name == "upsample2x_nhwc" else real[name](*views) if name == "upsample2x_add" else real[name](views)
            e["out"], e["node"] = y.detach(), type(y.grad_fn).__name__
            y.register_hook(lambda g, e=e: e.__setitem__("gout", g.detach()))
            log.append(e)
            return y
        monkeypatch.setattr(fused, name, entry)
    wrap("upsample2x_nhwc", lambda x, relu=False, bias=None: ([x], (relu, bias)))
    wrap("upsample2x_add", lambda fine, coarse: ([fine, coarse], ()))
    wrap("upsample2x_concat", lambda levels: (list(levels), ()))
    wrap("resize_concat", lambda levels: (list(levels), ()))
    return log, real


def _check_up2(x, gout_nhwc, gin, relu, what):
    ref, S = _up2_ref(_nhwc_cpu(x), gout_nhwc, relu)
    err = (_nhwc_cpu(gin).double() - ref).abs()
    assert bool((err <= 2.0 ** -19 * S).all()), (what, float(err.max()), float((err - 2.0 ** -19 * S).max()))
    return float((err / (2.0 ** -19 * S).clamp(min=1e-300)).max())


def _check_call(e, real):
    """One logged call: float32 gradients against the float64 definition, bounds as in 1. and 5.; returns the largest error / bound."""
    name, xs, gout = e["name"], e["inputs"], _nhwc_cpu(e["gout"])
    assert e["gout"] is not None and all(g is not None and g.shape == x.shape and g.dtype == torch.float32 for g, x in zip(e["gin"], xs)), name
    if e["node"] in OURS:                                                   # the recorded forward is the inference kernel's, bit for bit
        with torch.no_grad():
            plain = real[name](xs[0], *e["rest"]) if name == "upsample2x_nhwc" else real[name](*xs) if name == "upsample2x_add" else real[name](xs)
        assert torch.equal(plain, e["out"]), name
    if name == "upsample2x_nhwc":
        assert e["rest"][1] is None
        return _check_up2(xs[0], gout, e["gin"][0], bool(e["rest"][0]), name)
    if name == "upsample2x_add":
        assert torch.equal(e["gin"][0], e["gout"])                          # the identity to `fine`
        return _check_up2(xs[1], gout, e["gin"][1], False, name)
    worst, off = 0.0, 0
    H0, W0 = xs[0].shape[2:]
    for x, g in zip(xs, e["gin"]):
        c, (h, w) = x.shape[1], x.shape[2:]
        dy = gout[..., off:off + c].contiguous()
        off += c
        if name == "upsample2x_concat":
            worst = max(worst, _check_up2(x, dy, g, False, name))
        elif (h, w) == (H0, W0):
            assert torch.equal(_nhwc_cpu(g), dy), name                      # a level of level 0's size: its slice
        else:
            ref, bound = _resize_ref(_weights(H0, W0, h, w), dy, h, w)
            err = (_nhwc_cpu(g).double() - ref).abs()
            assert bool((err <= bound).all()), (name, (h, w), float(err.max()), float((err - bound).max()))
            worst = max(worst, float((err / bound.clamp(min=1e-300)).max()))
    return worst


# calls per head in one step of the tiny networks below: SETR-UP's four stages; UPerHead's pyramid output, three top-down sums and
# FPN output; UPerPUPHead's pyramid output, three sums, the six inner x2 steps of its 1-2-3-4 chains and the last step + concatenation
EXPECT_CALLS = {"SETRUPHead": {"upsample2x_nhwc": 4},
                "UPerHead": {"resize_concat": 2, "upsample2x_add": 3},
                "UPerPUPHead": {"resize_concat": 1, "upsample2x_add": 3, "upsample2x_nhwc": 6, "upsample2x_concat": 1}}
GATED = {"_Upsample2xFunctionBackward", "_Upsample2xAddFunctionBackward"}  # the single-operator forms: the library below the shipped gate


def _head_step(head, model, gate, monkeypatch, capsys):
    from ppnet_amd import fused
    cpu_net, img, gt, (ref_losses, ref_grads) = model
    if gate == "open":
        monkeypatch.setattr(fused, "UPSAMPLE_RECORD_MIN", dict(ZERO_GATE))
    expect_nodes = EXPECT_NODES[head] - (GATED if gate == "shipped" else set())
    net = copy.deepcopy(cpu_net).to(DEV)
    imgd, gtd = img.to(DEV), gt.to(DEV)
    assert type(net.decode_head).__name__ == head
    monkeypatch.setenv("PPNET_LIBRARY_UPSAMPLE", "1")
    lib_nodes = _recorded({k: v for k, v in net.forward_train(imgd, None, gtd).items() if k.endswith("loss_ce")})
    lib_losses, lib_grads = _model_run(net, imgd, gtd)
    monkeypatch.delenv("PPNET_LIBRARY_UPSAMPLE")
    assert not (lib_nodes & OURS), sorted(lib_nodes & OURS)
    log, real = _capture(monkeypatch)
    nodes = _recorded({k: v for k, v in net.forward_train(imgd, None, gtd).items() if k.endswith("loss_ce")})
    assert nodes & OURS == expect_nodes, (head, gate, sorted(nodes & OURS))
    del log[:]
    losses, grads = _model_run(net, imgd, gtd)
    for k in ("decode", "aux"):
        assert float(losses[f"{k}.loss_ce"]) == pytest.approx(float(lib_losses[f"{k}.loss_ce"]), rel=1e-5)
        assert float(losses[f"{k}.loss_ce"]) == pytest.approx(float(ref_losses[f"{k}.loss_ce"]), rel=1e-4)
    assert set(grads) == set(lib_grads) == set(ref_grads)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert all("decode_head." + n in grads for n, _ in net.decode_head.named_parameters())
    counts = {}
    for e in log:
        counts[e["name"]] = counts.get(e["name"], 0) + 1
    assert counts == EXPECT_CALLS[head], (head, counts)
    assert {e["node"] for e in log} & OURS == expect_nodes
    worst = max(_check_call(e, real) for e in log)
    with capsys.disabled():
        print(f"\n{head} training step, float32, gate {gate}: {len(log)} up-sampling calls, largest gradient error {worst:.3f} of its derived bound", end="")


@pytest.mark.parametrize("gate", ["open", "shipped"])
def test_setr_up_head_trains_on_the_kernels(tiny_model, gate, monkeypatch, capsys):  # noqa: F811
    _head_step("SETRUPHead", tiny_model, gate, monkeypatch, capsys)


@pytest.mark.parametrize("gate", ["open", "shipped"])
@pytest.mark.parametrize("head", ["UPerHead", "UPerPUPHead"])
def test_uper_heads_train_on_the_kernels(head, gate, monkeypatch, capsys):
    _head_step(head, _uper_model(head), gate, monkeypatch, capsys)
