"""CPU-side checks of ppn_gennet_stem_train_workspace / ppn_gennet_stem_train_fwd / ppn_gennet_stem_train_bwd (csrc/gennet_stem_train.hip):
header, library, bindings and the Makefile carry the entry points at ABI 111 with the argument order of the header; the workspace size
follows the header's formula; every bad argument is refused before any HIP call (the pointers below are never dereferenced); the host
constants are the kernels'; the file cross-compiles with the Makefile's flags and no kernel of it uses scratch; the algebra the kernels
implement (gennet.stem_from_moments) equals float64 autograd of conv -> BatchNorm(train) -> LeakyReLU; the gate keeps everything else on
the library; and without a GPU AEViT in train mode is the library composition bit for bit."""
import copy
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ppnet_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
E_INVALID, E_UNSUPPORTED = -1, -3
ONE = C.c_void_p(0x1000)                                       # 16-byte aligned, never dereferenced on these paths
FWD = ["x", "w", "bias", "gamma", "beta", "z", "stats", "moments", "workspace", "B", "H", "W", "C", "eps", "negative_slope", "dtype", "stream"]
BWD = ["dz", "x", "w", "bias", "gamma", "beta", "stats", "moments", "workspace", "dw", "dgamma", "dbeta", "B", "H", "W", "C", "negative_slope",
       "dtype", "stream"]
NAMES = ("ppn_gennet_stem_train_workspace", "ppn_gennet_stem_train_fwd", "ppn_gennet_stem_train_bwd")
CHANNELS = (8, 16, 24, 32)
KERNELS = ("stem_moments_kernel", "stem_stats_kernel", "stem_apply_kernel", "stem_bwd_reduce_kernel", "stem_bwd_finish_kernel")


def _args(decl):
    code = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    return [a.split()[-1].lstrip("*") for a in code.split(",")]


def test_header_library_bindings_and_makefile_carry_the_entry_points_at_abi_111():
    from ppnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "ppnet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    capi = open(os.path.join(CSRC, "capi.hip")).read()
    assert int(re.search(r"#define\s+PPN_ABI_VERSION\s+(\d+)", header).group(1)) == 111
    assert _lib.ABI_VERSION == 111 and _lib.lib.ppn_version() == 111
    version_note = re.search(r"/\* ABI version of this header.*?\*/", header, re.S).group(0)
    for name in NAMES + ("ppn_gennet_stem_train_tile", "ppn_gennet_stem_train_max_blocks"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name) and name in version_note, name
    for name, want in (("ppn_gennet_stem_train_fwd", FWD), ("ppn_gennet_stem_train_bwd", BWD)):
        assert _args(re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, code, re.S).group(1)) == want
        assert _args(re.search(r"\b%s\s*\((.*?)\)\s*\{" % name, capi, re.S).group(1)) == want
        f = getattr(_lib.lib, name)
        assert len(f.argtypes) == len(want) and f.restype is C.c_int
    at = {n: i for i, n in enumerate(FWD)}
    assert _lib.lib.ppn_gennet_stem_train_fwd.argtypes[at["eps"]] is C.c_float
    assert _lib.lib.ppn_gennet_stem_train_fwd.argtypes[at["negative_slope"]] is C.c_float
    assert _lib.lib.ppn_gennet_stem_train_bwd.argtypes[BWD.index("negative_slope")] is C.c_float
    assert _args(re.search(r"int64_t\s+ppn_gennet_stem_train_workspace\s*\((.*?)\)\s*;", code, re.S).group(1)) == ["B", "H", "W", "C"]
    assert _lib.lib.ppn_gennet_stem_train_workspace.restype is C.c_int64
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "gennet_stem_train.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    text = open(os.path.join(CSRC, "gennet_stem_train.hip")).read()
    for kernel in KERNELS:
        assert re.search(r"__global__[^;{]*\b%s\b" % kernel, text), kernel
    assert "atomic" not in text.lower()                                     # one writer per element, fixed-order sums


def test_workspace_follows_the_header_formula():
    from ppnet_amd import _lib, fused
    f = _lib.lib.ppn_gennet_stem_train_workspace
    tile, cap = _lib.lib.ppn_gennet_stem_train_tile(), _lib.lib.ppn_gennet_stem_train_max_blocks()
    for B, H, W, Cc in ((1, 1, 2, 8), (2, 1, 1, 24), (1, 3, 5, 16), (1, 32, 32, 8), (1, 1, 1025, 32), (4, 64, 64, 24), (8, 224, 224, 24),
                        (1, 724, 724, 8), (1, 725, 725, 16), (64, 224, 224, 24), (64, 512, 512, 24)):
        want = max(54 * 8, Cc * 11 * 4) * min(-(-(B * H * W) // tile), cap)
        assert f(B, H, W, Cc) == want == fused.stem_train_workspace_bytes(B, H, W, Cc), (B, H, W, Cc)
    for bad in ((0, 4, 4, 8), (1, 0, 4, 8), (1, 4, 0, 8), (1, 4, 4, 0), (-1, 4, 4, 8), (1, 1, 1, 8), (1, 4, 4, 12), (1, 4, 4, 64), (1, 4, 4, 4),
                (1, 1 << 14, 1 << 14, 8), (1 << 10, 1 << 10, 1 << 8, 8), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 32), (64, 1024, 1024, 32)):
        assert f(*bad) < 0, bad


def _caller(f, ok):
    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    return call


def _common_refusals(call, b):
    """Extents, channel counts and element counts: argument b is B, then H, W, C."""
    for i in range(b, b + 4):
        assert call(**{f"a{i}": 0}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID and call(**{f"a{i}": -(2 ** 31)}) == E_INVALID, i
    for ch in (12, 4, 7, 9, 20, 40, 48, 64, 2 ** 31 - 1):
        assert call(**{f"a{b + 3}": ch}) == E_UNSUPPORTED, ch
    B, H, W, Cc = (f"a{b + k}" for k in range(4))
    assert call(**{B: 1, H: 1, W: 1}) == E_INVALID                                         # one value per channel
    assert call(**{B: 1, H: 1 << 14, W: 1 << 14, Cc: 8}) == E_INVALID                      # 2^31 elements in z
    assert call(**{B: 1 << 10, H: 1 << 10, W: 1 << 8, Cc: 8}) == E_INVALID
    assert call(**{B: 64, H: 1024, W: 1024, Cc: 32}) == E_INVALID
    assert call(**{B: 2 ** 31 - 1, H: 2 ** 31 - 1, W: 2 ** 31 - 1, Cc: 32}) == E_INVALID
    assert call(**{B: 1, H: 1, W: 2 ** 31 - 1, Cc: 8}) == E_INVALID


@pytest.mark.parametrize("dtype", [0, 1])
def test_forward_rejects_bad_arguments_without_gpu(dtype):
    from ppnet_amd import _lib
    #                                                    9 pointers  B  H  W  C   eps   slope dtype  stream
    call = _caller(_lib.lib.ppn_gennet_stem_train_fwd, [ONE] * 9 + [2, 7, 5, 24, 1e-5, 0.01, dtype, None])
    at = {n: i for i, n in enumerate(FWD)}
    for n in ("x", "w", "gamma", "beta", "z", "stats", "moments", "workspace"):            # bias may be NULL, the others not
        assert call(**{f"a{at[n]}": None}) == E_INVALID, n
        assert call(**{f"a{at[n]}": None, f"a{at['bias']}": None}) == E_INVALID, n
    for n in ("x", "w", "bias", "gamma", "beta", "z", "workspace"):                         # 16 bytes
        for off in (8, 4, 2, 1):
            assert call(**{f"a{at[n]}": C.c_void_p(0x1000 + off)}) == E_INVALID, (n, off)
    for off in (4, 2, 1):                                                                  # moments: 8 bytes
        assert call(**{f"a{at['moments']}": C.c_void_p(0x1000 + off)}) == E_INVALID, off
    for off in (2, 1, 3):                                                                  # stats: 4 bytes
        assert call(**{f"a{at['stats']}": C.c_void_p(0x1000 + off)}) == E_INVALID, off
    _common_refusals(call, at["B"])
    for n in ("eps", "negative_slope"):
        for v in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
            assert call(**{f"a{at[n]}": v}) == E_INVALID, (n, v)
    for d in (2, -1, 7):
        assert call(**{f"a{at['dtype']}": d}) == E_INVALID, d


@pytest.mark.parametrize("dtype", [0, 1])
def test_backward_rejects_bad_arguments_without_gpu(dtype):
    from ppnet_amd import _lib
    #                                                    12 pointers  B  H  W  C   slope dtype  stream
    call = _caller(_lib.lib.ppn_gennet_stem_train_bwd, [ONE] * 12 + [2, 7, 5, 24, 0.01, dtype, None])
    at = {n: i for i, n in enumerate(BWD)}
    for n in ("dz", "x", "w", "gamma", "beta", "stats", "moments", "workspace", "dw", "dgamma", "dbeta"):
        assert call(**{f"a{at[n]}": None}) == E_INVALID, n
        assert call(**{f"a{at[n]}": None, f"a{at['bias']}": None}) == E_INVALID, n
    for n in ("dz", "x", "w", "bias", "gamma", "beta", "workspace", "dw", "dgamma", "dbeta"):
        for off in (8, 4, 2, 1):
            assert call(**{f"a{at[n]}": C.c_void_p(0x1000 + off)}) == E_INVALID, (n, off)
    for off in (4, 2, 1):
        assert call(**{f"a{at['moments']}": C.c_void_p(0x1000 + off)}) == E_INVALID, off
    for off in (2, 1, 3):
        assert call(**{f"a{at['stats']}": C.c_void_p(0x1000 + off)}) == E_INVALID, off
    _common_refusals(call, at["B"])
    for v in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        assert call(**{f"a{at['negative_slope']}": v}) == E_INVALID, v
    for d in (2, -1, 7):
        assert call(**{f"a{at['dtype']}": d}) == E_INVALID, d


def test_host_constants_are_the_kernels():
    from ppnet_amd import _lib, fused
    src = open(os.path.join(CSRC, "gennet_stem_train.hip")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr int (ST_\w+) = (\d+);", src)}
    assert const["ST_THREADS"] == fused.STEM_THREADS == 256
    assert const["ST_PPT"] == fused.STEM_LINE == 4
    assert const["ST_TILE"] == fused.STEM_TILE == _lib.lib.ppn_gennet_stem_train_tile() == const["ST_THREADS"] * const["ST_PPT"]
    assert const["ST_MAX_BLOCKS"] == fused.STEM_MAX_BLOCKS == _lib.lib.ppn_gennet_stem_train_max_blocks() == 512
    assert const["ST_MOMENTS"] == fused.STEM_MOMENTS == 54 and const["ST_SUMS"] == fused.STEM_SUMS == 11
    assert all(c % const["ST_FWD_CH"] == 0 and c % const["ST_BWD_CH"] == 0 for c in CHANNELS)
    assert fused.STEM_CHANNELS == frozenset(CHANNELS)
    for ch in range(0, 70):
        assert (_lib.lib.ppn_gennet_stem_train_workspace(2, 4, 4, ch) > 0) == (ch in CHANNELS), ch
    assert fused.STEM_CALLS.keys() == {"fwd", "bwd"}
    kernels_h = open(os.path.join(CSRC, "ppn_kernels.h")).read()
    for name in ("gennet_stem_channels_ok", "gennet_stem_tile", "gennet_stem_max_blocks", "gennet_stem_train_workspace_bytes",
                 "gennet_stem_train_fwd_launch", "gennet_stem_train_bwd_launch"):
        assert re.search(r"\b%s\s*\(" % name, kernels_h), name


def test_stem_source_is_built_and_uses_no_scratch(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not present")
    out = tmp_path / "gennet_stem_train.s"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize --cuda-device-only -S".split()
    for fl in flags[:-2]:
        assert fl.replace("gfx950", "$(ARCH)") in mk, fl                            # the Makefile's own flags
    subprocess.run([HIPCC, *flags, os.path.join(CSRC, "gennet_stem_train.hip"), "-o", str(out)], check=True, cwd=CSRC, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    scratch = dict(re.findall(r"\.amdhsa_kernel (\S+).*?; ScratchSize: (\d+)", out.read_text(), re.S))
    # moments, statistics and the backward's finish once; apply and the backward's sums for float32 and bfloat16
    assert len(scratch) == 7, scratch
    for kernel, n in zip(KERNELS, (1, 1, 2, 2, 1)):
        assert sum(kernel in k for k in scratch) == n, kernel
    assert all(int(v) == 0 for v in scratch.values()), scratch


# ------------------------------------------------------------------------------------------------------------------------- the algebra
ALGEBRA = [((2, 8, 8, 24), "binary"), ((1, 3, 5, 16), "gauss"), ((1, 1, 2, 8), "gauss"), ((3, 1, 9, 32), "gauss"), ((4, 64, 64, 24), "offset")]


def _float64_case(shape, kind, seed):
    import torch
    B, H, W, Cc = shape
    g = torch.Generator().manual_seed(seed)
    if kind == "binary":
        x = (torch.rand(B, 1, H, W, generator=g, dtype=torch.float64) < 0.5).double()
    else:
        x = torch.randn(B, 1, H, W, generator=g, dtype=torch.float64)
        if kind == "offset":
            x = 5.0 + 3.0 * x
    w = 0.3 * torch.randn(Cc, 1, 3, 3, generator=g, dtype=torch.float64)
    b = 0.1 * torch.randn(Cc, generator=g, dtype=torch.float64)
    gamma = 1.0 + 0.1 * torch.randn(Cc, generator=g, dtype=torch.float64)
    beta = 0.1 * torch.randn(Cc, generator=g, dtype=torch.float64)
    dz = torch.randn(B, Cc, H, W, generator=g, dtype=torch.float64)
    return x, dz, w, b, gamma, beta


@pytest.mark.parametrize("slope", [0.01, 0.0, 1.0])
@pytest.mark.parametrize("shape,kind", ALGEBRA)
def test_stem_from_moments_is_float64_autograd_of_the_composition(shape, kind, slope):
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F
    from ppnet_amd import gennet
    x, dz, w, b, gamma, beta = _float64_case(shape, kind, 17 + shape[1] * shape[2])
    ps = [t.clone().requires_grad_(True) for t in (w, b, gamma, beta)]
    y = F.conv2d(x, ps[0], ps[1], padding=1)
    z_ref = F.leaky_relu(F.batch_norm(y, None, None, ps[2], ps[3], training=True, eps=1e-5), slope)
    dw_ref, db_ref, dg_ref, dbeta_ref = torch.autograd.grad(z_ref, ps, dz)
    ref = (z_ref.detach(), y.detach().mean((0, 2, 3)), y.detach().var((0, 2, 3), unbiased=False), dw_ref, dg_ref, dbeta_ref)
    got = gennet.stem_from_moments(x, dz, w, b, gamma, beta, 1e-5, slope)
    assert all(t.dtype == torch.float64 for t in got)
    for name, a, r in zip(("z", "mean", "var", "dW", "dgamma", "dbeta"), got, ref):
        assert a.shape == r.shape, name
        err, top = (a - r).abs().max().item(), r.abs().max().item()
        assert err <= 1e-12 * top, (name, shape, slope, err, top)
    assert db_ref.abs().max().item() < 1e-9 * dw_ref.abs().max().item()            # the bias gradient the kernels never form is 0
    # the forms the wrapper passes: x without its channel axis, w as [C][9], no bias
    got2 = gennet.stem_from_moments(x[:, 0], dz, w.reshape(-1, 9), None, gamma, beta, 1e-5, slope)
    want2 = gennet.stem_from_moments(x, dz, w, torch.zeros_like(b), gamma, beta, 1e-5, slope)
    assert all(torch.equal(a.reshape(-1), r.reshape(-1)) for a, r in zip(got2, want2))


# ---------------------------------------------------------------------------------------------------------------------------- the gate
def _fake_cuda(torch, *shape, requires_grad=False, dtype=None, contiguous=True):
    class Fake:                                                                            # what the predicate reads of a CUDA tensor
        is_cuda, device = True, torch.device("cpu")

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return contiguous
    f = Fake()
    f.shape, f.requires_grad, f.dtype = shape, requires_grad, dtype or torch.float32
    return f


def test_gate_keeps_everything_else_on_the_library(monkeypatch):
    torch = pytest.importorskip("torch")
    nn = torch.nn
    from ppnet_amd import fused
    monkeypatch.delenv("PPNET_LIBRARY_STEM", raising=False)
    ok = fused.stem_train_ok
    conv, bn = nn.Conv2d(1, 24, 3, 1, 1), nn.BatchNorm2d(24)
    x = _fake_cuda(torch, 2, 1, 8, 8)
    assert ok(x, conv, bn)                                                                 # what a CUDA training step presents
    for ch in (8, 16, 32):
        assert ok(x, nn.Conv2d(1, ch, 3, 1, 1), nn.BatchNorm2d(ch)), ch
    assert ok(x, nn.Conv2d(1, 24, 3, 1, 1, bias=False), bn)
    assert ok(_fake_cuda(torch, 1, 1, 1, 2), conv, bn)
    assert not ok(torch.rand(2, 1, 8, 8), conv, bn)                                        # a CPU tensor
    assert not ok(_fake_cuda(torch, 2, 1, 8, 8, requires_grad=True), conv, bn)             # the input gradient is the library's
    assert not ok(_fake_cuda(torch, 2, 1, 8, 8, dtype=torch.bfloat16), conv, bn)
    assert not ok(_fake_cuda(torch, 2, 1, 8, 8, contiguous=False), conv, bn)
    assert not ok(_fake_cuda(torch, 1, 1, 1, 1), conv, bn)                                 # torch's own ValueError must come from torch
    assert not ok(_fake_cuda(torch, 2, 2, 8, 8), nn.Conv2d(2, 24, 3, 1, 1), bn)            # a 2-channel input
    assert not ok(_fake_cuda(torch, 2, 2, 8, 8), conv, bn)
    assert not ok(_fake_cuda(torch, 1 << 10, 1, 1 << 10, 1 << 8), nn.Conv2d(1, 8, 3, 1, 1), nn.BatchNorm2d(8))   # 2^31 outputs
    assert not ok(x, nn.Conv2d(1, 12, 3, 1, 1), nn.BatchNorm2d(12))                        # C = 12
    for other in (nn.Conv2d(1, 24, 3, 2, 1), nn.Conv2d(1, 24, 3, 1, 2, dilation=2), nn.Conv2d(1, 24, 5, 1, 2), nn.Conv2d(1, 24, 3, 1, 0),
                  nn.Conv2d(1, 24, 3, 1, 1, padding_mode="reflect"), nn.Conv2d(1, 24, 3, 1, 1).double(), nn.ConvTranspose2d(1, 24, 3, 1, 1)):
        assert not ok(x, other, bn), other
    assert not ok(x, conv, nn.BatchNorm2d(24).eval())                                      # eval mode: running statistics
    assert not ok(x, conv, nn.SyncBatchNorm(24))                                           # reduces over ranks
    assert not ok(x, conv, nn.BatchNorm2d(24, affine=False))
    assert not ok(x, conv, nn.BatchNorm2d(24, track_running_stats=False))
    assert not ok(x, conv, nn.BatchNorm2d(24, momentum=None))
    assert not ok(x, conv, nn.BatchNorm2d(16))
    assert not ok(x, conv, nn.Identity())
    with torch.no_grad():
        assert not ok(x, conv, bn)                                                         # nothing records
    frozen_c, frozen_b = nn.Conv2d(1, 24, 3, 1, 1).requires_grad_(False), nn.BatchNorm2d(24).requires_grad_(False)
    assert not ok(x, frozen_c, frozen_b) and ok(x, frozen_c, bn)
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: torch.float16)
    assert not ok(x, conv, bn)                                                             # float16 autocast keeps the library
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: torch.bfloat16)
    assert ok(x, conv, bn)
    monkeypatch.undo()
    monkeypatch.setenv("PPNET_LIBRARY_STEM", "1")
    assert not ok(x, conv, bn)


def test_cpu_aevit_training_is_the_library_composition_bit_for_bit(monkeypatch):
    """Without a GPU the gate is false: AEViT in train mode gives the output and the running statistics of the stem written out with
    F.conv2d, F.batch_norm and F.leaky_relu, and no launch is counted."""
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F
    from ppnet_amd import fused, gennet
    monkeypatch.delenv("PPNET_LIBRARY_STEM", raising=False)
    torch.manual_seed(3)
    m = gennet.AEViT(1, 1, 64, 24).train()
    for blk in m.vit_blocks:
        blk.drop_path_rate = 0.0
    ref = copy.deepcopy(m)

    class WrittenOut(torch.nn.Module):
        def __init__(self, stage):
            super().__init__()
            self.conv, self.bn, self.slope = stage[0], stage[1], stage[2].negative_slope

        def forward(self, x):
            c, bn = self.conv, self.bn
            bn.num_batches_tracked.add_(1)
            y = F.conv2d(x, c.weight, c.bias, stride=1, padding=1)
            y = F.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, training=True, momentum=bn.momentum, eps=bn.eps)
            return F.leaky_relu(y, self.slope)
    written = WrittenOut(ref.conv_first)
    ref.conv_first = written
    calls = dict(fused.STEM_CALLS)
    x = (torch.rand(2, 1, 64, 64) < 0.5).float()
    assert not fused.stem_train_ok(x, m.conv_first[0], m.conv_first[1])
    for _ in range(2):
        a, b = m(x), ref(x)
        assert torch.equal(a, b)
    bn = m.conv_first[1]
    assert torch.equal(bn.running_mean, written.bn.running_mean) and torch.equal(bn.running_var, written.bn.running_var)
    assert int(bn.num_batches_tracked) == int(written.bn.num_batches_tracked) == 2
    assert not torch.equal(bn.running_mean, torch.zeros(24))
    assert fused.STEM_CALLS == calls
    assert sorted(k for k in m.state_dict() if k.startswith("conv_first.")) == [
        "conv_first.0.bias", "conv_first.0.weight", "conv_first.1.bias", "conv_first.1.num_batches_tracked", "conv_first.1.running_mean",
        "conv_first.1.running_var", "conv_first.1.weight"]
