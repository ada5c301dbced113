"""CPU-side checks of ppn_gennet_tail_train_workspace / ppn_gennet_tail_train_fwd / ppn_gennet_tail_train_bwd (csrc/gennet_tail_train.hip):
header, library, bindings and the Makefile carry the entry points at ABI 111 with the argument order of the header; the workspace size
follows the header's formula; every bad argument is refused before any HIP call (the pointers below are never dereferenced); the host
constants are the kernels'; the file cross-compiles with the Makefile's flags and no kernel of it uses scratch; the algebra the kernels
implement (gennet.tail_from_sums) equals float64 autograd of BatchNorm(train) -> LeakyReLU -> conv; the gate keeps everything else on the
library; and without a GPU AEViT in train mode is the library composition bit for bit."""
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
FWD = ["y", "gamma", "beta", "wf", "bf", "out", "stats", "workspace", "B", "H", "W", "C", "eps", "negative_slope", "dtype", "stream"]
BWD = ["dout", "y", "gamma", "beta", "wf", "stats", "workspace", "dy", "dgamma", "dbeta", "dwf", "dbf", "B", "H", "W", "C", "negative_slope",
       "dtype", "stream"]
NAMES = ("ppn_gennet_tail_train_workspace", "ppn_gennet_tail_train_fwd", "ppn_gennet_tail_train_bwd")
CHANNELS = (8, 16, 24, 32)
KERNELS = ("tail_stats_kernel", "tail_stats_finish_kernel", "tail_apply_kernel", "tail_bwd_reduce_kernel", "tail_bwd_finish_kernel",
           "tail_bwd_apply_kernel")


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
    for name in NAMES + ("ppn_gennet_tail_train_tile", "ppn_gennet_tail_train_max_blocks"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name) and name in version_note, name
    for name, want in (("ppn_gennet_tail_train_fwd", FWD), ("ppn_gennet_tail_train_bwd", BWD)):
        assert _args(re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, code, re.S).group(1)) == want
        assert _args(re.search(r"\b%s\s*\((.*?)\)\s*\{" % name, capi, re.S).group(1)) == want
        f = getattr(_lib.lib, name)
        assert len(f.argtypes) == len(want) and f.restype is C.c_int
    at = {n: i for i, n in enumerate(FWD)}
    assert _lib.lib.ppn_gennet_tail_train_fwd.argtypes[at["eps"]] is C.c_float
    assert _lib.lib.ppn_gennet_tail_train_fwd.argtypes[at["negative_slope"]] is C.c_float
    assert _lib.lib.ppn_gennet_tail_train_bwd.argtypes[BWD.index("negative_slope")] is C.c_float
    assert _args(re.search(r"int64_t\s+ppn_gennet_tail_train_workspace\s*\((.*?)\)\s*;", code, re.S).group(1)) == ["B", "H", "W", "C"]
    assert _lib.lib.ppn_gennet_tail_train_workspace.restype is C.c_int64
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "gennet_tail_train.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    text = open(os.path.join(CSRC, "gennet_tail_train.hip")).read()
    for kernel in KERNELS:
        assert re.search(r"__global__[^;{]*\b%s\b" % kernel, text), kernel
    code_only = re.sub(r"//[^\n]*", "", text)
    assert "atomic" not in code_only.lower()                                # one writer per element, fixed-order sums
    assert len(re.findall(r"\btl_preact\s*\(", code_only)) >= 4 and "fmaf(cf[11], xh, cf[12])" in code_only   # ONE pre-activation function


def test_workspace_follows_the_header_formula():
    from ppnet_amd import _lib, fused
    f = _lib.lib.ppn_gennet_tail_train_workspace
    tile, cap = _lib.lib.ppn_gennet_tail_train_tile(), _lib.lib.ppn_gennet_tail_train_max_blocks()
    for B, H, W, Cc in ((1, 1, 2, 8), (2, 1, 1, 24), (1, 3, 5, 16), (1, 32, 32, 8), (1, 1, 1025, 32), (4, 64, 64, 24), (8, 224, 224, 24),
                        (1, 724, 724, 8), (1, 725, 725, 16), (64, 224, 224, 24), (64, 512, 512, 24)):
        want = max(Cc * 2 * 8, (Cc * 11 + 1) * 4) * min(-(-(B * H * W) // tile), cap)
        assert f(B, H, W, Cc) == want == fused.tail_train_workspace_bytes(B, H, W, Cc), (B, H, W, Cc)
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
    assert call(**{B: 1, H: 1 << 14, W: 1 << 14, Cc: 8}) == E_INVALID                      # 2^31 elements in y
    assert call(**{B: 1 << 10, H: 1 << 10, W: 1 << 8, Cc: 8}) == E_INVALID
    assert call(**{B: 64, H: 1024, W: 1024, Cc: 32}) == E_INVALID
    assert call(**{B: 2 ** 31 - 1, H: 2 ** 31 - 1, W: 2 ** 31 - 1, Cc: 32}) == E_INVALID
    assert call(**{B: 1, H: 1, W: 2 ** 31 - 1, Cc: 8}) == E_INVALID


@pytest.mark.parametrize("dtype", [0, 1])
def test_forward_rejects_bad_arguments_without_gpu(dtype):
    from ppnet_amd import _lib
    #                                                    8 pointers  B  H  W  C   eps   slope dtype  stream
    call = _caller(_lib.lib.ppn_gennet_tail_train_fwd, [ONE] * 8 + [2, 7, 5, 24, 1e-5, 0.01, dtype, None])
    at = {n: i for i, n in enumerate(FWD)}
    for n in ("y", "gamma", "beta", "wf", "out", "stats", "workspace"):                    # bf may be NULL, the others not
        assert call(**{f"a{at[n]}": None}) == E_INVALID, n
        assert call(**{f"a{at[n]}": None, f"a{at['bf']}": None}) == E_INVALID, n
    for n in ("y", "gamma", "beta", "wf", "out", "workspace"):                             # 16 bytes
        for off in (8, 4, 2, 1):
            assert call(**{f"a{at[n]}": C.c_void_p(0x1000 + off)}) == E_INVALID, (n, off)
    for n in ("stats", "bf"):                                                              # 4 bytes
        for off in (2, 1, 3):
            assert call(**{f"a{at[n]}": C.c_void_p(0x1000 + off)}) == E_INVALID, (n, off)
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
    call = _caller(_lib.lib.ppn_gennet_tail_train_bwd, [ONE] * 12 + [2, 7, 5, 24, 0.01, dtype, None])
    at = {n: i for i, n in enumerate(BWD)}
    for n in ("dout", "y", "gamma", "beta", "wf", "stats", "workspace", "dgamma", "dbeta", "dwf"):     # dy and dbf may be NULL
        assert call(**{f"a{at[n]}": None}) == E_INVALID, n
        assert call(**{f"a{at[n]}": None, f"a{at['dy']}": None, f"a{at['dbf']}": None}) == E_INVALID, n
    for n in ("dout", "y", "gamma", "beta", "wf", "workspace", "dy", "dgamma", "dbeta", "dwf"):
        for off in (8, 4, 2, 1):
            assert call(**{f"a{at[n]}": C.c_void_p(0x1000 + off)}) == E_INVALID, (n, off)
    for n in ("stats", "dbf"):
        for off in (2, 1, 3):
            assert call(**{f"a{at[n]}": C.c_void_p(0x1000 + off)}) == E_INVALID, (n, off)
    _common_refusals(call, at["B"])
    for v in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        assert call(**{f"a{at['negative_slope']}": v}) == E_INVALID, v
    for d in (2, -1, 7):
        assert call(**{f"a{at['dtype']}": d}) == E_INVALID, d
    # dy = NULL and dbf = NULL are no refusals of their own: the extents still decide
    assert call(**{f"a{at['dy']}": None, f"a{at['dbf']}": None, f"a{at['C']}": 12}) == E_UNSUPPORTED


def test_host_constants_are_the_kernels():
    from ppnet_amd import _lib, fused
    src = open(os.path.join(CSRC, "gennet_tail_train.hip")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr int (TL_\w+) = (\d+);", src)}
    assert const["TL_THREADS"] == fused.TAIL_THREADS == 256
    assert const["TL_PPT"] == fused.TAIL_LINE == 4
    assert const["TL_TILE"] == fused.TAIL_TILE == _lib.lib.ppn_gennet_tail_train_tile() == const["TL_THREADS"] * const["TL_PPT"]
    assert const["TL_MAX_BLOCKS"] == fused.TAIL_MAX_BLOCKS == _lib.lib.ppn_gennet_tail_train_max_blocks() == 512
    assert const["TL_SUMS"] == fused.TAIL_SUMS == 11
    assert all(c % const["TL_STAT_CH"] == 0 and c % const["TL_BWD_CH"] == 0 and c % const["TL_DY_CH"] == 0 and c <= const["TL_MAX_CH"]
               for c in CHANNELS)
    assert 2 * const["TL_MAX_CH"] <= 64                                       # the statistics' finishing step: 64 columns
    assert fused.TAIL_CHANNELS == frozenset(CHANNELS)
    for ch in range(0, 70):
        assert (_lib.lib.ppn_gennet_tail_train_workspace(2, 4, 4, ch) > 0) == (ch in CHANNELS), ch
    assert fused.TAIL_CALLS.keys() == {"fwd", "bwd"}
    assert isinstance(fused.TAIL_RECORD_MIN, int) and fused.TAIL_RECORD_MIN >= 0
    kernels_h = open(os.path.join(CSRC, "ppn_kernels.h")).read()
    for name in ("gennet_tail_channels_ok", "gennet_tail_tile", "gennet_tail_max_blocks", "gennet_tail_train_workspace_bytes",
                 "gennet_tail_train_fwd_launch", "gennet_tail_train_bwd_launch"):
        assert re.search(r"\b%s\s*\(" % name, kernels_h), name


def test_tail_source_is_built_and_uses_no_scratch(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not present")
    out = tmp_path / "gennet_tail_train.s"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize --cuda-device-only -S".split()
    for fl in flags[:-2]:
        assert fl.replace("gfx950", "$(ARCH)") in mk, fl                            # the Makefile's own flags
    subprocess.run([HIPCC, *flags, os.path.join(CSRC, "gennet_tail_train.hip"), "-o", str(out)], check=True, cwd=CSRC, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    scratch = dict(re.findall(r"\.amdhsa_kernel (\S+).*?; ScratchSize: (\d+)", out.read_text(), re.S))
    # the two finishing steps once; statistics, apply, the backward's sums and the backward's apply for float32 and bfloat16
    assert len(scratch) == 10, scratch
    for kernel, n in zip(KERNELS, (2, 1, 2, 2, 1, 2)):
        assert sum(re.search(r"\d+%s[A-Z]" % kernel, k) is not None for k in scratch) == n, kernel
    assert all(int(v) == 0 for v in scratch.values()), scratch


# ------------------------------------------------------------------------------------------------------------------------- the algebra
ALGEBRA = [(1, 1, 2, 8), (2, 1, 1, 24), (1, 3, 5, 16), (2, 9, 7, 24), (4, 64, 64, 24)]
OUTPUTS = ("out", "mean", "var", "dy", "dgamma", "dbeta", "dWf", "dbf")


def _float64_case(shape, seed=0):
    """The construction of the GPU tests (tests/test_gpu_tail_train.py), widened to float64: default-initialised BatchNorm2d and Conv2d
    under torch.manual_seed(seed) plus 0.1 randn on gamma, beta and b_f; from Generator(seed + 100) y in quarter steps,
    clamp(round(4 (0.5 + 1.5 randn)) / 4, -8, 8), then the upstream gradient rounded to bfloat16.  With two values per channel dy is a
    difference of nearly equal terms (it vanishes with eps), so its own maximum is a demanding scale there."""
    import torch
    B, H, W, Cc = shape
    torch.manual_seed(seed)
    bn, conv = torch.nn.BatchNorm2d(Cc), torch.nn.Conv2d(Cc, 1, 3, 1, 1)
    with torch.no_grad():
        for p in (bn.weight, bn.bias, conv.bias):
            p.add_(0.1 * torch.randn_like(p))
    g = torch.Generator().manual_seed(seed + 100)
    y = (torch.round(4 * (0.5 + 1.5 * torch.randn(B, Cc, H, W, generator=g))) / 4).clamp(-8, 8)
    d = torch.randn(B, 1, H, W, generator=g).to(torch.bfloat16)
    return [t.detach().double() for t in (y, d, bn.weight, bn.bias, conv.weight, conv.bias)]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("slope", [0.01, 0.0, 1.0])
@pytest.mark.parametrize("shape", ALGEBRA)
def test_tail_from_sums_is_float64_autograd_of_the_composition(shape, slope, bias):
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F
    from ppnet_amd import gennet
    y, d, gamma, beta, wf, bf = _float64_case(shape)
    leaves = [t.clone().requires_grad_(True) for t in ((y, gamma, beta, wf, bf) if bias else (y, gamma, beta, wf))]
    z = F.leaky_relu(F.batch_norm(leaves[0], None, None, leaves[1], leaves[2], training=True, eps=1e-5), slope)
    out_ref = F.conv2d(z, leaves[3], leaves[4] if bias else None, padding=1)
    grads = torch.autograd.grad(out_ref, leaves, d)
    ref = (out_ref.detach(), y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False), grads[0], grads[1], grads[2], grads[3],
           grads[4] if bias else None)
    got = gennet.tail_from_sums(y, d, gamma, beta, wf, bf if bias else None, 1e-5, slope)
    assert len(got) == len(OUTPUTS) and (got[7] is None) == (not bias)
    for name, a, r in zip(OUTPUTS, got, ref):
        if r is None:
            continue
        assert a.dtype == torch.float64 and a.shape == r.shape, name
        err, top = (a - r).abs().max().item(), r.abs().max().item()
        assert err <= 1e-12 * top, (name, shape, slope, err, top)
    # the form the wrapper passes: wf as [C][9]
    got2 = gennet.tail_from_sums(y, d, gamma, beta, wf.reshape(-1, 9), bf if bias else None, 1e-5, slope)
    assert all(torch.equal(a.reshape(-1), r.reshape(-1)) for a, r in zip(got2, got) if r is not None)


def test_tail_from_sums_pads_z_with_zeros_and_keeps_a_constant_plane_exact():
    """y constant per channel (c / 4): mean is it and var is 0 exactly; a halo pixel of z is 0, not leaky(beta): out is b_f plus
    leaky(beta_c) times the sum of the taps that fall inside the image."""
    torch = pytest.importorskip("torch")
    from ppnet_amd import gennet
    B, Cc, H, W = 2, 8, 5, 6
    y = (torch.arange(Cc, dtype=torch.float64) / 4).view(1, Cc, 1, 1).expand(B, Cc, H, W).contiguous()
    _, d, gamma, beta, wf, bf = _float64_case((B, H, W, Cc))
    out, mean, var = gennet.tail_from_sums(y, d, gamma, beta, wf, bf, 1e-5, 0.01)[:3]
    assert torch.equal(mean, torch.arange(Cc, dtype=torch.float64) / 4) and bool((var == 0).all())
    lb = torch.where(beta > 0, beta, beta * 0.01)
    for h, w in ((0, 0), (0, 3), (H - 1, W - 1), (2, 0), (2, 3)):
        inside = torch.tensor([[0 <= h + r - 1 < H and 0 <= w + j - 1 < W for j in range(3)] for r in range(3)], dtype=torch.float64)
        want = bf[0] + (lb * (wf[0] * inside).sum((1, 2))).sum()
        assert abs(out[1, 0, h, w].item() - want.item()) <= 1e-14 * max(1.0, abs(want.item())), (h, w)


# ---------------------------------------------------------------------------------------------------------------------------- the gate
def _fake_cuda(torch, *shape, requires_grad=True, dtype=None, contiguous=True):
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
    monkeypatch.delenv("PPNET_LIBRARY_TAIL", raising=False)
    monkeypatch.setattr(fused, "TAIL_RECORD_MIN", 0)
    ok = fused.tail_train_ok
    bn, conv = nn.BatchNorm2d(24), nn.Conv2d(24, 1, 3, 1, 1)
    y = _fake_cuda(torch, 2, 24, 8, 8)
    assert ok(y, bn, conv)                                                                 # what a CUDA training step presents
    for ch in (8, 16, 32):
        assert ok(_fake_cuda(torch, 2, ch, 8, 8), nn.BatchNorm2d(ch), nn.Conv2d(ch, 1, 3, 1, 1)), ch
    assert ok(y, bn, nn.Conv2d(24, 1, 3, 1, 1, bias=False))
    assert ok(_fake_cuda(torch, 1, 24, 1, 2), bn, conv)
    assert ok(_fake_cuda(torch, 2, 24, 8, 8, requires_grad=False), bn, conv)               # a parameter still records
    assert not ok(torch.rand(2, 24, 8, 8), bn, conv)                                       # a CPU tensor
    assert not ok(_fake_cuda(torch, 2, 24, 8, 8, dtype=torch.bfloat16), bn, conv)          # bfloat16 y outside autocast: the library refuses it
    assert not ok(_fake_cuda(torch, 2, 24, 8, 8, dtype=torch.float16), bn, conv)
    assert not ok(_fake_cuda(torch, 2, 24, 8, 8, dtype=torch.float64), bn, conv)
    assert not ok(_fake_cuda(torch, 2, 24, 8, 8, contiguous=False), bn, conv)
    assert not ok(_fake_cuda(torch, 1, 24, 1, 1), bn, conv)                                # torch's own ValueError must come from torch
    assert not ok(_fake_cuda(torch, 24, 8, 8), bn, conv)
    assert not ok(_fake_cuda(torch, 1 << 10, 8, 1 << 10, 1 << 8), nn.BatchNorm2d(8), nn.Conv2d(8, 1, 3, 1, 1))    # 2^31 elements
    assert not ok(_fake_cuda(torch, 2, 12, 8, 8), nn.BatchNorm2d(12), nn.Conv2d(12, 1, 3, 1, 1))                  # C = 12
    for other in (nn.Conv2d(24, 2, 3, 1, 1), nn.Conv2d(24, 24, 3, 1, 1), nn.Conv2d(16, 1, 3, 1, 1), nn.Conv2d(24, 1, 3, 2, 1),
                  nn.Conv2d(24, 1, 3, 1, 2, dilation=2), nn.Conv2d(24, 1, 5, 1, 2), nn.Conv2d(24, 1, 3, 1, 0), nn.Conv2d(24, 1, 1, 1, 0),
                  nn.Conv2d(24, 1, 3, 1, 1, padding_mode="reflect"), nn.Conv2d(24, 1, 3, 1, 1).double(), nn.ConvTranspose2d(24, 1, 3, 1, 1),
                  nn.Identity()):
        assert not ok(y, bn, other), other
    assert not ok(y, nn.BatchNorm2d(24).eval(), conv)                                      # eval mode: running statistics
    assert not ok(y, nn.SyncBatchNorm(24), conv)                                           # reduces over ranks

    class Sub(nn.BatchNorm2d):
        pass
    assert not ok(y, Sub(24), conv)                                                        # any subclass
    assert not ok(y, nn.BatchNorm2d(24, affine=False), conv)
    assert not ok(y, nn.BatchNorm2d(24, track_running_stats=False), conv)
    assert not ok(y, nn.BatchNorm2d(24, momentum=None), conv)
    assert not ok(y, nn.BatchNorm2d(16), conv)
    assert not ok(y, nn.BatchNorm2d(24).double(), conv)
    assert not ok(y, nn.Identity(), conv)
    with torch.no_grad():
        assert not ok(y, bn, conv)                                                         # nothing records
    frozen_b, frozen_c = nn.BatchNorm2d(24).requires_grad_(False), nn.Conv2d(24, 1, 3, 1, 1).requires_grad_(False)
    still = _fake_cuda(torch, 2, 24, 8, 8, requires_grad=False)
    assert not ok(still, frozen_b, frozen_c) and ok(still, frozen_b, conv) and ok(y, frozen_b, frozen_c)
    monkeypatch.setattr(fused, "TAIL_RECORD_MIN", 2 * 24 * 8 * 8 + 1)
    assert not ok(y, bn, conv)                                                             # below the recorded crossover
    monkeypatch.setattr(fused, "TAIL_RECORD_MIN", 2 * 24 * 8 * 8)
    assert ok(y, bn, conv)
    monkeypatch.setattr(fused, "TAIL_RECORD_MIN", 0)
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: torch.float16)
    assert not ok(y, bn, conv)                                                             # float16 autocast keeps the library
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: torch.bfloat16)
    assert ok(y, bn, conv) and ok(_fake_cuda(torch, 2, 24, 8, 8, dtype=torch.bfloat16), bn, conv)
    monkeypatch.undo()
    monkeypatch.setenv("PPNET_LIBRARY_TAIL", "1")
    assert not ok(y, bn, conv)


def test_cpu_aevit_training_is_the_library_composition_bit_for_bit(monkeypatch):
    """Without a GPU the gate is false: AEViT in train mode gives the output and the running statistics of the tail written out with
    F.conv_transpose2d, F.batch_norm, F.leaky_relu and F.conv2d, and no launch is counted.  A resolution below 56 has no decoder stage."""
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F
    from ppnet_amd import fused, gennet
    monkeypatch.delenv("PPNET_LIBRARY_TAIL", raising=False)
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
            y = F.conv_transpose2d(x, c.weight, c.bias, stride=2, padding=1, output_padding=1)
            y = F.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, training=True, momentum=bn.momentum, eps=bn.eps)
            return F.leaky_relu(y, self.slope)
    written = WrittenOut(ref.dec_conv[-1])
    ref.dec_conv[-1] = written
    calls = dict(fused.TAIL_CALLS)
    x = (torch.rand(2, 1, 64, 64) < 0.5).float()
    for _ in range(2):
        a, b = m(x), ref(x)
        assert torch.equal(a, b)
    a.sum().backward()
    b.sum().backward()
    assert torch.equal(m.conv_final.weight.grad, ref.conv_final.weight.grad)
    assert torch.equal(m.dec_conv[-1][1].weight.grad, written.bn.weight.grad) and torch.equal(m.conv_first[0].weight.grad, ref.conv_first[0].weight.grad)
    bn = m.dec_conv[-1][1]
    assert torch.equal(bn.running_mean, written.bn.running_mean) and torch.equal(bn.running_var, written.bn.running_var)
    assert int(bn.num_batches_tracked) == int(written.bn.num_batches_tracked) == 2
    assert not torch.equal(bn.running_mean, torch.zeros(24))
    assert fused.TAIL_CALLS == calls
    keys = sorted(k for k in m.state_dict() if k.startswith("dec_conv.") or k.startswith("conv_final."))
    assert keys == ["conv_final.bias", "conv_final.weight", "dec_conv.0.0.bias", "dec_conv.0.0.weight", "dec_conv.0.1.bias",
                    "dec_conv.0.1.num_batches_tracked", "dec_conv.0.1.running_mean", "dec_conv.0.1.running_var", "dec_conv.0.1.weight"]
    small = gennet.AEViT(1, 1, 28, 24).train()                                  # no decoder stage: conv_final alone
    assert len(small.dec_conv) == 0 and small(torch.rand(2, 1, 28, 28)).shape == (2, 1, 28, 28)
    assert fused.TAIL_CALLS == calls
