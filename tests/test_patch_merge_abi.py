"""CPU-side checks of ppn_patch_merge_ln_fwd / ppn_patch_merge_ln_bwd_workspace / ppn_patch_merge_ln_bwd (csrc/patch_merge_ln.hip):
header, library, bindings and the Makefile carry the three entry points at ABI 111 with the argument order of the header; the
workspace size follows the header's formula; every bad argument is refused before any HIP call (the pointers below are never
dereferenced); the host constants are the kernels'; and the wrapper takes the torch form for CPU tensors and unsupported widths."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ppnet_amd", "csrc")
E_INVALID, E_UNSUPPORTED = -1, -3
ONE = C.c_void_p(0x1000)                                       # 16-byte aligned, never dereferenced on these paths
FWD = ["x", "gamma", "beta", "y", "stats", "B", "H", "W", "C", "eps", "dtype", "stream"]
BWD = ["gy", "x", "stats", "gamma", "workspace", "dx", "dgamma", "dbeta", "B", "H", "W", "C", "dtype", "stream"]
NAMES = ("ppn_patch_merge_ln_fwd", "ppn_patch_merge_ln_bwd_workspace", "ppn_patch_merge_ln_bwd")
WIDTHS = (8, 16, 32, 64, 128, 256, 512)


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
    for name in NAMES + ("ppn_patch_merge_ln_rows", "ppn_patch_merge_ln_max_blocks"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name) and name in version_note, name
    for name, want in (("ppn_patch_merge_ln_fwd", FWD), ("ppn_patch_merge_ln_bwd", BWD)):
        assert _args(re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, code, re.S).group(1)) == want
        assert _args(re.search(r"\b%s\s*\((.*?)\)\s*\{" % name, capi, re.S).group(1)) == want
        f = getattr(_lib.lib, name)
        assert len(f.argtypes) == len(want) and f.restype is C.c_int
    assert _lib.lib.ppn_patch_merge_ln_fwd.argtypes[9] is C.c_float
    assert _args(re.search(r"int64_t\s+ppn_patch_merge_ln_bwd_workspace\s*\((.*?)\)\s*;", code, re.S).group(1)) == ["B", "H", "W", "C"]
    assert _lib.lib.ppn_patch_merge_ln_bwd_workspace.restype is C.c_int64
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "patch_merge_ln.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    text = open(os.path.join(CSRC, "patch_merge_ln.hip")).read()
    assert '#include "norm_vec.h"' in text and "struct Vec8" not in text                 # the shared row piece: included, not copied
    for kernel in ("pm_ln_fwd_kernel", "pm_ln_bwd_kernel", "pm_ln_colsum_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\b" % kernel, text), kernel
    assert "atomic" not in text.split("namespace ppn {", 1)[1].replace("no atomics", "").replace("without atomics", "")


def test_workspace_follows_the_header_formula():
    from ppnet_amd import _lib, fused
    f, rows_of, cap = _lib.lib.ppn_patch_merge_ln_bwd_workspace, _lib.lib.ppn_patch_merge_ln_rows, _lib.lib.ppn_patch_merge_ln_max_blocks()
    for B, H, W, Cc in ((1, 1, 1, 8), (1, 2, 2, 8), (2, 7, 5, 32), (3, 6, 9, 128), (8, 56, 56, 128), (8, 28, 28, 256), (8, 14, 14, 512),
                        (8, 128, 128, 128), (8, 32, 32, 512), (1, 129, 129, 512), (64, 200, 200, 8)):
        rows = B * -(-H // 2) * -(-W // 2)
        want = 4 * min(-(-rows // rows_of(Cc)), cap) * 2 * 4 * Cc
        assert f(B, H, W, Cc) == want == fused.patch_merge_workspace_bytes(B, H, W, Cc), (B, H, W, Cc)
    for bad in ((0, 4, 4, 8), (1, 0, 4, 8), (1, 4, 0, 8), (1, 4, 4, 0), (-1, 4, 4, 8), (1, 4, 4, 12), (1, 4, 4, 96), (1, 4, 4, 1024),
                (1, 1 << 15, 1 << 13, 8), (1 << 10, 1 << 10, 1 << 8, 8), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 512)):
        assert f(*bad) < 0, bad


def _caller(f, ok):
    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    return call


@pytest.mark.parametrize("dtype", [0, 1])
def test_forward_rejects_bad_arguments_without_gpu(dtype):
    from ppnet_amd import _lib
    #                                                 5 pointers  B  H  W  C   eps   dtype  stream
    call = _caller(_lib.lib.ppn_patch_merge_ln_fwd, [ONE] * 5 + [2, 7, 5, 32, 1e-5, dtype, None])
    at = {n: i for i, n in enumerate(FWD)}
    for n in ("x", "gamma", "beta", "y"):                                                  # stats may be NULL, the others not
        assert call(**{f"a{at[n]}": None}) == E_INVALID, n
        assert call(**{f"a{at[n]}": None, "a4": None}) == E_INVALID, n
        for off in (8, 4, 2, 1):                                                           # 16 bytes
            assert call(**{f"a{at[n]}": C.c_void_p(0x1000 + off)}) == E_INVALID, (n, off)
    for off in (2, 1, 3):                                                                  # stats: 4 bytes
        assert call(a4=C.c_void_p(0x1000 + off)) == E_INVALID, off
    _common_refusals(call, 5)
    for eps in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        assert call(a9=eps) == E_INVALID, eps
    for d in (2, -1, 7):
        assert call(a10=d) == E_INVALID, d


@pytest.mark.parametrize("dtype", [0, 1])
def test_backward_rejects_bad_arguments_without_gpu(dtype):
    from ppnet_amd import _lib
    #                                                 8 pointers  B  H  W  C   dtype  stream
    call = _caller(_lib.lib.ppn_patch_merge_ln_bwd, [ONE] * 8 + [2, 7, 5, 32, dtype, None])
    at = {n: i for i, n in enumerate(BWD)}
    for n in ("gy", "x", "stats", "gamma", "workspace", "dx"):                              # dgamma and dbeta may be NULL
        assert call(**{f"a{at[n]}": None}) == E_INVALID, n
        assert call(**{f"a{at[n]}": None, "a6": None, "a7": None}) == E_INVALID, n
    for n in ("gy", "x", "gamma", "workspace", "dx", "dgamma", "dbeta"):                    # 16 bytes
        for off in (8, 4, 2, 1):
            assert call(**{f"a{at[n]}": C.c_void_p(0x1000 + off)}) == E_INVALID, (n, off)
    for off in (2, 1, 3):                                                                  # stats: 4 bytes
        assert call(a2=C.c_void_p(0x1000 + off)) == E_INVALID, off
    _common_refusals(call, 8)
    for d in (2, -1, 7):
        assert call(a12=d) == E_INVALID, d


def _common_refusals(call, b):
    """Extents, widths and counts: argument b is B, then H, W, C."""
    for i in range(b, b + 4):
        assert call(**{f"a{i}": 0}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID and call(**{f"a{i}": -(2 ** 31)}) == E_INVALID, i
    for width in (12, 96, 1024, 4, 7, 9, 24, 48, 192, 384, 520, 768, 2048, 2 ** 31 - 1):
        assert call(**{f"a{b + 3}": width}) == E_UNSUPPORTED, width
    B, H, W, Cc = (f"a{b + k}" for k in range(4))
    assert call(**{B: 1, H: 1 << 15, W: 1 << 13, Cc: 8}) == E_INVALID                      # B H W C = 2^31
    assert call(**{B: 1 << 10, H: 1 << 10, W: 1 << 8, Cc: 8}) == E_INVALID
    assert call(**{B: 2 ** 31 - 1, H: 2 ** 31 - 1, W: 2 ** 31 - 1, Cc: 512}) == E_INVALID
    assert call(**{B: 2 ** 31 - 1, H: 1, W: 1, Cc: 8}) == E_INVALID                        # x fits; the gathered rows (4C each) do not
    assert call(**{B: (1 << 28) - 1, H: 1, W: 1, Cc: 8}) == E_INVALID                      # 2^28 - 1 rows of 32: 2^33 - 32 elements
    assert call(**{B: 1, H: 1, W: 2 ** 31 - 1, Cc: 8}) == E_INVALID


def test_host_constants_are_the_kernels():
    from ppnet_amd import _lib, fused
    src = open(os.path.join(CSRC, "patch_merge_ln.hip")).read()
    const = {k: v for k, v in re.findall(r"constexpr int (PM_\w+) = ([^;]+);", src)}
    assert int(const["PM_THREADS"]) == 256
    assert int(const["PM_MAX_BLOCKS"]) == fused.MERGE_MAX_BLOCKS == _lib.lib.ppn_patch_merge_ln_max_blocks() == 1024
    assert fused.MERGE_WIDTHS == frozenset(WIDTHS)
    for width in range(0, 1100):
        want = 256 // (width // 8) if width in WIDTHS else 0                               # C / 8 lanes per row
        assert _lib.lib.ppn_patch_merge_ln_rows(width) == want == fused.patch_merge_rows(width), width
    assert fused.MERGE_CALLS.keys() == {"fwd", "bwd"}
    kernels_h = open(os.path.join(CSRC, "ppn_kernels.h")).read()
    for name in ("patch_merge_ln_rows", "patch_merge_ln_max_blocks", "patch_merge_ln_bwd_workspace_bytes", "patch_merge_ln_fwd_launch",
                 "patch_merge_ln_bwd_launch"):
        assert re.search(r"\b%s\s*\(" % name, kernels_h), name


def test_wrapper_takes_the_torch_form_for_cpu_tensors_and_other_widths(monkeypatch):
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F
    from ppnet_amd import fused
    monkeypatch.delenv("PPNET_LIBRARY_MERGE", raising=False)
    calls = dict(fused.MERGE_CALLS)
    for Cc in (8, 12, 96, 1024):
        g = torch.Generator().manual_seed(Cc)
        x = torch.randn(2, 3, 5, Cc, generator=g)
        ln = torch.nn.LayerNorm(4 * Cc)
        with torch.no_grad():
            ln.weight.uniform_(0.7, 1.3, generator=g); ln.bias.uniform_(-0.2, 0.2, generator=g)
        assert not fused.patch_merge_ln_ok(x, ln)                                          # a CPU tensor, whatever the width
        xp = F.pad(x, (0, 0, 0, 1, 0, 1))
        want = ln(torch.cat([xp[:, 0::2, 0::2], xp[:, 1::2, 0::2], xp[:, 0::2, 1::2], xp[:, 1::2, 1::2]], -1))
        got = fused.patch_merge_ln(x, ln)
        assert got.shape == (2, 2, 3, 4 * Cc) and torch.equal(got, want)
    assert fused.MERGE_CALLS == calls                                                       # nothing was launched

    class Fake:                                                                            # what the predicate reads of a CUDA tensor
        is_cuda, dtype, device = True, torch.float32, torch.device("cpu")

        def __init__(self, *shape):
            self.shape = shape

        def dim(self):
            return len(self.shape)

        def numel(self):
            n = 1
            for s in self.shape:
                n *= s
            return n
    for Cc in (12, 96, 1024):
        assert not fused.patch_merge_ln_ok(Fake(1, 4, 4, Cc), torch.nn.LayerNorm(4 * Cc)), Cc
    for Cc in WIDTHS:
        assert fused.patch_merge_ln_ok(Fake(1, 4, 4, Cc), torch.nn.LayerNorm(4 * Cc)), Cc
        assert not fused.patch_merge_ln_ok(Fake(1, 4, 4, Cc), torch.nn.LayerNorm(4 * Cc, elementwise_affine=False)), Cc
        assert not fused.patch_merge_ln_ok(Fake(1, 4, 4, Cc), torch.nn.LayerNorm(Cc)), Cc
    monkeypatch.setenv("PPNET_LIBRARY_MERGE", "1")
    assert not fused.patch_merge_ln_ok(Fake(1, 4, 4, 64), torch.nn.LayerNorm(256))
