"""CPU-side checks of ppn_resize_dice_workspace / ppn_resize_dice_fwd / ppn_resize_dice_bwd (csrc/resize_dice.hip): header, library,
bindings and the Makefile carry the three entry points at ABI 111 with the argument order of the header; the workspace size follows
the header's formula; every bad argument is refused with PPN_E_INVALID before any HIP call (the pointers below are never
dereferenced); the host constants are the kernels'; and the wrapper refuses CPU tensors."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ppnet_amd", "csrc")
E_INVALID = -1
ONE = C.c_void_p(0x1000)                                       # 16-byte aligned, never dereferenced on these paths
SCALARS = ["B", "C", "h", "w", "H", "W", "ignore_index", "smooth", "logit_dtype", "label_dtype", "stream"]
FWD = ["logit", "label", "class_weight", "workspace", "lse", "sums", "loss", "correct"] + SCALARS
BWD = ["logit", "label", "lse", "sums", "class_weight", "grad_out", "workspace", "dlogit"] + SCALARS
NAMES = ("ppn_resize_dice_workspace", "ppn_resize_dice_fwd", "ppn_resize_dice_bwd")


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
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name) and name in version_note, name
    for name, want in (("ppn_resize_dice_fwd", FWD), ("ppn_resize_dice_bwd", BWD)):
        assert _args(re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, code, re.S).group(1)) == want
        assert _args(re.search(r"\b%s\s*\((.*?)\)\s*\{" % name, capi, re.S).group(1)) == want
        f = getattr(_lib.lib, name)
        assert len(f.argtypes) == len(want) == 19 and f.restype is C.c_int and f.argtypes[15] is C.c_float
    assert _args(re.search(r"int64_t\s+ppn_resize_dice_workspace\s*\((.*?)\)\s*;", code, re.S).group(1)) == ["B", "C", "H", "W"]
    assert _lib.lib.ppn_resize_dice_workspace.restype is C.c_int64
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "resize_dice.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    text = open(os.path.join(CSRC, "resize_dice.hip")).read()
    assert '#include "resize_tap.h"' in text and "bilinear_tap(int" not in text          # the shared taps: included, not copied
    assert not re.search(r"\b(void|float)\s+(tap_range|tap_weight|stf)\s*\(", text)      # nor the gather's scan, weight and store


def test_workspace_follows_the_header_formula():
    from ppnet_amd import _lib, fused
    f = _lib.lib.ppn_resize_dice_workspace
    px = fused.RESIZE_DICE_PIXELS
    for B, Cc, H, W in ((1, 1, 1, 1), (2, 2, 64, 64), (3, 19, 33, 47), (8, 2, 224, 224), (8, 19, 224, 224), (1, 256, 4, 4), (5, 150, 31, 33)):
        want = 4 * max(B * -(-(H * W) // px) * (3 * Cc + 1), B * H * W + 4 * B * Cc)
        assert f(B, Cc, H, W) == want == fused.resize_dice_workspace_bytes(B, Cc, H, W), (B, Cc, H, W)
    for bad in ((0, 2, 4, 4), (1, 0, 4, 4), (1, 2, 0, 4), (1, 2, 4, 0), (-1, 2, 4, 4), (1, 257, 4, 4), (1, 2, 1 << 16, 1 << 15),
                (1 << 11, 2, 1 << 10, 1 << 10)):
        assert f(*bad) < 0, bad


def _caller(f, ok):
    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    return call


@pytest.mark.parametrize("which", ["fwd", "bwd"])
@pytest.mark.parametrize("logit_dtype", [0, 1])
@pytest.mark.parametrize("label_dtype", [0, 1])
def test_rejects_bad_arguments_without_gpu(which, logit_dtype, label_dtype):
    from ppnet_amd import _lib
    f = getattr(_lib.lib, f"ppn_resize_dice_{which}")
    names = FWD if which == "fwd" else BWD
    #                   8 pointers   B  C  h   w   H   W   ignore smooth ldt          labdt        stream
    call = _caller(f, [ONE] * 8 + [2, 3, 16, 12, 64, 48, 255, 1.0, logit_dtype, label_dtype, None])
    at = {n: i for i, n in enumerate(names)}
    optional = {"class_weight", "lse"} if which == "fwd" else {"class_weight"}
    for n in names[:8]:
        if n not in optional:
            assert call(**{f"a{at[n]}": None}) == E_INVALID, n
            assert call(**{f"a{at[n]}": None, f"a{at['class_weight']}": None}) == E_INVALID, n
    for n in ("logit", "workspace", "lse") + (("dlogit",) if which == "bwd" else ()):      # 16 bytes
        for off in (8, 4, 2):
            assert call(**{f"a{at[n]}": C.c_void_p(0x1000 + off)}) == E_INVALID, (n, off)
    for n in ("sums",) + (("correct",) if which == "fwd" else ()):                         # 8 bytes
        for off in (4, 2, 1):
            assert call(**{f"a{at[n]}": C.c_void_p(0x1000 + off)}) == E_INVALID, (n, off)
    for n in ("class_weight",) + (("loss",) if which == "fwd" else ("grad_out",)):         # 4 bytes
        for off in (2, 1):
            assert call(**{f"a{at[n]}": C.c_void_p(0x1000 + off)}) == E_INVALID, (n, off)
    if label_dtype == 1:
        for off in (4, 2, 1):                                                              # int64 labels
            assert call(**{f"a{at['label']}": C.c_void_p(0x1000 + off)}) == E_INVALID, off
    for i in range(8, 14):                                                                 # B, C, h, w, H, W
        assert call(**{f"a{i}": 0}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID, i
    assert call(a9=257) == E_INVALID and call(a9=1 << 20) == E_INVALID and call(a9=2 ** 31 - 1) == E_INVALID     # C > DICE_MAX_C
    for i in (16, 17):
        assert call(**{f"a{i}": 2}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID, i
    for smooth in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        assert call(a15=smooth) == E_INVALID, smooth
    assert call(a8=1, a12=1 << 16, a13=1 << 15) == E_INVALID                               # B H W = 2^31
    assert call(a8=1 << 11, a12=1 << 10, a13=1 << 10) == E_INVALID
    assert call(a8=2 ** 31 - 1, a12=2 ** 31 - 1, a13=2 ** 31 - 1) == E_INVALID
    assert call(a8=1, a9=256, a10=1 << 12, a11=1 << 11) == E_INVALID                       # B C h w = 2^31
    assert call(a8=1 << 11, a9=4, a10=1 << 9, a11=1 << 9) == E_INVALID
    assert call(a9=256, a10=2 ** 31 - 1, a11=2 ** 31 - 1) == E_INVALID
    assert call(a8=1 << 23, a10=1, a11=1, a12=1, a13=1) == E_INVALID                       # a tile per image: 2^23 workgroups of 256
    if which == "bwd":
        assert call(a8=1, a9=16, a10=1 << 13, a11=1 << 13, a12=1 << 15, a13=1 << 15) == E_INVALID  # 2^30 outputs at 8 lanes each


def test_host_constants_are_the_kernels():
    from ppnet_amd import fused
    src = open(os.path.join(CSRC, "resize_dice.hip")).read()
    const = {k: v for k, v in re.findall(r"constexpr int (DICE_\w+) = ([^;]+);", src)}
    assert int(const["DICE_THREADS"]) == fused.RESIZE_DICE_THREADS == 256
    assert const["DICE_PX"] == "DICE_THREADS * DICE_PER_THREAD" and int(const["DICE_PER_THREAD"]) * 256 == fused.RESIZE_DICE_PIXELS == 1024
    assert 19 <= int(const["DICE_MAX_C"]) == fused.RESIZE_DICE_MAX_CLASSES <= 256
    assert fused.DICE_CALLS.keys() == {"fwd", "bwd"}
    kernels_h = open(os.path.join(CSRC, "ppn_kernels.h")).read()
    for name in ("resize_dice_max_classes", "resize_dice_pixels", "resize_dice_threads", "resize_dice_fwd_launch", "resize_dice_bwd_launch"):
        assert re.search(r"\b%s\s*\(" % name, kernels_h), name


def test_resize_dice_refuses_cpu_tensors_and_bad_values():
    torch = pytest.importorskip("torch")
    from ppnet_amd import fused
    lg, gt = torch.randn(1, 2, 4, 4), torch.zeros(1, 8, 8, dtype=torch.uint8)
    assert not fused.resize_dice_ok(lg, gt)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        fused.resize_dice(lg, gt)
