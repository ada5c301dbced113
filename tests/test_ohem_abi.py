"""CPU-side checks of ppn_ohem_ce_workspace / ppn_ohem_ce_fwd / ppn_ohem_ce_bwd (csrc/ohem_ce.hip): header, library, bindings and the
Makefile's SRCS carry the three names at ABI 111; the argument names agree between header and capi.hip; every bad argument is refused
with PPN_E_INVALID before any HIP call (the pointers below are never dereferenced); the source cross-compiles with the Makefile's flags
for gfx950, none of its kernels uses scratch, and it includes csrc/resize_tap.h instead of copying it; the host constants are the
kernel's; CPU tensors are refused."""
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
NAMES = ("ppn_ohem_ce_workspace", "ppn_ohem_ce_fwd", "ppn_ohem_ce_bwd")
FWD_ARGS = ["logit", "label", "class_weight", "lse", "score", "loss", "counts", "threshold", "mask", "workspace", "workspace_bytes", "B", "C", "h", "w",
            "H", "W", "ignore_index", "mode", "thresh", "min_kept", "logit_dtype", "label_dtype", "stream"]
BWD_ARGS = ["logit", "label", "class_weight", "lse", "score", "threshold", "grad_out", "dlogit", "B", "C", "h", "w", "H", "W", "ignore_index", "mode",
            "logit_dtype", "label_dtype", "stream"]
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize --cuda-device-only -S".split()


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
    for earlier in ("ppn_resize_ce_fwd", "ppn_seg_eval", "ppn_augment_params", "ppn_na2d_bwd_vpad"):       # nothing was removed from the note
        assert earlier in version_note
    for name, args, ret in (("ppn_ohem_ce_fwd", FWD_ARGS, "int"), ("ppn_ohem_ce_bwd", BWD_ARGS, "int"),
                            ("ppn_ohem_ce_workspace", ["B", "H", "W"], "int64_t")):
        assert _args(re.search(ret + r"\s+" + name + r"\s*\((.*?)\)\s*;", code, re.S).group(1)) == args, name
        assert _args(re.search(r"\b" + name + r"\s*\((.*?)\)\s*\{", capi, re.S).group(1)) == args, name
        assert len(getattr(_lib.lib, name).argtypes) == len(args), name
    assert len(FWD_ARGS) == 24 and len(BWD_ARGS) == 19
    assert _lib.lib.ppn_ohem_ce_fwd.restype is C.c_int and _lib.lib.ppn_ohem_ce_bwd.restype is C.c_int
    assert _lib.lib.ppn_ohem_ce_workspace.restype is C.c_int64
    assert _lib.lib.ppn_ohem_ce_fwd.argtypes[FWD_ARGS.index("thresh")] is C.c_float
    assert _lib.lib.ppn_ohem_ce_fwd.argtypes[FWD_ARGS.index("workspace_bytes")] is C.c_int64
    kernels_h = open(os.path.join(CSRC, "ppn_kernels.h")).read()
    assert re.search(r"\bint\s+ohem_ce_fwd_launch\s*\(", kernels_h) and re.search(r"\bint\s+ohem_ce_bwd_launch\s*\(", kernels_h)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "ohem_ce.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()


def test_workspace_is_bytes_and_refuses_bad_sizes():
    from ppnet_amd import _lib, fused
    f = _lib.lib.ppn_ohem_ce_workspace
    words = 3 * (1 << fused.OHEM_DIGIT_BITS[0]) + 16 + 2 * fused.OHEM_MAX_GROUPS        # three histograms | state | partial sums | kept counts
    assert f(1, 1, 1) == f(16, 512, 512) == f(1, 1 << 15, (1 << 16) - 1) == 4 * words and f(1, 1, 1) % 16 == 0
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1, 1 << 16, 1 << 15), (1 << 11, 1 << 10, 1 << 10), (2 ** 31 - 1,) * 3):
        assert f(*bad) < 0, bad


def _caller(f, ok):
    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    return call


def _sizes(call, first):
    """B, C, h, w, H, W at positions first .. first + 5."""
    B, Cc, h, w, H, W = (f"a{first + i}" for i in range(6))
    for i in range(first, first + 6):
        assert call(**{f"a{i}": 0}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID, i
    assert call(**{B: 1, H: 1 << 16, W: 1 << 15}) == E_INVALID                 # B H W = 2^31
    assert call(**{B: 1 << 11, H: 1 << 10, W: 1 << 10}) == E_INVALID
    assert call(**{B: 2 ** 31 - 1, H: 2 ** 31 - 1, W: 2 ** 31 - 1}) == E_INVALID
    assert call(**{B: 1, Cc: 256, h: 1 << 12, w: 1 << 11}) == E_INVALID         # B C h w = 2^31
    assert call(**{B: 1 << 11, Cc: 4, h: 1 << 9, w: 1 << 9}) == E_INVALID
    assert call(**{Cc: 256, h: 2 ** 31 - 1, w: 2 ** 31 - 1}) == E_INVALID


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("logit_dtype", [0, 1])
@pytest.mark.parametrize("label_dtype", [0, 1])
def test_forward_rejects_bad_arguments_without_gpu(logit_dtype, label_dtype, mode):
    from ppnet_amd import _lib
    need = _lib.lib.ppn_ohem_ce_workspace(2, 64, 48)
    #       logit label cw  lse  score loss counts thr mask ws   bytes B  C  h   w   H   W  ignore mode thresh kept
    ok = [ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, need, 2, 3, 16, 12, 64, 48, 255, mode, 0.7, 100, logit_dtype, label_dtype, None]
    call = _caller(_lib.lib.ppn_ohem_ce_fwd, ok)
    for i in (0, 1, 3, 4, 5, 6, 7, 9):                                     # every pointer but class_weight and mask
        assert call(**{f"a{i}": None}) == E_INVALID, i
        assert call(**{f"a{i}": None, "a2": None, "a8": None}) == E_INVALID, i
    for i in (0, 3, 4, 9):                                                 # logit, lse, score, workspace: 16 bytes
        for off in (8, 4, 2):
            assert call(**{f"a{i}": C.c_void_p(0x1000 + off)}) == E_INVALID, (i, off)
    for i in (2, 5, 7):                                                    # class_weight, loss, threshold: a float32
        for off in (2, 1):
            assert call(**{f"a{i}": C.c_void_p(0x1000 + off)}) == E_INVALID, (i, off)
    for off in (4, 2, 1):                                                  # counts: int64
        assert call(a6=C.c_void_p(0x1000 + off)) == E_INVALID, off
    if label_dtype == 1:
        for off in (4, 2, 1):
            assert call(a1=C.c_void_p(0x1000 + off)) == E_INVALID, off
    _sizes(call, 11)
    for i in (21, 22):                                                     # dtype codes
        assert call(**{f"a{i}": 2}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID, i
    assert call(a18=3) == E_INVALID and call(a18=-1) == E_INVALID          # mode
    assert call(a10=need - 1) == E_INVALID and call(a10=0) == E_INVALID and call(a10=-1) == E_INVALID      # workspace too small
    if mode != 0:
        assert call(a20=0) == E_INVALID and call(a20=-5) == E_INVALID      # min_kept < 1
    if mode == 1:
        for t in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")):  # thresh outside (0, 1]
            assert call(a19=t) == E_INVALID, t


@pytest.mark.parametrize("logit_dtype", [0, 1])
@pytest.mark.parametrize("label_dtype", [0, 1])
def test_backward_rejects_bad_arguments_without_gpu(logit_dtype, label_dtype):
    from ppnet_amd import _lib
    #       logit label cw  lse  score thr  grad dlogit B  C  h   w   H   W  ignore mode
    ok = [ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, 2, 3, 16, 12, 64, 48, 255, 1, logit_dtype, label_dtype, None]
    call = _caller(_lib.lib.ppn_ohem_ce_bwd, ok)
    for i in (0, 1, 3, 4, 5, 6, 7):                                        # every pointer but class_weight
        assert call(**{f"a{i}": None}) == E_INVALID, i
        assert call(**{f"a{i}": None, "a2": None}) == E_INVALID, i
    for i in (0, 3, 4, 7):                                                 # logit, lse, score, dlogit: 16 bytes
        for off in (8, 4, 2):
            assert call(**{f"a{i}": C.c_void_p(0x1000 + off)}) == E_INVALID, (i, off)
    for i in (2, 5, 6):                                                    # class_weight, threshold, grad_out: a float32
        for off in (2, 1):
            assert call(**{f"a{i}": C.c_void_p(0x1000 + off)}) == E_INVALID, (i, off)
    if label_dtype == 1:
        for off in (4, 2, 1):
            assert call(a1=C.c_void_p(0x1000 + off)) == E_INVALID, off
    _sizes(call, 8)
    for i in (16, 17):
        assert call(**{f"a{i}": 2}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID, i
    assert call(a15=3) == E_INVALID and call(a15=-1) == E_INVALID


def test_host_constants():
    from ppnet_amd import fused
    src = open(os.path.join(CSRC, "ohem_ce.hip")).read()
    const = {k: v for k, v in re.findall(r"constexpr int (OH_\w+) = ([^;,]+)[;,]", src)}
    assert int(const["OH_THREADS"]) == fused.OHEM_THREADS == 256
    assert const["OH_PX"] == "OH_THREADS * OH_PER_THREAD" and int(const["OH_PER_THREAD"]) * 256 == fused.OHEM_PIXELS == 1024
    assert int(const["OH_MAX_GROUPS"]) == fused.OHEM_MAX_GROUPS
    assert tuple(int(const[f"OH_BITS{i}"]) for i in (1, 2, 3)) == fused.OHEM_DIGIT_BITS and sum(fused.OHEM_DIGIT_BITS) == 32
    assert len(fused.OHEM_DIGIT_BITS) <= 3                                 # three digits at most
    assert fused.OHEM_CALLS.keys() == {"fwd", "bwd"} and fused.LOSS_CALLS.keys() == {"fwd", "bwd"}
    assert (fused.OHEM_MODE_NONE, fused.OHEM_MODE_THRESH, fused.OHEM_MODE_TOPK) == (0, 1, 2)


def test_ohem_source_cross_compiles_without_scratch_and_includes_the_shared_taps(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not present")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for fl in FLAGS[:-2]:
        assert fl.replace("gfx950", "$(ARCH)") in mk, fl                    # the Makefile's own flags
    out = tmp_path / "ohem_ce.s"
    subprocess.run([HIPCC, *FLAGS, os.path.join(CSRC, "ohem_ce.hip"), "-o", str(out)], check=True, cwd=CSRC, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    asm = out.read_text()
    scratch = dict(re.findall(r"\.amdhsa_kernel (\S+).*?; ScratchSize: (\d+)", asm, re.S))
    # score and reduce per (logit type, label type); two histogram passes; the final sum; the backward per (logit, label, lanes 1 / 8 / 64)
    count = lambda s: sum(s in k for k in scratch)
    assert len(scratch) == 23 and all("ohem_" in k for k in scratch), scratch
    assert (count("ohem_score_kernel"), count("ohem_hist_kernel"), count("ohem_reduce_kernel"), count("ohem_final_kernel"),
            count("ohem_bwd_kernel")) == (4, 2, 4, 1, 12), scratch
    assert all(int(v) == 0 for v in scratch.values()), scratch
    assert "global_atomic_add_f32" not in asm and "ds_add_f32" not in asm and "cmpswap" not in asm      # integer atomics only
    text = open(os.path.join(CSRC, "ohem_ce.hip")).read()
    assert '#include "resize_tap.h"' in text and "bilinear_tap(int" not in text and "struct Tap" not in text        # included, not copied
    assert not re.search(r"\b(void|float)\s+(tap_range|tap_weight|stf)\s*\(", text)                   # nor the gather's scan, weight and store


def test_ohem_cross_entropy_refuses_cpu_tensors_and_bad_options():
    torch = pytest.importorskip("torch")
    from ppnet_amd import fused
    lg, gt = torch.randn(1, 2, 4, 4), torch.zeros(1, 8, 8, dtype=torch.uint8)
    assert not fused.ohem_ce_ok(lg, gt)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        fused.ohem_cross_entropy(lg, gt, thresh=0.7, min_kept=10)
    with pytest.raises(ValueError):
        fused._ohem_mode(0.7, None)                                        # thresh without min_kept
    assert fused._ohem_mode(None, None)[0] == 0 and fused._ohem_mode(0.7, 5) == (1, 0.7, 5) and fused._ohem_mode(None, 5)[0] == 2
