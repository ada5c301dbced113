"""CPU-side checks of ppn_seg_eval (csrc/seg_eval.hip): header, library and bindings carry the entry point with its 14 arguments at
ABI 111; every bad argument is refused with PPN_E_INVALID before any HIP call (the pointers below are never dereferenced); the source
is in the Makefile's SRCS, cross-compiles with the Makefile's flags for gfx950 and none of its kernels uses scratch; resize_ce.hip,
which now shares its tap functions through csrc/resize_tap.h, still yields its 17 kernels; and the host constants are the kernel's."""
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
ARGS = ["logit", "label", "pred", "areas", "B", "C", "h", "w", "H", "W", "ignore_index", "logit_dtype", "label_dtype", "stream"]
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize --cuda-device-only -S".split()


def _args(decl):
    code = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    return [a.split()[-1].lstrip("*") for a in code.split(",")]


def test_header_library_and_bindings_carry_the_entry_point_at_abi_111():
    from ppnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "ppnet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert int(re.search(r"#define\s+PPN_ABI_VERSION\s+(\d+)", header).group(1)) == 111
    assert _lib.ABI_VERSION == 111 and _lib.lib.ppn_version() == 111
    assert "ppn_seg_eval" in _lib.EXPORTS and hasattr(_lib.lib, "ppn_seg_eval")
    assert "ppn_seg_eval" in re.search(r"/\* ABI version of this header.*?\*/", header, re.S).group(0)
    assert _args(re.search(r"int\s+ppn_seg_eval\s*\((.*?)\)\s*;", code, re.S).group(1)) == ARGS
    assert len(ARGS) == 14 and len(_lib.lib.ppn_seg_eval.argtypes) == 14 and _lib.lib.ppn_seg_eval.restype is C.c_int
    capi = open(os.path.join(CSRC, "capi.hip")).read()
    assert _args(re.search(r"\bppn_seg_eval\s*\((.*?)\)\s*\{", capi, re.S).group(1)) == ARGS
    kernels_h = open(os.path.join(CSRC, "ppn_kernels.h")).read()
    assert re.search(r"\bint\s+seg_eval_launch\s*\(", kernels_h)


def _caller(f, ok):
    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    return call


@pytest.mark.parametrize("logit_dtype", [0, 1])
@pytest.mark.parametrize("label_dtype", [0, 1])
def test_rejects_bad_arguments_without_gpu(logit_dtype, label_dtype):
    from ppnet_amd import _lib
    #                                   logit label pred areas B  C  h   w   H   W   ignore ldt          labdt        stream
    call = _caller(_lib.lib.ppn_seg_eval, [ONE, ONE, ONE, ONE, 2, 3, 16, 12, 64, 48, 255, logit_dtype, label_dtype, None])
    for i in (0, 1, 3):                                                    # every pointer but pred
        assert call(**{f"a{i}": None}) == E_INVALID, i
        assert call(**{f"a{i}": None, "a2": None}) == E_INVALID, i
    for off in (8, 4, 2):                                                  # logit: 16 bytes
        assert call(a0=C.c_void_p(0x1000 + off)) == E_INVALID, off
    for off in (4, 2, 1):                                                  # areas: an int64
        assert call(a3=C.c_void_p(0x1000 + off)) == E_INVALID, off
    if label_dtype == 1:
        for off in (4, 2, 1):                                              # int64 labels
            assert call(a1=C.c_void_p(0x1000 + off)) == E_INVALID, off
    for i in range(4, 10):                                                 # B, C, h, w, H, W
        assert call(**{f"a{i}": 0}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID, i
    assert call(a5=257) == E_INVALID and call(a5=1 << 20) == E_INVALID and call(a5=2 ** 31 - 1) == E_INVALID     # C > 256
    for i in (11, 12):
        assert call(**{f"a{i}": 2}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID, i
    assert call(a4=1, a8=1 << 16, a9=1 << 15) == E_INVALID                 # B H W = 2^31
    assert call(a4=1 << 11, a8=1 << 10, a9=1 << 10) == E_INVALID
    assert call(a4=2 ** 31 - 1, a8=2 ** 31 - 1, a9=2 ** 31 - 1) == E_INVALID
    assert call(a4=1, a5=256, a6=1 << 12, a7=1 << 11) == E_INVALID         # B C h w = 2^31
    assert call(a4=1 << 11, a5=4, a6=1 << 9, a7=1 << 9) == E_INVALID
    assert call(a5=256, a6=2 ** 31 - 1, a7=2 ** 31 - 1) == E_INVALID


def test_host_constants():
    from ppnet_amd import fused
    src = open(os.path.join(CSRC, "seg_eval.hip")).read()
    const = {k: v for k, v in re.findall(r"constexpr int (SE_\w+) = ([^;]+);", src)}
    assert int(const["SE_THREADS"]) == fused.SEG_EVAL_THREADS == 256
    assert const["SE_PX"] == "SE_THREADS * SE_PER_THREAD" and int(const["SE_PER_THREAD"]) * 256 == fused.SEG_EVAL_PIXELS == 1024
    assert int(const["SE_MAX_GROUPS"]) == fused.SEG_EVAL_MAX_GROUPS
    assert int(const["SE_BALLOT_C"]) == fused.SEG_EVAL_BALLOT_CLASSES
    assert int(const["SE_MAX_C"]) == fused.SEG_EVAL_MAX_CLASSES == 256
    assert fused.EVAL_CALLS.keys() == {"fwd"}


def _kernels(tmp_path, name):
    out = tmp_path / (name + ".s")
    subprocess.run([HIPCC, *FLAGS, os.path.join(CSRC, name + ".hip"), "-o", str(out)], check=True, cwd=CSRC, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    return dict(re.findall(r"\.amdhsa_kernel (\S+).*?; ScratchSize: (\d+)", out.read_text(), re.S))


def test_seg_eval_source_is_built_and_uses_no_scratch(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not present")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "seg_eval.hip" in srcs and "resize_ce.hip" in srcs
    assert "resize_tap.h" in re.search(r"^%\.o:(.*)$", mk, re.M).group(1).split()          # a change of the shared taps rebuilds both
    for fl in FLAGS[:-2]:
        assert fl.replace("gfx950", "$(ARCH)") in mk, fl                            # the Makefile's own flags
    scratch = _kernels(tmp_path, "seg_eval")
    # per (logit type, label type, counting: wave ballots | LDS atomics)
    assert len(scratch) == 8 and all("seg_eval_kernel" in k for k in scratch), scratch
    assert all(int(v) == 0 for v in scratch.values()), scratch
    # resize_ce.hip includes the same header and keeps its kernels
    ce = _kernels(tmp_path, "resize_ce")
    assert len(ce) == 17 and all("resize_ce_" in k for k in ce) and all(int(v) == 0 for v in ce.values()), ce
    for name in ("seg_eval.hip", "resize_ce.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "resize_tap.h"' in text and "bilinear_tap(int" not in text, name     # included, not copied
        assert not re.search(r"\b(void|float)\s+(tap_range|tap_weight|stf)\s*\(", text), name  # nor the gather's scan, weight and store


def test_seg_eval_refuses_cpu_tensors():
    torch = pytest.importorskip("torch")
    from ppnet_amd import fused
    lg, gt = torch.randn(1, 2, 4, 4), torch.zeros(1, 8, 8, dtype=torch.uint8)
    assert not fused.seg_eval_ok(lg, gt)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        fused.seg_eval(lg, gt)
