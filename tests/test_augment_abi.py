"""CPU-side checks of ppn_augment_params / ppn_augment_codes / ppn_augment_rgb (csrc/augment.hip): header, library, bindings and
capi.hip carry the three entry points with matching argument names at ABI 111; every bad argument is refused with PPN_E_INVALID
before any HIP call (the pointers below are never dereferenced); the source is in the Makefile's SRCS, cross-compiles with the
Makefile's flags for gfx950 and none of its kernels uses scratch; and the host constants are the header's."""
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
IMAGE_ARGS = ["label_in", "params", "img_out", "label_out", "B", "H", "W", "Ho", "Wo", "mean3", "std3", "seg_pad_val", "dtype", "stream"]
ARGS = {"ppn_augment_params": ["seed", "first_instance", "B", "flip_ratio", "brightness_delta", "contrast_lo", "contrast_hi", "saturation_lo",
                               "saturation_hi", "hue_delta", "params", "stream"],
        "ppn_augment_codes": ["grid"] + IMAGE_ARGS,
        "ppn_augment_rgb": ["rgb"] + IMAGE_ARGS}
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize --cuda-device-only -S".split()


def _args(decl):
    code = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    return [a.split()[-1].lstrip("*") for a in code.split(",")]


def test_header_library_and_bindings_carry_the_entry_points_at_abi_111():
    from ppnet_amd import _lib, fused, philox
    header = open(os.path.join(ROOT, "include", "ppnet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    capi = open(os.path.join(CSRC, "capi.hip")).read()
    assert int(re.search(r"#define\s+PPN_ABI_VERSION\s+(\d+)", header).group(1)) == 111
    assert _lib.ABI_VERSION == 111 and _lib.lib.ppn_version() == 111
    for name, args in ARGS.items():
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        assert name in re.search(r"/\* ABI version of this header.*?\*/", header, re.S).group(0), name
        assert _args(re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", code, re.S).group(1)) == args, name
        assert _args(re.search(r"\b" + name + r"\s*\((.*?)\)\s*\{", capi, re.S).group(1)) == args, name
        assert len(getattr(_lib.lib, name).argtypes) == len(args) and getattr(_lib.lib, name).restype is C.c_int, name
    kernels_h = open(os.path.join(CSRC, "ppn_kernels.h")).read()
    assert re.search(r"\bint\s+augment_launch\s*\(", kernels_h) and re.search(r"\bint\s+augment_params_launch\s*\(", kernels_h)
    # the host's constants are the header's and the device's
    defs = {k: int(v) for k, v in re.findall(r"#define\s+PPN_AUG_(\w+)\s+(\d+)", header)}
    assert defs == {"FLIP": fused.AUG_FLIP, "BRIGHTNESS": fused.AUG_BRIGHTNESS, "CONTRAST": fused.AUG_CONTRAST,
                    "CONTRAST_LAST": fused.AUG_CONTRAST_LAST, "SATURATION": fused.AUG_SATURATION, "HUE": fused.AUG_HUE,
                    "PARAM_WORDS": fused.AUG_PARAM_WORDS}
    assert sorted(v for k, v in defs.items() if k != "PARAM_WORDS") == [1, 2, 4, 8, 16, 32]
    device_h = open(os.path.join(CSRC, "ppn_device.h")).read()
    assert int(re.search(r"STREAM_AUG\s*=\s*(\d+)", device_h).group(1)) == philox.STREAM_AUG == 5


def _caller(f, ok):
    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    return call


def _f3():
    return (C.c_float * 3)(1.0, 2.0, 3.0)


@pytest.mark.parametrize("name", ["ppn_augment_codes", "ppn_augment_rgb"])
@pytest.mark.parametrize("dtype", [0, 1])
def test_image_entries_reject_bad_arguments_without_gpu(name, dtype):
    from ppnet_amd import _lib
    #                                        in  lab_in params img lab_out B  H  W   Ho  Wo  mean   std  pad  dtype  stream
    call = _caller(getattr(_lib.lib, name), [ONE, ONE, ONE, ONE, ONE, 2, 8, 16, 16, 24, _f3(), _f3(), 255, dtype, None])
    for i in (0, 2, 3, 10, 11):                                            # every pointer that must be there
        assert call(**{f"a{i}": None}) == E_INVALID, i
    assert call(a1=None) == E_INVALID and call(a4=None) == E_INVALID       # one label pointer without the other
    for i in range(5, 10):                                                 # B, H, W, Ho, Wo
        assert call(**{f"a{i}": 0}) == E_INVALID and call(**{f"a{i}": -8}) == E_INVALID, i
    for w in (4, 12, 17, 23):
        assert call(a7=w) == E_INVALID, w                                  # W % 8
    for wo in (28, 30, 33):
        assert call(a9=wo) == E_INVALID, wo                                # Wo % 8
    assert call(a8=7) == E_INVALID and call(a9=8) == E_INVALID             # Ho < H, Wo < W
    for d in (2, -1, 7):
        assert call(a13=d) == E_INVALID, d
    for i in (0, 1, 4):                                                    # code / label rows: 8 bytes
        for off in (4, 2, 1):
            assert call(**{f"a{i}": C.c_void_p(0x1000 + off)}) == E_INVALID, (i, off)
    for i in (2, 3):                                                       # parameters and image: 16 bytes
        for off in (8, 4, 2):
            assert call(**{f"a{i}": C.c_void_p(0x1000 + off)}) == E_INVALID, (i, off)
    # totals: B Ho Wo 3 >= 2^31
    assert call(a5=1, a8=1 << 16, a9=1 << 15) == E_INVALID                 # Ho Wo = 2^31
    assert call(a5=1 << 11, a8=1 << 10, a9=1 << 10) == E_INVALID           # B Ho Wo = 2^31
    assert call(a5=1 << 10, a8=1 << 10, a9=1 << 10) == E_INVALID           # B Ho Wo 3 = 3 * 2^30
    assert call(a5=2 ** 31 - 1, a8=2 ** 31 - 1, a9=2 ** 31 - 8) == E_INVALID


def test_params_entry_rejects_bad_arguments_without_gpu():
    from ppnet_amd import _lib
    #                                         seed first B flip  db   clo  chi  slo  shi  dh  params stream
    call = _caller(_lib.lib.ppn_augment_params, [1, 0, 4, 0.5, 32.0, 0.5, 1.5, 0.5, 1.5, 18, ONE, None])
    assert call(a10=None) == E_INVALID
    for off in (8, 4, 2):
        assert call(a10=C.c_void_p(0x1000 + off)) == E_INVALID, off
    assert call(a2=0) == E_INVALID and call(a2=-1) == E_INVALID and call(a2=1 << 28) == E_INVALID
    nan = float("nan")
    for i, bad in ((3, (-0.1, 1.5, nan)), (4, (-1.0, 256.0, nan)), (5, (-0.5, 2.0, nan)), (6, (0.25, 300.0, nan)), (7, (-0.5, 2.0, nan)),
                   (8, (0.25, 300.0, nan))):
        for v in bad:
            assert call(**{f"a{i}": v}) == E_INVALID, (i, v)
    assert call(a9=-1) == E_INVALID and call(a9=181) == E_INVALID


def test_wrappers_refuse_cpu_tensors():
    torch = pytest.importorskip("torch")
    from ppnet_amd import fused
    g = torch.zeros(1, 8, 8, dtype=torch.uint8)
    p = torch.zeros(1, 8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        fused.augment_params(0, 0, 1, "cpu")
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        fused.augment_codes(g, None, p, (0, 0, 0), (1, 1, 1), torch.float32)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        fused.augment_rgb(g.unsqueeze(-1).expand(1, 8, 8, 3), None, p, (0, 0, 0), (1, 1, 1), torch.float32)


def test_augment_source_is_built_and_uses_no_scratch(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not present")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "augment.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    for fl in FLAGS[:-2]:
        assert fl.replace("gfx950", "$(ARCH)") in mk, fl                            # the Makefile's own flags
    out = tmp_path / "augment.s"
    subprocess.run([HIPCC, *FLAGS, os.path.join(CSRC, "augment.hip"), "-o", str(out)], check=True, cwd=CSRC, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    scratch = dict(re.findall(r"\.amdhsa_kernel (\S+).*?; ScratchSize: (\d+)", out.read_text(), re.S))
    # the parameter kernel, and codes / rgb per output type
    assert len(scratch) == 5 and sum("augment_codes_kernel" in k for k in scratch) == 2 and sum("augment_rgb_kernel" in k for k in scratch) == 2
    assert sum("augment_params_kernel" in k for k in scratch) == 1
    assert all(int(v) == 0 for v in scratch.values()), scratch
