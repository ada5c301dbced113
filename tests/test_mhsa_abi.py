"""CPU-side checks of ppn_mhsa_fwd (csrc/mhsa.hip): every bad argument is refused with its code before any HIP call (the pointers
below are never dereferenced), and the emitted gfx950 code of both kernels uses no scratch (hipcc cross-compiles here; nothing
runs)."""
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


def test_mhsa_rejects_bad_arguments_without_gpu():
    from ppnet_amd import _lib
    f = _lib.lib.ppn_mhsa_fwd
    one = C.c_void_p(0x1000)                                   # 16-byte aligned, never dereferenced on these paths
    ok = [one, one, 2, 197, 12, 64, 0.125, 1, None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    assert call(a0=None) == E_INVALID and call(a1=None) == E_INVALID
    for i in (2, 3, 4):
        assert call(**{f"a{i}": 0}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID
    assert call(a5=0) == E_INVALID and call(a5=-64) == E_INVALID
    for s in (0.0, -0.125, float("nan"), float("inf"), float("-inf")):
        assert call(a6=s) == E_INVALID, s
    assert call(a7=2) == E_INVALID and call(a7=-1) == E_INVALID
    assert call(a5=32) == E_UNSUPPORTED and call(a5=128) == E_UNSUPPORTED and call(a5=32, a7=0) == E_UNSUPPORTED
    assert call(a0=C.c_void_p(0x1008)) == E_INVALID and call(a1=C.c_void_p(0x1002)) == E_INVALID     # 16-byte alignment
    big = 2 ** 31 - 1
    assert call(a2=big) == E_INVALID                                               # 2^31 - 1 workgroups of 256 work-items
    assert call(a2=1 << 16, a3=1 << 14, a4=1 << 8) == E_INVALID and call(a2=1 << 16, a3=1 << 14, a4=1 << 8, a7=0) == E_INVALID
    assert call(a2=64, a3=big, a4=1) == E_INVALID


def test_mhsa_kernels_use_no_scratch(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not present")
    out = tmp_path / "mhsa.s"
    flags = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize --cuda-device-only -S".split()
    subprocess.run([HIPCC, *flags, os.path.join(CSRC, "mhsa.hip"), "-o", str(out)], check=True, cwd=CSRC, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    asm = out.read_text()
    scratch = dict(re.findall(r"\.amdhsa_kernel (\S+).*?; ScratchSize: (\d+)", asm, re.S))
    assert len(scratch) == 2 and all(int(v) == 0 for v in scratch.values()), scratch
    bf16 = re.search(r"^(_ZN3ppn16mhsa_bf16_kernel\w*):[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M).group(2)
    assert "ds_read_b64_tr_b16" in bf16 and "v_mfma_f32_16x16x32_bf16" in bf16
