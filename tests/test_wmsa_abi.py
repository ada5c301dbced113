"""CPU-side checks of ppn_wmsa_fwd (csrc/wmsa_gen.hip): the symbol is exported and bound, the header, the library and the bindings
still agree on ABI version 111, and every bad argument is refused with its code before any HIP call (the pointers below are never
dereferenced; no GPU is touched)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED = -1, -3


def test_wmsa_fwd_is_exported_and_abi_stays_111():
    from ppnet_amd import _lib
    assert "ppn_wmsa_fwd" in _lib.EXPORTS
    f = _lib.lib.ppn_wmsa_fwd
    assert len(f.argtypes) == 14 and f.argtypes[11] is C.c_float and f.restype is C.c_int
    hdr = open(os.path.join(ROOT, "include", "ppnet_hip.h")).read()
    assert re.search(r"^int ppn_wmsa_fwd\(", hdr, re.M)
    assert int(re.search(r"#define PPN_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == _lib.lib.ppn_version() == 111
    mk = open(os.path.join(ROOT, "ppnet_amd", "csrc", "Makefile")).read()
    assert "wmsa_gen.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()


def test_wmsa_fwd_rejects_bad_arguments_without_gpu():
    from ppnet_amd import _lib
    f = _lib.lib.ppn_wmsa_fwd
    one = C.c_void_p(0x1000)                                   # 16-byte aligned, never dereferenced on these paths
    #     qkv  pad  rpb  out  B  H   W   heads head_dim window shift scale dtype stream
    ok = [one, one, one, one, 2, 15, 29, 3, 8, 14, 7, 0.125, 1, None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    for i in range(4):                                                             # each of the four pointers NULL
        assert call(**{f"a{i}": None}) == E_INVALID, i
    for i in (4, 5, 6, 7):                                                         # B, H, W, heads
        assert call(**{f"a{i}": 0}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID, i
    assert call(a7=65536) == E_INVALID and call(a7=65536, a12=0) == E_INVALID
    for s in (0.0, -0.125, float("nan"), float("inf"), float("-inf")):
        assert call(a11=s) == E_INVALID, s
    assert call(a12=2) == E_INVALID and call(a12=-1) == E_INVALID
    for i, off in enumerate((8, 2, 4, 12)):                                        # 16-byte alignment of all four buffers
        for dt in (0, 1):
            assert call(**{f"a{i}": C.c_void_p(0x1000 + off), "a12": dt}) == E_INVALID, (i, dt)
    assert call(a4=1 << 30, a5=1 << 10, a6=1 << 10) == E_INVALID                   # B * windows >= 2^31
    assert call(a4=1 << 20, a5=14, a6=14, a7=8) == E_INVALID                       # 2^20 windows x 8 heads x 256 work-items = 2^31
    assert call(a4=1 << 20, a5=7, a6=7, a7=32, a9=7, a10=3) == E_INVALID           # ... x 32 heads x 64 at window 7
    # (window, head dim) outside the set, and shifts other than 0 and window // 2
    for w, d in ((14, 4), (8, 16), (14, 64), (14, 0), (14, -8), (7, 4), (7, 64), (0, 8), (-14, 8), (28, 8), (14, 12)):
        assert call(a8=d, a9=w) == E_UNSUPPORTED and call(a8=d, a9=w, a10=0) == E_UNSUPPORTED, (w, d)
    for sh in (5, 1, 3, 6, 13, 14, -1, -7):
        assert call(a10=sh) == E_UNSUPPORTED, sh
    for d in (8, 16, 32):
        for sh in (7, 1, 2, 4, 6, -3):
            assert call(a8=d, a9=7, a10=sh) == E_UNSUPPORTED, (d, sh)
    # unsupported and misaligned at once: the shape is judged first, as documented
    assert call(a9=8, a3=C.c_void_p(0x1004)) == E_UNSUPPORTED
