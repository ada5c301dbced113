"""C ABI of the up-sampling backward entries (csrc/upsample_bwd.hip): ppn_upsample2x_nhwc_bwd, ppn_upsample2x_concat_nhwc_bwd and
ppn_resize_concat_nhwc_bwd are exported, declared and bound, joined the ABI without moving its version, and validate before any HIP
call: every bad argument returns PPN_E_INVALID (the pointers are never dereferenced, so host addresses stand in for device buffers).
No GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ppn_upsample2x_nhwc_bwd", "ppn_upsample2x_concat_nhwc_bwd", "ppn_resize_concat_nhwc_bwd")
E_INVALID = -1
_buf = (ctypes.c_char * 64)()
P = ctypes.cast(_buf, ctypes.c_void_p)


def test_symbols_exported_declared_and_bound():
    from ppnet_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "ppnet_hip.h")).read()
    for name in NAMES:
        assert name in L.EXPORTS
        f = getattr(L.lib, name)
        assert f.restype is ctypes.c_int and f.argtypes is not None
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert len(L.lib.ppn_upsample2x_nhwc_bwd.argtypes) == 9
    assert len(L.lib.ppn_upsample2x_concat_nhwc_bwd.argtypes) == 9
    assert len(L.lib.ppn_resize_concat_nhwc_bwd.argtypes) == 8
    # new symbols change no argument list: the version stays (the header's own rule)
    assert int(re.search(r"#define\s+PPN_ABI_VERSION\s+(\d+)", header).group(1)) == L.ABI_VERSION == L.lib.ppn_version() == 111


def test_upsample2x_bwd_rejects_bad_arguments():
    from ppnet_amd import _lib as L
    f = L.lib.ppn_upsample2x_nhwc_bwd

    def call(dy=P, x=None, dx=P, B=1, H=4, W=4, C=16, dtype=1):
        return f(dy, x, dx, B, H, W, C, dtype, None)
    assert call(dy=None) == E_INVALID and call(dx=None) == E_INVALID
    assert call(dy=None, x=P) == E_INVALID and call(dx=None, x=P) == E_INVALID
    assert call(C=12) == E_INVALID and call(C=0) == E_INVALID and call(C=-8) == E_INVALID
    assert call(dtype=2) == E_INVALID and call(dtype=-1) == E_INVALID
    assert call(B=0) == E_INVALID and call(H=0) == E_INVALID and call(W=0) == E_INVALID
    assert call(B=-1) == E_INVALID and call(H=-2) == E_INVALID and call(W=-3) == E_INVALID
    assert call(B=1 << 20, H=1 << 11) == E_INVALID                          # B (H + 1) block rows >= 2^31
    assert call(W=1 << 20, C=256) == E_INVALID                              # more than 65535 pieces of 256 threads per block row
    assert call(H=1 << 30) == E_INVALID and call(W=1 << 30, C=8) == E_INVALID


def test_upsample2x_concat_bwd_rejects_bad_arguments():
    from ppnet_amd import _lib as L
    f = L.lib.ppn_upsample2x_concat_nhwc_bwd

    def call(n=2, ptrs=(P, P), ch=(16, 8), dout=P, B=1, H=4, W=4, dtype=1):
        xs = (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs) if ptrs is not None else None
        cs = (ctypes.c_int32 * max(1, len(ch)))(*ch) if ch is not None else None
        return f(dout, xs, cs, n, B, H, W, dtype, None)
    assert call(n=0) == E_INVALID and call(n=9, ptrs=(P,) * 9, ch=(8,) * 9) == E_INVALID and call(n=-1) == E_INVALID
    assert call(ptrs=None) == E_INVALID and call(ch=None) == E_INVALID and call(dout=None) == E_INVALID
    assert call(ptrs=(P, None)) == E_INVALID
    assert call(ch=(16, 12)) == E_INVALID and call(ch=(0, 8)) == E_INVALID and call(ch=(-8, 8)) == E_INVALID
    assert call(dtype=2) == E_INVALID and call(dtype=-1) == E_INVALID
    assert call(B=0) == E_INVALID and call(H=0) == E_INVALID and call(W=-3) == E_INVALID
    assert call(B=1 << 20, H=1 << 11) == E_INVALID                          # B (H + 1) block rows >= 2^31
    assert call(W=1 << 20, ch=(256, 8)) == E_INVALID                        # more than 65535 pieces of 256 threads per block row
    assert call(H=1 << 30) == E_INVALID
    assert call(ch=(1 << 30, 1 << 30)) == E_INVALID                         # the channel offsets pass 2^31


def test_resize_concat_bwd_rejects_bad_arguments():
    from ppnet_amd import _lib as L
    f = L.lib.ppn_resize_concat_nhwc_bwd

    def call(n=2, ptrs=(P, P), hw=(8, 8, 2, 2), ch=(16, 8), dout=P, B=1, dtype=1):
        xs = (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs) if ptrs is not None else None
        hs = (ctypes.c_int32 * max(2, len(hw)))(*hw) if hw is not None else None
        cs = (ctypes.c_int32 * max(1, len(ch)))(*ch) if ch is not None else None
        return f(dout, xs, hs, cs, n, B, dtype, None)
    assert call(n=0) == E_INVALID and call(n=-1) == E_INVALID
    assert call(n=9, ptrs=(P,) * 9, hw=(8, 8) * 9, ch=(8,) * 9) == E_INVALID
    assert call(ptrs=None) == E_INVALID and call(hw=None) == E_INVALID and call(ch=None) == E_INVALID and call(dout=None) == E_INVALID
    assert call(ptrs=(P, None)) == E_INVALID
    assert call(ch=(16, 12)) == E_INVALID and call(ch=(0, 8)) == E_INVALID and call(ch=(-8, 8)) == E_INVALID
    assert call(dtype=2) == E_INVALID and call(dtype=-1) == E_INVALID
    assert call(B=0) == E_INVALID and call(B=-4) == E_INVALID
    assert call(hw=(8, 8, 0, 2)) == E_INVALID and call(hw=(0, 8, 2, 2)) == E_INVALID and call(hw=(8, 8, 2, -1)) == E_INVALID
    assert call(hw=(8, 8, 9, 2)) == E_INVALID and call(hw=(8, 8, 2, 16)) == E_INVALID       # a level larger than level 0
    assert call(hw=(1 << 16, 1 << 16, 2, 2)) == E_INVALID                                   # H0 W0 >= 2^31
    assert call(B=1 << 12, hw=(1 << 10, 1 << 10, 2, 2)) == E_INVALID                        # B H0 W0 >= 2^31
    assert call(B=1 << 10, hw=(1 << 10, 1 << 10, 2, 2), ch=(1 << 20, 8)) == E_INVALID        # 2^31 blocks of 256 threads or more
    assert call(ch=(1 << 30, 1 << 30)) == E_INVALID                                         # the channel offsets pass 2^31
