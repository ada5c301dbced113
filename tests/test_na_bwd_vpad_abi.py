"""CPU-side checks of ppn_na2d_bwd_vpad (csrc/na2d_bwd.hip): header, library and bindings carry the two new entry points at ABI
111, the workspace size follows the header's formula, and every bad argument is refused with PPN_E_INVALID before any HIP call
(the pointers below are never dereferenced)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
NAMES = ("ppn_na2d_bwd_vpad", "ppn_na2d_bwd_vpad_workspace")


def _regions(H, W, d):
    hs, ws = -(-H // d), -(-W // d)
    return -(-hs // 8) * -(-ws // 8) * d * d


def test_header_library_and_bindings_carry_the_entry_points_at_abi_111():
    from ppnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "ppnet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert int(re.search(r"#define\s+PPN_ABI_VERSION\s+(\d+)", header).group(1)) == 111
    assert _lib.ABI_VERSION == 111 and _lib.lib.ppn_version() == 111
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in _lib.EXPORTS and hasattr(_lib.lib, n), n
    # the argument list the issue fixes: pointers, the workspace size, the padded grid before the real one (ppn_na2d_fwd_vpad's order)
    decl = re.search(r"int\s+ppn_na2d_bwd_vpad\s*\((.*?)\)\s*;", code, re.S).group(1)
    args = [a.split()[-1].lstrip("*") for a in decl.split(",")]
    assert args == ["qkv", "pad_kv", "rpb", "dout", "dqkv", "dpad_kv", "drpb", "workspace", "workspace_floats", "B", "H", "W", "Hr", "Wr", "heads",
                    "dilation", "scale", "dtype", "stream"]
    decl = re.search(r"int64_t\s+ppn_na2d_bwd_vpad_workspace\s*\((.*?)\)\s*;", code, re.S).group(1)
    assert [a.split()[-1] for a in decl.split(",")] == ["B", "H", "W", "Hr", "Wr", "heads", "dilation"]
    # the materialised entry keeps its signature and its results
    assert _lib.lib.ppn_na2d_bwd_workspace(2, 19, 23, 2, 1) == 2 * 2 * 19 * 23 * 4 + 3 * 3 * 2 * 2 * 169
    assert len(_lib.lib.ppn_na2d_bwd.argtypes) == 15 and len(_lib.lib.ppn_na2d_bwd_vpad.argtypes) == 19


def test_workspace_size():
    from ppnet_amd import _lib
    w, w0 = _lib.lib.ppn_na2d_bwd_vpad_workspace, _lib.lib.ppn_na2d_bwd_workspace
    #             B  H    W    Hr  Wr  heads d
    for shape in ((2, 14, 14, 9, 10, 2, 2), (1, 21, 21, 2, 20, 1, 3), (2, 112, 112, 56, 56, 1, 16), (1, 40, 14, 40, 9, 1, 2), (1, 7, 7, 1, 1, 65535, 1)):
        B, H, W, Hr, Wr, heads, d = shape
        # statistics of the REAL queries (a float4 each) + 169 + 2 x 32 partial sums per (region of the padded grid, head)
        assert w(*shape) == 4 * B * heads * Hr * Wr + 233 * heads * B * _regions(H, W, d), shape
    # no padding: at least the statistics part of the materialised kernel's workspace (and its partial sums grow by 64 per region)
    B, H, W, heads, d = 1, 16, 16, 2, 2
    stats = 4 * B * heads * H * W
    assert w0(B, H, W, heads, d) == stats + 169 * heads * B * _regions(H, W, d)
    assert w(B, H, W, H, W, heads, d) >= stats
    assert w(B, H, W, H, W, heads, d) == stats + 233 * heads * B * _regions(H, W, d)
    assert w(1, 14, 14, 15, 7, 1, 2) < 0 and w(1, 14, 14, 7, 15, 1, 2) < 0                      # Hr > H, Wr > W
    assert w(1, 13, 14, 7, 7, 1, 2) < 0 and w(1, 14, 13, 7, 7, 1, 2) < 0                        # H, W < 7 * dilation
    for bad in ((0, 14, 14, 7, 7, 1, 2), (1, 14, 14, 0, 7, 1, 2), (1, 14, 14, 7, 0, 1, 2), (1, 14, 14, 7, 7, 0, 2), (-1, 14, 14, 7, 7, 1, 2),
                (1, 14, 14, -7, 7, 1, 2), (1, 14, 14, 7, -7, 1, 2), (1, 14, 14, 7, 7, -1, 2), (1, 14, 14, 7, 7, 1, 0), (1, 14, 14, 7, 7, 65536, 2)):
        assert w(*bad) < 0, bad
    assert w(1 << 20, 1 << 10, 1 << 10, 8, 8, 1, 1) < 0                                         # 2^34 regions
    assert w(1 << 17, 1 << 10, 1 << 10, 8, 8, 1, 1) < 0                                         # exactly 2^31 regions
    assert w((1 << 17) - 1, 1 << 10, 1 << 10, 8, 8, 1, 1) > 0


def test_rejects_bad_arguments_without_gpu():
    from ppnet_amd import _lib
    f = _lib.lib.ppn_na2d_bwd_vpad
    one = C.c_void_p(0x1000)                                   # 16-byte aligned, never dereferenced on these paths
    need = _lib.lib.ppn_na2d_bwd_vpad_workspace(2, 14, 14, 9, 10, 2, 2)
    #     qkv  pad  rpb  dout dqkv dpad drpb ws   ws_floats B  H   W   Hr Wr  heads dil scale dtype stream
    ok = [one, one, one, one, one, one, one, one, need, 2, 14, 14, 9, 10, 2, 2, 0.125, 1, None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    for i in range(8):                                                             # each of the eight pointers NULL
        assert call(**{f"a{i}": None}) == E_INVALID, i
    for i in (9, 12, 13, 14):                                                      # B, Hr, Wr, heads
        assert call(**{f"a{i}": 0}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID, i
    assert call(a12=15) == E_INVALID and call(a13=15) == E_INVALID                 # Hr > H, Wr > W
    assert call(a12=15, a8=1 << 62) == E_INVALID and call(a13=15, a8=1 << 62) == E_INVALID
    assert call(a10=13) == E_INVALID and call(a11=13) == E_INVALID                 # H, W < 7 * dilation
    assert call(a15=3, a8=1 << 62) == E_INVALID and call(a15=0) == E_INVALID and call(a15=-2) == E_INVALID
    assert call(a14=65536, a8=1 << 62) == E_INVALID
    for s in (0.0, -0.125, float("nan"), float("inf"), float("-inf")):
        assert call(a16=s) == E_INVALID, s
    assert call(a17=2) == E_INVALID and call(a17=-1) == E_INVALID
    for i, off in enumerate((8, 2, 4, 12, 4, 8, 4, 12)):                            # 16-byte alignment of all eight buffers
        assert call(**{f"a{i}": C.c_void_p(0x1000 + off)}) == E_INVALID, i
        assert call(**{f"a{i}": C.c_void_p(0x1000 + off), "a17": 0}) == E_INVALID, i
    assert call(a8=need - 1) == E_INVALID and call(a8=0) == E_INVALID and call(a8=-1) == E_INVALID      # a workspace too small
    assert call(a8=need - 1, a17=0) == E_INVALID
    assert call(a9=1 << 17, a10=1 << 10, a11=1 << 10, a15=1, a8=1 << 62) == E_INVALID                   # 2^31 workgroups
