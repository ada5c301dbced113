"""CPU-side checks of ppn_gennet_s2_down / ppn_gennet_s2_up / ppn_gennet_s2_wgrad (csrc/gennet_s2_train.hip): header, library, bindings and
the Makefile carry the entry points at ABI 111 with the argument order of the header; the workspace size follows the header's formula;
every bad argument is refused before any HIP call (the pointers below are never dereferenced); the host constants are the kernels'; and
conv_s2 is the library's conv(x), bit for bit, wherever its gate fails."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ppnet_amd", "csrc")
E_INVALID, E_UNSUPPORTED = -1, -3
ONE = C.c_void_p(0x1000)                                       # 16-byte aligned, never dereferenced on these paths
DOWN = ["big", "w", "bias", "small", "B", "H", "W", "C", "dtype", "stream"]
UP = ["small", "w", "bias", "big", "B", "H", "W", "C", "dtype", "stream"]
WGRAD = ["small", "big", "workspace", "dw", "sum_small", "sum_big", "B", "H", "W", "C", "dtype", "stream"]
ENTRIES = (("ppn_gennet_s2_down", DOWN), ("ppn_gennet_s2_up", UP), ("ppn_gennet_s2_wgrad", WGRAD))
NAMES = ("ppn_gennet_s2_tile", "ppn_gennet_s2_max_blocks", "ppn_gennet_s2_wgrad_workspace") + tuple(n for n, _ in ENTRIES)
PART = 24 * 24 * 9 + 2 * 24                                    # floats of one workgroup's partial


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
    for name, want in ENTRIES:
        assert _args(re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, code, re.S).group(1)) == want
        assert _args(re.search(r"\b%s\s*\((.*?)\)\s*\{" % name, capi, re.S).group(1)) == want
        f = getattr(_lib.lib, name)
        assert len(f.argtypes) == len(want) and f.restype is C.c_int
    assert _args(re.search(r"int64_t\s+ppn_gennet_s2_wgrad_workspace\s*\((.*?)\)\s*;", code, re.S).group(1)) == ["B", "Hs", "Ws"]
    assert _lib.lib.ppn_gennet_s2_wgrad_workspace.restype is C.c_int64
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "gennet_s2_train.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    text = open(os.path.join(CSRC, "gennet_s2_train.hip")).read()
    for kernel in ("s2_down_kernel", "s2_up_kernel", "s2_wgrad_kernel", "s2_wgrad_finish_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\b" % kernel, text), kernel
    assert "atomic" not in text.split("namespace ppn {", 1)[1].replace("no atomics", "").replace("without atomics", "")
    doc = re.search(r"/\* The training kernels of GenNet's 24 -> 24 stride-2 stages.*?\*/", header, re.S).group(0)
    for piece in ("w[o][c][ky][kx]", "w[a][c][ky][kx]", "dw[a][c][ky][kx]", "[out][in][3][3]", "[in][out][3][3]", "ppn_gennet_s2_tile()",
                  "ppn_gennet_s2_max_blocks()"):
        assert piece in doc, piece


def test_workspace_follows_the_header_formula():
    from ppnet_amd import _lib, fused
    f, tile, cap = _lib.lib.ppn_gennet_s2_wgrad_workspace, _lib.lib.ppn_gennet_s2_tile(), _lib.lib.ppn_gennet_s2_max_blocks()
    for B, Hs, Ws in ((1, 1, 1), (1, 7, 73), (1, 512, 1), (1, 27, 19), (2, 16, 16), (64, 112, 112), (8, 256, 256), (1, 513, 513), (3, 5, 7),
                      (1, 512, 512), (1, 512, 513), (1, 768, 512), (1, 628, 628), (2, 600, 600)):
        want = PART * 4 * min(-(-(B * Hs * Ws) // tile), cap)
        assert f(B, Hs, Ws) == want == fused.s2_wgrad_workspace_bytes(B, Hs, Ws), (B, Hs, Ws)
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, 1 << 15, 1 << 13), (1 << 10, 1 << 10, 1 << 8),
                (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 1, 1)):
        assert f(*bad) < 0, bad


def _caller(f, ok):
    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    return call


def _common_refusals(call, b):
    """Extents, widths, data types and counts: argument b is B, then H, W, C, dtype."""
    for i in range(b, b + 4):
        assert call(**{f"a{i}": 0}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID and call(**{f"a{i}": -(2 ** 31)}) == E_INVALID, i
    for width in (8, 16, 32, 12, 23, 25, 48, 96, 1, 2 ** 31 - 1):
        assert call(**{f"a{b + 3}": width}) == E_UNSUPPORTED, width
    for d in (2, -1, 7):
        assert call(**{f"a{b + 4}": d}) == E_INVALID, d
    B, H, W = (f"a{b + k}" for k in range(3))
    assert call(**{B: 1, H: 1 << 14, W: 1 << 13}) == E_INVALID                             # 24 B H W >= 2^31
    assert call(**{B: 1 << 10, H: 1 << 10, W: 1 << 8}) == E_INVALID
    assert call(**{B: 2 ** 31 - 1, H: 2 ** 31 - 1, W: 2 ** 31 - 1}) == E_INVALID
    assert call(**{B: 2 ** 31 - 1, H: 1, W: 1}) == E_INVALID
    assert call(**{B: 1, H: 1, W: 2 ** 31 - 1}) == E_INVALID
    assert call(**{B: 89478486, H: 1, W: 1}) == E_INVALID                                  # 24 B = 2^31 + 16


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("name,names", ENTRIES[:2])
def test_down_and_up_reject_bad_arguments_without_gpu(name, names, dtype):
    from ppnet_amd import _lib
    #                                          4 pointers  B  H  W  C   dtype  stream
    call = _caller(getattr(_lib.lib, name), [ONE] * 4 + [2, 7, 5, 24, dtype, None])
    for i in (0, 1, 3):                                                                    # bias may be NULL, the others not
        assert call(**{f"a{i}": None}) == E_INVALID, names[i]
        assert call(**{f"a{i}": None, "a2": None}) == E_INVALID, names[i]
        for off in (8, 4, 2, 1):                                                           # 16 bytes
            assert call(**{f"a{i}": C.c_void_p(0x1000 + off)}) == E_INVALID, (names[i], off)
    for off in (2, 1, 3):                                                                  # bias: 4 bytes
        assert call(a2=C.c_void_p(0x1000 + off)) == E_INVALID, off
    _common_refusals(call, 4)


@pytest.mark.parametrize("dtype", [0, 1])
def test_wgrad_rejects_bad_arguments_without_gpu(dtype):
    from ppnet_amd import _lib
    #                                                  6 pointers  B  H  W  C   dtype  stream
    call = _caller(_lib.lib.ppn_gennet_s2_wgrad, [ONE] * 6 + [2, 7, 5, 24, dtype, None])
    for i in range(4):                                                                     # sum_small and sum_big may be NULL
        assert call(**{f"a{i}": None}) == E_INVALID, WGRAD[i]
        assert call(**{f"a{i}": None, "a4": None, "a5": None}) == E_INVALID, WGRAD[i]
        for off in (8, 4, 2, 1):
            assert call(**{f"a{i}": C.c_void_p(0x1000 + off)}) == E_INVALID, (WGRAD[i], off)
    for i in (4, 5):
        for off in (2, 1, 3):                                                              # the sums: 4 bytes
            assert call(**{f"a{i}": C.c_void_p(0x1000 + off)}) == E_INVALID, (WGRAD[i], off)
    _common_refusals(call, 6)


def test_host_constants_are_the_kernels():
    torch = pytest.importorskip("torch")
    from ppnet_amd import _lib, fused
    src = open(os.path.join(CSRC, "gennet_s2_train.hip")).read()
    const = {k: v for k, v in re.findall(r"constexpr int (S2_\w+) = ([^;]+);", src)}
    assert int(const["S2_THREADS"]) == 256 and int(const["S2_PPT"]) * int(const["S2_THREADS"]) == int(const["S2_TILE"])
    assert int(const["S2_TILE"]) == fused.S2_TILE == _lib.lib.ppn_gennet_s2_tile() == 512
    assert int(const["S2_MAX_BLOCKS"]) == fused.S2_MAX_BLOCKS == _lib.lib.ppn_gennet_s2_max_blocks() == 768
    assert int(const["S2_C"]) == fused.S2_CHANNELS == 24 and int(const["S2_PART"]) == PART and int(const["S2_DW"]) == 24 * 24 * 9
    assert int(const["S2_TILE"]) % int(const["S2_CHUNK"]) == 0 and int(const["S2_PART"]) % 16 == 0
    assert fused.S2_CALLS.keys() == {"down", "up", "wgrad"} and isinstance(fused.S2_RECORD_MIN, int) and torch.float32 in fused.S2_DTYPES
    kernels_h = open(os.path.join(CSRC, "ppn_kernels.h")).read()
    for name in ("gennet_s2_tile", "gennet_s2_max_blocks", "gennet_s2_wgrad_workspace_bytes", "gennet_s2_down_launch", "gennet_s2_up_launch",
                 "gennet_s2_wgrad_launch"):
        assert re.search(r"\b%s\s*\(" % name, kernels_h), name


def test_conv_s2_is_the_library_wherever_the_gate_fails(monkeypatch):
    torch = pytest.importorskip("torch")
    nn = torch.nn
    from ppnet_amd import fused
    monkeypatch.delenv("PPNET_LIBRARY_S2", raising=False)
    monkeypatch.setattr(fused, "S2_RECORD_MIN", 0)                                          # the measured gates: opened, the others are tested
    monkeypatch.setattr(fused, "S2_DTYPES", frozenset({torch.float32, torch.bfloat16}))
    assert not fused.library_s2()
    calls = dict(fused.S2_CALLS)
    g = torch.Generator().manual_seed(0)

    class SubConv(nn.Conv2d):
        pass

    class SubConvT(nn.ConvTranspose2d):
        pass
    layers = [nn.Conv2d(24, 24, 3, 2, 1), nn.ConvTranspose2d(24, 24, 3, 2, 1, output_padding=1),          # CPU tensors
              nn.Conv2d(16, 16, 3, 2, 1), nn.Conv2d(24, 32, 3, 2, 1), nn.ConvTranspose2d(32, 32, 3, 2, 1, output_padding=1),
              nn.Conv2d(24, 24, 3, 1, 1), nn.Conv2d(24, 24, 3, 2, 0), nn.Conv2d(24, 24, 3, 2, 1, dilation=2), nn.Conv2d(24, 24, 3, 2, 1, groups=2),
              nn.Conv2d(24, 24, 5, 2, 2), nn.Conv2d(24, 24, 3, 2, 1, padding_mode="reflect"),
              nn.ConvTranspose2d(24, 24, 3, 2, 1, output_padding=0), nn.ConvTranspose2d(24, 24, 3, 1, 1), nn.ConvTranspose2d(24, 24, 3, 2, 0, output_padding=1),
              SubConv(24, 24, 3, 2, 1), SubConvT(24, 24, 3, 2, 1, output_padding=1)]
    for conv in layers:
        x = torch.randn(2, conv.in_channels, 6, 5, generator=g, requires_grad=True)
        assert not fused.conv_s2_ok(x, conv), conv
        assert torch.equal(fused.conv_s2(x, conv), conv(x)), conv
    assert fused.S2_CALLS == calls                                                          # nothing was launched

    class Fake:                                                                            # what the predicate reads of a CUDA tensor
        is_cuda, dtype, device, requires_grad = True, torch.float32, torch.device("cpu"), True

        def __init__(self, *shape):
            self.shape = shape

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return True
    ok = Fake(2, 24, 6, 5)
    assert fused.conv_s2_ok(ok, layers[0]) and fused.conv_s2_ok(ok, layers[1])              # the gate itself opens for the two layer types
    for conv in layers[2:]:
        assert not fused.conv_s2_ok(Fake(2, conv.in_channels, 6, 5), conv), conv
    assert not fused.conv_s2_ok(Fake(2, 24, 6), layers[0]) and not fused.conv_s2_ok(Fake(1, 24, 1 << 14, 1 << 13), layers[0])
    assert fused.conv_s2_ok(Fake(1, 24, 1 << 13, 1 << 13), layers[0]) and not fused.conv_s2_ok(Fake(1, 24, 1 << 13, 1 << 13), layers[1])
    with torch.no_grad():
        assert not fused.conv_s2_ok(ok, layers[0])                                          # nothing records
    half = nn.Conv2d(24, 24, 3, 2, 1).double()
    assert not fused.conv_s2_ok(ok, half)                                                   # float32 parameters only
    monkeypatch.setattr(fused, "S2_RECORD_MIN", 2 * 24 * 6 * 5 + 1)
    assert not fused.conv_s2_ok(ok, layers[0]) and fused.conv_s2_ok(ok, layers[1])          # the ConvTranspose2d's big side is its output
    monkeypatch.setattr(fused, "S2_RECORD_MIN", 0)
    monkeypatch.setattr(fused, "S2_DTYPES", frozenset({torch.bfloat16}))
    assert not fused.conv_s2_ok(ok, layers[0])
    monkeypatch.setattr(fused, "S2_DTYPES", frozenset({torch.float32}))
    hooked = nn.Conv2d(24, 24, 3, 2, 1)
    hooked.register_forward_hook(lambda *a: None)
    assert not fused.conv_s2_ok(ok, hooked)                                                 # a hook watches the module's own call
    monkeypatch.setenv("PPNET_LIBRARY_S2", "1")
    assert fused.library_s2() and not fused.conv_s2_ok(ok, layers[0]) and not fused.conv_s2_ok(ok, layers[1])
    x = torch.randn(2, 24, 6, 5, generator=g, requires_grad=True)
    assert torch.equal(fused.conv_s2(x, layers[0]), layers[0](x)) and fused.S2_CALLS == calls


def test_aevit_on_the_cpu_is_unchanged():
    """A CPU AE-ViT in train mode: the forward through _run_stage is the stages' own composition, bit for bit."""
    torch = pytest.importorskip("torch")
    from ppnet_amd import fused
    from ppnet_amd.gennet import AEViT
    torch.manual_seed(0)
    m = AEViT(1, 1, 56, 24).train()
    for blk in m.vit_blocks:
        blk.drop_path_rate = 0.0
    x = torch.randn(2, 1, 56, 56)
    calls = dict(fused.S2_CALLS)
    import copy
    m2 = copy.deepcopy(m)
    got = m(x)
    t = m2.conv_first(x)
    for blk in m2.enc_conv:
        t = blk(t)
    B, Cc, H, W = t.shape
    t = m2.vit_blocks(t.flatten(2).transpose(1, 2)).transpose(1, 2).reshape(B, Cc, H, W)
    for blk in m2.dec_conv:
        t = blk(t)
    assert torch.equal(got, m2.conv_final(t)) and fused.S2_CALLS == calls
