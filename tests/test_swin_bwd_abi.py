"""CPU-side checks of ppn_swin_wmsa_bwd (csrc/swin_wmsa_bwd.hip): the workspace size, every bad argument refused with its code
before any launch (the pointers below are never dereferenced), the emitted gfx950 code of every kernel (no scratch, the bfloat16
kernel on the matrix cores, no atomic instruction: the reproducibility claim, checked on the emitted code; hipcc cross-compiles
here, nothing runs), and on the CPU swin.ShiftWindowMSA with grad enabled is the torch composition bit for bit."""
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


def test_swin_bwd_workspace_size():
    from ppnet_amd import _lib
    w = _lib.lib.ppn_swin_wmsa_bwd_workspace
    for shape in ((1, 1, 1, 1), (256, 64, 64, 4), (2, 15, 23, 5), (1, 8, 8, 32), (1, 7, 7, 65535)):
        assert w(*shape) > 0, shape
    for bad in ((0, 7, 7, 1), (1, 0, 7, 1), (1, 7, 0, 1), (1, 7, 7, 0), (-1, 7, 7, 1), (1, -7, 7, 1), (1, 7, -7, 1), (1, 7, 7, -1)):
        assert w(*bad) < 0, bad


def test_swin_bwd_rejects_bad_arguments_without_gpu():
    from ppnet_amd import _lib
    f = _lib.lib.ppn_swin_wmsa_bwd
    one = C.c_void_p(0x1000)                                   # 16-byte aligned, never dereferenced on these paths
    need = _lib.lib.ppn_swin_wmsa_bwd_workspace(2, 15, 23, 4)
    #     qkv  pad  rpb  dout dqkv dpad drpb ws   ws_floats B  H   W   heads window shift scale  dtype stream
    ok = [one, one, one, one, one, one, one, one, need, 2, 15, 23, 4, 7, 3, 0.125, 1, None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    for i in range(8):                                                             # each of the eight pointers NULL
        assert call(**{f"a{i}": None}) == E_INVALID, i
    for i in (9, 10, 11, 12):                                                      # B, H, W, heads
        assert call(**{f"a{i}": 0}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID, i
    assert call(a12=65536, a8=1 << 62) == E_INVALID
    for s in (0.0, -0.125, float("nan"), float("inf"), float("-inf")):
        assert call(a15=s) == E_INVALID, s
    assert call(a16=2) == E_INVALID and call(a16=-1) == E_INVALID
    for i, off in enumerate((8, 2, 4, 12, 4, 8, 4, 12)):                            # 16-byte alignment of all eight buffers
        assert call(**{f"a{i}": C.c_void_p(0x1000 + off)}) == E_INVALID, i
        assert call(**{f"a{i}": C.c_void_p(0x1000 + off), "a16": 0}) == E_INVALID, i
    assert call(a8=need - 1) == E_INVALID and call(a8=0) == E_INVALID and call(a8=-1) == E_INVALID      # a workspace too small
    assert call(a8=need - 1, a16=0) == E_INVALID
    assert call(a9=1 << 30, a10=1 << 10, a11=1 << 10, a8=1 << 62) == E_INVALID     # B * windows >= 2^31
    assert call(a13=8) == E_UNSUPPORTED and call(a13=8, a14=0) == E_UNSUPPORTED and call(a13=0) == E_UNSUPPORTED
    for sh in (1, 2, 4, 6, -1, 7):
        assert call(a14=sh) == E_UNSUPPORTED, sh


def test_swin_bwd_kernels_no_scratch_mfma_and_no_atomics(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not present")
    out = tmp_path / "swin_wmsa_bwd.s"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "swin_wmsa_bwd.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    flags = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize --cuda-device-only -S".split()
    for fl in flags[:-2]:
        assert fl.replace("gfx950", "$(ARCH)") in mk, fl                            # the Makefile's own flags
    subprocess.run([HIPCC, *flags, os.path.join(CSRC, "swin_wmsa_bwd.hip"), "-o", str(out)], check=True, cwd=CSRC, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    asm = out.read_text()
    scratch = dict(re.findall(r"\.amdhsa_kernel (\S+).*?; ScratchSize: (\d+)", asm, re.S))
    assert len(scratch) == 3 and all(int(v) == 0 for v in scratch.values()), scratch
    bodies = dict(re.findall(r"^(_ZN3ppn\d+swin_wmsa_bwd_\w+):[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M))
    assert set(bodies) == set(scratch)
    bf16 = [k for k in bodies if "bf16" in k]
    assert len(bf16) == 1                                                           # the reduction kernel forms no products
    for k in bf16:
        assert "v_mfma_f32_16x16x32_bf16" in bodies[k], k
        assert "ds_read_b64_tr_b16" in bodies[k], k                                 # K^T, Q^T, dO^T out of the wave's LDS images
    code = "\n".join(line.split(";")[0] for line in asm.splitlines())                # instructions, comments dropped
    for word in ("global_atomic", "flat_atomic", "buffer_atomic", "ds_add", "ds_cmpst"):
        assert word not in code, word
    # The file's only inline assembly is the two waits around the wave's LDS-DMA images (as swin_wmsa.hip): in the emitted code
    # every DMA is followed by `s_waitcnt vmcnt(0)` before any LDS read, and the last transposed read of a window is followed by
    # `s_waitcnt lgkmcnt(0)` before the loop's backward branch, so the next window's DMAs cannot overtake this window's reads.
    src = open(os.path.join(CSRC, "swin_wmsa_bwd.hip")).read()
    assert sorted(re.findall(r'asm volatile\("([^"]*)"', src)) == ["s_waitcnt lgkmcnt(0)", "s_waitcnt vmcnt(0)"]
    body = [l.split(";")[0].strip() for l in bodies[bf16[0]].splitlines()]
    body = [l for l in body if l and not l.endswith(":") and not l.startswith(".")]
    dma = [i for i, l in enumerate(body) if l.startswith("global_load_lds")]
    assert len(dma) == 12, len(dma)                                                 # K, Q, dO images: 4 x 1 KB each
    for i in dma:
        nxt = next(k for k in range(i + 1, len(body)) if body[k].startswith("ds_read") or re.match(r"s_waitcnt.*vmcnt\(0\)", body[k]))
        assert body[nxt].startswith("s_waitcnt"), (i, body[nxt])
    last_tr = max(i for i, l in enumerate(body) if l.startswith("ds_read_b64_tr_b16"))
    nxt = next(k for k in range(last_tr + 1, len(body)) if body[k].startswith("s_cbranch") or re.match(r"s_waitcnt.*lgkmcnt\(0\)", body[k]))
    assert body[nxt].startswith("s_waitcnt"), body[nxt]


def test_cpu_module_is_the_torch_composition_bit_for_bit():
    """The kernel branch cannot be entered without a GPU: same output, same gradients as calling window_attention directly."""
    torch = pytest.importorskip("torch")
    from ppnet_amd import swin
    torch.manual_seed(5)
    m = swin.ShiftWindowMSA(64, 2, 7, shift_size=3)                                 # head dim 32, window 7: what the GPU branch takes
    m.train()
    x0 = torch.randn(2, 9, 11, 64)                                                  # a grid that pads
    calls = dict(swin.TRAIN_CALLS)
    assert set(calls) == {"fwd_kernel", "bwd_kernel"} and set(swin.CALLS) == {"kernel", "torch"}

    def run(direct):
        x = x0.clone().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        w = m.w_msa
        if direct:
            qkv = w.qkv(x.reshape(-1, 64)).view(2, 9, 11, 192)
            o = swin.window_attention(qkv, w.qkv.bias, w.relative_position_bias_table, 2, 3, w.scale, 7)
            y = w.proj(o.reshape(-1, 64)).view(2, 9, 11, 64)
        else:
            y = m(x)
        (y * torch.linspace(-1, 1, y.numel()).view_as(y)).sum().backward()
        return [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in (w.qkv.weight, w.qkv.bias, w.proj.weight, w.proj.bias,
                                                                                w.relative_position_bias_table)]
    a, b = run(False), run(True)
    assert len(a) == len(b) == 7
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert a[-1].abs().sum() > 0 and a[3].abs().sum() > 0
    assert swin.TRAIN_CALLS == calls
    with pytest.raises(RuntimeError, match="GPU only"):
        swin.wmsa_autograd(torch.randn(1, 7, 7, 96, requires_grad=True), torch.zeros(96), torch.zeros(169, 1), 1, 0, 32 ** -0.5)
