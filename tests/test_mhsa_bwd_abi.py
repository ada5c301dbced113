"""CPU-side checks of ppn_mhsa_bwd (csrc/mhsa_bwd.hip): every bad argument is refused with its code before any HIP call (the
pointers below are never dereferenced); the emitted gfx950 code of every kernel uses no scratch, the bfloat16 kernels run on the
matrix cores and no kernel contains an atomic (the reproducibility claim, checked on the emitted code; hipcc cross-compiles here,
nothing runs); and on the CPU vit.MultiheadAttention with grad enabled is nn.MultiheadAttention bit for bit."""
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


def test_mhsa_bwd_workspace_size():
    from ppnet_amd import _lib
    w = _lib.lib.ppn_mhsa_bwd_workspace
    for B, N, heads in ((1, 1, 1), (2, 197, 12), (64, 1024, 12), (1, 4096, 1)):
        assert w(B, N, heads) >= 2 * B * heads * N
    for bad in ((0, 197, 12), (2, 0, 12), (2, 197, 0), (-1, 197, 12), (2, -5, 12), (2, 197, -12)):
        assert w(*bad) < 0, bad


def test_mhsa_bwd_rejects_bad_arguments_without_gpu():
    from ppnet_amd import _lib
    f = _lib.lib.ppn_mhsa_bwd
    one = C.c_void_p(0x1000)                                   # 16-byte aligned, never dereferenced on these paths
    need = _lib.lib.ppn_mhsa_bwd_workspace(2, 197, 12)
    #     qkv  out  dout dqkv ws   ws_floats B  N    heads hd  scale  dtype stream
    ok = [one, one, one, one, one, need, 2, 197, 12, 64, 0.125, 1, None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    for i in range(5):
        assert call(**{f"a{i}": None}) == E_INVALID, i
    for i in (6, 7, 8):
        assert call(**{f"a{i}": 0}) == E_INVALID and call(**{f"a{i}": -1}) == E_INVALID
    assert call(a9=0) == E_INVALID and call(a9=-64) == E_INVALID
    for s in (0.0, -0.125, float("nan"), float("inf"), float("-inf")):
        assert call(a10=s) == E_INVALID, s
    assert call(a11=2) == E_INVALID and call(a11=-1) == E_INVALID
    assert call(a9=32) == E_UNSUPPORTED and call(a9=128) == E_UNSUPPORTED and call(a9=32, a11=0) == E_UNSUPPORTED
    for i, off in enumerate((8, 2, 4, 12, 4)):                                            # 16-byte alignment of all five buffers
        assert call(**{f"a{i}": C.c_void_p(0x1000 + off)}) == E_INVALID, i
    assert call(a5=need - 1) == E_INVALID and call(a5=0) == E_INVALID and call(a5=-1) == E_INVALID      # a workspace too small
    assert call(a5=need - 1, a11=0) == E_INVALID
    huge = 1 << 62                                                                 # the size is no excuse below: the launch is
    big = 2 ** 31 - 1
    assert call(a6=big, a5=huge) == E_INVALID                                      # 2^31 - 1 workgroups
    assert call(a6=1 << 16, a7=1 << 14, a8=1 << 8, a5=huge) == E_INVALID and call(a6=1 << 16, a7=1 << 14, a8=1 << 8, a5=huge, a11=0) == E_INVALID
    assert call(a6=64, a7=big, a8=1, a5=huge) == E_INVALID


def test_mhsa_bwd_kernels_no_scratch_mfma_and_no_atomics(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not present")
    out = tmp_path / "mhsa_bwd.s"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "mhsa_bwd.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1)
    flags = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize --cuda-device-only -S".split()
    for fl in flags[:-2]:
        assert fl.replace("gfx950", "$(ARCH)") in mk, fl                            # the Makefile's own flags
    subprocess.run([HIPCC, *flags, os.path.join(CSRC, "mhsa_bwd.hip"), "-o", str(out)], check=True, cwd=CSRC, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    asm = out.read_text()
    scratch = dict(re.findall(r"\.amdhsa_kernel (\S+).*?; ScratchSize: (\d+)", asm, re.S))
    assert len(scratch) == 6 and all(int(v) == 0 for v in scratch.values()), scratch
    bodies = dict(re.findall(r"^(_ZN3ppn\d+mhsa_bwd_\w+):[^\n]*\n(.*?)s_endpgm", asm, re.S | re.M))
    assert set(bodies) == set(scratch)
    bf16 = [k for k in bodies if "bf16" in k]
    assert len(bf16) == 3
    for k in bf16:
        assert "v_mfma_f32_16x16x32_bf16" in bodies[k], k
    for k in bf16:
        if "dkdv" in k or "_dq_" in k:
            assert "ds_read_b64_tr_b16" in bodies[k], k
    code = "\n".join(line.split(";")[0] for line in asm.splitlines())                # instructions, comments dropped
    for word in ("global_atomic", "flat_atomic", "buffer_atomic", "ds_add", "ds_cmpst"):
        assert word not in code, word


def test_cpu_module_is_nn_multihead_attention_bit_for_bit():
    """The kernel branch cannot be entered without a GPU: same output, same gradients as calling the wrapped module directly."""
    torch = pytest.importorskip("torch")
    from ppnet_amd import vit
    torch.manual_seed(3)
    m = vit.MultiheadAttention(128, 2)                                             # head dim 64: what the GPU branch takes
    m.train()
    x0 = torch.randn(2, 9, 128)
    ident = torch.randn(2, 9, 128)
    calls = dict(vit.CALLS)

    def run(direct):
        x = x0.clone().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        if direct:
            y = ident + m.attn(x.transpose(0, 1), x.transpose(0, 1), x.transpose(0, 1), need_weights=False)[0].transpose(0, 1)
        else:
            y = m(x, ident)
        (y * torch.linspace(-1, 1, y.numel()).view_as(y)).sum().backward()
        return [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in m.parameters()]
    a, b = run(False), run(True)
    assert len(a) == len(b) == 2 + 4
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert vit.CALLS == calls and "bwd_kernel" in vit.CALLS
    with pytest.raises(RuntimeError, match="GPU only"):
        vit.mhsa_autograd(torch.randn(1, 4, 192, requires_grad=True), 1, 0.125)
