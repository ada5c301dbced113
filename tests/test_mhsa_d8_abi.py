"""CPU-side checks of ppn_mhsa_fwd / ppn_mhsa_bwd at head dim 8 (csrc/mhsa_d8.hip): head dim 8 passes the head-dim gate and then
meets every remaining check (alignment, workspace size, N, launch size) with PPN_E_INVALID before any HIP call (the pointers below
are never dereferenced); every other head dim but 64 stays PPN_E_UNSUPPORTED; the new source is in the Makefile's SRCS,
cross-compiles with the Makefile's flags for gfx950 and no kernel of it uses scratch; and on the CPU AEViT in train mode is what it
was bit for bit (the kernel branch cannot be entered without a GPU)."""
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
ONE = C.c_void_p(0x1000)                                       # 16-byte aligned, never dereferenced on these paths
SCALE = 8 ** -0.5


def _caller(f, ok):
    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    return call


@pytest.mark.parametrize("dtype", [0, 1])
def test_mhsa_bwd_head_dim_8_meets_the_remaining_checks(dtype):
    from ppnet_amd import _lib
    need = _lib.lib.ppn_mhsa_bwd_workspace(2, 784, 3)
    assert need >= 2 * 2 * 3 * 784
    #                                   qkv  out  dout dqkv ws   ws_floats B  N    heads hd scale  dtype stream
    call = _caller(_lib.lib.ppn_mhsa_bwd, [ONE, ONE, ONE, ONE, ONE, need, 2, 784, 3, 8, SCALE, dtype, None])
    # on a build without the head-dim-8 kernels these two return PPN_E_UNSUPPORTED: the head-dim gate comes before them
    for i, off in enumerate((8, 2, 4, 12, 4)):                                            # 16-byte alignment of all five buffers
        assert call(**{f"a{i}": C.c_void_p(0x1000 + off)}) == E_INVALID, i
    assert call(a5=need - 1) == E_INVALID                                                 # a workspace one float short
    assert call(a5=0) == E_INVALID and call(a5=-1) == E_INVALID
    assert call(a7=0) == E_INVALID and call(a7=-1) == E_INVALID                            # N
    assert call(a6=0) == E_INVALID and call(a8=0) == E_INVALID
    for i in range(5):
        assert call(**{f"a{i}": None}) == E_INVALID, i
    for s in (0.0, -SCALE, float("nan"), float("inf")):
        assert call(a10=s) == E_INVALID, s
    assert call(a11=2) == E_INVALID
    huge = 1 << 62                                                                        # the size is no excuse below: the launch is
    big = 2 ** 31 - 1
    assert call(a6=big, a7=1, a8=1, a5=huge) == E_INVALID                                 # 2^31 - 1 workgroups: >= 2^31 work-items
    assert call(a6=1 << 16, a7=1 << 14, a8=1 << 8, a5=huge) == E_INVALID
    assert call(a6=64, a7=big, a8=1, a5=huge) == E_INVALID
    for hd in (16, 32, 128):
        assert call(a9=hd) == E_UNSUPPORTED, hd
        assert call(a9=hd, a0=C.c_void_p(0x1008)) == E_UNSUPPORTED, hd                     # the head-dim gate comes first
    assert call(a9=0) == E_INVALID and call(a9=-8) == E_INVALID


@pytest.mark.parametrize("dtype", [0, 1])
def test_mhsa_fwd_head_dim_8_meets_the_remaining_checks(dtype):
    from ppnet_amd import _lib
    #                                   qkv  out  B  N    heads hd scale  dtype stream
    call = _caller(_lib.lib.ppn_mhsa_fwd, [ONE, ONE, 2, 784, 3, 8, SCALE, dtype, None])
    for i, off in enumerate((8, 4)):
        assert call(**{f"a{i}": C.c_void_p(0x1000 + off)}) == E_INVALID, i                 # PPN_E_UNSUPPORTED without the feature
    assert call(a3=0) == E_INVALID and call(a3=-1) == E_INVALID
    assert call(a0=None) == E_INVALID and call(a1=None) == E_INVALID
    big = 2 ** 31 - 1
    assert call(a2=big, a3=1, a4=1) == E_INVALID
    assert call(a2=1 << 16, a3=1 << 14, a4=1 << 8) == E_INVALID
    assert call(a2=64, a3=big, a4=1) == E_INVALID
    for hd in (16, 32, 128):
        assert call(a5=hd) == E_UNSUPPORTED, hd
        assert call(a5=hd, a0=C.c_void_p(0x1008)) == E_UNSUPPORTED, hd


def test_mhsa_d8_source_is_built_and_uses_no_scratch(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not present")
    out = tmp_path / "mhsa_d8.s"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "mhsa_d8.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    flags = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fno-slp-vectorize --cuda-device-only -S".split()
    for fl in flags[:-2]:
        assert fl.replace("gfx950", "$(ARCH)") in mk, fl                            # the Makefile's own flags
    subprocess.run([HIPCC, *flags, os.path.join(CSRC, "mhsa_d8.hip"), "-o", str(out)], check=True, cwd=CSRC, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    asm = out.read_text()
    scratch = dict(re.findall(r"\.amdhsa_kernel (\S+).*?; ScratchSize: (\d+)", asm, re.S))
    # forward, statistics, dK / dV and dQ, each for float32 and bfloat16
    assert len(scratch) == 8 and all("mhsa_d8_" in k for k in scratch), scratch
    for part in ("fwd", "stats", "dkdv", "dq"):
        assert sum(f"mhsa_d8_{part}_kernel" in k for k in scratch) == 2, part
    assert all(int(v) == 0 for v in scratch.values()), scratch


def test_cpu_aevit_training_is_the_library_path_bit_for_bit(monkeypatch):
    """Without a GPU the kernel branch cannot be entered: AEViT in train mode gives the output and every gradient that the
    library's attention gives (the knob forces that path), and no launch is counted."""
    torch = pytest.importorskip("torch")
    from ppnet_amd import gennet, vit
    assert gennet.mhsa_autograd is vit.mhsa_autograd                               # imported at module level
    torch.manual_seed(5)
    m = gennet.AEViT(1, 1, 64, 24).train()
    for blk in m.vit_blocks:
        blk.drop_path_rate = 0.0
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x0 = torch.rand(2, 1, 64, 64)
    calls = dict(vit.CALLS)

    def run():
        m.load_state_dict(sd)                                                      # BatchNorm's running statistics back too
        m.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = m(x)
        (y * torch.linspace(-1, 1, y.numel()).view_as(y)).sum().backward()
        return [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in m.parameters()]
    a = run()
    monkeypatch.setenv("PPNET_LIBRARY_ATTENTION", "1")
    b = run()
    monkeypatch.delenv("PPNET_LIBRARY_ATTENTION")

    def sdpa_forward(self, x):                                                     # the module's forward before the kernel branch
        import torch.nn.functional as F
        B, N, Cc = x.shape
        q, k, v = self.qkv(x).view(B, N, 3, self.num_heads, Cc // self.num_heads).permute(2, 0, 3, 1, 4)
        o = F.scaled_dot_product_attention(q, k, v, scale=self.scale)
        return self.proj(o.transpose(1, 2).reshape(B, N, Cc))
    monkeypatch.setattr(gennet._Attention, "forward", sdpa_forward)
    c = run()
    assert len(a) == len(b) == len(c) == 2 + len(list(m.parameters()))
    for u, v, w in zip(a, b, c):
        assert torch.equal(u, v) and torch.equal(u, w)
    assert vit.CALLS == calls
    with pytest.raises(RuntimeError, match="GPU only"):
        vit.mhsa_autograd(torch.randn(1, 4, 72, requires_grad=True), 3, SCALE)
    assert sorted(k for k in m.state_dict() if "attn" in k and k.startswith("vit_blocks.0.")) == [
        "vit_blocks.0.attn.proj.bias", "vit_blocks.0.attn.proj.weight", "vit_blocks.0.attn.qkv.bias", "vit_blocks.0.attn.qkv.weight"]
