"""DiNAT-L and NAT-Mini on the HIP path: the GEMM seam (ppn_nat_gemm_bf16 at the shapes DiNAT-L's level 2 and NAT-Mini's levels 2-3
produce — K or N of 768 / 1536, three row-statistic partials), the level-3 gate (C = 1536 stays off ppn_nat_gemm_bf16 / ppn_row_stats_bf16),
and whole networks at DiNAT-L's and NAT-Mini's widths, bfloat16 prepared against float32 unprepared, each held to twice what its
base-width twin — which runs code this width change does not touch — shows in the same test."""
import copy

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------------------------------------ GEMM seam
def _ops(M, N, K, seed):                                                     # tests/test_gpu_natgemm.py's operands
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = (torch.randn(M, K, device="cuda", generator=g) * 1.3 + 0.4).to(torch.bfloat16)
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    b = torch.randn(N, device="cuda", generator=g) * 0.5
    return a, w, b


LN_SHAPES = [  # (mode, N, K) at M = 512
    ("ln", 2304, 768), ("ln_gelu", 1536, 768),                               # DiNAT-L level 2: qkv, fc1
    ("ln_gelu", 768, 256), ("ln_gelu", 1536, 512)]                           # NAT-Mini levels 2, 3: fc1 at mlp_ratio 3
ACC_SHAPES = [(768, 768), (768, 1536), (256, 768), (512, 1536)]              # (N, K): DiNAT-L level 2 proj, fc2; NAT-Mini fc2


@pytest.mark.parametrize("partials", ["row_stats", "tile_columns"])
@pytest.mark.parametrize("mode,N,K", LN_SHAPES)
def test_ln_folded_projection_vs_float64(mode, N, K, partials):
    """Modes "ln" / "ln_gelu" against the float64 definition on the same bfloat16 operands, with test_gpu_natgemm.py's tolerance for
    these modes.  The row statistics come in one partial (ppn_row_stats_bf16: a level's first layer) or in nat_partials(K) partials,
    one per tile column of the stream, as the accumulating GEMM in front leaves them (3 at K = 768)."""
    from ppnet_amd import fused
    M = 512
    a, w0, b0 = _ops(M, N, K, 1)
    g = torch.Generator(device="cuda").manual_seed(2)
    gamma = 1.0 + 0.2 * torch.randn(K, device="cuda", generator=g)
    beta = 0.1 * torch.randn(K, device="cuda", generator=g)
    w = (w0.float() * gamma).to(torch.bfloat16).contiguous()
    bias = (b0 + w0.float() @ beta).contiguous()
    colsum = w.float().sum(1).contiguous()
    ad = a.double()
    if partials == "row_stats":
        stats = fused.row_stats(a)
        assert torch.allclose(stats[0, :, 0].double(), ad.sum(1), rtol=1e-5, atol=1e-3)
        assert torch.allclose(stats[0, :, 1].double(), (ad * ad).sum(1), rtol=1e-5, atol=1e-3)
    else:
        P = fused.nat_partials(K)
        assert P == {256: 2, 512: 2, 768: 3}[K]
        cols = a.float().view(M, P, K // P)
        stats = torch.stack([cols.sum(2), (cols * cols).sum(2)], dim=2).permute(1, 0, 2).contiguous()    # [P, M, 2]
    out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    fused.nat_gemm(a, w, bias, mode, out, colsum=colsum, stats_in=stats, eps=1e-5)
    mean = ad.mean(1, keepdim=True)
    var = ad.var(1, unbiased=False, keepdim=True)
    ref = ((ad - mean) / torch.sqrt(var + 1e-5)) @ w.double().t() + bias.double()
    if mode == "ln_gelu":
        ref = F.gelu(ref)
    err = (out.double() - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + 4e-3                      # one bf16 rounding + accumulation / the logistic erf fit (3e-5)
    print(f"{mode} N {N} K {K} {partials}: max err {float(err.max()):.3e}, max (err - tol) {float((err - tol).max()):.3e}, mean err {float(err.mean()):.3e}")
    assert bool((err <= tol).all()), float((err - tol).max())
    assert float(err.mean()) < 2.5e-3 * float(ref.abs().mean() + 0.05)
    out2 = torch.empty_like(out)
    fused.nat_gemm(a, w, bias, mode, out2, colsum=colsum, stats_in=stats, eps=1e-5)
    assert torch.equal(out, out2)


@pytest.mark.parametrize("N,K", ACC_SHAPES)
def test_accumulating_projection_and_row_partials(N, K):
    """Mode "acc" against float64 with test_gpu_natgemm.py's tolerance; the row partials per tile column (3 at N = 768)."""
    from ppnet_amd import fused
    M = 512
    a, w, b = _ops(M, N, K, 3)
    g = torch.Generator(device="cuda").manual_seed(4)
    s0 = (torch.randn(M, N, device="cuda", generator=g) * 2.0).to(torch.bfloat16)
    s = s0.clone()
    P = fused.nat_partials(N)
    assert P == {256: 2, 512: 2, 768: 3}[N]
    st = torch.full((P, M, 2), float("nan"), dtype=torch.float32, device="cuda")
    fused.nat_gemm(a, w, b, "acc", s, stats_out=st)
    ref = s0.double() + a.double() @ w.double().t() + b.double()
    err = (s.double() - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + 2e-3
    print(f"acc N {N} K {K}: max err {float(err.max()):.3e}, max (err - tol) {float((err - tol).max()):.3e}")
    assert bool((err <= tol).all()), float((err - tol).max())
    sd = s.double().view(M, P, N // P)
    assert torch.allclose(st[:, :, 0].double().t(), sd.sum(2), rtol=1e-5, atol=2e-3)
    assert torch.allclose(st[:, :, 1].double().t(), (sd * sd).sum(2), rtol=1e-5, atol=2e-3)
    s2 = s0.clone()
    st2 = torch.empty_like(st)
    fused.nat_gemm(a, w, b, "acc", s2, stats_out=st2)
    assert torch.equal(s, s2) and torch.equal(st, st2)


# ------------------------------------------------------------------------------------------------ the level-3 gate
def _block_error(C, heads, seed):
    """A folded bfloat16 one-layer NATBlock on a (4, 8, 8, C) stream against the same block unfolded in float32: (folded block,
    relative RMS error of the returned stream)."""
    from ppnet_amd import segnet
    torch.manual_seed(seed)
    blk32 = segnet.randomize_neutral_parameters(segnet.NATBlock(C, 1, heads, 7, None, downsample=False, mlp_ratio=2.0), seed=seed).eval().to(DEV)
    x = torch.randn(4, 8, 8, C, device=DEV)
    blk16 = copy.deepcopy(blk32).to(torch.bfloat16).fold()
    with torch.no_grad():
        y32, _ = blk32(x)
        ok = blk16._ln_folded_ok(x.to(torch.bfloat16))
        y16, _ = blk16(x.to(torch.bfloat16))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y16).all())
    d = (y16.float() - y32)
    return ok, float(d.pow(2).mean().sqrt() / y32.pow(2).mean().sqrt())


def test_level3_of_dinat_l_takes_the_per_layer_path(monkeypatch):
    """C = 1536 is outside ppn_row_stats_bf16 (C <= 1024) and ppn_nat_gemm_bf16 (6 partials > 4): _ln_folded_ok says no — with the
    tile-count gate opened, so that the width alone decides — and the level runs on the LayerNorm kernel + accumulating GEMM without a
    PpnError.  Its error against float32 stays within twice that of the 1024-wide block (DiNAT-B's level 3), which does fold."""
    monkeypatch.setenv("PPNET_SMALL_GEMM_TILES", "1")
    ok_b, err_b = _block_error(1024, 32, 5)
    ok_l, err_l = _block_error(1536, 48, 5)
    print(f"one-layer block bf16 folded vs fp32: C 1024 on ppn_nat_gemm_bf16 {ok_b}, rel RMS {err_b:.3e}; C 1536 {ok_l}, rel RMS {err_l:.3e}")
    assert ok_b and not ok_l
    assert err_l <= 2.0 * err_b


# ------------------------------------------------------------------------------------------------ whole networks
def _codes(B, R, seed):
    g = torch.Generator().manual_seed(seed)
    lo = (torch.rand(B, 1, R // 16, R // 16, generator=g) > 0.4).float()
    return (F.interpolate(lo, size=(R, R), mode="nearest")[:, 0] * 255).to(torch.uint8)


def _setr(embed, heads, dilations):
    return dict(backbone=dict(type="DiNAT", embed_dim=embed, mlp_ratio=2.0, depths=[1, 1, 2, 1], num_heads=heads, kernel_size=7,
                              dilations=dilations, drop_path_rate=0.3),
                decode_head=dict(type="SETRUPHead", in_channels=embed * 8, channels=512, num_convs=4, up_scale=2, num_classes=2))


def _uper(embed, mlp_ratio, heads):
    return dict(backbone=dict(type="NAT", embed_dim=embed, mlp_ratio=mlp_ratio, depths=[1, 1, 2, 1], num_heads=heads, kernel_size=7, layer_scale=1e-5),
                decode_head=dict(type="UPerHead", in_channels=[embed, 2 * embed, 4 * embed, 8 * embed], in_index=[0, 1, 2, 3], channels=64,
                                 num_classes=2))


WIDE = _setr(192, [6, 12, 24, 48], [[20], [10], [1, 5], [2]])               # DiNAT-L's widths, heads and head at reduced depth
WIDE_TWIN = _setr(128, [4, 8, 16, 32], [[16], [8], [1, 4], [2]])            # DiNAT-B's: every kernel instance of the parent
MINI = _uper(64, 3.0, [2, 4, 8, 16])                                        # NAT-Mini's widths and mlp_ratio at reduced depth
MINI_TWIN = _uper(128, 2.0, [4, 8, 16, 32])                                 # NAT-B's widths (heads doubled with the width: head dim 32)


def _bf16_vs_fp32(cfg, codes):
    """(label disagreement, relative RMS error of the head's low-resolution logits, class-1 fraction) of the bfloat16
    prepare_inference() model against the float32 unprepared one, parameters from randomize_neutral_parameters, classifier balanced."""
    from ppnet_amd import fused, segnet
    torch.manual_seed(0)
    m32 = segnet.randomize_neutral_parameters(segnet.SegNet.from_config(cfg), seed=1).eval().to(DEV)
    img32 = fused.grid_to_image(codes, segnet.IMG_MEAN, segnet.IMG_STD, torch.float32)
    with torch.no_grad():
        segnet.balance_classifier_bias(m32, img32)
    m16 = copy.deepcopy(m32).to(torch.bfloat16).prepare_inference()
    setr = cfg["decode_head"]["type"] == "SETRUPHead"
    with torch.no_grad():
        l32, l16 = m32.labels_u8(codes), m16.labels_u8(codes)
        lo32 = m32.decode_head(m32.backbone(img32), lowres=True) if setr else m32.decode_head(m32.backbone(img32))
        img16 = img32.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        lo16 = m16.decode_head(m16.backbone(img16), lowres=True) if setr else m16.decode_head(m16.backbone(img16))
    torch.cuda.synchronize()
    assert lo16.shape == lo32.shape and bool(torch.isfinite(lo16.float()).all())
    d = lo16.float() - lo32
    return (float((l32 != l16).float().mean()), float(d.pow(2).mean().sqrt() / lo32.pow(2).mean().sqrt()), float(l32.float().mean()))


def _held_to_twice_the_twin(name, cfg, twin, capsys):
    codes = _codes(4, 256, 5).to(DEV)
    dis_t, err_t, frac_t = _bf16_vs_fp32(twin, codes)
    dis, err, frac = _bf16_vs_fp32(cfg, codes)
    with capsys.disabled():
        print(f"\n{name}: bf16 prepared vs fp32: label disagreement {dis:.5f} (twin {dis_t:.5f}), low-resolution logits rel RMS {err:.4e} "
              f"(twin {err_t:.4e}); class-1 fraction {frac:.3f} (twin {frac_t:.3f})")
    assert 0.05 < frac < 0.95 and 0.05 < frac_t < 0.95
    # same depth and arithmetic, reductions 1.5 x longer: an honest path stays well inside a factor 2, a wrong one does not
    assert dis <= 2.0 * dis_t, (dis, dis_t)
    assert err <= 2.0 * err_t, (err, err_t)


def test_wide_dinat_l_widths_bf16_vs_fp32(capsys):
    """192 / 384 / 768 / 1536 with 6 / 12 / 24 / 48 heads, dilations 20 / 10 / 5 / 2 (every dilated layer virtually padded at 256^2),
    SETR-UP on 1536 channels."""
    _held_to_twice_the_twin("wide (DiNAT-L widths)", WIDE, WIDE_TWIN, capsys)


def test_wide_level2_on_nat_gemm_bf16_vs_fp32(capsys, monkeypatch):
    """The same pair with the tile-count gate opened (PPNET_SMALL_GEMM_TILES=1): level 2 (C = 768, 1024 tokens; the twin's C = 512) and
    level 1 of the twin run on ppn_nat_gemm_bf16, as they do at DiNAT-L's real batch sizes; level 3 of the wide model (1536) must not."""
    monkeypatch.setenv("PPNET_SMALL_GEMM_TILES", "1")
    _held_to_twice_the_twin("wide, level 2 on ppn_nat_gemm_bf16", WIDE, WIDE_TWIN, capsys)


def test_nat_mini_shape_bf16_vs_fp32(capsys):
    """NAT(embed 64, mlp_ratio 3) + UPerHead(64 / 128 / 256 / 512 -> 64): hidden widths 192 / 384 / 768 / 1536."""
    _held_to_twice_the_twin("NAT-Mini widths", MINI, MINI_TWIN, capsys)
