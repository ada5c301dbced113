"""tests/_conv_ref.py (the float64 gather references the GPU convolution tests compare with) against the library's float64
convolutions and LayerNorm on the CPU: values within 1e-12, at odd sizes, at 1 x 1 and with more than one image; and the rounding
scale A against the same library convolution of the absolute values."""
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from tests import _conv_ref as R  # noqa: E402

TOL = 1e-12
SHAPES = [(1, 1, 1), (3, 1, 1), (1, 1, 7), (2, 7, 1), (2, 5, 9), (3, 6, 6), (1, 16, 18), (2, 9, 21)]


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _same(got, want):
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= TOL * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("Cin,Cout", [(1, 8), (24, 24), (24, 1), (3, 5)])
def test_conv3x3_matches_the_library_in_float64(B, H, W, stride, Cin, Cout):
    x, w, b = _rand(B + H, B, H, W, Cin), _rand(W, Cout, Cin, 3, 3), _rand(Cin, Cout)
    y, A = R.conv3x3(x, w, b, stride)
    _same(y, _nhwc(F.conv2d(_nchw(x), w, b, stride, 1)))
    _same(A, _nhwc(F.conv2d(_nchw(x).abs(), w.abs(), b.abs(), stride, 1)))
    y0, A0 = R.conv3x3(x, w, None, stride)
    _same(y0, _nhwc(F.conv2d(_nchw(x), w, None, stride, 1)))
    assert bool((A0 >= y0.abs() - 1e-12).all())


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("Cin,Cout", [(24, 24), (3, 5)])
def test_conv_transpose3x3_s2_matches_the_library_in_float64(B, H, W, Cin, Cout):
    x, w, b = _rand(B * H, B, H, W, Cin), _rand(W + 1, Cin, Cout, 3, 3), _rand(Cout, Cout)
    y, A = R.conv_transpose3x3_s2(x, w, b)
    assert y.shape == (B, 2 * H, 2 * W, Cout)
    _same(y, _nhwc(F.conv_transpose2d(_nchw(x), w, b, 2, 1, 1)))
    _same(A, _nhwc(F.conv_transpose2d(_nchw(x).abs(), w.abs(), b.abs(), 2, 1, 1)))


def test_leaky_and_bf16_round():
    x = torch.tensor([-2.0, -0.0, 0.0, 3.0], dtype=torch.float64)
    assert torch.equal(R.leaky(x, 0.5), torch.tensor([-1.0, 0.0, 0.0, 3.0], dtype=torch.float64))
    _same(R.leaky(_rand(1, 50), 0.01), F.leaky_relu(_rand(1, 50), 0.01))
    v = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -20, 255.0, 257.0, -0.75], dtype=torch.float64)
    assert torch.equal(R.bf16_round(v), torch.tensor([1.0 + 2.0 ** -7, 255.0, 256.0, -0.75], dtype=torch.float64))


@pytest.mark.parametrize("B,H,W", [(1, 2, 2), (3, 6, 6), (2, 10, 34)])
def test_first_enc_matches_the_library_composition(B, H, W):
    x = _rand(B, B, H, W, 1)
    c1, c2 = (_rand(2, 24, 1, 3, 3), _rand(3, 24)), (_rand(4, 24, 24, 3, 3) / 8, _rand(5, 24))
    r = R.first_enc(x, c1, c2, 0.01, 0.2)
    mid = F.leaky_relu(F.conv2d(_nchw(x), *c1, 1, 1), 0.01)
    _same(r.mid_exact, _nhwc(mid))
    mid = mid.float().to(torch.bfloat16).double()
    assert torch.equal(r.mid, _nhwc(mid))
    _same(r.out, _nhwc(F.leaky_relu(F.conv2d(mid, *c2, 2, 1), 0.2)))
    _same(r.A, _nhwc(F.conv2d(mid.abs(), c2[0].abs(), c2[1].abs(), 2, 1)))
    assert r.out.shape == (B, H // 2, W // 2, 24)


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 3, 5), (2, 9, 17)])
def test_dec_final_matches_the_library_composition(B, H, W):
    x = _rand(B, B, H, W, 24)
    dec, fin = (_rand(2, 24, 24, 3, 3) / 8, _rand(3, 24)), (_rand(4, 1, 24, 3, 3) / 8, _rand(5, 1))
    r = R.dec_final(x, dec, 0.01, fin)
    mid = F.leaky_relu(F.conv_transpose2d(_nchw(x), *dec, 2, 1, 1), 0.01).float().to(torch.bfloat16).double()
    assert torch.equal(r.mid, _nhwc(mid))
    _same(r.out, _nhwc(F.conv2d(mid, *fin, 1, 1)))
    assert r.out.shape == (B, 2 * H, 2 * W, 1)


@pytest.mark.parametrize("B,H,W", [(1, 4, 64), (2, 12, 64), (3, 6, 32)])
def test_tokenizer_matches_the_library_composition(B, H, W):
    mean, std = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
    g = torch.Generator().manual_seed(H)
    codes = torch.tensor([255, 128, 0, 77], dtype=torch.uint8)[torch.randint(0, 4, (B, H, W), generator=g)]
    c1, c2 = (_rand(2, 64, 3, 3, 3) / 5, _rand(3, 64)), (_rand(4, 128, 64, 3, 3) / 24, _rand(5, 128))
    lw, lb = _rand(6, 128), _rand(7, 128)
    r = R.tokenizer(codes, c1, c2, lw, lb, 1e-5, mean, std)
    # the palette: three colours, normalised in float32 and stored as bfloat16
    px = {255: (255.0, 255.0, 255.0), 128: (255.0, 0.0, 0.0), 0: (0.0, 0.0, 0.0), 77: (0.0, 0.0, 0.0)}
    rgb = torch.tensor([[px[int(c)] for c in row] for row in codes.reshape(-1, W)], dtype=torch.float32).reshape(B, H, W, 3)
    img = ((rgb - torch.tensor(mean)) / torch.tensor(std)).to(torch.bfloat16).double()
    assert torch.equal(r.image, img)
    y1 = F.conv2d(_nchw(img), *c1, 2, 1)
    _same(r.conv1, _nhwc(y1))
    _same(r.A1, _nhwc(F.conv2d(_nchw(img).abs(), c1[0].abs(), c1[1].abs(), 2, 1)))
    y1 = y1.float().to(torch.bfloat16).double()
    assert torch.equal(r.mid, _nhwc(y1))
    y2 = _nhwc(F.conv2d(y1, *c2, 2, 1))
    _same(r.conv2, y2)
    _same(r.out, F.layer_norm(y2, (128,), lw, lb, 1e-5))
    assert r.conv1.shape == (B, H // 2, W // 2, 64) and r.out.shape == (B, (H // 2 + 1) // 2, (W // 2 + 1) // 2, 128)
