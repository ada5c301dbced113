"""The float64 gather reference of the neighbourhood-attention forward (tests/_na_ref.py) against the brute-force definition
(oracle/na_np.py): values, the two padding forms, the rounding scale A and the selection map.  No GPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import na_np as NA  # noqa: E402
from tests import _na_ref as R  # noqa: E402


def _inputs(B, H, W, heads, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, H, W, 3 * heads * 32, generator=g, dtype=torch.float64),
            torch.randn(heads, 13, 13, generator=g, dtype=torch.float64))


@pytest.mark.parametrize("B,H,W,heads,d", [(2, 9, 11, 2, 1), (1, 15, 22, 3, 2), (1, 23, 29, 1, 3)])
def test_values_equal_the_brute_force_oracle(B, H, W, heads, d):
    qkv, rpb = _inputs(B, H, W, heads, H + d)
    ref = R.na2d_ref(qkv, rpb, heads, d, 32 ** -0.5)
    want = NA.na2d_from_qkv(qkv.numpy(), rpb.numpy(), heads, 7, d, 32 ** -0.5)
    assert ref.out.shape == (B, H, W, heads * 32)
    assert np.abs(ref.out.numpy() - want).max() < 1e-12
    # A = sum p |v|: with every v replaced by |v| the output IS that sum
    qa = qkv.clone()
    qa[..., 2 * heads * 32:] = qa[..., 2 * heads * 32:].abs()
    assert (R.na2d_ref(qa, rpb, heads, d, 32 ** -0.5).out - ref.A).abs().max() < 1e-12
    assert bool((ref.A >= ref.out.abs() - 1e-12).all())


@pytest.mark.parametrize("H,W,Hr,Wr,d", [(21, 28, 16, 13, 3), (28, 35, 3, 5, 4), (14, 14, 9, 10, 2)])
def test_virtual_padding_equals_materialised_padding(H, W, Hr, Wr, d):
    heads = 2
    real, rpb = _inputs(2, Hr, Wr, heads, H + Wr)
    pad = torch.randn(3 * heads * 32, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    full = pad.expand(2, H, W, -1).clone()
    full[:, :Hr, :Wr] = real
    v = R.na2d_ref(real, rpb, heads, d, 32 ** -0.5, pad_kv=pad, padded_hw=(H, W))
    m = R.na2d_ref(full, rpb, heads, d, 32 ** -0.5, real_hw=(Hr, Wr))
    assert v.out.shape == m.out.shape == (2, Hr, Wr, heads * 32)
    assert torch.equal(v.out, m.out) and torch.equal(v.A, m.A) and torch.equal(v.v_full, m.v_full)
    want = NA.na2d_from_qkv(full.numpy(), rpb.numpy(), heads, 7, d, 32 ** -0.5)[:, :Hr, :Wr]
    assert np.abs(m.out.numpy() - want).max() < 1e-12


@pytest.mark.parametrize("H,W,Hr,Wr,d", [(15, 22, 15, 22, 2), (21, 28, 16, 13, 3), (7, 9, 7, 9, 1), (28, 35, 3, 5, 4)])
def test_selection_map_agrees_with_the_window_definition(H, W, Hr, Wr, d):
    qkv, rpb = _inputs(1, H, W, 1, 1)
    ref = R.na2d_ref(qkv, rpb, 1, d, 1.0, real_hw=(Hr, Wr))
    rows = [NA.window(i, H, 7, d) for i in range(Hr)]
    cols = [NA.window(j, W, 7, d) for j in range(Wr)]
    for i, (pi, bi) in enumerate(rows):
        assert np.array_equal(ref.ri[i].numpy(), pi) and np.array_equal(ref.bi[i].numpy(), bi)
    for j, (pj, bj) in enumerate(cols):
        assert np.array_equal(ref.cj[j].numpy(), pj) and np.array_equal(ref.bj[j].numpy(), bj)
    seen = 0
    for a in range(13):
        for b in range(13):
            mask, row, col = ref.select(a, b)
            for i, (pi, bi) in enumerate(rows):
                for j, (pj, bj) in enumerate(cols):
                    hit = a in bi and b in bj
                    assert bool(mask[i, j]) == hit
                    if hit:
                        assert int(row[i, j]) == pi[list(bi).index(a)] and int(col[i, j]) == pj[list(bj).index(b)]
                        seen += 1
    assert seen == Hr * Wr * 49                                            # every window member of every query is selected once
    if (H, W, d) == (15, 22, 2):
        assert int(ref.select(0, 0)[0].sum()) == 4                         # offset (-6, -6): the last query of the 4 groups only
