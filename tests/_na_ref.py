"""TEST INFRASTRUCTURE — vectorised float64 reference of the 2-D neighbourhood-attention forward (kernel 7), for the tests that
compare every kernel variant behind ppn_na2d_fwd / _padded / _vpad with it (tests/test_gpu_na_variants.py).

The definition is oracle/na_np.py's (brute force, one query at a time); this file restates it as a gather, in the form of
oracle/segnet_ref.py's na_fp64, so that a 40 x 40 x 10-image case costs a second instead of minutes.  The axis tables are built
here from the formula, NOT from na_np.window: tests/test_na_ref.py holds the two against each other (values within 1e-12, the
tables entry for entry) on any machine.

Besides the output it returns what the GPU tests' bounds and known answers are made of:
  A         sum_j p_j |v_j| per output element — the scale of the bfloat16 rounding errors of p, of the sum and of the output;
  select    for a bias index (a, b): which queries' windows hold the member with that relative offset, and where it sits on the
            padded grid — from the same tables the output is gathered with.
"""
import torch

K = 7


def axis_tables(L, d, n_query=None, k=K):
    """Axis of length L, dilation d: (pos [n, k], bias [n, k]) int64 for the queries 0 .. n-1 (n = n_query or L).  A query i belongs
    to dilation group i % d (members i % d, i % d + d, ...: cnt of them); its window is the k consecutive members from member
    index clamp(i // d - k // 2, 0, cnt - k); member t has bias index (start + t - i // d) + k - 1."""
    n = L if n_query is None else n_query
    i = torch.arange(n, dtype=torch.int64)
    g, u = i % d, i // d
    cnt = (L - g + d - 1) // d
    if int(cnt.min()) < k:
        raise ValueError("axis shorter than kernel * dilation: pad first")
    start = torch.minimum(torch.clamp(u - k // 2, min=0), cnt - k)
    t = torch.arange(k, dtype=torch.int64)
    member = start[:, None] + t[None, :]
    return g[:, None] + member * d, member - u[:, None] + (k - 1)


class NARef:
    """out, A: [B, Hr, Wr, C] float64; ri / bi: [Hr, 7] and cj / bj: [Wr, 7] — key rows / columns on the padded grid and bias indices;
    v_full: [B, H, W, C] float64, the v of every position of the padded grid (pad_kv's v part on the padded ones)."""

    def __init__(self, out, A, ri, bi, cj, bj, v_full):
        self.out, self.A, self.ri, self.bi, self.cj, self.bj, self.v_full = out, A, ri, bi, cj, bj, v_full

    def select(self, a, b):
        """(mask [Hr, Wr] bool, row [Hr, Wr], col [Hr, Wr]): the queries whose window holds the member with bias index (a, b) and
        that member's position on the padded grid (0 where the mask is False)."""
        ti, tj = a - self.bi[:, 0], b - self.bj[:, 0]                     # bias indices of a window are consecutive
        oki, okj = (ti >= 0) & (ti < K), (tj >= 0) & (tj < K)
        row = torch.where(oki, self.ri.gather(1, ti.clamp(0, K - 1)[:, None])[:, 0], torch.zeros_like(ti))
        col = torch.where(okj, self.cj.gather(1, tj.clamp(0, K - 1)[:, None])[:, 0], torch.zeros_like(tj))
        mask = oki[:, None] & okj[None, :]
        Hr, Wr = mask.shape
        return mask, row[:, None].expand(Hr, Wr) * mask, col[None, :].expand(Hr, Wr) * mask


def na2d_ref(qkv, rpb, heads, dilation, scale, real_hw=None, pad_kv=None, padded_hw=None):
    """The arguments of ppnet_amd.na.na2d_forward.  qkv [B, Hs, Ws, 3C] is the STORED grid: the whole padded H x W grid (real_hw names
    the real tokens, which alone are queries), or the real tokens only with pad_kv [3C] standing for the k / v of every other position
    of the padded_hw grid.  Everything is computed in float64 on the CPU."""
    qkv = qkv.detach().cpu().double()
    rpb = rpb.detach().cpu().double()
    B, Hs, Ws, C3 = qkv.shape
    C = C3 // 3
    hd = C // heads
    if pad_kv is not None:
        assert real_hw is None
        H, W = padded_hw
        Hr, Wr = Hs, Ws
        full = pad_kv.detach().cpu().double().view(1, 1, 1, C3).expand(B, H, W, C3).clone()
        full[:, :Hr, :Wr] = qkv
    else:
        H, W = Hs, Ws
        Hr, Wr = real_hw if real_hw is not None else (H, W)
        full = qkv
    ri, bi = axis_tables(H, dilation, Hr)
    cj, bj = axis_tables(W, dilation, Wr)
    bias = rpb[:, bi[:, None, :, None], bj[None, :, None, :]]             # [heads, Hr, Wr, 7, 7]
    out = torch.empty(B, Hr, Wr, C, dtype=torch.float64)
    A = torch.empty_like(out)
    for b in range(B):                                                    # per image: bounds the gathered K / V
        t = full[b].view(H, W, 3, heads, hd).permute(2, 3, 0, 1, 4)
        q, kk, v = t[0][:, :Hr, :Wr] * scale, t[1], t[2]
        kg, vg = kk[:, ri][:, :, :, cj], v[:, ri][:, :, :, cj]            # [heads, Hr, 7, Wr, 7, hd]
        logit = torch.einsum("hijc,hiajbc->hijab", q, kg) + bias
        p = torch.softmax(logit.reshape(heads, Hr, Wr, K * K), dim=-1).view(heads, Hr, Wr, K, K)
        out[b] = torch.einsum("hijab,hiajbc->hijc", p, vg).permute(1, 2, 0, 3).reshape(Hr, Wr, C)
        A[b] = torch.einsum("hijab,hiajbc->hijc", p, vg.abs()).permute(1, 2, 0, 3).reshape(Hr, Wr, C)
    return NARef(out, A, ri, bi, cj, bj, full[..., 2 * C:].contiguous())
