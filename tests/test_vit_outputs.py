"""ViT backbone outputs (ppnet_amd/vit.py) as the reference orders them: one output per listed layer, in layer order
(SegNet/mmseg/backbones/vit.py:386-404), whatever the order or repetition of out_indices; and the torch path computes no LayerNorm
it throws away.  CPU only."""
import pytest

torch = pytest.importorskip("torch")


def _net(out_indices, **kw):
    from ppnet_amd.vit import VisionTransformer
    torch.manual_seed(3)
    m = VisionTransformer(img_size=32, embed_dims=64, num_layers=4, num_heads=1, out_indices=out_indices, **kw).double().eval()
    m.init_weights()
    return m


def test_outputs_follow_layer_order_once_per_layer():
    x = torch.randn(1, 3, 32, 32, dtype=torch.float64)
    ref = _net([0, 1, 2, 3])
    with torch.no_grad():
        every = ref(x)
    for given, layers in (([2, 0], [0, 2]), ([1, 1, 3], [1, 3]), ((3, 2, 1), [1, 2, 3]), ([0, 9], [0]), (-1, [3])):
        m = _net(given)
        assert m.out_indices == layers
        with torch.no_grad():
            outs = m(x)
        assert len(outs) == len(layers)
        for o, i in zip(outs, layers):
            assert torch.equal(o, every[i]), (given, i)


def test_torch_path_runs_each_layernorm_once():
    m = _net([3])
    calls = []
    for mod in m.modules():
        if isinstance(mod, torch.nn.LayerNorm):
            mod.register_forward_hook(lambda *a: calls.append(1))
    with torch.no_grad():
        m(torch.randn(1, 3, 32, 32, dtype=torch.float64))
    assert len(calls) == 2 * 4                                             # ln1 and ln2 of each of the 4 layers
    mf = _net([3], final_norm=True)
    calls.clear()
    for mod in mf.modules():
        if isinstance(mod, torch.nn.LayerNorm):
            mod.register_forward_hook(lambda *a: calls.append(1))
    with torch.no_grad():
        mf(torch.randn(1, 3, 32, 32, dtype=torch.float64))
    assert len(calls) == 2 * 4 + 1
