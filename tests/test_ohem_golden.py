"""heads.ohem_weight / decode_losses(class_weight, sampler) against the REFERENCE's own OHEMPixelSampler.sample and
CrossEntropyLoss (tests/golden/g21_ohem.npz, written by tests/golden/make_ohem_fixture.py from the reference's files, unmodified), in
float64 on the CPU: the 0 / 1 weights equal the recorded ones exactly and the reduced loss agrees to 1e-12; the fixture's cases have no
ties at the cut, so the keep-all-ties rule plays no part.  Also: both arguments None is today's decode_losses bit for bit; a head built
from a config dict carries sampler and class weights as plain attributes (its state_dict keys do not change); unsupported samplers and
weight files raise."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_ohem.npz"))
CASES = [str(c) for c in G["cases"]]


def _case(name):
    from ppnet_amd.heads import OHEMPixelSampler
    thresh = float(G[f"{name}/thresh"])
    cw = G[f"{name}/class_weight"]
    return (torch.from_numpy(G[f"{name}/logit"]), torch.from_numpy(G[f"{name}/label"]),
            OHEMPixelSampler(thresh=None if np.isnan(thresh) else thresh, min_kept=int(G[f"{name}/min_kept"])),
            [float(v) for v in cw] if cw.size else None, torch.from_numpy(G[f"{name}/seg_weight"]), float(G[f"{name}/loss"]))


def test_fixture_holds_every_case_of_both_class_counts():
    kinds = {c.rsplit("_", 1)[0] for c in CASES}
    assert kinds == {"a", "b", "c", "d1", "d2", "e", "fa", "fe"} and len(CASES) == 16
    for name in CASES:
        x, lab, sampler, cw, want, _ = _case(name)
        assert x.dtype == torch.float64 and tuple(x.shape) == (2, int(name[-1]), 12, 20) and tuple(lab.shape) == (2, 12, 20)
        assert (cw is not None) == name.startswith("f") and (sampler.thresh is None) == (name[0] == "e" or name[:2] in ("d2", "fe"))
        frac = float((lab == 255).double().mean())
        assert frac == 1.0 if name.startswith("d") else 0.1 < frac < 0.3


@pytest.mark.parametrize("name", CASES)
def test_ohem_weight_equals_the_references_exactly(name):
    from ppnet_amd.heads import ohem_weight
    x, lab, sampler, cw, want, _ = _case(name)
    got = ohem_weight(x, lab, sampler, cw, 255)
    assert got.dtype == torch.float64 and torch.equal(got, want)
    assert set(got.unique().tolist()) <= {0.0, 1.0} and float(got[lab == 255].sum()) == 0.0


@pytest.mark.parametrize("name", CASES)
def test_decode_losses_equals_the_references_loss(name):
    from ppnet_amd.heads import decode_losses
    x, lab, sampler, cw, _, want = _case(name)
    loss, acc = decode_losses(x, lab, 1.0, 255, class_weight=cw, sampler=sampler)
    assert abs(float(loss) - want) <= 1e-12, (float(loss), want)
    assert float(acc) == float(decode_losses(x, lab)[1])                       # sampling does not change acc_seg
    half, _ = decode_losses(x, lab, 0.5, 255, class_weight=cw, sampler=sampler)
    assert abs(float(half) - 0.5 * want) <= 1e-12


def test_without_sampler_and_weights_is_todays_decode_losses_bit_for_bit():
    from ppnet_amd.heads import decode_losses, ohem_weight
    x, lab, _, _, _, _ = _case("a_c5")
    for t in (x, x.float()):
        loss, acc = decode_losses(t, lab, 0.4, 255, class_weight=None, sampler=None)
        want = 0.4 * F.cross_entropy(t, lab, ignore_index=255, reduction="none").mean()
        assert torch.equal(loss, want) and torch.equal(acc, (t.argmax(1) == lab).float().sum() * (100.0 / lab.numel()))
        assert torch.equal(loss, decode_losses(t, lab, 0.4)[0])
    # no sampler: weight 1 on every valid pixel; class weights alone are F.cross_entropy(weight=...) under the mean over all pixels
    assert torch.equal(ohem_weight(x, lab, None), (lab != 255).double())
    cw = [0.5, 1.0, 2.0, 0.25, 3.0]
    got = decode_losses(x, lab, 1.0, 255, class_weight=cw)[0]
    want = F.cross_entropy(x, lab, weight=torch.tensor(cw, dtype=torch.float64), ignore_index=255, reduction="none").mean()
    assert abs(float(got) - float(want)) <= 1e-12


def test_ties_at_the_cut_are_all_kept_and_out_of_range_labels_are_ignored():
    from ppnet_amd.heads import OHEMPixelSampler, ohem_weight
    x = torch.zeros(1, 3, 4, 5, dtype=torch.float64)                            # every score ties
    lab = torch.randint(0, 3, (1, 4, 5), generator=torch.Generator().manual_seed(1))
    lab[0, 0, :2] = 255
    lab[0, 1, 0], lab[0, 1, 1] = 3, -1                                          # outside [0, C): ignored, never indexed
    valid = (lab >= 0) & (lab < 3)
    assert int(valid.sum()) == 16
    w = ohem_weight(x, lab, OHEMPixelSampler(min_kept=2), None, 255)            # top-k: the cut ties with everything
    assert torch.equal(w, valid.double())
    w = ohem_weight(x, lab, OHEMPixelSampler(thresh=0.7, min_kept=2), None, 255)    # p = 1/3 < 0.7 everywhere
    assert torch.equal(w, valid.double())
    w = ohem_weight(x, lab, OHEMPixelSampler(thresh=0.2, min_kept=2), None, 255)    # t = max(1/3, 0.2): p < t is strict, none
    assert float(w.sum()) == 0.0


HEADS = [("SETRUPHead", dict(in_channels=16, channels=8, num_classes=3)),
         ("UPerHead", dict(in_channels=(8, 8, 8, 8), channels=8, num_classes=3)),
         ("UPerPUPHead", dict(in_channels=(8, 8, 8, 8), channels=8, num_classes=3, num_convs=(1, 2, 3, 4))),
         ("FCNHead", dict(in_channels=8, channels=8, num_classes=3, num_convs=1))]


@pytest.mark.parametrize("typ,cfg", HEADS, ids=[h[0] for h in HEADS])
def test_heads_read_sampler_and_class_weight_from_the_config(typ, cfg):
    from ppnet_amd import heads
    cls = getattr(heads, typ)
    plain = cls(**cfg)
    assert plain.sampler is None and plain.class_weight is None
    h = cls(**cfg, sampler=dict(type="OHEMPixelSampler", thresh=0.7, min_kept=100000),
            loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.4, class_weight=[1.0, 2.0, 0.5]))
    assert isinstance(h.sampler, heads.OHEMPixelSampler) and h.sampler.thresh == 0.7 and h.sampler.min_kept == 100000
    assert h.class_weight == (1.0, 2.0, 0.5)
    assert list(h.state_dict()) == list(plain.state_dict())                    # plain attributes: no buffer, no checkpoint key
    assert cls(**cfg, sampler=dict(type="OHEMPixelSampler")).sampler.thresh is None
    if typ == "FCNHead":
        assert h.loss_weight == 0.4
    with pytest.raises(NotImplementedError):
        cls(**cfg, sampler=dict(type="RandomPixelSampler"))
    with pytest.raises(NotImplementedError):
        cls(**cfg, loss_decode=dict(type="CrossEntropyLoss", class_weight="weights.npy"))
    with pytest.raises(ValueError):
        cls(**cfg, loss_decode=dict(type="CrossEntropyLoss", class_weight=[1.0, 2.0]))
    with pytest.raises(AssertionError):
        cls(**cfg, sampler=dict(type="OHEMPixelSampler", min_kept=1))           # the reference's assert min_kept > 1


def test_segnet_hands_each_heads_own_options_to_the_loss(monkeypatch):
    from ppnet_amd import segnet
    seen = []

    def spy(logit, gt, w, **kw):
        seen.append((w, kw["class_weight"], kw["sampler"]))
        return logit.sum() * 0.0, torch.zeros(())
    monkeypatch.setattr(segnet, "resized_decode_losses", spy)
    m = segnet.SegNet.from_config(dict(
        type="EncoderDecoder",
        backbone=dict(type="DiNAT", embed_dim=32, mlp_ratio=2.0, depths=[1, 1, 1, 1], num_heads=[1, 2, 4, 8], kernel_size=7,
                      dilations=[[1], [1], [1], [1]]),
        decode_head=dict(type="UPerHead", in_channels=(32, 64, 128, 256), channels=8, num_classes=2,
                         sampler=dict(type="OHEMPixelSampler", thresh=0.7, min_kept=50)),
        auxiliary_head=dict(type="FCNHead", in_channels=128, channels=8, num_classes=2, num_convs=1, in_index=2,
                            loss_decode=dict(type="CrossEntropyLoss", loss_weight=0.4, class_weight=[1.0, 3.0]))))
    monkeypatch.setattr(m.backbone, "forward", lambda img: [])
    monkeypatch.setattr(m.decode_head, "forward", lambda f: torch.zeros(1, 2, 8, 8))
    monkeypatch.setattr(m.auxiliary_head, "forward", lambda f: torch.zeros(1, 2, 2, 2))
    m.forward_train(torch.zeros(1, 3, 32, 32), None, torch.zeros(1, 32, 32, dtype=torch.long))
    assert len(seen) == 2
    assert seen[0][0] == 1.0 and seen[0][1] is None and seen[0][2].thresh == 0.7 and seen[0][2].min_kept == 50
    assert seen[1][0] == 0.4 and seen[1][1] == (1.0, 3.0) and seen[1][2] is None
