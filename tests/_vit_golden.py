"""Storage form of tests/golden/g20_vit.npz, shared by its writer (tests/golden/make_vit_fixture.py) and its readers
(tests/test_vit_golden.py, tests/test_gpu_vit.py): outputs as float32 values plus float64 checksums, the checksum and comparison
of tests/_swin_golden.py.  The network inputs are not stored: image() regenerates them from the legacy MT19937 stream."""
import numpy as np

from tests._swin_golden import assert_matches, checksum  # noqa: F401  (the same storage form)

IMAGES = {"a64": (64, 64), "a96": (96, 128), "a70": (70, 50)}
SMALL = dict(img_size=64, patch_size=16, in_channels=3, embed_dims=128, num_layers=3, num_heads=2, mlp_ratio=4, out_indices=(1, 2),
             with_cls_token=False)
SMALL_CLS = dict(SMALL, with_cls_token=True, final_norm=True, patch_norm=True)


def image(case):
    """The float32-representable input image [1, 3, H, W] of a case."""
    hh, ww = IMAGES[case]
    return np.random.RandomState(2000 + hh + 7 * ww).normal(0.0, 1.0, (1, 3, hh, ww)).astype(np.float32)


def attn_tokens(n=40, c=128):
    """The token input [1, n, c] of case c (one attention layer with large logits)."""
    return np.random.RandomState(2020).normal(0.0, 1.0, (1, n, c)).astype(np.float32)
