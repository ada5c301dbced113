"""Cases and inputs of tests/golden/g19_uperpup.npz, shared by its writer (tests/golden/make_uperpup_fixture.py) and its readers
(tests/test_uperpup_golden.py, tests/test_gpu_uperpup.py).  The level features are not stored: features() regenerates them from the
legacy MT19937 stream (frozen across NumPy versions).  Outputs are kept in the form of tests/_swin_golden.py."""
import numpy as np

from tests._oracle_util import wiring_weights

# case: (num_convs, in_channels, channels, batch, level sizes finest first, weight seed)
CASES = {
    "a": ((1, 2, 3, 4), (16, 32, 64, 128), 16, 1, ((64, 64), (32, 32), (16, 16), (8, 8)), 19),
    "b": ((2, 3, 4, 5), (16, 32, 64, 128), 16, 2, ((16, 24), (8, 12), (4, 6), (2, 3)), 20),
}

# the heads of configs/nat/dense_nat_base.py and configs/swin/dense_swin_base.py (keys and shapes recorded, not run)
REAL = {"nat": (1, 2, 3, 4), "swin": (2, 3, 4, 5)}


def head_kwargs(case):
    num_convs, in_channels, channels, _, _, _ = CASES[case]
    return dict(in_channels=list(in_channels), channels=channels, num_convs=num_convs, num_classes=2, pool_scales=(1, 2, 3, 6),
                in_index=[0, 1, 2, 3], dropout_ratio=0.1, align_corners=False)


def features(case):
    """The float32-representable level features [B, C_l, H_l, W_l] of case a / b."""
    _, in_channels, _, B, sizes, _ = CASES[case]
    return [np.random.RandomState(1900 + 10 * l + ord(case)).normal(0.0, 1.0, (B, c) + hw).astype(np.float32)
            for l, (c, hw) in enumerate(zip(in_channels, sizes))]


def head_weights(keys, shapes, seed):
    """wiring_weights for every state-dict key but BatchNorm's num_batches_tracked; running variances mapped from the stream's
    +-0.2 to 1 + 2.5 v (0.5 .. 1.5), running means kept at +-0.2: every folded BatchNorm moves both scale and shift."""
    w = wiring_weights(keys, shapes, seed)
    for k in keys:
        if k.endswith("running_var"):
            w[k] = 1.0 + 2.5 * w[k]
    return w
