"""Storage form of tests/golden/g18_swin.npz, shared by its writer (tests/golden/make_swin_fixture.py) and its readers
(tests/test_swin_golden.py, tests/test_gpu_swin.py).  An output is kept as its float32 rounding plus four float64 checksums
(checksum below): elementwise to float32 precision and, through the checksums, to 1e-10 — at half the bytes of float64 arrays.
The network inputs are not stored: image() regenerates them from the legacy MT19937 stream (frozen across NumPy versions)."""
import numpy as np

IMAGES = {"a": (112, 112), "b": (60, 92)}


def image(case):
    """The float32-representable input image [1, 3, H, W] of case a / b."""
    hh, ww = IMAGES[case]
    return np.random.RandomState(1800 + hh).normal(0.0, 1.0, (1, 3, hh, ww)).astype(np.float32)


def checksum(y):
    """[sum, sum of squares, a fixed pseudo-random projection, sum of |y|] of a float64 array."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    w = np.random.RandomState(1818).uniform(-1.0, 1.0, y.size)
    return np.array([y.sum(), (y * y).sum(), (w * y).sum(), np.abs(y).sum()])


def assert_matches(got, y32, chk, rel=1e-10, what=""):
    """got (float64) equals the recorded float64 output: elementwise within its float32 rounding, and its checksums within what
    ONE element off by rel * max|y| would move them (rel * max|y| for the sums and the projection, twice max|y| that for the sum
    of squares).  Roundoff between two float64 evaluations of the same arithmetic stays orders of magnitude below."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == y32.shape, what
    scale = float(np.abs(y32).max())
    err = np.abs(got - y32.astype(np.float64)) - 1.2e-7 * np.abs(y32.astype(np.float64))
    assert err.max() <= rel * max(1.0, scale), (what, float(err.max()))
    c = checksum(got)
    e = rel * max(1.0, scale)
    tol = np.array([e, 2.0 * max(1.0, scale) * e, e, e])
    assert (np.abs(c - chk) <= tol + 1e-300).all(), (what, c - chk)
