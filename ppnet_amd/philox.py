"""Device-side Philox4x32-10 draws as tensors (same streams the generator kernels consume)."""
import ctypes as C

import torch

from . import _lib as L

STREAM_PATH, STREAM_POCKET, STREAM_PLACE, STREAM_OBST, STREAM_AUG = 1, 2, 3, 4, 5


def doubles_device(seed, stream_id, instance, first, count, device):
    device = torch.device(device)
    out = torch.empty(count, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        rc = L.lib.ppn_philox_doubles(seed, stream_id, instance, first, count, C.c_void_p(out.data_ptr()),
                                      C.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    L.check(rc, "ppn_philox_doubles")
    return out


def doubles_host(seed, stream_id, instance, first, count):
    """The same draws on the host as a NumPy float64 array (for code paths that run without a GPU): Philox4x32-10, Random123
    constants, counter (draw >> 1, instance >> 32, instance & 0xffffffff, stream), key = the two halves of seed; draw d takes
    words (0, 1) of its block when even and (2, 3) when odd, by numpy's random_sample recipe ((a >> 5) * 2^26 + (b >> 6)) / 2^53."""
    import numpy as np
    seed, instance, mask = int(seed) & (2 ** 64 - 1), int(instance) & (2 ** 64 - 1), 0xFFFFFFFF
    out = np.empty(count, dtype=np.float64)
    blocks = {}
    for i in range(count):
        d = first + i
        if d >> 1 not in blocks:
            c = [(d >> 1) & mask, instance >> 32, instance & mask, stream_id & mask]
            k0, k1 = seed & mask, seed >> 32
            for r in range(10):
                if r:
                    k0, k1 = (k0 + 0x9E3779B9) & mask, (k1 + 0xBB67AE85) & mask
                p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
                c = [(p1 >> 32) ^ c[1] ^ k0, p1 & mask, (p0 >> 32) ^ c[3] ^ k1, p0 & mask]
            blocks[d >> 1] = c
        a, b = blocks[d >> 1][2 * (d & 1): 2 * (d & 1) + 2]
        out[i] = ((a >> 5) * 67108864 + (b >> 6)) / 9007199254740992.0
    return out
