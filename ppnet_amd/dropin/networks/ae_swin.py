"""`networks.ae_swin` as the reference's GenNet/networks/ae_swin.py is imported (`from networks.ae_swin import AESwin`): the HIP-backed
AESwin with the reference's constructor (`AESwin(img_channels, out_channels, img_resolution, dim)`) and its 247 state-dict keys, so
`load_state_dict(torch.load(p)['model'])` works unchanged."""
from ppnet_amd.gennet import AESwin  # noqa: F401

__all__ = ["AESwin"]
