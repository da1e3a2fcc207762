"""Random model outputs for the tests of the sampling family (test_gpu_sampling.py, test_gpu_risk.py)."""
import torch


def random_pred(gen, n, p, v, dev, rho_raw=None):
    """(N,5,P,V) strided view of a (N,P,V,5) tensor: means, unequal log sigmas, correlations."""
    base = torch.empty((n, p, v, 5))
    base[..., 0:2] = torch.randn((n, p, v, 2), generator=gen) * 0.5
    base[..., 2] = torch.rand((n, p, v), generator=gen) * 1.5 - 1.0
    base[..., 3] = torch.rand((n, p, v), generator=gen) * 1.5 - 0.5
    base[..., 4] = torch.randn((n, p, v), generator=gen) if rho_raw is None else rho_raw
    return base.to(dev).permute(0, 3, 1, 2)
