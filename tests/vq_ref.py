"""CPU restatement of taming's `VectorQuantizer2` in its legacy form (taming/modules/vqvae/quantize.py), the `quantize` of the
latent-inpainting model's VQModelInterface (ldm/models/autoencoder.py:14-283; taming is not a dependency of this project).

    z  [B, D, H, W] -> z_flattened [B*H*W, D]
    d  = sum(z^2, 1, keepdim) + sum(e^2, 1) - 2 * einsum('bd,dn->bn', z, e^T)
    idx = argmin(d, 1)                               (first index on ties)
    z_q = z + (e[idx] - z)                            (the straight-through form, evaluated in fp32)
"""
import torch


def distances(z, e):
    zf = z.permute(0, 2, 3, 1).reshape(-1, z.shape[1])
    return torch.sum(zf ** 2, dim=1, keepdim=True) + torch.sum(e ** 2, dim=1) - 2 * torch.einsum('bd,dn->bn', zf, e.t())


def quantize(z, e):
    """z fp32 [B, D, H, W], e fp32 [n_embed, D] -> (z_q [B, D, H, W], idx int64 [B, H, W])."""
    B, D, H, W = z.shape
    d = distances(z, e)
    idx = torch.argmin(d, dim=1)
    zf = z.permute(0, 2, 3, 1)
    zq = e[idx].view(zf.shape)
    zq = zf + (zq - zf)
    return zq.permute(0, 3, 1, 2).contiguous(), idx.view(B, H, W)


def straight_through(z, e, idx):
    """z + (e[idx] - z) for given indices idx [B, H, W] (fp32)."""
    zf = z.permute(0, 2, 3, 1)
    return (zf + (e[idx] - zf)).permute(0, 3, 1, 2).contiguous()
