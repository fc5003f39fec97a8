"""`ClassEmbedderHIP` -- drop-in for `ldm.modules.encoders.modules.ClassEmbedder` (modules.py:21-33), the conditioner of the
class-conditional ImageNet model (configs/latent-diffusion/cin256-v2.yaml:63-68: n_classes 1001, class 1000 = the unconditional
label of classifier-free guidance).

One table lookup per sampling run: plain torch indexing, not a hot path.  The context it returns has ONE token
([B, 1, embed_dim]), for which `UNetModelHIP` copies the cross-attention output from the cached V^T (SDMI_CTX1).  Same constructor,
same `forward(batch, key=None)`, same state-dict key `embedding.weight`.
"""
import torch.nn as nn


class ClassEmbedderHIP(nn.Module):
    def __init__(self, embed_dim, n_classes=1000, key='class'):
        super().__init__()
        self.key = key
        self.embedding = nn.Embedding(n_classes, embed_dim)

    def forward(self, batch, key=None):
        if key is None:
            key = self.key
        return self.embedding(batch[key][:, None])      # [B] class ids -> [B, 1, embed_dim]: one token for the cross-attention
