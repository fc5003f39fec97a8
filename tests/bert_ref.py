"""CPU restatement (fp32, functional torch) of the LAION-400M model's text encoder.

`BERTEmbedder` (ldm/modules/encoders/modules.py:80-103) tokenizes and returns
`TransformerWrapper(num_tokens, max_seq_len, attn_layers=Encoder(dim=n_embed, depth=n_layer))(tokens,
return_embeddings=True)` of ldm/modules/x_transformer.py, every other setting at its default:

    x = token_emb[ids] + pos_emb.emb[0..L-1]                                        (x_transformer.py:609-610, :25-36)
    per layer i (pre-norm, residual = plain add; AttentionLayers.forward, :481-531):
      h = LayerNorm(x) (layers.{2i}.0, eps 1e-5; :417)
      q, k, v = h Wq^T, h Wk^T, h Wv^T (no bias, width heads * dim_head = 8 * 64; :236-242), split into heads
      x = x + to_out(softmax(q k^T * dim_head^-0.5) v)  -- no causal mask, no padding mask (:296-367)
      h = LayerNorm(x) (layers.{2i+1}.0)
      x = x + net.2(gelu_erf(net.0.0(h)))  (FeedForward(dim, mult=4): Linear, nn.GELU(), Dropout(0), Linear; :194-212)
    out = norm(x)                                                                   (:579, :624; to_logits never applied, :628)

`tools/make_golden_laion.py` loads `make_bert_state_dict` into the reference module (strict=True), asserts this
restatement equals it to 5e-5 and writes tests/golden/bert_*.npz.  Test infrastructure only: the product path never imports it.
"""
import math
from collections import OrderedDict
from dataclasses import dataclass

import torch
import torch.nn.functional as F


@dataclass(frozen=True)
class BertCfg:
    vocab_size: int = 30522
    dim: int = 1280
    depth: int = 32
    max_seq_len: int = 77
    heads: int = 8            # x_transformer.Attention defaults
    dim_head: int = 64
    ff_mult: int = 4

    @property
    def inner(self):
        return self.heads * self.dim_head

    def embedder_kwargs(self):
        """BERTEmbedder / BERTEmbedderHIP constructor arguments"""
        return dict(n_embed=self.dim, n_layer=self.depth, vocab_size=self.vocab_size, max_seq_len=self.max_seq_len)


LAION_BERT = BertCfg()                                          # txt2img-1p4B-eval.yaml cond_stage_config
LAION_BERT_D2 = BertCfg(depth=2)
TINY_BERT = BertCfg(vocab_size=1000, dim=128, depth=2)          # inner width stays 8 x 64 = 512
CFGS = {'tiny': TINY_BERT, 'laion_d2': LAION_BERT_D2, 'laion': LAION_BERT}


def bert_param_specs(cfg: BertCfg):
    D, I, Fi = cfg.dim, cfg.inner, cfg.ff_mult * cfg.dim
    specs = [('token_emb.weight', (cfg.vocab_size, D), 'emb'), ('pos_emb.emb.weight', (cfg.max_seq_len, D), 'emb')]
    for i in range(cfg.depth):
        a, f = f'attn_layers.layers.{2 * i}.', f'attn_layers.layers.{2 * i + 1}.'
        specs += [(a + '0.weight', (D,), 'gamma'), (a + '0.bias', (D,), 'beta'),
                  (a + '1.to_q.weight', (I, D), 'w'), (a + '1.to_k.weight', (I, D), 'w'), (a + '1.to_v.weight', (I, D), 'w'),
                  (a + '1.to_out.weight', (D, I), 'w'), (a + '1.to_out.bias', (D,), 'b'),
                  (f + '0.weight', (D,), 'gamma'), (f + '0.bias', (D,), 'beta'),
                  (f + '1.net.0.0.weight', (Fi, D), 'w'), (f + '1.net.0.0.bias', (Fi,), 'b'),
                  (f + '1.net.2.weight', (D, Fi), 'w'), (f + '1.net.2.bias', (D,), 'b')]
    specs += [('norm.weight', (D,), 'gamma'), ('norm.bias', (D,), 'beta'),
              ('to_logits.weight', (cfg.vocab_size, D), 'w'), ('to_logits.bias', (cfg.vocab_size,), 'b')]
    return specs


def make_bert_state_dict(cfg: BertCfg, seed: int = 0):
    """Seeded weights for `TransformerWrapper`'s state_dict (keys relative to `transformer.`)"""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for key, shape, kind in bert_param_specs(cfg):
        if kind == 'w':
            t = torch.randn(shape, generator=g) / math.sqrt(shape[1])
        elif kind == 'emb':
            t = torch.randn(shape, generator=g) * 0.5
        elif kind == 'b':
            t = torch.randn(shape, generator=g) * 0.05
        elif kind == 'gamma':
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            t = 0.1 * torch.randn(shape, generator=g)
        sd[key] = t.float()
    return sd


def make_bert_ids(cfg: BertCfg, batch, L, seed=1):
    """token ids shaped like BertTokenizerFast's padded output: [CLS]=101, words, [SEP]=102, [PAD]=0 to L"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(batch, L, dtype=torch.int64)
    for b in range(batch):
        n = int(torch.randint(1, max(2, L - 1), (1,), generator=g))       # words in this row
        ids[b, 0] = 101
        ids[b, 1:1 + n] = torch.randint(103, cfg.vocab_size, (n,), generator=g)
        if 1 + n < L:
            ids[b, 1 + n] = 102
    return ids


def bert_forward(sd, cfg: BertCfg, ids):
    """TransformerWrapper.forward(ids, return_embeddings=True) -> fp32 [B, L, dim]"""
    B, L = ids.shape
    H, dh = cfg.heads, cfg.dim_head
    x = sd['token_emb.weight'][ids] + sd['pos_emb.emb.weight'][:L][None]
    for i in range(cfg.depth):
        a, f = f'attn_layers.layers.{2 * i}.', f'attn_layers.layers.{2 * i + 1}.'
        h = F.layer_norm(x, (cfg.dim,), sd[a + '0.weight'], sd[a + '0.bias'], 1e-5)
        q, k, v = (F.linear(h, sd[a + f'1.to_{n}.weight']).view(B, L, H, dh).transpose(1, 2) for n in 'qkv')
        att = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, dim=-1) @ v
        x = x + F.linear(att.transpose(1, 2).reshape(B, L, H * dh), sd[a + '1.to_out.weight'], sd[a + '1.to_out.bias'])
        h = F.layer_norm(x, (cfg.dim,), sd[f + '0.weight'], sd[f + '0.bias'], 1e-5)
        h = F.gelu(F.linear(h, sd[f + '1.net.0.0.weight'], sd[f + '1.net.0.0.bias']))
        x = x + F.linear(h, sd[f + '1.net.2.weight'], sd[f + '1.net.2.bias'])
    return F.layer_norm(x, (cfg.dim,), sd['norm.weight'], sd['norm.bias'], 1e-5)
