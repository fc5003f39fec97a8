"""`BERTEmbedderHIP` -- drop-in for `ldm.modules.encoders.modules.BERTEmbedder` on MI355X: the text encoder of the LAION-400M
LDM-KL-8 model (`configs/latent-diffusion/txt2img-1p4B-eval.yaml`, `scripts/txt2img.py --laion400m`).

Plugged in through the reference's plugin mechanism (`instantiate_from_config(cond_stage_config)`):

    cond_stage_config:
      target: stable_diffusion_amd.bert.BERTEmbedderHIP
      params:
        n_embed: 1280
        n_layer: 32
        hip_precision: full      # optional: 'mixed' (default) or 'full' (split-fp16 on every MFMA operand)

Same constructor as the reference (`n_embed`, `n_layer`, `vocab_size`, `max_seq_len`, `device`, `use_tokenizer`,
`embedding_dropout`; modules.py:82-83) plus an injectable `tokenizer` and `hip_precision`; same `forward(text)` / `encode(text)` returning
[B, 77, n_embed]; same parameter names (`transformer.*` of x_transformer.TransformerWrapper, so the `cond_stage_model.*` part
of the checkpoint loads, `to_logits` included -- it is never used).  Tokenization stays on the host (BertTokenizerFast
"bert-base-uncased", modules.py:53-70); the transformer runs in libsdmi.so.  No CPU / PyTorch fallback.
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from .unet import PRECISIONS, _Node

# x_transformer.Attention defaults (DEFAULT_DIM_HEAD = 64, heads = 8) and FeedForward(mult=4)
BERT_HEADS, BERT_DIM_HEAD, BERT_FF_MULT = 8, 64, 4


def make_bert_cfg(n_embed, n_layer, vocab_size=30522, max_seq_len=77):
    cfg = _lib.BertCfg()
    cfg.vocab_size, cfg.dim, cfg.depth = int(vocab_size), int(n_embed), int(n_layer)
    cfg.heads, cfg.dim_head, cfg.ff_inner, cfg.max_seq_len = BERT_HEADS, BERT_DIM_HEAD, BERT_FF_MULT * int(n_embed), int(max_seq_len)
    return cfg


class _BertHandle:
    """Owns one sdmi_bert*."""

    def __init__(self, cfg, precision='mixed'):
        self.lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self.lib.sdmi_bert_create_precision(C.byref(cfg), PRECISIONS[precision], C.byref(h)))
        self.h = h

    def weight_specs(self):
        n = self.lib.sdmi_bert_num_weights(self.h)
        out = []
        buf = C.create_string_buffer(256)
        shape = (C.c_int64 * 4)()
        nd = C.c_int()
        for i in range(n):
            _lib.check(self.lib.sdmi_bert_weight_info(self.h, i, buf, 256, shape, C.byref(nd)))
            out.append((buf.value.decode(), tuple(shape[j] for j in range(nd.value))))
        return out

    def __del__(self):
        try:
            if self.h:
                self.lib.sdmi_bert_destroy(self.h)
                self.h = None
        except Exception:
            pass


def _bert_tokenizer(max_length):
    """modules.py:56-58 (BERTTokenizer): the tokenizer the reference loads"""
    from transformers import BertTokenizerFast
    return BertTokenizerFast.from_pretrained('bert-base-uncased')


class BERTEmbedderHIP(nn.Module):
    MAX_BATCH = 64
    UNUSED = ('to_logits.weight', 'to_logits.bias')      # return_embeddings=True: accepted, never uploaded

    def __init__(self, n_embed, n_layer, vocab_size=30522, max_seq_len=77, device='cuda', use_tokenizer=True,
                 embedding_dropout=0.0, tokenizer=None, hip_precision='mixed'):
        """`hip_precision` (not a keyword of the reference BERTEmbedder): 'mixed' (default) = fp16 MFMA operands; 'full' = every MFMA
        operand split-fp16 (~22-bit operands, fp32 accumulation), slower.  Fixed for the module's lifetime; same
        parameter names and shapes."""
        super().__init__()
        if hip_precision not in PRECISIONS:
            raise ValueError(f"hip_precision must be one of {sorted(PRECISIONS)}, got {hip_precision!r}")
        self.hip_precision = hip_precision
        self.use_tknz_fn = use_tokenizer
        self.max_length = max_seq_len
        self.tokenizer = None
        if use_tokenizer:
            self.tokenizer = tokenizer if tokenizer is not None else _bert_tokenizer(max_seq_len)
        self.device = device
        self.embedding_dropout = embedding_dropout        # identity at inference (eval mode)
        self._cfg = make_bert_cfg(n_embed, n_layer, vocab_size, max_seq_len)
        self._handle = _BertHandle(self._cfg, hip_precision)
        self._specs = self._handle.weight_specs()          # keys relative to `transformer.`
        self.add_module('transformer', _Node())
        for key, shape in self._specs:
            *path, leaf = key.split('.')
            node = self.transformer
            for name in path:
                if name not in node._modules:
                    node.add_module(name, _Node())
                node = node._modules[name]
            node.register_parameter(leaf, nn.Parameter(torch.zeros(shape), requires_grad=False))
        self._packed_sig = None
        self._sentinels = None
        self._ws = None
        self.eval()
        for p in self.parameters():
            p.requires_grad = False

    # ---- weights -> library (same dirty tracking as UNetModelHIP) --------------------------------------------------
    def _apply(self, fn, *a, **k):
        self._packed_sig = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._packed_sig = None
        return super().load_state_dict(*a, **k)

    def mark_dirty(self):
        self._packed_sig = None

    def _signature(self):
        if getattr(self, '_sentinels', None) is None:
            ps = dict(self.transformer.named_parameters())
            keys = [self._specs[0][0], self._specs[len(self._specs) // 2][0], self._specs[-3][0]]
            self._sentinels = [ps[k] for k in keys]
        return tuple((p.data_ptr(), p._version) for p in self._sentinels)

    def pack(self):
        lib = self._handle.lib
        stream = _lib.stream_ptr()
        ps = dict(self.transformer.named_parameters())
        for key, shape in self._specs:
            if key in self.UNUSED:
                continue
            p = ps[key].detach()
            if not p.is_cuda:
                raise RuntimeError('BERTEmbedderHIP parameters must live on the GPU (call model.cuda() first); '
                                   'there is no CPU implementation of this path')
            p = p.float().contiguous()
            shp = (C.c_int64 * len(shape))(*shape)
            _lib.check(lib.sdmi_bert_set_weight(self._handle.h, key.encode(), p.data_ptr(), shp, len(shape), stream))
        torch.cuda.current_stream().synchronize()
        _lib.check(lib.sdmi_bert_finalize(self._handle.h))
        self._sentinels = None
        self._packed_sig = self._signature()

    # ---- TransformerWrapper(tokens, return_embeddings=True) -----------------------------------------------------------
    @torch.no_grad()
    def encode_ids(self, ids):
        if not ids.is_cuda:
            raise RuntimeError('BERTEmbedderHIP runs on an MI355X device tensor only (no CPU fallback)')
        if ids.dim() != 2 or ids.shape[1] > self._cfg.max_seq_len:
            raise ValueError(f'token ids must be [B, L <= {self._cfg.max_seq_len}]')
        if self._packed_sig is None or self._packed_sig != self._signature():
            self.pack()
        ids = ids.detach().to(torch.int64).contiguous()
        if int(ids.min()) < 0 or int(ids.max()) >= self._cfg.vocab_size:
            raise IndexError('token id out of range')           # what nn.Embedding raises in the reference
        B, L = ids.shape
        out = torch.empty((B, L, self._cfg.dim), dtype=torch.float32, device=ids.device)
        for b0 in range(0, B, self.MAX_BATCH):
            nb = min(self.MAX_BATCH, B - b0)
            key = (nb, L, str(ids.device))
            if self._ws is None or self._ws[0] != key:
                need = self._handle.lib.sdmi_bert_workspace_bytes(self._handle.h, nb, L)
                if need <= 0:
                    _lib.check(-1)
                self._ws = (key, torch.empty(int(need), dtype=torch.uint8, device=ids.device))
            ws = self._ws[1]
            _lib.check(self._handle.lib.sdmi_bert_forward(self._handle.h, ids[b0:b0 + nb].data_ptr(), out[b0:b0 + nb].data_ptr(),
                                                          nb, L, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        return out

    def tokenize(self, text):
        """modules.py:63-66: padding to max_length, truncation, input_ids"""
        batch_encoding = self.tokenizer(text, truncation=True, max_length=self.max_length, return_length=True,
                                        return_overflowing_tokens=False, padding='max_length', return_tensors='pt')
        return batch_encoding['input_ids']

    def forward(self, text):
        """modules.py:94-100 (tokens stay where the tokenizer made them there; here they move to `device`)"""
        tokens = self.tokenize(text).to(self.device) if self.use_tknz_fn else text
        return self.encode_ids(tokens)

    def encode(self, text):
        return self(text)
