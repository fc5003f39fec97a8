"""The conditioning stage of the semantic-synthesis models (models/ldm/semantic_synthesis256 / 512, cond_stage_config):

    SpatialRescalerHIP <- ldm.modules.encoders.modules.SpatialRescaler

`n_stages` bilinear halvings of an fp32 NCHW map and the trained 1x1 `channel_mapper`, as one launch of csrc/rescale.hip over the input
(sdmi_k_spatial_rescale; the arithmetic is defined in include/sdmi.h).  `encode_labels` takes the label map itself: the one-hot tensor
the reference's data loader builds (182 channels at image resolution) is never materialised, and the result is the same bit for bit
(sdmi_k_spatial_rescale_labels).  State-dict keys are the reference's: `channel_mapper.weight` [Cout, Cin, 1, 1] (+ `.bias`).
"""
import torch
import torch.nn as nn

from . import _lib

MAX_STAGES, MAX_OUT_CHANNELS = 2, 8            # what csrc/rescale.hip instantiates


class SpatialRescalerHIP(nn.Module):
    def __init__(self, n_stages=1, method='bilinear', multiplier=0.5, in_channels=3, out_channels=None, bias=False):
        super().__init__()
        if method != 'bilinear':
            raise NotImplementedError(f"SpatialRescalerHIP: method={method!r}; only method='bilinear' is built")
        if multiplier != 0.5:
            raise NotImplementedError(f'SpatialRescalerHIP: multiplier={multiplier!r}; only multiplier=0.5 is built')
        if not 0 <= int(n_stages) <= MAX_STAGES:
            raise NotImplementedError(f'SpatialRescalerHIP: n_stages={n_stages}; n_stages 0 .. {MAX_STAGES} are built')
        if out_channels is not None and not 1 <= int(out_channels) <= MAX_OUT_CHANNELS:
            raise NotImplementedError(f'SpatialRescalerHIP: out_channels={out_channels}; out_channels 1 .. {MAX_OUT_CHANNELS} are built')
        if int(in_channels) < 1:
            raise ValueError(f'SpatialRescalerHIP: in_channels={in_channels}')
        self.n_stages, self.method, self.multiplier = int(n_stages), method, multiplier
        self.in_channels = int(in_channels)
        self.out_channels = None if out_channels is None else int(out_channels)
        self.remap_output = out_channels is not None
        if self.remap_output:
            self.channel_mapper = nn.Conv2d(self.in_channels, self.out_channels, 1, bias=bias)

    def _device_input(self, t, what):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f'SpatialRescalerHIP runs on an MI355X device tensor only (no CPU fallback): {what}')
        if self.remap_output and self.channel_mapper.weight.device != t.device:
            raise RuntimeError(f'SpatialRescalerHIP: channel_mapper is on {self.channel_mapper.weight.device}, the input on {t.device}')

    def _weights(self):
        if not self.remap_output:
            return None, None
        w = self.channel_mapper.weight.detach().float().contiguous()
        b = self.channel_mapper.bias
        return w, None if b is None else b.detach().float().contiguous()

    def _out(self, B, H, W, device):
        side = 1 << self.n_stages
        if H < side or W < side:
            raise ValueError(f'SpatialRescalerHIP: a {H} x {W} map is smaller than the {side} x {side} block of {self.n_stages} halvings')
        C = self.out_channels if self.remap_output else self.in_channels
        return torch.empty((B, C, H >> self.n_stages, W >> self.n_stages), dtype=torch.float32, device=device)

    @torch.no_grad()
    def forward(self, x):
        """x fp32 [B, in_channels, H, W] on the device -> [B, out_channels (or in_channels), H >> n_stages, W >> n_stages]"""
        self._device_input(x, 'x')
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError(f'SpatialRescalerHIP: x must be [B, {self.in_channels}, H, W], got {tuple(x.shape)}')
        if x.dtype != torch.float32:
            raise ValueError(f'SpatialRescalerHIP: x must be float32, got {x.dtype}')
        x = x.detach().contiguous()
        B, _, H, W = x.shape
        out = self._out(B, H, W, x.device)
        w, b = self._weights()
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().sdmi_k_spatial_rescale(x.data_ptr(), _lib.ptr(w), _lib.ptr(b), out.data_ptr(), B, self.in_channels, H, W,
                                                          self.n_stages, self.out_channels or 0, _lib.stream_ptr()))
        return out

    def encode(self, x):
        return self(x)

    @torch.no_grad()
    def encode_labels(self, labels, check_range=True):
        """labels [B, H, W] (uint8 / int32 / int64) on the device, class c = channel c of the one-hot map -> encode(one_hot(labels)) bit
        for bit.  The range check costs one amin / amax and a sync; this runs once per image.  (check_range=False for a caller that has
        checked: the kernel itself gives a label outside the range no class, it reads nothing out of bounds.)"""
        self._device_input(labels, 'labels')
        if not self.remap_output:
            raise NotImplementedError('SpatialRescalerHIP.encode_labels: out_channels=None (the pooled one-hot map alone has no label entry)')
        if labels.dim() != 3 or labels.dtype not in (torch.uint8, torch.int32, torch.int64):
            raise ValueError(f'SpatialRescalerHIP: labels must be [B, H, W] of uint8 / int32 / int64, got {tuple(labels.shape)} {labels.dtype}')
        lo, hi = (int(labels.amin()), int(labels.amax())) if check_range else (0, 0)
        if lo < 0 or hi >= self.in_channels:
            raise ValueError(f'SpatialRescalerHIP: labels span [{lo}, {hi}], outside the class range [0, {self.in_channels})')
        lab = labels.detach().to(torch.int32).contiguous()
        B, H, W = lab.shape
        out = self._out(B, H, W, lab.device)
        w, b = self._weights()
        with torch.cuda.device(lab.device):
            _lib.check(_lib.load().sdmi_k_spatial_rescale_labels(lab.data_ptr(), w.data_ptr(), _lib.ptr(b), out.data_ptr(), B, self.in_channels,
                                                                 H, W, self.n_stages, self.out_channels, _lib.stream_ptr()))
        return out
