"""FrozenCLIPTextEmbedderHIP on the MI355X: OpenAI CLIP's encode_text (tower, EOT pool at the first maximum of the ids, text_projection, L2
normalisation) against fp64 on the CPU.

Two seeded towers from transformers configs: tiny (2 layers, W = 64, 2 heads, E = 32, vocab 99) and an SD-shaped thin one (W = 768, 12 heads,
E = 768, 2 layers).  L in {77, 40}, B in {1, 3}; EOT = the largest id, at position 1, mid-sequence and L - 1, different per sample; zeros
behind it, as clip.tokenize pads.

  1. the head alone: embeds == LN-final hidden[argmax] @ text_projection^T (normalised), in fp64 from the EXISTING sdmi_clip_forward output
     of the same handle.  mixed: 2 x the fp16-operand floor of that one GEMM (both operands rounded to fp16 in the test); full: W 2^-21 on
     the unnormalised value relative to |h| |w_row|, the split-fp16 representation bound.
  2. end to end, mixed: against CLIPTextModelWithProjection.double() pooling at the same position (asserted), within 2 x the fp16-operand
     floor of the whole graph (every Linear input and weight and the q / k / v outputs rounded to fp16 once, the method of the ViT goldens);
     the floor itself must lie in (1e-5, 1e-2).
  3. end to end, full: the bar the full-precision text encoder's hidden state is held to (a tenth of the mixed hidden-state pin).
  4. the pad id behind EOT changes no output bit; 5. normalize=False; 6. n_repeat; 7. a handle without a projection refuses by name.

Measured on an MI355X (max-abs on the normalised embedding | bar):
  e2e mixed   tiny 2.67e-4 / 4.01e-4 | 2 x floor 6.05e-4 / 7.79e-4;  W = 768: 8.97e-5 / 1.07e-4 | 1.69e-4 / 1.78e-4
  e2e full    tiny 4.6e-7 / 3.1e-7, W = 768: 2.6e-7 / 2.7e-7 | 4.6e-4
  head mixed  tiny 1.60e-4 / 1.78e-4 | 3.19e-4 / 3.56e-4;  W = 768: 3.34e-5 / 3.85e-5 | 6.67e-5 / 7.71e-5
  head full   4.5e-8 ... 7.1e-8 of |h| |w_row| | W 2^-21 = 3.05e-5 (tiny), 3.66e-4 (W = 768)"""
import copy
import ctypes as C

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from stable_diffusion_amd import FrozenCLIPEmbedderHIP, FrozenCLIPTextEmbedderHIP, _lib  # noqa: E402
from stable_diffusion_amd.clip import make_clip_cfg  # noqa: E402

CONFIGS = {
    'tiny': dict(vocab_size=99, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                 max_position_embeddings=77, projection_dim=32),
    'sd_thin': dict(vocab_size=1000, hidden_size=768, intermediate_size=3072, num_hidden_layers=2, num_attention_heads=12,
                    max_position_embeddings=77, projection_dim=768),
}
FULL_BAR = 0.1 * 4.6e-3          # tests/test_text_encoder_full_gpu.py CLIP_HARD = 0.1 x tests/test_clip_gpu.py CLIP_TOL
CASES = [('tiny', 77, 3), ('tiny', 40, 1), ('sd_thin', 77, 1), ('sd_thin', 40, 3)]
_cache = {}


def reference_model(name):
    """CLIPTextModelWithProjection from the config, seeded, in fp64; eos_token_id = the largest id, so that it pools where argmax does"""
    if ('ref', name) not in _cache:
        from transformers import CLIPTextConfig, CLIPTextModelWithProjection
        tc = CONFIGS[name]
        torch.manual_seed(11)
        cfg = CLIPTextConfig(**tc, hidden_act='quick_gelu', attn_implementation='eager', eos_token_id=tc['vocab_size'] - 1, bos_token_id=1,
                             pad_token_id=0)
        m = CLIPTextModelWithProjection(cfg).double().eval()
        with torch.no_grad():        # LayerNorm gains and biases off their defaults, so a dropped affine shows
            for n_, p in m.named_parameters():
                if 'layer_norm' in n_:
                    p.add_(0.1 * torch.randn_like(p))
        _cache[('ref', name)] = m
    return _cache[('ref', name)]


def r16(t):
    return t.half().to(t.dtype)


def fp16_operand_model(m):
    e = copy.deepcopy(m)
    for name, mod in e.named_modules():
        if isinstance(mod, nn.Linear):
            mod.weight.data = r16(mod.weight.data)
            mod.register_forward_pre_hook(lambda _m, args: (r16(args[0]),) + tuple(args[1:]))
        if name.endswith(('.q_proj', '.k_proj', '.v_proj')):
            mod.register_forward_hook(lambda _m, _a, out: r16(out))
    return e


def hip_model(name, precision):
    if (name, precision) not in _cache:
        m = FrozenCLIPTextEmbedderHIP(text_config=CONFIGS[name], tokenizer=object(), hip_precision=precision)
        sd = {'transformer.' + k: v.float() for k, v in reference_model(name).state_dict().items() if 'position_ids' not in k}
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and all('position_ids' in k for k in missing), (missing, unexpected)
        _cache[(name, precision)] = m.cuda()
    return _cache[(name, precision)]


def make_ids(name, L, B, pad=0, seed=0):
    """EOT = the largest id at position 1, mid-sequence, L - 1 (sample b takes the b-th); random ids before it, `pad` behind it"""
    V = CONFIGS[name]['vocab_size']
    g = torch.Generator().manual_seed(seed + L + B)
    ids = torch.randint(2, V - 1, (B, L), generator=g)
    ids[:, 0] = 1
    pos = [1, L // 2, L - 1]
    eot = torch.tensor([pos[(b + (0 if B > 1 else L % 3)) % 3] for b in range(B)])
    for b in range(B):
        ids[b, eot[b]] = V - 1
        ids[b, eot[b] + 1:] = pad
    return ids, eot


def reference(name, ids):
    if ('out', name, tuple(ids.shape), int(ids.sum())) not in _cache:
        m = reference_model(name)
        with torch.no_grad():
            z = m(input_ids=ids).text_embeds
            z16 = fp16_operand_model(m)(input_ids=ids).text_embeds
        n, n16 = z / z.norm(dim=1, keepdim=True), z16 / z16.norm(dim=1, keepdim=True)
        _cache[('out', name, tuple(ids.shape), int(ids.sum()))] = (z, n, float((n16 - n).abs().max()))
    return _cache[('out', name, tuple(ids.shape), int(ids.sum()))]


@pytest.mark.parametrize('name,L,B', CASES)
@pytest.mark.parametrize('precision', ['mixed', 'full'])
def test_head_equals_projection_of_the_existing_hidden_state(name, L, B, precision):
    m = hip_model(name, precision)
    ids, eot = make_ids(name, L, B)
    assert torch.equal(ids.argmax(-1), eot)
    dev = ids.cuda()
    hidden = m.hidden_states(dev)                      # sdmi_clip_forward of the same handle
    raw = m.encode_ids(dev, normalize=False).double().cpu()
    nrm = m.encode_ids(dev).double().cpu()
    h = hidden.double().cpu()[torch.arange(B), eot]    # [B, W]
    w = m.transformer.text_projection.weight.detach().double().cpu()
    z = h @ w.T
    zn = z / z.norm(dim=1, keepdim=True)
    W = h.shape[1]
    if precision == 'mixed':
        z16 = r16(h) @ r16(w).T
        floor = float((z16 / z16.norm(dim=1, keepdim=True) - zn).abs().max())
        err = float((nrm - zn).abs().max())
        print(f'[head {name} L={L} B={B} mixed] max-abs {err:.3e} (2 x floor of the one GEMM {2 * floor:.3e})')
        assert floor > 0 and err <= 2 * floor
    else:
        scale = h.norm(dim=1, keepdim=True) * w.norm(dim=1)[None]
        rel = float(((raw - z).abs() / scale).max())
        print(f'[head {name} L={L} B={B} full] max |raw - fp64| / (|h| |w_row|) {rel:.3e} (bar {W * 2.0 ** -21:.3e}); normalised max-abs '
              f'{float((nrm - zn).abs().max()):.3e}')
        assert rel <= W * 2.0 ** -21
        assert float((nrm - zn).abs().max()) <= W * 2.0 ** -21 * float((scale / z.norm(dim=1, keepdim=True)).max()) + 2.0 ** -22


@pytest.mark.parametrize('name,L,B', CASES)
def test_end_to_end_mixed(name, L, B):
    ids, eot = make_ids(name, L, B)
    V = CONFIGS[name]['vocab_size']
    assert torch.equal(ids.argmax(-1), eot) and torch.equal((ids == V - 1).int().argmax(-1), eot)      # both pool at the same position
    _, ref, floor = reference(name, ids)
    got = hip_model(name, 'mixed').encode_ids(ids.cuda()).double().cpu()
    err = float((got - ref).abs().max())
    print(f'[e2e {name} L={L} B={B} mixed] max-abs {err:.3e}, fp16-operand floor of the graph {floor:.3e} (bar 2 x)')
    assert 1e-5 < floor < 1e-2
    assert err <= 2 * floor


@pytest.mark.parametrize('name,L,B', CASES)
def test_end_to_end_full(name, L, B):
    ids, _ = make_ids(name, L, B)
    _, ref, floor = reference(name, ids)
    got = hip_model(name, 'full').encode_ids(ids.cuda()).double().cpu()
    err = float((got - ref).abs().max())
    print(f'[e2e {name} L={L} B={B} full] max-abs {err:.3e} (bar {FULL_BAR:.2e}; mixed floor {floor:.3e})')
    assert err <= FULL_BAR


@pytest.mark.parametrize('precision', ['mixed', 'full'])
def test_pad_id_behind_eot_changes_no_bit(precision):
    """clip.tokenize pads with 0, CLIPTokenizer with its pad id (the EOT id for OpenAI's vocabulary, another id elsewhere); causal mask + EOT pool"""
    m = hip_model('tiny', precision)
    a_ids, eot = make_ids('tiny', 77, 3, pad=0)
    outs = [m.encode_ids(a_ids.cuda())]
    for pad in (CONFIGS['tiny']['vocab_size'] - 1, 7):
        b_ids, _ = make_ids('tiny', 77, 3, pad=pad)
        assert not torch.equal(a_ids, b_ids) and torch.equal(b_ids.argmax(-1), eot)      # (first maximum: still the EOT position)
        outs.append(m.encode_ids(b_ids.cuda()))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_normalize_false_repeat_and_interface():
    ids, _ = make_ids('tiny', 77, 3)
    z, _, _ = reference('tiny', ids)

    class Tok:
        def __call__(self, text, **kw):
            assert kw['padding'] == 'max_length' and kw['max_length'] == 77
            return {'input_ids': ids[:len(text)]}

    m = FrozenCLIPTextEmbedderHIP(text_config=CONFIGS['tiny'], tokenizer=Tok(), normalize=False, n_repeat=3)
    m.load_state_dict(hip_model('tiny', 'mixed').state_dict())
    m = m.cuda()
    raw = m(['a', 'b', 'c'])
    assert raw.shape == (3, 32) and raw.dtype == torch.float32
    assert float((raw.double().cpu() - z).abs().max()) <= 2e-2 * float(z.abs().max())          # the unnormalised projection, not a unit vector
    assert float((raw.norm(dim=1) - 1).abs().min()) > 1e-2
    enc = m.encode(['a', 'b', 'c'])
    assert enc.shape == (3, 3, 32) and all(torch.equal(enc[:, i], raw) for i in range(3))
    unit = hip_model('tiny', 'mixed').encode_ids(ids.cuda())
    assert float((unit.norm(dim=1) - 1).abs().max()) <= 1e-6
    one = FrozenCLIPTextEmbedderHIP(text_config=CONFIGS['tiny'], tokenizer=Tok())
    one.load_state_dict(m.state_dict())
    assert one.cuda().encode(['a', 'b']).shape == (2, 1, 32)


def test_a_handle_without_a_projection_refuses_text_embeds_by_name():
    lib = _lib.load()
    tc = {k: v for k, v in CONFIGS['tiny'].items() if k != 'projection_dim'}
    m = FrozenCLIPEmbedderHIP(text_config=tc, tokenizer=object())
    assert lib.sdmi_clip_projection_dim(m._handle.h) == 0
    assert all('text_projection' not in k for k, _ in m._specs)
    ids = torch.zeros((1, 77), dtype=torch.int64, device='cuda')
    out = torch.empty((1, 32), device='cuda')
    ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    assert lib.sdmi_clip_text_embeds(m._handle.h, ids.data_ptr(), out.data_ptr(), 1, 77, 1, ws.data_ptr(), ws.numel(), None) != 0
    assert 'created without a text projection' in lib.sdmi_last_error().decode()
    assert lib.sdmi_clip_text_embeds_workspace_bytes(m._handle.h, 1, 77) == 0
    h = C.c_void_p()
    assert lib.sdmi_clip_create_projection(C.byref(make_clip_cfg(tc)), 0, 0, C.byref(h)) != 0
    assert 'projection_dim must be positive' in lib.sdmi_last_error().decode()
