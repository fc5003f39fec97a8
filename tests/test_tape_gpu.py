"""Launch tapes (csrc/tape.h, round 6): sdmi_unet_forward records the launch list of a (shape, workspace, timestep mode, knobs) once and replays
it with only the caller's pointers patched.  A replayed forward must give the bits the executor gives -- for other inputs, other output
tensors, other timesteps (table row, int64 tensor, float tensor), pinned and passed contexts, interleaved shapes, changed weights, flipped
knobs -- and SDMI_REPLAY_VERIFY=1 (the executor runs on every would-be replay and its launch list is compared with the patched tape) must pass."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.plan import SD_V1, TINY  # noqa: E402
from oracle.weights import make_inputs, make_state_dict  # noqa: E402


def _model(cfg, seed=0):
    from stable_diffusion_amd import UNetModelHIP
    m = UNetModelHIP(**cfg.ref_kwargs())
    m.load_state_dict(make_state_dict(cfg, seed), strict=True)
    return m.cuda().eval()


def _stats(m):
    a, b = C.c_int64(0), C.c_int64(0)
    from stable_diffusion_amd import _lib
    _lib.check(m._handle.lib.sdmi_unet_tape_stats(m._handle.h, C.byref(a), C.byref(b)))
    return a.value, b.value


def _calls(cfg):
    """(x, t, ctx, hint) of a little sampling-like sequence: three inputs, three timestep forms"""
    out = []
    for seed, ts in ((1, (981, 981)), (2, (961, 961)), (3, (1, 1))):
        x, t, ctx = make_inputs(cfg, 2, 16, 16, seed=seed, timesteps=ts)
        out.append((x.cuda(), t.cuda(), ctx.cuda(), ts[0]))
    return out


@pytest.mark.parametrize('cfg_name', ['tiny', 'sdv1'])
def test_replayed_forwards_equal_executed_forwards(cfg_name, monkeypatch):
    cfg = {'tiny': TINY, 'sdv1': SD_V1}[cfg_name]
    m = _model(cfg)
    calls = _calls(cfg)
    ctx = calls[0][2]

    def sequence():
        outs = []
        m.cache_timesteps([981, 961, 1])
        for x, t, c, hint in calls:                       # pinned context, hinted timesteps: the samplers' mode
            m.pin_context(ctx)
            m.hint_timestep(hint)
            outs.append(m(x, t, context=ctx).clone())
        m.unpin_context()
        m.cache_timesteps([])
        for x, t, c, hint in calls:                       # a fresh context every call, int64 timesteps computed by the call
            outs.append(m(x, t, context=c).clone())
        for x, t, c, hint in calls[:2]:                   # float timesteps (DPM-Solver)
            outs.append(m(x, t.float(), context=c).clone())
        x1, t1, c1 = make_inputs(cfg, 1, 8, 8, seed=9, ctx_len=40)       # another shape in between ...
        outs.append(m(x1.cuda(), t1.cuda(), context=c1.cuda()).clone())
        x, t, c, hint = calls[1]
        outs.append(m(x, t, context=c).clone())           # ... and back
        torch.cuda.synchronize()
        return outs

    monkeypatch.setenv('SDMI_REPLAY', '0')
    want = sequence()
    h0, r0 = _stats(m)
    assert h0 == 0 and r0 == 0
    monkeypatch.setenv('SDMI_REPLAY', '1')
    got1 = sequence()                                     # records (and already replays the repeats inside the sequence)
    got2 = sequence()                                     # replays
    h, r = _stats(m)
    print(f'[tape {cfg_name}] {h} forwards replayed, {r} recorded', flush=True)
    assert r >= 4 and h >= len(want) + 4
    for i, (w, a, b) in enumerate(zip(want, got1, got2)):
        assert torch.equal(w, a), (i, float((w - a).abs().max()))
        assert torch.equal(w, b), (i, float((w - b).abs().max()))
    monkeypatch.setenv('SDMI_REPLAY_VERIFY', '1')         # the executor runs; its launch list must equal the patched tape
    got3 = sequence()
    for i, (w, a) in enumerate(zip(want, got3)):
        assert torch.equal(w, a), i
    monkeypatch.delenv('SDMI_REPLAY_VERIFY')
    # a knob the library reads per call changes the tape's identity (here: the chain launches off -> other kernels, same bits)
    monkeypatch.setenv('SDMI_ST_HEAD', '0')
    x, t, c, hint = calls[0]
    e = m(x, t, context=c)
    assert torch.equal(e, want[3])
    monkeypatch.delenv('SDMI_ST_HEAD')
    # new weights: the tapes of the old packed buffers are dead
    m.load_state_dict(make_state_dict(cfg, 5), strict=True)
    e_new = m(x, t, context=c).clone()
    assert not torch.equal(e_new, want[3])
    monkeypatch.setenv('SDMI_REPLAY', '0')
    assert torch.equal(m(x, t, context=c), e_new)


def _forward(m, x, t, ctx, out):
    """sdmi_unet_forward straight through ctypes (the module would allocate its own eps_out): int64 timesteps, context passed"""
    from stable_diffusion_amd import _lib
    B, _, H, W = x.shape
    L = ctx.shape[1]
    ws = m._workspace(B, H, W, L, x.device)
    m._reserve_context(B, L)
    _lib.check(m._handle.lib.sdmi_unet_forward(m._handle.h, x.data_ptr(), t.data_ptr(), None, ctx.data_ptr(), out.data_ptr(),
                                               B, H, W, L, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
    torch.cuda.synchronize()


def test_in_place_recorded_tape_replays_into_separate_buffers(monkeypatch):
    """A tape recorded with eps_out == x, replayed with separate x' / eps_out': eps_out' gets the executor's bits, x' stays as it was
    (the relocation of each caller pointer comes from its declaration, not from the range its address falls into)."""
    m = _model(TINY)
    (x, t, c, _), (x2, _, _, _) = _calls(TINY)[:2]
    m(x, t, context=c)                                    # (packs the weights)
    monkeypatch.setenv('SDMI_REPLAY', '0')
    want_in_place = x.clone()
    _forward(m, want_in_place, t, c, want_in_place)
    want2 = torch.empty_like(x2)
    _forward(m, x2, t, c, want2)
    monkeypatch.setenv('SDMI_REPLAY', '1')
    h0, r0 = _stats(m)
    buf = x.clone()
    _forward(m, buf, t, c, buf)                           # records, in place
    h1, r1 = _stats(m)
    assert (h1, r1) == (h0, r0 + 1)
    assert torch.equal(buf, want_in_place)
    x2c, out2 = x2.clone(), torch.full_like(x2, float('nan'))
    _forward(m, x2c, t, c, out2)                          # replays, separate buffers
    assert _stats(m) == (h1 + 1, r1)
    assert torch.equal(x2c, x2)
    assert torch.equal(out2, want2)


def test_caller_alignment_is_part_of_the_tape_key(monkeypatch):
    """conv_out takes its 16-byte-store kernel only for a 16-byte aligned eps_out: a tape recorded with an aligned one must not serve a
    call whose eps_out is 4 bytes off -- that call is executed (and recorded) and gives the executor's bits."""
    m = _model(TINY)
    x, t, c, _ = _calls(TINY)[0]
    m(x, t, context=c)

    def misaligned(src=None, k=1):
        big = torch.empty(x.numel() + k, dtype=torch.float32, device=x.device)
        out = big[k:].view(x.shape)
        assert out.data_ptr() % 16 == 4 * k
        if src is not None:
            out.copy_(src)
        return out

    monkeypatch.setenv('SDMI_REPLAY', '0')
    want = misaligned()
    _forward(m, x, t, c, want)
    monkeypatch.setenv('SDMI_REPLAY', '1')
    _forward(m, x, t, c, torch.empty_like(x))             # a tape of the aligned eps_out
    h, r = _stats(m)
    got = misaligned()
    _forward(m, x, t, c, got)
    assert _stats(m) == (h, r + 1)
    assert torch.equal(got, want)
    # each pointer's alignment is keyed on its own: a tape recorded with x 8 bytes off and eps_out aligned (conv_out's 16-byte stores)
    # must not serve a call with x aligned and eps_out 8 bytes off (an offset no tape above was recorded with)
    monkeypatch.setenv('SDMI_REPLAY', '0')
    want8 = misaligned(k=2)
    _forward(m, x, t, c, want8)
    monkeypatch.setenv('SDMI_REPLAY', '1')
    _forward(m, misaligned(x, k=2), t, c, torch.empty_like(x))
    h, r = _stats(m)
    got = misaligned(k=2)
    _forward(m, x, t, c, got)
    assert _stats(m) == (h, r + 1)
    assert torch.equal(got, want8)
