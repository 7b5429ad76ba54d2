"""GPU: utterances shorter than a window as rows of the windowed batch.

  * ttsk_mel_windows with short rows, bit for bit against torch slicing + zero fill + `ops.nct_to_ntc`;
  * every kernel that takes a per-row length (the *_rowlen entry points) against its plain entry point: a null length array is
    bit-equal on the whole tensor, and a row of v valid frames inside an (N, W s, C) batch equals the plain kernel on the
    (1, v s, C) tensor BIT FOR BIT — in all of these kernels a workgroup's tile starts at a multiple of the tile size from the row's
    own first frame and the taps are summed in a fixed order, so a position's arithmetic depends on neither the batch shape nor the
    row it sits in.  What lies past a row's end is NaN on the way in (a single read would poison the output) and a sentinel in `out`
    that must still be there afterwards (nothing is stored past the end);
  * a ragged call with lengths from one frame to several windows, V1 and V3, against the CPU oracle (rel-RMS <= 0.5 %, max-abs <=
    0.01: tests/test_windows_gpu.py's bars) and against `forward` on the utterance alone (rel-RMS <= 1e-3);
  * independence of the companions, the route (no solo call, a bounded graph set, replay = eager) and the fallback.

T = 1, 2 against the oracle: a one-frame utterance has little signal, so `_ragged_checks` measures the solo route (`forward`, which
this change does not touch) against the oracle at every length beside the batched one and prints both.  On an MI355X, V1: T = 1
0.069 % / 4e-5 batched against 0.072 % / 4e-5 solo, T = 2 0.076 % / 7e-5 against 0.074 % / 5e-5, the longer ones 0.086 - 0.089 % /
1.3e-4 - 1.7e-4 both ways; V3: 0.087 - 0.111 % / 3e-5 - 2.0e-4, identical both ways (the batched rows equal `forward` alone bit for
bit there; V1: rel-RMS 4.4e-4 - 5.4e-4, the windowed route's known distance to `forward`'s kernel choice).  The solo route is far
inside the bars at T = 1, 2, so they hold unchanged for every length."""
import copy

import numpy as np
import pytest
import torch

from oracle import hifigan as ohifi
from tests.oracle_util import hifi_state_dict_wn, rel_rms
from tests.test_hifigan_gpu import _mrf32_inputs, build
from tests.test_hifigan_v3_gpu import build_v3, v3_config
from tests.test_windows_cpu import generator_any
from tests.test_windows_gpu import _api, _mels, _stage
from tts_king_amd import windows
from tts_king_amd.synthetic import make_mel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = windows.W
SPF = 256
SENTINEL = 777.0


# ---------------------------------------------------------------------------------------------------- the gather

@pytest.mark.parametrize("v", [1, 31, 32, 33, 95])
@pytest.mark.parametrize("frames_first", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_mel_windows_with_short_rows(v, frames_first, dtype):
    """The short utterance last (the staging buffer behind it holds the sentinel), first (another utterance follows it) and between."""
    from tts_king_amd import ops
    for lens in ([200, v], [v, 200], [v], [W + 1, v, 50, 333]):
        mels = _mels(lens)
        plan = windows.plan_windows(lens, W, 14, short_rows=True)
        assert plan.short == [] and plan.has_short_rows
        got = ops.mel_windows(_stage(mels, plan, frames_first), torch.from_numpy(plan.table).to(DEV), W, dtype, frames_first)
        batch = torch.zeros(plan.N, 80, W)
        for r in range(plan.n_windows):
            u, s, n = int(plan.table[r, 0]), int(plan.table[r, 1]), int(plan.table[r, windows.VALID]) or W
            batch[r, :, :n] = mels[u][:, s:s + n]
        want = ops.nct_to_ntc(batch.to(DEV), dtype)
        torch.cuda.synchronize()
        assert got.shape == (plan.N, W, 80) and got.dtype == dtype
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), lens
        assert not bool((got.float() == SENTINEL).any())


def test_mel_windows_checks_a_short_row_against_the_buffer_with_its_own_length():
    """A short row at the very end of a staging buffer that holds fewer than W frames behind its start is read (v frames fit)."""
    from tts_king_amd import ops
    mel = _mels([40])[0]
    table = torch.tensor([[0, 0, 0, 40, 0, 0, 40, 0]], dtype=torch.int32, device=DEV)
    got = ops.mel_windows(mel.contiguous().reshape(-1).to(DEV), table, W)                 # (80, 40): 40 frames in all
    want = torch.zeros(1, 80, W)
    want[0, :, :40] = mel
    assert torch.equal(got.view(torch.int16), ops.nct_to_ntc(want.to(DEV), torch.float16).view(torch.int16))
    table[0, windows.VALID] = 41                                                          # one frame more than the buffer holds: skipped, zeros
    assert not bool(ops.mel_windows(mel.contiguous().reshape(-1).to(DEV), table, W).any())


# ---------------------------------------------------------------------------------------------------- the kernels

def _rows_case(C, s, dt, seed, N=3, vs=(7, 0, 95)):
    """x (N, W s, C) with row b valid for vs[b] frames (0 = all) and NaN past its end; the int32 length column inside a plan-shaped table."""
    g = torch.Generator().manual_seed(seed)
    ln = W * s
    x = (torch.randn(N, ln, C, generator=g) * 0.5).to(dt)
    prev = (torch.randn(N, ln, C, generator=g) * 0.5).to(dt)
    edges = [(v or W) * s for v in vs]
    for b, e in enumerate(edges):
        x[b, e:] = float("nan")
    table = torch.zeros(N, windows.ROW, dtype=torch.int32)
    table[:, windows.VALID] = torch.tensor(vs, dtype=torch.int32)
    return x.to(DEV), prev.to(DEV), edges, table.to(DEV)[:, windows.VALID], g


def _check_rows(run, x, prev, edges, frames, s, modes=(0, 1, 2)):
    """run(x, out, mode, rows) -> out.  Row b of the batched call, up to its edge, equals the plain call on that row alone, cut at the
    edge; `out` past the edge keeps its sentinel; with no length array the rows form equals the plain kernel on the whole tensor."""
    xf = torch.nan_to_num(x, nan=0.25)
    for mode in modes:
        base = prev.clone() if mode else torch.full_like(prev, 7.0)
        for b, e in enumerate(edges):
            base[b, e:] = 7.0
        got = run(x, base.clone(), mode, (frames, s))
        for b, e in enumerate(edges):
            want = run(x[b:b + 1, :e].contiguous(), base[b:b + 1, :e].clone().contiguous(), mode, None)
            assert torch.equal(got[b, :e].view(torch.int16), want[0].view(torch.int16)), (mode, b, e)
            assert bool((got[b, e:] == 7.0).all()), "stored past the end of row %d (mode %d)" % (b, mode)
        full = prev.clone()
        assert torch.equal(run(xf, full.clone(), mode, (None, s)).view(torch.int16), run(xf, full.clone(), mode, None).view(torch.int16)), mode
        # a length column of zeros = every row full
        zeros = torch.zeros_like(frames.contiguous())
        assert torch.equal(run(xf, full.clone(), mode, (zeros, s)).view(torch.int16), run(xf, full.clone(), mode, None).view(torch.int16)), mode


def _pair_weights(C, K, dt, g):
    from tts_king_amd import ops
    w1 = torch.randn(C, C, K, generator=g) * (C * K) ** -0.5
    w2 = torch.randn(C, C, K, generator=g) * (C * K) ** -0.5
    b1, b2 = (0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    return ops.pack_resblock_weight(w1.to(DEV), dtype=dt), b1, ops.pack_resblock_weight(w2.to(DEV), dtype=dt), b2


# (C, samples per frame of the V1 stage with C channels, K, dilation): conv_pair256 / conv_pair / conv_pair_fs<64> / conv_pair_fs<32>
@pytest.mark.parametrize("C,s,K,dil,dt", [(256, 8, 3, 1, torch.float16), (256, 8, 11, 5, torch.float16), (128, 64, 7, 3, torch.float16),
                                          (128, 64, 11, 5, torch.bfloat16), (64, 128, 7, 5, torch.float16), (64, 128, 11, 1, torch.bfloat16),
                                          (32, 256, 3, 3, torch.float16)])
def test_conv_pair_rows(C, s, K, dil, dt):
    from tts_king_amd import ops
    x, prev, edges, frames, g = _rows_case(C, s, dt, 1000 * K + C + dil)
    p1, b1, p2, b2 = _pair_weights(C, K, dt, g)
    run = lambda xx, out, mode, rows: ops.hifi_conv_pair(xx, p1, b1, p2, b2, K, dil, out=out, mode=mode, scale=1.0 / 3.0,
                                                         final_slope=0.1 if mode == 2 else 1.0, rows=rows)
    _check_rows(run, x, prev, edges, frames, s)


@pytest.mark.parametrize("C,s,K,dil,dt", [(64, 128, 3, 1, torch.float16), (64, 128, 7, 3, torch.float16), (64, 128, 11, 5, torch.float16),
                                          (64, 128, 11, 3, torch.bfloat16), (128, 64, 3, 5, torch.float16), (128, 64, 3, 1, torch.bfloat16)])
def test_conv_pair_ws_rows(C, s, K, dil, dt):
    """The weights-stationary pairs: also with the grid capped, so that a workgroup's run of tiles crosses rows of different lengths."""
    from tts_king_amd import ops
    x, prev, edges, frames, g = _rows_case(C, s, dt, 2000 * K + C + dil)
    p1, b1, p2, b2 = _pair_weights(C, K, dt, g)
    for cap in (0, 3):
        run = lambda xx, out, mode, rows: ops.hifi_conv_pair(xx, p1, b1, p2, b2, K, dil, out=out, mode=mode, scale=1.0 / 3.0,
                                                             final_slope=0.1 if mode == 2 else 1.0, ws=True, max_wgs=cap, rows=rows)
        _check_rows(run, x, prev, edges, frames, s)
    # and the two pair kernels agree with a row length as they do without
    a = ops.hifi_conv_pair(x, p1, b1, p2, b2, K, dil, out=torch.zeros_like(x), rows=(frames, s))
    b = ops.hifi_conv_pair(x, p1, b1, p2, b2, K, dil, out=torch.zeros_like(x), ws=True, rows=(frames, s))
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("C,s,K,dt", [(64, 128, 3, torch.float16), (64, 128, 7, torch.bfloat16), (64, 128, 11, torch.float16),
                                      (32, 256, 3, torch.float16), (32, 256, 7, torch.float16), (32, 256, 11, torch.bfloat16)])
def test_resblock1_rows(C, s, K, dt):
    from tts_king_amd import ops
    x, prev, edges, frames, g = _rows_case(C, s, dt, 3000 * K + C)
    ws = [ops.pack_resblock_weight((torch.randn(C, C, K, generator=g) * (C * K) ** -0.5).to(DEV), dtype=dt) for _ in range(6)]
    bs = [(0.05 * torch.randn(C, generator=g)).to(DEV) for _ in range(6)]
    run = lambda xx, out, mode, rows: ops.hifi_resblock1(xx, ws, bs, (1, 3, 5), out, K, mode=mode, scale=1.0 / 3.0, slope=0.1,
                                                         final_slope=0.1 if mode == 2 else 1.0, rows=rows)
    _check_rows(run, x, prev, edges, frames, s)


@pytest.mark.parametrize("C,s,K,dils,dt", [(128, 8, 3, (1, 2), torch.float16), (128, 8, 7, (2, 6), torch.float16), (64, 64, 5, (2, 6), torch.float16),
                                           (64, 64, 7, (3, 12), torch.bfloat16), (32, 256, 3, (1, 2), torch.float16), (32, 256, 7, (3, 12), torch.float16)])
def test_resblock2_rows(C, s, K, dils, dt):
    from tts_king_amd import ops
    assert ops.hifi_resblock2_supported(C, K, *dils)
    x, prev, edges, frames, g = _rows_case(C, s, dt, 4000 * K + C)
    p0, b0, p1, b1 = _pair_weights(C, K, dt, g)
    run = lambda xx, out, mode, rows: ops.hifi_resblock2(xx, p0, b0, p1, b1, K, dils, out=out, mode=mode, scale=1.0 / 3.0,
                                                         final_slope=0.1 if mode == 2 else 1.0, rows=rows)
    _check_rows(run, x, prev, edges, frames, s)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_mrf32_post_rows(dt):
    """The last stage: waveform and activated average of a short row = the plain kernel on the row alone, bit for bit."""
    from tts_king_amd import ops
    s, vs = SPF, (7, 0, 95, 1)
    x, ks, dil, ws, bs, wpost, bpost = _mrf32_inputs(dt, len(vs), W * s, 31)
    edges = [(v or W) * s for v in vs]
    for b, e in enumerate(edges):
        x[b, e:] = float("nan")
    frames = torch.tensor(vs, dtype=torch.int32, device=DEV)                 # a compact copy of the column: element stride 1
    stage = torch.full_like(x, 7.0)
    got = ops.hifi_mrf32_post(x, ws, bs, dil, ks, wpost, bpost, stage_out=stage, rows=(frames, s))
    for b, e in enumerate(edges):
        st1 = torch.empty(1, e, 32, dtype=dt, device=DEV)
        want = ops.hifi_mrf32_post(x[b:b + 1, :e].contiguous(), ws, bs, dil, ks, wpost, bpost, stage_out=st1)
        assert torch.equal(got[b, :, :e], want[0]), (b, float((got[b, :, :e] - want[0]).abs().max()))
        assert torch.equal(stage[b, :e].view(torch.int16), st1[0].view(torch.int16)) and bool((stage[b, e:] == 7.0).all())
    xf = torch.nan_to_num(x, nan=0.25)
    assert torch.equal(ops.hifi_mrf32_post(xf, ws, bs, dil, ks, wpost, bpost, rows=(None, s)), ops.hifi_mrf32_post(xf, ws, bs, dil, ks, wpost, bpost))


def test_zero_rows_past_and_bad_arguments():
    from tts_king_amd import ops
    x = torch.ones(4, W, 512, dtype=torch.float16, device=DEV)
    frames = torch.tensor([1, 0, 95, 200], dtype=torch.int32, device=DEV)   # 200 > W: clamped, nothing to zero
    ops.zero_rows_past(x, (frames, 1))
    torch.cuda.synchronize()
    for b, e in enumerate((1, W, 95, W)):
        assert bool((x[b, :e] == 1).all()) and not bool(x[b, e:].any())
    y = torch.ones(2, W * 8, 256, dtype=torch.bfloat16, device=DEV)
    ops.zero_rows_past(y, (frames[:2], 8))
    assert bool((y[0, :8] == 1).all()) and not bool(y[0, 8:].any()) and bool((y[1] == 1).all())
    with pytest.raises(ops.L.TtskError):
        ops.zero_rows_past(x, (frames, 0))                                                   # no samples per frame
    with pytest.raises(ops.L.TtskError):
        ops.zero_rows_past(x, (frames[:3], 1))                                               # three lengths for four rows
    with pytest.raises(ops.L.TtskError):
        ops.zero_rows_past(x, (frames.long(), 1))
    with pytest.raises(ops.L.TtskError):
        ops.hifi_conv_pair(x[:, :, :128].contiguous(), x, x, x, x, 3, 1, rows=(frames.cpu(), 8))   # a host length tensor


# ---------------------------------------------------------------------------------------------------- the ragged call

RAGGED = [1, 2, 13, 14, 15, 31, 50, 95, W, W + 1, 333]


def _ragged_checks(gen, oracle, lens):
    assert gen.short_rows()
    mels = _mels(lens, seed=3)
    out = gen.forward_ragged([m.to(DEV) for m in mels])
    torch.cuda.synchronize()
    assert len(out) == len(lens)
    for i, (m, y) in enumerate(zip(mels, out)):
        assert y.shape == (1, 1, SPF * lens[i]) and y.dtype == torch.float32
        want = oracle(m[None])
        solo = gen(m[None].to(DEV)).cpu()
        r, a, rs = rel_rms(y.cpu(), want), float((y.cpu() - want).abs().max()), rel_rms(y.cpu(), solo)
        ps, pa = rel_rms(solo, want), float((solo - want).abs().max())
        print("T=%d: vs oracle rel-RMS %.3f%% max-abs %.5f (forward alone vs oracle: %.3f%% %.5f); vs forward alone rel-RMS %.2e"
              % (lens[i], 100 * r, a, 100 * ps, pa, rs))
        assert r <= 0.005 and a <= 0.01
        assert rs <= 1e-3
    out2 = gen.forward_ragged([m.t().contiguous()[None] for m in mels], frames_first=True)
    assert all(torch.equal(a, b) for a, b in zip(out, out2))


def test_ragged_call_with_short_rows(cfg):
    gen = build(cfg, 11)
    sd = ohifi.fold_weight_norm(hifi_state_dict_wn(11))
    with torch.no_grad():
        _ragged_checks(gen, lambda m: ohifi.generator(sd, cfg.hifi, m), RAGGED)


def test_ragged_call_with_short_rows_v3(cfg):
    gen = build_v3(cfg, 11)
    sd = {k: v.detach().float().cpu() for k, v in gen.state_dict().items()}
    h = v3_config(cfg).hifi
    with torch.no_grad():
        _ragged_checks(gen, lambda m: generator_any(sd, h, m), RAGGED)


def test_a_call_of_full_windows_is_bit_for_bit_what_it_was(cfg):
    """No short utterance: the plan, the launches and the waveform of the windowed route as it stood (all rows full)."""
    gen = build(cfg, 11)
    lens = [W, 300, 2 * W + 5]
    mels = [m.to(DEV) for m in _mels(lens, seed=2)]
    plan = gen.plan(lens)
    old = windows.plan_windows(lens, W, gen.halo())
    assert np.array_equal(plan.table, old.table) and not plan.has_short_rows
    stage = gen.stage_mels(mels, old, False)
    table = torch.from_numpy(old.table).to(DEV)
    want = windows.split(gen.forward_windows(stage, table), old, SPF, {})
    rows = windows.split(gen.forward_windows(stage, table, row_lengths=True), old, SPF, {})     # the row kernels on full rows
    got = gen.forward_ragged(mels)
    for a, b, c in zip(got, want, rows):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_a_short_row_does_not_depend_on_its_companions(cfg):
    gen = build(cfg, 11)
    me = _mels([37], seed=1)[0].to(DEV)
    a = gen.forward_ragged([me] + [m.to(DEV) for m in _mels([20, 90], seed=2)])          # N = 3
    b = gen.forward_ragged([m.to(DEV) for m in _mels([300], seed=5)] + [me])             # 300 frames = 4 windows + 1: N = 6? (ladder)
    c = gen.forward_ragged([m.to(DEV) for m in _mels([64, 5], seed=7)] + [me])           # N = 3 again, another position
    Ns = [gen.plan(l).N for l in ([37, 20, 90], [300, 37], [64, 5, 37])]
    assert Ns[0] == Ns[2] != Ns[1]
    assert torch.equal(a[0], c[2])
    r = rel_rms(a[0].cpu(), b[1].cpu())
    print("the same 37-frame mel under N = %d and N = %d: rel-RMS %.2e" % (Ns[0], Ns[1], r))
    assert r <= 1e-3


def test_short_utterances_take_the_batched_route(cfg):
    """Eight utterances of 20-90 frames in a list call: neither `Generator.forward` nor `GraphedSynthesizer.wav` runs; 60 calls with random
    short lengths leave one graph per ladder value met and none per length; replay equals eager bit for bit."""
    api = _api(cfg, True)
    syn, gen = api._synth, api.model
    calls = {"forward": 0, "wav": 0}
    fwd, wav = gen.forward, syn.wav

    def count(name, fn):
        def inner(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return inner
    gen.forward, syn.wav = count("forward", fwd), count("wav", wav)
    try:
        lens = [20, 33, 47, 58, 64, 71, 85, 90]
        mels = [m.to(DEV) for m in _mels(lens, seed=4)]
        first = [y.clone() for y in syn.wav_ragged(mels)]                   # eager
        eager = gen.forward_ragged(mels)
        host = api.generate_ragged(mels)                                     # the int16 output is a key of its own: eager here
        third = [y.clone() for y in syn.wav_ragged(mels)]                   # captured
        assert len(syn._rag) == 1
        fourth = syn.wav_ragged(mels)                                        # replayed
        assert calls == {"forward": 0, "wav": 0}
        for i, T in enumerate(lens):
            assert first[i].shape == (1, 1, SPF * T)
            assert torch.equal(first[i], eager[i]) and torch.equal(third[i], eager[i]) and torch.equal(fourth[i], eager[i])
            assert np.array_equal(host[i], ohifi.to_int16(eager[i], 32768))
        rnd = np.random.RandomState(5)
        met = set()
        for k in range(60):
            ls = [int(t) for t in rnd.randint(1, W, size=rnd.randint(1, 13))]
            met.add(gen.plan(ls).N)
            out = syn.wav_ragged([m.to(DEV) for m in _mels(ls, seed=k)])
            assert [y.shape[-1] for y in out] == [SPF * t for t in ls]
        assert calls == {"forward": 0, "wav": 0}
        assert len(syn._voc) == 0
        # one graph per ladder value met (8 from the calls above), none per length
        assert len(syn._rag) <= len(met | {8}) and met <= {1, 2, 3, 4, 6, 8, 12}, (len(syn._rag), sorted(met))
    finally:
        gen.forward, syn.wav = fwd, wav


def test_fallback_keeps_the_solo_route(cfg):
    """A generator whose stages run conv by conv (fused kernels off) has no row kernels: `short_rows()` is False, short utterances go
    through `forward`, one call each, and the waveforms are those of the route as it stood."""
    gen = build(cfg, 11)
    gen.fused = False
    assert not gen.short_rows()
    lens = [30, W + 3, 64, 290]
    mels = [m.to(DEV) for m in _mels(lens, seed=6)]
    n = [0]
    fwd = gen.forward

    def counted(x):
        n[0] += 1
        return fwd(x)
    gen.forward = counted
    try:
        got = gen.forward_ragged(mels)
    finally:
        gen.forward = fwd
    assert n[0] == 2
    plan = windows.plan_windows(lens, W, gen.halo())
    assert plan.short == [0, 2]
    flat = gen.forward_windows(gen.stage_mels(mels, plan, False), torch.from_numpy(plan.table).to(DEV))
    want = windows.split(flat, plan, SPF, {i: gen(mels[i][None]) for i in plan.short})
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    from tts_king_amd import ops
    with pytest.raises(ops.L.TtskError):
        gen.forward_ntc(torch.zeros(1, W, 80, dtype=gen.act_dtype, device=DEV), row_frames=torch.tensor([5], dtype=torch.int32, device=DEV))
    gen.fused, gen.conv_pair = True, False                                   # the C = 256 / 128 stages conv by conv
    assert not gen.short_rows()
