"""GPU: windowed vocoding — the two data-movement kernels (csrc/windows.hip) bit for bit against torch slicing, a ragged call of
the V1 and V3 generators against the CPU oracle and against `forward` on each utterance alone, one graph per window count, and
the facades.

Bars: the kernels move data, so they are compared bit for bit (the gather's cast is `ops.nct_to_ntc`'s, the stitch's int16 is
`ops.to_int16`'s).  Ragged call vs the CPU oracle: the bars tests/test_hifigan_gpu.py holds for this generator (rel-RMS <= 0.5 %,
max-abs <= 0.01, which covers every seam sample); vs `forward` on the utterance alone: rel-RMS <= 1e-3, the bar of
test_batch_independence_and_determinism (kernel choice may differ with the batch shape, the arithmetic may not)."""
import copy

import numpy as np
import pytest
import torch

from oracle import hifigan as ohifi
from tests.oracle_util import hifi_state_dict_wn, rel_rms
from tests.test_hifigan_gpu import build
from tests.test_hifigan_v3_gpu import build_v3, v3_config
from tests.test_windows_cpu import generator_any
from tts_king_amd import windows
from tts_king_amd.synthetic import make_mel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = windows.W
SPF = 256


def _mels(lens, seed=0):
    return [make_mel(1, T, seed=seed + 7 * i + T)[0] for i, T in enumerate(lens)]          # (80, T_i) on the host


def _stage(mels, plan, frames_first):
    """The staging buffer as the product fills it, built with torch alone; unused frames hold a sentinel no window may read."""
    frames = plan.N * plan.W
    v = torch.full((frames, 80) if frames_first else (80, frames), 777.0)
    for i in plan.planned:
        o, T = plan.offsets[i], plan.lens[i]
        if frames_first:
            v[o:o + T] = mels[i].t()
        else:
            v[:, o:o + T] = mels[i]
    return v.reshape(-1).to(DEV)


# T = W, T = W + 1, an utterance one frame below W in the batch (not planned), window counts that need padding windows and that do not
KERNEL_CASES = [[W], [W + 1], [W, W - 1, W + 1, 333], [W - 1, 1000], [300, 50, 2 * W - 28 + 1, 3 * W]]


@pytest.mark.parametrize("lens", KERNEL_CASES)
@pytest.mark.parametrize("frames_first", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_mel_windows_equals_slicing_then_nct_to_ntc(lens, frames_first, dtype):
    from tts_king_amd import ops
    mels = _mels(lens)
    plan = windows.plan_windows(lens, W, 14)
    assert plan.N > 0
    got = ops.mel_windows(_stage(mels, plan, frames_first), torch.from_numpy(plan.table).to(DEV), W, dtype, frames_first)
    batch = torch.zeros(plan.N, 80, W)
    for r in range(plan.n_windows):
        u, s = int(plan.table[r, 0]), int(plan.table[r, 1])
        batch[r] = mels[u][:, s:s + W]
    want = ops.nct_to_ntc(batch.to(DEV), dtype)
    torch.cuda.synchronize()
    assert got.shape == (plan.N, W, 80) and got.dtype == dtype
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("lens", KERNEL_CASES)
def test_wav_stitch_equals_slicing_and_int16_equals_to_int16(lens):
    from tts_king_amd import ops
    plan = windows.plan_windows(lens, W, 14)
    y = (torch.rand(plan.N, 1, SPF * W, generator=torch.Generator().manual_seed(len(lens))) * 2.2 - 1.1).to(DEV)     # beyond full scale too
    table = torch.from_numpy(plan.table).to(DEV)
    flat = torch.full((plan.N * W * SPF,), 555.0, device=DEV)
    ops.wav_stitch(y, table, W, out=flat)
    i16 = ops.wav_stitch(y, table, W, int16_scale=32768.0)
    torch.cuda.synchronize()
    want = torch.cat([y[r, 0, (lo - s) * SPF:(hi - s) * SPF] for r, (u, s, lo, hi) in enumerate(plan.table[:plan.n_windows, :4].tolist())])
    n = plan.frames * SPF
    assert want.numel() == n and torch.equal(flat[:n], want)
    assert bool((flat[n:] == 555.0).all())                                  # nothing written past the call's own frames
    assert i16.dtype == torch.int16 and torch.equal(i16[:n], ops.to_int16(flat[:n].contiguous(), 32768.0))
    got = windows.split(flat, plan, SPF, {})
    for i in plan.planned:
        assert got[i].shape == (1, 1, SPF * lens[i])


def test_kernels_refuse_bad_arguments():
    from tts_king_amd import ops
    plan = windows.plan_windows([W], W, 14)
    table = torch.from_numpy(plan.table).to(DEV)
    with pytest.raises(ops.L.TtskError):
        ops.mel_windows(torch.zeros(W * 80, device=DEV), table, 48)                          # W not a multiple of 32
    with pytest.raises(ops.L.TtskError):
        ops.mel_windows(torch.zeros(W * 80), table, W)                                       # host tensor
    with pytest.raises(ops.L.TtskError):
        ops.wav_stitch(torch.zeros(2, 1, SPF * W, device=DEV), table, W)                     # rows != windows


RAGGED = [W, W + 1, 2 * W - 2 * 14 + 1, 333, 50, 1000]


def _ragged_checks(gen, oracle, lens):
    mels = _mels(lens, seed=3)
    out = gen.forward_ragged([m.to(DEV) for m in mels])
    torch.cuda.synchronize()
    assert len(out) == len(lens)
    for i, (m, y) in enumerate(zip(mels, out)):
        assert y.shape == (1, 1, SPF * lens[i]) and y.dtype == torch.float32
        want = oracle(m[None])
        solo = gen(m[None].to(DEV)).cpu()
        r, a, rs = rel_rms(y.cpu(), want), float((y.cpu() - want).abs().max()), rel_rms(y.cpu(), solo)
        print("T=%d: vs oracle rel-RMS %.3f%% max-abs %.5f; vs forward alone rel-RMS %.2e" % (lens[i], 100 * r, a, rs))
        assert r <= 0.005 and a <= 0.01
        assert rs <= 1e-3
    # FastSpeech2's layout, host tensors with a batch dimension: the same waveforms bit for bit
    out2 = gen.forward_ragged([m.t().contiguous()[None] for m in mels], frames_first=True)
    assert all(torch.equal(a, b) for a, b in zip(out, out2))


def test_ragged_call_vs_oracle_and_vs_forward_alone(cfg):
    gen = build(cfg, 11)
    assert gen.halo() == 14
    sd = ohifi.fold_weight_norm(hifi_state_dict_wn(11))
    with torch.no_grad():
        _ragged_checks(gen, lambda m: ohifi.generator(sd, cfg.hifi, m), RAGGED)


def test_ragged_call_v3(cfg):
    gen = build_v3(cfg, 11)
    assert gen.halo() == 12
    sd = {k: v.detach().float().cpu() for k, v in gen.state_dict().items()}
    h = v3_config(cfg).hifi
    with torch.no_grad():
        _ragged_checks(gen, lambda m: generator_any(sd, h, m), [W, W + 1, 2 * W - 2 * 12 + 1, 333, 50, 1000])


def test_forward_is_what_it_was(cfg):
    """`forward` = nct_to_ntc + `forward_ntc`: same waveform as the two steps by hand, bit for bit."""
    from tts_king_amd import ops
    gen = build(cfg, 3)
    mel = make_mel(2, 70, seed=4).to(DEV)
    assert torch.equal(gen(mel), gen.forward_ntc(ops.nct_to_ntc(mel, gen.act_dtype)))


def _api(cfg, graph):
    from hifiapi import HIFIapi
    c = copy.deepcopy(cfg)
    c.model_config["vocoder"]["use_cpu"] = False
    c.mi355x["hip_graph"] = graph
    return HIFIapi(c, "cuda:0")


def test_one_graph_per_window_count(cfg):
    api = _api(cfg, True)
    syn = api._synth
    calls = [[300, 200, 2 * W], [W + 5, 310, 250], [333, W, 3 * W - 60]]
    Ns = {windows.plan_windows(c, W, 14).N for c in calls}
    assert len(Ns) == 1 and len({tuple(c) for c in calls}) == 3
    outs = []
    for k, lens in enumerate(calls):
        mels = [m.to(DEV) for m in _mels(lens, seed=k)]
        outs.append((mels, [y.clone() for y in syn.wav_ragged(mels)]))
        assert len(syn._rag) == (0 if k == 0 else 1)                       # first sight eager, second captured, third replayed
    torch.cuda.synchronize()
    for mels, got in outs:                                                 # replayed (and eager) output = the eager call, bit for bit
        want = api.model.forward_ragged(mels)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    again = syn.wav_ragged(outs[0][0])                                     # the first call's lengths, now on the graph
    assert all(torch.equal(a, b) for a, b in zip(again, outs[0][1])) and len(syn._rag) == 1
    other = [m.to(DEV) for m in _mels([1000, 700], seed=9)]
    assert windows.plan_windows([1000, 700], W, 14).N not in Ns
    syn.wav_ragged(other)
    assert len(syn._rag) == 1
    y = syn.wav_ragged(other)
    assert len(syn._rag) == 2                                              # a different N adds exactly one graph
    assert all(torch.equal(a, b) for a, b in zip(y, api.model.forward_ragged(other)))


@pytest.mark.parametrize("graph", [False, True])
def test_facades(cfg, graph):
    api = _api(cfg, graph)
    lens = [W + 40, 60, 400]
    mels = _mels(lens, seed=5)
    for rep in range(3):                                                   # eager, captured, replayed when `graph`
        got = api.generate_ragged(mels if rep else [m[None] for m in mels])
        floats = api.model.forward_ragged([m.to(DEV) for m in mels])
        for i, g in enumerate(got):
            assert isinstance(g, np.ndarray) and g.dtype == np.int16 and g.shape == (1, 1, SPF * lens[i])
            assert np.array_equal(g, ohifi.to_int16(floats[i], 32768))     # the truncation of the float path
    # the tensor entry points give what they gave
    mel = make_mel(2, 40, seed=8)
    a = api.generate(mel)
    assert a.shape == (2, 1, SPF * 40) and np.array_equal(a, ohifi.to_int16(api.model(mel.to(DEV)), 32768))


def test_ttsking_mel_to_wav_takes_a_list(cfg):
    from tts_king import TTSKing
    k = TTSKing.__new__(TTSKing)                                           # the vocoder half only: no FastSpeech2 is built
    k.cfg, k.vocoder = cfg, _api(cfg, False)
    lens = [W + 3, 30, 290]
    mels = [m.t().contiguous()[None] for m in _mels(lens, seed=6)]         # (1, T_i, 80), FastSpeech2's layout
    got = k.mel_to_wav(mels)
    assert isinstance(got, list) and len(got) == 3
    want = k.vocoder.generate_ragged([m.transpose(1, 2) for m in mels])
    for g, w, T in zip(got, want, lens):
        assert g.dtype == np.int16 and g.shape == (1, 1, SPF * T) and np.array_equal(g, w)
    one = k.mel_to_wav(mels[2])
    assert one.shape == (1, 1, SPF * 290) and np.array_equal(one, k.vocoder.generate(mels[2].transpose(1, 2)))
