"""GPU: the HiFi-GAN V3 generator (ResBlock2, hifi/models.py:104-143; the published config_v3 through the unchanged `hifi:` keys)
on the fused ResBlock2 kernel (csrc/resblock2.hip, ttsk_hifi_resblock2): the kernel against fp64 math on its own 16-bit operands,
the generator's route, the fused route against the conv-by-conv one, the waveform against the reference's (tests/golden/
hifi_v3_b2_t32.npz) and HIFIapi on a V3 config.

Tolerances: kernel vs fp64 4 eps max|ref| (test_conv_pair_equals_two_window_convs' bar; x1 and lrelu(x1) rounded to 16 bits in
the fp64 restatement as the kernel rounds them); fused vs conv-by-conv waveform rel-RMS <= 2e-3 (the routes differ in where the
MRF sum is rounded); vs the reference the V1 bar: rel-RMS <= 0.5 %, max-abs <= 0.01, int16 within 0.5 % of full scale."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.oracle_util import GOLDEN, rel_rms
from tts_king_amd.synthetic import make_mel, seeded_fill

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V3 = dict(resblock="2", upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8], upsample_initial_channel=256,
          resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]])
V3_BLOCKS = [(C, K, d0, d1) for C in (128, 64, 32) for K, (d0, d1) in zip(V3["resblock_kernel_sizes"], V3["resblock_dilation_sizes"])]


def v3_config(cfg):
    c = copy.deepcopy(cfg)
    for k, v in V3.items():
        c.hifi[k] = v
    return c


def v3_state_dict_wn(weight_seed):
    g = np.load(os.path.join(GOLDEN, "hifi_v3_b2_t32.npz"))
    sd = {str(k): torch.zeros(tuple(int(x) for x in str(s).split(";"))) for k, s in zip(g["wn_keys"], g["wn_shapes"])}
    seeded_fill(sd, weight_seed)
    return sd


def build_v3(cfg, weight_seed, fold_on_device=True):
    from tts_king_amd.hifigan import Generator
    gen = Generator(v3_config(cfg).hifi)
    gen.load_state_dict(v3_state_dict_wn(weight_seed))
    if fold_on_device:
        gen.to(DEV)
        gen.remove_weight_norm()
    else:
        gen.remove_weight_norm()
        gen.to(DEV)
    return gen.eval()


def _lrelu(t, slope=0.1):
    return torch.where(t > 0, t, slope * t)


def _block_fp64(x, w0, b0, w1, b1, K, d0, d1, dt):
    """ResBlock2 (hifi/models.py:134-140) in fp64 on the kernel's 16-bit operands; x1 and lrelu(x1) rounded to 16 bits."""
    xd = x.double().cpu().transpose(1, 2)
    xl = _lrelu(x.float()).to(dt).double().cpu().transpose(1, 2)
    x1 = (F.conv1d(xl, w0.to(dt).double(), b0.double().cpu(), dilation=d0, padding=d0 * (K - 1) // 2) + xd).to(dt)
    xl1 = _lrelu(x1.float()).to(dt).double()
    y = F.conv1d(xl1, w1.to(dt).double(), b1.double().cpu(), dilation=d1, padding=d1 * (K - 1) // 2) + x1.double()
    return y.transpose(1, 2)


# every V3 block; ragged lengths, the tile sizes +- 1 (96 / 64 frames at C = 128, 192 at C = 64 / 32), lengths inside the 45-frame halo
CASES = ([(C, K, d0, d1, 2, 700, torch.float16) for C, K, d0, d1 in V3_BLOCKS] +
         [(C, K, d0, d1, 1, 5, torch.bfloat16 if C == 64 else torch.float16) for C, K, d0, d1 in V3_BLOCKS] +
         [(128, 3, 1, 2, 3, 95, torch.float16), (128, 5, 2, 6, 1, 97, torch.bfloat16), (128, 7, 3, 12, 3, 65, torch.float16),
          (128, 7, 3, 12, 1, 63, torch.bfloat16), (64, 3, 1, 2, 3, 191, torch.float16), (64, 7, 3, 12, 1, 193, torch.float16),
          (64, 5, 2, 6, 3, 383, torch.bfloat16), (32, 5, 2, 6, 1, 193, torch.float16), (32, 7, 3, 12, 3, 191, torch.bfloat16),
          (32, 3, 1, 2, 1, 30, torch.bfloat16), (128, 5, 2, 6, 3, 44, torch.float16), (32, 7, 3, 12, 3, 1000, torch.float16)])


@pytest.mark.parametrize("C,K,d0,d1,B,ln,dt", CASES)
def test_resblock2_vs_fp64(C, K, d0, d1, B, ln, dt):
    from tts_king_amd import ops
    g = torch.Generator().manual_seed(C * 7 + K * 1000 + ln + d1)
    x = torch.randn(B, ln, C, generator=g).to(dt).to(DEV)
    w0 = torch.randn(C, C, K, generator=g) * (C * K) ** -0.5
    w1 = torch.randn(C, C, K, generator=g) * (C * K) ** -0.5
    b0, b1 = (0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    p0, p1 = ops.pack_resblock_weight(w0.to(DEV), dtype=dt), ops.pack_resblock_weight(w1.to(DEV), dtype=dt)
    assert ops.hifi_resblock2_supported(C, K, d0, d1)
    got = ops.hifi_resblock2(x, p0, b0, p1, b1, K, (d0, d1))
    ref = _block_fp64(x, w0, b0, w1, b1, K, d0, d1, dt)
    eps = 2.0 ** (-10 if dt == torch.float16 else -7)
    bar = 4 * eps * float(ref.abs().max())
    err = float((got.double().cpu() - ref).abs().max())
    assert err <= bar, (err, bar)
    # the MRF modes: out += y, then out = lrelu((out + y) * scale, final_slope), scale 1/3, both consumers' slopes
    acc = got.clone()
    ops.hifi_resblock2(x, p0, b0, p1, b1, K, (d0, d1), out=acc, mode=1)
    assert float((acc.double().cpu() - (got.double().cpu() + ref)).abs().max()) <= bar
    for fs in (0.1, 0.01):
        out = acc.clone()
        ops.hifi_resblock2(x, p0, b0, p1, b1, K, (d0, d1), out=out, mode=2, scale=1.0 / 3.0, final_slope=fs)
        want = _lrelu((acc.double().cpu() + ref) / 3, fs)
        assert float((out.double().cpu() - want).abs().max()) <= bar


def test_resblock2_supported_and_rejects():
    from tts_king_amd import ops
    from tts_king_amd.lib import TtskError
    assert all(ops.hifi_resblock2_supported(*b) for b in V3_BLOCKS)
    assert not ops.hifi_resblock2_supported(256, 3, 1, 2)            # V1's first stage: not an instance
    assert not ops.hifi_resblock2_supported(128, 9, 1, 2)            # K = 9
    assert not ops.hifi_resblock2_supported(128, 7, 3, 14)           # conv1 halo 42 > 40 frames
    assert not ops.hifi_resblock2_supported(32, 7, 6, 12)            # conv0 halo 18 > 16 frames
    assert not ops.hifi_resblock2_supported(64, 7, 3, 17)            # conv1 halo 51 > 48 frames
    x = torch.zeros(1, 64, 128, dtype=torch.float16, device=DEV)
    p = ops.pack_resblock_weight(torch.zeros(128, 128, 3, device=DEV))
    b = torch.zeros(128, device=DEV)
    with pytest.raises(TtskError):
        ops.hifi_resblock2(x, p, b, p, b, 3, (1, 2), out=x)          # in place
    with pytest.raises(TtskError):
        ops.hifi_resblock2(x, p, b, p, b, 3, (1, 2), out=torch.zeros_like(x), mode=3)
    with pytest.raises(TtskError):
        ops.hifi_resblock2(x, p, b, p, b, 3, (1, 2), slope=1.5)
    with pytest.raises(TtskError):
        ops.hifi_resblock2(x, p, b, p, b, 3, (1, 2), mode=1)           # accumulates into a missing `out`


def test_v3_route_keeps_resblock2_convs_off_the_gemm(cfg, monkeypatch):
    """During a V3 forward no ResBlock2 convolution is an implicit-GEMM ops.conv1d: none of its weights has a ResBlock2 conv's tap-major
    shape (C, k, C) (the fused route packs no such weight at all)."""
    from tts_king_amd import ops
    gen = build_v3(cfg, 11)
    mel = make_mel(2, 40, seed=5).to(DEV)
    gen(mel)
    rb2_shapes = {(rb.convs[0].bias.shape[0], rb.k, rb.convs[0].bias.shape[0]) for rb in gen.resblocks if rb.kind == "2"}
    assert rb2_shapes == {(C, K, C) for C, K, _, _ in V3_BLOCKS} and len(gen.resblocks) == 9
    seen = []
    real = ops.conv1d

    def spy(x, W, *a, **kw):
        seen.append(tuple(W.shape))
        return real(x, W, *a, **kw)

    monkeypatch.setattr(ops, "conv1d", spy)
    calls = []
    real_rb2 = ops.hifi_resblock2
    monkeypatch.setattr(ops, "hifi_resblock2", lambda *a, **kw: calls.append(kw.get("mode")) or real_rb2(*a, **kw))
    gen(mel)
    assert not rb2_shapes & set(seen)
    assert calls == [0, 1, 2] * 3                  # three block launches per stage, the MRF average folded into the last


@pytest.mark.parametrize("B,T", [(2, 64), (8, 384)])
def test_v3_fused_route_vs_conv_by_conv(cfg, B, T):
    gen = build_v3(cfg, 3)
    mel = make_mel(B, T, seed=200 + T).to(DEV)
    fused = gen(mel)
    gen.resblock2_fused = False
    plain = gen(mel)
    gen.resblock2_fused = True
    assert fused.shape == plain.shape == (B, 1, 256 * T)
    r = rel_rms(fused.cpu(), plain.cpu())
    print("V3 B=%d T=%d fused vs conv-by-conv rel-RMS %.2e" % (B, T, r))
    assert r <= 2e-3 and bool(torch.isfinite(fused).all())


@pytest.mark.parametrize("fold_on_device", [True, False])
def test_v3_waveform_vs_reference_golden(cfg, fold_on_device):
    g = np.load(os.path.join(GOLDEN, "hifi_v3_b2_t32.npz"))
    gen = build_v3(cfg, int(g["weight_seed"]), fold_on_device)
    sd = gen.state_dict()
    assert sorted(sd.keys()) == sorted(str(k) for k in g["keys"]) and len(sd) == int(g["n_folded_keys"])
    for name in g.files:
        if name.startswith("fold/"):
            np.testing.assert_allclose(sd[name[5:]].cpu().reshape(-1)[:64].numpy(), g[name], rtol=1e-5, atol=1e-7)
    mel = make_mel(int(g["B"]), int(g["T"]), seed=int(g["seed"]))
    wav = gen(mel.to(DEV))
    torch.cuda.synchronize()
    assert wav.shape == (2, 1, 8192) and wav.dtype == torch.float32
    r, a = rel_rms(wav.cpu(), g["wav"]), float((wav.cpu() - torch.from_numpy(g["wav"])).abs().max())
    print("V3 waveform vs reference: rel-RMS %.3f%%  max-abs %.5f" % (100 * r, a))
    assert r <= 0.005 and a <= 0.01
    from oracle import hifigan as ohifi
    i16 = ohifi.to_int16(wav.cpu(), 32768.0)
    assert np.abs(i16.astype(np.int32) - g["int16"].astype(np.int32)).max() <= 164          # 0.5 % of full scale


def test_v3_hifiapi_generate_graph_replay(cfg):
    """HIFIapi on a config whose `hifi:` section is V3, with hip_graph: int16 (B, 1, 256 T), the replayed graph equal to eager
    launches bit for bit, and two different mels through the same graph do not alias."""
    import hifiapi
    from tts_king_amd import ops
    c = v3_config(cfg)
    c.mi355x["hip_graph"] = True
    api = hifiapi.HIFIapi(c, "cuda:0")
    assert api._synth is not None
    m1, m2 = make_mel(3, 48, seed=1), make_mel(3, 48, seed=2)

    def eager(m):
        with torch.no_grad():
            return ops.to_int16(api.model(m.to(DEV)), 32768.0).cpu().numpy()

    e1, e2 = eager(m1), eager(m2)
    outs = [api.generate(m1) for _ in range(3)]                    # eager, captured, replayed
    assert all(o.dtype == np.int16 and o.shape == (3, 1, 256 * 48) for o in outs)
    assert all(np.array_equal(o, e1) for o in outs)
    o2 = api.generate(m2)
    assert np.array_equal(o2, e2) and not np.array_equal(o2, e1)
    assert np.array_equal(outs[2], e1)                             # the earlier result was not overwritten by the replay
