"""GPU: the HiFi-GAN route that README calls "conv by conv on the implicit-GEMM kernel", at the channel counts of the published V2
generator (config_v2: 128 -> 64 -> 32 -> 16 -> 8, ResBlock1; hifi/models.py:12-95, :146-210) — the kernels at the shapes V2 gives
them against fp64, then the whole V2 generator against the suite's fp64 restatement (tests/test_windows_cpu.py: generator_any, pinned to
the reference's own waveform by tests/test_hifigan_v2_cpu.py) and the committed reference waveform.

Kernel bars.  Integer-valued operands (tests/test_gemm_gpu.py: rnd(ints=True)): every product and sum is exact in fp32, so the stored
16-bit tensor must EQUAL the fp64 result rounded once (LeakyReLU computed in fp32 first, as the epilogue does) — a dropped tap, phase
or column is a bit mismatch.  Gaussian operands: tests/test_gemm_gpu.py's check(), 2e-6 sqrt(K) (max|ref| + 1) for the fp32 summation
plus one storage rounding, 2^-8 max|ref| for bf16 and 2^-11 max|ref| for fp16.  conv_post (fp32 output): 2e-6 sqrt(C K)
(max|pre-tanh| + 1).  avg3: equal to fp32 math rounded once.  The fused ResBlock1 at C = 32: test_fused_resblock1_vs_oracle's bars and its
exact recomputation of the MRF modes.  Outputs start as a sentinel, so a row or column nobody stores cannot pass by luck.

Whole-generator bar: max(V1's bar, 1.5 x calibration), the calibration being the fp64 restatement with its weights and every stored
activation rounded to the storage type, against the plain one (tests/hifi_generic_ref.py: calibration).  Measured on MI355X, fp16
storage: rel-RMS 0.08-0.13 %, max-abs <= 2.3e-4 against the restatement, on a calibration of 0.08-0.13 % / <= 2.3e-4 (V1's bar 0.5 % /
0.01 holds at every shape; the figures per shape are in the tests' docstrings and in DESIGN.md 9.1)."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import hifigan as ohifi
from tests.hifi_generic_ref import (CAL_FACTOR, V1_BAR_BF16, V1_BAR_F16, V2_GOLDEN, calibration, conv1d_ref, conv_transpose_ref, lrelu32, stored,
                                    v2_config, v2_folded, v2_state_dict_wn)
from tests.oracle_util import rel_rms
from tests.test_gemm_gpu import check, rnd
from tts_king_amd import windows
from tts_king_amd.synthetic import make_mel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
ROUNDING = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
SENTINEL = 77.0


def _lrelu64(v, slope):
    return v if slope is None else torch.where(v > 0, v, slope * v)


def _cmp(out, v, slope, K, dt, ints, what):
    """`out` (16-bit, device) against the fp64 pre-activation value v: equal to v rounded once for an integer case, else inside check()'s bound."""
    if ints:
        want = stored(v, dt, slope)
        got = out.cpu()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), "%s: %d of %d elements differ, max %.4g" % (
            what, int((got != want).sum()), want.numel(), float((got.double() - want.double()).abs().max()))
        return
    try:
        check(out, _lrelu64(v, slope), K, rounding=ROUNDING[dt])
    except AssertionError as e:
        raise AssertionError("%s: (err, tol) = %s" % (what, e)) from None


def _sentinel(*shape, dt):
    return torch.full(shape, SENTINEL, dtype=dt, device=DEV)


# ------------------------------------------------------------------------------------------------------------ ops.conv1d
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("k", [3, 7, 11])
@pytest.mark.parametrize("Cin,Cout", [(16, 16), (8, 8), (16, 8), (8, 16), (80, 128)])
def test_conv1d_at_v2_widths_with_the_routes_epilogues(Cin, Cout, k, dt):
    """A tap's K run (8 or 16 values) shorter than a K tile, an output narrower than one 16-byte-slot row of a tile, fewer rows than a
    row tile (T = 1, 5), one frame over two tiles (257): plain, LRELU_OUT (convs1), R + C2 + C2_LRELU (convs2, both outputs) and R alone
    (the last pair), at every dilation the blocks use."""
    from tts_king_amd import ops
    for ints in (True, False):
        w = (rnd(Cout, Cin, k, seed=10 + k, ints=ints) * (1.0 if ints else (Cin * k) ** -0.5)).to(dt)
        b = rnd(Cout, seed=11, ints=ints)
        wk, bd = w.permute(0, 2, 1).contiguous().to(DEV), b.to(DEV)                     # (Cout, k, Cin)
        for dil in (1, 3, 5):
            for B in (1, 3):
                for T in (1, 5, 64, 257):
                    what = "Cin=%d Cout=%d k=%d dil=%d B=%d T=%d %s %s" % (Cin, Cout, k, dil, B, T, dt, "ints" if ints else "gauss")
                    x, r = rnd(B, T, Cin, seed=T + dil, ints=ints).to(dt), rnd(B, T, Cout, seed=T + 50, ints=ints).to(dt)
                    v, _ = conv1d_ref(x, w, b, dil)
                    vr, _ = conv1d_ref(x, w, b, dil, R=r)
                    xd, rd = x.to(DEV), r.to(DEV)
                    out = ops.conv1d(xd, wk, bd, dilation=dil, out=_sentinel(B, T, Cout, dt=dt))
                    _cmp(out, v, None, Cin * k, dt, ints, what + " plain")
                    out = ops.conv1d(xd, wk, bd, dilation=dil, out=_sentinel(B, T, Cout, dt=dt), flags=ops.LRELU_OUT, out_slope=0.1)
                    _cmp(out, v, 0.1, Cin * k, dt, ints, what + " LRELU_OUT")
                    c2 = _sentinel(B, T, Cout, dt=dt)
                    out = ops.conv1d(xd, wk, bd, dilation=dil, out=_sentinel(B, T, Cout, dt=dt), R=rd, C2=c2, flags=ops.C2_LRELU, out_slope=0.1)
                    _cmp(out, vr, None, Cin * k, dt, ints, what + " R+C2: first output")
                    _cmp(c2, vr, 0.1, Cin * k, dt, ints, what + " R+C2: second output")
                    out = ops.conv1d(xd, wk, bd, dilation=dil, out=_sentinel(B, T, Cout, dt=dt), R=rd)
                    _cmp(out, vr, None, Cin * k, dt, ints, what + " R alone")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,T", [(1, 5), (1, 64), (3, 257)])
def test_lockstep_grouped_convs_equal_the_single_launches(B, T, dt):
    """`Generator._resblocks_lockstep` at C = 16: conv m of the three blocks (k = 3, 7, 11) as ONE grouped launch on the 128-row tile,
    against `Generator._resblock`, which launches each conv alone on the tile the planner picks for it: bit-equal, and the blocks
    close to the oracle's res_block1 on the same 16-bit operands (test_fused_resblock1_vs_oracle's bars)."""
    from tts_king_amd import ops
    from tts_king_amd.hifigan import Generator
    C, dil = 16, (1, 3, 5)
    g = torch.Generator().manual_seed(B * 1000 + T)
    x = torch.randn(B, T, C, generator=g).to(dt)
    xl = lrelu32(x, 0.1).to(dt)
    rbs, packs, sds = [], [], []
    for k in (3, 7, 11):
        rbs.append(types.SimpleNamespace(kind="1", k=k, dilation=dil))
        ws = [(torch.randn(C, C, k, generator=g) * (C * k) ** -0.5).to(dt) for _ in range(6)]        # convs1[0..2], convs2[0..2]
        bs = [0.1 * torch.randn(C, generator=g) for _ in range(6)]
        packs.append([(w.permute(0, 2, 1).contiguous().to(DEV), b.to(DEV)) for w, b in zip(ws, bs)])
        sd = {}
        for m in range(3):
            sd["r.convs1.%d.weight" % m], sd["r.convs1.%d.bias" % m] = ws[m].float(), bs[m]
            sd["r.convs2.%d.weight" % m], sd["r.convs2.%d.bias" % m] = ws[3 + m].float(), bs[3 + m]
        sds.append(sd)
    me = types.SimpleNamespace(window_conv=False)
    xd, xld = x.to(DEV), xl.to(DEV)
    grouped = Generator._resblocks_lockstep(me, rbs, packs, xd, xld)
    singles = [Generator._resblock(me, rb, pk, xd, xld) for rb, pk in zip(rbs, packs)]
    torch.cuda.synchronize()
    tol = 0.008 if dt == torch.bfloat16 else 0.001
    for rb, a, s, sd in zip(rbs, grouped, singles, sds):
        assert a.shape == s.shape == (B, T, C)
        assert torch.equal(a.view(torch.int16), s.view(torch.int16)), "k=%d: grouped and single launches differ by %.3g" % (
            rb.k, float((a.float() - s.float()).abs().max()))
        with torch.no_grad():
            want = ohifi.res_block1(sd, "r.", x.float().transpose(1, 2), rb.k, dil).transpose(1, 2)
        got = s.float().cpu()
        r = rel_rms(got, want)
        print("C=16 k=%d B=%d T=%d %s: block vs oracle rel-RMS %.3f%%" % (rb.k, B, T, dt, 100 * r))
        assert r <= tol and float((got - want).abs().max()) <= 6 * tol * float(want.abs().max())


# ------------------------------------------------------------------------------------------------------------ ops.conv_transpose1d
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Cin,Cout,k,s", [(128, 64, 16, 8), (64, 32, 16, 8), (32, 16, 4, 2), (16, 8, 4, 2), (32, 16, 8, 4)])
def test_conv_transpose_at_v2_geometries(Cin, Cout, k, s, dt):
    """The polyphase GEMMs with the output-row remap, with and without the input activation and the second activated output (`C2=axl`,
    C2_LRELU: what the C = 16 / 8 stages ask for), against fp64 ConvTranspose1d: the whole output, and every phase's row at the first
    and last two input frames on its own (its own max in the bound), so that a phase's edge is not averaged away."""
    from tts_king_amd import ops
    Bsz = 2
    for ints in (True, False):
        w = (rnd(Cin, Cout, k, seed=19, ints=ints) * (1.0 if ints else (Cin * k / s) ** -0.5)).to(dt)      # torch's (Cin, Cout, k)
        b = rnd(Cout, seed=20, ints=ints)
        wp, bd = w.permute(2, 1, 0).contiguous().to(DEV), b.to(DEV)                     # (k, Cout, Cin)
        for T in (1, 2, 37, 130):
            x = rnd(Bsz, T, Cin, seed=18 + T, ints=ints).to(dt)
            for in_slope in (0.0, 0.5 if ints else 0.1):                                # 0.5 keeps an integer case exact in 16 bits
                xin = x if not in_slope else lrelu32(x, in_slope).to(dt)                # the kernel rounds lrelu(x) to 16 bits
                ref = conv_transpose_ref(xin, w, b, s, k)
                for second in (False, True):
                    what = "%d->%d k=%d s=%d T=%d %s %s in_slope=%g%s" % (Cin, Cout, k, s, T, dt, "ints" if ints else "gauss", in_slope,
                                                                          " C2" if second else "")
                    c2 = _sentinel(Bsz, T * s, Cout, dt=dt) if second else None
                    out = ops.conv_transpose1d(x.to(DEV), wp, bd, s, k, out=_sentinel(Bsz, T * s, Cout, dt=dt), in_slope=in_slope,
                                               flags=ops.C2_LRELU if second else 0, C2=c2, out_slope=0.1)
                    assert out.shape == ref.shape == (Bsz, T * s, Cout)
                    outs = [(out, None, "")] + ([(c2, 0.1, " second output")] if second else [])
                    for o, slope, tag in outs:
                        o = o.cpu()
                        _cmp(o, ref, slope, Cin * k // s, dt, ints, what + tag)
                        for t in sorted({0, 1, T - 2, T - 1} & set(range(T))):
                            for ph in range(s):
                                row = t * s + ph
                                _cmp(o[:, row], ref[:, row], slope, Cin * k // s, dt, ints, what + tag + " frame %d phase %d" % (t, ph))


def test_conv_transpose_refuses_what_it_does_not_compute():
    """k = 11, stride 5: phase 0 owns taps 0, 5 and 10, and k // stride = 2 taps per phase would drop tap 10; k = 7, stride 2 (and k = 6,
    stride 3: k - stride odd) would also give another length than torch.  A TtskError, no tensor."""
    from tts_king_amd import ops
    from tts_king_amd.lib import TtskError
    for k, s in [(11, 5), (7, 2), (6, 3), (3, 8)]:
        x = torch.zeros(1, 4, 16, dtype=torch.float16, device=DEV)
        wp = torch.zeros(k, 8, 16, dtype=torch.float16, device=DEV)
        with pytest.raises(TtskError) as e:
            ops.conv_transpose1d(x, wp, torch.zeros(8, device=DEV), s, k)
        assert "kernel size %d" % k in str(e.value) and "stride %d" % s in str(e.value)


# ------------------------------------------------------------------------------------------------------------ conv_post, avg3, fused block
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C", [8, 16, 32])
def test_conv_post_at_narrow_widths(C, dt):
    from tts_king_amd import ops
    K = 7
    g = torch.Generator().manual_seed(C)
    w = (torch.randn(1, C, K, generator=g) * (C * K) ** -0.5).to(dt)
    b = 0.1 * torch.randn(1, generator=g)
    wk = w.permute(0, 2, 1).contiguous().to(DEV)                                        # (1, k, C)
    for B in (1, 3):
        for ln in (1, 6, 255, 256, 257, 1000):
            x = torch.randn(B, ln, C, generator=g).to(dt)
            pre = F.conv1d(x.double().transpose(1, 2), w.double(), b.double(), padding=K // 2)
            out = ops.hifi_conv_post(x.to(DEV), wk, b.to(DEV))
            assert out.shape == (B, 1, ln) and out.dtype == torch.float32
            err = float((out.cpu().double() - torch.tanh(pre)).abs().max())
            tol = 2e-6 * (C * K) ** 0.5 * (float(pre.abs().max()) + 1)
            assert err <= tol, ("C=%d B=%d len=%d %s" % (C, B, ln, dt), err, tol)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("slope", [0.1, 0.01])
@pytest.mark.parametrize("C", [8, 16])
def test_avg3_at_narrow_widths_is_fp32_math_rounded_once(C, slope, dt):
    from tts_king_amd import ops
    g = torch.Generator().manual_seed(C)
    for B, ln in ((1, 1), (3, 257), (2, 1000)):
        a, b, c = [torch.randn(B, ln, C, generator=g).to(dt) for _ in range(3)]
        want = lrelu32(((a.float() + b.float()) + c.float()) * torch.tensor(1.0 / 3.0, dtype=torch.float32), slope).to(dt)
        got = ops.avg3(a.to(DEV), b.to(DEV), c.to(DEV), 1.0 / 3.0, out=_sentinel(B, ln, C, dt=dt), slope=slope).cpu()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (B, ln, int((got != want).sum()))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [3, 7, 11])
@pytest.mark.parametrize("B,ln", [(3, 5), (2, 257)])
def test_fused_resblock1_as_a_middle_stage(K, B, ln, dt):
    """ttsk_hifi_resblock1 at C = 32 where V2 puts it: mode 2 with final_slope = 0.1 and scale = 1/3, feeding an upsampler (V1 runs it
    with final_slope = 0.01 before conv_post, and never as three launches at C = 32).  test_fused_resblock1_vs_oracle's comparison and its
    recomputation of the modes from the stored 16-bit values."""
    from tts_king_amd import ops
    C = 32
    g = torch.Generator().manual_seed(C * K + ln)
    x = torch.randn(B, ln, C, generator=g).to(dt)
    ws = [(torch.randn(C, C, K, generator=g) * (C * K) ** -0.5).to(dt) for _ in range(6)]
    bs = [0.1 * torch.randn(C, generator=g) for _ in range(6)]
    sd = {}
    for m in range(3):
        sd["r.convs1.%d.weight" % m], sd["r.convs1.%d.bias" % m] = ws[2 * m].float(), bs[2 * m]
        sd["r.convs2.%d.weight" % m], sd["r.convs2.%d.bias" % m] = ws[2 * m + 1].float(), bs[2 * m + 1]
    with torch.no_grad():
        want = ohifi.res_block1(sd, "r.", x.float().transpose(1, 2), K, (1, 3, 5)).transpose(1, 2)
    assert ops.hifi_resblock1_supported(C, K)
    wk = [ops.pack_resblock_weight(w.float().to(DEV), dtype=dt) for w in ws]
    bd = [b.to(DEV) for b in bs]
    out = _sentinel(B, ln, C, dt=dt)
    ops.hifi_resblock1(x.to(DEV), wk, bd, (1, 3, 5), out, K, mode=0)
    got = out.float().cpu()
    tol = 0.008 if dt == torch.bfloat16 else 0.001
    r = rel_rms(got, want)
    print("C=32 K=%d B=%d len=%d %s: rel-RMS %.3f%%" % (K, B, ln, dt, 100 * r))
    assert r <= tol and float((got - want).abs().max()) <= 6 * tol * float(want.abs().max())
    out2 = out.clone()
    ops.hifi_resblock1(x.to(DEV), wk, bd, (1, 3, 5), out2, K, mode=1)
    assert torch.equal(out2.cpu(), (got + got).to(dt))
    ops.hifi_resblock1(x.to(DEV), wk, bd, (1, 3, 5), out2, K, mode=2, scale=1.0 / 3.0, final_slope=0.1)
    want2 = ((got + got).to(dt).float() + got) * (1.0 / 3.0)
    assert torch.equal(out2.cpu(), torch.where(want2 > 0, want2, want2 * 0.1).to(dt))


# ------------------------------------------------------------------------------------------------------------ the whole V2 generator
def build_v2(cfg, weight_seed, fold_on_device=True):
    from tts_king_amd.hifigan import Generator
    gen = Generator(v2_config(cfg).hifi)
    gen.load_state_dict(v2_state_dict_wn(weight_seed))
    if fold_on_device:
        gen.to(DEV)
        gen.remove_weight_norm()
    else:
        gen.remove_weight_norm()
        gen.to(DEV)
    return gen.eval()


WEIGHT_SEED = 7                                       # the golden's
SHAPES = [(1, 1), (3, 7), (2, 32), (2, 100)]
_CAL = {}


def _mel(B, T):
    return make_mel(B, T, seed=21 if (B, T) == (2, 32) else 100 + T)                    # (2, 32): the golden's mel


def _calibrated(cfg, B, T, dt):
    """(calibration rel-RMS, calibration max-abs, fp64 restatement's waveform) of a shape and storage type, computed once."""
    if (B, T, dt) not in _CAL:
        _CAL[(B, T, dt)] = calibration(v2_folded(WEIGHT_SEED), v2_config(cfg).hifi, _mel(B, T), dt)
    return _CAL[(B, T, dt)]


@pytest.mark.parametrize("B,T", SHAPES)
def test_v2_waveform_vs_fp64_restatement(cfg, B, T):
    """fp16 storage (the product's).  Bars max(0.5 %, 1.5 x calibration) rel-RMS and max(0.01, 1.5 x calibration) max-abs; the golden
    (2, 32) case also against the reference's own waveform.  Measured on MI355X, rel-RMS / max-abs (calibration):
        (1, 1)    0.084 % / 4.7e-5  (0.081 % / 4.3e-5)
        (3, 7)    0.130 % / 1.8e-4  (0.127 % / 1.6e-4)
        (2, 32)   0.131 % / 2.1e-4  (0.131 % / 1.8e-4); against the reference's waveform 0.131 % / 2.1e-4
        (2, 100)  0.131 % / 2.3e-4  (0.131 % / 2.3e-4)
    so both bars are V1's, 0.5 % and 0.01, at every shape."""
    r_cal, a_cal, want = _calibrated(cfg, B, T, torch.float16)
    bar_r, bar_a = max(V1_BAR_F16[0], CAL_FACTOR * r_cal), max(V1_BAR_F16[1], CAL_FACTOR * a_cal)
    gen = build_v2(cfg, WEIGHT_SEED)
    assert gen.stage_routes() == ["pair", "fused", "gemm", "gemm"] and not gen.short_rows()
    got = gen(_mel(B, T).to(DEV)).cpu()
    assert got.shape == want.shape == (B, 1, 256 * T) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    r, a = rel_rms(got, want), float((got.double() - want).abs().max())
    print("V2 B=%d T=%d fp16: rel-RMS %.4f%% max-abs %.2e (calibration %.4f%% / %.2e -> bars %.3f%% / %.3g)" % (
        B, T, 100 * r, a, 100 * r_cal, a_cal, 100 * bar_r, bar_a))
    assert r <= bar_r and a <= bar_a
    if (B, T) == (2, 32):
        g = np.load(V2_GOLDEN)
        rg, ag = rel_rms(got, g["wav"]), float((got - torch.from_numpy(g["wav"])).abs().max())
        print("V2 golden vs the reference's waveform: rel-RMS %.4f%% max-abs %.2e" % (100 * rg, ag))
        assert rg <= bar_r and ag <= bar_a


@pytest.mark.parametrize("B,T", SHAPES)
def test_v2_bf16_storage_variant(cfg, B, T):
    """`act_dtype = bf16`: bar max(1.5 % — test_bf16_storage_variant's for V1 —, 1.5 x the bf16 calibration) rel-RMS.  Measured on MI355X
    (calibration):
        (1, 1)    0.69 % / 3.7e-4  (0.68 % / 3.8e-4) -> bar 1.50 %
        (3, 7)    1.04 % / 1.3e-3  (1.03 % / 1.3e-3) -> bar 1.54 %
        (2, 32)   1.04 % / 1.3e-3  (1.05 % / 1.7e-3) -> bar 1.58 %
        (2, 100)  1.04 % / 1.8e-3  (1.05 % / 1.7e-3) -> bar 1.57 %"""
    r_cal, a_cal, want = _calibrated(cfg, B, T, torch.bfloat16)
    bar = max(V1_BAR_BF16, CAL_FACTOR * r_cal)
    gen = build_v2(cfg, WEIGHT_SEED)
    gen.act_dtype = torch.bfloat16
    got = gen(_mel(B, T).to(DEV)).cpu()
    r, a = rel_rms(got, want), float((got.double() - want).abs().max())
    print("V2 B=%d T=%d bf16: rel-RMS %.3f%% max-abs %.2e (calibration %.3f%% / %.2e -> bar %.2f%%)" % (B, T, 100 * r, a, 100 * r_cal, a_cal, 100 * bar))
    assert got.shape == (B, 1, 256 * T) and r <= bar


def test_v2_route_pairs_then_fused_then_conv_by_conv(cfg, monkeypatch):
    """Which kernels a V2 forward launches: C = 64 on the pair kernels (its k = 3 block on the six-conv kernel, as at V1's C = 64 stage),
    C = 32 on the fused block in modes 0 / 1 / 2 feeding an upsampler (not the fused last stage), C = 16 and C = 8 conv by conv on the
    implicit-GEMM kernel with the polyphase upsamplers' second output, avg3 and the streaming conv_post.  Stays true, and keeps this
    file on the generic route, if a fused kernel for the narrow stages is added later only by changing it."""
    from tts_king_amd import ops
    gen = build_v2(cfg, WEIGHT_SEED)
    mel = _mel(2, 32).to(DEV)
    gen(mel)
    seen = {n: [] for n in ("conv1d", "conv_transpose1d", "avg3", "hifi_conv_post", "hifi_conv_pair", "hifi_resblock1", "hifi_mrf32_post")}

    def spy(name, describe):
        real = getattr(ops, name)

        def f(*a, **kw):
            seen[name].append(describe(a, kw))
            return real(*a, **kw)
        monkeypatch.setattr(ops, name, f)

    spy("conv1d", lambda a, kw: (a[0].shape[2], a[1].shape[0], a[1].shape[1], kw.get("dilation", 1), kw.get("flags", 0), kw.get("R") is not None,
                                 kw.get("C2") is not None, kw.get("group") is not None))
    spy("conv_transpose1d", lambda a, kw: (a[0].shape[2], a[1].shape[1], a[3], a[4], kw.get("C2") is not None, kw.get("flags", 0)))
    spy("avg3", lambda a, kw: (a[0].shape[2], kw.get("slope")))
    spy("hifi_conv_post", lambda a, kw: a[0].shape[2])
    spy("hifi_conv_pair", lambda a, kw: (a[0].shape[2], a[5], a[6], kw.get("mode", 0)))
    spy("hifi_resblock1", lambda a, kw: (a[0].shape[2], a[5], kw.get("mode", 0), kw.get("final_slope", 1.0)))
    spy("hifi_mrf32_post", lambda a, kw: a[0].shape[2])
    gen(mel)
    # C = 64: k = 7 and 11 as three pair launches each, the last with the block's MRF mode; k = 3 on the six-conv kernel
    assert [p[:3] for p in seen["hifi_conv_pair"]] == [(64, k, d) for k in (7, 11) for d in (1, 3, 5)]
    assert [p[3] for p in seen["hifi_conv_pair"]] == [0, 0, 1, 0, 0, 2]
    assert seen["hifi_resblock1"] == [(64, 3, 0, 1.0), (32, 3, 0, 1.0), (32, 7, 1, 1.0), (32, 11, 2, 0.1)]
    assert seen["hifi_mrf32_post"] == []
    # C = 16 / 8: 18 grouped implicit-GEMM convs per stage, convs1 dilated with LRELU_OUT, convs2 with the residual and, but for the
    # last pair, the second activated output
    gemm = [c for c in seen["conv1d"] if c[0] in (16, 8)]
    assert not [c for c in seen["conv1d"] if c[0] in (64, 32)]
    for C in (16, 8):
        mine = [c for c in gemm if c[0] == C]
        assert len(mine) == 18 and all(c[1] == C and c[7] for c in mine)
        c1 = [c for c in mine if not c[5]]
        c2 = [c for c in mine if c[5]]
        assert sorted((c[2], c[3]) for c in c1) == sorted((k, d) for k in (3, 7, 11) for d in (1, 3, 5)) and all(c[4] == ops.LRELU_OUT for c in c1)
        assert sorted(c[2] for c in c2) == [3] * 3 + [7] * 3 + [11] * 3 and all(c[3] == 1 for c in c2)
        assert sum(1 for c in c2 if c[6] and c[4] == ops.C2_LRELU) == 6 and sum(1 for c in c2 if not c[6] and c[4] == 0) == 3
    assert (32, 16, 2, 4, True, ops.C2_LRELU) in seen["conv_transpose1d"] and (16, 8, 2, 4, True, ops.C2_LRELU) in seen["conv_transpose1d"]
    assert seen["avg3"] == [(16, 0.1), (8, 0.01)]
    assert seen["hifi_conv_post"] == [8]


def test_v2_hifiapi_graph_replay_is_bit_identical_to_eager(cfg):
    """HIFIapi on a V2 config with hip_graph: the captured and the replayed call equal the eager launches bit for bit (the grouped
    launches' tables travel in kernel arguments, their split-K workspaces come from the graph's pool), and a replay with another mel
    does not alias."""
    import hifiapi
    from tts_king_amd import ops
    c = v2_config(cfg)
    c.model_config["vocoder"]["use_cpu"] = False
    c.mi355x["hip_graph"] = True
    api = hifiapi.HIFIapi(c, "cuda:0")
    assert api._synth is not None and api.model.stage_routes()[2:] == ["gemm", "gemm"]
    m1, m2 = make_mel(3, 40, seed=1), make_mel(3, 40, seed=2)

    def eager(m):
        with torch.no_grad():
            return ops.to_int16(api.model(m.to(DEV)), 32768.0).cpu().numpy()

    e1, e2 = eager(m1), eager(m2)
    outs = [api.generate(m1) for _ in range(3)]                    # eager, captured, replayed
    assert all(o.dtype == np.int16 and o.shape == (3, 1, 256 * 40) for o in outs)
    assert all(np.array_equal(o, e1) for o in outs)
    o2 = api.generate(m2)
    assert np.array_equal(o2, e2) and not np.array_equal(o2, e1)
    assert np.array_equal(outs[2], e1)


def test_v2_ragged_call_sends_short_utterances_solo(cfg):
    """`short_rows()` is False for V2 (the conv-by-conv stages take no row length): an utterance shorter than a window goes through the
    generator alone, the others as windows.  generate_ragged on 20, 96 (= W) and 150 frames against each utterance alone: rel-RMS
    <= 1e-3 on the int16 samples, tests/test_windows_gpu.py's bar for V1.  The halo is V1's: the same ResBlocks and upsamplers."""
    import hifiapi
    c = v2_config(cfg)
    c.model_config["vocoder"]["use_cpu"] = False
    c.mi355x["hip_graph"] = False
    api = hifiapi.HIFIapi(c, "cuda:0")
    gen = api.model
    assert not gen.short_rows() and gen.halo() == windows.receptive_halo(cfg.hifi) == 14
    lens = [20, windows.W, 150]
    plan = gen.plan(lens)
    assert plan.short == [0] and plan.planned == [1, 2] and not plan.has_short_rows
    mels = [make_mel(1, T, seed=3 + 7 * i + T)[0] for i, T in enumerate(lens)]
    got = api.generate_ragged(mels)
    for m, y, T in zip(mels, got, lens):
        solo = api.generate(m[None])
        assert y.dtype == np.int16 and y.shape == solo.shape == (1, 1, 256 * T)
        r = rel_rms(y.astype(np.float64), solo.astype(np.float64))
        print("V2 ragged T=%d vs alone: rel-RMS %.2e (int16)" % (T, r))
        assert r <= 1e-3
    assert np.array_equal(got[0], api.generate(mels[0][None]))     # the short one IS a solo run


def test_other_than_three_resblocks_is_refused_before_any_launch(cfg, monkeypatch):
    from tts_king_amd import ops
    from tts_king_amd.hifigan import Generator
    c = v2_config(cfg)
    c.hifi["resblock_kernel_sizes"], c.hifi["resblock_dilation_sizes"] = [3, 7], [[1, 3, 5], [1, 3, 5]]
    gen = Generator(c.hifi)
    gen.reset_parameters(3)
    gen.to(DEV)
    gen.remove_weight_norm()
    launched = []
    for name in ("nct_to_ntc", "pack_conv_weight", "pack_resblock_weight", "conv1d", "conv_transpose1d"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **kw: launched.append(_n) or _r(*a, **kw))
    with pytest.raises(NotImplementedError):
        gen(make_mel(1, 8, seed=1).to(DEV))
    assert launched == []
