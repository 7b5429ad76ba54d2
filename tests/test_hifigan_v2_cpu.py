"""CPU: the HiFi-GAN V2 generator (config_v2: `upsample_initial_channel: 128`, ResBlock1; its C = 16 and C = 8 stages run conv by
conv on the implicit-GEMM kernel) — state-dict keys and shapes as recorded from the reference in tests/golden/hifi_v2_b2_t32.npz, the
suite's plain-torch restatement pinned to the reference's own waveform, what the generator refuses, and negative controls of the
comparisons tests/test_hifigan_generic_gpu.py makes (hifi/models.py:12-95, :146-210).

Bars: restatement in fp64 vs the reference's fp32 waveform <= 1e-5 max-abs (the bar of the V3 restatement: fp32 rounding through
~40 layers of a waveform below 0.14).  A refusal is a TtskError that names the stage and its (k, stride).  A negative control must
break exact equality on the integer-valued kernel cases and exceed the whole-generator bar max(V1's bar, 1.5 x calibration) on the
golden (2, 32) case."""
import numpy as np
import pytest
import torch

from tests.hifi_generic_ref import (CAL_FACTOR, V1_BAR_F16, V2, V2_GOLDEN, calibration, conv1d_ref, conv_transpose_ref, stored, v2_config,
                                    v2_folded)
from tests.oracle_util import rel_rms
from tests.test_hifigan_v3_cpu import _shapes
from tests.test_windows_cpu import generator_any
from tts_king_amd import windows
from tts_king_amd.lib import TtskError
from tts_king_amd.synthetic import make_mel


def test_v2_state_dict_keys_and_shapes_match_the_reference(cfg):
    from tts_king_amd.hifigan import Generator
    g = np.load(V2_GOLDEN)
    for k, v in V2.items():                                                   # the fixture was made with this configuration
        assert np.array_equal(g["cfg/" + k], np.array(v))
    gen = Generator(v2_config(cfg).hifi)
    assert all(rb.kind == "1" and rb.dilation == (1, 3, 5) for rb in gen.resblocks) and len(gen.resblocks) == 12
    assert [u.bias.shape[0] for u in gen.ups] == [64, 32, 16, 8]
    sd = gen.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["wn_keys"]] and len(sd) == int(g["n_wn_keys"])
    assert [tuple(v.shape) for v in sd.values()] == _shapes(g["wn_shapes"])
    ckpt = {k: torch.full(v.shape, 0.5) for k, v in sd.items()}
    gen.load_state_dict(ckpt, strict=True)
    gen.remove_weight_norm()
    sdf = gen.state_dict()
    assert list(sdf.keys()) == [str(k) for k in g["keys"]] and len(sdf) == int(g["n_folded_keys"])
    assert [tuple(v.shape) for v in sdf.values()] == _shapes(g["shapes"])


def test_v2_restatement_matches_the_reference_golden(cfg):
    g = np.load(V2_GOLDEN)
    mel = make_mel(int(g["B"]), int(g["T"]), seed=int(g["seed"]))
    assert torch.equal(mel, torch.from_numpy(g["mel"]))
    sd = {k: v.double() for k, v in v2_folded(int(g["weight_seed"])).items()}
    for name in g.files:
        if name.startswith("fold/"):
            np.testing.assert_allclose(sd[name[5:]].reshape(-1)[:64].numpy(), g[name], rtol=1e-5, atol=1e-7)
    with torch.no_grad():
        wav = generator_any(sd, v2_config(cfg).hifi, mel.double())
    d = float((wav - torch.from_numpy(g["wav"]).double()).abs().max())
    print("V2 restatement (fp64) vs reference golden: max-abs %.3g, rms of the reference %.4f" % (d, float(np.sqrt((g["wav"] ** 2).mean()))))
    assert wav.shape == (2, 1, 8192) and d <= 1e-5


def test_v2_halo_is_v1s(cfg):
    assert windows.receptive_halo(v2_config(cfg).hifi) == windows.receptive_halo(cfg.hifi) == 14


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("k,stride", [(11, 5), (7, 2), (5, 2), (3, 8), (16, 6), (6, 3), (2, 1)])
def test_upsampler_geometry_the_kernels_do_not_compute_is_refused(cfg, k, stride):
    """k % stride != 0 (the low phases would lose their last tap) or k - stride odd (torch's output is one sample longer): refused
    when the generator is built, naming the stage and its (k, stride)."""
    from tts_king_amd.hifigan import Generator
    c = v2_config(cfg)
    c.hifi["upsample_rates"][2], c.hifi["upsample_kernel_sizes"][2] = stride, k
    with pytest.raises(TtskError) as e:
        Generator(c.hifi)
    assert "upsampler 2" in str(e.value) and "kernel size %d" % k in str(e.value) and "stride %d" % stride in str(e.value)


def test_supported_upsampler_geometries_build(cfg):
    from tts_king_amd.hifigan import Generator
    c = v2_config(cfg)
    for k, stride in [(16, 8), (4, 2), (8, 4), (2, 2), (12, 4), (6, 2)]:
        c.hifi["upsample_rates"][1], c.hifi["upsample_kernel_sizes"][1] = stride, k
        Generator(c.hifi)


def test_other_than_three_resblocks_conv_by_conv_is_refused_before_a_launch(cfg):
    """Two MRF kernel sizes: the C = 64 and C = 32 stages have kernels that average any count, the C = 16 / 8 stages run conv by conv,
    whose average takes exactly three — NotImplementedError when the weights are first prepared, before anything is packed or run."""
    from tts_king_amd import ops
    from tts_king_amd.hifigan import Generator
    c = v2_config(cfg)
    c.hifi["resblock_kernel_sizes"], c.hifi["resblock_dilation_sizes"] = [3, 7], [[1, 3, 5], [1, 3, 5]]
    gen = Generator(c.hifi)
    assert gen.stage_routes() == ["pair", "fused", "gemm", "gemm"]
    launched = []
    keep = ops.pack_conv_weight
    ops.pack_conv_weight = lambda *a, **kw: launched.append(a) or keep(*a, **kw)
    try:
        with pytest.raises(NotImplementedError) as e:
            gen._prepare()
    finally:
        ops.pack_conv_weight = keep
    assert "stage 2" in str(e.value) and not launched
    assert Generator(v2_config(cfg).hifi).stage_routes() == ["pair", "fused", "gemm", "gemm"]
    assert Generator(cfg.hifi).stage_routes() == ["pair", "pair", "pair", "fused"]


# ---------------------------------------------------------------------------------------------- negative controls
def _ints(*shape, seed):
    return torch.randint(-3, 4, shape, generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_negative_controls_break_the_integer_kernel_cases(dt):
    """The integer-valued cases of the GPU file compare stored 16-bit tensors for equality: each defect changes them."""
    x, w, b, r = _ints(3, 5, 16, seed=1), _ints(16, 16, 3, seed=2), _ints(16, seed=3), _ints(3, 5, 16, seed=4)
    v, v2 = conv1d_ref(x, w, b, 1, R=r)
    for mut in ("zero_cols", "c2_before_residual"):
        mv, mv2 = conv1d_ref(x, w, b, 1, R=r, mutation=mut)
        same_out, same_c2 = torch.equal(stored(mv, dt), stored(v, dt)), torch.equal(stored(mv2, dt, 0.1), stored(v2, dt, 0.1))
        assert (mut == "zero_cols" and not same_out and not same_c2) or (mut == "c2_before_residual" and same_out and not same_c2)
    for (cin, cout, k, s) in [(32, 16, 4, 2), (16, 8, 4, 2), (64, 32, 16, 8)]:
        xu, wu, bu = _ints(2, 2, cin, seed=5), _ints(cin, cout, k, seed=6), _ints(cout, seed=7)
        good, bad = conv_transpose_ref(xu, wu, bu, s, k), conv_transpose_ref(xu, wu, bu, s, k, mutation="drop_tap")
        rows = (stored(good, dt) != stored(bad, dt)).any(dim=2).any(dim=0).nonzero().view(-1).tolist()
        p = (k - s) // 2
        # tap (k // s - 1) * s of input frame t lands on output row t * s + tap - p: only those rows change, and frame 0's is inside
        assert rows and all((o + p - (k // s - 1) * s) % s == 0 for o in rows) and (k // s - 1) * s - p in rows


def test_negative_controls_exceed_the_whole_generator_bar(cfg):
    g = np.load(V2_GOLDEN)
    sd, h = v2_folded(int(g["weight_seed"])), v2_config(cfg).hifi
    mel = torch.from_numpy(g["mel"])
    cal_r, cal_a, want = calibration(sd, h, mel, torch.float16)
    bar_r, bar_a = max(V1_BAR_F16[0], CAL_FACTOR * cal_r), max(V1_BAR_F16[1], CAL_FACTOR * cal_a)
    print("V2 (2, 32) fp16 calibration: rel-RMS %.4f%% max-abs %.2e -> bars %.3f%% / %.3g" % (100 * cal_r, cal_a, 100 * bar_r, bar_a))
    assert cal_r < V1_BAR_F16[0]                                # storage rounding alone is far inside the bar, or the bar says nothing
    sd64 = {k: v.double() for k, v in sd.items()}
    for mut in ("drop_tap", "zero_cols", "c2_before_residual"):
        with torch.no_grad():
            got = generator_any(sd64, h, mel.double(), mutation=mut)
        r, a = rel_rms(got, want), float((got - want).abs().max())
        print("  %-20s rel-RMS %.2f%% max-abs %.4f" % (mut, 100 * r, a))
        assert r > bar_r, (mut, r, bar_r)
