"""The FastSpeech2 configurations, other than the shipped one, that the suite builds a model for (tests/test_fs2_configs_cpu.py,
tests/test_fs2_configs_gpu.py, tools/make_goldens.py: g14_fs2_configs), and the configurations the constructor refuses.

Every entry of CONFIGS is a delta over the shipped `model_config` / `preprocess_config` chosen to select routes of the kernel plan
(tts_king_amd/fs2_plan.py: build_plan) that the shipped configuration (hidden 256, 2 heads, conv_filter_size 1024, conv_kernel_size
[9, 1], predictor filter 256 / kernel 3, 80 mels, max_seq_len 1000) never takes.  `selects` says which; tests/test_fs2_plan_cpu.py
checks that the plan names them, tests/test_fs2_configs_gpu.py that the launches say the same.  Shapes are the smallest that still reach each branch."""
import copy
import json
import os

import torch

from oracle import fs2 as ofs2
from tts_king_amd.synthetic import seeded_fill

N_SPK = 65
WEIGHT_SEED = 7

# name -> (model_config delta, n_mel_channels or None, the branch the entry selects)
CONFIGS = {
    "heads_1_4": ({"transformer": {"encoder_head": 1, "decoder_head": 4}}, None,
                  "head sizes 256 (encoder) and 64 (decoder): scores GEMM + softmax_fwd / softmax_bwd + P V GEMM, no flash attention"),
    "d512": ({"transformer": {"encoder_hidden": 512, "decoder_hidden": 512, "variance_hidden": 512, "encoder_head": 4, "decoder_head": 4}}, None,
             "hidden 512: flash attention with 4 heads; ops.linear + layernorm_fwd instead of the fused projection + LayerNorm; the "
             "window kernel's 512-channel instances for q|k|v, w_1, fc / w_2 input gradients; gather / scatter / va_embed / length "
             "regulator at D = 512; dwconv at Cin = 512, dwgemm at 512 / 1024 / 1536 channels"),
    "ffn_k3": ({"transformer": {"conv_kernel_size": [3, 3], "conv_filter_size": 512}}, None,
               "k2 != 1: w_2 on ops.conv1d + layernorm_fwd, its input gradient on conv1d_dx, the whole block backward unfused; w_1 at "
               "k = 3 and 512 outputs (no dwconv instance: conv1d_dw); Adam's tile walk over these shapes"),
    # (no predictor kernel size other than 3 here: the reference's predictor pads its second conv by 1 whatever the kernel size
    # (model/modules.py:290), so it runs with kernel_size 3 only -- every other size is refused by name, see REFUSED)
    "pred512": ({"variance_predictor": {"filter_size": 512}, "variance_embedding": {"n_bins": 64}}, None,
                "predictor convs and LayerNorms at 512 channels; the grouped predictors' parameter stride; bucketize and the "
                "embedding tables at 64 bins"),
    "mel40_layers_1_2": ({"transformer": {"encoder_layer": 1, "decoder_layer": 2}}, 40,
                         "40 mels: mel_linear 256 -> 40 and the PostNet's ends 40 <-> 512 on the implicit GEMM (no window instance), "
                         "BatchNorm and the loss at 40 channels; a one-block encoder (no next block to chain q|k|v into) and a two-block decoder"),
    "short_table": ({"max_seq_len": 48}, None,
                    "max_seq_len 48: the train-mode decoder cut and the eval-mode recomputed position tables at tiny shapes"),
}

# the training batch of every configuration: B = 3 ragged, one utterance across a 64-frame tile (75), one inside it (40); with
# max_seq_len 48 two of the three are cut
TRAIN_SRC, TRAIN_MEL, TRAIN_SPK = [21, 9, 15], [75, 40, 57], [3, 17, 40]
# the reference-recorded eval batch (B = 2); short_table's has a text and frame counts above max_seq_len 48
GOLDEN_SRC, GOLDEN_MEL, GOLDEN_SPK = [19, 11], [66, 43], [5, 31]
GOLDEN_SRC_SHORT, GOLDEN_MEL_SHORT = [52, 20], [70, 55]


def _merge(dst, delta):
    for k, v in delta.items():
        if isinstance(v, dict):
            _merge(dst[k], v)
        else:
            dst[k] = copy.deepcopy(v)


def apply_delta(cfg, delta, n_mel=None):
    """A deep copy of `cfg` (anything with model_config / preprocess_config mappings) with the delta applied."""
    c = copy.deepcopy(cfg)
    _merge(c["model_config"], delta)
    if n_mel is not None:
        c["preprocess_config"]["preprocessing"]["mel"]["n_mel_channels"] = n_mel
    return c


def config(cfg, name):
    delta, n_mel, _ = CONFIGS[name]
    return apply_delta(cfg, delta, n_mel)


def n_mel_of(c):
    return c["preprocess_config"]["preprocessing"]["mel"]["n_mel_channels"]


def batch(src_lens, mel_lens, speakers, n_mel, seed):
    """tests.test_step_shapes_gpu.exact_batch's 15-tuple with these speakers and `n_mel` mel channels."""
    from tests.test_step_shapes_gpu import exact_batch
    b = list(exact_batch(src_lens, mel_lens, seed))
    g = torch.Generator().manual_seed(seed + 1)
    B, T = len(src_lens), max(mel_lens)
    mels = torch.randn(B, T, n_mel, generator=g)
    mels[torch.arange(T)[None, :] >= b[7][:, None]] = 0
    b[6] = mels
    b[2] = torch.tensor(speakers, dtype=torch.int64)
    return tuple(b)


def train_batch(c):
    return batch(TRAIN_SRC, TRAIN_MEL, TRAIN_SPK, n_mel_of(c), seed=301)


def golden_batch(c, name):
    src, mel = (GOLDEN_SRC_SHORT, GOLDEN_MEL_SHORT) if name == "short_table" else (GOLDEN_SRC, GOLDEN_MEL)
    return batch(src, mel, GOLDEN_SPK, n_mel_of(c), seed=302)


def state_dict_from_spec(c, keys, shapes, dtypes, weight_seed=WEIGHT_SEED):
    """tests.oracle_util.fs2_state_dict for a recorded key / shape list: zeros of the reference's shapes, the position tables and
    bin edges as the reference builds them, everything else from seeded_fill."""
    sd = {}
    for k, s, dt in zip(keys, shapes, dtypes):
        shape = tuple(int(x) for x in str(s).split(";")) if str(s) else ()
        sd[str(k)] = torch.zeros(shape, dtype=torch.int64 if "int64" in str(dt) else torch.float32)
    mc = c["model_config"]
    tab = ofs2.sinusoid_table(mc["max_seq_len"] + 1, mc["transformer"]["encoder_hidden"])[None]
    sd["encoder.position_enc"], sd["decoder.position_enc"] = tab.clone(), tab.clone()
    with open(os.path.join(c["preprocess_config"]["path"]["preprocessed_path"], "stats.json")) as f:
        stats = json.load(f)
    nb = mc["variance_embedding"]["n_bins"]
    sd["variance_adaptor.pitch_bins"] = torch.linspace(stats["pitch"][0], stats["pitch"][1], nb - 1)
    sd["variance_adaptor.energy_bins"] = torch.linspace(stats["energy"][0], stats["energy"][1], nb - 1)
    seeded_fill(sd, weight_seed)
    return sd


# ---------------------------------------------------------------------------------------------------- refusals
# name -> (model_config delta, n_mel_channels or None, the key the exception must name).  Each limit is a TTSK_REQUIRE or a
# `*_supported` of the entry point the shape would reach (tts_king_amd/params.py: validate_config cites them).
REFUSED = {
    "pred_filter_384": ({"variance_predictor": {"filter_size": 384}}, None, "variance_predictor.filter_size"),
    "pred_filter_1280": ({"variance_predictor": {"filter_size": 1280}}, None, "variance_predictor.filter_size"),
    "hidden_384": ({"transformer": {"encoder_hidden": 384, "decoder_hidden": 384, "variance_hidden": 384}}, None, "transformer.encoder_hidden"),
    "hidden_1280": ({"transformer": {"encoder_hidden": 1280, "decoder_hidden": 1280, "variance_hidden": 1280}}, None, "transformer.encoder_hidden"),
    # (the LayerNorm kernels take 768 and 1024, but the q|k|v input gradient would need 9 / 12 slabs of ttsk_win_conv_split: at most 8)
    "hidden_768": ({"transformer": {"encoder_hidden": 768, "decoder_hidden": 768, "variance_hidden": 768, "encoder_head": 6, "decoder_head": 6}}, None,
                   "transformer.encoder_hidden"),
    "hidden_1024": ({"transformer": {"encoder_hidden": 1024, "decoder_hidden": 1024, "variance_hidden": 1024, "encoder_head": 8, "decoder_head": 8}}, None,
                    "transformer.encoder_hidden"),
    "decoder_hidden_differs": ({"transformer": {"decoder_hidden": 512}}, None, "transformer.decoder_hidden"),
    "variance_hidden_differs": ({"transformer": {"variance_hidden": 512}}, None, "transformer.variance_hidden"),
    "heads_3": ({"transformer": {"encoder_head": 3}}, None, "transformer.encoder_head"),
    "heads_64": ({"transformer": {"decoder_head": 64}}, None, "transformer.decoder_head"),          # head size 4: not a multiple of 8
    "mel_42": ({}, 42, "preprocessing.mel.n_mel_channels"),
    "mel_4": ({}, 4, "preprocessing.mel.n_mel_channels"),
    "mel_1032": ({}, 1032, "preprocessing.mel.n_mel_channels"),
    "ffn_kernel_even": ({"transformer": {"conv_kernel_size": [8, 1]}}, None, "transformer.conv_kernel_size"),
    "ffn_kernel_2_even": ({"transformer": {"conv_kernel_size": [9, 2]}}, None, "transformer.conv_kernel_size"),
    "ffn_kernel_17": ({"transformer": {"conv_kernel_size": [17, 1]}}, None, "transformer.conv_kernel_size"),
    "pred_kernel_even": ({"variance_predictor": {"kernel_size": 4}}, None, "variance_predictor.kernel_size"),
    "pred_kernel_5": ({"variance_predictor": {"kernel_size": 5}}, None, "variance_predictor.kernel_size"),
    "ffn_filter_2048": ({"transformer": {"conv_filter_size": 2048}}, None, "transformer.conv_filter_size"),
    "ffn_filter_1020": ({"transformer": {"conv_filter_size": 1020}}, None, "transformer.conv_filter_size"),
    "n_bins_1": ({"variance_embedding": {"n_bins": 1}}, None, "variance_embedding.n_bins"),
    "no_layers": ({"transformer": {"decoder_layer": 0}}, None, "transformer.decoder_layer"),
    "cwt_hidden_512": ({"use_cwt": True, "transformer": {"encoder_hidden": 512, "decoder_hidden": 512, "variance_hidden": 512,
                                                         "encoder_head": 4, "decoder_head": 4}}, None, "transformer.encoder_hidden"),
    "cwt_pred_filter_512": ({"use_cwt": True, "variance_predictor": {"filter_size": 512}}, None, "variance_predictor.filter_size"),
}
