"""What a HiFi-GAN generator forward launches, in which order, with which integer and float arguments: one recorder for
tools/make_goldens_hifi_routes.py and tests/test_hifi_routes_gpu.py, and the toggle grid of tests/test_hifi_plan_cpu.py.

The waveform tests compare values within a tolerance; a stage that moves to another kernel family, an upsampler that changes kernels or
an MRF mode that changes keeps them green.  This recorder sees it.  It uses only the generator's public surface — `Generator(h)`, the
toggle attributes, `gen(mel)`, `gen.forward_ntc(a0, row_frames=...)`, `stage_routes()`, `short_rows()` — and `lib._lib`.

A log entry is [name, stream index, [integer and float arguments]] (tests/adapt_util.LibProxy).  No pointers: they differ from run to run."""
import copy
import hashlib
import itertools

import torch

from tests.adapt_util import LibProxy
from tests.hifi_generic_ref import v2_config, v2_state_dict_wn
from tests.oracle_util import hifi_state_dict_wn
from tests.test_hifigan_v3_gpu import v3_config, v3_state_dict_wn
from tts_king_amd.synthetic import make_mel

DEV = "cuda:0"
ROW_FRAMES = [0, 17]                  # row 0 whole, row 1 an utterance of 17 frames
BF16 = {"act_dtype": torch.bfloat16}

# name -> (configuration, attributes that differ from the defaults, through forward_ntc with ROW_FRAMES)
CASES = {
    "v1": ("v1", {}, False),
    "v1_no_fused": ("v1", {"fused": False}, False),
    "v1_no_pairs": ("v1", {"conv_pair": False, "conv_pair_small": False}, False),
    "v1_no_conv_pair": ("v1", {"conv_pair": False}, False),
    "v1_no_window_conv": ("v1", {"window_conv": False}, False),
    "v1_no_stream_upsample": ("v1", {"stream_upsample": False}, False),
    "v1_no_loop_upsample": ("v1", {"loop_upsample": False}, False),
    "v1_no_window_upsample": ("v1", {"window_upsample": False}, False),
    "v1_no_mrf_fused": ("v1", {"mrf_fused": False}, False),
    "v1_ws_from_one_tile": ("v1", {"pair_ws_min_tiles": 1}, False),
    "v1_no_pair_ws_from_one_tile": ("v1", {"pair_ws": False, "pair_ws_min_tiles": 1}, False),
    "v1_bf16": ("v1", BF16, False),
    "v2": ("v2", {}, False),
    "v2_no_fused": ("v2", {"fused": False}, False),
    "v3": ("v3", {}, False),
    "v3_no_resblock2_fused": ("v3", {"resblock2_fused": False}, False),
    "v1_rows": ("v1", {}, True),
    "v3_rows": ("v3", {}, True),
    # refused: a stage conv by conv takes no row length (tests/test_short_rows_gpu.py::test_fallback_keeps_the_solo_route)
    "v1_no_fused_rows": ("v1", {"fused": False}, True),
    "v1_no_conv_pair_rows": ("v1", {"conv_pair": False}, True),
    "v2_rows": ("v2", {}, True),
}
GRID = ("resblock2_fused", "conv_pair", "window_conv", "conv_pair_small", "fused")        # the toggles `stage_routes()` depends on


def configs(cfg):
    """name -> (hifi configuration, weight-normed state dict maker)."""
    return {"v1": (cfg.hifi, lambda: hifi_state_dict_wn(5)), "v2": (v2_config(cfg).hifi, lambda: v2_state_dict_wn(7)),
            "v3": (v3_config(cfg).hifi, lambda: v3_state_dict_wn(11))}


def route_table(cfg):
    """{configuration: {"01101": stage_routes()}} over the 32 settings of GRID (a bit per toggle, in GRID's order), on generators without
    weights on any device: needs the built library's host predicates only."""
    from tts_king_amd.hifigan import Generator
    table = {}
    for name, (h, _) in configs(cfg).items():
        gen = Generator(copy.deepcopy(h))
        table[name] = {}
        for bits in itertools.product((False, True), repeat=len(GRID)):
            for k, v in zip(GRID, bits):
                setattr(gen, k, v)
            table[name]["".join("01"[b] for b in bits)] = gen.stage_routes()
    return table


class Recorder:
    """A fresh generator per case (seeded weights, the case's attributes set before its first forward, so that no case depends on what an
    earlier one left packed), one mel (2 utterances of 40 frames: stage lengths 320 / 2560 / 5120 / 10240 cross the 96- and 192-frame
    tiles)."""

    def __init__(self, cfg):
        from tts_king_amd import lib
        lib.load()
        self.configs = configs(cfg)
        self.mel = make_mel(2, 40, seed=9).to(DEV)
        # a main stream that is not the default one: its handle is not 0, so no host-only call with a trailing 0 counts as a launch
        self.main = torch.cuda.Stream()
        torch.cuda.synchronize()

    def gen(self, config, attrs=None):
        from tts_king_amd.hifigan import Generator
        h, state = self.configs[config]
        g = Generator(copy.deepcopy(h))
        g.load_state_dict(state())
        g.to(DEV)
        g.remove_weight_norm()
        for k, v in (attrs or {}).items():
            assert hasattr(g, k), k
            setattr(g, k, v)
        return g.eval()

    def forward(self, gen, rows=False, log=None):
        """One forward on the main stream, its launches appended to `log`."""
        from tts_king_amd import lib, ops
        real = lib.load()
        with torch.cuda.stream(self.main):
            if log is not None:
                lib._lib = LibProxy(real, log, floats=True)
            try:
                if not rows:
                    y = gen(self.mel)
                else:
                    a0 = ops.nct_to_ntc(self.mel.float(), gen.act_dtype)
                    frames = torch.tensor(ROW_FRAMES, dtype=torch.int32, device=DEV)
                    ops.zero_rows_past(a0, (frames, 1))
                    y = gen.forward_ntc(a0, row_frames=frames)
            finally:
                lib._lib = real
            torch.cuda.synchronize()
        return y

    def record(self, name):
        """{"routes", "short_rows"} and {"launches", "wav_sha256"} or {"raises"} of case `name`: one forward that is not recorded (the weight
        packs, the split-K plans: packing is not part of a forward), then one under the proxy."""
        config, attrs, rows = CASES[name]
        from tts_king_amd.lib import TtskError
        gen = self.gen(config, attrs)
        out = {"routes": gen.stage_routes(), "short_rows": bool(gen.short_rows())}
        try:
            self.forward(gen, rows)
        except (TtskError, NotImplementedError) as e:          # a refusal: its type is the record
            torch.cuda.synchronize()
            out["raises"] = type(e).__name__
            return out
        log = []
        y = self.forward(gen, rows, log)
        spf = y.shape[-1] // self.mel.shape[-1]
        # what lies past a row's end is unspecified: the digest covers each row's own samples
        kept = [y[b, :, :(f or self.mel.shape[-1]) * spf] for b, f in enumerate(ROW_FRAMES)] if rows else [y]
        out["launches"] = log
        out["wav_sha256"] = hashlib.sha256(b"".join(t.contiguous().cpu().numpy().tobytes() for t in kept)).hexdigest()
        return out
