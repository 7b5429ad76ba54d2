"""What FastSpeech2 launches in a train step, a teacher-forced eval forward and the two inference halves, in which order, with which
integer arguments, and the bits that come out: one recorder for tools/make_goldens_fs2_routes.py and tests/test_fs2_routes_gpu.py,
and the toggle grid of tests/test_fs2_plan_cpu.py.

The parity tests compare values within a tolerance; a layer that moves to another kernel keeps them green.  This recorder sees it.
It uses only what a model has had since before its kernel choices were gathered into one plan -- the constructor, the toggle
attributes, `_forward`, `ops.fs2_loss`, `backward_native`, the `eval()` forward, `eval_front` / `eval_back`, `_w1_packed`,
`_adam_items`, `_repack_after_step` -- and `lib._lib`.

A log entry is [name, stream index, [integer arguments]] (tests/adapt_util.LibProxy).  No pointers: they differ from run to run."""
import hashlib
import itertools
import os

import torch

from tests import fs2_configs as FC
from tests.adapt_util import LibProxy

DEV = "cuda:0"
TOGGLES = ("window_ffn", "flash_attention", "fused_ln", "postnet_ends_win", "dwconv")
PASSES = ("train", "eval", "eval_halves")

# name -> (configuration: "shipped" or a name of tests/fs2_configs.CONFIGS, toggles that differ from the defaults)
CASES = {"shipped": ("shipped", {})}
CASES.update({name: (name, {}) for name in FC.CONFIGS})
CASES.update({
    "no_window_ffn": ("shipped", {"window_ffn": False}),                                   # the only way gemm_ln_fwd runs
    "no_fused_ln": ("shipped", {"fused_ln": False}),
    "no_window_ffn_no_fused_ln": ("shipped", {"window_ffn": False, "fused_ln": False}),
    "no_flash_attention": ("shipped", {"flash_attention": False}),
    "no_postnet_ends_win": ("shipped", {"postnet_ends_win": False}),
    "no_dwconv": ("shipped", {"dwconv": False}),
})


def config(cfg, name):
    import copy
    return copy.deepcopy(cfg) if name == "shipped" else FC.config(cfg, name)


def toggle_grid():
    """Every setting of TOGGLES as a dict (32 of them)."""
    return [dict(zip(TOGGLES, bits)) for bits in itertools.product((True, False), repeat=len(TOGGLES))]


def build_model(c, toggles, device=DEV):
    """A fresh model, weights of seed 7, `toggles` set before its first forward.  `window_ffn` False is also handed to the constructor
    through its environment switch: a model from before the plan kept the packs it had built when the attribute was cleared later,
    so the switch is the one way of building that model on which both trees hold the same packs."""
    from tts_king_amd.fastspeech2 import FastSpeech2
    env = os.environ.get("TTSK_WINDOW_FFN")
    if not toggles.get("window_ffn", True):
        os.environ["TTSK_WINDOW_FFN"] = "0"
    try:
        m = FastSpeech2(c.preprocess_config, c.model_config, FC.N_SPK, device=device, seed=FC.WEIGHT_SEED)
    finally:
        if env is None:
            os.environ.pop("TTSK_WINDOW_FFN", None)
        else:
            os.environ["TTSK_WINDOW_FFN"] = env
    for k, v in toggles.items():
        assert k in TOGGLES and hasattr(m, k), k
        setattr(m, k, v)
    return m


def pack_sizes(m):
    """[[tag, key, elements]] of the model's window-kernel packs, sorted."""
    return sorted([tag, key, int(v.numel())] for (tag, key), v in (m._w1_packed or {}).items())


def _sha(tensors):
    return hashlib.sha256(b"".join(t.detach().contiguous().cpu().numpy().tobytes() for t in tensors)).hexdigest()


def _on_device(b):
    return [t.to(DEV) if torch.is_tensor(t) else t for t in b]


class Recorder:
    """A fresh model per case.  Train batch: tests/fs2_configs.train_batch (B = 3, L = 21 / 9 / 15, T = 75 / 40 / 57: one utterance
    across a 64-frame tile, one inside it, row counts that are no multiple of 32).  Eval batch: the golden one (B = 2, L = 19 / 11,
    T = 66 / 43; short_table: L = 52 / 20, T = 70 / 55, past its 48-entry tables).  The inference halves run the front free and the
    back on the eval batch's own durations, so that the frame count does not hang on a prediction.  Dropout is on; the model's
    dropout counter is never advanced, so every train step of every run draws the same masks."""

    def __init__(self, cfg):
        from tts_king_amd import lib
        lib.load()
        self.cfg = cfg
        # a main stream that is not the default one: its handle is not 0, so no host-only call with a trailing 0 counts as a launch.
        # torch hands out streams from a pool of 32 per priority, round robin: every model takes three of the normal pool for its side
        # streams, and the eleventh model's would be this one again.  So this one comes from the other pool.
        self.main = torch.cuda.Stream(priority=-1)
        torch.cuda.synchronize()

    def _passes(self, m, tb, eb, logs):
        """The three passes on the main stream; `logs`: None, or a dict that receives one launch log per pass.  Returns the five
        output tensors (mel, postnet mel, pitch, energy, log-duration) of each."""
        from tts_king_amd import lib, ops
        real = lib.load()
        outs = {}

        def run(name, fn):
            if logs is not None:
                logs[name] = []
                lib._lib = LibProxy(real, logs[name])
            try:
                with torch.no_grad():
                    outs[name] = fn()
            finally:
                lib._lib = real
            torch.cuda.synchronize()

        def train():
            b, d = tb
            m.train()
            out, ctx = m._forward(True, d[2], d[3], d[4], int(b[5]), d[7], b[8], d[9], d[10], d[11], 1.0, 1.0, 1.0)
            _, dmel_sum, dpost, dp, de, dd = ops.fs2_loss(out[0], out[8], d[6], d[7], out[1], out[2], out[3], d[11], d[9], d[10], d[4], grad_scale=1.0)
            m.backward_native(ctx, dmel_sum, dpost, dp, de, dd, accumulate=False)
            return [out[0], out[8], out[1], out[2], out[3]]

        def teacher_forced():
            m.eval()
            o = m(*eb[1][2:])
            return [o[0], o[9], o[1], o[2], o[3]]

        def halves():
            b, d = eb
            m.eval()
            x3, _, _, pred = m.eval_front(d[2], d[3], d[4], int(b[5]))
            mel, post = m.eval_back(x3, d[10], int(b[5]), int(b[8]))[:2]
            return [mel, post, pred[0], pred[1], pred[2]]

        with torch.cuda.stream(self.main):
            run("train", train)
            outs["grad"] = m.flat_buffers()[1].clone()
            run("eval", teacher_forced)
            run("eval_halves", halves)
            torch.cuda.synchronize()
        return outs

    def record(self, name, model=None):
        """{"launches": {pass: log}, "sha256": {pass: digest, "grad": digest}, "packs", "adam_items", "repack_after_step"} of case
        `name`: every pass once unrecorded (the bf16 shadow, the packs, the side streams and the split-K plans of a first step are not
        part of a step), then once under the proxy.  `model`: record this model instead of a fresh one."""
        cname, toggles = CASES[name]
        c = config(self.cfg, cname)
        m = build_model(c, toggles) if model is None else model
        tb, eb = FC.train_batch(c), FC.golden_batch(c, cname)
        tb, eb = (tb, _on_device(tb)), (eb, _on_device(eb))
        self._passes(m, tb, eb, None)
        logs = {}
        outs = self._passes(m, tb, eb, logs)
        sha = {p: _sha(outs[p]) for p in PASSES}
        sha["grad"] = _sha([outs["grad"]])
        return {"launches": logs, "sha256": sha, "packs": pack_sizes(m),
                "adam_items": None if m._adam_items is None else len(m._adam_items), "repack_after_step": bool(m._repack_after_step)}
