"""What the FastSpeech2 backward launches, on which stream, in which order: one recorder for tools/make_goldens_dw_schedule.py and
tests/test_dw_schedule_gpu.py.

The deferred weight-gradient work (grouped dW GEMMs, the dwconv / dwgemm problems, their split-K reducers, the column sums) goes out
late, on up to three streams, with gradient buckets announced in between in the data-parallel schedules.  The gradient tests cannot
see a launch that moved to another stream or behind a bucket's announcement; this recorder can.  It uses only `lib._lib`,
`FastSpeech2._forward`, `backward_native`, `ops.fs2_loss`, `parallel.GradReducer` and the model's public toggles.

A log entry is [name, stream] (+ [n] for a *_batch entry point, + [max_wgs] where the call takes one) or ["bucket", start, end, stream];
`stream` is the index of the stream in order of first appearance in that log.  No pointers: they differ from run to run."""
import copy
import ctypes as C
import hashlib

import torch

DEV = "cuda:0"
BUCKET_MB = 24
WITH_MAX_WGS = {"ttsk_gemm_group_launch_capped": 2, "ttsk_gemm_group_launch_uploaded": 2, "ttsk_dwgemm_batch": 2}     # name -> argument index

# name -> (model attributes that differ from the defaults, a gradient reducer is listening)
CONFIGS = {
    "default": ({}, False),
    "no_side_stream": ({"dw_side_wgs": 0}, False),
    "no_dwconv": ({"dwconv": False}, False),
    "sequential_predictors": ({"group_predictors": False}, False),     # reaches conv1d_dw(defer=...)
    "dp_side": ({"dp_schedule": "side"}, True),
    "dp_late": ({"dp_schedule": "late"}, True),
    "dp_no_side_stream": ({"dw_side_wgs": 0}, True),                   # a flush per completed bucket (_GroupNotifier.ready)
}
TOGGLES = ("dw_side_wgs", "dw_side_frac", "dwconv", "group_predictors", "dp_schedule")


def _handle(x):
    return x.value if isinstance(x, C.c_void_p) else x


class _LibProxy:
    """Stands in for the loaded library: every call whose last argument is the current torch stream's handle (include/ttsk.h: an
    entry point that takes a stream takes it last) is logged, then forwarded."""

    def __init__(self, real, rec):
        self.__dict__["_real"], self.__dict__["_rec"] = real, rec

    def __setattr__(self, name, value):
        setattr(self._real, name, value)

    def __getattr__(self, name):
        fn, rec = getattr(self._real, name), self._rec

        def forward(*args):
            cur = torch.cuda.current_stream().cuda_stream
            last = _handle(args[-1]) if args else None
            if type(last) is int and last == cur:
                entry = [name, rec.stream_index(cur)]
                if name.endswith("_batch"):
                    entry.append(next(a for a in args[:-1] if type(a) is int))       # the item count: the first plain integer
                if name in WITH_MAX_WGS:
                    entry.append(int(args[WITH_MAX_WGS[name]]))
                rec.log.append(entry)
            return fn(*args)
        return forward


class Recorder:
    """One model (weights of seed 7), one ragged batch (5 utterances of 24-48 phonemes: the shape of test_dwconv_path_equals_grouped_gemm_path, small, and its
    decoder-side dwgemm problems still split: 21 reduce items go through the batched reducer), any number of configurations."""

    def __init__(self, cfg):
        from tests.oracle_util import fs2_state_dict
        from tts_king_amd import lib
        from tts_king_amd.fastspeech2 import FastSpeech2
        from tts_king_amd.synthetic import make_batch
        c = copy.deepcopy(cfg)
        lib.load()
        self.model = FastSpeech2(c.preprocess_config, c.model_config, 65, device=DEV).train()
        self.model.load_state_dict(fs2_state_dict(c, 7))
        self.defaults = {k: getattr(self.model, k) for k in TOGGLES}
        self.batch = make_batch(5, 48, seed=33, ragged=True)
        self.dev_b = [t.to(DEV) if torch.is_tensor(t) else t for t in self.batch]
        # a main stream that is not the default one: its handle is not 0, so no host-only call with a trailing 0 counts as a launch
        self.main = torch.cuda.Stream()
        self.log, self._streams = [], {}
        torch.cuda.synchronize()
        # one step that is not recorded: what a model does once (the bf16 shadow and the weight packs after load_state_dict, its
        # dropout state block, its side streams) is not part of a step's schedule
        with torch.cuda.stream(self.main):
            self._step(None)
        torch.cuda.synchronize()

    def stream_index(self, handle):
        return self._streams.setdefault(handle, len(self._streams))

    def _reducer(self):
        from tts_king_amd.parallel import GradReducer
        rec, m = self, self.model

        class LoggingReducer(GradReducer):
            def _launch_down_to(self, watermark):
                sidx = rec.stream_index(torch.cuda.current_stream().cuda_stream)
                i = self._next
                while i < len(self.buckets) and self.buckets[i][0] >= watermark:
                    rec.log.append(["bucket", int(self.buckets[i][0]), int(self.buckets[i][1]), sidx])
                    i += 1
                super()._launch_down_to(watermark)
        # no process group: world size 1, no collective
        return LoggingReducer(m.flat_buffers()[1], m.grad_buckets(BUCKET_MB), m.group_offsets())

    def _step(self, red):
        from tts_king_amd import ops
        m, b, d = self.model, self.batch, self.dev_b
        with torch.no_grad():
            out, ctx = m._forward(True, d[2], d[3], d[4], int(b[5]), d[7], b[8], d[9], d[10], d[11], 1.0, 1.0, 1.0)
            _, dmel_sum, dpost, dp, de, dd = ops.fs2_loss(out[0], out[8], d[6], d[7], out[1], out[2], out[3], d[11], d[9], d[10], d[4], grad_scale=1.0)
            m.backward_native(ctx, dmel_sum, dpost, dp, de, dd, on_bucket=None if red is None else red.on_group_done, accumulate=False)
        if red is not None:
            red.finish()

    def record(self, name):
        """{"launches", "counts", "trace", "grad_sha256"} of configuration `name`: one step under the proxy with ops.LAUNCH_COUNTS, a
        second one with ops.GEMM_TRACE (so that the event records of the trace do not enter the launch log)."""
        from tts_king_amd import lib, ops
        attrs, dp = CONFIGS[name]
        m = self.model
        for k, v in self.defaults.items():
            setattr(m, k, v)
        for k, v in attrs.items():
            setattr(m, k, v)
        self.log, self._streams = [], {}
        counts, trace = {}, []
        real = lib.load()
        try:
            with torch.cuda.stream(self.main):
                lib._lib = _LibProxy(real, self)
                ops.LAUNCH_COUNTS = counts
                try:
                    self._step(self._reducer() if dp else None)
                finally:
                    lib._lib = real
                    ops.LAUNCH_COUNTS = None
                torch.cuda.synchronize()
                launches, self.log = self.log, []          # (the second step's bucket announcements are not recorded)
                digest = hashlib.sha256(m.flat_buffers()[1].cpu().numpy().tobytes()).hexdigest()
                ops.GEMM_TRACE = trace
                try:
                    self._step(self._reducer() if dp else None)
                finally:
                    ops.GEMM_TRACE = None
                torch.cuda.synchronize()
        finally:
            for k, v in self.defaults.items():
                setattr(m, k, v)
        return {"launches": launches, "counts": dict(sorted(counts.items())),
                "trace": [[t[3], [x if isinstance(x, str) else int(x) for x in t[4]]] for t in trace], "grad_sha256": digest}
