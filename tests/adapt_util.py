"""Helpers of tests/test_adapt_gpu.py (speaker adaptation: trained units beside frozen ones): one training step recorded through a
stand-in for the loaded library, and the oracle trainer restricted to the same units."""
import ctypes as C

import torch

DEV = "cuda:0"


def _handle(x):
    return x.value if isinstance(x, C.c_void_p) else x


class LibProxy:
    """Stands in for the loaded library (`lib._lib`): every call whose last argument is the current torch stream's handle (an entry
    point of include/ttsk.h that takes a stream takes it last) is logged as [name, stream index, integer arguments below 2^31], then
    forwarded.  No pointers in the log (tensor addresses arrive as plain integers too, far above that): they differ from run to run.
    `floats`: plain float arguments (slopes, scales) are logged too, in place among the integers."""

    def __init__(self, real, log, floats=False):
        self.__dict__["_real"], self.__dict__["_log"], self.__dict__["_streams"] = real, log, {}
        self.__dict__["_floats"] = floats

    def __setattr__(self, name, value):
        setattr(self._real, name, value)

    def __getattr__(self, name):
        fn, log, streams, floats = getattr(self._real, name), self._log, self._streams, self._floats

        def forward(*args):
            cur = torch.cuda.current_stream().cuda_stream
            last = _handle(args[-1]) if args else None
            if type(last) is int and last == cur:
                log.append([name, streams.setdefault(cur, len(streams)),
                            [a for a in args[:-1] if (type(a) is int and abs(a) < (1 << 31)) or (floats and type(a) is float)]])
            return fn(*args)
        return forward


def step_log(m, batch, dev_batch):
    """The launches of one forward + loss + backward_native of `m` on `batch` (after one step that is not recorded: the shadow, the
    packs, the side streams and the split-K plans of a first step are not part of a step's schedule), on a stream of its own so that
    no host-only call with a trailing 0 counts as a launch."""
    from tts_king_amd import lib, ops

    def step():
        b, d = batch, dev_batch
        with torch.no_grad():
            out, ctx = m._forward(True, d[2], d[3], d[4], int(b[5]), d[7], b[8], d[9], d[10], d[11], 1.0, 1.0, 1.0)
            _, dmel_sum, dpost, dp, de, dd = ops.fs2_loss(out[0], out[8], d[6], d[7], out[1], out[2], out[3], d[11], d[9], d[10], d[4], grad_scale=1.0)
            m.backward_native(ctx, dmel_sum, dpost, dp, de, dd, accumulate=False)

    main = torch.cuda.Stream()
    torch.cuda.synchronize()
    log = []
    real = lib.load()
    with torch.cuda.stream(main):
        step()
        torch.cuda.synchronize()
        lib._lib = LibProxy(real, log)
        try:
            step()
        finally:
            lib._lib = real
        torch.cuda.synchronize()
    return log


def restrict_oracle(tr, units):
    """An OracleTrainer that trains `units` only: its clip and Adam walk `tr.keys` and skip parameters without gradients."""
    from tts_king_amd import params as P
    keep = [k for k in tr.keys if P.unit_of(k) in units]
    for k in tr.keys:
        if k not in keep:
            tr.sd[k].requires_grad_(False)
    tr.keys = keep
    return tr
