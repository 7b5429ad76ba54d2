"""Thin torch-tensor -> C-ABI adapters (plumbing only: device pointers, strides, the current HIP stream).

Every function here enqueues hand-written gfx950 kernels from libttsk_hip.so on torch's current stream and
returns immediately; nothing is computed by PyTorch.  Tensors must live on a HIP device ("cuda:N" in
PyTorch-ROCm naming) — CPU tensors are rejected, there is no fallback.
"""
import ctypes as C

import threading

import torch

from . import lib as L
from .lib import (A_TR, B_TR, C_F32, RELU, ADD_R, R_F32, MASK_G, LRELU_IN, TANH, ACCUM_C, LRELU_OUT, F16, C2_LRELU, DEFER_REDUCE, RAW_SLABS,  # noqa: F401
                  GemmDesc, check)

bf16 = torch.bfloat16
f16 = torch.float16


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.TtskError("tts_king_amd kernels need HIP device tensors (got %s); there is no CPU path" % t.device)


def _ptr(t):
    return None if t is None else t.data_ptr()


import os as _os
# K steps one workgroup of a grouped weight-gradient launch walks (128x128 tile, 256x128 tile): more steps = fewer split-K slabs
DW_STEPS_PER_WG = (28, 72)
LAUNCH_COUNTS = None   # bench.py sets this to a dict: grouped-GEMM / batched-reducer / column-sum launches issued by the flushes
STAMPS = None       # tools/debug/step_stamps.py (diagnostic library only): (uint64 device buffer, [names]) — `stamp(name)` then launches a
                    # one-thread kernel that writes the device's 100 MHz clock into the next slot, on the current stream
GEMM_TRACE = None   # bench.py sets this to a list: every ttsk_gemm launch is then bracketed by HIP events on its stream
                    # (and, through `_family`, every launch of the other MFMA kernel families and of the step's HBM-bound passes)


def _traced(launch, describe):
    """launch(), and when GEMM_TRACE is set, between two HIP events on the current stream: (e0, e1, *describe()) joins the trace,
    describe() -> (algorithmic FLOPs, kind, shape).  The one place that brackets a launch; no cost beyond two closures otherwise."""
    if GEMM_TRACE is None:
        return launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = launch()
    e1.record()
    GEMM_TRACE.append((e0, e1) + tuple(describe()))
    return out


def _count(key):
    if LAUNCH_COUNTS is not None:
        LAUNCH_COUNTS[key] = LAUNCH_COUNTS.get(key, 0) + 1


def _family(kind, flops):
    """Decorator: when GEMM_TRACE is set, bracket the wrapped launch with HIP events on its stream and record (events, algorithmic
    FLOPs = flops(*args, **kwargs), family name) — bench.py's per-family roofline (`roofline.families`).  No cost otherwise."""
    def deco(fn):
        import functools

        @functools.wraps(fn)
        def wrapped(*a, **kw):
            return _traced(lambda: fn(*a, **kw),
                           lambda: (float(flops(*a, **kw)), kind, (0, 0, 0, 1, 1, 0, fn.__name__)))      # (last: the wrapper, for bench.py's per-instance rows)
        return wrapped
    return deco


def _conv_flops(x, packed, Cout, k, *a, **kw):
    return 2.0 * x.shape[0] * x.shape[1] * x.shape[2] * Cout * k


def stamp(name):
    """Diagnostic (a no-op unless ops.STAMPS is set, which needs libttsk_hip_stamps.so): mark this point of the current stream."""
    if STAMPS is None:
        return
    buf, names = STAMPS
    i = len(names)
    if i >= buf.numel():
        return
    names.append(name)
    fn = L.load().ttsk_debug_stamp
    fn.argtypes = [C.c_void_p, C.c_void_p]
    fn(C.c_void_p(buf.data_ptr() + 8 * i), C.c_void_p(_stream()))


class Slabs:
    """Raw split-K partial tiles of a GEMM (gemm(raw=True)): fp32 [splits][M*N] in `ws`."""

    def __init__(self, ws, splits, stride):
        self.ws, self.splits, self.stride = ws, splits, stride


class GemmGroup:
    """Independent GEMMs (same operand layout per launch) that run as one grouped launch: `gemm(..., group=g)` ... `g.flush()`.
    Problems are launched per (operand layout, tile configuration): at most a handful of grids."""

    def __init__(self):
        self.descs, self.keep = [], []

    def flush(self):
        flush_group(self.descs, self.keep)
        self.keep = []


def _group_tables(descs, keep):
    """The queued descriptors as grouped-launch tables, one per (operand layout, tile configuration): yields (host table, device
    table, FLOPs, trace kind, trace shape).  `keep` holds the descriptors' tensors and receives the device tables."""
    if not descs:
        return
    lib = L.load()
    by_layout = {}
    for d in descs:
        by_layout.setdefault((d.flags & (A_TR | B_TR | F16), d.kernel), []).append(d)
    dev = keep[0].device
    for ds in by_layout.values():
        # longest workgroups first: a grouped grid is dispatched in workgroup order and its problems differ several-fold in K steps
        # per workgroup (HiFi-GAN's k = 11 / 7 / 3 convs, a decoder vs an encoder weight gradient), so the short ones should fill the
        # tail of the launch instead of opening it.  The problems are independent: their order changes no result.
        ds.sort(key=lambda d: -(d.K * max(d.taps, 1)) // max(d.splits, 1))
        n = len(ds)
        nbytes = int(lib.ttsk_gemm_group_table_bytes(n))
        host = (C.c_ubyte * nbytes)()
        arr = (GemmDesc * n)(*ds)
        total = C.c_int32(0)
        check(lib.ttsk_gemm_group_build(arr, n, host, C.byref(total)), "ttsk_gemm_group_build")
        table = torch.empty(nbytes, dtype=torch.uint8, device=dev)      # filled by group_launch through kernel arguments
        keep.append(table)
        fl = sum(2.0 * d.M * d.N * d.K * max(d.taps, 1) * d.nz1 * d.nz2 for d in ds)
        kind = ("TT" if ds[0].flags & A_TR else ("NT_btr" if ds[0].flags & B_TR else "NT")) + "%dg" % ds[0].kernel
        _count("grouped_gemm")
        yield host, table, fl, kind, (n, 0, 0, 1, 1, int(total.value))
    descs.clear()


def flush_group(descs, keep, max_wgs=0):
    """Grouped launches (ttsk_gemm_group_*) of the queued descriptors on the current stream, one per operand layout; `keep` holds
    their tensors.  max_wgs > 0 caps the grid of the 256x128 configuration (ttsk_gemm_group_launch_capped)."""
    lib = L.load()
    for host, table, fl, kind, shape in _group_tables(descs, keep):
        _traced(lambda: check(lib.ttsk_gemm_group_launch_capped(host, C.c_void_p(table.data_ptr()), int(max_wgs), _stream()), "ttsk_gemm_group_launch"),
                lambda: (fl, kind, shape))


def upload_group(descs, keep):
    """flush_group in two parts: only the tables go to the device now (current stream); returns a function that issues the
    launches (uncapped) on the stream current when it is called, which the caller has ordered behind this one."""
    lib = L.load()
    pending = []
    for host, table, fl, kind, shape in _group_tables(descs, keep):
        check(lib.ttsk_gemm_group_upload(host, C.c_void_p(table.data_ptr()), _stream()), "ttsk_gemm_group_upload")
        pending.append((host, table, fl, kind, shape))

    def launch():
        for host, table, fl, kind, shape in pending:
            _traced(lambda: check(lib.ttsk_gemm_group_launch_uploaded(host, C.c_void_p(table.data_ptr()), 0, _stream()), "ttsk_gemm_group_launch_uploaded"),
                    lambda: (fl, kind, shape))
    return launch


DWG_TARGET_STEPS = (72, 72)   # K steps per workgroup: k = 1, taps (3 ranges at B = 16, T = 423: the measured optimum of 2 / 3 / 4)


DWG_SHORT_STEPS = 16


def dwgemm_splits(Bsz, S, k=1):
    """Utterance ranges per problem for dwgemm_batch: workgroups of about DWG_TARGET_STEPS 32-row K steps — at the 16 x 423-row step 4
    ranges for every problem (432 workgroups; 3 ranges for the PostNet's k = 5 — 372 workgroups, two even rounds of the capped 192 —
    measured the same: 2.816 vs 2.804 ms); short problems (the phoneme side: 2 steps per utterance) of about 16 steps, so that their few
    tiles still spread over the chip."""
    steps = Bsz * ((S + 31) // 32)
    target_steps = DWG_TARGET_STEPS[0] if k == 1 else DWG_TARGET_STEPS[1]
    if steps <= 64:
        target_steps = DWG_SHORT_STEPS
    return max(1, min(Bsz, (steps + target_steps // 2) // target_steps))


class DeferQueue:
    """The weight-gradient work a backward pass puts off (nothing but the optimiser reads its results), in the order it was queued:
    `group`   whole weight-gradient GEMMs (GemmDesc) for grouped launches — what `gemm(defer=...)` queues;
              group_gemms=False: it launches them one by one instead and queues only their split-K reduce items;
    `dwconv`  weight gradients of convs with taps: (dy, x, dst, lens, accumulate) for dwconv_batch (csrc/dwconv.hip);
    `dwgemm`  ... of Linear / k = 1 / PostNet layers with 256-multiple channels: (dy, x, dst, lens, accumulate, splits) (csrc/dwgemm.hip);
    `reduce`  (ReduceItem, slabs) of every split-K problem, for the batched reducer;
    `keep`    every tensor a launch of this queue reads or writes (operands, slabs, tables): alive until `flush`, because the launches
              may run on other streams than the one that allocated them and the caching allocator would hand them out again.
    The three kinds of problems stay three lists: each flush below states which it launches, on the stream current at the call."""

    def __init__(self, group_gemms=True):
        self.group_gemms = group_gemms
        self.group, self.dwconv, self.dwgemm, self.reduce, self.keep = [], [], [], [], []

    def _reduce(self, items):
        """One ttsk_gemm_reduce_batch launch over `items` [(ReduceItem, slabs)] on the current stream; the slabs join `keep`."""
        arr = (L.ReduceItem * len(items))(*[it for it, _ in items])
        check(L.load().ttsk_gemm_reduce_batch(arr, len(items), _stream()), "ttsk_gemm_reduce_batch")
        _count("reduce_batch")
        self.keep.extend(ws for _, ws in items)

    def flush_dwconv(self):
        """The queued conv weight gradients as ttsk_dwconv_batch launches (12 problems each, one kernel size each) on the current stream."""
        by_k = {}
        for it in self.dwconv:
            by_k.setdefault(it[2].shape[1], []).append(it)
            self.keep.extend(t for t in it[:4] if t is not None)
        for lst in by_k.values():
            for i in range(0, len(lst), 12):
                dwconv_batch(lst[i:i + 12])
        self.dwconv.clear()

    def flush_dwgemm(self, reduce_now=False, max_wgs=0):
        """The queued dwgemm problems as ttsk_dwgemm_batch launches on the current stream (grid capped at max_wgs when > 0); the reduce
        items of the split ones join `reduce` (summed by a later reduce_queued / flush), or are summed right here (reduce_now)."""
        if not self.dwgemm:
            return
        for it in self.dwgemm:
            self.keep.extend(t for t in it[:4] if t is not None)
        red = dwgemm_batch(self.dwgemm, max_wgs)
        self.dwgemm.clear()
        if reduce_now and red:
            self._reduce(red)
        else:
            self.reduce.extend(red)

    def flush_gemms(self, max_wgs=0, frac=1.0, small_too=False):
        """Everything but the reducer, on the current stream: the queued dwconv and dwgemm problems, all of them (dwgemm's grid capped
        at max_wgs workgroups when > 0, and its slabs then summed right behind it: this is the side stream's launch, which has the
        time), then the queued grouped GEMMs; their split-K slabs stay queued for reduce_queued / flush.  frac < 1: only about that
        fraction of the grouped FLOPs (the problems queued first); the rest stays queued for the next flush.
        A capped launch exists for the 256x128 configuration only: with max_wgs > 0 the few 128x128 problems (80-row / 80-column
        outputs: mel_linear, the PostNet's first and last conv) go behind it uncapped (small_too: 168 workgroups, two per CU) or
        stay queued for the final flush."""
        self.flush_dwconv()
        stamp("dw.dwconv")
        self.flush_dwgemm(reduce_now=max_wgs > 0, max_wgs=max_wgs)
        stamp("dw.dwgemm")
        now, small, later = list(self.group), [], []
        if max_wgs > 0:
            now, small = [d for d in self.group if d.kernel == 2], [d for d in self.group if d.kernel != 2]
        if frac < 1.0:
            fl = [2.0 * d.M * d.N * d.K * max(d.taps, 1) * d.nz1 * d.nz2 for d in now]
            want, acc, n = frac * sum(fl), 0.0, 0
            while n < len(now) and acc < want:
                acc += fl[n]
                n += 1
            now, later = now[:n], now[n:]
        flush_group(now, self.keep, max_wgs)
        if small_too:
            flush_group(small, self.keep)
        self.group[:] = later if small_too else later + small

    def upload_gemms(self):
        """The tables of the queued grouped GEMMs to the device now (current stream); returns the function that launches them, on the
        stream current when it is called (ordered behind this one by the caller).  The dwconv / dwgemm problems stay queued."""
        return upload_group(self.group, self.keep)

    def reduce_queued(self):
        """The batched reducer over every split-K item queued so far, on the current stream: the gradients of the problems launched
        so far are final behind it (the data-parallel "side" schedule announces its buckets there)."""
        if self.reduce:
            self._reduce(self.reduce)
            self.reduce.clear()

    def flush(self):
        """Whatever is still queued, on the current stream — dwconv, dwgemm, the grouped GEMMs, then one ttsk_gemm_reduce_batch launch
        for the split-K slabs — and the end of the queue's keep list: the caller has joined every stream the queue launched on."""
        self.flush_dwconv()
        self.flush_dwgemm()
        flush_group(self.group, self.keep)
        self.reduce_queued()
        self.keep = []


def queue_dw(defer, dy, x, dst, lens, accumulate, k=1, use_dwgemm=True):
    """Queue the weight gradient dst (Cout, k, Cin) (+)= dy (B,S,Cout)^T x (B,S,Cin) [taps: "same" padding] in the DeferQueue `defer`:
    on the 256x256-tile kernel (dwgemm.hip) when the shape allows, else as a grouped GEMM.  `lens`: rows of each utterance that carry
    a gradient (or None)."""
    Bsz, S, Cout = dy.shape
    Cin = x.shape[2]
    if (use_dwgemm and defer.group_gemms and dy.dtype == bf16 and x.dtype == bf16 and dwgemm_supported(Cout, Cin, k)
            and dst.is_contiguous()):
        sp = dwgemm_splits(Bsz, S, k)
        if (Bsz + sp - 1) // sp <= 64:
            defer.dwgemm.append((dy, x, dst.view(Cout, k, Cin), lens, accumulate, sp))
            return
    if k == 1:
        linear_dw(dy.reshape(Bsz * S, Cout), x.reshape(Bsz * S, Cin), dst.view(Cout, Cin), defer=defer, accumulate=accumulate)
    else:
        conv1d_dw(dy, x, dst, k=k, defer=defer, accumulate=accumulate)



def plan(d):
    """(kernel, splits, workspace_bytes) the library will use for descriptor `d` (ttsk_gemm_plan)."""
    k, sp, ws = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    check(L.load().ttsk_gemm_plan(C.byref(d), C.byref(k), C.byref(sp), C.byref(ws)), "ttsk_gemm_plan")
    return k.value, sp.value, ws.value


def gemm(A, B, Cout, M, N, K, lda, ldb, ldc, flags=0, alpha=1.0, bias=None, R=None, ldr=0, G=None, ldg=0, C2=None,
         nz1=1, nz2=1, sA=(0, 0), sB=(0, 0), sC=(0, 0), sR=(0, 0), taps=0, seg_len=0, tap_shift0=0, tap_dshift=0,
         b_tap_stride=0, bseg_len=0, bshift0=0, bdshift=0, out_seg=0, out_mul=0, out_add=0, out_add_dz=0, splits=0, kernel=0,
         in_slope=0.0, out_slope=0.0, defer=None, group=None, s_bias1=0, raw=False):
    """Raw descriptor-level call of ttsk_gemm (see include/ttsk.h).  A/B/Cout may be views: the data pointer of
    the view is the operand origin.  splits / kernel = 0 let the library plan (tile configuration, split-K factor);
    the split-K workspace is allocated here (the C library never allocates).  `defer`: a DeferQueue — a plain weight-
    gradient GEMM is then queued there whole for a grouped launch (group_gemms=False: launched here), and when it splits K it
    leaves its slabs un-reduced and queues a reduce item (see DeferQueue).  `group`: a
    GemmGroup — independent problems collected there run as ONE grouped launch at `group.flush()`.  `raw`: leave the fp32
    partial tiles [splits][M][N] un-reduced and without epilogue (TTSK_GEMM_RAW_SLABS); returns Slabs(ws, splits, M*N) for
    layernorm_bwd(slabs=...) — `Cout` may be None."""
    _dev(A, B, Cout, bias, R, G, C2)
    if raw:
        flags |= RAW_SLABS | C_F32
        if Cout is None:
            Cout = A                  # not written: any valid device pointer
    d = GemmDesc()
    d.A, d.B, d.C, d.C2 = _ptr(A), _ptr(B), _ptr(Cout), _ptr(C2)
    d.bias, d.R, d.G = _ptr(bias), _ptr(R), _ptr(G)
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc, d.ldr, d.ldg = lda, ldb, ldc, ldr, ldg
    if A.dtype == f16:
        flags |= F16
    if Cout.dtype == torch.float32 and not raw:
        flags |= C_F32
    if R is not None:
        flags |= ADD_R | (R_F32 if R.dtype == torch.float32 else 0)
    if G is not None:
        flags |= MASK_G
    d.flags, d.alpha, d.in_slope, d.out_slope = flags, alpha, in_slope, out_slope
    d.nz1, d.nz2 = nz1, nz2
    d.sA1, d.sA2 = sA
    d.sB1, d.sB2 = sB
    d.sC1, d.sC2 = sC
    d.sR1, d.sR2 = sR
    d.taps, d.seg_len, d.tap_shift0, d.tap_dshift, d.b_tap_stride = taps, seg_len, tap_shift0, tap_dshift, b_tap_stride
    d.bseg_len, d.bshift0, d.bdshift = bseg_len, bshift0, bdshift
    d.out_seg, d.out_mul, d.out_add, d.out_add_dz = out_seg, out_mul, out_add, out_add_dz
    d.splits, d.kernel, d.s_bias1 = splits, kernel, s_bias1
    user_splits, user_kernel = splits, kernel
    kernel, splits, ws_bytes = plan(d)
    if kernel == 3 and group is not None:
        # grouped launches exist for the 128x128 and 256x128 tiles only: plan again with the 128x128 tile
        d.kernel, d.splits = 1, user_splits
        kernel, splits, ws_bytes = plan(d)
    # a plain weight-gradient GEMM: fp32 output (+= or =) and nothing else — no epilogue, no bias, no first batch index, bf16 operands
    # (an fp16 A sets F16).  Only such a problem is deferred: its split-K slabs wait for the queue's reducer, and the problem itself
    # for a grouped launch when the queue groups
    plain_dw = defer is not None and nz1 == 1 and bool(flags & C_F32) and not (flags & ~(A_TR | B_TR | C_F32 | ACCUM_C)) and bias is None
    grouped_dw = plain_dw and defer.group_gemms
    if grouped_dw and user_splits == 0 and user_kernel == 0:
        # The planner splits K until ONE problem fills the chip (a 256x256 weight gradient over 6768 rows: 36 ways, 36 fp32
        # slabs to write and to reduce).  In a grouped launch the other problems fill it: ~28 (128x128 tiles) / ~36 (256x128) K steps per workgroup keep the
        # grid balanced with 4x-9x fewer slabs (750 MB -> ~50 MB of split-K traffic per train step).
        # Tile configuration: the 256x128 LDS-DMA kernel unless the output has too few rows to fill its tile.
        steps = (K + 63) // 64 * max(taps, 1)
        d.kernel = 2 if (M >= 192 and N >= 128) else 1        # (an 80-column output on the 256x128 tile would waste 3/8 of it)
        per1, per2 = DW_STEPS_PER_WG
        d.splits = max(1, (steps + per1 // 2) // per1) if d.kernel == 1 else max(1, (steps + per2 // 2) // per2)
        kernel, splits, ws_bytes = plan(d)
    d.splits, d.kernel = splits, kernel
    ws = None
    if ws_bytes > 0:
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=A.device)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws_bytes
        if plain_dw:
            d.flags = flags | DEFER_REDUCE
            it = L.ReduceItem()
            it.ws, it.C, it.M, it.N, it.ldc, it.nz, it.splits = ws.data_ptr(), Cout.data_ptr(), M, N, ldc, nz2, splits
            it.accumulate, it.sC2, it.alpha = int(bool(flags & ACCUM_C)), sC[1], alpha
            defer.reduce.append((it, ws))
    if raw:
        check(L.load().ttsk_gemm(C.byref(d), _stream()), "ttsk_gemm")
        return Slabs(ws, splits, M * N * nz1 * nz2)
    if group is not None:
        group.descs.append(d)
        group.keep.extend(t for t in (A, B, Cout, ws, bias, R, G, C2) if t is not None)
        return Cout
    if grouped_dw:
        # a weight-gradient GEMM: queued whole, launched with the others by one of the queue's flushes
        defer.group.append(d)
        defer.keep.extend(t for t in (A, B, Cout, ws) if t is not None)
        return Cout
    _traced(lambda: check(L.load().ttsk_gemm(C.byref(d), _stream()), "ttsk_gemm"),
            lambda: (2.0 * M * N * K * max(taps, 1) * nz1 * nz2, ("TT" if flags & A_TR else ("NT_btr" if flags & B_TR else "NT")) + str(kernel),
                     (M, N, K, max(taps, 1), nz1 * nz2, splits)))
    return Cout


_DUR_DTYPE = {torch.int64: 0, torch.float32: 1, torch.int32: 2}


def length_regulator_fwd(x, dur, T, pe=None, want_idx=True):
    """x (B,L,D) bf16, dur (B,L) int64/fp32/int32 -> out (B,T,D) bf16, idx (B,T) int32, cumsum (B,L) int32,
    mel_len (B,) int64 (uncropped).  reference: fs_two/model/modules.py:225-252."""
    _dev(x, dur, pe)
    B, Lp, D = x.shape
    out = torch.empty(B, T, D, dtype=bf16, device=x.device)
    idx = torch.empty(B, T, dtype=torch.int32, device=x.device) if want_idx else None
    cs = torch.empty(B, Lp, dtype=torch.int32, device=x.device)
    mel_len = torch.empty(B, dtype=torch.int64, device=x.device)
    dur = dur.contiguous()
    check(L.load().ttsk_length_regulator_fwd(_ptr(x.contiguous()), _ptr(dur), _DUR_DTYPE[dur.dtype], _ptr(pe), _ptr(out),
                                             _ptr(idx), _ptr(cs), _ptr(mel_len), B, Lp, T, D, _stream()),
          "ttsk_length_regulator_fwd")
    return out, idx, cs, mel_len


def length_regulator_bwd(dout, cs, L_src):
    _dev(dout, cs)
    B, T, D = dout.shape
    dx = torch.empty(B, L_src, D, dtype=bf16, device=dout.device)
    check(L.load().ttsk_length_regulator_bwd(_ptr(dout.contiguous()), _ptr(cs), _ptr(dx), B, L_src, T, D, _stream()),
          "ttsk_length_regulator_bwd")
    return dx


# ----------------------------------------------------------------------------------------------------------------
# GEMM-shaped ops expressed on the one kernel.  Activations are channels-last bf16 [rows][C], rows = B*T.
# Weights are the bf16 shadows: Linear (out,in); Conv1d (out, k, in)  [the fp32 masters use the same layout].

def linear(x, W, bias=None, out=None, flags=0, out_dtype=None, R=None, G=None, C2=None, alpha=1.0, out_slope=0.0, **kw):
    """y[M,N] = x[M,K] @ W[N,K]^T (+bias, epilogue).  reference: nn.Linear sites SubLayers.py:41-43,62; fastspeech2.py:102."""
    M, K = x.shape
    N = W.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype or x.dtype, device=x.device)
    return gemm(x, W, out, M, N, K, x.stride(0), W.stride(0), out.stride(0), flags=flags, alpha=alpha, bias=bias,
                R=R, ldr=0 if R is None else R.stride(0), G=G, ldg=0 if G is None else G.stride(0), C2=C2,
                out_slope=out_slope, **kw)


def linear_dx(dy, W, out=None, R=None, G=None, out_dtype=bf16, **kw):
    """dx[M,K] = dy[M,N] @ W[N,K]   (W read in place through the transposing LDS read)."""
    M, N = dy.shape
    K = W.shape[1]
    if kw.get("raw"):
        return gemm(dy, W, None, M, K, N, dy.stride(0), W.stride(0), K, flags=B_TR, **kw)
    if out is None:
        out = torch.empty(M, K, dtype=out_dtype, device=dy.device)
    return gemm(dy, W, out, M, K, N, dy.stride(0), W.stride(0), out.stride(0), flags=B_TR, R=R,
                ldr=0 if R is None else R.stride(0), G=G, ldg=0 if G is None else G.stride(0), **kw)


def linear_dw(dy, x, dst, accumulate=True, **kw):
    """dst[N,K] (fp32) (+)= dy[M,N]^T @ x[M,K]: contraction over rows (split-K over the rows, deterministic reduce)."""
    M, N = dy.shape
    K = x.shape[1]
    return gemm(dy, x, dst, N, K, M, dy.stride(0), x.stride(0), K, flags=A_TR | B_TR | (ACCUM_C if accumulate else 0), **kw)


def conv1d(x, W, bias, dilation=1, out=None, flags=0, out_dtype=None, R=None, C2=None, in_slope=0.0, out_slope=0.0,
           alpha=1.0, **kw):
    """'same' Conv1d on channels-last activations.  x (B,T,Cin) bf16, W (Cout,k,Cin) bf16 -> (B,T,Cout).
    reference: SubLayers.py:96 (k=9/1), modules.py:337-355 (k=3), Layers.py:59-67 (k=5), hifi/models.py:88-95."""
    Bsz, T, Cin = x.shape
    Cout, k, _ = W.shape
    pad = dilation * (k - 1) // 2
    if out is None:
        out = torch.empty(Bsz, T, Cout, dtype=out_dtype or x.dtype, device=x.device)
    gemm(x, W, out, Bsz * T, Cout, Cin, Cin, k * Cin, Cout, flags=flags, bias=bias, R=R, ldr=Cout, C2=C2, taps=k,
         seg_len=T, tap_shift0=-pad, tap_dshift=dilation, b_tap_stride=Cin, in_slope=in_slope, out_slope=out_slope,
         alpha=alpha, **kw)
    return out


def ffn_conv_supported(Cin, Cout, k):
    return bool(L.load().ttsk_ffn_conv_supported(Cin, Cout, k))


def ffn_pack_weight(W, out=None):
    """Tap-major (Cout,k,256) bf16 -> fragment-major pack for ffn_conv_fwd(packed=...) (ttsk_ffn_pack_weight)."""
    _dev(W, out)
    Cout, k, _ = W.shape
    if out is None:
        out = torch.empty(W.numel(), dtype=bf16, device=W.device)
    check(L.load().ttsk_ffn_pack_weight(_ptr(W), _ptr(out), Cout, k, _stream()), "ttsk_ffn_pack_weight")
    return out


def ffn_pack_weight_batch(Ws, outs):
    """ffn_pack_weight for up to 16 weights of one shape in one launch (ttsk_ffn_pack_weight_batch)."""
    _dev(*Ws, *outs)
    n = len(Ws)
    Cout, k, _ = Ws[0].shape
    src = (C.c_void_p * n)(*[w.data_ptr() for w in Ws])
    dst = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    check(L.load().ttsk_ffn_pack_weight_batch(C.cast(src, C.c_void_p), C.cast(dst, C.c_void_p), n, Cout, k, _stream()), "ttsk_ffn_pack_weight_batch")


def win_conv_supported(Cin, Cout, k):
    return bool(L.load().ttsk_win_conv_supported(Cin, Cout, k))


def win_conv_pack_batch(Ws, outs, transpose=False):
    """Fragment-major packs of up to 16 tap-major weights (Cs, k, Ds) of one shape in one launch (ttsk_win_conv_pack_batch);
    transpose: the pack of the conv's input gradient as a forward conv (taps flipped, channels swapped)."""
    _dev(*Ws, *outs)
    n = len(Ws)
    Cs, k, Ds = Ws[0].shape
    src = (C.c_void_p * n)(*[w.data_ptr() for w in Ws])
    dst = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    check(L.load().ttsk_win_conv_pack_batch(C.cast(src, C.c_void_p), C.cast(dst, C.c_void_p), n, Cs, k, Ds, int(transpose), _stream()),
          "ttsk_win_conv_pack_batch")


def win_conv_pack_items(items):
    """items: [(W (Cs,k,Ds) bf16 tap-major, out flat bf16, transpose)], up to 48 of any shapes, one launch (ttsk_win_conv_pack_items)."""
    n = len(items)
    arr = (L.PackItem * n)()
    for i, (W, out, tr) in enumerate(items):
        _dev(W, out)
        arr[i].src, arr[i].dst = W.data_ptr(), out.data_ptr()
        arr[i].Cs, arr[i].K, arr[i].Ds, arr[i].transpose = W.shape[0], W.shape[1], W.shape[2], int(tr)
    check(L.load().ttsk_win_conv_pack_items(arr, n, _stream()), "ttsk_win_conv_pack_items")


def win_conv_pack_table(items, device):
    """A device-resident item table for win_conv_pack_run: int32 tensor holding n `ttsk_pack_item`s (the tensors must stay where
    they are).  items as for win_conv_pack_items, any number."""
    n = len(items)
    arr = (L.PackItem * n)()
    for i, (W, out, tr) in enumerate(items):
        _dev(W, out)
        arr[i].src, arr[i].dst = W.data_ptr(), out.data_ptr()
        arr[i].Cs, arr[i].K, arr[i].Ds, arr[i].transpose = W.shape[0], W.shape[1], W.shape[2], int(tr)
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.int32).clone()
    return host.to(device), n


def win_conv_pack_run(table, n):
    """Rewrite every pack of a win_conv_pack_table in one launch (ttsk_win_conv_pack_table)."""
    check(L.load().ttsk_win_conv_pack_table(_ptr(table), n, _stream()), "ttsk_win_conv_pack_table")


@_family("win_conv", _conv_flops)
def win_conv(x, packed, Cout, k, bias=None, relu=False, out_dtype=None, gate=None, delta_o32=None, delta_out=None):
    """[relu](Conv1d(Cin -> Cout, k)(x) + bias) on the window kernel, weights = a win_conv_pack_batch pack (ttsk_win_conv); `gate`
    (B,S,Cout) bf16: result zeroed where gate <= 0.  x (B,S,Cin) bf16 -> (B,S,Cout) bf16 or fp32."""
    _dev(x, packed, bias, gate)
    Bsz, S, Cin = x.shape
    out = torch.empty(Bsz, S, Cout, dtype=out_dtype or bf16, device=x.device)
    _dev(delta_o32, delta_out)
    check(L.load().ttsk_win_conv(_ptr(x), _ptr(packed), _ptr(bias), _ptr(gate), _ptr(delta_o32), _ptr(delta_out), _ptr(out),
                                 int(out.dtype == torch.float32), Bsz, S, Cin, Cout, k, int(relu), _stream()), "ttsk_win_conv")
    return out


@_family("win_conv", _conv_flops)
def win_conv_stats(x, packed, Cout, k, bias=None, frame_limit=None):
    """win_conv with fp32 output (Cin = 512) that also returns the BatchNorm statistics partials of its output
    ([B * ceil(S/64)][2*Cout] fp32: sum | sum of squares per tile) for bn_train(partials=...) (ttsk_win_conv_stats)."""
    _dev(x, packed, bias)
    Bsz, S, Cin = x.shape
    lib = L.load()
    out = torch.empty(Bsz, S, Cout, dtype=torch.float32, device=x.device)
    stats = _f32(lib.ttsk_win_conv_stats_rows(Bsz, S), 2 * Cout, device=x.device)
    lp, _ = _lim(frame_limit)
    check(lib.ttsk_win_conv_stats(_ptr(x), _ptr(packed), _ptr(bias), _ptr(out), _ptr(stats), lp, Bsz, S, Cin, Cout, k, _stream()),
          "ttsk_win_conv_stats")
    return out, stats


@_family("win_conv", _conv_flops)
def win_conv_bnb(x, packed, Cout, k, bn_x, mean, rstd, gamma, beta, use_tanh, p=0.0, keep=None, frame_limit=None):
    """win_conv with bf16 output (Cin = 512: a PostNet conv's input gradient on its transposed pack) that also returns the BatchNorm-
    backward statistics partials of the layer below, whose upstream gradient the output is ([B * ceil(S/64)][2*Cout] fp32: sum of dy | sum
    of dy * xhat per tile) for bn_bwd(partials=...) (ttsk_win_conv_bnb).  bn_x (B*S, Cout) fp32: that layer's conv output; keep: its
    bn_train keep bits."""
    _dev(x, packed, bn_x, mean, rstd, gamma, beta, keep)
    Bsz, S, Cin = x.shape
    lib = L.load()
    out = torch.empty(Bsz, S, Cout, dtype=bf16, device=x.device)
    stats = _f32(lib.ttsk_win_conv_stats_rows(Bsz, S), 2 * Cout, device=x.device)
    lp, _ = _lim(frame_limit)
    check(lib.ttsk_win_conv_bnb(_ptr(x), _ptr(packed), _ptr(out), _ptr(stats), _ptr(bn_x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta),
                                _ptr(keep), float(p), int(use_tanh), lp, Bsz, S, Cin, Cout, k, _stream()), "ttsk_win_conv_bnb")
    return out, stats


@_family("win_conv", lambda x, packed, resid, Cout, k: 2.0 * x.shape[0] * x.shape[1] * x.shape[2] * Cout * k)
def win_conv_resid(x, packed, resid, Cout, k):
    """bf16 (B,S,Cout) = Conv1d(Cin -> Cout, k)(x) + resid (fp32 (B,S,Cout)) on the window kernel (ttsk_win_conv_resid): the PostNet's
    first conv's input gradient (512 -> 80 on the transposed pack) + the mel terms' own gradient."""
    _dev(x, packed, resid)
    Bsz, S, Cin = x.shape
    out = torch.empty(Bsz, S, Cout, dtype=bf16, device=x.device)
    check(L.load().ttsk_win_conv_resid(_ptr(x), _ptr(packed), _ptr(resid), _ptr(out), Bsz, S, Cin, Cout, k, _stream()), "ttsk_win_conv_resid")
    return out


@_family("win_conv", _conv_flops)
def win_conv_dual(x, packed, Cout, k, bias=None):
    """fp32 (B,S,Cout) = Conv1d(Cin -> Cout, k)(x) + bias on the window kernel, and its bf16 copy (ttsk_win_conv_dual: mel_linear)."""
    _dev(x, packed, bias)
    Bsz, S, Cin = x.shape
    out = torch.empty(Bsz, S, Cout, dtype=torch.float32, device=x.device)
    out16 = torch.empty(Bsz, S, Cout, dtype=bf16, device=x.device)
    check(L.load().ttsk_win_conv_dual(_ptr(x), _ptr(packed), _ptr(bias), _ptr(out), _ptr(out16), Bsz, S, Cin, Cout, k, _stream()), "ttsk_win_conv_dual")
    return out, out16


def win_pack_numel(Cs, k, Ds, transpose):
    """Elements of the fragment-major pack of a (Cs, k, Ds) tap-major weight (win_conv_pack_*): the contraction padded to whole 32-channel k-steps."""
    cout, cin = (Ds, Cs) if transpose else (Cs, Ds)
    return k * ((cin + 31) // 32) * 32 * cout


@_family("win_conv", _conv_flops)
def win_conv_split(x, packed, Cout, k):
    """An input-gradient conv with a wide contraction (x (B,S,n*256) bf16) as n window convs over 256-channel slices in one launch:
    fp32 Slabs (n, B*S*Cout) for layernorm_bwd(slabs=...) (ttsk_win_conv_split).  `packed`: the whole transposed pack."""
    _dev(x, packed)
    Bsz, S, Cin = x.shape
    n = Cin // 256
    ws = _f32(n, Bsz * S * Cout, device=x.device)
    check(L.load().ttsk_win_conv_split(_ptr(x), _ptr(packed), _ptr(ws), n, Bsz, S, Cin, Cout, k, _stream()), "ttsk_win_conv_split")
    return Slabs(ws, n, Bsz * S * Cout)


@_family("win_conv", lambda x, W, *a, **kw: 2.0 * x.shape[0] * x.shape[1] * x.shape[2] * W.shape[0] * W.shape[1])
def ffn_conv_fwd(x, W, bias, relu=True, packed=None):
    """relu(Conv1d(256 -> Cout, k)(x) + bias) on the window kernel (ttsk_ffn_conv_fwd; SubLayers.py:93-101, w_1).
    x (B,S,256) bf16, W (Cout,k,256) bf16 tap-major -> (B,S,Cout) bf16; `packed`: ffn_pack_weight(W), read instead of W."""
    _dev(x, W, bias, packed)
    Bsz, S, Cin = x.shape
    Cout, k, _ = W.shape
    out = torch.empty(Bsz, S, Cout, dtype=bf16, device=x.device)
    check(L.load().ttsk_ffn_conv_fwd(_ptr(x), _ptr(W if packed is None else packed), _ptr(bias), _ptr(out), Bsz, S, Cin, Cout, k, int(relu),
                                     int(packed is not None), _stream()), "ttsk_ffn_conv_fwd")
    return out


def conv1d_dx(dy, W, dilation=1, out=None, R=None, G=None, **kw):
    """dx (B,T,Cin) = sum_j dy[t + pad - j*dil] @ W[:, j, :]."""
    Bsz, T, Cout = dy.shape
    _, k, Cin = W.shape
    pad = dilation * (k - 1) // 2
    if kw.get("raw"):
        return gemm(dy, W, None, Bsz * T, Cin, Cout, Cout, k * Cin, Cin, flags=B_TR, taps=k, seg_len=T, tap_shift0=pad,
                    tap_dshift=-dilation, b_tap_stride=Cin, **kw)
    if out is None:
        out = torch.empty(Bsz, T, Cin, dtype=bf16, device=dy.device)
    gemm(dy, W, out, Bsz * T, Cin, Cout, Cout, k * Cin, Cin, flags=B_TR, R=R, ldr=Cin, G=G, ldg=Cin, taps=k, seg_len=T,
         tap_shift0=pad, tap_dshift=-dilation, b_tap_stride=Cin, **kw)
    return out


def conv1d_dw(dy, x, dst, dilation=1, k=1, accumulate=True, **kw):
    """dst (Cout,k,Cin) fp32 (+)= sum_rows dy[r, co] * x[r + j*dil - pad, ci]  (taps as the second batch index)."""
    Bsz, T, Cout = dy.shape
    Cin = x.shape[2]
    pad = dilation * (k - 1) // 2
    rows = Bsz * T
    gemm(dy, x, dst, Cout, Cin, rows, Cout, Cin, k * Cin, flags=A_TR | B_TR | (ACCUM_C if accumulate else 0), nz2=k,
         sC=(0, Cin), bseg_len=T, bshift0=-pad, bdshift=dilation, **kw)
    return dst


def dwconv_supported(Cout, Cin, k):
    return bool(L.load().ttsk_dwconv_supported(int(Cout), int(Cin), int(k)))


def dwconv_batch(items):
    """Weight gradients of Conv1d layers with taps, one launch (ttsk_dwconv_batch, csrc/dwconv.hip).  items: [(dy (B,S,Cout) bf16,
    x (B,S,Cin) bf16, dst (Cout,k,Cin) fp32, lens int64 (B,) or None, accumulate)], all of one k, at most 12."""
    arr = (L.DwConvItem * len(items))()
    for i, (dy, x, dst, lens, accumulate) in enumerate(items):
        _dev(dy, x, dst, lens)
        Bsz, S, Cout = dy.shape
        Cin = x.shape[2]
        if dst.shape[0] != Cout or dst.shape[2] != Cin or not dst.is_contiguous() or dst.dtype != torch.float32:
            raise L.TtskError("dwconv_batch: dst must be a contiguous fp32 (Cout, k, Cin) tensor")
        if dy.stride(2) != 1 or x.stride(2) != 1 or dy.stride(0) != S * dy.stride(1) or x.stride(0) != S * x.stride(1) or dy.dtype != bf16 or x.dtype != bf16:
            raise L.TtskError("dwconv_batch: dy / x must be bf16 (B, S, C) with unit channel stride and utterances back to back")
        it = arr[i]
        it.dy, it.x, it.dw, it.lens = dy.data_ptr(), x.data_ptr(), dst.data_ptr(), _ptr(lens)
        it.Cout, it.Cin, it.K, it.ldy, it.ldx, it.B, it.S, it.accumulate = Cout, Cin, dst.shape[1], dy.stride(1), x.stride(1), Bsz, S, int(bool(accumulate))
    def describe():
        # algorithmic FLOPs: every row of every utterance (2*B*S*Cout*Cin*k), whatever `lens` lets the kernel skip
        fl = sum(2.0 * it[0].shape[0] * it[0].shape[1] * it[0].shape[2] * it[1].shape[2] * it[2].shape[1] for it in items)
        nwg = sum((it[0].shape[2] // 256) * (it[1].shape[2] // 32) for it in items)
        return fl, "dwconv%d" % items[0][2].shape[1], (len(items), 0, 0, 1, 1, nwg)
    _traced(lambda: check(L.load().ttsk_dwconv_batch(arr, len(items), _stream()), "ttsk_dwconv_batch"), describe)
    _count("dwconv")


def dwgemm_supported(Cout, Cin, k):
    return bool(L.load().ttsk_dwgemm_supported(int(Cout), int(Cin), int(k)))


def dwgemm_batch(items, max_wgs=0):
    """Weight gradients with Cout, Cin multiples of 256 on the 256x256-tile kernel (ttsk_dwgemm_batch, csrc/dwgemm.hip), one launch per
    28 problems.  items: [(dy (B,S,Cout) bf16, x (B,S,Cin) bf16, dst (Cout,k,Cin) fp32 or (Cout,Cin), lens int64 (B,) or None, accumulate,
    splits)].  Returns [(ReduceItem, slabs)] for the problems with splits > 1: run gemm_reduce_batch on them (DeferQueue does)."""
    lib = L.load()
    reduce = []
    for base in range(0, len(items), 28):
        chunk = items[base:base + 28]
        arr = (L.DwGemmItem * len(chunk))()
        keep = []
        for i, (dy, x, dst, lens, accumulate, splits) in enumerate(chunk):
            _dev(dy, x, dst, lens)
            Bsz, S, Cout = dy.shape
            Cin = x.shape[2]
            k = dst.shape[1] if dst.dim() == 3 else 1
            if dst.numel() != Cout * k * Cin or not dst.is_contiguous() or dst.dtype != torch.float32:
                raise L.TtskError("dwgemm_batch: dst must be a contiguous fp32 (Cout, k, Cin) tensor")
            if dy.stride(2) != 1 or x.stride(2) != 1 or dy.stride(0) != S * dy.stride(1) or x.stride(0) != S * x.stride(1) or dy.dtype != bf16 or x.dtype != bf16:
                raise L.TtskError("dwgemm_batch: dy / x must be bf16 (B, S, C) with unit channel stride and utterances back to back")
            splits = max(1, min(int(splits), Bsz))
            ws = torch.empty(splits * k * Cout * Cin, dtype=torch.float32, device=dy.device) if splits > 1 else None
            it = arr[i]
            it.dy, it.x, it.dw, it.workspace, it.lens = dy.data_ptr(), x.data_ptr(), dst.data_ptr(), _ptr(ws), _ptr(lens)
            it.Cout, it.Cin, it.K, it.ldy, it.ldx, it.B, it.S = Cout, Cin, k, dy.stride(1), x.stride(1), Bsz, S
            it.accumulate, it.splits = int(bool(accumulate)), splits
            if ws is not None:
                r = L.ReduceItem()
                r.ws, r.C, r.M, r.N, r.ldc, r.nz, r.splits = ws.data_ptr(), dst.data_ptr(), Cout, Cin, k * Cin, k, splits
                r.accumulate, r.sC2, r.alpha = int(bool(accumulate)), Cin, 1.0
                reduce.append((r, ws))
        _traced(lambda: check(lib.ttsk_dwgemm_batch(arr, len(chunk), int(max_wgs), _stream()), "ttsk_dwgemm_batch"),
                lambda: (sum(2.0 * it[0].shape[0] * it[0].shape[1] * it[0].shape[2] * it[1].shape[2] * (it[2].shape[1] if it[2].dim() == 3 else 1)
                             for it in chunk), "dwgemm", (len(chunk), 0, 0, 1, 1, 0)))
        _count("dwgemm")
    return reduce


def check_upsampler(k, stride, what):
    """Every upsampler kernel here computes ConvTranspose1d(k, stride, padding=(k - stride) // 2) as `stride` phases of k // stride
    taps each, T * stride samples out.  That is torch's layer only when stride divides k (else the low phases own one tap more, which
    would be dropped) and k - stride is even (else torch's output is one sample longer): anything else is refused, by name."""
    if k < stride or k % stride != 0 or (k - stride) % 2 != 0:
        raise L.TtskError("%s: kernel size %d with stride %d is not supported (the stride must divide the kernel size and their "
                          "difference must be even)" % (what, k, stride))


def conv_transpose1d(x, Wp, bias, stride, k, out=None, in_slope=0.0, flags=0, C2=None, out_slope=0.0, **kw):
    """ConvTranspose1d(padding=(k-stride)//2) as `stride` polyphase implicit GEMMs.
    x (B,T,Cin) bf16, Wp (k, Cout, Cin) bf16 (tap-major repack of torch's (Cin,Cout,k)) -> (B,T*stride,Cout).
    reference: hifi/models.py:166-176,189."""
    Bsz, T, Cin = x.shape
    Cout = Wp.shape[1]
    check_upsampler(k, stride, "conv_transpose1d")
    p = (k - stride) // 2
    if out is None:
        out = torch.empty(Bsz, T * stride, Cout, dtype=x.dtype, device=x.device)
    taps = k // stride
    # phases r = 0..stride-1; phases with the same first tap offset qoff share one launch (batch index z2 = phase):
    # their weights Wp[r] are consecutive, their output rows differ by one (out_add_dz = 1)
    groups = []
    for r in range(stride):
        qoff = max(0, -((r - p) // stride))          # ceil((p - r)/stride) clipped at 0
        if groups and groups[-1][1] == qoff:
            groups[-1][2] += 1
        else:
            groups.append([r, qoff, 1])
    for r0, qoff, n in groups:
        gemm(x, Wp[r0], out, Bsz * T, Cout, Cin, Cin, Cin, Cout, flags=flags | (LRELU_IN if in_slope else 0),
             bias=bias, taps=taps, seg_len=T, tap_shift0=qoff, tap_dshift=-1, b_tap_stride=stride * Cout * Cin,
             out_seg=T * stride, out_mul=stride, out_add=qoff * stride + r0 - p, out_add_dz=1, nz2=n, sB=(0, Cout * Cin),
             in_slope=in_slope, C2=C2, out_slope=out_slope, **kw)
    return out


# ----------------------------------------------------------------------------------------------------------------
# row kernels

def _f32(*shape, device):
    return torch.empty(*shape, dtype=torch.float32, device=device)


def layernorm_fwd(y, res, gamma, beta, lens=None, seg_len=0, p_pre=0.0, site_pre=0, p_post=0.0, site_post=0, rng=None,
                  save_z=True, head=None, want_out=True, eps=1e-5, out=None):
    """Fused block tail (see include/ttsk.h).  y/res (rows,D) bf16.  Returns (out, z, mean, rstd, head_out)."""
    _dev(y, res, gamma, beta, lens, rng)
    rows, D = y.shape
    dev = y.device
    if out is None:
        out = torch.empty(rows, D, dtype=bf16, device=dev) if want_out else None
    z = torch.empty(rows, D, dtype=bf16, device=dev) if save_z else None
    mean, rstd = _f32(rows, device=dev), _f32(rows, device=dev)
    hw = hb = ho = None
    if head is not None:
        hw, hb = head
        ho = _f32(rows, device=dev)
    check(L.load().ttsk_layernorm_fwd(_ptr(y), _ptr(res), _ptr(gamma), _ptr(beta), _ptr(out), _ptr(z), _ptr(mean), _ptr(rstd),
                                      _ptr(lens), seg_len, rows, D, eps, p_pre, site_pre, p_post, site_post, _ptr(rng),
                                      _ptr(hw), _ptr(hb), _ptr(ho), _stream()), "ttsk_layernorm_fwd")
    return out, z, mean, rstd, ho


def gemm_ln_fwd(x, W, bias, res, gamma, beta, lens=None, seg_len=0, p_pre=0.0, site_pre=0, rng=None, save_z=True, eps=1e-5, out=None):
    """LayerNorm(dropout(x @ W^T + bias) + res) with PAD rows zeroed, one kernel (D = 256).  x (rows, K) bf16, W (256, K) or
    (256, 1, K) bf16.  Returns (out, z, mean, rstd) like layernorm_fwd."""
    _dev(x, W, bias, res, gamma, beta, lens, rng)
    rows, K = x.shape
    D = W.shape[0]
    W2 = W.reshape(D, -1)
    dev = x.device
    if out is None:
        out = torch.empty(rows, D, dtype=bf16, device=dev)
    z = torch.empty(rows, D, dtype=bf16, device=dev) if save_z else None
    mean, rstd = _f32(rows, device=dev), _f32(rows, device=dev)
    check(L.load().ttsk_gemm_ln_fwd(_ptr(x), x.stride(0), _ptr(W2), W2.stride(0), _ptr(bias), _ptr(res), _ptr(gamma), _ptr(beta),
                                    _ptr(out), _ptr(z), _ptr(mean), _ptr(rstd), _ptr(lens), seg_len, rows, K, D, eps, p_pre, site_pre,
                                    _ptr(rng), _stream()), "ttsk_gemm_ln_fwd")
    return out, z, mean, rstd


def win_ln_supported(K, D):
    return bool(L.load().ttsk_win_ln_supported(K, D))


@_family("win_ln", lambda x, *a, **kw: 2.0 * x.shape[0] * x.shape[1] * 256 + (2.0 * x.shape[0] * 256 * 768 if kw.get("proj") is not None else 0.0))
def win_ln_fwd(x, packed, bias, res, gamma, beta, lens=None, seg_len=0, p_pre=0.0, site_pre=0, rng=None, save_z=True, eps=1e-5, out=None,
               proj=None):
    """gemm_ln_fwd with the weight as a fragment-major pack (win_conv_pack_*; ttsk_win_ln_fwd): x (rows, K) bf16, K = 256 or 1024.
    proj = (packed q|k|v weight, bias fp32[768]): the next block's q|k|v projection of the output rows in the same launch
    (ttsk_win_ln_proj_fwd); then returns (out, z, mean, rstd, qkv)."""
    _dev(x, packed, bias, res, gamma, beta, lens, rng)
    rows, K = x.shape
    D = 256
    dev = x.device
    if out is None:
        out = torch.empty(rows, D, dtype=bf16, device=dev)
    z = torch.empty(rows, D, dtype=bf16, device=dev) if save_z else None
    mean, rstd = _f32(rows, device=dev), _f32(rows, device=dev)
    if proj is not None:
        pw, pb = proj
        _dev(pw, pb)
        qkv = torch.empty(rows, 3 * D, dtype=bf16, device=dev)
        check(L.load().ttsk_win_ln_proj_fwd(_ptr(x), x.stride(0), _ptr(packed), _ptr(bias), _ptr(res), _ptr(gamma), _ptr(beta), _ptr(out), _ptr(z),
                                            _ptr(mean), _ptr(rstd), _ptr(lens), seg_len, rows, K, D, eps, p_pre, site_pre, _ptr(rng), _ptr(pw),
                                            _ptr(pb), 3 * D, _ptr(qkv), _stream()), "ttsk_win_ln_proj_fwd")
        return out, z, mean, rstd, qkv
    check(L.load().ttsk_win_ln_fwd(_ptr(x), x.stride(0), _ptr(packed), _ptr(bias), _ptr(res), _ptr(gamma), _ptr(beta), _ptr(out), _ptr(z),
                                   _ptr(mean), _ptr(rstd), _ptr(lens), seg_len, rows, K, D, eps, p_pre, site_pre, _ptr(rng), _stream()),
          "ttsk_win_ln_fwd")
    return out, z, mean, rstd


def layernorm_bwd(dout, z, mean, rstd, gamma, beta, lens=None, seg_len=0, relu_in=False, p_pre=0.0, site_pre=0,
                  p_post=0.0, site_post=0, rng=None, dhead=None, head_w=None, want_dz=True, slabs=None, R=None):
    """Returns (dz, dy, partials, nblk).  dy is dz when p_pre == 0.  partials layout: see include/ttsk.h.
    `slabs` (a Slabs from gemm(raw=True)) + `R` (bf16 residual) replace `dout`: dout = sum of the slabs + R, summed in fp32
    while the rows are read (ttsk_layernorm_bwd_slabs)."""
    _dev(dout, z, dhead, R)
    rows, D = z.shape
    dev = z.device
    lib = L.load()
    nblk = lib.ttsk_layernorm_bwd_nblocks(rows)
    ncol = (4 * D + 1) if dhead is not None else 3 * D
    partials = _f32(nblk, ncol, device=dev)
    dz = torch.empty(rows, D, dtype=bf16, device=dev) if (want_dz or p_pre == 0.0) else None
    dy = torch.empty(rows, D, dtype=bf16, device=dev) if p_pre > 0.0 else None
    if slabs is not None:
        check(lib.ttsk_layernorm_bwd_slabs(_ptr(slabs.ws), slabs.splits, slabs.stride, _ptr(R), _ptr(z), _ptr(mean), _ptr(rstd), _ptr(gamma),
                                           _ptr(beta), _ptr(lens), seg_len, rows, D, int(relu_in), p_pre, site_pre, p_post, site_post,
                                           _ptr(rng), _ptr(dz), _ptr(dy), _ptr(partials), _stream()), "ttsk_layernorm_bwd_slabs")
        return dz, (dy if dy is not None else dz), partials, nblk
    check(lib.ttsk_layernorm_bwd(_ptr(dout), _ptr(dhead), _ptr(head_w), _ptr(z), _ptr(mean), _ptr(rstd), _ptr(gamma),
                                 _ptr(beta), _ptr(lens), seg_len, rows, D, int(relu_in), p_pre, site_pre, p_post,
                                 site_post, _ptr(rng), _ptr(dz), _ptr(dy), _ptr(partials), _stream()), "ttsk_layernorm_bwd")
    return dz, (dy if dy is not None else dz), partials, nblk


@_family("ln_bwd_proj", lambda dout, z, mean, rstd, gamma, packed, Cout, *a, **kw: 2.0 * z.shape[0] * 256 * Cout + (2.0 * z.shape[0] * 768 * 256 if kw.get("pre") is not None else 0.0))
def layernorm_bwd_proj(dout, z, mean, rstd, gamma, packed, Cout, lens=None, seg_len=0, p_pre=0.0, site_pre=0, rng=None, slabs=None, R=None,
                       gate=None, delta_o32=None, delta_out=None, pre=None):
    """layernorm_bwd (D = 256) and the k = 1 window conv on its dy in ONE launch (ttsk_layernorm_bwd_proj): `packed` is the
    win_conv pack of the transposed weight, Cout 256 or 1024; gate / delta as for win_conv.
    pre = (x (rows, 768) bf16, packed transposed weight): the upstream gradient is x · W' (+ R), computed inside the kernel too
    (instead of dout / slabs).  Returns (dz, dy, partials, nblk, out)."""
    _dev(dout, z, R, gate, delta_o32, delta_out, packed)
    px, pw = pre if pre is not None else (None, None)
    _dev(px, pw)
    rows, D = z.shape
    dev = z.device
    lib = L.load()
    nblk = lib.ttsk_layernorm_bwd_proj_nblocks(rows)
    partials = _f32(nblk, 3 * D, device=dev)
    dz = torch.empty(rows, D, dtype=bf16, device=dev)
    dy = torch.empty(rows, D, dtype=bf16, device=dev) if p_pre > 0.0 else None
    out = torch.empty(rows, Cout, dtype=bf16, device=dev)
    check(lib.ttsk_layernorm_bwd_proj(_ptr(dout), _ptr(slabs.ws) if slabs is not None else None, slabs.splits if slabs is not None else 0,
                                      slabs.stride if slabs is not None else 0, _ptr(R), _ptr(z), _ptr(mean), _ptr(rstd), _ptr(gamma),
                                      _ptr(lens), seg_len, rows, D, p_pre, site_pre, _ptr(rng), _ptr(dz), _ptr(dy), _ptr(partials),
                                      _ptr(packed), Cout, _ptr(gate), _ptr(delta_o32), _ptr(delta_out), _ptr(out), _ptr(px), _ptr(pw),
                                      px.shape[1] if px is not None else 0, _stream()),
          "ttsk_layernorm_bwd_proj")
    return dz, (dy if dy is not None else dz), partials, nblk, out


@_family("ln_bwd_proj", lambda dqkv, *a, **kw: 2.0 * dqkv.shape[0] * dqkv.shape[1] * 256)
def qkv_dx(dqkv, packed, R=None):
    """dqkv (rows, 768) bf16 x the packed transposed q|k|v weight (+ R) -> (rows, 256) bf16 (ttsk_qkv_dx)."""
    _dev(dqkv, packed, R)
    rows, K = dqkv.shape
    out = torch.empty(rows, 256, dtype=bf16, device=dqkv.device)
    check(L.load().ttsk_qkv_dx(_ptr(dqkv), _ptr(packed), _ptr(R), _ptr(out), rows, K, 256, _stream()), "ttsk_qkv_dx")
    return out


def layernorm_fwd_grouped(y, gamma, beta, groups, param_stride, site_stride, lens=None, seg_len=0, p_post=0.0, site_post=0, rng=None,
                          head=None, want_out=True, eps=1e-5):
    """`groups` independent LayerNorm tails in one launch (the three VariancePredictors): y (groups*group_rows, D) bf16; group g
    takes its gamma / beta / head at + g*param_stride floats and dropout site site_post + g*site_stride.  -> (out, mean, rstd, head_out)."""
    _dev(y, gamma, beta, lens, rng)
    rows, D = y.shape
    dev = y.device
    out = torch.empty(rows, D, dtype=bf16, device=dev) if want_out else None
    mean, rstd = _f32(rows, device=dev), _f32(rows, device=dev)
    hw = hb = ho = None
    if head is not None:
        hw, hb = head
        ho = _f32(rows, device=dev)
    check(L.load().ttsk_layernorm_fwd_grouped(_ptr(y), None, _ptr(gamma), _ptr(beta), _ptr(out), None, _ptr(mean), _ptr(rstd), _ptr(lens),
                                              seg_len, groups, rows // groups, param_stride, site_stride, D, eps, 0.0, 0, p_post, site_post,
                                              _ptr(rng), _ptr(hw), _ptr(hb), _ptr(ho), _stream()), "ttsk_layernorm_fwd_grouped")
    return out, mean, rstd, ho


def layernorm_bwd_grouped(dout, z, mean, rstd, gamma, beta, groups, param_stride, site_stride, lens=None, seg_len=0, relu_in=False,
                          p_post=0.0, site_post=0, rng=None, dhead=None, head_w=None):
    """Backward of layernorm_fwd_grouped.  Returns (dz, partials [groups][nblk][ncol], nblk per group)."""
    _dev(dout, z, dhead)
    rows, D = z.shape
    dev = z.device
    lib = L.load()
    nblk = lib.ttsk_layernorm_bwd_nblocks(rows // groups)
    ncol = (4 * D + 1) if dhead is not None else 3 * D
    partials = _f32(groups, nblk, ncol, device=dev)
    dz = torch.empty(rows, D, dtype=bf16, device=dev)
    check(lib.ttsk_layernorm_bwd_grouped(_ptr(dout), _ptr(dhead), _ptr(head_w), _ptr(z), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta),
                                         _ptr(lens), seg_len, groups, rows // groups, param_stride, site_stride, D, int(relu_in), 0.0, 0,
                                         p_post, site_post, _ptr(rng), _ptr(dz), None, _ptr(partials), _stream()), "ttsk_layernorm_bwd_grouped")
    return dz, partials, nblk


def va_embed(stack, speakers, spk_table, Lp, pitch_t, pitch_bins, pitch_table, energy_t, energy_bins, energy_table, row_limit=None):
    """stack (3, rows, D) bf16 with stack[0] = encoder output: fills stack[1] = x + speaker, stack[2] = stack[1] + pitch embedding and
    returns (x3 = stack[2] + energy embedding, pitch bucket indices, energy bucket indices).  reference: modules.py:158-193."""
    _dev(stack, speakers, spk_table, pitch_t, pitch_bins, pitch_table, energy_t, energy_bins, energy_table)
    _, rows, D = stack.shape
    x3 = torch.empty(rows, D, dtype=bf16, device=stack.device)
    pidx = torch.empty(rows, dtype=torch.int32, device=stack.device)
    eidx = torch.empty(rows, dtype=torch.int32, device=stack.device)
    check(L.load().ttsk_va_embed(_ptr(stack[0]), _ptr(spk_table), _ptr(speakers), Lp, _ptr(pitch_t), _ptr(pitch_bins), _ptr(pitch_table),
                                 _ptr(energy_t), _ptr(energy_bins), _ptr(energy_table), pitch_bins.numel(), _ptr(stack[1]), _ptr(stack[2]),
                                 _ptr(x3), _ptr(pidx), _ptr(eidx), rows, D, _ptr(row_limit), _stream()), "ttsk_va_embed")
    return x3, pidx, eidx


def va_combine(dx3, dxin, Lp=0, row_limit=None):
    """dx3 (rows, D) bf16, dxin (3, rows, D) fp32 -> (dx2, dx1, dx) bf16: see include/ttsk.h."""
    _dev(dx3, dxin, row_limit)
    rows, D = dx3.shape
    dx2, dx1, dx = torch.empty_like(dx3), torch.empty_like(dx3), torch.empty_like(dx3)
    check(L.load().ttsk_va_combine(_ptr(dx3), _ptr(dxin), _ptr(dx2), _ptr(dx1), _ptr(dx), rows, D, Lp, _ptr(row_limit), _stream()), "ttsk_va_combine")
    return dx2, dx1, dx


def colsum_finalize(partials, nblk, ncols, ld, dst, accumulate=True, scale=1.0, defer=None):
    """dst[c] (+)= scale * sum_b partials[b*ld + c].  `defer`: a list — the item is queued for flush_finalize instead."""
    if defer is not None:
        it = L.FinalizeItem()
        it.partials, it.dst, it.nblk, it.ncols, it.ld, it.accumulate, it.scale = partials.data_ptr(), dst.data_ptr(), nblk, ncols, ld, int(accumulate), scale
        defer.append((it, partials))
        return dst
    check(L.load().ttsk_colsum_finalize(_ptr(partials), nblk, ncols, ld, _ptr(dst), int(accumulate), scale, _stream()),
          "ttsk_colsum_finalize")
    return dst


def flush_finalize(items):
    """One launch each for the queued embedding scatter-sums, the queued column sums (bias gradients) and then all queued
    finalisations (ttsk_scatter_sum_batch, ttsk_colsum_batch, ttsk_colsum_finalize_batch)."""
    if not items:
        return
    if LAUNCH_COUNTS is not None:
        LAUNCH_COUNTS["colsum_flush"] = LAUNCH_COUNTS.get("colsum_flush", 0) + 1
    sc = [it for it, _ in items if isinstance(it, L.ScatterItem)]
    if sc:
        check(L.load().ttsk_scatter_sum_batch((L.ScatterItem * len(sc))(*sc), len(sc), _stream()), "ttsk_scatter_sum_batch")
    cs = [it for it, _ in items if isinstance(it, L.ColsumItem)]
    if cs:
        check(L.load().ttsk_colsum_batch((L.ColsumItem * len(cs))(*cs), len(cs), _stream()), "ttsk_colsum_batch")
    fin = [(it, keep) for it, keep in items if isinstance(it, L.FinalizeItem)]
    items[:] = fin
    if items:
        arr = (L.FinalizeItem * len(items))(*[it for it, _ in items])
        check(L.load().ttsk_colsum_finalize_batch(arr, len(items), _stream()), "ttsk_colsum_finalize_batch")
    items.clear()


def colsum_into(x, dst, accumulate=True, defer=None):
    """dst[C] (+)= column sums of x (rows, C) — bias gradients."""
    _dev(x, dst)
    rows, Cn = x.shape
    if Cn > 1024:
        # ttsk_colsum sums at most 1024 columns per pass (a hidden size of 512: the q|k|v bias gradient has 1536): column slices of
        # the same rows, each a column sum of its own (1024 columns keep a slice's rows 16-byte aligned)
        for c0 in range(0, Cn, 1024):
            colsum_into(x[:, c0:c0 + 1024], dst[c0:c0 + 1024], accumulate=accumulate, defer=defer)
        return dst
    lib = L.load()
    nblk = lib.ttsk_colsum_nblocks(rows)
    partials = _f32(nblk, Cn, device=x.device)
    if defer is not None:          # queue the column sum itself as well; `x` stays alive until flush_finalize
        it = L.ColsumItem()
        it.x, it.partials, it.is_f32, it.rows, it.C, it.ld, it.nblk = x.data_ptr(), partials.data_ptr(), int(x.dtype == torch.float32), rows, Cn, x.stride(0), nblk
        defer.append((it, x))
    else:
        check(lib.ttsk_colsum(_ptr(x), int(x.dtype == torch.float32), rows, Cn, x.stride(0), _ptr(partials), _stream()), "ttsk_colsum")
    return colsum_finalize(partials, nblk, Cn, Cn, dst, accumulate, defer=defer)


@_family("flash_attention", lambda qkv, lens, Bn, H, S, *a, **kw: 4.0 * Bn * S * S * (qkv.shape[1] // 3))
def flash_attention_fwd(qkv, lens, Bn, H, S, want_lse):
    """softmax(Q K^T / sqrt(128) + key mask) V on the q|k|v buffer (rows, 3d) -> (o (rows, d) bf16, lse (B*H, S) fp32 or None,
    o32 (rows, d) fp32 or None) with no S x S tensor in HBM (ttsk_flash_attention_fwd); lse and o32 are what the backward needs."""
    _dev(qkv, lens)
    d = qkv.shape[1] // 3
    o = torch.empty(Bn * S, d, dtype=bf16, device=qkv.device)
    lse = _f32(Bn * H, S, device=qkv.device) if want_lse else None
    o32 = _f32(Bn * S, d, device=qkv.device) if want_lse else None
    check(L.load().ttsk_flash_attention_fwd(_ptr(qkv), _ptr(o), _ptr(o32), _ptr(lse), _ptr(lens), Bn, H, S, d, (d // H) ** -0.5, _stream()),
          "ttsk_flash_attention_fwd")
    return o, lse, o32


@_family("flash_attention", lambda qkv, o, do, lse, lens, Bn, H, S, *a, **kw: 8.0 * Bn * S * S * (qkv.shape[1] // 3))
def flash_attention_bwd(qkv, o, do, lse, lens, Bn, H, S, o32=None, delta=None):
    """dqkv (rows, 3d) bf16 = gradients of q | k | v (ttsk_flash_attention_bwd: delta, then dQ and dK/dV sides as one grid; P
    recomputed from lse).  `delta` (B*H, S) fp32: already computed by the producer of `do` (win_conv(delta_out=...)): no delta launch."""
    _dev(qkv, o, do, lse, lens, o32, delta)
    d = qkv.shape[1] // 3
    dqkv = torch.empty(Bn * S, 3 * d, dtype=bf16, device=qkv.device)
    ready = delta is not None
    if delta is None:
        delta = _f32(Bn * H, S, device=qkv.device)
    check(L.load().ttsk_flash_attention_bwd(_ptr(qkv), _ptr(o), _ptr(o32), _ptr(do), _ptr(lse), _ptr(delta), int(ready), _ptr(dqkv), _ptr(lens),
                                            Bn, H, S, d, (d // H) ** -0.5, _stream()), "ttsk_flash_attention_bwd")
    return dqkv


def softmax_fwd(scores, lens, H):
    """scores (nz,S,Sp) fp32 -> probs (nz,S,Sp) bf16; keys >= lens[z // H] masked."""
    _dev(scores, lens)
    nz, S, Sp = scores.shape
    probs = torch.empty(nz, S, Sp, dtype=bf16, device=scores.device)
    check(L.load().ttsk_softmax_fwd(_ptr(scores), _ptr(probs), _ptr(lens), nz, H, S, Sp, _stream()), "ttsk_softmax_fwd")
    return probs


def softmax_bwd(probs, dprobs, alpha):
    _dev(probs, dprobs)
    nz, S, Sp = probs.shape
    ds = torch.empty(nz, S, Sp, dtype=bf16, device=probs.device)
    check(L.load().ttsk_softmax_bwd(_ptr(probs), _ptr(dprobs), _ptr(ds), nz, S, Sp, alpha, _stream()), "ttsk_softmax_bwd")
    return ds


def bucketize(values, bins, scale=1.0, want_scaled=False):
    _dev(values, bins)
    values = values.contiguous()
    idx = torch.empty(values.shape, dtype=torch.int32, device=values.device)
    scaled = torch.empty_like(values) if want_scaled else None
    check(L.load().ttsk_bucketize(_ptr(values), _ptr(bins), bins.numel(), scale, _ptr(idx), _ptr(scaled), values.numel(),
                                  _stream()), "ttsk_bucketize")
    return (idx, scaled) if want_scaled else idx


def duration_round(logd, d_control=1.0):
    _dev(logd)
    out = torch.empty_like(logd)
    check(L.load().ttsk_duration_round(_ptr(logd), d_control, _ptr(out), logd.numel(), _stream()), "ttsk_duration_round")
    return out


def duration_round_dev(logd, d_control):
    """`duration_round` with one control per utterance: logd (B, L) fp32, d_control (B,) fp32 on the device."""
    _dev(logd, d_control)
    if logd.dtype != torch.float32 or d_control.dtype != torch.float32 or logd.dim() != 2 or not logd.is_contiguous() \
            or not d_control.is_contiguous() or d_control.numel() != logd.shape[0]:
        raise L.TtskError("duration_round_dev: needs contiguous fp32 logd (B, L) and d_control (B,), got %s and %s" % (tuple(logd.shape), tuple(d_control.shape)))
    out = torch.empty_like(logd)
    check(L.load().ttsk_duration_round_dev(_ptr(logd), _ptr(d_control), logd.shape[-1], _ptr(out), logd.numel(), _stream()),
          "ttsk_duration_round_dev")
    return out


def length_mask(lens, T):
    """(B,) int64 -> (B,T) bool, True = PAD.  reference: fs_two/utils/tools.py:121-131."""
    _dev(lens)
    B = lens.shape[0]
    mask = torch.empty(B, T, dtype=torch.bool, device=lens.device)
    check(L.load().ttsk_length_mask(_ptr(lens), _ptr(mask), B, T, _stream()), "ttsk_length_mask")
    return mask


def add_f32(a, b, out=None, scale_b=1.0):
    """out = a + scale_b * b (fp32, same shapes)."""
    _dev(a, b)
    if out is None:
        out = torch.empty_like(a)
    check(L.load().ttsk_add_f32(_ptr(a), _ptr(b), scale_b, _ptr(out), a.numel(), _stream()), "ttsk_add_f32")
    return out


def gather_add(x, table, idx, idx_div=1, pe=None, pe_mod=1, rows=None, out=None):
    """out[row] = (x[row] if x is not None) + table[idx[row // idx_div]] + pe[row % pe_mod]; bf16 (rows, D)."""
    _dev(x, table, idx, pe)
    D = table.shape[1]
    if rows is None:
        rows = x.shape[0]
    if out is None:
        out = torch.empty(rows, D, dtype=bf16, device=table.device)
    check(L.load().ttsk_gather_add(_ptr(x), _ptr(table), _ptr(idx), int(idx.dtype == torch.int64), idx_div, _ptr(pe), pe_mod,
                                   _ptr(out), rows, D, _stream()), "ttsk_gather_add")
    return out


def gather_add_lens(x, table, idx, lens, seg_len, out=None):
    """out[u*seg_len + l] = x[..] + table[idx[u]] for l < lens[u], a zero row past it; x bf16 (rows, D), idx / lens (B,) int64."""
    _dev(x, table, idx, lens)
    if idx.dtype != torch.int64 or lens.dtype != torch.int64:
        raise L.TtskError("gather_add_lens: idx and lens must be int64")
    rows, D = x.shape
    Bn = rows // max(int(seg_len), 1)
    if seg_len <= 0 or Bn * seg_len != rows or idx.numel() != Bn or lens.numel() != Bn or not (x.is_contiguous() and idx.is_contiguous() and lens.is_contiguous()):
        raise L.TtskError("gather_add_lens: %d rows of seg_len %d need contiguous idx and lens of %d entries, got %d and %d"
                          % (rows, seg_len, Bn, idx.numel(), lens.numel()))
    if out is None:
        out = torch.empty(rows, D, dtype=bf16, device=x.device)
    check(L.load().ttsk_gather_add_lens(_ptr(x), _ptr(table), _ptr(idx), _ptr(lens), seg_len, _ptr(out), rows, D, _stream()),
          "ttsk_gather_add_lens")
    return out


def embed_step(pred, control, bins, table, x, lens, seg_len):
    """The free-running embedding step in one launch: scaled = pred * control[u], idx = bucketize(scaled, bins), x_out = x + table[idx]
    with zero rows past lens[u].  pred (B, L) fp32, control (B,) fp32, x bf16 (B * L, D), lens (B,) int64 -> (x_out, scaled, idx)."""
    _dev(pred, control, bins, table, x, lens)
    if lens.dtype != torch.int64 or control.dtype != torch.float32 or pred.dtype != torch.float32:
        raise L.TtskError("embed_step: pred / control must be fp32, lens int64")
    pred = pred.contiguous()
    rows, D = x.shape
    Bn = rows // max(int(seg_len), 1)
    if seg_len <= 0 or Bn * seg_len != rows or pred.numel() != rows or control.numel() != Bn or lens.numel() != Bn or table.shape[0] <= bins.numel() \
            or not (x.is_contiguous() and control.is_contiguous() and lens.is_contiguous()):
        raise L.TtskError("embed_step: %d rows of seg_len %d need %d predictions, contiguous control and lens of %d entries and a table of more than "
                          "%d rows; got %d, %d, %d, %d" % (rows, seg_len, rows, Bn, bins.numel(), pred.numel(), control.numel(), lens.numel(), table.shape[0]))
    out = torch.empty(rows, D, dtype=bf16, device=x.device)
    scaled = torch.empty_like(pred)
    idx = torch.empty(pred.shape, dtype=torch.int32, device=x.device)
    check(L.load().ttsk_embed_step(_ptr(pred), _ptr(control), _ptr(bins), bins.numel(), _ptr(table), _ptr(x), _ptr(lens), seg_len,
                                   _ptr(out), _ptr(scaled), _ptr(idx), rows, D, _stream()), "ttsk_embed_step")
    return out, scaled, idx


def _rows_like(name, ref, **arrays):
    """Per-row inputs of the per-phoneme kernels: contiguous, on the device, `ref.numel()` entries, fp32 (uint8 for the `has` flags)."""
    for key, (a, dt) in arrays.items():
        if a.dtype != dt or a.numel() != ref.numel() or not a.is_contiguous():
            raise L.TtskError("%s: %s must be contiguous %s with %d entries (one per row), got %s %s"
                              % (name, key, dt, ref.numel(), a.dtype, tuple(a.shape)))


def embed_step_rows(pred, control, value, has, bins, table, x, lens, seg_len):
    """`embed_step` with one control per row and an optional explicit value per row: scaled = value where has else pred * control.
    pred / control / value (B, L) fp32, has (B, L) uint8, x bf16 (B * L, D), lens (B,) int64 -> (x_out, scaled, idx)."""
    _dev(pred, control, value, has, bins, table, x, lens)
    if lens.dtype != torch.int64 or pred.dtype != torch.float32:
        raise L.TtskError("embed_step_rows: pred must be fp32, lens int64")
    pred = pred.contiguous()
    rows, D = x.shape
    Bn = rows // max(int(seg_len), 1)
    if seg_len <= 0 or Bn * seg_len != rows or pred.numel() != rows or lens.numel() != Bn or table.shape[0] <= bins.numel() \
            or not (x.is_contiguous() and lens.is_contiguous()):
        raise L.TtskError("embed_step_rows: %d rows of seg_len %d need %d predictions, contiguous lens of %d entries and a table of more than "
                          "%d rows; got %d, %d, %d" % (rows, seg_len, rows, Bn, bins.numel(), pred.numel(), lens.numel(), table.shape[0]))
    _rows_like("embed_step_rows", pred, control=(control, torch.float32), value=(value, torch.float32), has=(has, torch.uint8))
    out = torch.empty(rows, D, dtype=bf16, device=x.device)
    scaled = torch.empty_like(pred)
    idx = torch.empty(pred.shape, dtype=torch.int32, device=x.device)
    check(L.load().ttsk_embed_step_rows(_ptr(pred), _ptr(control), _ptr(value), _ptr(has), _ptr(bins), bins.numel(), _ptr(table), _ptr(x),
                                        _ptr(lens), seg_len, _ptr(out), _ptr(scaled), _ptr(idx), rows, D, _stream()), "ttsk_embed_step_rows")
    return out, scaled, idx


def duration_rows(logd, d_control, durations, has):
    """v = durations where has else max(rint(exp(logd) - 1) * d_control, 0): logd / d_control / durations (B, L) fp32, has uint8."""
    _dev(logd, d_control, durations, has)
    if logd.dtype != torch.float32 or logd.dim() != 2 or not logd.is_contiguous():
        raise L.TtskError("duration_rows: needs contiguous fp32 logd (B, L), got %s %s" % (logd.dtype, tuple(logd.shape)))
    _rows_like("duration_rows", logd, d_control=(d_control, torch.float32), durations=(durations, torch.float32), has=(has, torch.uint8))
    out = torch.empty_like(logd)
    check(L.load().ttsk_duration_rows(_ptr(logd), _ptr(d_control), _ptr(durations), _ptr(has), _ptr(out), logd.numel(), _stream()),
          "ttsk_duration_rows")
    return out


FIT_MAX_L = 1024     # duration_fit: one workgroup per utterance keeps the fractional parts in LDS


def duration_fit(v, has, target, lens):
    """Fit each utterance's durations to its frame budget (include/ttsk.h): v (B, L) fp32, has (B, L) uint8 (the
    fixed phonemes), target (B,) int32 (< 0: none, the row is copied), lens (B,) int64 -> (B, L) fp32 whole frame counts."""
    _dev(v, has, target, lens)
    if v.dtype != torch.float32 or v.dim() != 2 or not v.is_contiguous() or not 0 < v.shape[1] <= FIT_MAX_L:
        raise L.TtskError("duration_fit: needs contiguous fp32 v (B, L) with L <= %d, got %s %s" % (FIT_MAX_L, v.dtype, tuple(v.shape)))
    _rows_like("duration_fit", v, has=(has, torch.uint8))
    Bn = v.shape[0]
    if target.dtype != torch.int32 or lens.dtype != torch.int64 or target.numel() != Bn or lens.numel() != Bn \
            or not (target.is_contiguous() and lens.is_contiguous()):
        raise L.TtskError("duration_fit: target must be int32 and lens int64, contiguous with %d entries; got %s (%d) and %s (%d)"
                          % (Bn, target.dtype, target.numel(), lens.dtype, lens.numel()))
    out = torch.empty_like(v)
    check(L.load().ttsk_duration_fit(_ptr(v), _ptr(has), _ptr(target), _ptr(lens), v.shape[1], _ptr(out), Bn, _stream()), "ttsk_duration_fit")
    return out


def scatter_sum(dx, idx, dtable, idx_div=1, skip_row=-1, accumulate=True, defer=None):
    """dtable[v] (+)= sum of the rows of dx whose index is v.  `defer` (the list flush_finalize drains): the embedding-table
    gradients of a backward pass are independent and nothing but the optimiser reads them — queued, they share one launch."""
    _dev(dx, idx, dtable)
    V, D = dtable.shape
    if defer is not None:
        it = L.ScatterItem()
        it.dx, it.idx, it.dtable = dx.data_ptr(), idx.data_ptr(), dtable.data_ptr()
        it.idx_is_i64, it.idx_div, it.n_idx, it.n_table_rows, it.D = int(idx.dtype == torch.int64), idx_div, idx.numel(), V, D
        it.skip_row, it.accumulate = skip_row, int(accumulate)
        defer.append((it, (dx, idx)))
        return dtable
    check(L.load().ttsk_scatter_sum(_ptr(dx), _ptr(idx), int(idx.dtype == torch.int64), idx_div, idx.numel(), _ptr(dtable), V, D,
                                    skip_row, int(accumulate), _stream()), "ttsk_scatter_sum")
    return dtable


def cast_bf16(src, dst=None):
    _dev(src)
    if dst is None:
        dst = torch.empty(src.shape, dtype=bf16, device=src.device)
    check(L.load().ttsk_cast_bf16(_ptr(src), _ptr(dst), src.numel(), _stream()), "ttsk_cast_bf16")
    return dst


def nct_to_ntc(x, dtype=bf16):
    """(B,C,T) fp32 contiguous -> (B,T,C) bf16 / fp16."""
    _dev(x)
    B, Cn, T = x.shape
    out = torch.empty(B, T, Cn, dtype=dtype, device=x.device)
    check(L.load().ttsk_nct_to_ntc(_ptr(x.contiguous()), _ptr(out), int(dtype == f16), B, Cn, T, _stream()), "ttsk_nct_to_ntc")
    return out


def to_int16(x, scale):
    _dev(x)
    out = torch.empty(x.shape, dtype=torch.int16, device=x.device)
    check(L.load().ttsk_to_int16(_ptr(x.contiguous()), _ptr(out), x.numel(), scale, _stream()), "ttsk_to_int16")
    return out


def mel_windows(stage, plan, W, dtype=f16, frames_first=False, C=80):
    """The windows of a call, gathered from the mel staging buffer by the device-resident plan (tts_king_amd/windows.py): `stage` fp32,
    contiguous, holding the utterances back to back as (C, frames) rows (the reference's mel layout) or, `frames_first`, as FastSpeech2's
    (frames, C) rows -> (N, W, C) 16-bit channels-last, bit for bit `nct_to_ntc` of the sliced windows.  Padding windows read zeros."""
    _dev(stage, plan)
    if stage.dtype != torch.float32 or not stage.is_contiguous() or plan.dtype != torch.int32 or not plan.is_contiguous():
        raise L.TtskError("mel_windows: needs a contiguous fp32 staging buffer and a contiguous int32 plan")
    N, frames = plan.shape[0], stage.numel() // C
    out = torch.empty(N, W, C, dtype=dtype, device=stage.device)
    st, sc = (C, 1) if frames_first else (1, frames)
    check(L.load().ttsk_mel_windows(_ptr(stage), st, sc, frames, _ptr(plan), _ptr(out), int(dtype == f16), N, W, C, _stream()), "ttsk_mel_windows")
    return out


def wav_stitch(y, plan, W, out=None, int16_scale=None):
    """y (N, 1, spf * W) fp32 window waveforms -> the kept samples of every window, utterances back to back, in one flat buffer of
    N * W * spf samples (what the plan can fill at most; the tail past the call's frames is not written): fp32, or int16 with
    `to_int16`'s arithmetic when `int16_scale` is given."""
    _dev(y, plan)
    N = plan.shape[0]
    spf = y.shape[-1] // W
    if y.dtype != torch.float32 or not y.is_contiguous() or y.numel() != N * W * spf or plan.dtype != torch.int32 or not plan.is_contiguous():
        raise L.TtskError("wav_stitch: needs contiguous fp32 (N, 1, spf * W) window waveforms and a contiguous int32 plan of N rows")
    i16 = int16_scale is not None
    if out is None:
        out = torch.empty(N * W * spf, dtype=torch.int16 if i16 else torch.float32, device=y.device)
    check(L.load().ttsk_wav_stitch(_ptr(y), _ptr(plan), _ptr(out), out.numel() // spf, int(i16), float(int16_scale or 0.0), N, W, spf, _stream()),
          "ttsk_wav_stitch")
    return out


def resample(x_flat, segs, filt, out=None, int16_scale=None):
    """x_flat: contiguous fp32 utterances back to back (what `wav_stitch` writes); segs: (rows, 4) int32 device table {src_off, src_len,
    dst_off, dst_len} (tts_king_amd/resample.py); filt: a `resample.Filter` on the same device (table (P, L)) -> every utterance resampled by
    filt.L / filt.M at its dst_off in `out`: fp32, or int16 = clamp(y * int16_scale, -32768, 32767) truncated toward zero.  Without
    `out` the buffer is sized to the end of the last segment, which costs a host read of the table: a capturable call passes `out`.
    Samples of `out` that belong to no segment are not written."""
    _dev(x_flat, segs, filt.table)
    if (x_flat.dtype != torch.float32 or not x_flat.is_contiguous() or segs.dtype != torch.int32 or not segs.is_contiguous() or segs.dim() != 2 or
            segs.shape[1] != 4 or filt.table.dtype != torch.float32 or not filt.table.is_contiguous() or filt.table.numel() != filt.L * filt.P):
        raise L.TtskError("resample: needs a contiguous fp32 source, a contiguous (rows, 4) int32 segment table and a (P, L) fp32 filter table")
    i16 = int16_scale is not None
    dt = torch.int16 if i16 else torch.float32
    if out is None:
        s = segs.cpu()
        out = torch.empty(int((s[:, 2].long() + s[:, 3].long()).max()) if s.shape[0] else 0, dtype=dt, device=x_flat.device)
    elif out.dtype != dt or not out.is_contiguous() or not out.is_cuda:
        raise L.TtskError("resample: `out` must be a contiguous %s device tensor" % dt)
    _count("resample")
    check(L.load().ttsk_resample(_ptr(x_flat), x_flat.numel(), _ptr(segs), segs.shape[0], _ptr(filt.table), filt.L, filt.M, filt.P, filt.C,
                                 _ptr(out), out.numel(), int(i16), float(int16_scale or 0.0), _stream()), "ttsk_resample")
    return out


def _join_args(what, x_flat, join, info):
    """The checks `wav_join_stats` and `wav_join` share; returns (U, info), `info` allocated when None."""
    from .narrate import MAX_ROWS, ROW
    _dev(x_flat, join, info)
    if (x_flat.dtype != torch.float32 or not x_flat.is_contiguous() or x_flat.dim() != 1 or join.dtype != torch.int32 or not join.is_contiguous() or
            join.dim() != 2 or join.shape[1] != ROW or join.shape[0] < 2):
        raise L.TtskError("%s: needs a contiguous flat fp32 source and a contiguous (1 + rows, %d) int32 join table (narrate.join_table)" % (what, ROW))
    U = join.shape[0] - 1
    if U > MAX_ROWS or not 0 < x_flat.numel() < 2 ** 31:
        raise L.TtskError("%s: %d rows (at most %d) over a source of %d samples (1 .. 2^31 - 1)" % (what, U, MAX_ROWS, x_flat.numel()))
    if info is None:
        info = torch.empty(U + 1, ROW, dtype=torch.int32, device=x_flat.device)
    elif info.dtype != torch.int32 or not info.is_contiguous() or tuple(info.shape) != (U + 1, ROW):
        raise L.TtskError("%s: `info` must be a contiguous (%d, %d) int32 device tensor" % (what, U + 1, ROW))
    return U, info


def wav_join_stats(x_flat, join, info=None):
    """The statistics launch of `wav_join` alone: x_flat contiguous fp32 (utterances wherever `join` puts them), join the (1 + U, 8)
    int32 device table of tts_king_amd/narrate.py (`join_table`: row 0 the settings, then one row per utterance) -> `info`, (U + 1, 8)
    int32 on the device with every row's kept range [a, b), peak, sum of squares and gain (include/ttsk.h; `narrate.read_info`
    decodes a host copy).  The layout columns (o_u, total) are written by `wav_join`."""
    U, info = _join_args("wav_join_stats", x_flat, join, info)
    _count("wav_join_stats")
    check(L.load().ttsk_wav_join_stats(_ptr(x_flat), x_flat.numel(), _ptr(join), U, _ptr(info), _stream()), "ttsk_wav_join_stats")
    return info


def wav_join(x_flat, join, n_dst=None, out=None, info=None, int16_scale=None):
    """The U utterances of `x_flat` that the join table names, trimmed, levelled, faded and laid out behind each other with their pauses
    as ONE waveform (two launches, no host synchronisation; tts_king_amd/narrate.py) -> (out, info): `out` a flat
    buffer of `n_dst` samples (or the `out` given), EVERY sample written, zeros from the waveform's end (`info[U, 0]`) on: fp32, or
    int16 = clamp(y * int16_scale, -32768, 32767) truncated toward zero; `info` as in `wav_join_stats` plus every row's first output
    sample and the total.  `n_dst` is the caller's bound (`narrate.out_bound`): samples past it are dropped."""
    U, info = _join_args("wav_join", x_flat, join, info)
    i16 = int16_scale is not None
    dt = torch.int16 if i16 else torch.float32
    if out is None:
        if n_dst is None or not 0 < int(n_dst) < 2 ** 31:
            raise L.TtskError("wav_join: needs `out` or its size n_dst (1 .. 2^31 - 1), got %r" % (n_dst,))
        out = torch.empty(int(n_dst), dtype=dt, device=x_flat.device)
    elif out.dtype != dt or not out.is_contiguous() or not out.is_cuda or not 0 < out.numel() < 2 ** 31:
        raise L.TtskError("wav_join: `out` must be a contiguous %s device tensor of 1 .. 2^31 - 1 samples" % dt)
    wav_join_stats(x_flat, join, info)
    _count("wav_join")
    check(L.load().ttsk_wav_join(_ptr(x_flat), x_flat.numel(), _ptr(join), U, _ptr(info), _ptr(out), out.numel(), int(i16),
                                 float(int16_scale or 0.0), _stream()), "ttsk_wav_join")
    return out, info


def collate_batch(table, n_fields, idx_dev, idx_host, n_utts, out, fl_off=-1, t_true=0, pl_off=-1, l_true=0):
    """One packed training batch gathered from a device-resident set (tts_king_amd/resident.py): `table` = a `lib.CollateField` array of
    `n_fields` rows (include/ttsk.h: where each field's flat array and per-utterance offset / length tables live, and where the field
    goes in `out`); idx_dev: contiguous int32 device tensor of the batch's utterance numbers, idx_host: the same as a contiguous int32
    numpy array (checked on the host together with the fields' host-side lengths: an index outside the store or a row longer than
    its padded length is refused, nothing is launched); out: contiguous uint8 device buffer with the feeder's layout, every byte of
    which is written.  fl_off / pl_off >= 0: the int32 frame limit `t_true` / the B int64 phoneme limits `l_true` at those bytes."""
    _dev(idx_dev, out)
    B = idx_dev.numel()
    if (idx_dev.dtype != torch.int32 or not idx_dev.is_contiguous() or out.dtype != torch.uint8 or not out.is_contiguous() or
            idx_host.dtype.str != "<i4" or not idx_host.flags["C_CONTIGUOUS"] or idx_host.size != B):
        raise L.TtskError("collate_batch: needs contiguous int32 indices (device tensor and numpy array of the same %d entries) and a "
                          "contiguous uint8 batch buffer" % B)
    _count("collate_batch")
    check(L.load().ttsk_collate_batch(table, n_fields, _ptr(idx_dev), idx_host.ctypes.data, B, int(n_utts), _ptr(out), out.numel(), int(fl_off),
                                      int(t_true), int(pl_off), int(l_true), _stream()), "ttsk_collate_batch")
    return out


def resample_tile(filt):
    """Samples of the destination one workgroup of `resample` serves for this filter (host only; segments need no alignment to it)."""
    return int(L.load().ttsk_resample_tile(filt.L, filt.M, filt.P))


def _row_args(what, rows, Bn):
    """(pointer, element stride, samples per frame) of a per-row length for the *_rowlen entry points (include/ttsk.h): `rows` =
    (frames, spf) with `frames` a 1-D int32 device tensor or view of Bn entries (column `windows.VALID` of a plan table, or a compact
    copy) or None (every row full).  The kernels clamp the VALUES; the extent is checked here."""
    frames, spf = rows
    if int(spf) <= 0:
        raise L.TtskError("%s: %d samples per frame" % (what, spf))
    if frames is None:
        return None, 1, int(spf)
    _dev(frames)
    if frames.dtype != torch.int32 or frames.dim() != 1 or frames.numel() != Bn or (Bn > 1 and frames.stride(0) <= 0):
        raise L.TtskError("%s: %d rows need a 1-D int32 length tensor of %d entries, got %s %s" % (what, Bn, Bn, frames.dtype, tuple(frames.shape)))
    return frames.data_ptr(), (int(frames.stride(0)) if Bn > 1 else 1), int(spf)


def zero_rows_past(x, rows):
    """x (B, len, C) 16-bit, in place: the positions of row b from frames[b] * spf on := 0 (`rows` as for `_row_args`)."""
    _dev(x)
    Bn, ln, Cn = x.shape
    if not x.is_contiguous():
        raise L.TtskError("zero_rows_past: needs a contiguous (B, len, C) tensor")
    rp, rs, spf = _row_args("zero_rows_past", rows, Bn)
    check(L.load().ttsk_zero_rows_past(_ptr(x), Bn, ln, Cn, rp, rs, spf, _stream()), "ttsk_zero_rows_past")
    return x


_PINNED = {}
_PINNED_LOCK = threading.Lock()


def to_host(t):
    """A device tensor on the host, through a pinned staging buffer kept per (device, shape, dtype) — at most eight of them: the pageable
    `.cpu()` of a waveform (0.2 MB for one utterance, 1.5 MB for a batch of eight) goes through the driver's own staging and takes 0.1-0.3 ms,
    a third to a seventh of that from pinned memory.  The caller gets its own copy (the staging buffer is reused by the next call).  The copy
    runs on the current stream of the TENSOR's device and that stream is the one waited for (not the current device's: `HIFIapi(device=
    "cuda:1")`); lookup, copy and clone happen under one lock, so two threads with same-shaped outputs cannot read each other's samples."""
    _dev(t)
    key = (t.device.index, tuple(t.shape), t.dtype)
    with _PINNED_LOCK:
        buf = _PINNED.get(key)
        if buf is None:
            if len(_PINNED) >= 8:
                _PINNED.pop(next(iter(_PINNED)))
            buf = _PINNED[key] = torch.empty(t.shape, dtype=t.dtype).pin_memory()
        with torch.cuda.device(t.device):
            buf.copy_(t, non_blocking=True)
            torch.cuda.current_stream(t.device).synchronize()
        return buf.clone()


# ---------------------------------------------------------------------------------------------------- batch norm

def _lim(frame_limit):
    """(pointer, seg_len) of a frame limit (None, or (int32[1] device tensor, frames per utterance in the row layout))."""
    return (None, 0) if frame_limit is None else (frame_limit[0].data_ptr(), int(frame_limit[1]))


def zero_frames_from(x, frame_limit):
    """x (rows, C) bf16/fp32, rows = utterances * seg_len: frames t >= frame_limit of every utterance := 0."""
    _dev(x)
    lp, seg = _lim(frame_limit)
    rows, Cn = x.shape
    check(L.load().ttsk_zero_frames_from(_ptr(x), x.element_size(), rows, Cn, seg, lp, _stream()), "ttsk_zero_frames_from")
    return x


def _check_lens(what, lens, rows, seg_len):
    """The kernels clamp the VALUES of a per-utterance limit; its extent (one int64 per utterance) is checked here."""
    if seg_len <= 0 or rows % seg_len or lens.dtype != torch.int64 or not lens.is_contiguous() or lens.numel() != rows // seg_len:
        raise L.TtskError("%s: %d rows of seg_len %d need a contiguous int64 lens of %d entries, got %s %s"
                          % (what, rows, seg_len, rows // max(seg_len, 1), lens.dtype, tuple(lens.shape)))


def zero_frames_lens(x, lens, seg_len):
    """x (rows, C) bf16/fp32, rows = utterances * seg_len: frames t >= lens[u] of utterance u := 0 (lens (B,) int64)."""
    _dev(x, lens)
    rows, Cn = x.shape
    _check_lens("zero_frames_lens", lens, rows, seg_len)
    check(L.load().ttsk_zero_frames_lens(_ptr(x), x.element_size(), rows, Cn, seg_len, _ptr(lens), _stream()), "ttsk_zero_frames_lens")
    return x


BN_SLAB = True      # two-launch BatchNorm (channel slabs) where the channel count allows; the three-launch kernels serve the rest and inference


def bn_train_stats(x, running_mean=None, running_var=None, nbt=None, eps=1e-5, momentum=0.1, frame_limit=None):
    """x (rows, C) bf16 or fp32 -> (mean, rstd) fp32 of the batch; updates the running buffers in place."""
    _dev(x)
    rows, Cn = x.shape
    lib = L.load()
    nblk = lib.ttsk_bn_nblocks(rows)
    partials = _f32(nblk, 2 * Cn, device=x.device)
    mean, rstd = _f32(Cn, device=x.device), _f32(Cn, device=x.device)
    lp, seg = _lim(frame_limit)
    check(lib.ttsk_bn_stats(_ptr(x), int(x.dtype == torch.float32), rows, Cn, _ptr(partials), lp, seg, _stream()), "ttsk_bn_stats")
    check(lib.ttsk_bn_finalize(_ptr(partials), nblk, Cn, rows, eps, momentum, _ptr(mean), _ptr(rstd), _ptr(running_mean),
                               _ptr(running_var), _ptr(nbt), lp, seg, _stream()), "ttsk_bn_finalize")
    return mean, rstd


def rsqrt_eps(var, eps=1e-5):
    out = torch.empty_like(var)
    check(L.load().ttsk_rsqrt_eps(_ptr(var), eps, _ptr(out), var.numel(), _stream()), "ttsk_rsqrt_eps")
    return out


def bn_apply(x, mean, rstd, gamma, beta, use_tanh, p=0.0, site=0, rng=None, resid=None, out_f32=False, frame_limit=None):
    rows, Cn = x.shape
    o16 = None if out_f32 else torch.empty(rows, Cn, dtype=bf16, device=x.device)
    o32 = _f32(rows, Cn, device=x.device) if out_f32 else None
    check(L.load().ttsk_bn_apply(_ptr(x), int(x.dtype == torch.float32), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), rows, Cn, int(use_tanh), p, site,
                                 _ptr(rng), _ptr(resid), _ptr(o16), _ptr(o32), *_lim(frame_limit), _stream()), "ttsk_bn_apply")
    return o32 if out_f32 else o16


def bn_apply_lens(x, mean, rstd, gamma, beta, use_tanh, lens, seg_len, resid=None, out_f32=False):
    """Inference `bn_apply` whose frames t >= lens[u] come out as zero rows (lens (B,) int64, rows = B * seg_len)."""
    _dev(x, lens)
    rows, Cn = x.shape
    _check_lens("bn_apply_lens", lens, rows, seg_len)
    o16 = None if out_f32 else torch.empty(rows, Cn, dtype=bf16, device=x.device)
    o32 = _f32(rows, Cn, device=x.device) if out_f32 else None
    check(L.load().ttsk_bn_apply_lens(_ptr(x), int(x.dtype == torch.float32), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), rows, Cn,
                                      int(use_tanh), _ptr(resid), _ptr(o16), _ptr(o32), _ptr(lens), seg_len, _stream()), "ttsk_bn_apply_lens")
    return o32 if out_f32 else o16


def bn_slab_supported(Cn):
    return BN_SLAB and Cn % 4 == 0 and (Cn % 64 == 0 or Cn <= 128)


@_family("batchnorm", lambda *a, **kw: 0.0)
def bn_train(x, running_mean, running_var, nbt, gamma, beta, use_tanh, p=0.0, site=0, rng=None, resid=None, out_f32=False,
             frame_limit=None, eps=1e-5, momentum=0.1, partials=None, want_keep=False):
    """Training-mode BatchNorm forward in two launches: batch statistics partials, then normalise (+tanh, dropout, residual)
    with mean / rstd finished per channel slab inside the second kernel.  -> (out, mean, rstd).  partials: rows already
    produced elsewhere ([nblk][2C] fp32) skip the first launch.  want_keep: -> (out, mean, rstd, keep), keep = the dropout's
    keep bits (uint8 [rows][C/4], None when p == 0) for bn_bwd(keep=...)."""
    _dev(x)
    rows, Cn = x.shape
    lib = L.load()
    lp, seg = _lim(frame_limit)
    xf = int(x.dtype == torch.float32)
    if partials is None:
        partials = _f32(lib.ttsk_bn_nchunks(rows), 2 * Cn, device=x.device)
        check(lib.ttsk_bn_stats_slab(_ptr(x), xf, rows, Cn, _ptr(partials), lp, seg, _stream()), "ttsk_bn_stats_slab")
    mean, rstd = _f32(Cn, device=x.device), _f32(Cn, device=x.device)
    o16 = None if out_f32 else torch.empty(rows, Cn, dtype=bf16, device=x.device)
    o32 = _f32(rows, Cn, device=x.device) if out_f32 else None
    keep = torch.empty(rows, Cn // 4, dtype=torch.uint8, device=x.device) if (want_keep and p > 0.0) else None
    check(lib.ttsk_bn_train_apply(_ptr(x), xf, _ptr(partials), partials.shape[0], eps, momentum, _ptr(mean), _ptr(rstd), _ptr(running_mean),
                                  _ptr(running_var), _ptr(nbt), _ptr(gamma), _ptr(beta), rows, Cn, int(use_tanh), p, site, _ptr(rng),
                                  _ptr(resid), _ptr(o16), _ptr(o32), _ptr(keep), lp, seg, _stream()), "ttsk_bn_train_apply")
    return ((o32 if out_f32 else o16), mean, rstd, keep) if want_keep else ((o32 if out_f32 else o16), mean, rstd)


@_family("batchnorm", lambda *a, **kw: 0.0)
def bn_bwd(dout, x, mean, rstd, gamma, beta, use_tanh, p=0.0, site=0, rng=None, dgamma=None, dbeta=None, frame_limit=None, keep=None,
           accumulate=True, partials=None):
    """dx (rows,C) bf16; dgamma/dbeta (fp32, accumulated in place when given, or overwritten with accumulate=False).  keep: bn_train's
    keep bits (slab kernels only).  partials: the statistics partial rows when the conv that produced `dout` emitted them (win_conv_bnb)."""
    rows, Cn = x.shape
    lib = L.load()
    if bn_slab_supported(Cn):
        f32, xf = int(dout.dtype == torch.float32), int(x.dtype == torch.float32)
        lp, seg = _lim(frame_limit)
        if partials is None:
            partials = _f32(lib.ttsk_bn_nchunks(rows), 2 * Cn, device=x.device)
            check(lib.ttsk_bn_bwd_stats_slab(_ptr(dout), f32, _ptr(x), xf, _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), rows, Cn, int(use_tanh),
                                             p, site, _ptr(rng), _ptr(keep), _ptr(partials), lp, seg, _stream()), "ttsk_bn_bwd_stats_slab")
        dx = torch.empty(rows, Cn, dtype=bf16, device=x.device)
        check(lib.ttsk_bn_bwd_apply_slab(_ptr(dout), f32, _ptr(x), xf, _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), rows, Cn, int(use_tanh),
                                         p, site, _ptr(rng), _ptr(keep), _ptr(partials), partials.shape[0], _ptr(dx), _ptr(dgamma), _ptr(dbeta), int(accumulate),
                                         lp, seg, _stream()), "ttsk_bn_bwd_apply_slab")
        return dx
    nblk = lib.ttsk_bn_nblocks(rows)
    partials = _f32(nblk, 2 * Cn, device=x.device)
    sums = _f32(2 * Cn, device=x.device)
    f32 = int(dout.dtype == torch.float32)
    check(lib.ttsk_bn_bwd_stats(_ptr(dout), f32, _ptr(x), int(x.dtype == torch.float32), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), rows, Cn,
                                int(use_tanh), p, site, _ptr(rng), _ptr(partials), *_lim(frame_limit), _stream()), "ttsk_bn_bwd_stats")
    colsum_finalize(partials, nblk, 2 * Cn, 2 * Cn, sums, accumulate=False)
    dx = torch.empty(rows, Cn, dtype=bf16, device=x.device)
    check(lib.ttsk_bn_bwd_apply(_ptr(dout), f32, _ptr(x), int(x.dtype == torch.float32), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), rows, Cn,
                                int(use_tanh), p, site, _ptr(rng), _ptr(sums), _ptr(dx), _ptr(dgamma), _ptr(dbeta), int(accumulate), *_lim(frame_limit),
                                _stream()), "ttsk_bn_bwd_apply")
    return dx


# ---------------------------------------------------------------------------------------------------- loss / optimiser

def fs2_loss(mel, post, mel_t, mel_lens, pitch, energy, logd, pitch_t, energy_t, dur_t, src_lens, grad_scale=1.0, frame_limit=None):
    """Returns (losses[8] fp32 device, dmel_sum, dpost, dpitch, denergy, dlogd).  See include/ttsk.h."""
    _dev(mel, post, mel_t, mel_lens, pitch, energy, logd, pitch_t, energy_t, dur_t, src_lens)
    B, T, nm = mel.shape
    Tt = mel_t.shape[1]
    Lp = pitch.shape[1]
    dev = mel.device
    lib = L.load()
    dmel, dpost = _f32(B, T, nm, device=dev), _f32(B, T, nm, device=dev)
    dstack = _f32(3, B, Lp, device=dev)          # (duration, pitch, energy): the order of the grouped predictor backward
    dd, dp, de = dstack[0], dstack[1], dstack[2]
    partials = _f32(lib.ttsk_fs2_loss_nblocks(), 6, device=dev)
    losses = _f32(8, device=dev)
    check(lib.ttsk_fs2_loss(_ptr(mel), _ptr(post), _ptr(mel_t), _ptr(mel_lens), _ptr(pitch), _ptr(energy), _ptr(logd),
                            _ptr(pitch_t), _ptr(energy_t), _ptr(dur_t), _ptr(src_lens), B, T, Tt, nm, Lp, grad_scale,
                            _ptr(dmel), _ptr(dpost), _ptr(dp), _ptr(de), _ptr(dd), _ptr(partials), _ptr(losses), _lim(frame_limit)[0], _stream()),
          "ttsk_fs2_loss")
    return losses, dmel, dpost, dp, de, dd


def fs2_loss_split(mel, post, mel_t, mel_lens, pitch, energy, logd, pitch_t, energy_t, dur_t, src_lens, side, grad_scale=1.0, frame_limit=None):
    """fs2_loss for a step whose variance predictors ran on stream `side` and nobody has waited for it: the frame-level terms and dmel_sum /
    dpost on the current stream (which does NOT wait for `side`), the phoneme-level terms and dpitch / denergy / dlogd on `side`, right
    behind the predictors (they need nothing of this stream).  The eight loss values come from fs2_loss_finalize, on any stream that has
    waited for both.  Same values, bit for bit, as fs2_loss (include/ttsk.h: ttsk_fs2_loss_mel / _var / _finalize)."""
    _dev(mel, post, mel_t, mel_lens, pitch, energy, logd, pitch_t, energy_t, dur_t, src_lens)
    B, T, nm = mel.shape
    Tt = mel_t.shape[1]
    Lp = pitch.shape[1]
    dev = mel.device
    lib = L.load()
    dmel, dpost = _f32(B, T, nm, device=dev), _f32(B, T, nm, device=dev)
    partials = _f32(lib.ttsk_fs2_loss_nblocks(), 6, device=dev)
    losses = _f32(8, device=dev)
    lim = _lim(frame_limit)[0]
    check(lib.ttsk_fs2_loss_mel(_ptr(mel), _ptr(post), _ptr(mel_t), _ptr(mel_lens), B, T, Tt, nm, grad_scale, _ptr(dmel), _ptr(dpost), _ptr(partials),
                                lim, _stream()), "ttsk_fs2_loss_mel")
    with torch.cuda.stream(side):
        # what `side` writes is allocated under `side`: the allocator hands a stream memory whose earlier users ran on that stream (a buffer of
        # the current stream's pool may still hold a live activation when `side` — far ahead of it — gets here; so it is in a captured step)
        dstack = _f32(3, B, Lp, device=dev)
        dd, dp, de = dstack[0], dstack[1], dstack[2]
        partials_var = _f32(lib.ttsk_fs2_loss_nblocks(), 6, device=dev)
        check(lib.ttsk_fs2_loss_var(_ptr(pitch), _ptr(energy), _ptr(logd), _ptr(pitch_t), _ptr(energy_t), _ptr(dur_t), _ptr(src_lens), B, Lp,
                                    grad_scale, _ptr(dp), _ptr(de), _ptr(dd), _ptr(partials_var), _stream()), "ttsk_fs2_loss_var")
    return losses, dmel, dpost, dp, de, dd, (partials, partials_var, lim, (B, T, nm))


def fs2_loss_finalize(losses, pending, src_lens):
    """The eight loss values of fs2_loss_split, on the current stream — which must have waited for both halves."""
    partials, partials_var, lim, (B, T, nm) = pending
    check(L.load().ttsk_fs2_loss_finalize(_ptr(partials), _ptr(partials_var), _ptr(src_lens), B, T, nm, lim, _ptr(losses), _stream()),
          "ttsk_fs2_loss_finalize")


# ---------------------------------------------------------------------------------------------- CWT pitch branch (csrc/cwt.hip)
CWT_CHANNELS = 11
CNNSCALAR_FLOATS = 456      # one CNNscalar's parameter block (include/ttsk.h: TTSK_CNNSCALAR_FLOATS)
CNNSCALAR_OFFSETS = (0, 256, 264, 296, 328, 344, 352, 384, 416, 448)     # its ten tensors, in state_dict order
_ZEROS = {}                 # (device, B, L) -> a (B, L) fp32 tensor of zeros nobody writes (fs2_loss_cwt), kept so that a step allocates none


def layernorm_head_fwd(y, gamma, beta, lens, seg_len, head_w, head_b, p_post=0.0, site_post=0, rng=None, eps=1e-5):
    """LayerNorm -> dropout -> Linear(256 -> 11) -> PAD mask (the CWT pitch predictor's tail).  y (rows, 256) bf16, head_w (11, 256),
    head_b (11,).  Returns (mean, rstd, head_out (rows, 11) fp32)."""
    _dev(y, gamma, beta, lens, head_w, head_b, rng)
    rows, D = y.shape
    n_out = head_b.numel()
    mean, rstd, ho = _f32(rows, device=y.device), _f32(rows, device=y.device), _f32(rows, n_out, device=y.device)
    check(L.load().ttsk_layernorm_head_fwd(_ptr(y), _ptr(gamma), _ptr(beta), _ptr(lens), seg_len, rows, D, n_out, eps, p_post, site_post,
                                           _ptr(rng), _ptr(head_w), _ptr(head_b), _ptr(mean), _ptr(rstd), _ptr(ho), _stream()),
          "ttsk_layernorm_head_fwd")
    return mean, rstd, ho


def layernorm_head_bwd(dhead, head_w, z, mean, rstd, gamma, beta, lens, seg_len, p_post=0.0, site_post=0, rng=None):
    """Backward of layernorm_head_fwd.  dhead (rows, 11) fp32.  Returns (dz (rows, 256) bf16 — through the ReLU that produced z —,
    partials (nblk, 14 * 256 + 11) = dbias | dgamma | dbeta | dhead_w | dhead_b, nblk)."""
    _dev(dhead, head_w, z, mean, rstd, gamma, beta, lens, rng)
    rows, D = z.shape
    n_out = dhead.shape[-1]
    lib = L.load()
    nblk = lib.ttsk_layernorm_head_bwd_nblocks(rows)
    partials = _f32(nblk, (3 + n_out) * D + n_out, device=z.device)
    dz = torch.empty(rows, D, dtype=bf16, device=z.device)
    check(lib.ttsk_layernorm_head_bwd(_ptr(dhead), _ptr(head_w), _ptr(z), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(lens), seg_len,
                                      rows, D, n_out, p_post, site_post, _ptr(rng), _ptr(dz), _ptr(partials), _stream()),
          "ttsk_layernorm_head_bwd")
    return dz, partials, nblk


def cnnscalar_fwd(x, cwt, params, B, Lp):
    """Both CNNscalar heads in one launch.  x (B * Lp, 256) bf16, cwt (B, Lp, 11) fp32, params: the two heads' parameter blocks
    (2 * CNNSCALAR_FLOATS fp32).  Returns (heads (2, B) fp32 = pitch_mean row, pitch_std row; saved = what cnnscalar_bwd needs)."""
    _dev(x, cwt, params)
    dev = x.device
    rowdot, pooled = _f32(B, 4, Lp, device=dev), _f32(B, 4, 30, device=dev)
    stats, pre, out = _f32(B, 4, 2, device=dev), _f32(B, 2, device=dev), _f32(2, B, device=dev)
    check(L.load().ttsk_cnnscalar_fwd(_ptr(x), _ptr(cwt), _ptr(params), B, Lp, x.shape[-1], _ptr(rowdot), _ptr(pooled), _ptr(stats), _ptr(pre),
                                      _ptr(out), _stream()), "ttsk_cnnscalar_fwd")
    return out, (x, cwt, pooled, stats, pre, rowdot, B, Lp)


def cnnscalar_bwd(dheads, saved, params):
    """dheads (2, B) fp32 -> per-utterance partials (B, 2 * CNNSCALAR_FLOATS) of the 20 parameter gradients (sum them over B with
    colsum_finalize).  No input gradients: the reference detaches both inputs (model/modules.py:118-119)."""
    x, cwt, pooled, stats, pre, rowdot, B, Lp = saved
    _dev(dheads)
    partials = _f32(B, 2 * CNNSCALAR_FLOATS, device=x.device)
    check(L.load().ttsk_cnnscalar_bwd(_ptr(dheads), _ptr(x), _ptr(cwt), _ptr(params), _ptr(pooled), _ptr(stats), _ptr(pre), B, Lp, x.shape[-1],
                                      _ptr(rowdot), _ptr(partials), _stream()), "ttsk_cnnscalar_bwd")
    return partials


def cwt_pitch(cwt, heads, bins, p_control=1.0):
    """inverse_batch_cwt + `* std + mean` + bucketize(pitch * p_control).  cwt (B, L, 11) fp32, heads (2, B).  Returns (pitch (B, L) fp32,
    idx (B, L) int32)."""
    _dev(cwt, heads, bins)
    B, Lp, _ = cwt.shape
    pitch = _f32(B, Lp, device=cwt.device)
    idx = torch.empty(B, Lp, dtype=torch.int32, device=cwt.device)
    check(L.load().ttsk_cwt_pitch(_ptr(cwt), _ptr(heads), _ptr(bins), bins.numel(), p_control, B, Lp, _ptr(pitch), _ptr(idx), _stream()),
          "ttsk_cwt_pitch")
    return pitch, idx


def fs2_loss_cwt(mel, post, mel_t, mel_lens, cwt, heads, energy, logd, cwt_t, mean_t, std_t, energy_t, dur_t, src_lens, grad_scale=1.0,
                 frame_limit=None):
    """The loss of the CWT branch (loss.py:24-134 with use_cwt): ttsk_fs2_loss with a pitch term of exactly zero, then ttsk_fs2_loss_cwt
    behind it on the same stream.  Returns (losses[8] = {total, mel, pitch, energy, duration, mean_pitch, std_pitch, n_valid}, dmel_sum,
    dpost, dcwt (B, L, 11), denergy, dlogd, dheads (2, B))."""
    _dev(cwt, heads, cwt_t, mean_t, std_t)
    B, Lp, _ = cwt.shape
    # the (B, L) pitch slot of the plain loss takes zeros as prediction and as target: its term and its gradient are exactly 0
    zero = _ZEROS.get((cwt.device, B, Lp))
    if zero is None:
        zero = torch.zeros(B, Lp, dtype=torch.float32, device=cwt.device)
        if not torch.cuda.is_current_stream_capturing():       # (memory made inside a capture belongs to that graph: not kept)
            _ZEROS[(cwt.device, B, Lp)] = zero
    losses, dmel, dpost, _, de, dd = fs2_loss(mel, post, mel_t, mel_lens, zero, energy, logd, zero, energy_t, dur_t, src_lens,
                                              grad_scale=grad_scale, frame_limit=frame_limit)
    dcwt, dheads = torch.empty_like(cwt), _f32(2, B, device=cwt.device)
    check(L.load().ttsk_fs2_loss_cwt(_ptr(cwt), _ptr(cwt_t), _ptr(heads), _ptr(mean_t), _ptr(std_t), _ptr(src_lens), B, Lp, grad_scale,
                                     _ptr(dcwt), _ptr(dheads), _ptr(losses), _stream()), "ttsk_fs2_loss_cwt")
    return losses, dmel, dpost, dcwt, de, dd, dheads


def optim_state(device, seed=1234, sched_step=0):
    """Device state block (see include/ttsk.h): int64[8] view; fields set here, advanced by kernels."""
    n = L.load().ttsk_optim_state_bytes() // 8
    st = torch.zeros(n, dtype=torch.int64)
    st[0] = sched_step
    st[2] = seed
    return st.to(device)


def rng_of(state):
    return state[2:4]


def dropout_keep_mask(state, site, n, p):
    """uint8[n] keep-mask of dropout site `site` at the current (seed, step) of the device state block (ttsk_dropout_keep_mask): what
    every kernel of the step draws for that site; element order = row-major over the site's [rows][C] tensor."""
    keep = torch.empty(n, dtype=torch.uint8, device=state.device)
    check(L.load().ttsk_dropout_keep_mask(_ptr(rng_of(state)), int(site), int(n), float(p), _ptr(keep), _stream()), "ttsk_dropout_keep_mask")
    return keep


def rng_advance(state):
    check(L.load().ttsk_rng_advance(_ptr(state), _stream()), "ttsk_rng_advance")


def optim_tables(ranges, items, device):
    """Device tables for optim_step.  ranges: sorted, disjoint [start, end) element ranges of the flat buffers (multiples of 4): what
    the step may touch; [(0, n)] is everything.  items: [(flat offset, (Cs, K, Ds), plain pack tensor or None, transposed pack tensor
    or None)] — the window kernels' packed weights INSIDE the ranges whose packs the Adam launch is to write (may be empty); the rest
    of the ranges becomes the gap ranges.  Returns a dict of the tensors / counts the call needs (the tensors must stay alive and the
    packs where they are), or None when an item does not tile (Cs % 32, Ds % 256), the ranges overlap or an item sticks out of them."""
    ranges = sorted((int(a), int(b)) for a, b in ranges)
    r, acc, pos = [], 0, 0
    for a, b in ranges:
        if a < pos or b <= a or a % 4 or b % 4:
            return None
        r += [a, b, acc]
        acc += (b - a) // 4
        pos = b
    out = {"ranges": torch.tensor(r if r else [0, 0, 0], dtype=torch.int64).to(device), "n_ranges": len(ranges), "range_floats": acc * 4, "end": pos,
           "items": None, "n_items": 0, "n_tiles": 0, "gaps": None, "n_gaps": 0, "gap_floats": 0}
    items = sorted(items, key=lambda it: it[0])
    if not items:
        return out
    arr = (L.AdamItem * len(items))()
    tile0, gaps, ri = 0, [], 0
    cursor = ranges[0][0]
    for i, (off, (Cs, K, Ds), pk, pkt) in enumerate(items):
        if Cs % 32 or Ds % 256 or off % 4:
            return None
        end = off + Cs * K * Ds
        while ri < len(ranges) and ranges[ri][1] <= off:          # the rest of the ranges in front of this item are gaps
            if ranges[ri][1] > cursor:
                gaps.append((cursor, ranges[ri][1]))
            ri += 1
            cursor = ranges[ri][0] if ri < len(ranges) else None
        if ri == len(ranges) or off < cursor or end > ranges[ri][1]:
            return None
        if off > cursor:
            gaps.append((cursor, off))
        cursor = end
        arr[i].off, arr[i].pack, arr[i].pack_t = off, _ptr(pk), _ptr(pkt)
        arr[i].Cs, arr[i].K, arr[i].Ds, arr[i].tile0 = Cs, K, Ds, tile0
        tile0 += K * (Cs // 32) * (Ds // 256)
    while ri < len(ranges):
        if ranges[ri][1] > cursor:
            gaps.append((cursor, ranges[ri][1]))
        ri += 1
        cursor = ranges[ri][0] if ri < len(ranges) else None
    g, gacc = [], 0
    for a, b in gaps:
        g += [a, b, gacc]
        gacc += (b - a) // 4
    if tile0 * 8192 + gacc * 4 != acc * 4:
        return None
    out.update(items=torch.frombuffer(bytearray(bytes(arr)), dtype=torch.int64).clone().to(device), n_items=len(items), n_tiles=tile0,
               gaps=torch.tensor(g if g else [0, 0, 0], dtype=torch.int64).to(device), n_gaps=len(gaps), gap_floats=gacc * 4)
    return out


@_family("clip_adam", lambda *a, **kw: 0.0)
def optim_step(params, grads, m, v, shadow, state, partials, max_norm, beta1, beta2, eps, d_model, warmup, anneal_steps, anneal_rate,
               tables, zero_grad=True, advance_rng=False):
    """The optimizer step over the element ranges of `tables` (optim_tables) only: counters / lr advanced, norm, clip, Adam, bf16 shadow
    and the packs of the tables' items, in two launches (ttsk_optim_step).  Elements outside the ranges are neither read nor written."""
    _dev(params, grads, m, v, shadow, state, partials, tables["ranges"], tables["items"], tables["gaps"])
    n = params.numel()
    if tables["end"] > n or min(grads.numel(), m.numel(), v.numel(), shadow.numel()) < n:
        raise L.TtskError("optim_step: the ranges end at element %d, the buffers hold %d" % (tables["end"], n))
    arr = (C.c_float * 4)(*([float(a) for a in anneal_steps] + [0.0] * (4 - len(anneal_steps))))
    check(L.load().ttsk_optim_step(_ptr(params), _ptr(grads), _ptr(m), _ptr(v), _ptr(shadow), params.numel(), _ptr(state), _ptr(partials),
                                   max_norm, beta1, beta2, eps, int(zero_grad), float(d_model), float(warmup), C.cast(arr, C.c_void_p),
                                   len(anneal_steps), anneal_rate, int(advance_rng), _ptr(tables["ranges"]), tables["n_ranges"],
                                   tables["range_floats"], _ptr(tables["items"]), tables["n_items"], tables["n_tiles"],
                                   _ptr(tables["gaps"]), tables["n_gaps"], tables["gap_floats"], _stream()),
          "ttsk_optim_step")


# ---------------------------------------------------------------------------------------------------- HiFi-GAN helpers

def weight_norm_fold(v, g):
    """w = g * v / ||v|| with the norm over every dim but 0 (reference: hifi/models.py:203-210)."""
    _dev(v, g)
    v = v.contiguous()
    rows = v.shape[0]
    w = torch.empty_like(v)
    check(L.load().ttsk_weight_norm_fold(_ptr(v), _ptr(g.contiguous()), _ptr(w), rows, v.numel() // rows, _stream()),
          "ttsk_weight_norm_fold")
    return w


def pack_conv_weight(w, transposed=False, dtype=bf16):
    """Conv1d (Cout,Cin,k) fp32 -> (Cout,k,Cin) 16-bit, or ConvTranspose1d (Cin,Cout,k) fp32 -> (k,Cout,Cin) 16-bit."""
    _dev(w)
    d0, d1, d2 = w.shape
    shape = (d2, d1, d0) if transposed else (d0, d2, d1)
    out = torch.empty(shape, dtype=dtype, device=w.device)
    check(L.load().ttsk_pack_conv_weight(_ptr(w.contiguous()), _ptr(out), int(dtype == f16), d0, d1, d2, int(transposed), _stream()),
          "ttsk_pack_conv_weight")
    return out


def avg3(a, b, c, scale, out=None, slope=1.0):
    """out = leaky_relu((a + b + c) * scale, slope)  (slope 1.0 = no activation)."""
    _dev(a, b, c)
    if out is None:
        out = torch.empty_like(a)
    check(L.load().ttsk_avg3(_ptr(a), _ptr(b), _ptr(c), _ptr(out), int(a.dtype == f16), a.numel(), scale, slope, _stream()), "ttsk_avg3")
    return out


def hifi_resblock1_supported(C_, K):
    return bool(L.load().ttsk_hifi_resblock1_supported(C_, K))


def pack_resblock_weight(w, dtype=f16):
    """Folded Conv1d weight (C, C, K) fp32 -> MFMA-fragment-major 16-bit pack for ttsk_hifi_resblock1."""
    _dev(w)
    Cn, _, K = w.shape
    out = torch.empty(L.load().ttsk_resblock_pack_elems(Cn, K), dtype=dtype, device=w.device)
    check(L.load().ttsk_pack_resblock_weight(_ptr(w.contiguous()), _ptr(out), int(dtype == f16), Cn, K, _stream()),
          "ttsk_pack_resblock_weight")
    return out


def hifi_resblock1(x, weights, biases, dilations, out, K, mode=0, scale=1.0, slope=0.1, final_slope=1.0, rows=None):
    """Fused ResBlock1 (reference: hifi/models.py:88-95).  x/out (B, len, C) 16-bit; weights: six fragment-major packs
    (pack_resblock_weight) and biases six fp32 (C,) in the order convs1[0], convs2[0], convs1[1], convs2[1], convs1[2],
    convs2[2].  mode 0: out = y, 1: out += y, 2: out = (out + y) * scale; final_slope: LeakyReLU on the stored value.
    rows (`_row_args`): a per-row length beside the batch stride (ttsk_hifi_resblock1_rowlen): nothing is read or stored past a row's end."""
    _dev(x, out, *weights, *biases)
    Bn, ln, Cn = x.shape
    wp = (C.c_void_p * 6)(*[w.data_ptr() for w in weights])
    bp = (C.c_void_p * 6)(*[b.data_ptr() for b in biases])
    dl = (C.c_int32 * 3)(*[int(d) for d in dilations])
    if rows is not None:
        check(L.load().ttsk_hifi_resblock1_rowlen(_ptr(x), _ptr(out), int(x.dtype == f16), C.cast(wp, C.c_void_p), C.cast(bp, C.c_void_p),
                                                C.cast(dl, C.c_void_p), Bn, ln, Cn, K, mode, scale, slope, final_slope,
                                                *_row_args("hifi_resblock1", rows, Bn), _stream()), "ttsk_hifi_resblock1_rowlen")
        return out
    check(L.load().ttsk_hifi_resblock1(_ptr(x), _ptr(out), int(x.dtype == f16), C.cast(wp, C.c_void_p), C.cast(bp, C.c_void_p),
                                       C.cast(dl, C.c_void_p), Bn, ln, Cn, K, mode, scale, slope, final_slope, _stream()),
          "ttsk_hifi_resblock1")
    return out


def hifi_mrf32_post_supported(C_, ks, k_post):
    return len(ks) == 3 and bool(L.load().ttsk_hifi_mrf32_post_supported(C_, int(ks[0]), int(ks[1]), int(ks[2]), int(k_post)))


def hifi_mrf32_post(x, weights, biases, dilations, ks, w_post, b_post, slope=0.1, final_slope=0.01, scale=1.0 / 3.0, stage_out=None, rows=None):
    """The generator's whole last stage in one launch (reference: hifi/models.py:190-199; csrc/mrf32.hip): x (B, len, 32) 16-bit raw
    stage input -> (B, 1, len) fp32 waveform = tanh(conv_post(leaky_relu(mean_j ResBlock1_j(x), 0.01))).  weights / biases: 18 packs /
    (32,) fp32 vectors, block j's six convs at [6 j ..] in hifi_resblock1's order; dilations: three triples; ks: the three kernel sizes;
    w_post (1, 7, 32) tap-major 16-bit.  stage_out (optional, like x): receives the activated average conv_post reads.
    rows (`_row_args`): a per-row length (ttsk_hifi_mrf32_post_rowlen); the samples past a row's end are not written."""
    _dev(x, w_post, b_post, stage_out, *weights, *biases)
    Bn, ln, Cn = x.shape
    assert len(weights) == 18 and len(biases) == 18 and x.is_contiguous()
    wp = (C.c_void_p * 18)(*[w.data_ptr() for w in weights])
    bp = (C.c_void_p * 18)(*[b.data_ptr() for b in biases])
    dl = (C.c_int32 * 9)(*[int(d) for tri in dilations for d in tri])
    out = torch.empty(Bn, 1, ln, dtype=torch.float32, device=x.device)
    if rows is not None:
        check(L.load().ttsk_hifi_mrf32_post_rowlen(_ptr(x), _ptr(out), _ptr(stage_out), int(x.dtype == f16), C.cast(wp, C.c_void_p),
                                                 C.cast(bp, C.c_void_p), C.cast(dl, C.c_void_p), _ptr(w_post), _ptr(b_post), Bn, ln, Cn, int(ks[0]),
                                                 int(ks[1]), int(ks[2]), int(w_post.shape[-2]), slope, final_slope, scale,
                                                 *_row_args("hifi_mrf32_post", rows, Bn), _stream()), "ttsk_hifi_mrf32_post_rowlen")
        return out
    check(L.load().ttsk_hifi_mrf32_post(_ptr(x), _ptr(out), _ptr(stage_out), int(x.dtype == f16), C.cast(wp, C.c_void_p), C.cast(bp, C.c_void_p),
                                        C.cast(dl, C.c_void_p), _ptr(w_post), _ptr(b_post), Bn, ln, Cn, int(ks[0]), int(ks[1]), int(ks[2]),
                                        int(w_post.shape[-2]), slope, final_slope, scale, _stream()), "ttsk_hifi_mrf32_post")
    return out


def hifi_upsample2_supported(Cin, Cout, stride, k):
    return bool(L.load().ttsk_hifi_upsample2_supported(Cin, Cout, stride, k))


def hifi_upsample2(x, Wp, bias):
    """ConvTranspose1d(stride 2, kernel 4, padding 1): x (B, T, Cin) 16-bit, Wp (4, Cout, Cin) -> (B, 2T, Cout)."""
    _dev(x, Wp, bias)
    Bsz, T, Cin = x.shape
    Cout = Wp.shape[1]
    out = torch.empty(Bsz, 2 * T, Cout, dtype=x.dtype, device=x.device)
    check(L.load().ttsk_hifi_upsample2(_ptr(x), _ptr(Wp), _ptr(bias), _ptr(out), int(x.dtype == f16), Bsz, T, Cin, Cout, _stream()),
          "ttsk_hifi_upsample2")
    return out


def hifi_upsample_win_supported(Cin, Cout, stride, k):
    return k == 2 * stride and bool(L.load().ttsk_hifi_upsample_win_supported(Cin, Cout, stride))


def hifi_upsample8_supported(Cin, Cout, stride, k):
    return stride == 8 and hifi_upsample_win_supported(Cin, Cout, stride, k)


def hifi_upsample_win_pack(Wp, bias, stride):
    """Wp (2*stride, Cout, Cin) 16-bit (pack_conv_weight(..., transposed=True) of a ConvTranspose1d weight, padding stride/2) ->
    (fragment-major pack of the (stride*Cout, 2, Cin) pseudo-weight, bias repeated for the phases): output frame stride*t + r =
    x[t] . w[r + h] + (r < h ? x[t - 1] . w[r + h + stride] : x[t + 1] . w[r - h]), h = stride / 2 — include/ttsk.h:ttsk_hifi_upsample_win."""
    _dev(Wp, bias)
    k, Cout, Cin = Wp.shape
    h = stride // 2
    r = torch.arange(stride, device=Wp.device)
    slot0 = Wp[r + h]                                             # (stride, Cout, Cin)
    slot1 = Wp[torch.where(r < h, r + h + stride, r - h)]
    W2 = torch.stack([slot0, slot1], dim=2).reshape(stride * Cout, 2, Cin).contiguous()      # [(r, co)][slot][ci]
    pack = torch.empty(W2.numel(), dtype=Wp.dtype, device=Wp.device)
    win_conv_pack_items([(W2, pack, False)])
    return pack, bias.float().repeat(stride).contiguous()


def hifi_upsample8_pack(Wp, bias):
    return hifi_upsample_win_pack(Wp, bias, 8)


def hifi_upsample_win(x, pack, bias_rep, Cout, stride):
    """ConvTranspose1d(kernel 2*stride, padding stride/2) on the window-conv kernel: x (B, T, Cin) fp16 -> (B, stride*T, Cout)."""
    _dev(x, pack, bias_rep)
    Bsz, T, Cin = x.shape
    out = torch.empty(Bsz, stride * T, Cout, dtype=x.dtype, device=x.device)
    check(L.load().ttsk_hifi_upsample_win(_ptr(x), _ptr(pack), _ptr(bias_rep), _ptr(out), int(x.dtype == f16), Bsz, T, Cin, Cout, stride,
                                          _stream()), "ttsk_hifi_upsample_win")
    return out


def hifi_conv_pre_win_supported(Cin, Cout, k):
    return bool(L.load().ttsk_hifi_conv_pre_win_supported(Cin, Cout, k))


def hifi_conv_pre_win_pack(w16):
    """(Cout, k, 80) fp16 tap-major weight (pack_conv_weight) -> the window kernel's fragment-major pack (contraction padded to 96)."""
    _dev(w16)
    Cout, k, Cin = w16.shape
    pack = torch.empty(win_pack_numel(Cout, k, Cin, False), dtype=w16.dtype, device=w16.device)
    win_conv_pack_items([(w16.contiguous(), pack, False)])
    return pack


def hifi_conv_pre_win(x, pack, bias, Cout, k, slope):
    """lrelu(Conv1d(80 -> Cout, k)(x) + bias, slope) on the window-conv kernel: x (B, T, 80) fp16 -> (B, T, Cout) fp16."""
    _dev(x, pack, bias)
    Bsz, T, Cin = x.shape
    out = torch.empty(Bsz, T, Cout, dtype=x.dtype, device=x.device)
    check(L.load().ttsk_hifi_conv_pre_win(_ptr(x), _ptr(pack), _ptr(bias), _ptr(out), int(x.dtype == f16), Bsz, T, Cin, Cout, k, slope, _stream()),
          "ttsk_hifi_conv_pre_win")
    return out


def hifi_upsample_loop_supported(Cin, Cout, stride, k):
    return k == 2 * stride and bool(L.load().ttsk_hifi_upsample_loop_supported(Cin, Cout, stride))


def hifi_upsample_loop(x, pack, bias_rep, Cout, stride):
    """hifi_upsample_win's operator and operands on the kernel that loops over the channel groups per frame tile (Cin = 256, stride 8)."""
    _dev(x, pack, bias_rep)
    Bsz, T, Cin = x.shape
    out = torch.empty(Bsz, stride * T, Cout, dtype=x.dtype, device=x.device)
    check(L.load().ttsk_hifi_upsample_loop(_ptr(x), _ptr(pack), _ptr(bias_rep), _ptr(out), int(x.dtype == f16), Bsz, T, Cin, Cout, stride,
                                           _stream()), "ttsk_hifi_upsample_loop")
    return out


def hifi_upsample8(x, pack, bias8, Cout):
    return hifi_upsample_win(x, pack, bias8, Cout, 8)


def hifi_conv_post(x, w, bias):
    """tanh(Conv1d(C -> 1, k)(x)): x (B, len, C) 16-bit already activated, w (1, k, C) 16-bit -> (B, 1, len) fp32.
    reference: hifi/models.py:198-199."""
    _dev(x, w, bias)
    Bn, ln, Cn = x.shape
    out = torch.empty(Bn, 1, ln, dtype=torch.float32, device=x.device)
    check(L.load().ttsk_hifi_conv_post(_ptr(x), _ptr(w), _ptr(bias), _ptr(out), int(x.dtype == f16), Bn, ln, Cn, w.shape[1], _stream()),
          "ttsk_hifi_conv_post")
    return out


def hifi_conv_window_supported(Cn, K, dil):
    return bool(L.load().ttsk_hifi_conv_window_supported(Cn, K, dil))


def hifi_conv_pair_supported(Cn, K, dil):
    return bool(L.load().ttsk_hifi_conv_pair_supported(Cn, K, dil))


def hifi_conv_pair_ws_tile(Cn):
    """Frames per tile of ttsk_hifi_conv_pair_ws at Cn channels (csrc/pairws.hip WsGeom::TT)."""
    return 192 if Cn <= 64 else 96


def hifi_conv_pair_ws_supported(Cn, K, dil, ln=0):
    """The weights-stationary pair kernel (csrc/pairws.hip) covers (C, K, dil) and utterances of `ln` frames (32-bit buffer offsets per utterance)."""
    return bool(L.load().ttsk_hifi_conv_pair_ws_supported(Cn, K, dil)) and ln * Cn * 2 < 2 ** 30


def hifi_conv_pair(x, w1_pack, bias1, w2_pack, bias2, K, dilation, slope=0.1, out=None, mode=0, scale=1.0, final_slope=1.0, ws=False, max_wgs=0,
                   rows=None):
    """y = c2(lrelu(c1_{K,dil}(lrelu(x)) + b1)) + b2 + x in one launch (C = 128; hifi/models.py:88-95, one dilation of ResBlock1).
    mode 0: out = y; 1: out += y; 2: out = lrelu((out + y) * scale, final_slope) (the MRF average, :190-197; ttsk_hifi_resblock1's modes).
    ws: the weights-stationary persistent kernel (C = 64, or C = 128 with K = 3; ttsk_hifi_conv_pair_ws, bit-identical).
    rows (`_row_args`): a per-row length beside the batch stride (ttsk_hifi_conv_pair_rowlen / _ws_rowlen): nothing is read or stored past a
    row's end, so an `out` a later kernel reads there must come in zeroed."""
    _dev(x, w1_pack, bias1, w2_pack, bias2, out)
    Bn, ln, Cn = x.shape
    if out is None:
        if mode >= 1:
            raise L.TtskError("hifi_conv_pair: mode %d accumulates into `out`" % mode)
        out = torch.empty_like(x)
    if rows is not None:
        ra = _row_args("hifi_conv_pair", rows, Bn)
        if ws:
            check(L.load().ttsk_hifi_conv_pair_ws_rowlen(_ptr(x.contiguous()), _ptr(w1_pack), _ptr(bias1), _ptr(w2_pack), _ptr(bias2), _ptr(out),
                                                       int(x.dtype == f16), Bn, ln, Cn, K, dilation, slope, mode, scale, final_slope, int(max_wgs),
                                                       *ra, _stream()), "ttsk_hifi_conv_pair_ws_rowlen")
        else:
            check(L.load().ttsk_hifi_conv_pair_rowlen(_ptr(x), _ptr(w1_pack), _ptr(bias1), _ptr(w2_pack), _ptr(bias2), _ptr(out), int(x.dtype == f16),
                                                    Bn, ln, Cn, K, dilation, slope, mode, scale, final_slope, *ra, _stream()),
                  "ttsk_hifi_conv_pair_rowlen")
        return out
    if ws:
        check(L.load().ttsk_hifi_conv_pair_ws(_ptr(x.contiguous()), _ptr(w1_pack), _ptr(bias1), _ptr(w2_pack), _ptr(bias2), _ptr(out), int(x.dtype == f16),
                                              Bn, ln, Cn, K, dilation, slope, mode, scale, final_slope, int(max_wgs), _stream()), "ttsk_hifi_conv_pair_ws")
        return out
    check(L.load().ttsk_hifi_conv_pair(_ptr(x), _ptr(w1_pack), _ptr(bias1), _ptr(w2_pack), _ptr(bias2), _ptr(out), int(x.dtype == f16), Bn,
                                       ln, Cn, K, dilation, slope, mode, scale, final_slope, _stream()), "ttsk_hifi_conv_pair")
    return out


def hifi_resblock2_supported(Cn, K, d0, d1):
    return bool(L.load().ttsk_hifi_resblock2_supported(Cn, K, d0, d1))


def hifi_resblock2(x, w0_pack, bias0, w1_pack, bias1, K, dilations, slope=0.1, out=None, mode=0, scale=1.0, final_slope=1.0, rows=None):
    """One ResBlock2 (hifi/models.py:134-140) in one launch: x1 = x + b0 + conv_{K,d0}(lrelu(x)), y = x1 + b1 + conv_{K,d1}(lrelu(x1)).
    x (B, len, C) 16-bit raw block input; packs from pack_resblock_weight.  mode 0: out = y; 1: out += y;
    2: out = lrelu((out + y) * scale, final_slope) (the MRF average, :190-197; hifi_conv_pair's modes).
    rows (`_row_args`): a per-row length beside the batch stride (ttsk_hifi_resblock2_rowlen), as for hifi_conv_pair."""
    _dev(x, w0_pack, bias0, w1_pack, bias1, out)
    x = x.contiguous()
    Bn, ln, Cn = x.shape
    d0, d1 = (int(d) for d in dilations)
    if out is None:
        if mode >= 1:
            raise L.TtskError("hifi_resblock2: mode %d accumulates into `out`" % mode)
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != x.dtype or not out.is_contiguous():
        raise L.TtskError("hifi_resblock2: `out` must be a contiguous %s tensor of shape %s" % (x.dtype, tuple(x.shape)))
    if w0_pack.numel() < Cn * Cn * K or w1_pack.numel() < Cn * Cn * K or bias0.numel() < Cn or bias1.numel() < Cn:
        raise L.TtskError("hifi_resblock2: weight packs / biases too small for C=%d K=%d" % (Cn, K))
    if rows is not None:
        check(L.load().ttsk_hifi_resblock2_rowlen(_ptr(x), _ptr(w0_pack), _ptr(bias0), _ptr(w1_pack), _ptr(bias1), _ptr(out), int(x.dtype == f16), Bn,
                                                ln, Cn, K, d0, d1, slope, mode, scale, final_slope, *_row_args("hifi_resblock2", rows, Bn), _stream()),
              "ttsk_hifi_resblock2_rowlen")
        return out
    check(L.load().ttsk_hifi_resblock2(_ptr(x), _ptr(w0_pack), _ptr(bias0), _ptr(w1_pack), _ptr(bias1), _ptr(out), int(x.dtype == f16), Bn,
                                       ln, Cn, K, d0, d1, slope, mode, scale, final_slope, _stream()), "ttsk_hifi_resblock2")
    return out


def hifi_conv_window(x, w_pack, bias, K, dilation=1, R=None, out2=None, lrelu_out=False, slope=0.1):
    """out = [lrelu](conv_{K,dil}(x) + bias [+ R]) on the window kernel (C = 128); out2 (optional tensor) = lrelu(out)."""
    _dev(x, w_pack, bias, R, out2)
    Bn, ln, Cn = x.shape
    out = torch.empty_like(x)
    check(L.load().ttsk_hifi_conv_window(_ptr(x), _ptr(w_pack), _ptr(bias), _ptr(R), _ptr(out), _ptr(out2), int(x.dtype == f16), Bn, ln,
                                         Cn, K, dilation, int(lrelu_out), slope, _stream()), "ttsk_hifi_conv_window")
    return out


# ---------------------------------------------------------------------------------------------------- mel extraction (f-3)

def stft_frames(wav, pad, rows, hop, scale):
    """wav (B, len) fp32 -> fp16 (B, rows, 3*hop) = [hi | hi | lo]: reflect-padded, scaled hop-block rows split as hi + lo."""
    _dev(wav)
    Bsz, n = wav.shape
    out = torch.empty(Bsz, rows, 3 * hop, dtype=f16, device=wav.device)
    check(L.load().ttsk_stft_frames(_ptr(wav), _ptr(out), Bsz, n, pad, rows, hop, scale, _stream()), "ttsk_stft_frames")
    return out


def mel_from_spec(spec, Bsz, rows, T, nbins, vals, start, off, nnz, n_mels, eps, clip=1e-5):
    """spec (B*rows, ld) fp32 [Re | Im] -> log-mel (B, n_mels, T), energy (B, T)."""
    _dev(spec, vals, start, off)
    mel = torch.empty(Bsz, n_mels, T, dtype=torch.float32, device=spec.device)
    energy = torch.empty(Bsz, T, dtype=torch.float32, device=spec.device)
    check(L.load().ttsk_mel_from_spec(_ptr(spec), spec.stride(0), _ptr(vals), _ptr(start), _ptr(off), nnz, _ptr(mel),
                                      _ptr(energy), Bsz, rows, T, nbins, n_mels, eps, clip, _stream()), "ttsk_mel_from_spec")
    return mel, energy


# ---------------------------------------------------------------------------------------------------- Griffin-Lim

def _gl_f32(what, **tensors):
    for name, t in tensors.items():
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise L.TtskError("%s: %s must be a contiguous fp32 tensor" % (what, name))


def _gl_lens(what, lens, Bsz):
    if lens is not None and (lens.dtype != torch.int32 or lens.dim() != 1 or lens.numel() != Bsz or not lens.is_contiguous()):
        raise L.TtskError("%s: lens must be a contiguous int32 tensor of %d entries" % (what, Bsz))


def _gl_polar(what, mag, other=None):
    """(sB, sk, st) of a (B, bins, T) fp32 tensor in any layout; `other` must share shape and strides."""
    def strides(t):          # the stride of an axis of one element is arbitrary and never used
        return tuple(s if n > 1 else 0 for s, n in zip(t.stride(), t.shape))
    if mag.dim() != 3 or mag.dtype != torch.float32 or (other is not None and (other.dtype != torch.float32 or other.shape != mag.shape or
                                                                                 strides(other) != strides(mag))):
        raise L.TtskError("%s: needs (B, bins, T) fp32 tensors of one shape and layout" % what)
    return tuple(max(s, 1) for s in strides(mag))


def stft_polar(wav, lens, n_fft, hop, window, twiddle):
    """wav (B, N) fp32, lens int32 (B,) samples per row or None -> (magnitude, phase) (B, n_fft/2 + 1, 1 + N // hop) (include/ttsk.h)."""
    _dev(wav, lens, window, twiddle)
    _gl_f32("stft_polar", wav=wav, window=window, twiddle=twiddle)
    Bsz, n = wav.shape
    _gl_lens("stft_polar", lens, Bsz)
    T = 1 + n // hop
    mag = torch.empty(Bsz, n_fft // 2 + 1, T, dtype=torch.float32, device=wav.device)
    phase = torch.empty_like(mag)
    _count("stft_polar")
    check(L.load().ttsk_stft_polar(_ptr(wav), _ptr(lens), Bsz, n, n_fft, hop, _ptr(window), _ptr(twiddle), _ptr(mag), _ptr(phase), T, _stream()),
          "ttsk_stft_polar")
    return mag, phase


def istft_frames(mag, phase, lens, n_fft, hop, window, twiddle):
    """mag, phase (B, n_fft/2 + 1, T) fp32 in any (shared) layout, lens int32 (B,) frames per row or None -> windowed frames (B, T, n_fft)."""
    _dev(mag, phase, lens, window, twiddle)
    sB, sk, st = _gl_polar("istft_frames", mag, phase)
    Bsz, _, T = mag.shape
    _gl_lens("istft_frames", lens, Bsz)
    out = torch.empty(Bsz, T, n_fft, dtype=torch.float32, device=mag.device)
    _gl_f32("istft_frames", window=window, twiddle=twiddle)
    _count("istft_frames")
    check(L.load().ttsk_istft_frames(_ptr(mag), _ptr(phase), sB, sk, st, _ptr(lens), Bsz, T, n_fft, hop, _ptr(window), _ptr(twiddle), _ptr(out),
                                     _stream()), "ttsk_istft_frames")
    return out


def istft_ola(frames, lens, hop, window):
    """windowed frames (B, T, n_fft) -> wav (B, hop * (T - 1)): overlap-add as a gather, window-sum division, ends trimmed; zeros past a row."""
    _dev(frames, lens, window)
    _gl_f32("istft_ola", frames=frames, window=window)
    Bsz, T, n_fft = frames.shape
    _gl_lens("istft_ola", lens, Bsz)
    wav = torch.empty(Bsz, hop * (T - 1), dtype=torch.float32, device=frames.device)
    _count("istft_ola")
    check(L.load().ttsk_istft_ola(_ptr(frames), _ptr(lens), Bsz, T, n_fft, hop, _ptr(window), _ptr(wav), _stream()), "ttsk_istft_ola")
    return wav


def istft(mag, phase, lens, n_fft, hop, window, twiddle):
    """`istft_frames` then `istft_ola` through ttsk_istft: (B, n_fft/2 + 1, T) -> wav (B, hop * (T - 1))."""
    _dev(mag, phase, lens, window, twiddle)
    sB, sk, st = _gl_polar("istft", mag, phase)
    _gl_f32("istft", window=window, twiddle=twiddle)
    Bsz, _, T = mag.shape
    _gl_lens("istft", lens, Bsz)
    work = torch.empty(Bsz, T, n_fft, dtype=torch.float32, device=mag.device)
    wav = torch.empty(Bsz, hop * max(T - 1, 0), dtype=torch.float32, device=mag.device)
    _count("istft")
    check(L.load().ttsk_istft(_ptr(mag), _ptr(phase), sB, sk, st, _ptr(lens), Bsz, T, n_fft, hop, _ptr(window), _ptr(twiddle), _ptr(work),
                              _ptr(wav), _stream()), "ttsk_istft")
    return wav


def griffinlim_step(src, mag, lens, n_fft, hop, window, twiddle, out, zprev=None, momentum=0.0):
    """One Griffin-Lim iteration (include/ttsk.h).  src: the signal (B, >= hop * (T - 1)) or the previous step's frames (B, T, n_fft);
    mag (B, n_fft/2 + 1, T) in any layout; out: frames (B, T, n_fft), another buffer than src; zprev (B, T, n_fft/2 + 1, 2) with momentum > 0."""
    _dev(src, mag, lens, window, twiddle, out, zprev)
    sB, sk, st = _gl_polar("griffinlim_step", mag)
    Bsz, _, T = mag.shape
    _gl_lens("griffinlim_step", lens, Bsz)
    _gl_f32("griffinlim_step", src=src, window=window, twiddle=twiddle, out=out, zprev=zprev)
    if tuple(out.shape) != (Bsz, T, n_fft) or (zprev is not None and tuple(zprev.shape) != (Bsz, T, n_fft // 2 + 1, 2)):
        raise L.TtskError("griffinlim_step: out must be (B, T, n_fft) and zprev (B, T, n_fft/2 + 1, 2)")
    from_frames = src.dim() == 3
    if (from_frames and src.shape != out.shape) or (not from_frames and (src.dim() != 2 or src.shape[0] != Bsz)):
        raise L.TtskError("griffinlim_step: src must be frames (B, T, n_fft) or a signal (B, samples)")
    _count("griffinlim_step")
    check(L.load().ttsk_griffinlim_step(None if from_frames else _ptr(src), 0 if from_frames else src.shape[1], _ptr(src) if from_frames else None,
                                        _ptr(mag), sB, sk, st, _ptr(lens), _ptr(zprev), float(momentum), Bsz, T, n_fft, hop, _ptr(window),
                                        _ptr(twiddle), _ptr(out), _stream()), "ttsk_griffinlim_step")
    return out


def mel_to_spec(mel, vals, start, off, nbins, scale=1000.0):
    """log-mel (B, n_mels, T) fp32, the packed filterbank of `MelExtractor` -> (B, nbins, T) = scale * exp(mel)^T @ filterbank, transposed."""
    _dev(mel, vals, start, off)
    _gl_f32("mel_to_spec", mel=mel, vals=vals)
    if mel.dim() != 3 or start.dtype != torch.int32 or off.dtype != torch.int32 or off.numel() != mel.shape[1] + 1 or start.numel() != mel.shape[1]:
        raise L.TtskError("mel_to_spec: mel must be (B, n_mels, T) with int32 tables of n_mels starts and n_mels + 1 offsets")
    Bsz, n_mels, T = mel.shape
    spec = torch.empty(Bsz, nbins, T, dtype=torch.float32, device=mel.device)
    _count("mel_to_spec")
    check(L.load().ttsk_mel_to_spec(_ptr(mel), _ptr(vals), _ptr(start), _ptr(off), Bsz, n_mels, nbins, T, float(scale), _ptr(spec), _stream()),
          "ttsk_mel_to_spec")
    return spec


def yin_lags(sr, f0_floor, f0_ceil):
    """(tau_min, tau_max) = (ceil(sr / f0_ceil), floor(sr / f0_floor)): the lags `pitch_yin` scans."""
    import math
    if not (0.0 < f0_floor < f0_ceil):
        raise L.TtskError("pitch_yin: needs 0 < f0_floor < f0_ceil, got %r, %r" % (f0_floor, f0_ceil))
    return int(math.ceil(sr / f0_ceil)), int(math.floor(sr / f0_floor))


def pitch_yin(wav, lens=None, *, sr=22050, hop=256, window=1024, f0_floor=71.0, f0_ceil=800.0, threshold=0.15):
    """wav (B, ld) fp32, lens int32 (B,) device tensor or None -> f0 (B, 1 + ld // hop) fp32 by YIN (include/ttsk.h): row b has
    1 + lens[b] // hop frames, later ones are 0; 0 = unvoiced.  Samples from lens[b] on are never read."""
    _dev(wav, lens)
    if wav.dim() != 2 or wav.dtype != torch.float32 or not wav.is_contiguous():
        raise L.TtskError("pitch_yin: wav must be a contiguous (B, ld) fp32 tensor")
    Bsz, ld = wav.shape
    if lens is not None and (lens.dtype != torch.int32 or lens.dim() != 1 or lens.numel() != Bsz or not lens.is_contiguous()):
        raise L.TtskError("pitch_yin: lens must be a contiguous int32 tensor of %d entries" % Bsz)
    tau_min, tau_max = yin_lags(sr, f0_floor, f0_ceil)
    T_max = 1 + ld // int(hop) if hop > 0 else 0
    f0 = torch.empty(Bsz, max(T_max, 0), dtype=torch.float32, device=wav.device)
    _count("pitch_yin")
    check(L.load().ttsk_pitch_yin(_ptr(wav), _ptr(lens), Bsz, ld, int(hop), int(window), tau_min, tau_max, float(sr), float(threshold),
                                  _ptr(f0), T_max, _stream()), "ttsk_pitch_yin")
    return f0


def phoneme_prosody(f0, energy, dur, T, Lp):
    """f0, energy (B, ldT) fp32; dur (B, ldL) int32; T, Lp (B,) int32: frames and phonemes per row -> (pitch (B, ldL), energy (B, ldL),
    pitch_mean (B,), pitch_std (B,), status (B,) int32): the reference's phoneme-level reduction (include/ttsk.h).  status 0: good;
    1: fewer than two voiced frames; 2: more duration than frames; 3: constant pitch.  A row with a status holds zeros."""
    _dev(f0, energy, dur, T, Lp)
    if (f0.dim() != 2 or f0.shape != energy.shape or f0.dtype != torch.float32 or energy.dtype != torch.float32 or not f0.is_contiguous() or
            not energy.is_contiguous()):
        raise L.TtskError("phoneme_prosody: f0 and energy must be contiguous (B, frames) fp32 tensors of one shape")
    Bsz, ldT = f0.shape
    if dur.dim() != 2 or dur.shape[0] != Bsz or dur.dtype != torch.int32 or not dur.is_contiguous():
        raise L.TtskError("phoneme_prosody: dur must be a contiguous (B, phonemes) int32 tensor")
    for name, v in (("T", T), ("Lp", Lp)):
        if v.dtype != torch.int32 or v.dim() != 1 or v.numel() != Bsz or not v.is_contiguous():
            raise L.TtskError("phoneme_prosody: %s must be a contiguous int32 tensor of %d entries" % (name, Bsz))
    ldL = dur.shape[1]
    pitch = torch.empty(Bsz, ldL, dtype=torch.float32, device=f0.device)
    en = torch.empty(Bsz, ldL, dtype=torch.float32, device=f0.device)
    pmean = torch.empty(Bsz, dtype=torch.float32, device=f0.device)
    pstd = torch.empty(Bsz, dtype=torch.float32, device=f0.device)
    status = torch.empty(Bsz, dtype=torch.int32, device=f0.device)
    _count("phoneme_prosody")
    check(L.load().ttsk_phoneme_prosody(_ptr(f0), _ptr(energy), ldT, _ptr(dur), ldL, _ptr(T), _ptr(Lp), Bsz, _ptr(pitch), _ptr(en),
                                        _ptr(pmean), _ptr(pstd), _ptr(status), _stream()), "ttsk_phoneme_prosody")
    return pitch, en, pmean, pstd, status


DTW_MAX_C, DTW_MAX_T, DTW_MAX_L = 128, 2048, 1024      # ttsk_dtw_align's limits


def dtw_align(x, y, x_lens=None, y_lens=None, x_seg=None, n_seg=None):
    """x (B, ldx, C), y (B, ldy, C) fp32; x_lens, y_lens (B,) int32 or None (full rows) -> (path_x (B, ldy) int32, cost (B,) fp32,
    status (B,) int32): the dynamic-time-warping path of every pair (include/ttsk.h): path_x[b, j] is the last row of x matched to
    row j of y (-1 from y_lens[b] on), cost the cumulative squared distance along the path.  With x_seg (B, ldL) int32, the rows of x
    per phoneme (n_seg (B,) int32 phonemes per row, None: ldL), also dur (B, ldL) int32: the rows of y per phoneme.  status 0: good;
    2: an empty sequence; 3: x_seg is negative somewhere or does not sum to x_lens.  The workspace is allocated here."""
    for name, v in (("x", x), ("y", y)):
        if v.dim() != 3 or v.dtype != torch.float32 or not v.is_contiguous():
            raise L.TtskError("dtw_align: %s must be a contiguous (B, frames, C) fp32 tensor" % name)
    Bsz, ldx, Cc = x.shape
    if y.shape[0] != Bsz or y.shape[2] != Cc:
        raise L.TtskError("dtw_align: y is %s, x is %s: batch and channels must agree" % (tuple(y.shape), tuple(x.shape)))
    ldy = y.shape[1]
    if not 1 <= Cc <= DTW_MAX_C:
        raise L.TtskError("dtw_align: C = %d channels, 1..%d are taken" % (Cc, DTW_MAX_C))
    for name, ld in (("x", ldx), ("y", ldy)):
        if not 1 <= ld <= DTW_MAX_T:
            raise L.TtskError("dtw_align: %s has %d frames per row, 1..%d are taken" % (name, ld, DTW_MAX_T))
    for name, v in (("x_lens", x_lens), ("y_lens", y_lens), ("n_seg", n_seg)):
        if v is not None and (v.dtype != torch.int32 or v.dim() != 1 or v.numel() != Bsz or not v.is_contiguous()):
            raise L.TtskError("dtw_align: %s must be a contiguous int32 tensor of %d entries" % (name, Bsz))
    ldL = 0
    if x_seg is not None:
        if x_seg.dim() != 2 or x_seg.shape[0] != Bsz or x_seg.dtype != torch.int32 or not x_seg.is_contiguous():
            raise L.TtskError("dtw_align: x_seg must be a contiguous (B, phonemes) int32 tensor")
        ldL = x_seg.shape[1]
        if not 1 <= ldL <= DTW_MAX_L:
            raise L.TtskError("dtw_align: x_seg has %d phonemes per row, 1..%d are taken" % (ldL, DTW_MAX_L))
    elif n_seg is not None:
        raise L.TtskError("dtw_align: n_seg without x_seg")
    _dev(x, y, x_lens, y_lens, x_seg, n_seg)
    lib = L.load()
    path_x = torch.empty(Bsz, ldy, dtype=torch.int32, device=x.device)
    cost = torch.empty(Bsz, dtype=torch.float32, device=x.device)
    status = torch.empty(Bsz, dtype=torch.int32, device=x.device)
    dur = torch.empty(Bsz, ldL, dtype=torch.int32, device=x.device) if x_seg is not None else None
    nbytes = int(lib.ttsk_dtw_workspace_bytes(Bsz, ldx, ldy))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    _count("dtw_align")
    check(lib.ttsk_dtw_align(_ptr(x), _ptr(y), _ptr(x_lens), _ptr(y_lens), Bsz, ldx, ldy, Cc, _ptr(x_seg), _ptr(n_seg), ldL, _ptr(ws), nbytes,
                             _ptr(path_x), _ptr(cost), _ptr(status), _ptr(dur), _stream()), "ttsk_dtw_align")
    return (path_x, cost, status) if dur is None else (path_x, cost, status, dur)
