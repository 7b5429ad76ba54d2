"""Diagnostic: where a workgroup of the slab BatchNorm kernels (ttsk_bn_train_apply, ttsk_bn_bwd_apply_slab, ttsk_bn_bwd_stats_slab)
spends its lifetime at the training shape (B = 16, T = 423; C = 512 and C = 80), each launched right behind the kernel that writes its
input, so that its rows are as cold as in the step.  s_memrealtime stamps (100 MHz), thread 0 of every workgroup: [0] start, [1] rows
requested, [2] requested rows and partial rows arrived (the stamp waits for them), [3] totals done, [4] mean / rstd (or the two sums)
published, [5] arithmetic done, [6] stores issued, [7] stores acknowledged.  A slot a kernel does not stamp repeats the one before it.
Also prints the device-event time of producer + BatchNorm against the producer alone."""
# Needs the diagnostic build: `make -C tts_king_amd/csrc stamps` and TTSK_LIB_PATH=tts_king_amd/libttsk_hip_stamps.so (the product
# library carries neither the stamp code nor the *_set_stamps hooks).

import ctypes as C, os, sys
import numpy as np
import torch
sys.path.insert(0, os.getcwd())
from tts_king_amd import ops, lib as L
DEV = "cuda:0"
BF = torch.bfloat16
g = torch.Generator().manual_seed(0)
lib = L.load()
hook = getattr(lib, "ttsk_bn_set_stamps", None)
if hook is not None:
    hook.argtypes = [C.c_void_p]
B, T, NWG = 16, 423, 4096
rows = B * T
st = ops.optim_state(DEV, seed=1234)
rng = ops.rng_of(st)
P = lambda t: ops._ptr(t)


def layer(Cn):
    gamma, beta = (1 + 0.1 * torch.randn(Cn, generator=g)).to(DEV), (0.1 * torch.randn(Cn, generator=g)).to(DEV)
    run = (torch.zeros(Cn, device=DEV), torch.ones(Cn, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV))
    return gamma, beta, run


# C = 512: a PostNet 512 -> 512 conv writes x and the statistics partial rows, its input-gradient conv writes dout and the backward's
xin = torch.randn(B, T, 512, generator=g).to(BF).to(DEV)
W = (torch.randn(512, 5, 512, generator=g) * 0.02).to(BF).to(DEV)
bias = (0.1 * torch.randn(512, generator=g)).to(DEV)
pk, pkT = (torch.empty(W.numel(), dtype=BF, device=DEV) for _ in range(2))
ops.win_conv_pack_items([(W, pk, False), (W, pkT, True)])
g5, b5, run5 = layer(512)
s5 = {}


def pre_f512():
    s5["x"], s5["stats"] = ops.win_conv_stats(xin, pk, 512, 5, bias=bias)


def f512():
    s5["out"], s5["mean"], s5["rstd"], s5["keep"] = ops.bn_train(s5["x"].view(rows, 512), *run5, g5, b5, True, p=0.5, site=300, rng=rng, want_keep=True,
                                                                 partials=s5["stats"])


def pre_b512():
    s5["dout"], s5["bstats"] = ops.win_conv_bnb(xin, pkT, 512, 5, s5["x"].view(rows, 512), s5["mean"], s5["rstd"], g5, b5, True, p=0.5, keep=s5["keep"])


def b512():
    dg, db = torch.zeros(512, device=DEV), torch.zeros(512, device=DEV)
    ops.bn_bwd(s5["dout"].view(rows, 512), s5["x"].view(rows, 512), s5["mean"], s5["rstd"], g5, b5, True, p=0.5, site=300, rng=rng, dgamma=dg, dbeta=db,
               keep=s5["keep"], partials=s5["bstats"])


# C = 80: the last layer (no tanh, no dropout, residual, fp32 out); x, dout and the partial rows are rewritten by a kernel just before
src80, res80, dsrc80 = (torch.randn(rows, 80, generator=g).to(DEV) for _ in range(3))
g8, b8, run8 = layer(80)
s8 = {"p": torch.empty(lib.ttsk_bn_nchunks(rows), 160, device=DEV), "bp": torch.empty(lib.ttsk_bn_nchunks(rows), 160, device=DEV)}


def pre_f80():
    s8["x"] = src80 + 0.25
    ops.check(lib.ttsk_bn_stats_slab(P(s8["x"]), 1, rows, 80, P(s8["p"]), None, 0, ops._stream()), "ttsk_bn_stats_slab")


def f80():
    s8["out"], s8["mean"], s8["rstd"] = ops.bn_train(s8["x"], *run8, g8, b8, False, resid=res80, out_f32=True, partials=s8["p"])


def pre_bs80():
    s8["dout"] = dsrc80 * 0.5


def bs80():
    ops.check(lib.ttsk_bn_bwd_stats_slab(P(s8["dout"]), 1, P(s8["x"]), 1, P(s8["mean"]), P(s8["rstd"]), P(g8), P(b8), rows, 80, 0, 0.0, 0, None, None,
                                         P(s8["bp"]), None, 0, ops._stream()), "ttsk_bn_bwd_stats_slab")


def pre_b80():
    pre_bs80()
    bs80()


def b80():
    dg, db = torch.zeros(80, device=DEV), torch.zeros(80, device=DEV)
    ops.bn_bwd(s8["dout"], s8["x"], s8["mean"], s8["rstd"], g8, b8, False, dgamma=dg, dbeta=db, partials=s8["bp"])


cases = [("bn_apply2<false>     C = 512 behind win_conv_stats", pre_f512, f512), ("bn_bwd_apply2        C = 512 behind win_conv_bnb", pre_b512, b512),
         ("bn_apply2<true>      C = 80", pre_f80, f80), ("bn_bwd_stats2        C = 80", pre_bs80, bs80), ("bn_bwd_apply2        C = 80", pre_b80, b80)]
NAMES = ["rows requested", "all arrived", "totals", "published", "arithmetic", "stores issued", "stores acked"]
N = int(os.environ.get("ITERS", "40"))
print("library:", os.environ.get("TTSK_LIB_PATH", "tts_king_amd/libttsk_hip.so"))
for name, pre, fn in cases:
    for _ in range(3):
        pre(); fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    for _ in range(N):
        pre()
    ev[1].record()
    for _ in range(N):
        pre(); fn()
    ev[2].record()
    torch.cuda.synchronize()
    alone, both = ev[0].elapsed_time(ev[1]) * 1e3 / N, ev[1].elapsed_time(ev[2]) * 1e3 / N
    print("%s: producer %.1f us, producer + BatchNorm %.1f us, difference %.1f us (device events, %d iterations)" % (name, alone, both, both - alone, N))
    if hook is None:
        continue
    buf = torch.zeros(NWG * 8, dtype=torch.int64, device=DEV)
    pre()
    hook(C.c_void_p(buf.data_ptr()))
    fn()
    torch.cuda.synchronize()
    hook(C.c_void_p(0))
    raw = buf.cpu().numpy().reshape(NWG, 8).astype(np.float64)
    raw = raw[raw[:, 0] > 0]
    for i in range(1, 8):           # a slot the kernel does not stamp repeats the one before it
        raw[:, i] = np.where(raw[:, i] > 0, raw[:, i], raw[:, i - 1])
    s = (raw - raw[:, 0].min()) * 0.01
    dd = np.diff(s, axis=1)
    life = s[:, 7] - s[:, 0]
    print("   %d workgroups, span %.1f us, starts up to %.1f us, lifetime mean %.1f (max %.1f) us" % (len(s), s[:, 7].max(), s[:, 0].max(), life.mean(), life.max()))
    print("   phases, mean (max) us: " + " | ".join("%s %.2f (%.2f)" % (NAMES[i], dd[:, i].mean(), dd[:, i].max()) for i in range(7)))
