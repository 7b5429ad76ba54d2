"""GPU: every kernel family that applies dropout applies exactly the mask `ttsk_dropout_keep_mask` exports, and that mask is
Philox4x32-10 over the counter layout of csrc/rowops.hip (element e of a site's row-major tensor is kept iff word e & 3 of
Philox(key = seed, counter = (e >> 2, site, step lo, step hi)) >= keep_threshold(p)), restated here in numpy.

The kernels draw the keep bits early (under their memory waits, csrc/common.h keep4) and apply them late (drop4), so what is checked
is WHERE an output was dropped, read off outputs that reveal it exactly:
* forward (ttsk_win_ln_fwd / _proj_fwd, ttsk_gemm_ln_fwd): z_save = dropout(A W' + bias) + residual equals the bf16 residual exactly
  where the element was dropped; the bias is 64, so a kept element ((acc + 64) / (1 - p) + residual, |acc| and |residual| of order 1)
  never does;
* backward (ttsk_layernorm_bwd_proj: plain, slabs, PRE; ttsk_layernorm_bwd / _slabs): dy is zero exactly at the dropped elements
  wherever dz is not zero itself (PAD rows, closed ReLUs);
* PostNet (ttsk_bn_train_apply): the keep nibbles it stores are the mask; the backward gives the same dx from them and from rng.
Row counts 1, 31, 33, 75: the last 32-row tile is partly live (33: one live row); outputs sit in front of guard rows that must keep
their fill.  With p = 0 and a null rng every entry point returns TTSK_OK and what it returns with an rng."""
import numpy as np
import pytest
import torch

from tts_king_amd import lib as L, ops

DEV = "cuda:0"
BF16 = torch.bfloat16
SEED = 0x5DEECE66D1234567            # high word set
STEP = (1 << 40) + 3                 # high step word set
MS = [1, 31, 33, 75]
GUARD, FILL = 8, 12352.0             # guard rows behind every output, and their fill (exact in bf16)
gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- the reference

_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(key, ctr):
    """key: two ints; ctr: four uint64 arrays of 32-bit values -> four uint64 arrays of 32-bit values."""
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    c = [np.asarray(x, dtype=np.uint64) for x in ctr]
    m0, m1, s32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                      # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & _MASK, (p0 >> s32) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _MASK, (k1 + np.uint64(0xBB67AE85)) & _MASK
    return c


def keep_threshold(p):
    t = float(np.float32(p)) * 4294967296.0                # the kernels take p as a float
    return 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def keep_ref(seed, step, site, n, p):
    """uint8[n]: 1 = kept."""
    e4 = np.arange(n // 4, dtype=np.uint64)
    full = lambda v: np.full(n // 4, v, dtype=np.uint64)
    w = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (e4, full(site), full(step & 0xFFFFFFFF), full(step >> 32)))
    return (np.stack(w, axis=1).reshape(-1) >= np.uint64(keep_threshold(p))).astype(np.uint8)


def test_reference_philox_known_answers():
    """The numpy generator against the published philox4x32-10 vectors, the threshold rule at its ends, and the keep rate."""
    kat = [((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff, 0xffffffff), (0xffffffff,) * 4, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for key, ctr, want in kat:
        got = philox4x32_10(key, [np.array([v], dtype=np.uint64) for v in ctr])
        assert tuple(int(g[0]) for g in got) == want
    assert keep_threshold(0.0) == 0 and keep_threshold(0.5) == 1 << 31 and keep_threshold(1 - 2.0 ** -20) == (1 << 32) - 4096
    assert keep_ref(SEED, STEP, 7, 4096, 0.0).all()
    for p in (0.1, 0.5):
        rate = 1.0 - keep_ref(SEED, STEP, 7, 1 << 16, p).mean()
        assert abs(rate - p) < 4 * (p * (1 - p) / (1 << 16)) ** 0.5, (p, rate)        # four sigma
    # a different step, site or seed word gives another mask
    a = keep_ref(SEED, STEP, 7, 4096, 0.5)
    for other in (keep_ref(SEED, STEP + 1, 7, 4096, 0.5), keep_ref(SEED, STEP + (1 << 32), 7, 4096, 0.5), keep_ref(SEED, STEP, 8, 4096, 0.5),
                  keep_ref(SEED ^ (1 << 32), STEP, 7, 4096, 0.5)):
        assert (a != other).mean() > 0.3


# ---------------------------------------------------------------------------------------------------------------- helpers

def state(step=STEP):
    st = ops.optim_state(DEV, seed=SEED)
    st[3] = step
    return st


def mask(site, n, p, step=STEP):
    """Host bool[n]: True = dropped, from the numpy reference."""
    return torch.from_numpy(keep_ref(SEED, step, site, n, p) == 0)


def share_ok(dropped, p):
    s = dropped.float().mean().item()
    print("dropped share %.4f (p = %g, %d elements)" % (s, p, dropped.numel()))
    assert p / 2 <= s <= 2 * p, (s, p)


def guarded(rows, cols, dtype=BF16):
    """(view of the first `rows` rows, whole tensor) of a (rows + GUARD, cols) allocation filled with FILL."""
    t = torch.full((rows + GUARD, cols), FILL, dtype=dtype, device=DEV)
    return t[:rows], t


def guard_intact(whole, rows):
    return bool((whole[rows:] == FILL).all())


def pack(W, transpose):
    out = torch.empty(W.numel(), dtype=BF16, device=DEV)
    ops.win_conv_pack_items([(W, out, transpose)])
    return out


# ---------------------------------------------------------------------------------------------------------------- the exported mask

@gpu
@pytest.mark.parametrize("site", [0, 30, (1 << 32) - 1])
@pytest.mark.parametrize("step", [0, 1, 1 << 32, (1 << 40) + 3])
def test_exported_mask_is_philox(site, step):
    n = 4 * 1031
    st = state(step)
    for p in (0.0, 0.1, 0.5, 1 - 2.0 ** -20):
        got = ops.dropout_keep_mask(st, site, n, p).cpu().numpy()
        want = keep_ref(SEED, step, site, n, p)
        assert got.tobytes() == want.tobytes(), (site, step, p, int((got != want).sum()))


# ---------------------------------------------------------------------------------------------------------------- forward

FWD = ["win256", "win1024", "win256_proj", "win1024_proj", "gemm_ln"]
# M <= 75: few tiles, so the projection behind a 1,024-wide contraction runs as its SPLIT parts; 2081 rows (66 tiles, the last with one
# live row) reach the unsplit instance of that family
FWD_CASES = [(f, M) for f in FWD for M in MS] + [("win1024_proj", 2081)]


def fwd_inputs(family, M, seed=0):
    g = torch.Generator().manual_seed(seed)
    K = {"win256": 256, "win256_proj": 256, "win1024": 1024, "win1024_proj": 1024, "gemm_ln": 192}[family]
    d = dict(K=K, proj=family.endswith("_proj"), gemm=family == "gemm_ln")
    d["x"] = torch.randn(M, K, generator=g).to(BF16).to(DEV)
    W = (torch.randn(256, 1, K, generator=g) * K ** -0.5).to(BF16).to(DEV)
    d["W"] = W.reshape(256, K).contiguous() if d["gemm"] else pack(W, False)
    d["bias"] = torch.full((256,), 64.0, device=DEV)
    d["res"] = torch.randn(M, 256, generator=g).to(BF16).to(DEV)
    d["gamma"], d["beta"] = (1 + 0.1 * torch.randn(256, generator=g)).to(DEV), (0.1 * torch.randn(256, generator=g)).to(DEV)
    if d["proj"]:
        d["pw"] = pack((torch.randn(768, 1, 256, generator=g) * 256 ** -0.5).to(BF16).to(DEV), False)
        d["pb"] = (0.1 * torch.randn(768, generator=g)).to(DEV)
    return d


def fwd_run(d, M, p, site, rng):
    """-> dict of (view, whole) outputs; raises unless the entry point returns TTSK_OK."""
    lib, P, K = L.load(), ops._ptr, d["K"]
    o = {"out": guarded(M, 256), "z": guarded(M, 256), "mean": guarded(M, 1, torch.float32), "rstd": guarded(M, 1, torch.float32)}
    common = (P(d["bias"]), P(d["res"]), P(d["gamma"]), P(d["beta"]), P(o["out"][1]), P(o["z"][1]), P(o["mean"][1]), P(o["rstd"][1]), None, 0, M, K, 256,
              1e-5, p, site, P(rng))
    if d["gemm"]:
        rc = lib.ttsk_gemm_ln_fwd(P(d["x"]), K, P(d["W"]), K, *common, ops._stream())
    elif d["proj"]:
        o["qkv"] = guarded(M, 768)
        rc = lib.ttsk_win_ln_proj_fwd(P(d["x"]), K, P(d["W"]), *common, P(d["pw"]), P(d["pb"]), 768, P(o["qkv"][1]), ops._stream())
    else:
        rc = lib.ttsk_win_ln_fwd(P(d["x"]), K, P(d["W"]), *common, ops._stream())
    ops.check(rc, "forward " + str(d["K"]))
    torch.cuda.synchronize()
    return o


@gpu
@pytest.mark.parametrize("family,M", FWD_CASES)
def test_forward_drops_exactly_the_mask(family, M):
    p, site, st = 0.1, 30, state()
    d = fwd_inputs(family, M)
    o = fwd_run(d, M, p, site, ops.rng_of(st))
    dropped = (o["z"][0].view(torch.int16) == d["res"].view(torch.int16)).cpu()
    want = mask(site, M * 256, p).view(M, 256)
    assert torch.equal(dropped, want), int((dropped != want).sum())
    share_ok(dropped, p)
    for k, (view, whole) in o.items():
        assert guard_intact(whole, M), k
        assert bool(torch.isfinite(view.float()).all()), k


@gpu
@pytest.mark.parametrize("family", FWD)
def test_forward_p0_null_rng(family):
    M, st = 33, state()
    d = fwd_inputs(family, M)
    a, b = fwd_run(d, M, 0.0, 30, None), fwd_run(d, M, 0.0, 30, ops.rng_of(st))
    for k in a:
        assert torch.equal(a[k][1], b[k][1]), k
    assert not bool((a["z"][0].view(torch.int16) == d["res"].view(torch.int16)).any())        # nothing dropped


# ---------------------------------------------------------------------------------------------------------------- backward

BWD = ["proj256", "proj1024", "proj256_slabs", "proj256_pre", "proj1024_pre", "ln_bwd256", "ln_bwd256_slabs", "ln_bwd_relu", "ln_bwd512"]
# M <= 75: the 1,024-channel projection runs as its SPLIT parts; 2049 rows (65 tiles, the last with one live row) reach the unsplit instances
BWD_CASES = [(f, M) for f in BWD for M in MS] + [("proj1024", 2049), ("proj1024_pre", 2049)]


def bwd_run(family, M, p, site, rng, seed=1):
    """-> (dz, dy, n masked rows at the end); one utterance of M rows whose last quarter is PAD."""
    g = torch.Generator().manual_seed(seed)
    D = 512 if family == "ln_bwd512" else 256
    r = lambda *s: torch.randn(*s, generator=g)
    z = r(M, D).to(BF16).to(DEV)
    mean, rstd = (0.1 * r(M)).to(DEV), (0.5 + torch.rand(M, generator=g)).to(DEV)
    gamma, beta = (1 + 0.1 * r(D)).to(DEV), (0.1 * r(D)).to(DEV)
    dout, R = r(M, D).to(BF16).to(DEV), r(M, D).to(BF16).to(DEV)
    npad = M // 4
    lens = torch.tensor([M - npad], dtype=torch.int64, device=DEV)
    slabs = ops.Slabs(r(3, M * D).to(DEV), 3, M * D)
    kw = dict(lens=lens, seg_len=M, p_pre=p, site_pre=site, rng=rng)
    if family.startswith("proj"):
        Cout = 1024 if "1024" in family else 256
        w = pack((r(256, 1, Cout) * 256 ** -0.5).to(BF16).to(DEV), True)
        gate = r(M, Cout).clamp(min=0).to(BF16).to(DEV) if Cout == 1024 else None
        if family.endswith("_pre"):
            pre = (r(M, 768).to(BF16).to(DEV), pack((r(768, 1, 256) * 768 ** -0.5).to(BF16).to(DEV), True))
            dz, dy = ops.layernorm_bwd_proj(None, z, mean, rstd, gamma, w, Cout, R=R, gate=gate, pre=pre, **kw)[:2]
        elif family.endswith("_slabs"):
            dz, dy = ops.layernorm_bwd_proj(None, z, mean, rstd, gamma, w, Cout, slabs=slabs, R=R, gate=gate, **kw)[:2]
        else:
            dz, dy = ops.layernorm_bwd_proj(dout, z, mean, rstd, gamma, w, Cout, gate=gate, **kw)[:2]
    elif family == "ln_bwd256_slabs":
        dz, dy = ops.layernorm_bwd(None, z, mean, rstd, gamma, beta, slabs=slabs, R=R, **kw)[:2]
    else:
        dz, dy = ops.layernorm_bwd(dout, z, mean, rstd, gamma, beta, relu_in=family == "ln_bwd_relu", **kw)[:2]
    torch.cuda.synchronize()
    return dz.float().cpu(), dy.float().cpu(), npad


@gpu
@pytest.mark.parametrize("family,M", BWD_CASES)
def test_backward_zeroes_exactly_the_mask(family, M):
    p, site, st = 0.1, 30, state()
    dz, dy, npad = bwd_run(family, M, p, site, ops.rng_of(st))
    D = dz.shape[1]
    want = mask(site, M * D, p).view(M, D)
    nz = dz != 0
    assert torch.equal((dy == 0)[nz], want[nz]), int(((dy == 0) != want)[nz].sum())
    assert bool((dy[~nz] == 0).all())
    live = M - npad
    assert bool((dz[live:] == 0).all()) and bool((dy[live:] == 0).all())                    # PAD rows carry no gradient
    assert nz[:live].float().mean().item() > (0.3 if family == "ln_bwd_relu" else 0.99)      # the check is not vacuous
    share_ok((dy == 0)[:live][nz[:live]], p)


@gpu
@pytest.mark.parametrize("family", BWD)
def test_backward_p0_null_rng(family):
    st = state()
    a, b = bwd_run(family, 33, 0.0, 30, None), bwd_run(family, 33, 0.0, 30, ops.rng_of(st))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], a[1])                                                            # dy is dz without dropout


# ---------------------------------------------------------------------------------------------------------------- PostNet BatchNorm

def bn_run(rows, C, cut, p, rng, seed=2):
    g = torch.Generator().manual_seed(seed)
    B = 1 if rows == 5 else 3
    seg = rows // B
    limit = (seg - seg // 5 - 1) if cut else None
    fl = (torch.tensor([limit], dtype=torch.int32, device=DEV), seg) if cut else None
    x = torch.randn(rows, C, generator=g).to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    run = (torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV))
    out, mean, rstd, keep = ops.bn_train(x, *run, gamma, beta, True, p=p, site=40, rng=rng, frame_limit=fl, want_keep=True)
    dout = torch.randn(rows, C, generator=g).to(BF16).to(DEV)
    dxs = [ops.bn_bwd(dout, x, mean, rstd, gamma, beta, True, p=p, site=40, rng=rng, frame_limit=fl, keep=k, accumulate=False) for k in (keep, None)]
    torch.cuda.synchronize()
    live = torch.ones(rows, dtype=torch.bool) if not cut else (torch.arange(rows) % seg) < limit
    return out, keep, dxs, live


@gpu
@pytest.mark.parametrize("cut", [False, True], ids=["all_rows", "frame_limit"])
@pytest.mark.parametrize("rows", [5, 141])
@pytest.mark.parametrize("C", [512, 80])
def test_bn_keep_nibbles_are_the_mask(C, rows, cut):
    p, st = 0.5, state()
    out, keep, dxs, live = bn_run(rows, C, cut, p, ops.rng_of(st))
    k = torch.from_numpy(keep_ref(SEED, STEP, 40, rows * C, p)).view(rows, C // 4, 4).to(torch.int32)
    want = (k[..., 0] | (k[..., 1] << 1) | (k[..., 2] << 2) | (k[..., 3] << 3)) * live.view(-1, 1).to(torch.int32)
    got = keep.cpu().to(torch.int32)
    assert torch.equal(got, want), int((got != want).sum())
    share_ok((k == 0)[live], p)
    # a dropped element of a live row is an exact zero of the output (tanh(...) * 2 is zero for no kept element of these inputs)
    o = out.float().cpu().view(rows, C // 4, 4)
    assert torch.equal((o == 0)[live], (k == 0)[live])
    assert bool((o[~live] == 0).all())
    assert torch.equal(dxs[0], dxs[1])                              # the backward from the keep bytes and from rng


@gpu
@pytest.mark.parametrize("C", [512, 80])
def test_bn_p0_null_rng(C):
    st = state()
    a, b = bn_run(141, C, True, 0.0, None), bn_run(141, C, True, 0.0, ops.rng_of(st))
    assert a[1] is None and b[1] is None
    assert torch.equal(a[0], b[0])
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)
