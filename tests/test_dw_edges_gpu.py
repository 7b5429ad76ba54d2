"""GPU: csrc/dwgemm.hip and csrc/dwconv.hip (every large weight gradient of the FS2 step) at the edges of their K-step pipelines, `lens`
handling, per-lane utterance tables, row pitches, multi-problem launches and dwgemm's capped grid — against tests/dw_ref.py (fp64,
tied to torch's conv1d weight gradient by tests/test_dw_ref_cpu.py).

Two input modes:
* `ints`   dy, x are integers in [-3, 3] as bf16, a destination that is accumulated into holds an integer: every product and every
           partial sum is exact in fp32 (|sum| <= 9 * rows + fill < 2^24), so the result is `torch.equal` to the reference whatever the
           order of summation — overwrite, accumulate, split + reduce, capped or not.  This is what catches an index error of any size.
* `randn`  Gaussian operands with channel co of dy scaled by 2^-(co mod 11) and channel ci of x by 2^-(ci mod 7) (elements of dW span
           2^16 in size), held to the PER-ELEMENT bar dw_ref.dw_bar: (n + splits + 1) 2^-24 sum|dy x|, n = rows walked.  Derived, not
           measured; every case prints its worst ratio to it ("dwbar ..." lines).

Whenever `lens` is given, the dY rows at and past len_b hold NaN and the X rows there hold ordinary finite values (dwconv multiplies them
by zero): the kernels' contract is that `lens` masks dY only (tests/dw_ref.py).  Operands always sit in the middle of a larger NaN-filled
allocation, and an overwritten destination starts as NaN: a row read outside the operands, or a tile nobody wrote, is a value.

Shapes are the smallest tiles the kernels have (dwgemm 256 x 256, dwconv 256 x 32 per workgroup), S <= 288."""
import pytest
import torch

from tests.dw_ref import clamp_lens, dw_bar, dw_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
GUARD = 64                     # NaN rows in front of and behind every operand
BF16 = torch.bfloat16

# "both kernels": dwgemm at k = 1 and k = 5, dwconv at k = 9 — (kernel, k, Cout, Cin)
BOTH = [("dwgemm", 1, 256, 256), ("dwgemm", 5, 256, 256), ("dwconv", 9, 256, 64)]
BOTH_IDS = ["dwgemm-k1", "dwgemm-k5", "dwconv-k9"]
MODES = ["ints", "randn"]


# ---------------------------------------------------------------------------------------------------------------- operands

def operands(B, S, Cout, Cin, mode, seed):
    """Host (B, S, Cout), (B, S, Cin) bf16."""
    g = torch.Generator().manual_seed(seed)
    if mode == "ints":
        return (torch.randint(-3, 4, (B, S, Cout), generator=g).to(BF16), torch.randint(-3, 4, (B, S, Cin), generator=g).to(BF16))
    dy = torch.randn(B, S, Cout, generator=g) * 2.0 ** -(torch.arange(Cout) % 11).float()
    x = torch.randn(B, S, Cin, generator=g) * 2.0 ** -(torch.arange(Cin) % 7).float()
    return dy.to(BF16), x.to(BF16)


def dead_rows(dy, lens, value):
    """A copy of dy with the rows >= len_b set to `value` (lens None: dy itself)."""
    if lens is None:
        return dy
    out = dy.clone()
    for b, n in enumerate(clamp_lens(lens, dy.shape[0], dy.shape[1])):
        out[b, n:] = value
    return out


def on_device(t, extra_cols=0, col0=0):
    """The (B, S, C) host tensor as a device view in the middle of a NaN-filled (GUARD + B*S + GUARD, C + extra_cols) allocation, at
    column col0: utterances back to back, row pitch C + extra_cols."""
    B, S, Cn = t.shape
    buf = torch.full((GUARD + B * S + GUARD, Cn + extra_cols), NAN, dtype=t.dtype, device=DEV)
    v = buf[GUARD:GUARD + B * S, col0:col0 + Cn].unflatten(0, (B, S))
    v.copy_(t)
    assert v.stride(1) == Cn + extra_cols and v.stride(0) == S * v.stride(1)
    return v


def dev_lens(lens):
    return None if lens is None else torch.tensor([int(v) for v in lens], dtype=torch.int64, device=DEV)


def filled(shape, fill):
    """A destination: `fill` a number (NaN = poison) or a host tensor."""
    if torch.is_tensor(fill):
        return fill.to(DEV).clone()
    return torch.full(shape, float(fill), dtype=torch.float32, device=DEV)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- launches

def reduce_slabs(red):
    from tts_king_amd import lib as L
    if red:
        arr = (L.ReduceItem * len(red))(*[r for r, _ in red])
        L.check(L.load().ttsk_gemm_reduce_batch(arr, len(red), torch.cuda.current_stream().cuda_stream), "ttsk_gemm_reduce_batch")


def dwgemm(items, max_wgs=0):
    """ops.dwgemm_batch on [(dy, x, dst, lens, accumulate, splits)] and the slab sums of the split ones."""
    from tts_king_amd import ops
    reduce_slabs(ops.dwgemm_batch(items, max_wgs))
    torch.cuda.synchronize()


def dwgemm_poisoned_slabs(items, max_wgs=0):
    """One ttsk_dwgemm_batch launch as ops.dwgemm_batch makes it, but with the split problems' slabs filled with NaN beforehand
    (ops allocates them uninitialised: a tile nobody walked could keep an earlier launch's values there).  The packing below is a
    copy of ops.dwgemm_batch's (tts_king_amd/ops.py), the original: a change to DwGemmItem, ReduceItem or the reducer's arguments
    there has to be repeated here."""
    from tts_king_amd import lib as L
    lib = L.load()
    arr, red = (L.DwGemmItem * len(items))(), []
    for i, (dy, x, dst, lens, accumulate, splits) in enumerate(items):
        it = arr[i]
        (B, S, Cout), Cin, k = dy.shape, x.shape[2], dst.shape[1]
        ws = torch.full((splits * k * Cout * Cin,), NAN, dtype=torch.float32, device=DEV) if splits > 1 else None
        it.dy, it.x, it.dw, it.lens = dy.data_ptr(), x.data_ptr(), dst.data_ptr(), None if lens is None else lens.data_ptr()
        it.workspace = None if ws is None else ws.data_ptr()
        it.Cout, it.Cin, it.K, it.ldy, it.ldx, it.B, it.S = Cout, Cin, k, dy.stride(1), x.stride(1), B, S
        it.accumulate, it.splits = int(accumulate), splits
        if ws is not None:
            r = L.ReduceItem()
            r.ws, r.C, r.M, r.N, r.ldc, r.nz, r.splits = ws.data_ptr(), dst.data_ptr(), Cout, Cin, k * Cin, k, splits
            r.accumulate, r.sC2, r.alpha = int(accumulate), Cin, 1.0
            red.append((r, ws))
    L.check(lib.ttsk_dwgemm_batch(arr, len(items), int(max_wgs), torch.cuda.current_stream().cuda_stream), "ttsk_dwgemm_batch")
    reduce_slabs(red)
    torch.cuda.synchronize()


def launch(kern, dyd, xd, dst, lnd, accumulate=False, splits=1):
    from tts_king_amd import ops
    if kern == "dwconv":
        assert splits == 1
        ops.dwconv_batch([(dyd, xd, dst, lnd, accumulate)])
        torch.cuda.synchronize()
    else:
        dwgemm([(dyd, xd, dst, lnd, accumulate, splits)])
    return dst


# ---------------------------------------------------------------------------------------------------------------- the two checks

def compare(got, want, mode, bar, tag):
    """`ints`: torch.equal.  `randn`: |got - want| <= bar element by element (bar: a callable, evaluated only here); prints the
    worst ratio.  Finite either way."""
    got = got.detach().double().cpu()
    assert got.shape == want.shape, tag
    assert bool(torch.isfinite(got).all()), "%s: %d non-finite elements" % (tag, int((~torch.isfinite(got)).sum()))
    if mode == "ints":
        assert torch.equal(got, want), "%s: %d elements differ, max |diff| %g" % (tag, int((got != want).sum()), float((got - want).abs().max()))
        return
    b = bar()
    err = (got - want).abs()
    ratio = float((err[b > 0] / b[b > 0]).max()) if bool((b > 0).any()) else 0.0
    print("dwbar %s worst ratio to the bar %.4f" % (tag, ratio))
    assert bool((err <= b).all()), "%s: %d elements over the bar, worst ratio %.3f" % (tag, int((err > b).sum()), ratio)


def verify(kern, k, dy, x, lens, mode, tag, splits=1, dyd=None, xd=None):
    """Overwrite into a NaN destination and accumulate onto a filled one, both against the reference.  dy carries NaN at its dead
    rows already (or lens is None).  Returns the overwritten destination."""
    Cout, Cin = dy.shape[2], x.shape[2]
    want = dw_ref(dy, x, k, lens)
    dyd = on_device(dy) if dyd is None else dyd
    xd = on_device(x) if xd is None else xd
    lnd = dev_lens(lens)
    tag = "%s k=%d B=%d S=%d lens=%s splits=%d %s %s" % (kern, k, dy.shape[0], dy.shape[1], lens, splits, mode, tag)
    out = launch(kern, dyd, xd, filled((Cout, k, Cin), NAN), lnd, False, splits)
    compare(out, want, mode, lambda: dw_bar(dy, x, k, lens, splits), tag + " overwrite")
    if mode == "ints":
        acc = launch(kern, dyd, xd, filled((Cout, k, Cin), 5.0), lnd, True, splits)
        compare(acc, want + 5.0, mode, None, tag + " accumulate")
    else:
        old = torch.randn(Cout, k, Cin, generator=torch.Generator().manual_seed(k)) * float(want.abs().mean() + 1e-3)
        acc = launch(kern, dyd, xd, filled(None, old), lnd, True, splits)
        compare(acc, want + old.double(), mode, lambda: dw_bar(dy, x, k, lens, splits, old.double().abs()), tag + " accumulate")
    return out


def refused(call, match, *poisoned):
    """`call` raises TtskError naming the reason, and every poisoned destination still holds its fill (7.0) afterwards."""
    from tts_king_amd import lib as L
    with pytest.raises(L.TtskError, match=match):
        call()
    torch.cuda.synchronize()
    for t in poisoned:
        assert bool((t == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- A. lens, observed

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kern,k,Cout,Cin", BOTH, ids=BOTH_IDS)
def test_lens_skip_observed(kern, k, Cout, Cin, mode):
    """dY rows at and past len_b are NaN, X rows there are finite and non-trivial: the result is finite, equals the reference (which
    masks dY only), and equals bit for bit the same call with those dY rows zeroed.  [45, 13, 40] of 45: a part-filled last K step in
    the first utterance (45 = 32 + 13), a part-filled only step, and a part-filled LAST utterance (a read past its end leaves the
    tensor for the NaN rows behind it); [64, 33] of 64: a last utterance whose second step holds one row."""
    for B, S, lens in [(3, 45, [45, 13, 40]), (2, 64, [64, 33])]:
        dy, x = operands(B, S, Cout, Cin, mode, seed=100 + k + S)
        dyn = dead_rows(dy, lens, NAN)
        xd = on_device(x)
        out = verify(kern, k, dyn, x, lens, mode, "A", xd=xd)
        zeroed = launch(kern, on_device(dead_rows(dy, lens, 0.0)), xd, filled((Cout, k, Cin), NAN), dev_lens(lens))
        assert same_bits(out, zeroed)
        # and the X rows [len, len + k//2) did take part: the reference with them zeroed differs wherever k > 1
        if k > 1:
            xz = dead_rows(x, lens, 0.0)
            assert not torch.equal(dw_ref(dyn, xz, k, lens), dw_ref(dyn, x, k, lens))


# ---------------------------------------------------------------------------------------------------------------- B. K steps, lengths

SWEEP = [1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 161, 256, 288]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kern,k,Cout,Cin", BOTH, ids=BOTH_IDS)
def test_k_step_counts(kern, k, Cout, Cin, mode):
    """One utterance of 288 rows, lens swept over 1 .. 9 K steps (32 rows each), odd and even, full and part-filled last steps, below
    and above the prologue depth (dwgemm loads four steps ahead, dwconv three; odd counts get a phantom step of zeros).  One
    allocation; only `lens` and the NaN rows of dY change."""
    S = 288
    dy, x = operands(1, S, Cout, Cin, mode, seed=200 + k)
    dyd, xd = on_device(dy), on_device(x)
    pristine = dyd.clone()
    for n in SWEEP:
        dyd.copy_(pristine)
        dyd[0, n:] = NAN
        verify(kern, k, dead_rows(dy, [n], NAN), x, [n], mode, "B steps=%d" % ((n + 31) // 32), dyd=dyd, xd=xd)


PATTERNS = [[70, 0, 32, 1, 33, 64], [0, 0, 5, 70, 0, 0], [0, 0, 0, 0, 0, 70], [1000, -3, 70, 71, 69, 0], None]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kern,k,Cout,Cin", BOTH, ids=BOTH_IDS)
def test_length_patterns(kern, k, Cout, Cin, mode):
    """Six utterances of 70 rows: empty ones in front, between and behind, exact multiples of the K step and one past it, lens beyond
    S and below zero (the kernels clamp to [0, S]), and no lens at all."""
    B, S = 6, 70
    dy, x = operands(B, S, Cout, Cin, mode, seed=300 + k)
    xd = on_device(x)
    for lens in PATTERNS:
        verify(kern, k, dead_rows(dy, lens, NAN), x, lens, mode, "B", xd=xd)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("S", [7, 33])
def test_dwgemm_taps_against_short_utterances(S, k, mode):
    """Taps wider than the utterance is long (k = 15 at S = 7: the outer taps see nothing but padding), and the largest k
    ttsk_dwgemm_supported admits."""
    from tts_king_amd import ops
    assert ops.dwgemm_supported(256, 256, k) and not ops.dwgemm_supported(256, 256, 17)
    dy, x = operands(3, S, 256, 256, mode, seed=400 + k + S)
    xd = on_device(x)
    for lens in (None, [S, S // 2, 1]):
        verify("dwgemm", k, dead_rows(dy, lens, NAN), x, lens, mode, "B", xd=xd)


# ---------------------------------------------------------------------------------------------------------------- C. nothing to add

@pytest.mark.parametrize("kern,k,Cout,Cin", BOTH, ids=BOTH_IDS)
def test_nothing_to_add(kern, k, Cout, Cin):
    """All lens zero (no K step at all): overwrite stores exact zeros everywhere, accumulate leaves a random destination bit-identical."""
    B, S = 3, 40
    dy, x = operands(B, S, Cout, Cin, "randn", seed=500 + k)
    lens = [0, 0, 0]
    dyd, xd, lnd = on_device(dead_rows(dy, lens, NAN)), on_device(x), dev_lens(lens)
    out = launch(kern, dyd, xd, filled((Cout, k, Cin), NAN), lnd)
    assert torch.equal(out, torch.zeros_like(out))
    old = torch.randn(Cout, k, Cin, generator=torch.Generator().manual_seed(k))
    acc = launch(kern, dyd, xd, filled(None, old), lnd, True)
    assert same_bits(acc, old.to(DEV))
    if kern == "dwgemm":
        for splits in (2, 3):
            out = launch(kern, dyd, xd, filled((Cout, k, Cin), NAN), lnd, False, splits)
            assert torch.equal(out, torch.zeros_like(out))
            acc = launch(kern, dyd, xd, filled(None, old), lnd, True, splits)
            assert same_bits(acc, old.to(DEV))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [1, 5])
def test_dwgemm_split_with_an_empty_range(k, mode):
    """splits > 1 where one whole utterance range walks nothing: its slab is zeros, the sum is the other ranges'."""
    B, S = 4, 40
    dy, x = operands(B, S, 256, 256, mode, seed=520 + k)
    xd = on_device(x)
    for lens, splits in [([0, 0, 40, 5], 2), ([33, 7, 0, 0], 2), ([9, 0, 0, 40], 4)]:
        verify("dwgemm", k, dead_rows(dy, lens, NAN), x, lens, mode, "C", splits=splits, xd=xd)


# ---------------------------------------------------------------------------------------------------------------- D. 64 utterances

def ragged(B, S):
    """Ragged lens with empty utterances in front and inside, and a full last one (the last lane of the table)."""
    lens = [0 if i % 9 == 0 else (7 * i + 3) % (S + 1) for i in range(B)]
    lens[B - 1] = S
    return lens


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S", [5, 40])
@pytest.mark.parametrize("kern,k,Cout,Cin", BOTH, ids=BOTH_IDS)
def test_64_utterances(kern, k, Cout, Cin, S, mode):
    """B = 64 in one range: every lane of the per-lane utterance table holds an utterance."""
    B = 64
    dy, x = operands(B, S, Cout, Cin, mode, seed=600 + k + S)
    lens = ragged(B, S)
    verify(kern, k, dead_rows(dy, lens, NAN), x, lens, mode, "D")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [1, 5])
def test_dwgemm_130_utterances_in_3_ranges(k, mode):
    """B = 130 with splits = 3: ranges of 43 / 43 / 44 utterances (floor(s * 130 / 3) boundaries), each with its own lane table."""
    B, S = 130, 9
    dy, x = operands(B, S, 256, 256, mode, seed=650 + k)
    lens = ragged(B, S)
    verify("dwgemm", k, dead_rows(dy, lens, NAN), x, lens, mode, "D", splits=3)


def test_65_utterances_refused():
    from tts_king_amd import ops
    dy, x = operands(65, 5, 256, 256, "ints", seed=660)
    dyd, xd = on_device(dy), on_device(x)
    dst = filled((256, 1, 256), 7.0)
    refused(lambda: ops.dwgemm_batch([(dyd, xd, dst, None, False, 1)]), "at most 64 per split", dst)
    dst9 = filled((256, 9, 64), 7.0)
    xc = on_device(x[:, :, :64].contiguous())
    refused(lambda: ops.dwconv_batch([(dyd, xc, dst9, None, False)]), "1..64 utterances", dst9)
    dwgemm([(dyd, xd, dst, None, False, 2)])                                  # 33 + 32: fine
    compare(dst, dw_ref(dy, x, 1), "ints", None, "dwgemm B=65 splits=2")


# ---------------------------------------------------------------------------------------------------------------- E. row pitches

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kern,k,Cout,Cin", BOTH, ids=BOTH_IDS)
def test_row_pitches(kern, k, Cout, Cin, mode):
    """dy, x as channel slices of wider NaN-filled buffers (ldy = Cout + 256, ldx = Cin + 64, origin at a non-zero, 16-byte aligned
    column): bit for bit the result of the same data in contiguous tensors, and the reference's."""
    B, S, lens = 3, 45, [45, 13, 40]
    dy, x = operands(B, S, Cout, Cin, mode, seed=700 + k)
    dyn = dead_rows(dy, lens, NAN)
    dyp, xp = on_device(dyn, 256, 136), on_device(x, 64, 24)
    assert dyp.stride(1) == Cout + 256 and xp.stride(1) == Cin + 64 and dyp.data_ptr() % 16 == 0 and xp.data_ptr() % 16 == 0
    out = verify(kern, k, dyn, x, lens, mode, "E pitched", dyd=dyp, xd=xp)
    flat = launch(kern, on_device(dyn), on_device(x), filled((Cout, k, Cin), NAN), dev_lens(lens))
    assert same_bits(out, flat)
    if kern == "dwgemm":
        out3 = launch(kern, dyp, xp, filled((Cout, k, Cin), NAN), dev_lens(lens), False, 3)
        flat3 = launch(kern, on_device(dyn), on_device(x), filled((Cout, k, Cin), NAN), dev_lens(lens), False, 3)
        assert same_bits(out3, flat3)


def test_refusals_by_name():
    """What neither kernel has an instance or an addressing mode for is refused with the reason, before anything is launched."""
    from tts_king_amd import ops
    B, S = 2, 8
    dy, x = operands(B, S, 256, 256, "ints", seed=720)
    dyd, xd = on_device(dy), on_device(x)
    x64 = on_device(x[:, :, :64].contiguous())
    g1, c9 = filled((256, 1, 256), 7.0), filled((256, 9, 64), 7.0)
    gemm = lambda dyv, xv, dst=g1: (lambda: ops.dwgemm_batch([(dyv, xv, dst, None, False, 1)]))
    conv = lambda dyv, xv, dst=c9: (lambda: ops.dwconv_batch([(dyv, xv, dst, None, False)]))
    # a pitch that is no multiple of 8 elements
    refused(gemm(on_device(dy, 4), xd), "row pitches", g1)
    refused(gemm(dyd, on_device(x, 12)), "row pitches", g1)
    refused(conv(on_device(dy, 4), x64), "row pitches", c9)
    refused(conv(dyd, on_device(x[:, :, :64].contiguous(), 12)), "row pitches", c9)
    # an origin that is 8-byte but not 16-byte aligned
    odd_dy, odd_x, odd_x64 = on_device(dy, 8, 4), on_device(x, 8, 4), on_device(x[:, :, :64].contiguous(), 8, 4)
    assert odd_dy.data_ptr() % 16 == 8 and odd_x.data_ptr() % 16 == 8 and odd_x64.data_ptr() % 16 == 8
    refused(gemm(odd_dy, xd), "16-byte alignment", g1)
    refused(gemm(dyd, odd_x), "16-byte alignment", g1)
    refused(conv(odd_dy, x64), "16-byte alignment", c9)
    refused(conv(dyd, odd_x64), "16-byte alignment", c9)
    # channel counts without an instance
    assert not ops.dwconv_supported(256, 48, 9) and not ops.dwgemm_supported(256, 128, 1) and not ops.dwgemm_supported(128, 256, 1)
    c48, g128 = filled((256, 9, 48), 7.0), filled((256, 1, 128), 7.0)
    refused(conv(dyd, on_device(x[:, :, :48].contiguous()), c48), "no instance for Cout=256 Cin=48 K=9", c48)
    refused(gemm(dyd, on_device(x[:, :, :128].contiguous()), g128), "no instance for Cout=256 Cin=128 K=1", g128)
    # kernel sizes: even, and for dwconv anything but 9
    assert not ops.dwgemm_supported(256, 256, 4) and not ops.dwconv_supported(256, 64, 4) and not ops.dwconv_supported(256, 64, 5)
    g4, c4, c5 = filled((256, 4, 256), 7.0), filled((256, 4, 64), 7.0), filled((256, 5, 64), 7.0)
    refused(gemm(dyd, xd, g4), "no instance for Cout=256 Cin=256 K=4", g4)
    refused(conv(dyd, x64, c4), "no instance for Cout=256 Cin=64 K=4", c4)
    refused(conv(dyd, x64, c5), "no instance for Cout=256 Cin=64 K=5", c5)


# ---------------------------------------------------------------------------------------------------------------- F. many problems

def solo_and_batched(problems, mode, kern):
    """problems: [(Cout, Cin, k, B, S, lens, splits, accumulate)].  Builds each on the device with its own destination fill, runs each
    alone and all in one call: every destination of the one call is bit-identical to its solo run and holds the reference's values."""
    from tts_king_amd import ops
    built = []
    for i, (Cout, Cin, k, B, S, lens, splits, accumulate) in enumerate(problems):
        dy, x = operands(B, S, Cout, Cin, mode, seed=800 + i)
        dyn = dead_rows(dy, lens, NAN)
        if not accumulate:
            old = None
        elif mode == "ints":
            old = torch.full((Cout, k, Cin), float(i + 2))
        else:
            old = torch.randn(Cout, k, Cin, generator=torch.Generator().manual_seed(i))
        built.append((dyn, x, on_device(dyn), on_device(x), dev_lens(lens), old))
    def items(dsts):
        out = []
        for (Cout, Cin, k, B, S, lens, splits, accumulate), (dyn, x, dyd, xd, lnd, old), dst in zip(problems, built, dsts):
            out.append((dyd, xd, dst, lnd, accumulate) + ((splits,) if kern == "dwgemm" else ()))
        return out
    fresh = lambda: [filled((p[0], p[2], p[1]), NAN if b[5] is None else b[5]) for p, b in zip(problems, built)]
    run = (lambda its: dwgemm(its)) if kern == "dwgemm" else (lambda its: (ops.dwconv_batch(its), torch.cuda.synchronize()))
    solo = fresh()
    for it in items(solo):
        run([it])
    counts = {}
    ops.LAUNCH_COUNTS = counts
    try:
        together = fresh()
        run(items(together))
    finally:
        ops.LAUNCH_COUNTS = None
    assert counts.get(kern) == 1, counts
    for i, ((Cout, Cin, k, B, S, lens, splits, accumulate), (dyn, x, dyd, xd, lnd, old), a, b) in enumerate(zip(problems, built, solo, together)):
        tag = "%s problem %d of %d: %dx%d k=%d B=%d S=%d lens=%s splits=%d acc=%d %s" % (kern, i, len(problems), Cout, Cin, k, B, S, lens, splits, accumulate, mode)
        assert same_bits(a, b), tag
        want = dw_ref(dyn, x, k, lens) + (0.0 if old is None else old.double())
        compare(b, want, mode, lambda: dw_bar(dyn, x, k, lens, splits, 0.0 if old is None else old.double().abs()), tag)


@pytest.mark.parametrize("mode", MODES)
def test_dwgemm_six_different_problems_in_one_launch(mode):
    solo_and_batched([(256, 256, 1, 3, 40, [40, 7, 33], 1, False),
                      (512, 256, 3, 2, 33, None, 2, True),
                      (256, 512, 5, 5, 20, [0, 20, 3, 0, 11], 3, False),
                      (512, 512, 1, 1, 70, [65], 1, True),
                      (256, 256, 5, 4, 64, [64, 32, 0, 1], 2, True),
                      (512, 256, 3, 7, 9, None, 3, False)], mode, "dwgemm")


@pytest.mark.parametrize("mode", MODES)
def test_dwconv_twelve_different_problems_in_one_launch(mode):
    problems = []
    for i in range(12):
        B, S = 1 + (i * 3) % 5, [7, 33, 40, 70][i % 4]
        lens = None if i % 4 == 0 else [(i * 7 + b * 13) % (S + 1) for b in range(B)]
        problems.append(([256, 512][i % 2], [32, 64, 96][i % 3], 9, B, S, lens, 1, i % 3 == 1))
    assert {(p[0], p[1]) for p in problems} == {(co, ci) for co in (256, 512) for ci in (32, 64, 96)}
    solo_and_batched(problems, mode, "dwconv")


def test_dwgemm_thirty_problems_make_two_launches():
    """ops.dwgemm_batch cuts its list into launches of 28 problems (DWG_MAXP): 30 make two, and the 29th and 30th are as right as the first."""
    from tts_king_amd import ops
    n, S = 30, 8
    dy, x = operands(n, S, 256, 256, "ints", seed=900)
    dyd, xd = on_device(dy), on_device(x)
    dsts = [filled((256, 1, 256), NAN) for _ in range(n)]
    counts = {}
    ops.LAUNCH_COUNTS = counts
    try:
        dwgemm([(dyd[i:i + 1], xd[i:i + 1], dsts[i], None, False, 1) for i in range(n)])
    finally:
        ops.LAUNCH_COUNTS = None
    assert counts == {"dwgemm": 2}
    for i in range(n):
        compare(dsts[i], dw_ref(dy[i:i + 1], x[i:i + 1], 1), "ints", None, "dwgemm problem %d of 30" % i)


def test_dwconv_thirteen_problems():
    """DeferQueue.flush_dwconv cuts its queue into launches of 12 problems (DWC_MAXP): 13 make two.  A direct 13-item dwconv_batch is
    refused by name."""
    from tts_king_amd import ops
    n, S = 13, 8
    dy, x = operands(n, S, 256, 32, "ints", seed=910)
    dyd, xd = on_device(dy), on_device(x)
    dsts = [filled((256, 9, 32), 7.0) for _ in range(n)]
    its = [(dyd[i:i + 1], xd[i:i + 1], dsts[i], None, False) for i in range(n)]
    refused(lambda: ops.dwconv_batch(its), r"1\.\.12 items", *dsts)
    q = ops.DeferQueue()
    q.dwconv.extend(its)
    counts = {}
    ops.LAUNCH_COUNTS = counts
    try:
        q.flush_dwconv()
        torch.cuda.synchronize()
    finally:
        ops.LAUNCH_COUNTS = None
    assert counts == {"dwconv": 2} and not q.dwconv
    for i in range(n):
        compare(dsts[i], dw_ref(dy[i:i + 1], x[i:i + 1], 9), "ints", None, "dwconv problem %d of 13" % i)


# ---------------------------------------------------------------------------------------------------------------- G. capped grid

# name -> [(Cout, Cin, k, B, S, lens, splits, accumulate)], tile total
CAPPED = {"T30": ([(512, 256, 5, 5, 40, [40, 0, 33, 17, 40], 3, False)], 30),
          "T13": ([(256, 256, 5, 3, 33, [33, 1, 20], 1, True), (256, 512, 1, 6, 40, None, 4, False)], 13)}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(CAPPED))
def test_dwgemm_capped_grid(name, mode):
    """max_wgs < tiles: a workgroup walks tiles w, w + G, ... through the XCD-major remap of a total that is no multiple of 8, with a
    barrier between tiles.  Every destination (slab sums included, from NaN-poisoned slabs) is bit-identical to the uncapped launch's
    and holds the reference's values."""
    problems, T = CAPPED[name]
    assert T % 8 != 0 and T == sum((co // 256) * (ci // 256) * k * sp for co, ci, k, _, _, _, sp, _ in problems)
    built = []
    for i, (Cout, Cin, k, B, S, lens, splits, accumulate) in enumerate(problems):
        dy, x = operands(B, S, Cout, Cin, mode, seed=1000 + i)
        dyn = dead_rows(dy, lens, NAN)
        old = None if not accumulate else (torch.full((Cout, k, Cin), 4.0) if mode == "ints" else torch.randn(Cout, k, Cin, generator=torch.Generator().manual_seed(i)))
        built.append((dyn, x, on_device(dyn), on_device(x), dev_lens(lens), old))
    def run(max_wgs):
        dsts = [filled((p[0], p[2], p[1]), NAN if b[5] is None else b[5]) for p, b in zip(problems, built)]
        dwgemm_poisoned_slabs([(b[2], b[3], d, b[4], p[7], p[6]) for p, b, d in zip(problems, built, dsts)], max_wgs)
        return dsts
    base = run(0)
    for (Cout, Cin, k, B, S, lens, splits, accumulate), (dyn, x, _, _, _, old), d in zip(problems, built, base):
        want = dw_ref(dyn, x, k, lens) + (0.0 if old is None else old.double())
        compare(d, want, mode, lambda: dw_bar(dyn, x, k, lens, splits, 0.0 if old is None else old.double().abs()), "G %s %dx%d k=%d uncapped" % (name, Cout, Cin, k))
    for max_wgs in (1, 3, 7, 8, T - 1, T, T + 1):
        for i, (a, b) in enumerate(zip(base, run(max_wgs))):
            assert same_bits(a, b), "%s problem %d: max_wgs=%d differs from the uncapped launch" % (name, i, max_wgs)


# ---------------------------------------------------------------------------------------------------------------- H. same bits twice

@pytest.mark.parametrize("kern,k,Cout,Cin", BOTH, ids=BOTH_IDS)
def test_same_bits_twice(kern, k, Cout, Cin):
    """Run to run, into fresh destinations: bit-identical — unsplit, and (dwgemm) split + reduce.  The split sum need not equal the
    unsplit one bit for bit (another order of the same terms), only stay inside the bar."""
    B, S, lens = 5, 70, [70, 33, 0, 64, 9]
    dy, x = operands(B, S, Cout, Cin, "randn", seed=1100 + k)
    dyn = dead_rows(dy, lens, NAN)
    dyd, xd, lnd = on_device(dyn), on_device(x), dev_lens(lens)
    for splits in ((1, 2, 5) if kern == "dwgemm" else (1,)):
        a = launch(kern, dyd, xd, filled((Cout, k, Cin), NAN), lnd, False, splits)
        b = launch(kern, dyd, xd, filled((Cout, k, Cin), NAN), lnd, False, splits)
        assert same_bits(a, b), "splits=%d" % splits
        compare(a, dw_ref(dyn, x, k, lens), "randn", lambda: dw_bar(dyn, x, k, lens, splits), "H %s k=%d splits=%d" % (kern, k, splits))
