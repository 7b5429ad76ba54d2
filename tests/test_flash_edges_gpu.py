"""GPU: flash attention (tts_king_amd/csrc/flash_attn.hip) where tests/test_attention_gpu.py does not look — the XCD workgroup remap
(B*H a multiple of 8), peaked scores (a trained model's attention, not random weights'), key lengths 0, 1, 2 and both sides of the
64- and 128-key seams, sequence lengths 1, 63, 65, 128, 129, a dominant key in every key tile, the delta-given entry, determinism.
Reference, inputs, metrics and the list of cases are tests/flash_ref.py; tests/test_flash_ref_cpu.py shows that the bf16 roundings a
correct kernel must make use at most half of each bar below on every case here, and that five typical defects exceed them.

Bars (those of test_attention_gpu.py, per (batch, head) slab / per query row instead of over the whole tensor):
  O             slab_err <= 0.02; peaked and planted cases also row_err <= 0.02
  dQ, dK, dV    slab_err <= 0.03 with delta from the fp32 O, <= 0.04 with delta from the bf16 O
  LSE           |err| <= 2e-3 * max(1, |lse| / 8)
Every test prints its figures as shares of these bars (pytest -s); DESIGN.md section 4.1 keeps the measured ones."""
import pytest
import torch

from tests import flash_ref as fr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


def _fmt(sh):
    return "  ".join("%s %.3f" % (k, v) for k, v in sh.items())


def _run(qkv, do, lens, B, H, S, o32_delta=True, delta=None):
    """forward + backward on the GPU -> dict of CPU tensors (O, o32, LSE, dQ, dK, dV, dqkv), kernel layouts."""
    from tts_king_amd import ops
    q, g, ln = qkv.to(DEV), do.to(DEV), lens.to(DEV)
    o, lse, o32 = ops.flash_attention_fwd(q, ln, B, H, S, want_lse=True)
    dqkv = ops.flash_attention_bwd(q, o, g, lse, ln, B, H, S, o32=o32 if o32_delta else None, delta=delta)
    torch.cuda.synchronize()
    d = H * fr.DK
    dqkv = dqkv.cpu()
    return {"O": o.cpu(), "o32": o32.cpu(), "LSE": lse.cpu(), "dqkv": dqkv, "dQ": dqkv[:, :d], "dK": dqkv[:, d:2 * d], "dV": dqkv[:, 2 * d:]}


def _check_case(name, row_bar):
    """The case against the fp64 reference under every bar, with delta from the fp32 O and from the bf16 O.  -> the first run's outputs."""
    B, H, S = fr.CASES[name][:3]
    (qkv, do, lens), ref = fr.case_reference(name)
    got = _run(qkv, do, lens, B, H, S)
    assert torch.equal(got["o32"].to(BF), got["O"])                 # the fp32 copy the backward's delta is taken from
    for n in ("O", "o32", "LSE", "dqkv"):
        assert bool(torch.isfinite(got[n].float()).all()), (name, n)
    sh = fr.shares(got, ref, lens, B, H, S, row_bar=row_bar)
    print("flash vs fp64, share of bar  %-24s delta from o32   %s" % (name, _fmt(sh)))
    assert max(sh.values()) <= 1.0, (name, sh)
    got_b = _run(qkv, do, lens, B, H, S, o32_delta=False)
    sh_b = fr.shares({n: got_b[n] for n in ("O", "dQ", "dK", "dV")}, ref, lens, B, H, S, bar_grad=fr.BAR_GRAD_BF16_DELTA, row_bar=row_bar)
    print("flash vs fp64, share of bar  %-24s delta from bf16  %s" % (name, _fmt(sh_b)))
    assert max(sh_b.values()) <= 1.0, (name, sh_b)
    # keys past the utterance: exactly zero dK / dV; an utterance without keys: exactly zero everywhere, LSE included
    lens_c = lens.clamp(min=0, max=S)
    for b in range(B):
        n = int(lens_c[b])
        for g_ in (got, got_b):
            if n < S:
                assert float(g_["dqkv"][b * S + n:(b + 1) * S, H * fr.DK:].float().abs().max()) == 0.0, (name, b)
            if n == 0:
                for t in ("O", "o32", "dqkv"):
                    assert float(g_[t][b * S:(b + 1) * S].float().abs().max()) == 0.0, (name, b, t)
                assert float(g_["LSE"][b * H:(b + 1) * H].abs().max()) == 0.0, (name, b)
    return got


XCD_SHAPES = [(4, 2, 130), (8, 2, 65), (8, 1, 64), (4, 4, 129), (3, 2, 130)]


@pytest.mark.parametrize("regime", ["uniform", "planted"])
@pytest.mark.parametrize("B,H,S", XCD_SHAPES)
def test_xcd_remap_vs_fp64(B, H, S, regime):
    """xcd_tile()'s bijective branch (B*H % 8 == 0) with 3, 2, 1 and 3 tiles per (batch, head), and the plain order (B*H = 6) beside it.
    Every utterance has its own length: a tile sent to the wrong (b, h) has the wrong data AND the wrong mask."""
    assert ((B * H) % 8 == 0) == ((B, H, S) != (3, 2, 130))
    lens = fr.CASES["xcd-%dx%dx%d-%s" % (B, H, S, regime)][3]
    assert len(set(lens)) == B
    _check_case("xcd-%dx%dx%d-%s" % (B, H, S, regime), row_bar=regime != "uniform")


@pytest.mark.parametrize("B,H,S,parts", [(4, 2, 130, (2, 2)), (8, 1, 64, (5, 3))])
def test_xcd_remap_equals_plain_order_bit_for_bit(B, H, S, parts):
    """The remapped grid computes exactly what plain-order grids compute on the same utterances: the whole batch (B*H = 8) against the
    same batch as two calls whose B*H is no multiple of 8."""
    name = "xcd-%dx%dx%d-planted" % (B, H, S)
    (qkv, do, lens), _ = fr.case_reference(name)
    whole = _run(qkv, do, lens, B, H, S)
    b0 = 0
    for nb in parts:
        assert (nb * H) % 8 != 0
        part = _run(qkv[b0 * S:(b0 + nb) * S], do[b0 * S:(b0 + nb) * S], lens[b0:b0 + nb], nb, H, S)
        for n in ("O", "o32", "dqkv"):
            assert torch.equal(whole[n][b0 * S:(b0 + nb) * S], part[n]), (n, b0)
        assert torch.equal(whole["LSE"][b0 * H:(b0 + nb) * H], part["LSE"]), b0
        b0 += nb
    assert b0 == B


@pytest.mark.parametrize("regime", fr.REGIMES)
@pytest.mark.parametrize("heads", [1, 2])
def test_key_length_edges(heads, regime):
    """lens = 0, 1, 2, 63 | 64 | 65, 127 | 128 | 129, 199, 200 at S = 200 (H = 1), and 1, 64, 65, 200 with two heads: whole key tiles
    unvisited by the forward while the key side of the backward still writes their zeros; the empty utterance; one and two keys."""
    name = "keylen-h%d-%s" % (heads, regime)
    lens = fr.CASES[name][3]
    assert lens == (fr.KEY_LENS_H1 if heads == 1 else fr.KEY_LENS_H2)
    _check_case(name, row_bar=regime != "uniform")


@pytest.mark.parametrize("S", fr.SEQ_EDGES)
def test_sequence_length_edges(S):
    """S = 1 (one query, one key), 63, 65 (a second query tile of ONE row), 128, 129; lens = [S, max(1, S // 3)], planted keys."""
    assert fr.CASES["seq-%d" % S][:4] == (2, 2, S, [S, max(1, S // 3)])
    _check_case("seq-%d" % S, row_bar=True)


@pytest.mark.parametrize("S", [70, 200])
def test_one_key_is_exact(S):
    """An utterance with ONE key: every softmax is exactly 1, so O is v[0] to the bit, LSE is the score, dV[0] is the column sum of dO
    and dQ, dK vanish (dS = P (dP - delta) with dP = delta)."""
    name = "onekey-%d" % S
    B, H, S_, lens = fr.CASES[name][:4]
    assert S_ == S and lens[1] == 1
    (qkv, do, _), ref = fr.case_reference(name)
    got = _check_case(name, row_bar=True)
    d = H * fr.DK
    b = 1
    rows = slice(b * S, (b + 1) * S)
    v0 = qkv[b * S, 2 * d:]
    assert torch.equal(got["O"][rows], v0[None, :].expand(S, d))
    assert torch.equal(got["o32"][rows], v0.float()[None, :].expand(S, d))
    q, k, _ = fr._split(qkv.float(), B, H, S)
    score = (q[b] * k[b, :, :1]).sum(-1) * torch.tensor(fr.DK ** -0.5)          # fp32 (H, S)
    ex = fr.lse_excess(got["LSE"][b * H:(b + 1) * H], score)
    print("one key, S = %d: LSE vs the fp32 score %.4f of its bar" % (S, ex))
    assert ex <= 1.0
    dv0, want = got["dV"][b * S].double(), do[rows].double().sum(0)
    # one rounding to bf16 (2^-8 relative covers round-to-nearest and truncation) on top of an fp32 sum of S terms
    slack = 2.0 ** -8 * want.abs() + 2.0 ** -20 * do[rows].double().abs().sum(0)
    assert bool(((dv0 - want).abs() <= slack).all()), float(((dv0 - want).abs() / slack).max())
    mdv = float(got["dV"][rows].float().abs().max())
    mdq, mdk = float(got["dQ"][rows].float().abs().max()), float(got["dK"][rows].float().abs().max())
    print("one key, S = %d: max|dQ| %.3g  max|dK| %.3g  max|dV| %.3g" % (S, mdq, mdk, mdv))
    assert mdq <= 1e-3 * mdv and mdk <= 1e-3 * mdv


def test_masked_keys_do_not_matter_bit_for_bit():
    """K and V rows at keys >= lens[b] are multiplied by an exact zero: large finite values there (K x 64, V = +-3e4) change nothing, to
    the bit.  (Inf or NaN there would: 0 * Inf inside the P V MFMA is NaN by construction; ttsk.h requires finite rows.)  And lens beyond S
    mean S."""
    name = "masked-keys"
    B, H, S, lens = fr.CASES[name][:4]
    (qkv, do, lens_t), _ = fr.case_reference(name)
    got = _check_case(name, row_bar=True)
    d = H * fr.DK
    x = qkv.float().clone().view(B, S, 3 * d)
    g = torch.Generator().manual_seed(9)
    for b in range(B):
        n = lens[b]
        x[b, n:, d:2 * d] *= 64.0
        x[b, n:, 2 * d:] = torch.where(torch.rand(S - n, d, generator=g) < 0.5, -3e4, 3e4)
    loud = x.view(B * S, 3 * d).to(BF)
    assert bool(torch.isfinite(loud.float()).all()) and not torch.equal(loud, qkv) and float(loud.float().abs().max()) > 2.9e4
    got2 = _run(loud, do, lens_t, B, H, S)
    for n in ("O", "o32", "LSE"):
        assert torch.equal(got[n], got2[n]), n
    assert torch.equal(got["dQ"], got2["dQ"])
    for b in range(B):
        live = slice(b * S, b * S + lens[b])
        assert torch.equal(got["dqkv"][live], got2["dqkv"][live]), b
        if lens[b] < S:
            assert float(got2["dqkv"][b * S + lens[b]:(b + 1) * S, d:].float().abs().max()) == 0.0, b
    # lens beyond S are clamped by the kernel
    full = _run(qkv, do, torch.full((B,), S, dtype=torch.int64), B, H, S)
    over = _run(qkv, do, torch.full((B,), S + 50, dtype=torch.int64), B, H, S)
    for n in ("O", "o32", "LSE", "dqkv"):
        assert torch.equal(full[n], over[n]), n


def test_peak_position_in_every_tile():
    """S = 200, every key live; eight query rows with a dominant key each: query tile t peaking in key tile t (first key of the first
    tile ... last key of the last tile) and in a tile far from its own.  A peak in the last tile rescales everything accumulated before
    it by ~ e^-80; after a peak in the first tile every later p underflows.  Judged on exactly those rows."""
    name = "peaks"
    B, H, S = fr.CASES[name][:3]
    _, ref = fr.case_reference(name)
    got = _check_case(name, row_bar=True)
    rows = [r for r, _ in fr.PEAK_PAIRS]
    re = fr.row_err(got["O"], ref["O"], B, H, S, rows=rows)
    print("peak rows: O row_err %.4f (%.3f of its bar)" % (re, re / fr.BAR_O_ROW))
    assert re <= fr.BAR_O_ROW
    # the rows really are what the test is about: the reference puts nearly all of each row's weight on its key
    (qkv, _, lens), _ = fr.case_reference(name)
    P, _, _ = fr.ref_attention(qkv.float(), lens, B, H, S)
    for r, k in fr.PEAK_PAIRS:
        assert float(P[:, r, k].min()) > 0.999, (r, k)
    ex = fr.lse_excess(got["LSE"][:, rows], ref["LSE"][:, rows])
    print("peak rows: LSE %.4f of its bar" % ex)
    assert ex <= 1.0


@pytest.mark.parametrize("regime", ["uniform", "peaked"])
def test_delta_given_equals_delta_computed(regime):
    """delta handed in (delta_ready = 1: what ttsk_win_conv's epilogue does in a train step) against delta computed by the kernel's own
    launch: both meet the bars, and differ from each other by summation order only."""
    name = "delta-given-" + regime
    B, H, S = fr.CASES[name][:3]
    (qkv, do, lens), ref = fr.case_reference(name)
    got = _check_case(name, row_bar=regime != "uniform")
    delta = (do.float() * got["o32"]).view(B, S, H, fr.DK).sum(-1).permute(0, 2, 1).reshape(B * H, S).contiguous()
    given = _run(qkv, do, lens, B, H, S, delta=delta.to(DEV))
    assert torch.equal(given["O"], got["O"]) and torch.equal(given["LSE"], got["LSE"])
    sh = fr.shares({n: given[n] for n in ("dQ", "dK", "dV")} | {"O": given["O"]}, ref, lens, B, H, S, row_bar=False)
    print("flash vs fp64, share of bar  %-24s delta given      %s" % (name, _fmt(sh)))
    assert max(sh.values()) <= 1.0, sh
    d = H * fr.DK
    for i, n in enumerate(("dQ", "dK", "dV")):
        e = fr.slab_err(given[n], got[n], B, H, S)
        print("delta given vs delta computed (%s): %s slab_err %.5f" % (regime, n, e))
        assert e <= 0.005, (n, e)


def test_repeat_is_bit_identical():
    """"no atomics, each output tile is written once: deterministic" (flash_attn.hip): the same call twice."""
    name = "xcd-4x2x130-planted"
    B, H, S = fr.CASES[name][:3]
    (qkv, do, lens), _ = fr.case_reference(name)
    a = _run(qkv, do, lens, B, H, S)
    b = _run(qkv, do, lens, B, H, S)
    for n in ("O", "o32", "LSE", "dqkv"):
        assert torch.equal(a[n], b[n]), n
