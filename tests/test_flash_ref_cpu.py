"""CPU: the yardstick of tests/test_flash_edges_gpu.py is itself checked (tests/flash_ref.py; no kernel runs here).
  - reference() agrees with torch.nn.functional.scaled_dot_product_attention in fp64;
  - rounding_model() — fp64 math with the kernel's bf16 roundings and nothing else — stays within HALF of every bar on every case the
    GPU file runs: a correct kernel can pass, with a factor of two for what the model leaves out (fp32 accumulation order, fast exp);
  - five defects a flash kernel can have (reference(mutation=...)) each exceed a bar on a named case: the cases can see them;
  - an fp32 emulation of LSE against the LSE bar (printed; the finding is recorded in DESIGN.md)."""
import pytest
import torch
import torch.nn.functional as F

from tests import flash_ref as fr


def _fmt(sh):
    return "  ".join("%s %.3f" % (k, v) for k, v in sh.items())


@pytest.mark.parametrize("name", ["xcd-4x2x130-planted", "keylen-h2-peaked"])
def test_reference_agrees_with_sdpa(name):
    B, H, S = fr.CASES[name][:3]
    (qkv, do, lens), ref = fr.case_reference(name)
    assert int(lens.min()) > 0          # (an utterance without keys is defined by the kernel, not by torch: NaN there)
    x = qkv.double().clone().requires_grad_(True)
    xv = x.view(B, S, 3, H, fr.DK)
    q, k, v = (xv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    keep = (torch.arange(S)[None, :] < lens.clamp(max=S)[:, None])[:, None, None, :]
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=keep).permute(0, 2, 1, 3).reshape(B * S, H * fr.DK)
    o.backward(do.double())
    d = H * fr.DK
    for n, want in (("O", o.detach()), ("dQ", x.grad[:, :d]), ("dK", x.grad[:, d:2 * d]), ("dV", x.grad[:, 2 * d:])):
        err = float((ref[n] - want).abs().max())
        assert err <= 1e-10 * float(want.abs().max()), (n, err)
    # LSE has no counterpart in sdpa: against the plain definition
    s = (q.detach() @ k.detach().transpose(-1, -2)) / fr.DK ** 0.5
    want_lse = torch.logsumexp(s.masked_fill(~keep, float("-inf")), dim=-1).reshape(B * H, S)
    assert float((ref["LSE"] - want_lse).abs().max()) <= 1e-10
    # ... and the helper the older GPU test uses
    _, o2, _ = fr.ref_attention(qkv.float(), lens.clamp(max=S), B, H, S)
    assert float((o2 - ref["O"]).abs().max()) <= 1e-10 * float(ref["O"].abs().max())


def test_empty_utterance_is_defined_as_zeros():
    name = "keylen-h1-planted"
    B, H, S, lens = fr.CASES[name][:4]
    assert lens[0] == 0
    _, ref = fr.case_reference(name)
    for n in ("O", "dQ", "dK", "dV"):
        assert float(ref[n][:S].abs().max()) == 0.0 and bool(torch.isfinite(ref[n]).all()), n
    assert float(ref["LSE"][0].abs().max()) == 0.0 and bool(torch.isfinite(ref["LSE"]).all())
    # keys past the utterance get exactly zero dK / dV in the reference too
    for b in range(B):
        assert float(ref["dK"][b * S + lens[b]:(b + 1) * S].abs().max() if lens[b] < S else 0.0) == 0.0
        assert float(ref["dV"][b * S + lens[b]:(b + 1) * S].abs().max() if lens[b] < S else 0.0) == 0.0


def test_metrics_see_one_wrong_head_and_one_wrong_row():
    B, H, S = 2, 2, 70
    g = torch.Generator().manual_seed(1)
    want = torch.randn(B * S, H * fr.DK, generator=g, dtype=torch.float64)
    want.view(B, S, H, fr.DK)[0, :, 0] *= 100.0             # a loud head, behind which a whole-tensor max-abs metric hides the others
    got = want.clone()
    got.view(B, S, H, fr.DK)[1, 7, 1] *= 1.5                # one row of a quiet head off by 50 %
    whole = float((got - want).abs().max() / want.abs().max())
    assert whole < 0.02 < fr.slab_err(got, want, B, H, S)
    assert abs(fr.row_err(got, want, B, H, S) - 0.5) < 1e-12
    assert fr.row_err(got, want, B, H, S, rows=[6, 8]) == 0.0
    zero = torch.zeros_like(want)
    assert fr.slab_err(zero, zero, B, H, S) == 0.0 and fr.slab_err(got, zero, B, H, S) == float("inf")
    assert fr.lse_excess(torch.tensor([80.0 + 0.019]), torch.tensor([80.0])) < 1.0 < fr.lse_excess(torch.tensor([80.0 + 0.021]), torch.tensor([80.0]))
    assert fr.lse_excess(torch.tensor([3.0 + 0.0019]), torch.tensor([3.0])) < 1.0 < fr.lse_excess(torch.tensor([3.0 + 0.0021]), torch.tensor([3.0]))


def test_planted_inputs_are_what_they_claim():
    """The planted keys dominate their rows, and the first masked key would dominate row 0 if it leaked."""
    name = "keylen-h2-planted"
    B, H, S, lens = fr.CASES[name][:4]
    (qkv, _, _), _ = fr.case_reference(name)
    q, k, v = fr._split(qkv.double(), B, H, S)
    s = (q @ k.transpose(-1, -2)) / fr.DK ** 0.5
    for b in range(B):
        n = lens[b]
        for row, key in fr.plant_pairs(S, n):
            others = torch.cat([s[b, :, row, :key], s[b, :, row, key + 1:n]], dim=-1)
            if others.numel():
                assert float((s[b, :, row, key] - others.max(-1).values).min()) > 20.0, (b, row, key)
        if n < S:
            assert float((s[b, :, 0, n] - s[b, :, 0, :n].max(-1).values).min()) > 100.0 and float(v[b, :, n].min()) == 100.0
    assert {k_ for _, k_ in fr.plant_pairs(200, 200)} == {0, 63, 64, 199} and {k_ for _, k_ in fr.plant_pairs(200, 1)} == {0}
    assert sorted(k_ // fr.TK for _, k_ in fr.PEAK_PAIRS) == [0, 0, 1, 1, 2, 2, 3, 3] and len({k_ for _, k_ in fr.PEAK_PAIRS}) == 8


@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_rounding_model_within_half_of_every_bar(name):
    """The condition under which a correct kernel can meet the bars of the GPU file: bf16 roundings alone use at most half of each."""
    B, H, S = fr.CASES[name][:3]
    (qkv, do, lens), ref = fr.case_reference(name)
    for src, bar in (("o32", fr.BAR_GRAD), ("bf16", fr.BAR_GRAD_BF16_DELTA)):
        sh = fr.shares(fr.rounding_model(qkv, do, lens, B, H, S, delta_from=src), ref, lens, B, H, S, bar_grad=bar)
        print("rounding model, share of bar  %-24s delta from %-4s  %s" % (name, src, _fmt(sh)))
        assert max(sh.values()) <= 0.5, (name, src, sh)


def test_rounding_model_worst_shares(capsys):
    """The worst share per quantity over all cases, shown whether or not output is captured (the per-case lines above need -s)."""
    worst = {}
    for name in sorted(fr.CASES):
        B, H, S = fr.CASES[name][:3]
        (qkv, do, lens), ref = fr.case_reference(name)
        for src, bar in (("o32", fr.BAR_GRAD), ("bf16", fr.BAR_GRAD_BF16_DELTA)):
            sh = fr.shares(fr.rounding_model(qkv, do, lens, B, H, S, delta_from=src), ref, lens, B, H, S, bar_grad=bar)
            for k, v in sh.items():
                k = k if k[0] != "d" else "%s (delta from %s)" % (k, src)
                if v >= worst.get(k, (-1.0, None))[0]:
                    worst[k] = (v, name)
    with capsys.disabled():
        print()
        for k, (v, name) in worst.items():
            print("rounding model, worst share of bar over %d cases: %-30s %.3f  (%s)" % (len(fr.CASES), k, v, name))
    assert max(v for v, _ in worst.values()) <= 0.5


# the defect -> the case of the GPU file that must catch it (others may too: printed)
CAUGHT_BY = {
    "mask_gt": "keylen-h1-planted",
    "last_key_masked": "keylen-h1-planted",
    "heads_swapped": "xcd-4x2x130-uniform",
    "no_rescale": "peaks",
    "len_from_prev": "xcd-8x1x64-uniform",
}


@pytest.mark.parametrize("mutation", fr.MUTATIONS)
def test_negative_control_is_caught(mutation, capsys):
    assert set(CAUGHT_BY) == set(fr.MUTATIONS)
    catching = []
    for name in sorted(fr.CASES):
        B, H, S = fr.CASES[name][:3]
        if mutation == "heads_swapped" and (B * H) % 2:
            continue
        (qkv, do, lens), ref = fr.case_reference(name)
        sh = fr.shares(fr.reference(qkv, do, lens, B, H, S, mutation=mutation), ref, lens, B, H, S)
        worst = max(sh, key=sh.get)
        if sh[worst] > 1.0:
            catching.append(name)
        if name == CAUGHT_BY[mutation]:
            with capsys.disabled():
                print("\nnegative control %-16s caught by %-22s %s = %.3g x its bar" % (mutation, name, worst, sh[worst]), end="")
            assert sh[worst] > 2.0, (mutation, name, sh)          # not by a hair: twice the bar
    print("negative control %-16s exceeds a bar on %d of %d cases: %s" % (mutation, len(catching), len(fr.CASES), ", ".join(catching)))
    assert CAUGHT_BY[mutation] in catching


def test_lse_in_fp32_against_its_bar():
    """fp32 scores and an fp32 logsumexp on the CPU against the fp64 LSE, as a share of the LSE bar: what fp32 arithmetic alone
    uses of it, before any kernel."""
    worst = (0.0, None)
    for name in sorted(fr.CASES):
        B, H, S = fr.CASES[name][:3]
        (qkv, _, lens), ref = fr.case_reference(name)
        q, k, _ = fr._split(qkv.float(), B, H, S)
        vis, live = fr._visible(lens, S)
        s = (q @ k.transpose(-1, -2)) * torch.tensor(fr.DK ** -0.5, dtype=torch.float32)
        lse = torch.logsumexp(s.masked_fill(~vis[:, None, None, :], float("-inf")), dim=-1) * live.float()[:, None, None]
        assert lse.dtype == torch.float32
        share = fr.lse_excess(lse.reshape(B * H, S), ref["LSE"])
        print("fp32 LSE emulation, share of bar  %-24s %.4f  (max |lse| %.1f)" % (name, share, float(ref["LSE"].abs().max())))
        worst = max(worst, (share, name))
    assert worst[0] <= 0.5, worst
