"""Reference, rounding model, inputs and metrics for the flash-attention tests (tts_king_amd/csrc/flash_attn.hip).  No GPU here:
tests/test_flash_ref_cpu.py checks this file against torch and against itself, tests/test_flash_edges_gpu.py holds the kernel to it.

Layouts are the kernel's: qkv [B*S][3*d] (q | k | v, head h = columns h*128.. of each part), O and dO [B*S][d], LSE [B*H][S],
dqkv [B*S][3*d] (dQ | dK | dV).  reference: fs_two/transformer/Modules.py:14-24, SubLayers.py:44-60.

  reference()       fp64 attention and its autograd gradients on the bf16-rounded inputs.
  rounding_model()  the same math in fp64 with a rounding to bf16 wherever the kernel has one: what a CORRECT kernel is allowed to
                    differ from reference() by.  Derived from the kernel's description (ttsk.h, the header of flash_attn.hip), never
                    from its output.
  make_case()       inputs in three regimes: near-uniform scores, peaked scores, peaked scores with planted dominant keys.
  slab_err / row_err / lse_excess   metrics under which one wrong head, utterance or key cannot hide behind the rest of the tensor.
  CASES             every (shape, lengths, regime) the GPU file runs; the CPU file proves on each of them that the rounding model
                    stays within half of every bar and that the negative controls (reference(mutation=...)) are caught."""
import functools

import torch

DK = 128
TK = 64                     # key tile of the kernel's online softmax (the "no_rescale" negative control emulates it)
BF = torch.bfloat16

# The bars of tests/test_attention_gpu.py (2 % of max for O, 3 % / 4 % for the gradients, 2e-3 for LSE), applied per slab and per row
BAR_O = 0.02
BAR_O_ROW = 0.02
BAR_GRAD = 0.03             # delta = rowsum(dO o O) from the fp32 O
BAR_GRAD_BF16_DELTA = 0.04  # delta from the bf16 O
BAR_LSE = 2e-3              # times max(1, |lse| / 8): 2e-3 at the magnitude near-uniform scores have (lse ~ log S ~ 5), relative beyond


def ref_attention(qkv, lens, B, H, S):
    """softmax(q k^T / sqrt(d_k), keys >= lens[b] masked) v in fp64 -> (P (B*H, S, S), O (B*S, d), (q, k, v) each (B, H, S, d_k))."""
    d = qkv.shape[1] // 3
    dk = d // H
    x = qkv.double().view(B, S, 3, H, dk)
    q, k, v = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3), x[:, :, 2].permute(0, 2, 1, 3)   # (B,H,S,dk)
    s = q @ k.transpose(-1, -2) / dk ** 0.5
    mask = torch.arange(S)[None, :] >= lens[:, None]
    s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(B * S, d)
    return p.reshape(B * H, S, S), o, (q, k, v)


def _bf(x):
    """fp64 -> nearest bf16 -> fp64 (through fp32: the double rounding moves a value by 2^-24 relative at most)."""
    return x.float().to(BF).double()


def _split(qkv, B, H, S):
    x = qkv.view(B, S, 3, H, DK)
    return x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3), x[:, :, 2].permute(0, 2, 1, 3)     # (B, H, S, 128)


def _merge(x, B, H, S):
    """(B, H, S, 128) -> [B*S][H*128]"""
    return x.permute(0, 2, 1, 3).reshape(B * S, H * DK)


def _visible(lens, S):
    """(B, S) bool: key j of utterance b takes part.  An utterance without keys is computed as if it had all of them and zeroed
    afterwards (`live`), so that no row is a softmax over nothing."""
    lens = lens.clamp(min=0, max=S)
    live = lens > 0
    vis = torch.arange(S)[None, :] < torch.where(live, lens, torch.full_like(lens, S))[:, None]
    return vis, live


MUTATIONS = ("mask_gt", "last_key_masked", "heads_swapped", "no_rescale", "len_from_prev")


def reference(qkv_bf16, dO_bf16, lens, B, H, S, mutation=None):
    """fp64 attention and autograd gradients on the bf16-rounded inputs -> dict(O [B*S][d], LSE [B*H][S], dQ, dK, dV [B*S][d]).
    An utterance with lens[b] <= 0 is all zeros, LSE included, as the kernel defines it; lens beyond S mean S.

    `mutation` (negative controls, tests/test_flash_ref_cpu.py) computes what a kernel with one specific defect would:
      mask_gt          key lens[b] is visible (`>` for `>=` in the mask)
      last_key_masked  key lens[b] - 1 is masked
      heads_swapped    (batch, head) pair z computes pair z ^ 1's attention (with its own utterance's length)
      no_rescale       the online softmax over 64-key tiles forgets to rescale its sum and accumulators when the maximum rises
      len_from_prev    utterance b uses the length of utterance b - 1"""
    assert mutation is None or mutation in MUTATIONS
    lens = lens.clone()
    if mutation == "mask_gt":
        lens = torch.where(lens > 0, lens + 1, lens)
    elif mutation == "last_key_masked":
        lens = lens.clamp(max=S) - 1
    elif mutation == "len_from_prev":
        lens = torch.roll(lens, 1)
    vis, live = _visible(lens, S)
    x = qkv_bf16.double().clone().requires_grad_(True)
    q, k, v = _split(x, B, H, S)
    if mutation == "heads_swapped":
        zz = torch.arange(B * H) ^ 1
        q, k, v = (t.reshape(B * H, S, DK)[zz].reshape(B, H, S, DK) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) / DK ** 0.5
    s = s.masked_fill(~vis[:, None, None, :], float("-inf"))
    if mutation == "no_rescale":
        m = torch.full((B, H, S), float("-inf"), dtype=torch.float64)
        l = torch.zeros(B, H, S, dtype=torch.float64)
        acc = torch.zeros(B, H, S, DK, dtype=torch.float64)
        for j0 in range(0, S, TK):
            st = s[..., j0:j0 + TK]
            mn = torch.maximum(m, st.max(-1).values.detach())
            mn_safe = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)      # a tile past every key of the utterance
            p = torch.exp(st - mn_safe[..., None])
            l = l + p.sum(-1)                                                     # (a correct kernel: l * exp(m - mn) + ...)
            acc = acc + p @ v[:, :, j0:j0 + TK]
            m = mn
        o = acc / l[..., None]
        lse = m + torch.log(l)
    else:
        lse = torch.logsumexp(s, dim=-1)
        o = torch.exp(s - lse[..., None]) @ v
    alive = live.double()[:, None, None]
    o = _merge(o * alive[..., None], B, H, S)
    o.backward(dO_bf16.double())
    d = H * DK
    g = x.grad
    return {"O": o.detach(), "LSE": (lse.detach() * alive).reshape(B * H, S), "dQ": g[:, :d], "dK": g[:, d:2 * d], "dV": g[:, 2 * d:]}


def rounding_model(qkv_bf16, dO_bf16, lens, B, H, S, delta_from="o32"):
    """reference()'s math in fp64 with the kernel's roundings to bf16, and only those:
      forward   p = exp(s - rowmax) is rounded before the P V product, the row sum is taken over the unrounded p; O is rounded;
      backward  P = exp(s - LSE) is rounded for dV = P^T dO; dS = scale * P * (dP - delta) is rounded for dQ = dS K and dK = dS^T Q
                (P itself stays unrounded inside dS); the three outputs are rounded;
      delta     rowsum(dO o O) from the unrounded O (`delta_from="o32"`: the fp32 copy a training forward keeps) or from the
                rounded one (`"bf16"`).
    fp32 accumulation and the fp32 LSE are below all of these (2^-24 against 2^-9) and are not modelled.  The kernel rounds p
    against the maximum it has seen so far, not the final one: bf16 rounding is relative, so the size of the error is the same."""
    assert delta_from in ("o32", "bf16")
    vis, live = _visible(lens, S)
    q, k, v = _split(qkv_bf16.double(), B, H, S)
    do = dO_bf16.double().view(B, S, H, DK).permute(0, 2, 1, 3)
    scale = DK ** -0.5
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~vis[:, None, None, :], float("-inf"))
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    o32 = (_bf(p) @ v) / l
    o = _bf(o32)
    lse = m + torch.log(l)
    delta = (do * (o32 if delta_from == "o32" else o)).sum(-1, keepdim=True)
    P = torch.exp(s - lse)
    dS = _bf(scale * P * (do @ v.transpose(-1, -2) - delta))
    alive = live.double()[:, None, None, None]
    out = {"O": o * alive, "dQ": _bf(dS @ k) * alive, "dK": _bf(dS.transpose(-1, -2) @ q) * alive,
           "dV": _bf(_bf(P).transpose(-1, -2) @ do) * alive}
    out = {n: _merge(t, B, H, S) for n, t in out.items()}
    out["LSE"] = (lse * alive).reshape(B * H, S)
    return out


# ------------------------------------------------------------------------------------------------------------------ inputs
REGIMES = ("uniform", "peaked", "planted")


def plant_pairs(S, n):
    """(query row, dominant key) pairs of the planted regime for an utterance of n keys: the dominant keys are key 0, the last key, and
    the keys on both sides of the first tile seam (or the last key, when the utterance ends before them); one query row each, spread
    over the sequence (query rows are not masked: a row may lie past the utterance)."""
    if n <= 0:
        return []
    keys, rows = [], []
    for key in (0, n - 1, min(63, n - 1), min(64, n - 1)):
        if key not in keys:
            keys.append(key)
    for row in (S - 1, S // 3, S // 2, 1 % S, 0):
        if row not in rows:
            rows.append(row)
    return list(zip(rows, keys))


def make_case(B, H, S, lens, regime, seed, plant=None):
    """-> (qkv bf16 [B*S][3*d], dO bf16 [B*S][d], lens int64 [B]).  Every value is finite and exact in bf16.
      uniform  0.7 * randn: q.k / sqrt(128) has std ~ 0.5, the softmax is nearly flat (what random weights give)
      peaked   the q part times 8 (a power of two: exact): score std ~ 4, a handful of keys carry each row
      planted  peaked, and per (utterance, head) the rows of plant_pairs() (or of `plant`, a list of (row, key)) get a key that
               dominates them outright: k[key] = 2 * q[row] / 8, a score of ~ 90 against a spread of ~ 8.  When lens[b] < S the
               first MASKED key gets k = q[0] (a score of ~ 350 for row 0, spread ~ 30 over the others) and v = 100: one row of
               leakage through the mask swamps the output."""
    assert regime in REGIMES
    g = torch.Generator().manual_seed(seed)
    d = H * DK
    x = (torch.randn(B * S, 3 * d, generator=g) * 0.7).to(BF).float().view(B, S, 3, H, DK)
    do = torch.randn(B * S, d, generator=g).to(BF)
    lens = torch.as_tensor(lens, dtype=torch.int64)
    assert lens.shape == (B,)
    if regime != "uniform":
        q0 = x[:, :, 0].clone()
        x[:, :, 0] *= 8.0
        if regime == "planted":
            for b in range(B):
                n = int(lens[b].clamp(max=S))
                for row, key in (plant if plant is not None else plant_pairs(S, n)):
                    x[b, key, 1] = 2.0 * q0[b, row]
                if 0 <= n < S:
                    x[b, n, 1] = 8.0 * q0[b, 0]
                    x[b, n, 2] = 100.0
    qkv = x.reshape(B * S, 3 * d).to(BF)
    assert torch.equal(qkv.float(), x.reshape(B * S, 3 * d)) and bool(torch.isfinite(qkv.float()).all())
    return qkv, do, lens


# ------------------------------------------------------------------------------------------------------------------ metrics
def _slabs(t, B, H, S):
    """[B*S][H*128] -> (B*H, S, 128)"""
    return t.double().view(B, S, H, DK).permute(0, 2, 1, 3).reshape(B * H, S, DK)


def slab_err(got, want, B, H, S, skip=None):
    """max over (b, h) of (max-abs error over that head's [S][128] slab) / (that slab's own max-abs).  A slab whose reference is all
    zero (an utterance without keys) must be all zero: any other value counts as an infinite error.  `skip` (B*H bools): slabs left
    out (shares() judges the dQ / dK of one-key utterances by a rule of their own)."""
    g, w = _slabs(got, B, H, S), _slabs(want, B, H, S)
    err = (g - w).abs().amax(dim=(1, 2))
    ref = w.abs().amax(dim=(1, 2))
    rel = torch.where(ref > 0, err / ref.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    if skip is not None:
        rel = rel[~skip]
    return float(rel.max()) if rel.numel() else 0.0


def row_err(got, want, B, H, S, rows=None):
    """max over (b, h, query row) of the row's relative L2 error, over the rows whose reference norm is at least 0.1 x the largest
    row norm of their slab (`rows`: only these row indices)."""
    g, w = _slabs(got, B, H, S), _slabs(want, B, H, S)
    wn = w.norm(dim=-1)
    en = (g - w).norm(dim=-1)
    keep = (wn >= 0.1 * wn.amax(dim=1, keepdim=True)) & (wn > 0)
    if rows is not None:
        sel = torch.zeros(S, dtype=torch.bool)
        sel[torch.as_tensor(rows)] = True
        keep &= sel[None, :]
    if not bool(keep.any()):
        return 0.0
    return float((en[keep] / wn[keep]).max())


def lse_excess(got, want):
    """max of |got - want| / (BAR_LSE * max(1, |want| / 8)): <= 1 passes."""
    w = want.double()
    return float(((got.double() - w).abs() / (BAR_LSE * torch.clamp(w.abs() / 8, min=1.0))).max())


ONE_KEY_GRAD = 1e-3         # an utterance with ONE key: max|dQ|, max|dK| <= this x max|dV| of the same (batch, head)


def shares(got, want, lens, B, H, S, bar_grad=BAR_GRAD, row_bar=True):
    """Every judged quantity as a share of its bar -> dict; a share <= 1 passes.  dQ, dK, dV are judged per slab only: under peaked
    scores a dQ row is the difference of nearly equal terms and its own relative error is 5-12 % for the rounding model already.
    An utterance with ONE key has softmax = 1 whatever q and k are: its dQ and dK are exactly zero in the reference (dS = P (dP - delta)
    with dP = delta), so there is no slab maximum to divide by; the kernel's dP and delta are two fp32 sums of the same 128 products in
    different orders, and what is left of their difference is held to ONE_KEY_GRAD x the slab's max|dV| instead ("dQ 1key")."""
    out = {"O slab": slab_err(got["O"], want["O"], B, H, S) / BAR_O}
    if row_bar:
        out["O row"] = row_err(got["O"], want["O"], B, H, S) / BAR_O_ROW
    if "LSE" in got:
        out["LSE"] = lse_excess(got["LSE"], want["LSE"])
    one = (torch.as_tensor(lens).clamp(max=S) == 1).repeat_interleave(H)
    for n in ("dQ", "dK", "dV"):
        if n not in got:
            continue
        out[n + " slab"] = slab_err(got[n], want[n], B, H, S, skip=one if n != "dV" else None) / bar_grad
        if n != "dV" and bool(one.any()):
            assert float(_slabs(want[n], B, H, S)[one].abs().max()) == 0.0
            dv = _slabs(want["dV"], B, H, S)[one].abs().amax(dim=(1, 2))
            out[n + " 1key"] = float((_slabs(got[n], B, H, S)[one].abs().amax(dim=(1, 2)) / (ONE_KEY_GRAD * dv)).max())
    return out


# ------------------------------------------------------------------------------------------------------------------ the GPU file's cases
# name -> (B, H, S, lens, regime, seed).  B*H % 8 == 0 takes xcd_tile()'s remap (nx = query / key tiles = 3, 2, 1, 3); every utterance
# of those has a length of its own, so a tile that lands on the wrong (b, h) computes with the wrong mask as well as the wrong data.
_XCD = {
    (4, 2, 130): [130, 65, 17, 101],
    (8, 2, 65): [65, 1, 64, 33, 2, 50, 63, 17],
    (8, 1, 64): [64, 1, 63, 32, 5, 48, 17, 60],
    (4, 4, 129): [129, 128, 64, 70],
    (3, 2, 130): [130, 66, 9],              # B*H = 6: the plain order, as a control
}
KEY_LENS_H1 = [0, 1, 2, 63, 64, 65, 127, 128, 129, 199, 200]
KEY_LENS_H2 = [1, 64, 65, 200]
SEQ_EDGES = (1, 63, 65, 128, 129)
# (query row, dominant key), S = 200: the first four have query tile t peak in key tile t (first key of the first tile, last key of the
# last tile), the other four peak in a tile far from their own (key tiles 3, 0, 2, 1), both sides of the first seam among them
PEAK_PAIRS = [(5, 0), (70, 101), (140, 128), (199, 199), (60, 192), (130, 63), (100, 150), (20, 64)]

CASES = {}
for (_B, _H, _S), _lens in _XCD.items():
    for _r in ("uniform", "planted"):
        CASES["xcd-%dx%dx%d-%s" % (_B, _H, _S, _r)] = (_B, _H, _S, _lens, _r, 100 + _B * _H + _S)
for _r in REGIMES:
    CASES["keylen-h1-" + _r] = (11, 1, 200, KEY_LENS_H1, _r, 211)
    CASES["keylen-h2-" + _r] = (4, 2, 200, KEY_LENS_H2, _r, 212)
for _S in SEQ_EDGES:
    CASES["seq-%d" % _S] = (2, 2, _S, [_S, max(1, _S // 3)], "planted", 300 + _S)
for _S in (70, 200):
    CASES["onekey-%d" % _S] = (2, 2, _S, [_S // 2, 1], "planted", 400 + _S)
CASES["masked-keys"] = (3, 2, 150, [150, 77, 1], "planted", 501)
CASES["peaks"] = (1, 2, 200, [200], "planted", 601)
CASES["delta-given-peaked"] = (2, 2, 130, [130, 71], "peaked", 701)
CASES["delta-given-uniform"] = (2, 2, 130, [130, 71], "uniform", 702)


def case_inputs(name):
    B, H, S, lens, regime, seed = CASES[name]
    return make_case(B, H, S, lens, regime, seed, plant=PEAK_PAIRS if name == "peaks" else None)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(inputs, reference) of a case, computed once per process and shared: callers must not write into the tensors."""
    B, H, S = CASES[name][:3]
    qkv, do, lens = case_inputs(name)
    return (qkv, do, lens), reference(qkv, do, lens, B, H, S)
