"""GPU: the memory-bound row kernels (LayerNorm tail, softmax, embeddings, BatchNorm, loss, clip+Adam) through the
C ABI against fp32/fp64 CPU torch math on the same bf16-rounded inputs.

Tolerances: bf16 outputs carry one rounding (rel 2^-8); fp32 outputs are compared at 1e-5..1e-4; integer outputs
(bucketize, int16 audio) are exact."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def close_bf16(out, ref, extra=0.0):
    out, ref = out.float().cpu().double(), ref.double()
    tol = 2 ** -7 * ref.abs() + 2 ** -7 * float(ref.abs().mean()) + extra
    bad = (out - ref).abs() > tol
    assert not bool(bad.any()), (int(bad.sum()), float((out - ref).abs().max()))


def close_f32(out, ref, rtol=1e-4, atol=1e-5):
    np.testing.assert_allclose(out.float().cpu().numpy(), ref.float().numpy(), rtol=rtol, atol=atol)


def lens_mask(lens, seg):
    return (torch.arange(seg)[None, :] >= lens[:, None]).reshape(-1)


@pytest.mark.parametrize("rows_seg", [(4, 100), (16, 64)])
def test_layernorm_residual_mask_fwd_bwd(rows_seg):
    from tts_king_amd import ops
    Bn, seg = rows_seg
    rows, D = Bn * seg, 256
    y, res = rnd(rows, D, seed=1).to(BF), rnd(rows, D, seed=2).to(BF)
    gamma, beta = 1 + 0.1 * rnd(D, seed=3), 0.1 * rnd(D, seed=4)
    lens = torch.randint(seg // 2, seg + 1, (Bn,), generator=torch.Generator().manual_seed(5))
    dout = rnd(rows, D, seed=6).to(BF)
    pad = lens_mask(lens, seg)
    zf = (y.float() + res.float()).to(BF).float().requires_grad_(True)   # kernel's backward sees the rounded z
    g2, b2 = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ref = F.layer_norm(zf, (D,), g2, b2).masked_fill(pad[:, None], 0)
    ref.backward(dout.float())
    out, z, mean, rstd, _ = ops.layernorm_fwd(y.to(DEV), res.to(DEV), gamma.to(DEV), beta.to(DEV), lens.to(DEV), seg)
    ref_fwd = F.layer_norm(y.float() + res.float(), (D,), gamma, beta).masked_fill(pad[:, None], 0)
    close_bf16(out, ref_fwd)
    assert torch.equal(z.cpu(), (y.float() + res.float()).to(BF))
    dz, dy, partials, nblk = ops.layernorm_bwd(dout.to(DEV), z, mean, rstd, gamma.to(DEV), beta.to(DEV), lens.to(DEV), seg)
    assert dy is dz
    close_bf16(dz, zf.grad, extra=1e-3)
    sums = partials.sum(0).cpu()
    close_f32(sums[D:2 * D], g2.grad, rtol=2e-3, atol=2e-2)             # layout: dbias | dgamma | dbeta
    close_f32(sums[2 * D:3 * D], b2.grad, rtol=2e-3, atol=2e-2)
    close_f32(sums[:D], zf.grad.to(BF).float().sum(0), rtol=2e-2, atol=0.1)


def test_layernorm_predictor_tail_head_relu():
    """VariancePredictor tail: h = relu(...) -> LN -> Linear(256,1) -> masked_fill; backward gates by (h > 0)."""
    from tts_king_amd import ops
    Bn, seg, D = 4, 64, 256
    rows = Bn * seg
    h = torch.relu(rnd(rows, D, seed=7)).to(BF)
    gamma, beta = 1 + 0.1 * rnd(D, seed=8), 0.1 * rnd(D, seed=9)
    w, b = rnd(D, seed=10, scale=D ** -0.5), torch.tensor([0.3])
    lens = torch.tensor([64, 40, 33, 64])
    pad = lens_mask(lens, seg)
    dhead = rnd(rows, seed=11)
    pre = rnd(rows, D, seed=12)       # stand-in for the pre-activation: only its sign pattern matters
    hf = h.float().requires_grad_(True)
    g2, b2, w2, bb2 = [t.clone().requires_grad_(True) for t in (gamma, beta, w, b)]
    ref = (F.layer_norm(hf, (D,), g2, b2) @ w2 + bb2).masked_fill(pad, 0.0)
    ref.backward(dhead)
    _, _, mean, rstd, ho = ops.layernorm_fwd(h.to(DEV), None, gamma.to(DEV), beta.to(DEV), lens.to(DEV), seg, save_z=False,
                                             head=(w.to(DEV), b.to(DEV)), want_out=False)
    close_f32(ho, ref.detach(), rtol=1e-4, atol=1e-4)
    dz, _, partials, nblk = ops.layernorm_bwd(None, h.to(DEV), mean, rstd, gamma.to(DEV), beta.to(DEV), lens.to(DEV), seg,
                                              relu_in=True, dhead=dhead.to(DEV), head_w=w.to(DEV))
    want = hf.grad * (h.float() > 0)
    close_bf16(dz, want, extra=1e-3)
    sums = partials.sum(0).cpu()
    close_f32(sums[D:2 * D], g2.grad, rtol=2e-3, atol=2e-2)
    close_f32(sums[2 * D:3 * D], b2.grad, rtol=2e-3, atol=2e-2)
    close_f32(sums[3 * D:4 * D], w2.grad, rtol=2e-3, atol=2e-2)
    close_f32(sums[4 * D:], bb2.grad, rtol=1e-3, atol=1e-3)


def test_layernorm_dropout_masks_consistent():
    from tts_king_amd import ops
    rows, D, p = 512, 256, 0.2
    y = (rnd(rows, D, seed=13).abs() + 0.5).to(BF)
    gamma, beta = torch.ones(D), torch.zeros(D)
    st = ops.optim_state(DEV, seed=99)
    rng = ops.rng_of(st)
    out, z, mean, rstd, _ = ops.layernorm_fwd(y.to(DEV), None, gamma.to(DEV), beta.to(DEV), p_pre=p, site_pre=5, rng=rng)
    zc = z.cpu().float()
    keep = zc != 0
    frac = float(keep.float().mean())
    assert abs(frac - (1 - p)) < 0.01, frac
    close_bf16(zc[keep], y.float()[keep] / (1 - p))
    out2, z2, *_ = ops.layernorm_fwd(y.to(DEV), None, gamma.to(DEV), beta.to(DEV), p_pre=p, site_pre=5, rng=rng)
    assert torch.equal(z2, z)                                     # same (seed, step, site) -> same mask
    _, z3, *_ = ops.layernorm_fwd(y.to(DEV), None, gamma.to(DEV), beta.to(DEV), p_pre=p, site_pre=6, rng=rng)
    assert not torch.equal(z3, z)                                 # another site -> another mask
    ops.rng_advance(st)
    _, z4, *_ = ops.layernorm_fwd(y.to(DEV), None, gamma.to(DEV), beta.to(DEV), p_pre=p, site_pre=5, rng=rng)
    assert not torch.equal(z4, z)                                 # next step -> another mask
    # backward regenerates the step's mask
    st2 = ops.optim_state(DEV, seed=99)
    dout = rnd(rows, D, seed=14).to(BF)
    dz, dy, _, _ = ops.layernorm_bwd(dout.to(DEV), z, mean, rstd, gamma.to(DEV), beta.to(DEV), p_pre=p, site_pre=5,
                                     rng=ops.rng_of(st2))
    dzc, dyc = dz.cpu().float(), dy.cpu().float()
    assert torch.equal(dyc != 0, keep & (dzc != 0))
    close_bf16(dyc[keep], dzc[keep] / (1 - p))
    # post-LN dropout (predictor style)
    out5, *_ = ops.layernorm_fwd(y.to(DEV), None, gamma.to(DEV), beta.to(DEV), p_post=0.5, site_post=7, rng=rng, save_z=False)
    f5 = float((out5.cpu().float() != 0).float().mean())
    assert abs(f5 - 0.5) < 0.01, f5


@pytest.mark.parametrize("S", [64, 423])
def test_softmax_fwd_bwd(S):
    from tts_king_amd import ops
    Bn, H = 3, 2
    Sp = (S + 7) // 8 * 8
    s = torch.zeros(Bn * H, S, Sp)
    s[:, :, :S] = rnd(Bn * H, S, S, seed=15, scale=2.0)
    lens = torch.tensor([S, S // 2, 5])
    mask = torch.arange(S)[None, None, :] >= lens.repeat_interleave(H)[:, None, None]
    sf = s[:, :, :S].clone().requires_grad_(True)
    ref = torch.softmax(sf.masked_fill(mask, float("-inf")), dim=2)
    P = ops.softmax_fwd(s.to(DEV), lens.to(DEV), H)
    close_bf16(P[:, :, :S], ref.detach(), extra=1e-4)
    assert float(P[:, :, S:].float().abs().max()) == 0 if Sp > S else True
    dP = torch.zeros(Bn * H, S, Sp)
    dP[:, :, :S] = rnd(Bn * H, S, S, seed=16)
    Pb = P.cpu().float()[:, :, :S]
    want = 0.25 * Pb * (dP[:, :, :S] - (dP[:, :, :S] * Pb).sum(-1, keepdim=True))
    dS = ops.softmax_bwd(P, dP.to(DEV), 0.25)
    close_bf16(dS[:, :, :S], want, extra=1e-4)


def test_bucketize_exact(cfg):
    import json, os
    from tts_king_amd import ops
    with open(os.path.join(cfg.preprocess_config.path.preprocessed_path, "stats.json")) as f:
        stats = json.load(f)
    for key in ("pitch", "energy"):
        bins = torch.linspace(stats[key][0], stats[key][1], 255)
        v = torch.cat([rnd(4000, seed=17, scale=3.0), bins, bins + 1e-6, bins - 1e-6,
                       torch.tensor([-1e9, 1e9, stats[key][0], stats[key][1], 0.0])])
        for scale in (1.0, 1.5):
            got = ops.bucketize(v.to(DEV), bins.to(DEV), scale).cpu()
            assert torch.equal(got.long(), torch.bucketize(v * scale, bins))


def test_gather_add_scatter_sum():
    from tts_king_amd import ops
    Bn, Lp, D, V = 4, 64, 256, 207
    g = torch.Generator().manual_seed(18)
    tok = torch.randint(0, V, (Bn, Lp), generator=g)
    tok[:, -5:] = 0
    table, pe = rnd(V, D, seed=19), rnd(Lp + 3, D, seed=20)
    out = ops.gather_add(None, table.to(DEV), tok.to(DEV), pe=pe.to(DEV), pe_mod=Lp, rows=Bn * Lp)
    ref = table[tok].reshape(-1, D) + pe[:Lp].repeat(Bn, 1)
    assert torch.equal(out.cpu(), ref.to(BF))
    spk_tab, spk = rnd(65, D, seed=21), torch.tensor([3, 64, 0, 3])
    out2 = ops.gather_add(out, spk_tab.to(DEV), spk.to(DEV), idx_div=Lp)
    ref2 = out.cpu().float() + spk_tab[spk].repeat_interleave(Lp, 0)
    assert torch.equal(out2.cpu(), ref2.to(BF))
    idx32 = torch.randint(0, 256, (Bn * Lp,), generator=g).int()
    out3 = ops.gather_add(out, rnd(256, D, seed=22).to(DEV), idx32.to(DEV))
    assert torch.equal(out3.cpu(), (out.cpu().float() + rnd(256, D, seed=22)[idx32.long()]).to(BF))
    # backward: deterministic scatter sums
    dx = rnd(Bn * Lp, D, seed=23).to(BF)
    dt = torch.ones(V, D)
    got = ops.scatter_sum(dx.to(DEV), tok.to(DEV), dt.to(DEV), skip_row=0, accumulate=True).cpu()
    want = torch.ones(V, D).double().index_add_(0, tok.reshape(-1), dx.double())
    want[0] = 1.0
    close_f32(got, want.float(), rtol=1e-5, atol=1e-5)
    ds = ops.scatter_sum(dx.to(DEV), spk.to(DEV), torch.zeros(65, D, device=DEV), idx_div=Lp, accumulate=False).cpu()
    wants = torch.zeros(65, D).double().index_add_(0, spk.repeat_interleave(Lp), dx.double())
    close_f32(ds, wants.float(), rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("xdt", [BF, torch.float32])
@pytest.mark.parametrize("C,use_tanh", [(512, True), (80, False)])
def test_batchnorm_train_fwd_bwd(C, use_tanh, xdt):
    from tts_king_amd import ops
    rows = 2 * 423
    x = rnd(rows, C, seed=24, scale=1.5).to(xdt)
    gamma, beta = 1 + 0.1 * rnd(C, seed=25), 0.1 * rnd(C, seed=26)
    rm, rv = 0.02 * rnd(C, seed=27), 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(28))
    resid = rnd(rows, C, seed=29)
    dout = rnd(rows, C, seed=30)
    xf = x.float().requires_grad_(True)
    g2, b2 = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm2, rv2 = rm.clone(), rv.clone()
    y = F.batch_norm(xf, rm2, rv2, g2, b2, training=True, momentum=0.1, eps=1e-5)
    y = torch.tanh(y) if use_tanh else y
    (y + resid).backward(dout)
    drm, drv, nbt = rm.to(DEV), rv.to(DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    mean, rstd = ops.bn_train_stats(x.to(DEV), drm, drv, nbt)
    close_f32(drm, rm2, rtol=1e-4, atol=1e-5)
    close_f32(drv, rv2, rtol=1e-4, atol=1e-5)
    assert int(nbt) == 1
    out = ops.bn_apply(x.to(DEV), mean, rstd, gamma.to(DEV), beta.to(DEV), use_tanh, resid=resid.to(DEV), out_f32=True)
    close_f32(out, (y + resid).detach(), rtol=1e-4, atol=1e-4)
    out16 = ops.bn_apply(x.to(DEV), mean, rstd, gamma.to(DEV), beta.to(DEV), use_tanh)
    close_bf16(out16, y.detach(), extra=1e-3)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx = ops.bn_bwd(dout.to(DEV), x.to(DEV), mean, rstd, gamma.to(DEV), beta.to(DEV), use_tanh, dgamma=dg, dbeta=db)
    close_bf16(dx, xf.grad, extra=2e-3)
    close_f32(dg, g2.grad, rtol=1e-3, atol=1e-2)
    close_f32(db, b2.grad, rtol=1e-3, atol=1e-2)
    # dropout keep-rate and fwd/bwd mask agreement
    st = ops.optim_state(DEV, seed=7)
    o = ops.bn_apply(x.to(DEV), mean, rstd, gamma.to(DEV), torch.ones(C, device=DEV) * 3, False, p=0.5, site=3, rng=ops.rng_of(st))
    keep = o.cpu().float() != 0
    assert abs(float(keep.float().mean()) - 0.5) < 0.02
    dxd = ops.bn_bwd(torch.ones(rows, C, device=DEV), x.to(DEV), mean, rstd, gamma.to(DEV), beta.to(DEV), False, p=0.5, site=3,
                     rng=ops.rng_of(st))
    assert dxd.shape == (rows, C)


@pytest.mark.parametrize("C,use_tanh,rows,seg", [(512, True, 2 * 423, 423), (80, False, 2 * 423, 423), (64, True, 3 * 40, 40), (512, True, 16 * 423, 423)])
def test_batchnorm_two_launch_path_equals_three_launch(C, use_tanh, rows, seg):
    """ops.bn_train (partials per channel slab + one kernel that finishes mean / rstd itself) against the stats / finalize /
    apply kernels: same statistics (1e-6), the same dropout mask, the same running buffers; with and without a frame limit;
    and its backward (bn_bwd takes the slab kernels by default) against the three-launch backward."""
    from tts_king_amd import ops
    assert ops.bn_slab_supported(C)
    x = rnd(rows, C, seed=40, scale=1.5).to(DEV)
    gamma, beta = (1 + 0.1 * rnd(C, seed=41)).to(DEV), (0.1 * rnd(C, seed=42)).to(DEV)
    resid = rnd(rows, C, seed=43).to(DEV)
    dout = rnd(rows, C, seed=44).to(DEV)
    st = ops.optim_state(DEV, seed=9)
    rng = ops.rng_of(st)
    for fl in (None, (torch.tensor([seg - 7], dtype=torch.int32, device=DEV), seg)):
        rm1, rv1, n1 = torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
        rm2, rv2, n2 = rm1.clone(), rv1.clone(), n1.clone()
        mean, rstd = ops.bn_train_stats(x, rm1, rv1, n1, frame_limit=fl)
        want = ops.bn_apply(x, mean, rstd, gamma, beta, use_tanh, p=0.5, site=302, rng=rng, resid=resid, out_f32=True, frame_limit=fl)
        got, m2, r2, keep = ops.bn_train(x, rm2, rv2, n2, gamma, beta, use_tanh, p=0.5, site=302, rng=rng, resid=resid, out_f32=True,
                                         frame_limit=fl, want_keep=True)
        close_f32(m2, mean.cpu(), rtol=1e-6, atol=1e-7)
        close_f32(r2, rstd.cpu(), rtol=1e-6, atol=1e-7)
        close_f32(rm2, rm1.cpu(), rtol=1e-6, atol=1e-7)
        close_f32(rv2, rv1.cpu(), rtol=1e-6, atol=1e-7)
        assert int(n2) == 1
        close_f32(got, want.cpu(), rtol=1e-5, atol=1e-5)
        dropped = (got == resid).view(rows, C // 4, 4)
        assert torch.equal(got == resid, want == resid)                      # the same elements dropped
        live = torch.ones(rows, dtype=torch.bool, device=DEV) if fl is None else (torch.arange(rows, device=DEV) % seg) < int(fl[0])
        bits = torch.stack([(keep >> e) & 1 for e in range(4)], dim=-1).bool()
        assert torch.equal(bits[live], ~dropped[live])                       # the keep bits say so too
        assert 0.48 < float(bits[live].float().mean()) < 0.52
        got16, _, _ = ops.bn_train(x, rm2.clone(), rv2.clone(), n2.clone(), gamma, beta, use_tanh, frame_limit=fl)
        close_bf16(got16, ops.bn_apply(x, mean, rstd, gamma, beta, use_tanh, frame_limit=fl).float().cpu(), extra=1e-3)
        # backward: slab kernels regenerating the mask, slab kernels reading the keep bits, the three-launch kernels
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        dx = ops.bn_bwd(dout, x, mean, rstd, gamma, beta, use_tanh, p=0.5, site=302, rng=rng, dgamma=dg, dbeta=db, frame_limit=fl)
        dgk, dbk = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        dxk = ops.bn_bwd(dout, x, mean, rstd, gamma, beta, use_tanh, p=0.5, site=302, rng=None, dgamma=dgk, dbeta=dbk, frame_limit=fl, keep=keep)
        assert torch.equal(dxk, dx) and torch.equal(dgk, dg) and torch.equal(dbk, db)
        ops.BN_SLAB = False
        try:
            dg0, db0 = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
            dx0 = ops.bn_bwd(dout, x, mean, rstd, gamma, beta, use_tanh, p=0.5, site=302, rng=rng, dgamma=dg0, dbeta=db0, frame_limit=fl)
        finally:
            ops.BN_SLAB = True
        close_bf16(dx, dx0.float().cpu(), extra=1e-3)
        close_f32(dg, dg0.cpu(), rtol=1e-4, atol=1e-3)
        close_f32(db, db0.cpu(), rtol=1e-4, atol=1e-3)


def test_loss_and_grads():
    from oracle import fs2 as ofs2
    from tts_king_amd import ops
    from tts_king_amd.synthetic import make_batch
    b = make_batch(4, 32, seed=31, ragged=True)
    Bn, Lp, T = 4, 32, b[8]
    mel = rnd(Bn, T, 80, seed=32).requires_grad_(True)
    post = rnd(Bn, T, 80, seed=33).requires_grad_(True)
    p, e, d = [rnd(Bn, Lp, seed=s).requires_grad_(True) for s in (34, 35, 36)]
    src_pad, mel_pad = ofs2.mask_from_lengths(b[4], Lp), ofs2.mask_from_lengths(b[7], T)
    out = (mel, p, e, d, None, src_pad, mel_pad, b[4], b[7], post, None, None)
    ls = ofs2.fs2_loss(b, out)
    (ls[0].sum() * 0.25).backward()
    dev = lambda t: t.detach().to(DEV)
    losses, dmel, dpost, dp, de, dd = ops.fs2_loss(dev(mel), dev(post), dev(b[6]), dev(b[7]), dev(p), dev(e), dev(d), dev(b[11]),
                                                   dev(b[9]), dev(b[10]), dev(b[4]), grad_scale=0.25)
    close_f32(losses[:5], torch.stack([l.sum().detach() for l in ls[:5]]), rtol=2e-5, atol=1e-6)
    assert float(losses[7]) == float(b[4].sum())
    close_f32(dpost, post.grad, rtol=1e-5, atol=1e-9)
    close_f32(dmel, mel.grad + post.grad, rtol=1e-5, atol=1e-9)
    close_f32(dp, p.grad, rtol=1e-5, atol=1e-9)
    close_f32(de, e.grad, rtol=1e-5, atol=1e-9)
    close_f32(dd, d.grad, rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("start", [0, 3999, 300000])
def test_clip_adam_lr(start):
    """ttsk_optim_step with one range over the whole buffer and no items, against clip + Adam + the lr rule restated in fp64; the
    scheduler / Adam counters (start 3999: across the warm-up boundary, 4000 -> 4001 at the second step), the lr of every step, the
    dropout counter with and without `advance_rng`, and the zeroed gradients."""
    from oracle import fs2 as ofs2
    from tts_king_amd import ops
    n = 100000
    p, g = rnd(n, seed=37), rnd(n, seed=38, scale=0.05)
    tables = ops.optim_tables([(0, n)], [], DEV)
    sched = (256, 4000, [300000, 400000, 500000], 0.7)
    b1, b2, eps = 0.95, 0.999, 1e-5
    for advance_rng in (False, True):
        st = ops.optim_state(DEV, seed=1, sched_step=start)
        dp, dg = p.to(DEV), g.to(DEV)
        m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        shadow = torch.empty(n, dtype=BF, device=DEV)
        partials = torch.empty(1024, device=DEV)
        pr, mr, vr = p.double().clone(), torch.zeros(n).double(), torch.zeros(n).double()
        for t in range(1, 4):
            dg.copy_(g * t)
            ops.optim_step(dp, dg, m, v, shadow, st, partials, 1.0, b1, b2, eps, *sched, tables, zero_grad=True, advance_rng=advance_rng)
            gg = (g * t).double()
            coef = min(1.0, 1.0 / (float(gg.norm()) + 1e-6))
            gg = gg * coef
            lr = ofs2.lr_at(start + t)
            mr = b1 * mr + (1 - b1) * gg
            vr = b2 * vr + (1 - b2) * gg * gg
            pr = pr - lr / (1 - b1 ** t) * mr / (vr.sqrt() / math.sqrt(1 - b2 ** t) + eps)
            assert float(dg.abs().max()) == 0.0
            stc = st.cpu()
            assert int(stc[0]) == start + t and int(stc[1]) == t
            assert int(stc[2]) == 1 and int(stc[3]) == (t if advance_rng else 0)          # dropout seed kept, counter ticked on request only
            lr_dev = stc[4:5].view(torch.float32)[0]
            assert abs(float(lr_dev) - lr) < 1e-9 + 1e-6 * lr
        np.testing.assert_allclose((dp.cpu().double() - p.double()).numpy(), (pr - p.double()).numpy(), rtol=2e-3, atol=6e-7)  # fp32 ulp of |p| <= 4
        assert torch.equal(shadow.cpu(), dp.cpu().to(BF))


def test_conversions():
    from tts_king_amd import ops
    x = rnd(3, 80, 50, seed=39)
    assert torch.equal(ops.nct_to_ntc(x.to(DEV)).cpu(), x.transpose(1, 2).to(BF))
    w = rnd(1003, seed=40)
    w4 = torch.zeros(1004); w4[:1003] = w
    assert torch.equal(ops.cast_bf16(w4.to(DEV)).cpu(), w4.to(BF))
    a = torch.tensor([0.99999, -0.99999, 0.5, -0.5, 1e-5, -1e-5, 0.123456, -0.654321, 0.0])
    got = ops.to_int16(a.to(DEV), 32768.0).cpu().numpy()
    np.testing.assert_array_equal(got, (a * 32768).numpy().astype("int16"))


def test_va_embed_and_combine_match_step_by_step_kernels():
    """ttsk_va_embed == gather_add(speaker) -> bucketize -> gather_add(pitch) -> bucketize -> gather_add(energy), bit for bit;
    ttsk_va_combine == the three rounded residual adds."""
    from tts_king_amd import ops
    Bn, Lp, D, nb = 5, 24, 256, 256
    rows = Bn * Lp
    g = torch.Generator().manual_seed(3)
    stack = torch.zeros(3, rows, D, dtype=BF, device=DEV)
    stack[0] = rnd(rows, D, seed=1).to(BF).to(DEV)
    spk_t, p_t, e_t = rnd(7, D, seed=2).to(DEV), rnd(nb, D, seed=3).to(DEV), rnd(nb, D, seed=4).to(DEV)
    speakers = torch.randint(0, 7, (Bn,), generator=g).to(DEV)
    pbins, ebins = torch.linspace(-2, 2, nb - 1).to(DEV), torch.linspace(-1, 3, nb - 1).to(DEV)
    pt, et = (rnd(rows, seed=5) * 1.5).to(DEV), (rnd(rows, seed=6) * 1.5 + 1).to(DEV)
    pt[3] = pbins[10]                                      # a value exactly on an edge: right=False puts it in bucket 10
    x3, pidx, eidx = ops.va_embed(stack, speakers, spk_t, Lp, pt, pbins, p_t, et, ebins, e_t)
    x1 = ops.gather_add(stack[0], spk_t, speakers, idx_div=Lp)
    pi = ops.bucketize(pt, pbins)
    x2 = ops.gather_add(x1, p_t, pi)
    ei = ops.bucketize(et, ebins)
    x3w = ops.gather_add(x2, e_t, ei)
    assert torch.equal(pidx, pi) and torch.equal(eidx, ei) and int(pidx[3]) == 10
    assert torch.equal(pidx.cpu().long(), torch.bucketize(pt.cpu(), pbins.cpu()))
    assert torch.equal(stack[1], x1) and torch.equal(stack[2], x2) and torch.equal(x3, x3w)
    dx3 = rnd(rows, D, seed=7).to(BF).to(DEV)
    dxin = rnd(3, rows, D, seed=8).to(DEV)
    dx2, dx1, dx = ops.va_combine(dx3, dxin)
    w2 = (dx3.float() + dxin[2]).to(BF)
    w1 = (w2.float() + dxin[1]).to(BF)
    w0 = (w1.float() + dxin[0]).to(BF)
    assert torch.equal(dx2, w2) and torch.equal(dx1, w1) and torch.equal(dx, w0)


def test_grouped_layernorm_equals_single_launches():
    """One grouped launch over 3 parameter sets == 3 single launches, bit for bit (forward with post-dropout + head, backward)."""
    from tts_king_amd import ops
    G, Bn, seg, D, p = 3, 4, 32, 256, 0.5
    rows = Bn * seg
    stride = 1032                                            # floats between the groups' parameter blocks (16-byte aligned)
    flat = rnd(G * stride + 4 * D, seed=20).to(DEV)          # gamma | beta | head_w | head_b inside each block
    y = torch.relu(rnd(G * rows, D, seed=21)).to(BF).to(DEV)
    lens = torch.tensor([32, 20, 7, 32]).to(DEV)
    dhead = rnd(G * rows, seed=22).to(DEV)
    st = ops.optim_state(DEV, seed=5)
    rng = ops.rng_of(st)
    gam, bet, hw, hb = flat[0:D], flat[D:2 * D], flat[2 * D:3 * D], flat[3 * D:3 * D + 1]
    _, mean, rstd, ho = ops.layernorm_fwd_grouped(y, gam, bet, G, stride, 2, lens, seg, p_post=p, site_post=201, rng=rng, head=(hw, hb), want_out=False)
    out, *_ = ops.layernorm_fwd_grouped(y, gam, bet, G, stride, 2, None, 0, p_post=p, site_post=200, rng=rng)
    dz, part, nblk = ops.layernorm_bwd_grouped(None, y, mean, rstd, gam, bet, G, stride, 2, lens, seg, relu_in=True, p_post=p, site_post=201,
                                               rng=rng, dhead=dhead, head_w=hw)
    for g in range(G):
        o = g * stride
        sl = slice(g * rows, (g + 1) * rows)
        gg, bb, ww, wb = flat[o:o + D], flat[o + D:o + 2 * D], flat[o + 2 * D:o + 3 * D], flat[o + 3 * D:o + 3 * D + 1]
        _, _, m1, r1, h1 = ops.layernorm_fwd(y[sl], None, gg, bb, lens, seg, p_post=p, site_post=201 + 2 * g, rng=rng, save_z=False, head=(ww, wb), want_out=False)
        o1, *_ = ops.layernorm_fwd(y[sl], None, gg, bb, None, 0, p_post=p, site_post=200 + 2 * g, rng=rng, save_z=False)
        assert torch.equal(h1, ho[sl]) and torch.equal(m1, mean[sl]) and torch.equal(r1, rstd[sl]) and torch.equal(o1, out[sl])
        dz1, _, p1, n1 = ops.layernorm_bwd(None, y[sl], m1, r1, gg, bb, lens, seg, relu_in=True, p_post=p, site_post=201 + 2 * g, rng=rng,
                                           dhead=dhead[sl], head_w=ww)
        assert n1 == nblk and torch.equal(dz1, dz[sl]) and torch.equal(p1, part[g])


# ------------------------------------------------------------------------------------------------ bias-gradient column sums

def _colsum_input(rows, C, ld, dt, seed):
    """(rows, C) column slice at offset C of a (rows, ld) matrix — the layout of the q|k|v bias gradient's middle third."""
    big = rnd(rows, ld, seed=seed).to(dt)
    off = C if ld >= 2 * C else 0
    return big, off


@pytest.mark.parametrize("dt", [BF, torch.float32])
@pytest.mark.parametrize("C,ld", [(4, 12), (80, 240), (256, 768), (1024, 1280)])
def test_colsum_into_vs_fp64(C, ld, dt):
    """ttsk_colsum + ttsk_colsum_finalize (every bias gradient of the step) against an fp64 column sum, at row counts on both
    sides of the 16-row block and of the 256-block cap (rows > 4080), with a column slice of a wider matrix (ld > C), bf16 and
    fp32 inputs, accumulate on and off.  Error bound: fp32 summation of at most 6768 terms, 2e-6 of the column's sum of |x|."""
    from tts_king_amd import ops
    for rows in (1, 15, 16, 17, 4080, 4081, 6768):
        big, off = _colsum_input(rows, C, ld, dt, seed=rows + C)
        x = big.to(DEV)[:, off:off + C]
        assert x.stride(0) == ld
        xs = big[:, off:off + C].double()
        ref = xs.sum(0)
        bound = 2e-6 * xs.abs().sum(0) + 1e-7
        for acc in (False, True):
            dst0 = rnd(C, seed=3) if acc else torch.full((C,), 777.0)
            got = ops.colsum_into(x, dst0.to(DEV), accumulate=acc).cpu().double()
            want = ref + (dst0.double() if acc else 0.0)
            err = (got - want).abs()
            assert bool((err <= bound + (1e-6 * dst0.double().abs() if acc else 0.0)).all()), (rows, C, acc, float(err.max()))


@pytest.mark.parametrize("nblk,ncols,ld", [(1, 4, 4), (15, 80, 96), (16, 256, 768), (17, 1024, 1024), (64, 80, 80), (65, 12, 20), (256, 512, 768)])
def test_colsum_finalize_vs_fp64(nblk, ncols, ld):
    """ttsk_colsum_finalize: dst (+)= scale * sum_b partials[b * ld + c] for c < ncols (the 4-loads-in-flight loop and its remainder
    at nblk around 16 / 64, a partials row stride ld > ncols), scale 1 and not 1, accumulate on and off, against fp64."""
    from tts_king_amd import ops
    part = rnd(nblk, ld, seed=nblk + ld, scale=10.0)
    ref = part[:, :ncols].double().sum(0)
    for scale in (1.0, 0.37):
        for acc in (False, True):
            dst0 = rnd(ncols, seed=8)
            sentinel = torch.full((ncols + 8,), -5.0)
            sentinel[:ncols] = dst0
            dst = sentinel.to(DEV)
            ops.colsum_finalize(part.to(DEV), nblk, ncols, ld, dst, accumulate=acc, scale=scale)
            got = dst.cpu().double()
            want = scale * ref + (dst0.double() if acc else 0.0)
            tol = 1e-6 * (scale * part[:, :ncols].double().abs().sum(0) + dst0.double().abs()) + 1e-7
            assert bool(((got[:ncols] - want).abs() <= tol).all()), (scale, acc, float((got[:ncols] - want).abs().max()))
            assert bool((got[ncols:] == -5.0).all())                         # nothing past ncols is written


def test_colsum_deferred_batch_equals_immediate_calls():
    """The deferred path of the backward pass (colsum_into(defer=...) queues the column sum and its finalisation; flush_finalize
    runs them as ttsk_colsum_batch + ttsk_colsum_finalize_batch, in chunks of 64 items) is bit-identical to the immediate calls —
    with 70 queued column sums (> 64: two chunks each), mixed dtypes, widths, row counts, slices and accumulate flags."""
    from tts_king_amd import ops
    shapes = []
    for i in range(70):
        C, ld = [(4, 12), (80, 240), (256, 768), (1024, 1024), (512, 512)][i % 5]
        rows = [1, 17, 423, 4081, 6768, 64, 2016][i % 7]
        shapes.append((rows, C, ld, BF if i % 3 else torch.float32, bool(i % 2)))
    xs, dsts0 = [], []
    for i, (rows, C, ld, dt, acc) in enumerate(shapes):
        big, off = _colsum_input(rows, C, ld, dt, seed=100 + i)
        xs.append(big.to(DEV)[:, off:off + C])
        dsts0.append(rnd(C, seed=200 + i).to(DEV))
    immediate = [ops.colsum_into(x, d.clone(), accumulate=acc) for x, d, (_, _, _, _, acc) in zip(xs, dsts0, shapes)]
    queue, deferred = [], []
    for x, d, (_, _, _, _, acc) in zip(xs, dsts0, shapes):
        deferred.append(ops.colsum_into(x, d.clone(), accumulate=acc, defer=queue))
    # ... and finalisations queued on their own with scale != 1 (the path of the LayerNorm-family bias gradients)
    parts = [rnd(nb, ld, seed=300 + i) for i, (nb, ld) in enumerate([(1, 80), (17, 256), (64, 768), (65, 1024), (256, 512)])]
    fin_now, fin_later = [], []
    for i, pt in enumerate(parts):
        nb, ld = pt.shape
        nc = ld if i % 2 else ld // 3
        d0 = rnd(nc, seed=400 + i).to(DEV)
        fin_now.append(ops.colsum_finalize(pt.to(DEV), nb, nc, ld, d0.clone(), accumulate=bool(i % 2), scale=0.37 + i))
        fin_later.append(ops.colsum_finalize(pt.to(DEV), nb, nc, ld, d0.clone(), accumulate=bool(i % 2), scale=0.37 + i, defer=queue))
    assert len(queue) == 140 + len(parts)
    ops.flush_finalize(queue)
    assert queue == []
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(immediate + fin_now, deferred + fin_later)):
        assert torch.equal(a, b), (i, float((a - b).abs().max()))


# ------------------------------------------------------------------------------------------------ eval helpers

@pytest.mark.parametrize("d_control", [0.5, 1.0, 2.3])
def test_duration_round_vs_fp64_rule(d_control):
    """ttsk_duration_round against clamp(round_half_even(exp(x) - 1) * d_control, 0) (reference: modules.py:199-203) with the
    rounding decided in fp64: negative log-durations (rounding to 0 and to -1, clamped), n = 1037 (not a multiple of 256).
    Positions within 1e-5 of a rounding tie are left out (the device's expf may differ from fp64 by an ulp there)."""
    from tts_king_amd import ops
    x = torch.cat([torch.linspace(-4.0, 3.5, 1000), rnd(37, seed=41)]).float()
    got = ops.duration_round(x.to(DEV), d_control).cpu()
    v = torch.exp(x.double()) - 1.0
    k = torch.round(v)                                                   # torch.round: half to even
    want = torch.clamp(k.float() * torch.tensor(d_control, dtype=torch.float32), min=0.0)
    tie = (v - torch.floor(v) - 0.5).abs() < 1e-5
    assert int(tie.sum()) < 10 and bool((x < 0).sum() > 300) and bool((k == -1).any())
    bad = (got != want) & ~tie
    assert not bool(bad.any()), (x[bad][:5].tolist(), got[bad][:5].tolist(), want[bad][:5].tolist())


@pytest.mark.parametrize("T", [77, 1031])
def test_length_mask_exact(T):
    """ttsk_length_mask: mask[b, t] = t >= lens[b] for lens in {0, 1, T-1, T, T+5}; B * T not a multiple of 256."""
    from tts_king_amd import ops
    lens = torch.tensor([0, 1, T - 1, T, T + 5], dtype=torch.int64)
    assert (len(lens) * T) % 256 != 0
    got = ops.length_mask(lens.to(DEV), T).cpu()
    assert got.dtype == torch.bool and tuple(got.shape) == (5, T)
    assert torch.equal(got, torch.arange(T)[None, :] >= lens[:, None])
