"""GPU: utterances joined into one waveform (csrc/join.hip, ops.wav_join) against the numpy restatement (tests/join_ref.py).

Bars.  The kept ranges, the layout, the peak and the timing are decisions on exact comparisons: equal.  In mode "given" the copy is
two fp32 multiplications per sample (and the fade's one correctly rounded division): bit for bit.  The sum of squares is the one
quantity whose rounding depends on the reduction's shape: |ss - ss_fp64| <= gamma_k * ss_fp64 with k read off the kernel
(join_ref.ss_bound, derived there); the gain of the modes "rms" / "peak" inherits that bound through a division, a square root and a
division (join_ref.gain_bound), and the copy is then bit for bit the restatement's under the device's own gain."""
import numpy as np
import pytest
import torch

from tests import join_ref as ref
from tts_king_amd import narrate, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = 20                       # the table's capacity: the utterances below, then padding rows
R45 = np.float32(10.0 ** (-45.0 / 20.0))


def _utterances(rng):
    """(name, samples) in the order the flat buffer holds them."""
    g = lambda n, s=0.1: (rng.standard_normal(n) * s).astype(np.float32)
    out = [("n%d" % n, g(n)) for n in (1, 63, 64, 65, 255, 256)]
    out.append(("empty", np.zeros(0, np.float32)))                     # a zero-length row in the middle
    out += [("n4352", g(4352)), ("n20000", g(20000))]
    out.append(("zeros", np.zeros(300, np.float32)))
    first = g(500, 1e-5)
    first[0] = 0.5
    last = g(700, 1e-5)
    last[-1] = -0.6
    out += [("first", first), ("last", last)]
    out.append(("loud", (rng.uniform(0.3, 0.9, 900) * rng.choice([-1.0, 1.0], 900)).astype(np.float32)))
    burst = g(2900, 1e-5)
    burst[1000:1700] = g(700, 0.2)
    burst[1000], burst[1699] = 0.4, -0.4                               # the burst's edges are above the threshold, whatever was drawn
    out.append(("burst", burst))
    return out


def _lay_out(utts, misalign):
    """The flat buffer (what lies between the utterances is loud and never signal) and every utterance's offset: with `misalign`
    no offset is a multiple of 4 samples, without it every one is."""
    offs, pos, parts = [], 0, []
    for i, (_, x) in enumerate(utts):
        gap = 3 + (i % 3)
        start = pos + gap
        start += (1 + i % 3 - start % 4) % 4 if misalign else -start % 4
        parts.append(np.full(start - pos, 7.0, np.float32))
        parts.append(x)
        offs.append(start)
        pos = start + len(x)
    parts.append(np.full(5, 7.0, np.float32))
    flat = np.concatenate(parts)
    assert all((o % 4 != 0) == misalign for o in offs)
    return flat, offs


@pytest.fixture(scope="module")
def data():
    utts = _utterances(np.random.default_rng(22))
    d = {"utts": utts, "lens": [len(x) for _, x in utts]}
    for mis in (True, False):
        flat, offs = _lay_out(utts, mis)
        d[mis] = (flat, offs, torch.from_numpy(flat).to(DEV))
    return d


def _table(data, mis, mode=narrate.GIVEN, fade=0, keep=0, lead=0, trim=True, pauses=(0, 1, 1000), gains=(2.0, 0.5, 1.0, 0.7)):
    _, offs, _ = data[mis]
    U = len(offs)
    st = narrate.Settings(mode, fade, keep, lead, r=R45, floor=1e-4, target=10.0 ** (-23.0 / 20.0), limit=0.95, trim=trim)
    return narrate.join_table(offs, data["lens"], [pauses[u % len(pauses)] for u in range(U)], st, rows=ROWS,
                              gains=[gains[u % len(gains)] for u in range(U)])


def _run(data, mis, table, scale=None, extra=37):
    """The kernels on a destination filled with NaN (int16: with 0x7f7f) beforehand, `extra` samples larger than the table can fill."""
    flat, _, x = data[mis]
    n_dst = narrate.out_bound(table) + extra
    if scale is None:
        out = torch.full((n_dst,), float("nan"), dtype=torch.float32, device=DEV)
    else:
        out = torch.full((n_dst,), 0x7f7f, dtype=torch.int16, device=DEV)
    info = torch.full((ROWS + 1, narrate.ROW), -1, dtype=torch.int32, device=DEV)
    ops.wav_join(x, torch.from_numpy(table).to(DEV), out=out, info=info, int16_scale=scale)
    torch.cuda.synchronize()
    return out.cpu().numpy(), narrate.Info(info.cpu().numpy())


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _check_decisions(info, want):
    assert info.a.tolist() == want["a"].tolist() and info.b.tolist() == want["b"].tolist()
    assert info.o.tolist() == want["o"].tolist() and info.total == want["total"]
    assert np.array_equal(_bits(np.ascontiguousarray(info.peak)), _bits(want["peak"]))
    assert info.timing() == want["timing"]


@pytest.mark.parametrize("mis", [True, False])
@pytest.mark.parametrize("fade,keep,lead,trim,scale", [(0, 0, 0, True, None), (1, 3, 5, True, None), (7, 40, 0, True, None), (40, 330, 2, True, None),
                                                       (7, 0, 0, False, None), (0, 0, 3, True, 32767.0), (7, 40, 0, True, 32767.0),
                                                       (40, 0, 1, False, 32767.0)])
def test_given_gains_bit_for_bit(data, mis, fade, keep, lead, trim, scale):
    """Mode "given": gains 1, 0.5, 2, 0.7, pauses 0, 1, 1000, fades 0, 1, 7 and 40 (more than half of the kept ranges up to 65
    samples; every fade >= 1 is more than half of the one-sample utterance).  int16 at scale 32767: the loud utterance (row 12, gain 2)
    reaches +-1.8, so saturation runs on both sides."""
    table = _table(data, mis, fade=fade, keep=keep, lead=lead, trim=trim)
    got, info = _run(data, mis, table, scale)
    want = ref.join_ref(data[mis][0], table, got.size, scale)
    _check_decisions(info, want)
    names = [n for n, _ in data["utts"]]
    if trim:
        kept = dict(zip(names, zip(info.a.tolist(), info.b.tolist())))
        assert kept["zeros"] == (0, 0) and kept["empty"] == (0, 0)
        assert kept["first"] == (0, min(500, 1 + keep)) and kept["last"] == (max(0, 699 - keep), 700)
        assert kept["loud"] == (0, 900) and kept["burst"] == (max(0, 1000 - keep), min(2900, 1700 + keep))
    assert np.array_equal(_bits(got), _bits(want["out"]))
    assert not got[info.total:].any() and got.size - info.total >= 37          # zeros from the end on, where NaN stood
    if scale is not None:
        assert (got == 32767).any() and (got == -32768).any()


@pytest.mark.parametrize("mis", [True, False])
def test_sum_of_squares_within_the_reduction_bound(data, mis):
    """ss against fp64 on the Gaussian utterances and on the burst, trimmed and whole: |ss - ss64| <= ss_bound(m) * ss64 (derived at
    join_ref.ss_bound from the reduction's shape), plus 2^-149 per term for squares that underflow."""
    for trim in (True, False):
        table = _table(data, mis, trim=trim, keep=10)
        _, info = _run(data, mis, table)
        want = ref.join_ref(data[mis][0], table, 1)
        for u, (name, _) in enumerate(data["utts"]):
            m = int(info.b[u] - info.a[u])
            err = abs(float(info.ss[u]) - want["ss64"][u])
            bound = ref.ss_bound(m) * want["ss64"][u] + m * 2.0 ** -149 if m else 0.0
            print("%s trim=%d m=%d ss=%.9g ss64=%.17g err=%.3g bound=%.3g" % (name, trim, m, info.ss[u], want["ss64"][u], err, bound))
            assert err <= bound, (name, trim)


@pytest.mark.parametrize("mode", [narrate.RMS, narrate.PEAK])
@pytest.mark.parametrize("fade,scale", [(0, None), (7, None), (7, 32767.0)])
def test_levelled_modes(data, mode, fade, scale):
    """Modes "rms" and "peak": the gain within join_ref.gain_bound of the restatement's; the copy bit for bit the restatement's under
    the device's gain; and, without a fade, every non-empty sentence's RMS over its kept samples of the output within that bound
    (plus the copy's one rounding per sample) of the target, or its peak at the limit."""
    table = _table(data, True, mode=mode, fade=fade, keep=330)        # 330 kept samples of near-silence: "first" / "last" get a crest above limit / target
    got, info = _run(data, True, table, scale)
    flat = data[True][0]
    own = ref.join_ref(flat, table, got.size, scale)
    _check_decisions(info, own)
    target, limit = (float(v) for v in table[0, 6:8].view(np.float32))
    for u, (name, _) in enumerate(data["utts"]):
        m = int(info.b[u] - info.a[u])
        rel = abs(float(info.g[u]) - float(own["g"][u])) / float(own["g"][u])
        print("%s m=%d g=%.9g want %.9g rel=%.3g bound=%.3g" % (name, m, info.g[u], own["g"][u], rel, ref.gain_bound(max(m, 1))))
        assert rel <= (ref.gain_bound(m) if m else 0.0), name
    want = ref.join_ref(flat, table, got.size, scale, g_device=info.g)
    assert np.array_equal(_bits(got), _bits(want["out"]))
    assert not got[info.total:].any()
    if fade == 0 and scale is None:
        some_rms = some_peak = False
        for u, (name, _) in enumerate(data["utts"]):
            m = int(info.b[u] - info.a[u])
            if not m:
                continue
            y = got[info.o[u]:info.o[u] + m].astype(np.float64)
            rms, peak = float(np.sqrt(np.mean(y * y))), float(np.abs(y).max())
            at_target = abs(rms - target) <= (ref.gain_bound(m) + 2 * ref.U_ROUND) * target
            # the peak sample is the row's peak only when nothing louder was trimmed away: it never is (a sample at the peak is kept)
            at_limit = abs(peak - limit) <= 3 * ref.U_ROUND * limit
            print("%s rms=%.9g target=%.9g peak=%.9g limit=%.9g" % (name, rms, target, peak, limit))
            assert peak <= limit * (1 + 3 * ref.U_ROUND), name
            assert at_limit if mode == narrate.PEAK else (at_target or at_limit), name
            some_rms, some_peak = some_rms or at_target, some_peak or at_limit
        assert some_peak and (some_rms or mode == narrate.PEAK)            # both branches of the min ran


def test_two_runs_same_bits(data):
    table = _table(data, True, mode=narrate.RMS, fade=7, keep=20)
    a, ia = _run(data, True, table)
    b, ib = _run(data, True, table)
    assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(np.ascontiguousarray(ia.ss)), _bits(np.ascontiguousarray(ib.ss)))
    assert np.array_equal(_bits(np.ascontiguousarray(ia.g)), _bits(np.ascontiguousarray(ib.g)))


def test_place_does_not_matter(data):
    """A row's numbers depend on its samples, not on where it lies: the aligned and the misaligned layout give the same table and bits."""
    ta, tm = _table(data, False, mode=narrate.RMS, fade=7, keep=20), _table(data, True, mode=narrate.RMS, fade=7, keep=20)
    a, ia = _run(data, False, ta)
    b, ib = _run(data, True, tm)
    assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(np.ascontiguousarray(ia.ss)), _bits(np.ascontiguousarray(ib.ss)))


def test_destination_too_small_is_cut_not_overrun(data):
    """A destination smaller than the waveform: what fits is written, the rest dropped, `total` still the full length."""
    table = _table(data, True)
    full, info = _run(data, True, table)
    n = 5001
    out = torch.full((n + 64,), float("nan"), dtype=torch.float32, device=DEV)
    ops.wav_join(data[True][2], torch.from_numpy(table).to(DEV), out=out[:n])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got[:n]), _bits(full[:n])) and np.isnan(got[n:]).all() and info.total > n


def test_a_row_outside_the_source_counts_as_empty(data):
    table = _table(data, True)
    bad = table.copy()
    bad[1 + 8, 0] = data[True][0].size - 100                              # the 20000-sample row now ends past the buffer
    got, info = _run(data, True, bad)
    want = ref.join_ref(data[True][0], bad, got.size)
    _check_decisions(info, want)
    assert (info.a[8], info.b[8]) == (0, 0) and np.array_equal(_bits(got), _bits(want["out"]))


def test_wrapper_refusals(data):
    x = data[True][2]
    table = torch.from_numpy(_table(data, True)).to(DEV)
    L = ops.L
    with pytest.raises(L.TtskError, match="join table"):
        ops.wav_join(x, table[:, :4].contiguous(), n_dst=100)
    with pytest.raises(L.TtskError, match="join table"):
        ops.wav_join(x.double(), table, n_dst=100)
    with pytest.raises(L.TtskError, match="n_dst"):
        ops.wav_join(x, table)
    with pytest.raises(L.TtskError, match="`out` must be"):
        ops.wav_join(x, table, out=torch.empty(10, dtype=torch.int16, device=DEV))
    with pytest.raises(L.TtskError, match="`info` must be"):
        ops.wav_join(x, table, n_dst=100, info=torch.empty(3, 8, dtype=torch.int32, device=DEV))
    with pytest.raises(L.TtskError, match="at most 4096"):
        ops.wav_join(x, torch.zeros(4098, 8, dtype=torch.int32, device=DEV), n_dst=100)
    with pytest.raises(L.TtskError, match="no CPU path"):
        ops.wav_join(x.cpu(), table, n_dst=100)
