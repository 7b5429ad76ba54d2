"""CPU: tests/dw_ref.py (the fp64 restatement that tests/test_dw_edges_gpu.py holds csrc/dwgemm.hip and csrc/dwconv.hip to) against
what torch itself leaves in `weight.grad` of an fp64 F.conv1d(padding = k // 2) whose output gradient is zero at rows >= len — the
operation the kernels stand in for — and its error bar against the same sum carried out in fp32 in 32-row pieces."""
import pytest
import torch
import torch.nn.functional as F

from tests.dw_ref import clamp_lens, dw_abs_ref, dw_bar, dw_fp32_chunked, dw_ref, rows_walked

B, S, COUT, CIN = 5, 21, 6, 4
LENS = [None, [21, 0, 7, 1, 20], [0, 0, 0, 0, 0], [21, 21, 21, 21, 21], [30, -2, 11, 21, 0]]


def _operands(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, S, COUT, generator=g, dtype=torch.float64), torch.randn(B, S, CIN, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("lens", LENS, ids=lambda v: "none" if v is None else "-".join(map(str, v)))
@pytest.mark.parametrize("k", [1, 3, 5, 9])
def test_dw_ref_is_torch_conv1d_weight_grad(k, lens):
    """`weight.grad` is (Cout, Cin, k); the kernels' layout is (Cout, k, Cin).  x is NOT zeroed past len: with the output gradient
    zero there, torch's sum takes the rows x[len .. len + k//2) beside the last live rows exactly as dw_ref states."""
    dy, x = _operands(k)
    ln = clamp_lens(lens, B, S)
    w = torch.zeros(COUT, CIN, k, dtype=torch.float64, requires_grad=True)
    y = F.conv1d(x.transpose(1, 2), w, padding=k // 2)                        # (B, Cout, S)
    gy = dy.clone()
    for b in range(B):
        gy[b, ln[b]:] = 0
    y.backward(gy.transpose(1, 2))
    want = w.grad.permute(0, 2, 1)
    dyn = dy.clone()
    if lens is not None:
        for b in range(B):
            dyn[b, ln[b]:] = float("nan")                                     # dead dY rows never enter, whatever they hold
    got = dw_ref(dyn, x, k, lens)
    assert got.shape == (COUT, k, CIN) and got.dtype == torch.float64
    assert float((got - want).abs().max()) <= 1e-12
    if rows_walked(lens, B, S) == 0:
        assert not got.any()


def test_dw_ref_elementwise_loops():
    """The definition as four nested loops, one element at a time (no einsum, no padding trick), and the |.| sum beside it."""
    k, lens = 5, [3, 0, 21, 20, 1]
    dy, x = _operands(11)
    want = torch.zeros(COUT, k, CIN, dtype=torch.float64)
    wabs = torch.zeros_like(want)
    for b in range(B):
        for t in range(lens[b]):
            for j in range(k):
                s = t + j - k // 2
                if 0 <= s < S:
                    want[:, j] += dy[b, t][:, None] * x[b, s][None, :]
                    wabs[:, j] += (dy[b, t][:, None] * x[b, s][None, :]).abs()
    assert float((dw_ref(dy, x, k, lens) - want).abs().max()) <= 1e-12
    assert float((dw_abs_ref(dy, x, k, lens) - wabs).abs().max()) <= 1e-12


def test_x_rows_past_len_take_part_and_dy_rows_do_not():
    k, lens = 9, [7, 21, 0, 10, 1]
    dy, x = _operands(3)
    base = dw_ref(dy, x, k, lens)
    x2, dy2 = x.clone(), dy.clone()
    x2[0, 7:11] += 1.0                       # X[len .. len + k//2): beside live dY rows under the taps j > k//2
    assert float((dw_ref(dy, x2, k, lens) - base)[:, k // 2 + 1:].abs().max()) > 0
    assert torch.equal(dw_ref(dy, x2, k, lens)[:, :k // 2 + 1], base[:, :k // 2 + 1])
    x3 = x.clone()
    x3[0, 11:] += 1.0                        # further out: never read
    x3[2] += 1.0                             # an empty utterance's rows: never read
    assert torch.equal(dw_ref(dy, x3, k, lens), base)
    dy2[0, 7:] = float("inf")
    dy2[2] = float("nan")
    assert torch.equal(dw_ref(dy2, x, k, lens), base)


@pytest.mark.parametrize("k,splits", [(1, 1), (5, 3), (9, 1)])
def test_bar_holds_for_fp32_in_32_row_pieces(k, splits):
    """The per-element bar of the GPU tests is derived, not measured; the same sum in fp32 on the CPU, accumulated in 32-row pieces as
    the kernels' K steps do, must stay inside it — at operands whose channels span 2^16 in size, as the GPU tests scale them."""
    g = torch.Generator().manual_seed(k)
    Bn, Sn, Co, Ci = 3, 70, 24, 16
    dy = (torch.randn(Bn, Sn, Co, generator=g) * 2.0 ** -(torch.arange(Co) % 11).float()).to(torch.bfloat16)
    x = (torch.randn(Bn, Sn, Ci, generator=g) * 2.0 ** -(torch.arange(Ci) % 7).float()).to(torch.bfloat16)
    lens = [70, 33, 5]
    want, bar = dw_ref(dy, x, k, lens), dw_bar(dy, x, k, lens, splits)
    err = (dw_fp32_chunked(dy, x, k, lens).double() - want).abs()
    assert bool((err <= bar).all()), float((err / bar.clamp_min(1e-300)).max())
    assert float(bar.max()) / float(bar[bar > 0].min()) > 2.0 ** 12            # a bar per element, not one of the maximum
