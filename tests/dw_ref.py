"""The weight gradient that tts_king_amd/csrc/dwgemm.hip and csrc/dwconv.hip compute, restated once in fp64 on the CPU:

    dW[co, j, ci] = sum_b sum_{t < len_b} dy[b, t, co] * x[b, t + j - k//2, ci]

* `x` is taken AS STORED for 0 <= t + j - k//2 < S and as zero outside (the conv's zero padding; never the neighbouring utterance);
* `lens` is clamped to [0, S]; None = every row;
* `lens` masks dY ONLY.  That is the kernels' contract: dwgemm loads an X row only beside a live dY row, dwconv fetches the whole
  window of X and multiplies the rows beside dead dY rows by the zeros the buffer load returns for those.  So the rows
  X[len .. len + k//2) DO take part (they meet the last live dY rows through the tap shift), whatever they hold, and the values of
  dY at rows >= len never do, whatever they hold (NaN included).

tests/test_dw_ref_cpu.py ties this to torch's own `weight.grad` of an fp64 conv1d; tests/test_dw_edges_gpu.py holds the kernels to it.
`dw_abs_ref` is the same sum over |dy * x|: the scale of the per-element rounding bar (`dw_bar`)."""
import torch


def clamp_lens(lens, B, S):
    """`lens` as a list of B ints in [0, S]; None = all S."""
    if lens is None:
        return [S] * B
    lens = [int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
    assert len(lens) == B
    return [min(max(v, 0), S) for v in lens]


def rows_walked(lens, B, S):
    """n of the bar: the dY rows that enter the sum."""
    return sum(clamp_lens(lens, B, S))


def _sum(dy, x, k, lens):
    B, S, Cout = dy.shape
    assert x.shape[:2] == (B, S) and k % 2 == 1
    live = torch.arange(S)[None, :] < torch.tensor(clamp_lens(lens, B, S))[:, None]
    dym = torch.where(live[:, :, None], dy, torch.zeros((), dtype=dy.dtype))          # (where, not a product: dead rows may hold NaN)
    xp = torch.nn.functional.pad(x, (0, 0, k // 2, k // 2))
    return torch.stack([torch.einsum("btc,bti->ci", dym, xp[:, j:j + S]) for j in range(k)], dim=1)


def dw_ref(dy, x, k, lens=None):
    """(Cout, k, Cin) fp64."""
    return _sum(dy.detach().cpu().double(), x.detach().cpu().double(), k, lens)


def dw_abs_ref(dy, x, k, lens=None):
    """The same sum over |dy * x|, fp64."""
    return _sum(dy.detach().cpu().double().abs(), x.detach().cpu().double().abs(), k, lens)


def dw_bar(dy, x, k, lens=None, splits=1, old_abs=0.0):
    """Per-element bound on |fp32 result - dw_ref| for bf16 operands: (n + splits + 1) * 2^-24 * dw_abs_ref.  The products of two bf16
    numbers are exact in fp32; an fp32 sum of n exact terms in ANY order is within (n - 1) u sum|terms| of the true sum to first order
    (u = 2^-24, round to nearest), the sum of `splits` slabs adds at most `splits` u, and the remaining terms cover the second order
    (n u << 1 here) and one more addend: the destination's old value when accumulating, whose magnitude `old_abs` then joins the
    sum of magnitudes."""
    B, S, _ = dy.shape
    return (rows_walked(lens, B, S) + splits + 1) * 2.0 ** -24 * (dw_abs_ref(dy, x, k, lens) + old_abs)


def dw_fp32_chunked(dy, x, k, lens=None, chunk=32):
    """The restatement in fp32, summed in `chunk`-row pieces per utterance the way the kernels' K steps do (each piece's partial sum
    rounded to fp32, then added to an fp32 running sum): a sanity check of `dw_bar` that needs no GPU."""
    B, S, Cout = dy.shape
    Cin = x.shape[2]
    ln = clamp_lens(lens, B, S)
    dy32, xp = dy.detach().cpu().float(), torch.nn.functional.pad(x.detach().cpu().float(), (0, 0, k // 2, k // 2))
    out = torch.zeros(Cout, k, Cin)
    for b in range(B):
        for t0 in range(0, ln[b], chunk):
            t1 = min(t0 + chunk, ln[b])
            for j in range(k):
                out[:, j] += dy32[b, t0:t1].t() @ xp[b, t0 + j:t1 + j]
    return out
