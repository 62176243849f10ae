"""The row-indexed classifier steps (linear_ce_step_rows, linear_ce_sweep_step_rows and their _mfma
forms; csrc/kernels/linear_ce.hip, linear_ce_sweep.hip, head_gemm.hip): a step that reads its batch
from a feature bank x [N][K], labels [N] through rows [B] is BIT-identical to the plain op on
x[rows].contiguous(), labels[rows] — logits, statistics, weights and momentum buffers, over chained
training steps and an evaluation call. Through that identity the row-indexed ops inherit the
oracle coverage of the plain ones (tests/test_gpu_aux_oracle.py, tests/test_headgemm_oracle.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MOM = 0.9
BS = [1, 63, 65, 130]                       # one row, under / over one 64-row tile, more than two tiles
SHAPES = {"fma": [(64, 10), (512, 100), (64, 100), (512, 10)],
          "mfma": [(64, 10), (192, 65), (64, 65), (192, 10)]}      # (K, C); K = 192: no power of two; C = 65: a tile + 1
HEADS = [None, 1, 3, 16]                    # None: the single-head op


def _op(m, gemm, heads, rows):
    name = "linear_ce_step" if heads is None else "linear_ce_sweep_step"
    return getattr(m, name + ("_mfma" if gemm == "mfma" else "") + ("_rows" if rows else ""))


def _state(heads, K, C, gpu, seed):
    g = torch.Generator().manual_seed(seed)
    lead = () if heads is None else (heads,)
    W = (torch.randn(*lead, C, K, generator=g) * 0.05).to(gpu)
    b = (torch.randn(*lead, C, generator=g) * 0.1).to(gpu)
    return [W, b, torch.zeros_like(W), torch.zeros_like(b)]


def _bank(N, K, C, gpu, seed, offset=None):
    """(x [N][K], labels [N]); offset: a view that starts ``offset`` floats into a larger tensor."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, K, generator=g).relu()
    y = torch.randint(0, C, (N,), generator=g).to(gpu)
    if offset is None:
        return x.to(gpu), y
    big = torch.full((N * K + offset + 8,), 7.0, device=gpu)
    view = big[offset:offset + N * K].view(N, K)
    view.copy_(x)
    return view, y


def _rows(B, N, gpu, seed):
    """Identity when the bank is the batch; else unsorted, with the first and the last bank row and a duplicate."""
    if N == B:
        return torch.arange(B, device=gpu)
    g = torch.Generator().manual_seed(seed)
    r = torch.randint(0, N, (B,), generator=g)
    if B >= 3:
        r[0], r[1], r[2] = N - 1, 0, N - 1
    return r.to(gpu)


def _hyper(heads, step):
    n = 1 if heads is None else heads
    f = [1.0, 0.5, 0.1][step]
    lrs = [f * 0.01 * (5.0 / 0.01) ** ((i + 1) / n) for i in range(n)]          # per head, 0.01 < lr <= 5
    wds = [1e-3 if i % 2 == 0 else 0.0 for i in range(n)]
    return (lrs[0], wds[0]) if heads is None else (lrs, wds)


def _check_identity(m, gemm, heads, x, y, B, C, gpu, seed, steps=3):
    N, K = x.shape
    got, ref = _state(heads, K, C, gpu, seed), _state(heads, K, C, gpu, seed)
    plain, indexed = _op(m, gemm, heads, False), _op(m, gemm, heads, True)

    def compare(a, r, what):
        for name, t, u in zip(("logits", "stats"), a, r):
            assert t.shape == u.shape and torch.equal(t, u), (what, name)
        for name, t, u in zip(("W", "b", "bufW", "bufb"), got, ref):
            assert torch.equal(t, u), (what, name)

    for step in range(steps):
        rows = _rows(B, N, gpu, seed + step)
        lr, wd = _hyper(heads, step)
        a = indexed(x, got[0], got[1], y, rows, got[2], got[3], lr, MOM, wd, step == 0, True)
        r = plain(x[rows].contiguous(), ref[0], ref[1], y[rows], ref[2], ref[3], lr, MOM, wd, step == 0, True)
        torch.cuda.synchronize()
        assert torch.isfinite(a[0]).all() and torch.isfinite(got[0]).all()
        compare(a, r, f"step {step}")
    rows = _rows(B, N, gpu, seed + 50)
    keep = [t.clone() for t in got]
    zero = 0.0 if heads is None else [0.0] * heads
    a = indexed(x, got[0], got[1], y, rows, None, None, zero, 0.0, zero, False, False)
    r = plain(x[rows].contiguous(), ref[0], ref[1], y[rows], None, None, zero, 0.0, zero, False, False)
    torch.cuda.synchronize()
    compare(a, r, "eval")
    for t, k in zip(got, keep):
        assert torch.equal(t, k)                                    # an evaluation call writes no parameter
    assert not torch.equal(got[0], _state(heads, K, C, gpu, seed)[0])


def _cases():
    out = []
    for gemm in ("fma", "mfma"):
        for hi, heads in enumerate(HEADS):
            for bi, B in enumerate(BS):
                K, C = SHAPES[gemm][(bi + hi) % 4]
                N = B if (bi + hi) % 2 == 0 else 1000
                out.append(pytest.param(gemm, heads, B, K, C, N, id=f"{gemm}-G{heads}-B{B}-K{K}-C{C}-N{N}"))
    return out


@pytest.mark.parametrize("gemm,heads,B,K,C,N", _cases())
def test_rows_step_bit_identical_to_gathered_batch(gpu, gemm, heads, B, K, C, N):
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    x, y = _bank(N, K, C, gpu, 7 * B + K)
    _check_identity(m, gemm, heads, x, y, B, C, gpu, 11 * B + C + (heads or 0))


@pytest.mark.parametrize("offset", [4, 1, 3], ids=["16B-aligned-slice", "4B-off", "12B-off"])
@pytest.mark.parametrize("heads", [None, 3], ids=["single", "G3"])
@pytest.mark.parametrize("gemm", ["fma", "mfma"])
def test_bank_as_an_offset_slice(gpu, gemm, heads, offset):
    """A bank that starts inside a larger tensor; 1 or 3 floats in, its rows are not 16-byte aligned
    and the kernels take their 4-byte loads (the plain op sees an aligned copy either way)."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    N, B, K, C = 1000, 65, 64, 10
    x, y = _bank(N, K, C, gpu, 91, offset)
    assert x.is_contiguous() and x.data_ptr() % 16 == (4 * offset) % 16
    _check_identity(m, gemm, heads, x, y, B, C, gpu, 13 + offset, steps=2)


@pytest.mark.parametrize("heads", [None, 3], ids=["single", "G3"])
@pytest.mark.parametrize("gemm", ["fma", "mfma"])
def test_label_out_of_range_in_the_bank(gpu, gemm, heads):
    """A bank label outside [0, C): NaN loss and no hits for that row, as the plain op reports."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    N, B, K, C = 100, 9, 64, 10
    x, y = _bank(N, K, C, gpu, 5)
    rows = _rows(B, N, gpu, 6)
    y[rows[3]] = C
    y[rows[4]] = -1
    W, b, _, _ = _state(heads, K, C, gpu, 3)
    zero = 0.0 if heads is None else [0.0] * heads
    a = _op(m, gemm, heads, True)(x, W, b, y, rows, None, None, zero, 0.0, zero, False, False)
    r = _op(m, gemm, heads, False)(x[rows].contiguous(), W, b, y[rows], None, None, zero, 0.0, zero, False, False)
    torch.cuda.synchronize()
    assert torch.equal(a[0], r[0])
    sa, sr = a[1].reshape(-1, 3), r[1].reshape(-1, 3)
    assert torch.isnan(sa[:, 0]).all() and torch.isnan(sr[:, 0]).all()
    assert torch.equal(sa[:, 1:], sr[:, 1:]) and (sa[:, 1:] <= B - 2).all()


@pytest.mark.parametrize("heads", [None, 2], ids=["single", "G2"])
@pytest.mark.parametrize("gemm", ["fma", "mfma"])
def test_refusals(gpu, gemm, heads):
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    N, B, K, C = 50, 4, 64, 5
    x, y = _bank(N, K, C, gpu, 1)
    rows = _rows(B, N, gpu, 2)
    st = [torch.full_like(t, 7.0) for t in _state(heads, K, C, gpu, 3)]
    op = _op(m, gemm, heads, True)
    lr, wd = _hyper(heads, 0)

    def refused(xx, yy, rr, exc=RuntimeError):
        with pytest.raises(exc):
            op(xx, st[0], st[1], yy, rr, st[2], st[3], lr, MOM, wd, True, True)

    refused(x, y, rows.int())                                       # rows: int64 only (no cast launch)
    refused(x, y, rows.cpu())                                       # rows live on the bank's device
    refused(x, y, rows.view(2, 2))                                  # rows [B]
    refused(x, y, torch.arange(0, 2 * B, device=gpu)[::2])          # contiguous rows
    refused(x, y[:N - 1], rows)                                     # one label per bank row
    refused(x, y.int(), rows)
    refused(x, y.cpu(), rows)
    refused(x.double(), y, rows)
    refused(x.cpu(), y.cpu(), rows.cpu())
    refused(torch.full((N, 2 * K), 1.0, device=gpu)[:, :K], y, rows)    # a bank with a row stride
    refused(x[:, :K - 1].contiguous(), y, rows)                     # K of the bank != K of W
    refused(x, y, rows[:0])                                         # an empty batch
    refused(x, y, None, TypeError)
    torch.cuda.synchronize()
    for t in st:
        assert (t == 7.0).all()
