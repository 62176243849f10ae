"""The residual-block oracle and the comparisons of tests/block_checks.py, on the CPU: the fp64
oracle's backward against torch autograd, the clean twin of the executor's sequencing inside
every comparison with the fp32-arithmetic allowances of every derived bound halved (the reach
of a single rounding cannot be halved), and every named defect of the twin caught at
its named case. tests/test_gpu_block_oracle.py holds the executor to the same comparisons."""
import pytest
import torch
import torch.nn.functional as F

import block_checks as K
import block_oracle as O

F64 = torch.float64


@pytest.mark.parametrize("kind,shape", K.CASES)
def test_case_conditions(kind, shape):
    """rows <= channels (the one-hot transcripts exist) and the mask margin: no recomputed
    mask can differ between fp32 and fp64, so no element is excluded anywhere."""
    assert K.onehot_ok(kind, shape)
    assert K.margins_ok(kind, shape)
    spec, N, H, W, P, Q = K.geometry(kind, shape)
    if spec.stride == 2 and shape == "3x3x3":
        assert (P, Q) == (2, 2) and H % 2 == 1      # the subgrid does not tile the input


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _torch_block(spec, x, ws, bns):
    def conv(t, i):
        Kc, R, Cc, s, p = spec.convs[i]
        return F.conv2d(t, ws[i], stride=s, padding=p)

    def bn(t, i):
        return F.batch_norm(t, None, None, bns[4 * i], bns[4 * i + 1], True, 0.1, float(torch.tensor(K.EPS).float()))

    cur = x
    for i in range(spec.nconv):
        cur = bn(conv(cur, i), i)
        if i < spec.nconv - 1:
            cur = F.relu(cur)
    sc = bn(conv(x, spec.nconv), spec.nconv) if spec.proj else x
    return F.relu(cur + sc)


@pytest.mark.parametrize("kind,shape", K.CASES)
def test_oracle_backward_matches_autograd(kind, shape):
    a = K.fwd_inputs(kind, shape)
    spec = a["spec"]
    g = torch.Generator().manual_seed(5)
    x = a["x"].clone()
    bns = [t.to(F64) for t in a["bns"]]
    fwd = O.forward(spec, x, a["ws"], bns, True, K.EPS, K.MOMENTUM)
    dout = torch.randn(fwd["out"].shape, generator=g, dtype=F64)
    bwd = O.backward(spec, x, a["ws"], bns, fwd, dout)
    xt = _nchw(x).requires_grad_(True)
    wt = [_nchw(w).requires_grad_(True) for w in a["ws"]]          # [K, R, S, C] -> [K, C, R, S]
    bt = [t.clone().requires_grad_(i % 4 < 2) for i, t in enumerate(bns)]
    out = _torch_block(spec, xt, wt, bt)
    assert torch.allclose(out, _nchw(fwd["out"]), rtol=1e-12, atol=1e-12)
    out.backward(_nchw(dout))

    def close(name, got, ref):
        err = (got - ref).abs().max().item()
        assert err <= 1e-12 * max(ref.abs().max().item(), 1.0), f"{name}: {err}"

    close("dx", _nchw(bwd["dx"]), xt.grad)
    for i in range(spec.nbn):
        close(f"dW{i}", _nchw(bwd["dw"][i]), wt[i].grad)
        close(f"dgamma{i}", bwd["dgamma"][i], bt[4 * i].grad)
        close(f"dbeta{i}", bwd["dbeta"][i], bt[4 * i + 1].grad)


def test_oracle_eval_and_running_buffers():
    """Eval normalises with the running buffers; training moves them by the momentum towards
    the batch mean and the unbiased variance."""
    a = K.fwd_inputs("basic_id", "3x3x3")
    spec = a["spec"]
    bns = [t.to(F64) for t in a["bns"]]
    tr = O.forward(spec, a["x"], a["ws"], bns, True, K.EPS, K.MOMENTUM)
    y1 = tr["y"][0].reshape(-1, spec.cout)
    m = float(torch.tensor(K.MOMENTUM).float())
    assert torch.allclose(tr["st"][0]["running_var"], (1 - m) * bns[3] + m * y1.var(0, unbiased=True), rtol=1e-12)
    assert torch.allclose(tr["st"][0]["running_mean"], (1 - m) * bns[2] + m * y1.mean(0), rtol=1e-12)
    ev = O.forward(spec, a["x"], a["ws"], bns, False, K.EPS, K.MOMENTUM)
    ref = (tr["y"][0] - bns[2]) / torch.sqrt(bns[3] + float(torch.tensor(K.EPS).float())) * bns[0] + bns[1]
    assert torch.allclose(ev["a"][0], ref.clamp_min(0), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("mode", K.FWD_MODES)
@pytest.mark.parametrize("kind,shape", K.CASES)
def test_twin_forward_at_half_bound(kind, shape, mode):
    K.check_forward(K.TwinImpl(), kind, shape, mode, scale=0.5)


@pytest.mark.parametrize("kind,shape,mode", K.BWD_CASES)
def test_twin_backward_at_half_bound(kind, shape, mode):
    K.check_backward(K.TwinImpl(), kind, shape, mode, scale=0.5)


@pytest.mark.parametrize("defect", K.DEFECTS)
def test_defect_is_caught(defect):
    direction, kind, shape, mode = K.DEFECT_CASES[defect]
    K.run_case(K.TwinImpl(), direction, kind, shape, mode)            # the clean twin passes this case
    with pytest.raises(AssertionError):
        K.run_case(K.TwinImpl([defect]), direction, kind, shape, mode)


def test_backward_case_table():
    """Every (kind, shape, mode) is either run or, for the masked store behind a strided final
    dgrad, asserted refused on the GPU."""
    plain = [c for c in K.BWD_CASES if c[2] in K.BWD_MODES]
    assert len(plain) + len(K.BWD_REFUSED) == len(K.CASES) * len(K.BWD_MODES)
    assert {k for k, s, m in K.BWD_REFUSED} == {"basic_proj_s2"}
    # every bottleneck folds: [W3], Grams (length 3, or 6 on the stride-1 projection), no y3;
    # [W3, Ws] on the stride-1 projection
    folds = {(k, m) for k, s, m in K.BWD_CASES if m in K.FOLD_MODES}
    assert folds == {(k, m) for k in ("bott_id", "bott_proj_s1", "bott_proj_s2") for m in ("fold", "fold_gram", "no_y3")} \
        | {("bott_proj_s1", "fold_sc")} | {(K.NONCAT_KIND, m) for m in ("fold", "fold_gram", "no_y3")}
    assert K.fold_spec("bott_proj_s1", "fold_gram")["n"] == 2 and K.fold_spec("bott_id", "fold_gram")["n"] == 1


def test_all_sixteen_defects():
    assert len(K.DEFECTS) == 16 and set(K.DEFECT_CASES) == set(K.DEFECTS)


@pytest.mark.parametrize("kind,shape", K.CASES)
def test_case_paths(kind, shape):
    """Each case's launches sit on the path they are meant to hit (conv_plan is host only)."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.ext()
    if m is None or not hasattr(m, "conv_plan"):
        pytest.skip("native extension not built")
    K.check_paths(m, kind, shape)


@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_noncat_fold_operand_is_reached(shape):
    """C3 = 3·K3: conv_plan refuses the K-concatenated dgrad, so fold_dgrad_operands takes the
    Wd + T form; rows <= channels still holds, so the case keeps its transcripts."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.ext()
    if m is None or not hasattr(m, "conv_plan"):
        pytest.skip("native extension not built")
    spec, N, H, W, P, Q = K.geometry(K.NONCAT_KIND, shape)
    assert K.onehot_ok(K.NONCAT_KIND, shape) and K.margins_ok(K.NONCAT_KIND, shape)
    assert not K.dgrad_cat_supported(spec.cout, spec.mid)
    g = (N, P, Q, spec.mid, spec.cout, 1, 1, 1, 0)
    assert not m.conv_plan(*g, True, full=True, kind="dgrad", bnstat=True, cat_ch=spec.mid)["ok"]
    assert m.conv_plan(*g, True, full=True, kind="dgrad", bnstat=True)["ok"]
    assert K.dgrad_cat_supported(256, 64) and m.conv_plan(N, P, Q, 64, 256, 1, 1, 1, 0, True, full=True, kind="dgrad",
                                                          bnstat=True, cat_ch=64)["ok"]
