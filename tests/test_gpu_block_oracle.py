"""The native residual-block executor (block_fwd / block_bwd, csrc/bindings/block_ops.cpp)
against the stage-wise fp64 oracle of tests/block_oracle.py, within the derived bounds of
tests/block_checks.py (GPU). Tiny shapes only; the environment knobs are read once per process,
so only the defaults run here (SDX_DGRAD_BNSTAT=0, SDX_FOLD_CAT=0, SDX_SUB_ADDEND=0 and SyncBN
are out of scope; tests/test_gpu_comm.py covers the last). tests/test_block_oracle.py shows on
the CPU that the comparisons catch each named sequencing defect."""
import pytest
import torch

import block_checks as K

pytestmark = pytest.mark.gpu


@pytest.fixture
def impl(gpu):
    from simclr_pytorch_distributed_amd.ops import _ext
    return K.ExtImpl(_ext.require(), gpu)


def _report(stats):
    for k in sorted(stats):
        print(f"{k}: largest error / bound = {stats[k]:.4f}")
    print(f"worst error / bound = {max(stats.values()):.4f}")


@pytest.mark.parametrize("mode", K.FWD_MODES)
@pytest.mark.parametrize("kind,shape", K.CASES)
def test_block_fwd(impl, kind, shape, mode):
    """Every returned slot against one oracle stage fed the returned slots: conv stores,
    statistics and running buffers (count stated per BN), activations, out, the bitmask."""
    stats = {}
    K.check_forward(impl, kind, shape, mode, stats)
    _report(stats)


@pytest.mark.parametrize("kind,shape,mode", K.BWD_CASES)
def test_block_bwd(impl, kind, shape, mode):
    """Stage by stage along the weight-gradient transcripts: every dγ, dβ and dW sink, every
    stored gradient of the chain, dx, the statistics slab for the previous block; inputs
    bitwise unchanged."""
    stats = {}
    K.check_backward(impl, kind, shape, mode, stats)
    _report(stats)


@pytest.mark.parametrize("kind,shape,mode", K.BWD_REFUSED)
def test_masked_store_behind_a_strided_dgrad_is_refused(impl, kind, shape, mode):
    """A fold marker in ``prev`` of a block whose final dgrad is strided: conv_dgrad_bnstat
    raises at the final dgrad (the earlier launches of the block have run by then, so the sinks
    are partly updated) instead of storing dx unmasked. No caller asks for this (a strided
    BasicBlock follows a block that never folds); the case table names these combinations so
    that none of (kind, shape, mode) is silently absent."""
    with pytest.raises(RuntimeError, match="store_masked"):
        impl.bwd(K.bwd_args(kind, shape, mode))


@pytest.mark.parametrize("kind,shape", [("bott_proj_s2", "3x3x3"), ("basic_id", "2x4x4")])
def test_side_stream_is_bit_identical(gpu, kind, shape):
    """The weight gradients on a side stream (side != 0) give the same bits as side = 0."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    a = K.bwd_args(kind, shape, "prev2")
    ref = K.ExtImpl(m, gpu).bwd(a)
    stream = torch.cuda.Stream(device=gpu)
    got = K.ExtImpl(m, gpu, side=stream.cuda_stream).bwd(a)
    K.BC.same_bits("dx", got["dx"], ref["dx"])
    K.BC.same_bits("prev_slab", got["prev_slab"], ref["prev_slab"])
    for k in ("dw", "dg", "db"):
        for i, (g, r) in enumerate(zip(got[k], ref[k])):
            K.BC.same_bits(f"{k}[{i}]", g, r)


# ---- the wiring of _NativeBlock (ops/block.py) -------------------------------------------------
# BlockSlot layout of block_fwd's result, from the comments above block_fwd / block_bwd in
# csrc/bindings/block_ops.cpp: [out, y1, a1, y2, a2, y3, ys, mask], then sc, sh, mu, iv per BN in
# the order bn1, bn2, bn3, (shortcut bn).
_OUT, _Y3, _YS, _MASK, _SLOTS, _MU = 0, 5, 6, 7, 8, 2


def _chain_blocks(gpu):
    from simclr_pytorch_distributed_amd.models.resnet import Bottleneck
    torch.manual_seed(3)
    blocks = [Bottleneck(64, 64, 1), Bottleneck(256, 64, 1), Bottleneck(256, 64, 1)]     # projection, identity x 2
    for b in blocks:
        b.to(gpu).to(memory_format=torch.channels_last).train()
        for bn in (m for m in b.modules() if isinstance(m, torch.nn.BatchNorm2d)):
            with torch.no_grad():
                bn.weight.uniform_(0.5, 1.5)
                bn.bias.normal_()
                bn.running_mean.normal_()
                bn.running_var.uniform_(0.5, 1.5)
    return blocks


def _convs_bns(b):
    proj = len(b.shortcut) > 0
    return ([b.conv1, b.conv2, b.conv3] + ([b.shortcut[0]] if proj else []),
            [b.bn1, b.bn2, b.bn3] + ([b.shortcut[1]] if proj else []), proj)


def test_native_block_wiring_is_bit_identical_to_direct_calls(gpu, monkeypatch):
    """Three tiny bottlenecks (projection, identity, identity; every fold on) through the public
    autograd path (ops/block.py ``bottleneck`` with a BlockChain; wgrads on the side stream)
    against the same chain driven by direct block_fwd / block_bwd calls on the current stream,
    whose prev, in_slab and fold_w this test assembles from the layout documented above
    block_fwd / block_bwd: outputs, running buffers, dx and every sink bit-identical."""
    from simclr_pytorch_distributed_amd.ops import _ext, block as fb, streams
    from simclr_pytorch_distributed_amd.ops.weights import ConvWeightCache
    m = _ext.require()
    monkeypatch.setattr(fb, "BN3_FOLD_ROWS_PER_K2", 0.0)        # the folds' size rule would refuse 32 rows
    assert fb.NATIVE_EXEC and fb.BN3_FOLD and fb.FOLD_FWD and fb.DGRAD_BNSTAT and not fb.FOLD_GRAM_FWD
    blocks = _chain_blocks(gpu)
    infos = [_convs_bns(b) for b in blocks]
    wc = ConvWeightCache([cv for convs, _, _ in infos for cv in convs], None)
    wc.refresh()
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(2, 4, 4, 64, generator=g).to(torch.bfloat16).to(gpu)
    dout = torch.randn(2, 4, 4, 256, generator=g).to(torch.bfloat16).to(gpu)
    running0 = [[(bn.running_mean.clone(), bn.running_var.clone()) for bn in bns] for _, bns, _ in infos]

    # ---- the public path
    x = x0.clone().requires_grad_(True)
    chain = fb.BlockChain()
    out = x
    outs = []
    for i, b in enumerate(blocks):
        out = fb.bottleneck(out, b, wc, True, None, chain, next_native=i + 1 < len(blocks))
        outs.append(out.detach().clone())
        # the folds are really on in the public path: fold marker published, y3 not kept where a
        # native successor follows
        assert len(chain.last.prev) == 6 and (chain.last.prev[0].numel() == 0) == (i + 1 < len(blocks))
    out.backward(dout)
    streams.join(gpu)
    torch.cuda.synchronize()
    pub_dx = x.grad.clone()
    pub_grads = [[p.grad.clone() for p in list(cv.weight for cv in convs) + [q for bn in bns for q in (bn.weight, bn.bias)]]
                 for convs, bns, _ in infos]
    pub_running = [[(bn.running_mean.clone(), bn.running_var.clone()) for bn in bns] for _, bns, _ in infos]

    # ---- the same chain by direct calls
    e = torch.empty(0, dtype=torch.bfloat16, device=gpu)
    ef = torch.empty(0, dtype=torch.float32, device=gpu)
    marker = torch.ones(1, dtype=torch.uint8, device=gpu)
    fwd, cur = [], x0
    for i, (b, (convs, bns, proj)) in enumerate(zip(blocks, infos)):
        bn_list = []
        for bn, (rm, rv) in zip(bns, running0[i]):
            bn_list += [bn.weight.detach(), bn.bias.detach(), rm, rv]
        fold_fwd = i + 1 < len(blocks)           # the successor's final dgrad supplies the slab
        r = m.block_fwd(cur, [wc.fwd(cv) for cv in convs], bn_list, 1, True, proj, True, bns[0].eps, bns[0].momentum,
                        0, fold_fwd, 0)
        assert (r[_Y3] is None or r[_Y3].numel() == 0) == fold_fwd
        fwd.append((cur, r))
        cur = r[_OUT]
        assert torch.equal(outs[i].view(torch.int16), cur.view(torch.int16)), f"block {i}: out differs"
        for k, (rm, rv) in enumerate(running0[i]):
            assert torch.equal(rm, pub_running[i][k][0]) and torch.equal(rv, pub_running[i][k][1]), \
                f"block {i} bn {k}: running buffers differ"
    d, in_slab = dout, None
    for i in range(len(blocks) - 1, -1, -1):
        convs, bns, proj = infos[i]
        xin, r = fwd[i]
        nbn = len(bns)
        saved = [xin] + [t if t is not None else e for t in r[1:_MASK]] + [r[_MASK]]
        bnst = list(r[_SLOTS:_SLOTS + 4 * nbn])
        dw = [torch.zeros_like(cv.weight, memory_format=torch.preserve_format) for cv in convs]
        dgb = [(torch.zeros_like(bn.weight), torch.zeros_like(bn.bias)) for bn in bns]
        bng = [t for bn, (dg_, db_) in zip(bns, dgb) for t in (bn.weight.detach(), dg_, db_)]
        prev = []
        if i > 0:
            pconvs, pbns, pproj = infos[i - 1]
            pr = fwd[i - 1][1]
            y3 = pr[_Y3] if pr[_Y3] is not None else e                       # forward-folded: never stored
            prev = [y3, pr[_SLOTS + 4 * 2 + _MU], pr[_YS] if pproj else e, pr[_SLOTS + 4 * 3 + _MU] if pproj else ef,
                    pr[_MASK], marker]                                        # the previous block folds its BN3
        # this block folds when a slab arrives: conv3, and the stride-1 shortcut of the projection
        fold_w = [wc.fwd(convs[2])] + ([wc.fwd(convs[3])] if proj else [])
        dx, pslab = m.block_bwd(d.contiguous(), saved, bnst, [wc.dgrad(cv) for cv in convs], dw, bng, 1, True, proj, 0,
                                0, in_slab, prev, fold_w)
        torch.cuda.synchronize()
        assert (pslab is not None and pslab.numel() > 0) == (i > 0)
        got = dw + [t for pair in dgb for t in pair]
        for k, (a, b_) in enumerate(zip(got, pub_grads[i])):
            assert a.shape == b_.shape and torch.equal(a.view(torch.int32), b_.view(torch.int32)), \
                f"block {i}: sink {k} differs from the public path"
        d, in_slab = dx, pslab
    assert torch.equal(d.view(torch.int16), pub_dx.view(torch.int16)), "dx differs from the public path"
