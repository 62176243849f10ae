"""--cache_features on the native path (engine/linear.py with the row-indexed classifier steps): the
checks of tests/test_probe_cache.py on a ResNet-18 LinearEngine, for both classifier GEMMs and for
a single head and a 3-head sweep. val: every epoch's (loss, acc1, acc5) and the final result are
those of a run without the cache, exactly. all (one evaluation view, and two augmented views): the
classifier ends bit-identical to a hand loop that feeds bank[rows] to the plain ops in the sampler's
order, and the encoder runs ceil(96/40)·max(V, 1) + ceil(40/16) times in the whole run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CONFIGS = [pytest.param(g, s, id=f"{g}-{'sweep' if s else 'single'}") for g in ("fma", "mfma") for s in (False, True)]


def _native(eng, gemm, sweep):
    n = eng.native_sweep if sweep else eng.native_ce
    assert n is not None and n.gemm == gemm and eng.folded is not None
    return n


@pytest.mark.parametrize("gemm,sweep", CONFIGS)
def test_val_cache_equals_off(gpu, tmp_path, gemm, sweep):
    from test_probe_cache import check_val_equals_off
    off, val = check_val_equals_off(tmp_path, torch.device("cuda:0"), "native", sweep, gemm)
    _native(off, gemm, sweep)
    _native(val, gemm, sweep)


@pytest.mark.parametrize("views", [0, 2], ids=["V0", "V2"])
@pytest.mark.parametrize("gemm,sweep", CONFIGS)
def test_bank_training_equals_hand_loop(gpu, tmp_path, gemm, sweep, views):
    from test_probe_cache import check_all_equals_hand_loop
    eng = check_all_equals_hand_loop(tmp_path, torch.device("cuda:0"), "native", sweep, views, gemm)
    _native(eng, gemm, sweep)
    assert eng.bank.feats.is_cuda and eng.bank.feats.is_contiguous()


def test_training_reads_the_bank_in_place(gpu, tmp_path, monkeypatch):
    """The native cached step hands the whole bank view and the sampler's index tensor to the
    row-indexed op: nothing is gathered in front of it."""
    from test_probe_cache import N_TRAIN, make_engine
    from simclr_pytorch_distributed_amd.ops import linear_probe
    eng = make_engine(tmp_path, torch.device("cuda:0"), "native", "inplace", "all", 2)
    seen = []
    inner = linear_probe.NativeLinearCE.train_batch_rows

    def spy(self, bank, labels, rows, lr):
        seen.append((bank.data_ptr(), tuple(bank.shape), labels.data_ptr(), rows.dtype, rows.is_cuda))
        return inner(self, bank, labels, rows, lr)

    monkeypatch.setattr(linear_probe.NativeLinearCE, "train_batch_rows", spy)
    monkeypatch.setattr(linear_probe.NativeLinearCE, "train_batch", None)      # the gathered form is not used
    eng.train_epoch(1)
    eng.train_epoch(2)
    f, y = eng.bank.feats, eng.bank.labels
    assert len(seen) == 6
    assert seen[:3] == [(f.data_ptr(), (N_TRAIN, 512), y.data_ptr(), torch.int64, True)] * 3
    assert seen[3:] == [(f[N_TRAIN:].data_ptr(), (N_TRAIN, 512), y[N_TRAIN:].data_ptr(), torch.int64, True)] * 3


def test_refusal_reads_the_device_memory(gpu, tmp_path, monkeypatch):
    """free_memory is torch.cuda.mem_get_info's free bytes, and the refusal goes through it."""
    from test_probe_cache import N_VAL, make_engine
    from simclr_pytorch_distributed_amd.engine.linear import free_memory
    dev = torch.device("cuda:0")
    free, total = torch.cuda.mem_get_info(dev)
    got = free_memory(dev)
    assert isinstance(got, int) and 0 < got <= total and 0 < free <= total
    eng = make_engine(tmp_path, dev, "native", "oom", "val")
    need = N_VAL * (512 * 4 + 8)
    asked = []

    def tiny(device=None):
        asked.append(device)
        return need - 1, total

    monkeypatch.setattr(torch.cuda, "mem_get_info", tiny)
    with pytest.raises(RuntimeError, match=rf"need {need} bytes, the device has {need - 1} free; use --cache_features off$"):
        eng.run()
    assert asked == [dev] and eng.encoder_calls == 0 and eng.val_bank is None
