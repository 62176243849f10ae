"""The device store (data/store.py) and the trainers' common base (engine/base.py) without a GPU."""
import numpy as np
import pytest
import torch

MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)


def _configs():
    from simclr_pytorch_distributed_amd.data.augment import AugConfig
    return {"simclr": AugConfig.simclr(8, MEAN, STD), "linear_train": AugConfig.linear_train(8, MEAN, STD),
            "evaluation": AugConfig.evaluation(8, MEAN, STD), "center_crop": AugConfig.center_crop(8, MEAN, STD, 9)}


@pytest.mark.parametrize("cfg", ["simclr", "linear_train", "evaluation"])
def test_dense_store_views_are_the_augment_call(cfg):
    from simclr_pytorch_distributed_amd.data.augment import augment
    from simclr_pytorch_distributed_amd.data.datasets import ArrayDataset
    from simclr_pytorch_distributed_amd.data.store import DeviceStore
    rng = np.random.default_rng(0)
    ds = ArrayDataset(rng.integers(0, 256, (8, 8, 8, 3), dtype=np.uint8), np.arange(8) % 3, 3)
    store = DeviceStore.from_dataset(ds, torch.device("cpu"))
    assert not store.ragged and len(store) == 8 and store.num_classes == 3 and store.classes is None
    assert store.offs is None and store.hw is None and torch.equal(store.labels, torch.arange(8) % 3)
    cfg = _configs()[cfg]
    idx = torch.tensor([5, 0, 7, 5])
    want = augment(torch.from_numpy(ds.images), idx, cfg, 1234)
    got = store.views(idx, cfg, 1234)
    assert got.shape == (cfg.n_views * 4, 8, 8, 8) and torch.equal(got, want)
    assert torch.equal(store.to("cpu").views(idx, cfg, 1234), want)
    assert not torch.equal(store.views(idx, _configs()["simclr"], 1235), store.views(idx, _configs()["simclr"], 1234))


@pytest.mark.parametrize("cfg", ["simclr", "linear_train", "center_crop"])
def test_ragged_store_views_and_length(cfg):
    from simclr_pytorch_distributed_amd.data.augment import augment
    from simclr_pytorch_distributed_amd.data.datasets import ArrayDataset
    from simclr_pytorch_distributed_amd.data.store import DeviceStore
    rng = np.random.default_rng(1)
    sizes = np.asarray([(12, 9), (5, 20), (8, 8)], dtype=np.int32)      # (5, 20): shorter side below the crop
    nbytes = sizes[:, 0].astype(np.int64) * sizes[:, 1] * 3
    offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    flat = rng.integers(0, 256, int(nbytes.sum()), dtype=np.uint8)
    ds = ArrayDataset(flat, np.asarray([0, 1, 1]), 2, offsets=offsets, sizes=sizes, classes=["a", "b"])
    store = DeviceStore.from_dataset(ds, torch.device("cpu"))
    assert store.ragged and len(store) == 3 and store.images.shape[0] == int(nbytes.sum()) > 3
    assert store.classes == ["a", "b"] and store.num_classes == 2
    cfg = _configs()[cfg]
    idx = torch.tensor([1, 2, 0, 1])
    want = augment(torch.from_numpy(flat), idx, cfg, 99, torch.from_numpy(offsets), torch.from_numpy(sizes))
    got = store.views(idx, cfg, 99)
    assert got.shape == (cfg.n_views * 4, 8, 8, 8) and torch.equal(got, want)
    moved = store.to("cpu")
    assert moved.ragged and len(moved) == 3 and torch.equal(moved.views(idx, cfg, 99), want)
    with pytest.raises(ValueError, match="given together"):
        DeviceStore(store.images, store.labels, offs=store.offs)


def _ce_opt(tmp_path):
    from simclr_pytorch_distributed_amd.config import parse_ce
    return parse_ce(["--model", "resnet18", "--backend", "torch", "--dist_backend", "gloo", "--synthetic",
                     "--synthetic_size", "32", "--batch_size", "16", "--epochs", "1", "--work_dir", str(tmp_path)])


@pytest.mark.parametrize("flag,value", [("cuda_graph", True), ("micro_batch", 8)])
def test_supervised_engine_rejects_graph_and_micro_batch(tmp_path, flag, value):
    from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
    opt = _ce_opt(tmp_path)
    setattr(opt, flag, value)
    with pytest.raises(ValueError, match="supports neither --cuda_graph nor --micro_batch"):
        SupervisedEngine(opt, device=torch.device("cpu"))


def test_supervised_engine_is_built_by_the_base(tmp_path):
    from simclr_pytorch_distributed_amd.engine.base import TrainEngine
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
    eng = SupervisedEngine(_ce_opt(tmp_path), device=torch.device("cpu"))
    assert isinstance(eng, TrainEngine) and not isinstance(eng, PretrainEngine)
    # what only pretraining can do is not callable on the supervised trainer
    for name in ("enable_cuda_graph", "_step_body_gradcache", "knn_eval", "_build_knn", "_norm_terms"):
        assert hasattr(PretrainEngine, name) and not hasattr(eng, name), name
    # state that only TrainEngine.__init__ assigns
    own = vars(eng)
    assert own["syncbn_tune"] is None and own["_syncbn_cands"] == {} and own["syncbn_transport"] == "none"
    assert own["_one_grad"] is None and own["_zg_ev"] is None and own["_cpu_store"] is None
    assert own["_syncbn_pending"] is False and eng.reducer is None and eng.optimizer.grad_scale == 1.0
    assert own["start_epoch"] == 1 and own["global_step"] == 0 and eng.history == []
    # the classes keep no mutable state of their own
    for cls in (TrainEngine, PretrainEngine, SupervisedEngine):
        assert not {"_syncbn_cands", "_syncbn_pending", "syncbn_tune", "syncbn_transport"} & set(vars(cls))
    assert len(eng.train) == 32 and len(eng.val) == 1000 and eng.model.fc.out_features == eng.opt.n_cls == 10
    idx, labels = next(eng.epoch_batches(1))
    st = eng.train_step(idx, labels, 1, 0, 2)
    assert eng.global_step == 1 and torch.isfinite(st["loss_local"]) and own["_one_grad"] is not None
