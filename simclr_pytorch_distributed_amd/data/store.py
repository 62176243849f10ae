"""A dataset as it is resident on a device: uint8 images + labels, and for an ImageFolder kept at
native resolution (data/datasets.py load_image_folder) the byte offsets and sizes of its ragged
store. The engines index it with a batch of image numbers and get augmented views back."""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Optional

import torch

from .augment import AugConfig, augment, default_resize, gpu_augment
from .datasets import build_dataset


@dataclass
class DeviceStore:
    images: torch.Tensor                    # uint8 [N, H, W, 3], or the flat bytes of a ragged store
    labels: torch.Tensor                    # int64 [N]
    offs: Optional[torch.Tensor] = None     # ragged: int64 [N] byte offsets, int32 [N, 2] (h, w)
    hw: Optional[torch.Tensor] = None
    classes: Optional[list] = None          # ImageFolder: the class directory names
    num_classes: int = 0

    def __post_init__(self):
        if (self.offs is None) != (self.hw is None):
            raise ValueError("offs and hw of a ragged store must be given together")

    @classmethod
    def from_dataset(cls, ds, device) -> "DeviceStore":
        def up(a):
            return torch.from_numpy(a).to(device)
        return cls(up(ds.images), up(ds.labels), up(ds.offsets) if ds.ragged else None,
                   up(ds.sizes) if ds.ragged else None, ds.classes, ds.num_classes)

    @property
    def ragged(self) -> bool:
        return self.offs is not None

    def __len__(self) -> int:
        """Images in the store: by index, not by the (flat, when ragged) tensor's first dimension."""
        return int((self.offs if self.ragged else self.images).shape[0])

    def to(self, device) -> "DeviceStore":
        def mv(t):
            return None if t is None else t.to(device)
        return replace(self, images=mv(self.images), labels=mv(self.labels), offs=mv(self.offs), hw=mv(self.hw))

    def views(self, idx: torch.Tensor, cfg: AugConfig, seed: int) -> torch.Tensor:
        """Augmented views (NHWC, C=8) of images ``idx``: the kernel on a GPU store, the torch twin otherwise."""
        return augment(self.images, idx, cfg, seed, self.offs, self.hw)

    def views_gpu(self, idx: torch.Tensor, cfg: AugConfig, seed: int, seed_t=None) -> torch.Tensor:
        """The kernel itself; ``seed_t``: the device-side seed a captured step reads at replay."""
        return gpu_augment(self.images, idx, cfg, seed, seed_t, self.offs, self.hw)


def probe_stores(opt, device, train: Optional[DeviceStore] = None, n_cls_from_labels: bool = False):
    """(train store, validation store, Resize target, evaluation AugConfig, class count) of a run
    that evaluates on the validation split. A real ImageFolder: native-resolution ragged training
    store (RandomResizedCrop on the original pixels), ``--val_folder`` capped at the Resize target,
    Resize + CenterCrop on the GPU; CIFAR and ``--synthetic``: dense stores, normalize only.
    ``train``: the training store the caller already holds (used as it is, no second copy).
    ``n_cls_from_labels``: without ``--n_cls``, dense stores count their classes as largest
    label + 1 instead of the dataset's nominal class count."""
    size, nw = getattr(opt, "size", 32), getattr(opt, "num_workers", 1)
    folder = (opt.dataset == "path" and not opt.synthetic) if train is None else train.ragged
    resize = (getattr(opt, "resize", 0) or default_resize(size)) if folder else 0
    if train is None:
        train = DeviceStore.from_dataset(
            build_dataset(opt.dataset, opt.data_folder, True, opt.synthetic, opt.synthetic_size, size, opt.seed,
                          native=folder, workers=nw), device)
    val = DeviceStore.from_dataset(
        build_dataset(opt.dataset, opt.val_folder if folder else opt.data_folder, False, opt.synthetic,
                      opt.synthetic_size, size, opt.seed, workers=nw, eval_resize=resize), device)
    if folder and train.classes != val.classes:
        raise ValueError("--val_folder has other classes than --data_folder")
    if n_cls_from_labels and not folder:
        n_cls = opt.n_cls or int(max(int(train.labels.max()), int(val.labels.max()))) + 1
    else:
        n_cls = opt.n_cls or max(train.num_classes, val.num_classes)
    aug_val = (AugConfig.center_crop(size, opt.mean_t, opt.std_t, resize) if folder
               else AugConfig.evaluation(size, opt.mean_t, opt.std_t))
    return train, val, resize, aug_val, n_cls
