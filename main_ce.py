"""Supervised cross-entropy training and fine-tuning entry point, and the supervised data
loaders (reference main_ce.py:19-68 keeps only ``set_loader``).

Baseline:     python main_ce.py --dataset cifar10 --model resnet50 --epochs 500 --cosine
Fine-tuning:  python main_ce.py --ckpt path/to/last.pth --label_frac 0.1 --learning_rate 0.05 --epochs 100
Distillation: python main_ce.py --distill_ckpt path/to/finetuned/last.pth --distill_model resnet50 --model resnet18 \
                  --distill_temp 1.0 --distill_alpha 1.0 --label_frac 0.1
Multi GPU:    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 main_ce.py --syncBN ...

``set_loader(opt)`` returns (train, val) in-memory datasets plus the GPU augmentation
configs used by the linear probe: RandomResizedCrop(32, scale=(0.2,1)) + flip +
normalize for training, normalize only for validation.
"""
from simclr_pytorch_distributed_amd.config import DATASET_STATS
from simclr_pytorch_distributed_amd.data.augment import AugConfig
from simclr_pytorch_distributed_amd.data.datasets import build_dataset


def set_loader(opt):
    if opt.dataset not in DATASET_STATS:
        raise ValueError("dataset not supported: {}".format(opt.dataset))
    mean, std = DATASET_STATS[opt.dataset]
    synthetic = getattr(opt, "synthetic", False)
    train = build_dataset(opt.dataset, opt.data_folder, True, synthetic)
    val = build_dataset(opt.dataset, opt.data_folder, False, synthetic)
    return (train, AugConfig.linear_train(32, mean, std)), (val, AugConfig.evaluation(32, mean, std))


def main(argv=None):
    from simclr_pytorch_distributed_amd.config import parse_ce
    from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
    opt = parse_ce(argv)
    return SupervisedEngine(opt).run()


if __name__ == "__main__":
    from simclr_pytorch_distributed_amd.utils.faults import guarded_main
    guarded_main(main)
