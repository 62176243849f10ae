"""Command-line configuration with flag/default/derived-field parity to the reference.

* :func:`pretrain_parser` / :func:`parse_pretrain` mirror main_supcon.py:22-152
  (30 flags, ``model_name`` derivation, warm-up auto-enable for ``batch_size > 256``,
  ``./work_space/{dataset}_{models,tensorboard}/{dataset}_{MMDD_HHMM}_{model_name}``).
* :func:`linear_parser` / :func:`parse_linear` mirror main_linear.py:21-116.
* :func:`ce_parser` / :func:`parse_ce`: supervised cross-entropy training and fine-tuning
  (main_ce.py; the reference keeps only its loaders), with ``--ckpt``, ``--label_frac``,
  ``--val_freq`` and ``--n_cls``.

Additions (new flags only; no reference flag changes meaning):
``--local-rank`` (dashed alias), env rank discovery (Q13),
``--precision``, ``--backend``, ``--synthetic``, ``--stem``, ``--optimizer {sgd,lars}``,
``--grad_semantics {ref,exact}`` (Q2), ``--dist_backend``, ``--seed``, ``--head``,
``--feat_dim`` (Q11), ``--resume``, ``--cuda_graph``, ``--work_dir``,
``--knn_freq`` / ``--knn`` with ``--knn_k`` / ``--knn_t`` (weighted k-NN monitor, engine/knn.py),
``--blur_p`` / ``--blur_kernel`` / ``--blur_sigma`` (Gaussian-blur augmentation, data/augment.py),
``--val_folder`` / ``--resize`` (ImageFolder evaluation: Resize + CenterCrop on the GPU; the linear
probe also takes ``--dataset path`` with ``--size`` / ``--mean`` / ``--std``),
``--sweep_lr`` / ``--sweep_wd`` (linear probe: one classifier per (lr, wd) pair on one encoder pass),
``--cache_features`` / ``--cache_views`` (linear probe: encode the frozen encoder's features once),
``--label_smoothing`` / ``--mixup`` / ``--cutmix`` / ``--mix_prob`` / ``--mix_switch_prob`` (supervised
trainer: soft-target regularisers, data/augment.py ``mix_draw``),
``--distill_ckpt`` / ``--distill_model`` / ``--distill_temp`` / ``--distill_alpha`` (supervised trainer:
knowledge distillation from a frozen ``main_ce.py`` checkpoint, the SimCLRv2 stage 3).
Fixes: ``--num_workers`` is honoured (Q6): it sizes the image-decode thread pool of
``dataset=path`` and the CPU augmentation threads of ``--gpu_aug 0`` (the default pipeline
is the GPU kernel, which needs no workers); ``dataset=path`` parses ``--mean/--std``
safely and uses the std (Q5); run folders get a collision guard (Q21).
"""
from __future__ import annotations

import argparse
import ast
import datetime
import math
import os
from typing import List, Optional, Sequence

DATASET_STATS = {
    # main_supcon.py:157-162 / main_ce.py:21-26
    "cifar10": ((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)),
    "cifar100": ((0.5071, 0.4867, 0.4408), (0.2675, 0.2565, 0.2761)),
}
N_CLASSES = {"cifar10": 10, "cifar100": 100}


def parse_tuple(s: Optional[str]):
    """Parse ``"(0.5, 0.5, 0.5)"`` without ``eval`` (reference uses eval, main_supcon.py:164)."""
    if s is None:
        return None
    v = ast.literal_eval(s)
    if isinstance(v, (int, float)):
        return (float(v),)
    return tuple(float(x) for x in v)


def env_rank_info(cli_local_rank: Optional[int] = None):
    """Return (rank, local_rank, world_size) from torchrun env vars, falling back to the CLI."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = os.environ.get("LOCAL_RANK")
    local_rank = int(local) if local is not None else (cli_local_rank or 0)
    if "RANK" not in os.environ and cli_local_rank:
        rank = cli_local_rank
    return rank, local_rank, world


def _add_common_new_flags(p: argparse.ArgumentParser):
    g = p.add_argument_group("MI355X framework options (new)")
    g.add_argument("--backend", type=str, default="auto", choices=["auto", "native", "torch"],
                   help="compute path: native gfx950 kernels, stock torch ops, or auto")
    g.add_argument("--precision", type=str, default="bf16", choices=["bf16", "fp32"],
                   help="activation/compute dtype on GPU (fp32 master weights always)")
    g.add_argument("--synthetic", action="store_true", help="use synthetic data (no dataset files)")
    g.add_argument("--synthetic_size", type=int, default=50000)
    g.add_argument("--seed", type=int, default=0)
    g.add_argument("--stem", type=str, default="cifar", choices=["cifar", "imagenet"])
    g.add_argument("--head", type=str, default="mlp", choices=["mlp", "linear"])
    g.add_argument("--feat_dim", type=int, default=128)
    g.add_argument("--work_dir", type=str, default="./work_space")
    g.add_argument("--dist_backend", type=str, default="auto", choices=["auto", "nccl", "gloo"])
    g.add_argument("--cuda_graph", action="store_true", help="capture the train step in a HIP graph")
    g.add_argument("--max_steps", type=int, default=0, help="stop each epoch after this many steps (0 = all)")
    g.add_argument("--gpu_aug", type=int, default=1,
                   help="augmentation on the GPU kernel (1) or the CPU torch pipeline on --num_workers threads (0)")
    # default rccl: the fused xGMI exchange has only ever run as same-device IPC
    # rehearsals (several processes on one GPU, emulated ranks); its peer stores and flag
    # protocol have not yet executed across real xGMI links, so it is opt-in until they have
    g.add_argument("--syncbn_comm", type=str, default="rccl", choices=["auto", "rccl", "xgmi"],
                   help="SyncBN statistics exchange: rccl (default: a dedicated RCCL communicator, "
                        "reduce -> ncclAllReduce -> finalize per BN), xgmi (the fused one-shot xGMI exchange, "
                        "every rank on one node; RCCL is the fallback when the arena's self-check fails), "
                        "auto (set up both and keep the one measured fastest on the first batch, agreed by "
                        "all ranks). xgmi/auto are EXPERIMENTAL: the fused exchange has been validated on "
                        "one GPU (multi-process IPC rehearsals, emulated ranks) but not yet across real "
                        "peer GPUs")
    g.add_argument("--comm_timeout", type=float, default=600.0,
                   help="collective timeout in seconds (a dead/stalled peer raises instead of hanging)")
    g.add_argument("--profile", action="store_true",
                   help="per-phase HIP-event timings in the log + ROCTX ranges for rocprofv3 --marker-trace")


def _add_eval_flags(g):
    g.add_argument("--val_folder", type=str, default=None,
                   help="ImageFolder of the validation split of --dataset path (same class sub-directories "
                        "as --data_folder)")
    g.add_argument("--resize", type=int, default=0,
                   help="evaluation Resize target of the shorter side before CenterCrop(--size) "
                        "(0 = size / 0.875 rounded: 256 for 224)")


def list_classes(root: str) -> List[str]:
    """Sorted class sub-directory names of an ImageFolder."""
    return sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))


def _check_val_folder(opt):
    """--val_folder and --resize of a ``path`` dataset; the two folders must hold the same classes."""
    if opt.resize < 0 or (opt.resize and opt.resize < opt.size) or opt.resize > 32768:
        raise ValueError(f"--resize {opt.resize} must be 0 (automatic) or in [--size, 32768]")
    if opt.val_folder is None or opt.synthetic:
        return
    for f in (opt.data_folder, opt.val_folder):
        if not os.path.isdir(f):
            raise ValueError(f"{f!r} is not a directory")
    tr, va = list_classes(opt.data_folder), list_classes(opt.val_folder)
    if tr != va:
        diff = sorted(set(tr) ^ set(va))
        raise ValueError(f"--val_folder has other classes than --data_folder ({len(va)} vs {len(tr)}; "
                         f"differing: {diff[:5]}{' ...' if len(diff) > 5 else ''})")


def _add_knn_flags(g):
    g.add_argument("--knn_k", type=int, default=200, help="neighbours of the weighted k-NN evaluation")
    g.add_argument("--knn_t", type=float, default=0.1, help="temperature of the k-NN vote exp(sim/T)")


def pretrain_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser("argument for training")
    # main_supcon.py:26-34
    p.add_argument("--print_freq", type=int, default=10, help="print frequency")
    p.add_argument("--save_freq", type=int, default=20, help="save frequency")
    p.add_argument("--batch_size", type=int, default=256, help="batch_size (global)")
    p.add_argument("--num_workers", type=int, default=16, help="num of workers to use")
    p.add_argument("--epochs", type=int, default=1000, help="number of training epochs")
    # optimization (main_supcon.py:37-46)
    p.add_argument("--learning_rate", type=float, default=0.5, help="learning rate")
    p.add_argument("--lr_decay_epochs", type=str, default="700,800,900", help="where to decay lr")
    p.add_argument("--lr_decay_rate", type=float, default=0.1, help="decay rate for learning rate")
    p.add_argument("--weight_decay", type=float, default=1e-4, help="weight decay")
    p.add_argument("--momentum", type=float, default=0.9, help="momentum")
    # model dataset (main_supcon.py:49-56)
    p.add_argument("--model", type=str, default="resnet50")
    p.add_argument("--dataset", type=str, default="cifar10", choices=["cifar10", "cifar100", "path"])
    p.add_argument("--mean", type=str, help="mean of dataset in path in form of str tuple")
    p.add_argument("--std", type=str, help="std of dataset in path in form of str tuple")
    p.add_argument("--data_folder", type=str, default=None, help="path to custom dataset")
    p.add_argument("--size", type=int, default=32, help="parameter for RandomResizedCrop")
    # method / temperature (main_supcon.py:59-63)
    p.add_argument("--method", type=str, default="SimCLR", choices=["SupCon", "SimCLR"])
    p.add_argument("--temp", type=float, default=0.5, help="temperature for loss function")
    # other (main_supcon.py:66-88)
    p.add_argument("--cosine", action="store_true", help="using cosine annealing")
    p.add_argument("--syncBN", action="store_true", help="using synchronized batch normalization")
    p.add_argument("--warm", action="store_true", help="warm-up for large batch training")
    p.add_argument("--trial", type=str, default="0", help="id for recording multiple runs")
    p.add_argument("--sec", action="store_true", help="add sec loss")
    p.add_argument("--sec_wei", type=float, default=0.0)
    p.add_argument("--norm_momentum", type=float, default=1.0)
    p.add_argument("--l2reg", action="store_true", help="add l2reg loss")
    p.add_argument("--l2reg_wei", type=float, default=0.0)
    p.add_argument("--ckpt", type=str, default="", help="path to pre-trained model")
    p.add_argument("--local_rank", "--local-rank", dest="local_rank", type=int, default=0)
    p.add_argument("--ngpu", type=int, default=None,
                   help="world size (defaults to WORLD_SIZE from the launcher)")
    g = p.add_argument_group("pretraining additions")
    g.add_argument("--optimizer", type=str, default="sgd", choices=["sgd", "lars"])
    g.add_argument("--grad_semantics", type=str, default="ref", choices=["ref", "exact"],
                   help="ref: DDP-mean of the global loss gradient (reference, SURVEY Q2); exact: W x that")
    g.add_argument("--grad_compress", type=str, default="none", choices=["none", "bf16"],
                   help="gradient bucket all-reduce payload: fp32 (reference DDP) or bf16 (half the "
                        "xGMI bytes; sums rounded to bf16)")
    g.add_argument("--base_temperature", type=float, default=0.07)
    g.add_argument("--contrast_mode", type=str, default="all", choices=["all", "one"])
    g.add_argument("--resume", type=str, default="", help="resume model+optimizer+epoch+state from a ckpt")
    g.add_argument("--micro_batch", type=int, default=0,
                   help="gradient-cache micro-batching: encoder forward/backward in chunks of this many "
                        "VIEWS per rank (0 = whole local batch); the contrastive loss still sees the full batch")
    g.add_argument("--knn_freq", type=int, default=0,
                   help="weighted k-NN accuracy of the encoder on the validation split every N epochs and "
                        "after the last epoch (0 = off)")
    _add_knn_flags(g)
    g.add_argument("--blur_p", type=float, default=0.0,
                   help="probability of the Gaussian-blur augmentation after grayscale (SimCLR's ImageNet "
                        "recipe uses 0.5; 0 = off, the CIFAR recipe)")
    g.add_argument("--blur_kernel", type=int, default=0,
                   help="blur kernel size, odd (0 = 10%% of --size, made odd, at least 3)")
    g.add_argument("--blur_sigma", type=float, nargs=2, default=[0.1, 2.0], metavar=("LO", "HI"),
                   help="blur sigma is drawn uniformly from [LO, HI]")
    _add_eval_flags(g)
    _add_common_new_flags(p)
    return p


def _finish_common(opt, prefix_dirs: bool):
    it = opt.lr_decay_epochs.split(",") if isinstance(opt.lr_decay_epochs, str) else opt.lr_decay_epochs
    opt.lr_decay_epochs = [int(x) for x in it if str(x).strip() != ""]
    return opt


def _warm_fields(opt):
    # main_supcon.py:120-131 / main_linear.py:79-89
    if opt.warm:
        opt.model_name = f"{opt.model_name}_warm"
        opt.warmup_from = 0.01
        opt.warm_epochs = 10
        if opt.cosine:
            eta_min = opt.learning_rate * (opt.lr_decay_rate ** 3)
            opt.warmup_to = eta_min + (opt.learning_rate - eta_min) * (
                1 + math.cos(math.pi * opt.warm_epochs / opt.epochs)) / 2
        else:
            opt.warmup_to = opt.learning_rate


def unique_dir(path: str) -> str:
    """Collision guard for minute-resolution run folders."""
    if not os.path.exists(path):
        return path
    i = 1
    while os.path.exists(f"{path}_{i}"):
        i += 1
    return f"{path}_{i}"


def parse_pretrain(argv: Optional[Sequence[str]] = None, make_dirs: bool = True,
                   now: Optional[datetime.datetime] = None):
    opt = pretrain_parser().parse_args(argv)
    if opt.dataset == "path":
        assert opt.data_folder is not None and opt.mean is not None and opt.std is not None
    if opt.knn_freq < 0 or opt.knn_k < 1 or not opt.knn_t > 0:
        raise ValueError("--knn_freq >= 0, --knn_k >= 1 and --knn_t > 0 are required")
    if opt.knn_freq > 0 and opt.dataset == "path" and opt.val_folder is None:
        raise ValueError("--knn_freq needs a dataset with a validation split (cifar10, cifar100 or --synthetic); "
                         "--dataset path has none unless --val_folder names one")
    if opt.dataset == "path":
        _check_val_folder(opt)
    opt.blur_sigma = tuple(opt.blur_sigma)
    if not 0.0 <= opt.blur_p <= 1.0 or opt.blur_kernel < 0 or not 0.0 < opt.blur_sigma[0] <= opt.blur_sigma[1]:
        raise ValueError("--blur_p in [0, 1], --blur_kernel >= 0 and --blur_sigma 0 < LO <= HI are required")
    rank, local_rank, world = env_rank_info(opt.local_rank)
    opt.rank, opt.local_rank = rank, local_rank
    if opt.ngpu is None:
        opt.ngpu = world
    opt.world_size = opt.ngpu
    if opt.data_folder is None:
        opt.data_folder = "./datasets/"
    opt.model_path = os.path.join(opt.work_dir, f"{opt.dataset}_models")
    opt.tb_path = os.path.join(opt.work_dir, f"{opt.dataset}_tensorboard")
    _finish_common(opt, True)
    # main_supcon.py:109-117
    opt.model_name = "{}_{}_{}_lr_{}_decay_{}_bsz_{}_temp_{}_trial_{}".format(
        opt.method, opt.dataset, opt.model, opt.learning_rate, opt.weight_decay,
        opt.batch_size, opt.temp, opt.trial)
    if opt.cosine:
        opt.model_name = f"{opt.model_name}_cosine"
    if opt.sec:
        opt.model_name = f"{opt.model_name}_sec"
    if opt.batch_size > 256:
        opt.warm = True
    _warm_fields(opt)
    now = now or datetime.datetime.now()
    conf_work_path = f"{opt.dataset}_" + now.strftime("%m%d_%H%M") + "_"
    opt.conf_work_path = conf_work_path
    opt.tb_folder = os.path.join(opt.tb_path, conf_work_path + opt.model_name)
    opt.save_folder = os.path.join(opt.model_path, conf_work_path + opt.model_name)
    if make_dirs and opt.rank == 0:
        if os.path.isdir(opt.save_folder) and not opt.resume:
            opt.save_folder = unique_dir(opt.save_folder)
            opt.tb_folder = unique_dir(opt.tb_folder)
        os.makedirs(opt.tb_folder, exist_ok=True)
        os.makedirs(opt.save_folder, exist_ok=True)
    if opt.dataset == "path":
        opt.mean_t, opt.std_t = parse_tuple(opt.mean), parse_tuple(opt.std)
    else:
        opt.mean_t, opt.std_t = DATASET_STATS[opt.dataset]
    opt.n_cls = N_CLASSES.get(opt.dataset, 0)
    opt.record_norm_mean = None  # main_supcon.py:150
    if opt.batch_size % opt.world_size != 0:
        raise ValueError(f"--batch_size {opt.batch_size} must be divisible by world size {opt.world_size}")
    opt.local_batch = opt.batch_size // opt.world_size
    return opt


def linear_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser("argument for training")
    # main_linear.py:24-61
    p.add_argument("--print_freq", type=int, default=10, help="print frequency")
    p.add_argument("--save_freq", type=int, default=10, help="save frequency")
    p.add_argument("--batch_size", type=int, default=512, help="batch_size")
    p.add_argument("--num_workers", type=int, default=16, help="num of workers to use")
    p.add_argument("--epochs", type=int, default=100, help="number of training epochs")
    p.add_argument("--learning_rate", type=float, default=0.1, help="learning rate")
    p.add_argument("--lr_decay_epochs", type=str, default="60,75,90", help="where to decay lr")
    p.add_argument("--lr_decay_rate", type=float, default=0.2, help="decay rate for learning rate")
    p.add_argument("--weight_decay", type=float, default=0, help="weight decay")
    p.add_argument("--momentum", type=float, default=0.9, help="momentum")
    p.add_argument("--model", type=str, default="resnet50")
    p.add_argument("--dataset", type=str, default="cifar10", choices=["cifar10", "cifar100", "path"])
    p.add_argument("--cosine", action="store_true", help="using cosine annealing")
    p.add_argument("--warm", action="store_true", help="warm-up for large batch training")
    p.add_argument("--ckpt", type=str, default="", help="path to pre-trained model")
    g = p.add_argument_group("linear-probe additions")
    g.add_argument("--data_folder", type=str, default="./datasets/")
    g.add_argument("--val_batch_size", type=int, default=256)
    g.add_argument("--local_rank", "--local-rank", dest="local_rank", type=int, default=0)
    g.add_argument("--knn", action="store_true",
                   help="report the loaded checkpoint's weighted k-NN accuracy before classifier training")
    _add_knn_flags(g)
    g.add_argument("--size", type=int, default=32, help="input size (CenterCrop / RandomResizedCrop)")
    g.add_argument("--mean", type=str, help="mean of dataset in path in form of str tuple")
    g.add_argument("--std", type=str, help="std of dataset in path in form of str tuple")
    _add_eval_flags(g)
    g.add_argument("--sweep_lr", type=float, nargs="+", default=None, metavar="LR",
                   help="train one classifier per learning rate on the same encoder pass (with --sweep_wd: "
                        "one per (lr, wd) pair, at most 16) and report the best")
    g.add_argument("--sweep_wd", type=float, nargs="+", default=None, metavar="WD",
                   help="weight decays of the sweep (absent: --weight_decay)")
    _add_head_gemm_flag(g)
    g.add_argument("--cache_features", type=str, default=argparse.SUPPRESS, choices=list(CACHE_MODES),
                   help="the encoder is frozen: val = encode the validation store once and validate every epoch on "
                        "those features (results identical to off); all = also train on a feature bank of the "
                        "training store extracted once (see --cache_views); default off")
    g.add_argument("--cache_views", type=int, default=argparse.SUPPRESS, metavar="V",
                   help="with --cache_features all: 0 = one bank row per image under the evaluation transform (no "
                        "training augmentation); V >= 1 = V rows per image, independent draws of the training "
                        "augmentation, epoch e using view (e - 1) mod V; default 0")
    _add_common_new_flags(p)
    return p


SWEEP_MAX_HEADS = 16
CACHE_MODES = ("off", "val", "all")


class _HeadOptions(argparse.Namespace):
    """``opt.head_gemm`` reads "fma" (and ``opt.cache_features`` "off", ``opt.cache_views`` 0) when
    the flag is absent without becoming an entry of ``vars(opt)``: a run that does not use the flag
    keeps the namespace (and the saved options) it had before the flag existed."""
    head_gemm = "fma"
    cache_features = "off"
    cache_views = 0


class _CeOptions(_HeadOptions):
    """The supervised trainer's soft-target flags, absent from ``vars(opt)`` when not given."""
    label_smoothing = 0.0
    mixup = 0.0
    cutmix = 0.0
    mix_prob = 1.0
    mix_switch_prob = 0.5
    # knowledge distillation (likewise absent from ``vars(opt)`` without --distill_ckpt)
    distill_ckpt = ""
    distill_model = None
    distill_temp = 1.0
    distill_alpha = 1.0


def _add_mix_flags(g):
    S = argparse.SUPPRESS
    g.add_argument("--label_smoothing", type=float, default=S, metavar="E",
                   help="label smoothing: the target is (1 - E) x the label distribution + E / n_cls; 0 <= E < 1, "
                        "default 0")
    g.add_argument("--mixup", type=float, default=S, metavar="A",
                   help="Mixup: blend every image with its batch neighbour, lambda ~ Beta(A, A) per step; default 0 = off")
    g.add_argument("--cutmix", type=float, default=S, metavar="A",
                   help="CutMix: paste a box of the batch neighbour, box area 1 - lambda, lambda ~ Beta(A, A) per step; "
                        "default 0 = off")
    g.add_argument("--mix_prob", type=float, default=S, metavar="P",
                   help="probability that a step mixes at all (with --mixup / --cutmix); default 1")
    g.add_argument("--mix_switch_prob", type=float, default=S, metavar="Q",
                   help="with both --mixup and --cutmix: probability that a mixing step uses CutMix; default 0.5")


def _check_mix_flags(parser, opt):
    """Ranges of the soft-target flags (a parser error outside them) and the model_name suffix of
    those in effect."""
    if not 0.0 <= opt.label_smoothing < 1.0:
        parser.error(f"--label_smoothing {opt.label_smoothing} must be in [0, 1)")
    for name in ("mixup", "cutmix"):
        a = getattr(opt, name)
        if not (0.0 <= a < math.inf):
            parser.error(f"--{name} {a}: the Beta parameter must be finite and >= 0 (0 = off)")
    for name in ("mix_prob", "mix_switch_prob"):
        v = getattr(opt, name)
        if not 0.0 <= v <= 1.0:
            parser.error(f"--{name} {v} must be in [0, 1]")
    suffix = ""
    if opt.label_smoothing > 0:
        suffix += f"_ls_{opt.label_smoothing}"
    if opt.mixup > 0:
        suffix += f"_mixup_{opt.mixup}"
    if opt.cutmix > 0:
        suffix += f"_cutmix_{opt.cutmix}"
    if opt.mixup > 0 or opt.cutmix > 0:
        if opt.mix_prob != 1.0:
            suffix += f"_mixp_{opt.mix_prob}"
        if opt.mixup > 0 and opt.cutmix > 0 and opt.mix_switch_prob != 0.5:
            suffix += f"_switch_{opt.mix_switch_prob}"
    return suffix


def _add_distill_flags(g):
    S = argparse.SUPPRESS
    g.add_argument("--distill_ckpt", type=str, default=S, metavar="PATH",
                   help="knowledge distillation: a main_ce.py checkpoint whose whole model (encoder and fc) is the "
                        "frozen teacher; the loss becomes (1 - A) x cross-entropy + A x T^2 x KL(teacher || student) "
                        "at temperature T")
    g.add_argument("--distill_model", type=str, default=S, metavar="NAME",
                   help="the teacher's architecture (with --distill_ckpt); default: --model")
    g.add_argument("--distill_temp", type=float, default=S, metavar="T",
                   help="distillation temperature (with --distill_ckpt), > 0; default 1")
    g.add_argument("--distill_alpha", type=float, default=S, metavar="A",
                   help="weight of the distillation term (with --distill_ckpt), in [0, 1]; default 1: no label is "
                        "used and every training image is sampled, whatever --label_frac is")


def _check_distill_flags(parser, opt):
    """The distillation flags: the dependent ones need --distill_ckpt, ranges (a parser error
    otherwise); -> the model_name suffix."""
    given = vars(opt)
    if not given.get("distill_ckpt"):
        if "distill_ckpt" in given:
            parser.error("--distill_ckpt needs a path")
        for name in ("distill_model", "distill_temp", "distill_alpha"):
            if name in given:
                parser.error(f"--{name} needs --distill_ckpt")
        return ""
    if not 0.0 < opt.distill_temp < math.inf:
        parser.error(f"--distill_temp {opt.distill_temp} must be finite and > 0")
    if not 0.0 <= opt.distill_alpha <= 1.0:
        parser.error(f"--distill_alpha {opt.distill_alpha} must be in [0, 1]")
    if opt.distill_model is None:
        opt.distill_model = opt.model
    return f"_distill_{opt.distill_model}_T_{opt.distill_temp}_a_{opt.distill_alpha}"


def _add_head_gemm_flag(g):
    g.add_argument("--head_gemm", type=str, default=argparse.SUPPRESS, choices=["fma", "mfma"],
                   help="classifier GEMMs: fma = the fp32 kernels (K = 64·2^j <= 2048, C <= 1024), mfma = split-bf16 "
                        "MFMA GEMMs (csrc/kernels/head_gemm.hip: K = 64·j <= 4096, C <= 32768); default fma")


def _sweep_heads(parser, opt):
    """``opt.sweep``: None, or the (lr, wd) of every head of --sweep_lr x --sweep_wd, lr-major; an
    absent list stands for the single --learning_rate / --weight_decay."""
    lrs, wds = opt.sweep_lr, opt.sweep_wd
    del opt.sweep_lr, opt.sweep_wd
    opt.sweep = None
    if lrs is None and wds is None:
        return
    lrs = [opt.learning_rate] if lrs is None else lrs
    wds = [opt.weight_decay] if wds is None else wds
    if any(not lr > 0 for lr in lrs):
        parser.error("--sweep_lr: every learning rate must be positive")
    if any(not wd >= 0 for wd in wds):
        parser.error("--sweep_wd: a weight decay cannot be negative")
    if len(lrs) * len(wds) > SWEEP_MAX_HEADS:
        parser.error(f"--sweep_lr x --sweep_wd gives {len(lrs) * len(wds)} heads; at most {SWEEP_MAX_HEADS}")
    opt.sweep = [(float(lr), float(wd)) for lr in lrs for wd in wds]


def sweep_head_opts(opt):
    """One copy of ``opt`` per sweep head with that head's ``learning_rate``, ``weight_decay`` and,
    with --warm, ``warmup_to``: the schedules (optim/schedules.py) read these."""
    import copy
    heads = []
    for lr, wd in opt.sweep:
        o = copy.copy(opt)
        o.learning_rate, o.weight_decay = lr, wd
        name = o.model_name
        _warm_fields(o)
        o.model_name = name
        heads.append(o)
    return heads


def parse_linear(argv: Optional[Sequence[str]] = None, make_dirs: bool = True,
                 now: Optional[datetime.datetime] = None):
    parser = linear_parser()
    opt = parser.parse_args(argv, namespace=_HeadOptions())
    _sweep_heads(parser, opt)
    if opt.cache_views < 0:
        parser.error(f"--cache_views {opt.cache_views}: the number of cached views cannot be negative")
    if opt.cache_views > 0 and opt.cache_features != "all":
        parser.error(f"--cache_views {opt.cache_views} needs --cache_features all (got {opt.cache_features}): "
                     "only the training bank has views")
    if opt.knn_k < 1 or not opt.knn_t > 0:
        raise ValueError("--knn_k >= 1 and --knn_t > 0 are required")
    if opt.size < 1:
        raise ValueError("--size >= 1 is required")
    if opt.dataset == "path":
        if opt.mean is None or opt.std is None:
            raise ValueError("--dataset path needs --mean and --std")
        if opt.val_folder is None and not opt.synthetic:
            raise ValueError("--dataset path needs --val_folder (the validation ImageFolder) or --synthetic")
        _check_val_folder(opt)
    rank, local_rank, world = env_rank_info(opt.local_rank)
    opt.rank, opt.local_rank, opt.world_size = rank, local_rank, world
    _finish_common(opt, True)
    opt.model_name = "{}_{}_lr_{}_decay_{}_bsz_{}".format(
        opt.dataset, opt.model, opt.learning_rate, opt.weight_decay, opt.batch_size)
    if opt.cosine:
        opt.model_name = f"{opt.model_name}_cosine"
    _warm_fields(opt)
    if opt.sweep is not None:
        opt.model_name = f"{opt.model_name}_sweep{len(opt.sweep)}"
    # path: the class count comes from the dataset at engine start
    opt.n_cls = N_CLASSES.get(opt.dataset, 0)
    now = now or datetime.datetime.now()
    conf_work_path = "classifier_" + now.strftime("%m%d_%H%M") + "_"
    opt.conf_work_path = conf_work_path
    opt.tb_path = os.path.join(opt.work_dir, f"{opt.dataset}_tensorboard")
    opt.tb_folder = os.path.join(opt.tb_path, conf_work_path + opt.model_name)
    opt.model_path = os.path.join(opt.work_dir, f"{opt.dataset}_models")
    opt.save_folder = os.path.join(opt.model_path, conf_work_path + opt.model_name)
    if make_dirs and opt.rank == 0:
        if os.path.isdir(opt.save_folder):
            opt.save_folder = unique_dir(opt.save_folder)
            opt.tb_folder = unique_dir(opt.tb_folder)
        os.makedirs(opt.tb_folder, exist_ok=True)
        os.makedirs(opt.save_folder, exist_ok=True)
    if opt.dataset == "path":
        opt.mean_t, opt.std_t = parse_tuple(opt.mean), parse_tuple(opt.std)
    else:
        opt.mean_t, opt.std_t = DATASET_STATS[opt.dataset]
    return opt


def ce_parser() -> argparse.ArgumentParser:
    """Supervised cross-entropy training / fine-tuning (main_ce.py). Flag names and defaults follow
    main_linear.py (schedule) and main_supcon.py (training: --syncBN, --optimizer, --resume)."""
    p = argparse.ArgumentParser("argument for supervised training")
    p.add_argument("--print_freq", type=int, default=10, help="print frequency")
    p.add_argument("--save_freq", type=int, default=50, help="save frequency")
    p.add_argument("--batch_size", type=int, default=256, help="batch_size (global)")
    p.add_argument("--num_workers", type=int, default=16, help="num of workers to use")
    p.add_argument("--epochs", type=int, default=500, help="number of training epochs")
    p.add_argument("--learning_rate", type=float, default=0.2, help="learning rate")
    p.add_argument("--lr_decay_epochs", type=str, default="350,400,450", help="where to decay lr")
    p.add_argument("--lr_decay_rate", type=float, default=0.1, help="decay rate for learning rate")
    p.add_argument("--weight_decay", type=float, default=1e-4, help="weight decay")
    p.add_argument("--momentum", type=float, default=0.9, help="momentum")
    p.add_argument("--model", type=str, default="resnet50")
    p.add_argument("--dataset", type=str, default="cifar10", choices=["cifar10", "cifar100", "path"])
    p.add_argument("--mean", type=str, help="mean of dataset in path in form of str tuple")
    p.add_argument("--std", type=str, help="std of dataset in path in form of str tuple")
    p.add_argument("--data_folder", type=str, default=None, help="path to custom dataset")
    p.add_argument("--size", type=int, default=32, help="parameter for RandomResizedCrop")
    p.add_argument("--cosine", action="store_true", help="using cosine annealing")
    p.add_argument("--syncBN", action="store_true", help="using synchronized batch normalization")
    p.add_argument("--warm", action="store_true", help="warm-up for large batch training")
    p.add_argument("--trial", type=str, default="0", help="id for recording multiple runs")
    p.add_argument("--ckpt", type=str, default="",
                   help="SupCon / SimCLR checkpoint whose encoder initialises the model (fine-tuning); "
                        "without it the run is the supervised baseline from scratch")
    p.add_argument("--local_rank", "--local-rank", dest="local_rank", type=int, default=0)
    p.add_argument("--ngpu", type=int, default=None, help="world size (defaults to WORLD_SIZE from the launcher)")
    g = p.add_argument_group("supervised-training additions")
    g.add_argument("--optimizer", type=str, default="sgd", choices=["sgd", "lars"])
    g.add_argument("--grad_compress", type=str, default="none", choices=["none", "bf16"],
                   help="gradient bucket all-reduce payload: fp32 or bf16")
    g.add_argument("--resume", type=str, default="", help="resume model+optimizer+epoch from a ckpt of this trainer")
    g.add_argument("--label_frac", type=float, default=1.0,
                   help="train on a class-balanced subset: per class ceil(f * n_c) images, drawn once from "
                        "--seed (the semi-supervised protocol: 0.01, 0.1)")
    g.add_argument("--val_freq", type=int, default=1, help="validate every N epochs and after the last epoch")
    g.add_argument("--val_batch_size", type=int, default=256)
    g.add_argument("--n_cls", type=int, default=0, help="number of classes (0 = from the dataset)")
    g.add_argument("--micro_batch", type=int, default=0, help="not supported by this trainer")
    g.add_argument("--blur_p", type=float, default=0.0,
                   help="> 0: the SimCLR augmentation with one view (colour jitter, grayscale and this "
                        "Gaussian-blur probability: the ImageNet recipe) instead of crop + flip")
    g.add_argument("--blur_kernel", type=int, default=0, help="blur kernel size, odd (0 = automatic)")
    g.add_argument("--blur_sigma", type=float, nargs=2, default=[0.1, 2.0], metavar=("LO", "HI"))
    _add_eval_flags(g)
    _add_head_gemm_flag(g)
    _add_mix_flags(g)
    _add_distill_flags(g)
    _add_common_new_flags(p)
    return p


def parse_ce(argv: Optional[Sequence[str]] = None, make_dirs: bool = True,
             now: Optional[datetime.datetime] = None):
    parser = ce_parser()
    opt = parser.parse_args(argv, namespace=_CeOptions())
    mix_suffix = _check_mix_flags(parser, opt) + _check_distill_flags(parser, opt)
    if opt.cuda_graph or opt.micro_batch:
        raise ValueError("main_ce.py supports neither --cuda_graph nor --micro_batch")
    if not 0.0 < opt.label_frac <= 1.0:
        raise ValueError(f"--label_frac {opt.label_frac} must be in (0, 1]")
    if opt.val_freq < 1 or opt.size < 1 or opt.n_cls < 0:
        raise ValueError("--val_freq >= 1, --size >= 1 and --n_cls >= 0 are required")
    opt.blur_sigma = tuple(opt.blur_sigma)
    if not 0.0 <= opt.blur_p <= 1.0 or opt.blur_kernel < 0 or not 0.0 < opt.blur_sigma[0] <= opt.blur_sigma[1]:
        raise ValueError("--blur_p in [0, 1], --blur_kernel >= 0 and --blur_sigma 0 < LO <= HI are required")
    if opt.dataset == "path":
        if opt.mean is None or opt.std is None:
            raise ValueError("--dataset path needs --mean and --std")
        if not opt.synthetic and (opt.data_folder is None or opt.val_folder is None):
            raise ValueError("--dataset path needs --data_folder and --val_folder (or --synthetic)")
        _check_val_folder(opt)
    rank, local_rank, world = env_rank_info(opt.local_rank)
    opt.rank, opt.local_rank = rank, local_rank
    if opt.ngpu is None:
        opt.ngpu = world
    opt.world_size = opt.ngpu
    if opt.data_folder is None:
        opt.data_folder = "./datasets/"
    _finish_common(opt, True)
    opt.model_name = "SupCE_{}_{}_lr_{}_decay_{}_bsz_{}_trial_{}".format(
        opt.dataset, opt.model, opt.learning_rate, opt.weight_decay, opt.batch_size, opt.trial)
    if opt.label_frac < 1.0:
        opt.model_name = f"{opt.model_name}_frac_{opt.label_frac}"
    opt.model_name += mix_suffix
    if opt.cosine:
        opt.model_name = f"{opt.model_name}_cosine"
    if opt.batch_size > 256:
        opt.warm = True
    _warm_fields(opt)
    now = now or datetime.datetime.now()
    conf_work_path = f"{opt.dataset}_" + now.strftime("%m%d_%H%M") + "_"
    opt.conf_work_path = conf_work_path
    opt.model_path = os.path.join(opt.work_dir, f"{opt.dataset}_models")
    opt.tb_path = os.path.join(opt.work_dir, f"{opt.dataset}_tensorboard")
    opt.tb_folder = os.path.join(opt.tb_path, conf_work_path + opt.model_name)
    opt.save_folder = os.path.join(opt.model_path, conf_work_path + opt.model_name)
    if make_dirs and opt.rank == 0:
        if os.path.isdir(opt.save_folder) and not opt.resume:
            opt.save_folder = unique_dir(opt.save_folder)
            opt.tb_folder = unique_dir(opt.tb_folder)
        os.makedirs(opt.tb_folder, exist_ok=True)
        os.makedirs(opt.save_folder, exist_ok=True)
    if opt.dataset == "path":
        opt.mean_t, opt.std_t = parse_tuple(opt.mean), parse_tuple(opt.std)
    else:
        opt.mean_t, opt.std_t = DATASET_STATS[opt.dataset]
    # path: the class count comes from the dataset at engine start
    if not opt.n_cls:
        opt.n_cls = N_CLASSES.get(opt.dataset, 0)
    if opt.batch_size % opt.world_size != 0:
        raise ValueError(f"--batch_size {opt.batch_size} must be divisible by world size {opt.world_size}")
    opt.local_batch = opt.batch_size // opt.world_size
    return opt
