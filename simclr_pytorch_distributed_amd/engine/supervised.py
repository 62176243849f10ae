"""Supervised cross-entropy training and end-to-end fine-tuning — the trainer of the reference's
main_ce.py (of which the reference keeps only the loaders, main_ce.py:19-68): ``SupCEResNet``
(networks/resnet_big.py:184-193) trained with ``nn.CrossEntropyLoss`` on single-view batches.

* from scratch it is the supervised baseline every SupCon / SimCLR number is reported against;
* ``--ckpt`` initialises the encoder from a SupCon / SimCLR checkpoint (projection-head keys
  ignored, ``fc`` fresh): fine-tuning, with ``--label_frac 0.01 / 0.1`` the semi-supervised
  protocol on a class-balanced label subset.

Per step (native backend): the rank's slice of the epoch permutation indexes the HBM-resident
uint8 dataset, the fused augmentation kernel writes one view per image, the fused block executor
encodes it (``ModelRunner.encode``), the classifier + cross-entropy node (ops/ce_head.py: two
launches) back-propagates into the features and accumulates the ``fc`` gradients into the flat
gradient buffer, the bucket reducer sums the buffer over the ranks and ONE fused SGD / LARS
kernel updates every parameter, ``fc`` included. The loss is the local-batch mean; the
optimizer's ``grad_scale`` = 1/W turns the ranks' sum into the global mean (DDP semantics).

Validation folds the CURRENT BatchNorm statistics into the convs (ops/linear_probe.py
``FoldedEncoder``, rebuilt every time: the encoder trains here) and evaluates with the fused
classifier kernel; ImageFolder runs use the GPU Resize + CenterCrop transform.

``--distill_ckpt`` (knowledge distillation, the SimCLRv2 stage 3): a frozen teacher — the whole
``model`` of a checkpoint of this trainer, ``fc`` included — encodes every step's views in eval
mode (native: a ``FoldedEncoder`` built once) and its logits enter the loss node as a constant:
(1 − α)·cross-entropy + α·τ²·KL(teacher ‖ student) (ops/ce_head.py). The teacher is no part of the
flat buffer, the optimizer, the reducer or the saved checkpoint; with α = 1 no label is used and
the sampler runs over the whole training store.

Checkpoints have the reference's 4-key layout (engine/checkpoint.py); their ``encoder.*`` keys
load into ``main_linear.py --ckpt`` and the whole ``model`` into ``SupCEResNet``.
"""
from __future__ import annotations

import dataclasses
import logging
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

from ..data import augment as aug_mod
from ..data.augment import AugConfig
from ..data.sampler import DistributedIndexSampler, label_subset
from ..data.store import probe_stores
from ..models.executor import ModelRunner
from ..models.resnet import SupCEResNet
from ..ops import _ext, linear_probe
from ..ops import ce_head
from ..ops.ce_head import classifier_ce
from ..parallel import comm
from ..utils.meters import AverageMeter
from ..utils.profiling import PhaseTimer
from . import checkpoint as ckpt_mod
from .base import TrainEngine


def load_encoder(model: torch.nn.Module, path: str):
    """Initialise ``model.encoder`` from the checkpoint of a SupCon / SimCLR (or supervised) run:
    every ``encoder.*`` tensor must be present; head / classifier keys are ignored."""
    sd = ckpt_mod.strip_prefix(ckpt_mod.load_checkpoint(path)["model"])
    enc = {k: v for k, v in sd.items() if k.startswith("encoder.")}
    missing, _ = ckpt_mod.load_model_state(model, enc, strict=False)
    lost = [k for k in missing if k.startswith("encoder.")]
    if lost or not enc:
        raise KeyError(f"{path}: encoder tensors missing from the checkpoint: {lost[:5] or 'all'}")
    return len(enc)


def load_teacher(path: str, name: str, n_cls: int, stem: str) -> SupCEResNet:
    """The distillation teacher: the whole ``model`` of a supervised-trainer checkpoint, ``fc``
    included, loaded strictly into a ``SupCEResNet`` of architecture ``name``; frozen and in eval
    mode. A classifier of another width than ``n_cls`` is refused."""
    sd = ckpt_mod.strip_prefix(ckpt_mod.load_checkpoint(path)["model"])
    if "fc.weight" not in sd:
        raise KeyError(f"{path}: no classifier (fc.weight) in the checkpoint: --distill_ckpt takes a main_ce.py "
                       f"checkpoint")
    n_teacher = int(sd["fc.weight"].shape[0])
    if n_teacher != int(n_cls):
        raise ValueError(f"--distill_ckpt {path}: the teacher classifies {n_teacher} classes (fc.out_features), "
                         f"the run has n_cls = {int(n_cls)}")
    with torch.random.fork_rng(devices=[]):      # the teacher's throw-away initial weights draw no student number
        teacher = SupCEResNet(name, n_teacher, stem)
    ckpt_mod.load_model_state(teacher, sd, strict=True)
    teacher.eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    return teacher


class SupervisedEngine(TrainEngine):
    """Shares the distributed set-up, SyncBN transports, augmentation call and gradient-buffer
    zeroing of :class:`PretrainEngine` through their base :class:`TrainEngine`; the model, the
    loss, validation and logging are its own."""

    data_first = True       # n_cls comes from the data

    def __init__(self, opt, device=None):
        if getattr(opt, "cuda_graph", False) or getattr(opt, "micro_batch", 0):
            raise ValueError("the supervised trainer supports neither --cuda_graph nor --micro_batch")
        super().__init__(opt, device)

    def _build_data(self):
        # data: whole uint8 training set resident on the device; an ImageFolder keeps native
        # resolutions (ragged store) for RandomResizedCrop, its validation split the Resize target
        opt = self.opt
        self.train, self.val, self.resize, self.aug_val, opt.n_cls = probe_stores(opt, self.device)
        # --label_frac: the labelled subset, the same on every rank; the sampler runs over it
        self._labels_np = self.train.labels.cpu().numpy().astype(np.int64)
        self.subset = label_subset(self._labels_np, opt.label_frac, opt.seed)
        if opt.label_frac < 1.0:
            logging.info(f"--label_frac {opt.label_frac}: {self.subset.size} of {len(self.train)} training images")
        if getattr(opt, "distill_ckpt", "") and float(getattr(opt, "distill_alpha", 1.0)) == 1.0:
            # no label enters the loss: every image is distilled
            self.subset = np.arange(len(self.train), dtype=np.int64)
            logging.info(f"--distill_alpha 1: sampling all {self.subset.size} training images whatever --label_frac "
                         f"is; the stored labels serve only the logged train Acc@1")
        self.sampler = DistributedIndexSampler(int(self.subset.size), opt.local_batch, self.world, self.rank,
                                               seed=opt.seed)
        if len(self.sampler) < 1:
            raise ValueError(f"{self.subset.size} training images make no batch of {opt.batch_size}")
        if getattr(opt, "blur_p", 0.0) > 0:
            self.aug = dataclasses.replace(AugConfig.simclr(opt.size, opt.mean_t, opt.std_t, blur_p=opt.blur_p,
                                                            blur_kernel=opt.blur_kernel, blur_sigma=opt.blur_sigma),
                                           n_views=1)
        else:
            self.aug = AugConfig.linear_train(opt.size, opt.mean_t, opt.std_t)

    def _build_model(self):
        # fc is part of the flat buffer: SGD / LARS, weight decay and the reducer treat it like
        # every other parameter
        opt = self.opt
        model = SupCEResNet(opt.model, opt.n_cls, opt.stem)
        if opt.ckpt:
            n = load_encoder(model, opt.ckpt)
            logging.info(f"fine-tuning: {n} encoder tensors from {opt.ckpt}, fresh classifier")
        return model

    def _init_state(self):
        self._syncbn_pending = False      # (no transport measurement in this trainer)
        self.history = []          # one dict per finished epoch (train / validation figures)
        self._head_gemm = None     # decided at the first step, when the model sits on its device
        opt = self.opt
        self.smoothing = float(getattr(opt, "label_smoothing", 0.0))
        self.mixing = getattr(opt, "mixup", 0.0) > 0 or getattr(opt, "cutmix", 0.0) > 0
        if self.mixing or self.smoothing > 0:
            on = [f"{k} {getattr(opt, k)}" for k in ("mixup", "cutmix") if getattr(opt, k, 0.0) > 0]
            if self.mixing:
                on.append(f"mix_prob {getattr(opt, 'mix_prob', 1.0)}")
            if len(on) == 3:
                on.append(f"mix_switch_prob {getattr(opt, 'mix_switch_prob', 0.5)}")
            if self.smoothing > 0:
                on.append(f"label_smoothing {self.smoothing}")
            logging.info("soft targets: " + ", ".join(on) + " (train Acc@1 counts the dominant label)")
        self.teacher = None
        if getattr(opt, "distill_ckpt", ""):
            self._build_teacher()

    def _build_teacher(self):
        """The frozen teacher of --distill_ckpt, built once: on the native backend a
        ``FoldedEncoder`` (it never changes) and, where the classifier kernels take its shape,
        the name of their evaluation op for its logits."""
        opt = self.opt
        name = getattr(opt, "distill_model", None) or opt.model
        self.distill_temp = float(getattr(opt, "distill_temp", 1.0))
        self.distill_alpha = float(getattr(opt, "distill_alpha", 1.0))
        teacher = load_teacher(opt.distill_ckpt, name, opt.n_cls, opt.stem).to(self.device)
        if self.device.type == "cuda":
            teacher = teacher.to(memory_format=torch.channels_last)
        self.teacher = teacher
        self._teacher_step = None
        if self.backend == "native":
            self._teacher_encode = linear_probe.FoldedEncoder(teacher.encoder)
            for gemm in dict.fromkeys((getattr(opt, "head_gemm", "fma"), "fma")):
                if linear_probe.supported(teacher, gemm=gemm):
                    self._teacher_step = "linear_ce_step_mfma" if gemm == "mfma" else "linear_ce_step"
                    break
        else:
            runner = ModelRunner(teacher, "torch", opt.precision)
            self._teacher_encode = lambda x: runner.encode(x, training=False)
        logging.info(f"distillation: teacher {name} from {opt.distill_ckpt}, temperature {self.distill_temp}, "
                     f"alpha {self.distill_alpha}, {self.subset.size} training images sampled")

    @torch.no_grad()
    def _teacher_logits(self, x: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """The teacher's fp32 logits [B, n_cls] of the step's views, queued on the compute stream."""
        fc = self.teacher.fc
        feat = self._teacher_encode(x).float()
        if self._teacher_step is not None:
            # the classifier kernels' evaluation form (as validate): logits only, nothing is updated
            return getattr(_ext.require(), self._teacher_step)(feat.contiguous(), fc.weight, fc.bias, labels.long().contiguous(), None, None,
                                      0.0, 0.0, 0.0, False, False)[0]
        return F.linear(feat, fc.weight, fc.bias)

    def head_gemm(self) -> str:
        """--head_gemm where it can run; else the default path, with one warning line."""
        if self._head_gemm is None:
            want = getattr(self.opt, "head_gemm", "fma")
            fc = self.model.fc
            if want == "mfma" and not (self.backend == "native" and ce_head.supported(fc, "mfma")):
                logging.warning("--head_gemm mfma cannot run here (backend %s, device %s, %d x %d classifier): "
                                "using the fma path", self.backend, fc.weight.device, fc.in_features,
                                fc.out_features)
                want = "fma"
            self._head_gemm = want
        return self._head_gemm

    def _extra_state(self, epoch):
        return dict(super()._extra_state(epoch), n_cls=int(self.opt.n_cls), label_frac=float(self.opt.label_frac))

    # ------------------------------------------------------------------------------
    def _step_body(self, idx: torch.Tensor, labels: torch.Tensor, epoch: int = 1, it: int = 0):
        """Device work of one step: no host synchronisation."""
        ph = self.prof.phase
        with ph("augment"):
            zeroed, x = self._start_step(idx, epoch, it)
        soft = {}
        if self.mixing or self.smoothing > 0:
            x, soft = self._mix(x, labels, epoch, it)
            labels = soft.pop("labels")
        if self.teacher is not None:
            with ph("teacher"):
                soft.update(teacher_logits=self._teacher_logits(x, labels), temp=self.distill_temp,
                            alpha=self.distill_alpha)
        with ph("forward"):
            feat = self.runner.encode(x)
        with ph("loss"):
            loss, stats = classifier_ce(feat, self.model.fc, labels, native=self.backend == "native",
                                        gemm=self.head_gemm(), **soft)
        self._backward_and_update(loss, zeroed)
        return {"loss_local": loss.detach(), "stats": stats}

    def _mix(self, x: torch.Tensor, labels: torch.Tensor, epoch: int, it: int):
        """Mixup / CutMix of the step's views by the host draw of ``mix_draw`` (one λ and one box
        per step, by value: no device random numbers, no synchronisation) and the soft-target
        arguments of ``classifier_ce``. The partner of row i is row i − 1; ``labels`` comes back as
        the label that weighs at least one half."""
        mode, lam, box = aug_mod.mix_draw(self.opt, self.opt.seed, epoch, it, self.rank)
        soft = {"labels": labels, "smoothing": self.smoothing}
        if mode == aug_mod.MIX_NONE:
            return x, soft
        with self.prof.phase("mix"):
            if self.backend == "native" and getattr(self.opt, "gpu_aug", 1):
                x = aug_mod.mix_views(x, mode, lam, *box)
            else:
                x = aug_mod.mix_reference(x, mode, lam, box, "nhwc" if self.backend == "native" else "nchw")
        labels2 = labels.roll(1)
        if lam < 0.5:
            labels, labels2, lam = labels2, labels, 1.0 - lam
        soft.update(labels=labels, labels2=labels2, lam=lam)
        return x, soft

    def train_step(self, idx: torch.Tensor, labels: torch.Tensor, epoch: int, it: int, iters: int):
        return self._train_step((idx, labels), epoch, it, iters)

    def epoch_batches(self, epoch: int):
        """(dataset indices, labels) of this rank's batches of ``epoch``: the sampler's
        permutation of the labelled subset mapped to dataset indices on the host and uploaded
        once per epoch, so a step gathers neither indices nor labels."""
        self.sampler.set_epoch(epoch)
        pos = self.sampler.indices()
        idx = self.subset[pos]
        idx_t = torch.from_numpy(idx).to(self.device, non_blocking=True)
        lab_t = torch.from_numpy(self._labels_np[idx]).to(self.device, non_blocking=True)
        b = self.sampler.b
        for i in range(len(self.sampler)):
            yield idx_t[i * b:(i + 1) * b], lab_t[i * b:(i + 1) * b]

    def train_epoch(self, epoch: int):
        opt = self.opt
        self.model.train()
        iters = len(self.sampler)
        if opt.max_steps:
            iters = min(iters, opt.max_steps)
        bt, dtm, losses, top1 = AverageMeter(), AverageMeter(), AverageMeter(), AverageMeter()
        win = torch.zeros(3, device=self.device)     # Σ CE, top-1 hits, top-5 hits of the window
        win_n = 0
        b = self.sampler.b
        end = time.time()
        t_window = time.time()
        for it, (idx, labels) in enumerate(self.epoch_batches(epoch)):
            if it >= iters:
                break
            dtm.update(time.time() - end)
            st = self.train_step(idx, labels, epoch, it, iters)
            win += st["stats"]
            win_n += 1
            bt.update(time.time() - end)
            end = time.time()
            if (it + 1) % opt.print_freq == 0 or it + 1 == iters:
                red = torch.cat([win, st["stats"]])
                if self.world > 1:
                    comm.all_reduce_sum_(red)
                v = red.tolist()                     # one host sync per print window
                n_win, n_last = win_n * b * self.world, b * self.world
                dt = (time.time() - t_window) / win_n
                t_window = time.time()
                losses.update(v[0] / n_win, n_win)
                top1.update(100.0 * v[1] / n_win, n_win)
                losses.val, top1.val, bt.val = v[3] / n_last, 100.0 * v[4] / n_last, dt
                if self.rank == 0:
                    logging.info("Train: [{0}][{1}/{2}]\tBT {bt.val:.3f} ({bt.avg:.3f})\t"
                                 "DT {dt.val:.3f} ({dt.avg:.3f})\tloss {loss.val:.3f} ({loss.avg:.3f})\t"
                                 "Acc@1 {top1.val:.3f} ({top1.avg:.3f})\timg/s {ips:.0f}".format(
                                     epoch, it + 1, iters, bt=bt, dt=dtm, loss=losses, top1=top1,
                                     ips=opt.batch_size / max(dt, 1e-9)))
                    if self.prof.enabled:
                        logging.info("phases (ms/step): " + PhaseTimer.format(self.prof.summary()))
                    sys.stdout.flush()
                win = torch.zeros(3, device=self.device)
                win_n = 0
        self.runner.flush_bn_counters()
        return losses.avg, top1.avg

    # ------------------------------------------------------------------------------
    @torch.no_grad()
    def validate(self):
        """(loss, top-1, top-5) of the current model on the validation split, eval-mode BatchNorm.
        Every rank evaluates the whole split (the replicas are identical)."""
        fc = self.model.fc
        native = self.backend == "native"
        encode, restore = linear_probe.eval_encoder(self.model, self.backend, self.runner)   # the weights of NOW
        gemm = self.head_gemm()
        native_ce = native and linear_probe.supported(self.model, gemm=gemm)
        step = getattr(_ext.require(), "linear_ce_step_mfma" if gemm == "mfma" else "linear_ce_step") \
            if native_ce else None
        tot = torch.zeros(3, dtype=torch.float64, device=self.device)
        n, vb = len(self.val), self.opt.val_batch_size
        for s in range(0, n, vb):
            idx = torch.arange(s, min(s + vb, n), device=self.device)
            x = self.val.views(idx, self.aug_val, 0)
            labels = self.val.labels[idx]
            feat = encode(x)
            if native_ce:
                st = step(feat.float().contiguous(), fc.weight.data, fc.bias.data,
                          labels.long(), None, None, 0.0, 0.0, 0.0, False, False)[1]
            else:
                st = classifier_ce(feat, fc, labels, native=False)[1]
            tot += st.double()
        restore()
        v = tot.tolist()
        loss, acc1, acc5 = v[0] / n, 100.0 * v[1] / n, 100.0 * v[2] / n
        logging.info(" * Acc@1 {:.3f}, Acc@5 {:.3f}, loss {:.4f}".format(acc1, acc5, loss))
        return loss, acc1, acc5

    def _epoch(self, epoch: int) -> dict:
        t1 = time.time()
        loss, acc = self.train_epoch(epoch)
        logging.info("Train epoch {}, total time {:.2f}, accuracy:{:.2f}".format(epoch, time.time() - t1, acc))
        self.history.append({"epoch": epoch, "train_loss": loss, "train_acc": acc})
        return {"train_loss": loss, "train_acc": acc}

    def _evaluate(self, epoch: int) -> dict:
        if not (epoch % self.opt.val_freq == 0 or epoch == self.opt.epochs):
            return {}
        vloss, vacc, vacc5 = self.validate()
        rec = {"val_loss": vloss, "val_acc": vacc, "val_acc5": vacc5}
        self.history[-1].update(rec)
        return rec

    def _end_of_run(self):
        best = max((h.get("val_acc", 0.0) for h in self.history), default=0.0)
        logging.info("best accuracy: {:.2f}".format(best))
