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

Checkpoints have the reference's 4-key layout (engine/checkpoint.py); their ``encoder.*`` keys
load into ``main_linear.py --ckpt`` and the whole ``model`` into ``SupCEResNet``.
"""
from __future__ import annotations

import logging
import os
import sys
import time
from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from ..data.augment import AugConfig, augment, default_resize, nhwc8_to_nchw
from ..data.datasets import build_dataset
from ..data.sampler import DistributedIndexSampler, label_subset
from ..models.executor import ModelRunner
from ..models.resnet import SupCEResNet
from ..ops import _ext
from ..ops.ce_head import classifier_ce
from ..optim.flat import FlatParams, build_optimizer
from ..optim.schedules import adjust_learning_rate, warmup_learning_rate
from ..parallel import comm
from ..parallel.ddp import GradBucketReducer
from ..utils.logging import setup_logging
from ..utils.meters import AverageMeter
from ..utils.profiling import PhaseTimer
from . import checkpoint as ckpt_mod
from .pretrain import PretrainEngine, _priority_stream, resolve_backend, step_seed


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


class SupervisedEngine(PretrainEngine):
    """Shares the distributed set-up, SyncBN transports, augmentation call and gradient-buffer
    zeroing of :class:`PretrainEngine`; the model, the step, validation and logging are its own."""

    def __init__(self, opt, device: Optional[torch.device] = None):
        if getattr(opt, "cuda_graph", False) or getattr(opt, "micro_batch", 0):
            raise ValueError("the supervised trainer supports neither --cuda_graph nor --micro_batch")
        self.opt = opt
        rank, local_rank, world, dev = comm.init_distributed(opt.dist_backend, getattr(opt, "comm_timeout", 600.0),
                                                             device=device)
        self.rank, self.world, self.device = rank, world, dev
        self.stream = None
        if dev.type == "cuda" and os.environ.get("SDX_STREAM_PRIO", "1") != "0":
            self.stream = _priority_stream(dev)
            torch.cuda.set_stream(self.stream)
        if opt.ngpu != world and world > 1:
            logging.warning(f"--ngpu {opt.ngpu} != launcher WORLD_SIZE {world}; using {world}")
        opt.world_size = world
        opt.local_batch = opt.batch_size // world
        setup_logging(opt.save_folder, rank)
        if rank == 0:
            logging.info(f"create {opt.conf_work_path} ...")
        torch.manual_seed(opt.seed)
        self.backend = resolve_backend(opt.backend, dev, opt.stem)

        # data: whole uint8 training set resident on the device; an ImageFolder keeps native
        # resolutions (ragged store) for RandomResizedCrop, its validation split the Resize target
        nw, size = opt.num_workers, opt.size
        folder = opt.dataset == "path" and not opt.synthetic
        self.resize = (getattr(opt, "resize", 0) or default_resize(size)) if folder else 0
        tr = build_dataset(opt.dataset, opt.data_folder, True, opt.synthetic, opt.synthetic_size, size, opt.seed,
                           native=folder, workers=nw)
        va = build_dataset(opt.dataset, opt.val_folder if folder else opt.data_folder, False, opt.synthetic,
                           opt.synthetic_size, size, opt.seed, workers=nw, eval_resize=self.resize)
        if folder and tr.classes != va.classes:
            raise ValueError("--val_folder has other classes than --data_folder")
        if not opt.n_cls:
            opt.n_cls = max(tr.num_classes, va.num_classes)
        self.data = torch.from_numpy(tr.images).to(dev)
        self.data_offs = torch.from_numpy(tr.offsets).to(dev) if tr.ragged else None
        self.data_hw = torch.from_numpy(tr.sizes).to(dev) if tr.ragged else None
        self.labels = torch.from_numpy(tr.labels).to(dev)
        self.va_x, self.va_y = torch.from_numpy(va.images).to(dev), torch.from_numpy(va.labels).to(dev)
        self.va_offs = torch.from_numpy(va.offsets).to(dev) if va.ragged else None
        self.va_hw = torch.from_numpy(va.sizes).to(dev) if va.ragged else None
        self.n_val = len(va)
        # --label_frac: the labelled subset, the same on every rank; the sampler runs over it
        self._labels_np = np.asarray(tr.labels).astype(np.int64)
        self.subset = label_subset(self._labels_np, opt.label_frac, opt.seed)
        if opt.label_frac < 1.0:
            logging.info(f"--label_frac {opt.label_frac}: {self.subset.size} of {len(tr)} training images")
        self.sampler = DistributedIndexSampler(int(self.subset.size), opt.local_batch, world, rank, seed=opt.seed)
        if len(self.sampler) < 1:
            raise ValueError(f"{self.subset.size} training images make no batch of {opt.batch_size}")
        if getattr(opt, "blur_p", 0.0) > 0:
            import dataclasses
            self.aug = dataclasses.replace(AugConfig.simclr(size, opt.mean_t, opt.std_t, blur_p=opt.blur_p,
                                                            blur_kernel=opt.blur_kernel, blur_sigma=opt.blur_sigma),
                                           n_views=1)
        else:
            self.aug = AugConfig.linear_train(size, opt.mean_t, opt.std_t)
        self.aug_val = (AugConfig.center_crop(size, opt.mean_t, opt.std_t, self.resize) if folder
                        else AugConfig.evaluation(size, opt.mean_t, opt.std_t))

        model = SupCEResNet(opt.model, opt.n_cls, opt.stem)
        if opt.ckpt:
            n = load_encoder(model, opt.ckpt)
            logging.info(f"fine-tuning: {n} encoder tensors from {opt.ckpt}, fresh classifier")
        self.sync_group = None
        if opt.syncBN and world > 1:
            if self.backend == "torch":
                from ..parallel.syncbn import convert_sync_bn
                model = convert_sync_bn(model)
                self.syncbn_transport = "torch-syncbn"
            else:
                self.sync_group = dist.group.WORLD
                self._setup_syncbn_comm(opt, dev)
                if self.syncbn_transport == "none":
                    self.syncbn_transport = "process-group"
                self._syncbn_pending = False      # (no transport measurement in this trainer)
        model = model.to(dev)
        if dev.type == "cuda":
            model = model.to(memory_format=torch.channels_last)
        self.model = model
        # fc is part of the flat buffer: SGD / LARS, weight decay and the reducer treat it like
        # every other parameter
        self.flat = FlatParams(model)
        self.optimizer = build_optimizer(opt.optimizer, self.flat, opt.learning_rate, opt.momentum,
                                         opt.weight_decay, backend="torch" if self.backend == "torch" else "auto")
        self.reducer = (GradBucketReducer(self.flat, compress=getattr(opt, "grad_compress", "none"))
                        if world > 1 else None)
        self.optimizer.grad_scale = 1.0 / world
        self.runner = ModelRunner(model, self.backend, opt.precision, self.sync_group, master=self.flat.flat)
        self.logger = None
        if rank == 0:
            from ..utils.tb import Logger
            self.logger = Logger(opt.tb_folder, flush_secs=2)
        self.start_epoch = 1
        self.global_step = 0
        self._seed_t = torch.zeros((1,), dtype=torch.int64, device=dev)
        self._seed_host = 0
        self._seed_dev = False
        self.prof = PhaseTimer(getattr(opt, "profile", False), dev)
        self.knn = None
        self.history = []          # one dict per finished epoch (train / validation figures)
        if getattr(opt, "resume", ""):
            self._resume(opt.resume)

    def _resume(self, path):
        st = ckpt_mod.load_checkpoint(path)
        ckpt_mod.load_model_state(self.model, st["model"])
        self.optimizer.load_state_dict(st["optimizer"])
        self.start_epoch = int(st["epoch"]) + 1
        self.global_step = int((st.get("sdx_state") or {}).get("global_step", 0))
        logging.info(f"resumed from {path} at epoch {self.start_epoch}")

    def _extra_state(self, epoch):
        return {"global_step": self.global_step, "epoch": epoch, "n_cls": int(self.opt.n_cls),
                "label_frac": float(self.opt.label_frac)}

    # ------------------------------------------------------------------------------
    def _host_prelude(self, epoch: int, it: int, iters: int):
        warmup_learning_rate(self.opt, epoch, it, iters, self.optimizer)
        self.optimizer._sync_lr()
        self._seed_host = step_seed(self.opt.seed, epoch, it, self.rank)

    def _step_body(self, idx: torch.Tensor, labels: torch.Tensor, epoch: int = 1, it: int = 0):
        """Device work of one step: no host synchronisation."""
        ph = self.prof.phase
        with ph("augment"):
            prefetch = getattr(self.runner, "prefetch_weights", None)
            if prefetch is not None:
                prefetch()
            zeroed = self._zero_grad_side()
            x = self.make_views(idx, epoch, it)
        with ph("forward"):
            feat = self.runner.encode(x)
        with ph("loss"):
            loss, stats = classifier_ce(feat, self.model.fc, labels, native=self.backend == "native")
        with ph("backward"):
            if zeroed is not None:
                torch.cuda.current_stream(self.device).wait_event(zeroed)
            else:
                self.optimizer.zero_grad()
            one = getattr(self, "_one_grad", None)
            if one is None or one.device != loss.device or one.dtype != loss.dtype:
                one = self._one_grad = torch.ones((), device=loss.device, dtype=loss.dtype)
            loss.backward(one)
        if self.reducer is not None:
            with ph("grad_sync_wait"):
                self.reducer.finish()
        with ph("optimizer"):
            self.optimizer.step()
        return {"loss_local": loss.detach(), "stats": stats}

    def train_step(self, idx: torch.Tensor, labels: torch.Tensor, epoch: int, it: int, iters: int):
        self._host_prelude(epoch, it, iters)
        st = self._step_body(idx, labels, epoch, it)
        self.global_step += 1
        return st

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
        flush = getattr(self.runner, "flush_bn_counters", None)
        if flush is not None:
            flush()
        return losses.avg, top1.avg

    # ------------------------------------------------------------------------------
    @torch.no_grad()
    def validate(self):
        """(loss, top-1, top-5) of the current model on the validation split, eval-mode BatchNorm.
        Every rank evaluates the whole split (the replicas are identical)."""
        opt = self.opt
        was_training = self.model.training
        self.model.eval()
        fc = self.model.fc
        native = self.backend == "native"
        folded = None
        if native:
            from ..ops import linear_probe
            folded = linear_probe.FoldedEncoder(self.model.encoder)    # the weights of NOW
            native_ce = linear_probe.supported(self.model)
        tot = torch.zeros(3, dtype=torch.float64, device=self.device)
        n, vb = self.n_val, opt.val_batch_size
        for s in range(0, n, vb):
            idx = torch.arange(s, min(s + vb, n), device=self.device)
            x = augment(self.va_x, idx, self.aug_val, 0, self.va_offs, self.va_hw)
            labels = self.va_y[idx]
            if native:
                feat = folded(x)
                if native_ce:
                    st = _ext.require().linear_ce_step(feat.float().contiguous(), fc.weight.data, fc.bias.data,
                                                       labels.long(), None, None, 0.0, 0.0, 0.0, False, False)[1]
                else:
                    st = classifier_ce(feat, fc, labels, native=False)[1]
            else:
                feat = self.runner.encode(nhwc8_to_nchw(x), training=False).float()
                st = classifier_ce(feat, fc, labels, native=False)[1]
            tot += st.double()
        v = tot.tolist()
        self.model.train(was_training)
        loss, acc1, acc5 = v[0] / n, 100.0 * v[1] / n, 100.0 * v[2] / n
        logging.info(" * Acc@1 {:.3f}, Acc@5 {:.3f}, loss {:.4f}".format(acc1, acc5, loss))
        return loss, acc1, acc5

    def run(self):
        opt = self.opt
        best_acc = 0.0
        for epoch in range(self.start_epoch, opt.epochs + 1):
            adjust_learning_rate(opt, self.optimizer, epoch)
            t1 = time.time()
            loss, acc = self.train_epoch(epoch)
            logging.info("Train epoch {}, total time {:.2f}, accuracy:{:.2f}".format(epoch, time.time() - t1, acc))
            rec = {"epoch": epoch, "train_loss": loss, "train_acc": acc}
            if self.rank == 0:
                self.logger.log_value("train_loss", loss, epoch)
                self.logger.log_value("train_acc", acc, epoch)
                self.logger.log_value("learning_rate", self.optimizer.param_groups[0]["lr"], epoch)
            if epoch % opt.val_freq == 0 or epoch == opt.epochs:
                vloss, vacc, vacc5 = self.validate()
                rec.update(val_loss=vloss, val_acc=vacc, val_acc5=vacc5)
                best_acc = max(best_acc, vacc)
                if self.rank == 0:
                    self.logger.log_value("val_loss", vloss, epoch)
                    self.logger.log_value("val_acc", vacc, epoch)
                    self.logger.log_value("val_acc5", vacc5, epoch)
            self.history.append(rec)
            if epoch % opt.save_freq == 0 and self.rank == 0:
                f = os.path.join(opt.save_folder, f"ckpt_epoch_{epoch}.pth")
                ckpt_mod.save_model(self.model, self.optimizer, opt, epoch, f, self._extra_state(epoch))
            comm.barrier()
        logging.info("best accuracy: {:.2f}".format(best_acc))
        if self.rank == 0:
            f = os.path.join(opt.save_folder, "last.pth")
            ckpt_mod.save_model(self.model, self.optimizer, opt, opt.epochs, f, self._extra_state(opt.epochs))
            self.logger.close()
        comm.barrier()
        return os.path.join(opt.save_folder, "last.pth")
