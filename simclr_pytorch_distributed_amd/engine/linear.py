"""Linear-probe evaluation engine — replaces main_linear.py:119-288 (+ main_ce.py:19-68 loaders).

Frozen encoder (eval-mode BN, no grad) + ``LinearClassifier`` trained with SGD and
cross-entropy; validation top-1/top-5 every epoch; the reported number is the best
validation top-1 (and the top-5 of that epoch), as in main_linear.py:284-288.

Fixes vs reference: checkpoint weights are always loaded (prefix-tolerant),
independent of GPU count. Augmentation runs on the GPU (RandomResizedCrop + flip +
normalize for training, normalize for validation) from the HBM-resident dataset.

Native backend (ops/linear_probe.py): the frozen encoder runs with every
eval-mode BatchNorm folded into its conv (one implicit-GEMM launch per conv + BN + ReLU, no
BN kernels), and the classifier's logits, cross-entropy, top-1/5 hits, gradient and SGD
update are two fused launches per batch; the meters stay on the device.

Sweep (``--sweep_lr`` / ``--sweep_wd``): G classifiers, one per (lr, wd) pair, are trained on
the same encoder pass, each on the reference schedule for its own base lr; on the native path
all of them are the same two launches (ops/linear_probe.py ``NativeLinearSweep``), elsewhere a
loop over G torch classifiers. Every head computes what a single run with its settings computes.

Feature cache (``--cache_features``): the encoder is frozen, so its features can be extracted once.
``val``: the validation store is encoded before epoch 1, in the batches ``validate`` uses, and every
epoch validates on slices of those features — the same numbers as ``off``. ``all``: the training
store is encoded once too, into a feature bank (``--cache_views`` 0: one row per image under the
evaluation transform; V >= 1: V draws of the training augmentation per image, epoch e on view
(e − 1) mod V), and a training step reads its batch from the bank by the sampler's indices; on the
native path inside the classifier's own launches (ops/linear_probe.py ``train_batch_rows``),
elsewhere as ``bank[rows]`` in front of the step that runs without a cache.
"""
from __future__ import annotations

import copy
import logging
import sys
import time
from typing import Optional

import torch

from ..config import sweep_head_opts
from ..data.augment import AugConfig
from ..data.sampler import DistributedIndexSampler
from ..data.store import probe_stores
from ..models.executor import ModelRunner
from ..models.resnet import LinearClassifier, SupConResNet
from ..ops import linear_probe
from ..optim.schedules import adjust_learning_rate, lr_at_epoch, set_lr, warmup_learning_rate, warmup_lr
from ..parallel import comm
from ..utils.logging import setup_logging
from ..utils.meters import AverageMeter, accuracy
from ..utils.profiling import PhaseTimer
from . import checkpoint as ckpt_mod
from .base import resolve_backend, step_seed


def free_memory(device: torch.device) -> Optional[int]:
    """Bytes a new allocation on ``device`` can take (``torch.cuda.mem_get_info``); None: not known."""
    if device.type != "cuda":
        return None
    return int(torch.cuda.mem_get_info(device)[0])


class LinearEngine:
    def __init__(self, opt, device: Optional[torch.device] = None, model: Optional[torch.nn.Module] = None):
        self.opt = opt
        rank, local_rank, world, dev = comm.init_distributed(opt.dist_backend, getattr(opt, "comm_timeout", 600.0), device=device)
        self.device = dev
        setup_logging(opt.save_folder, rank)
        logging.info(f"create {opt.conf_work_path} ...")
        torch.manual_seed(opt.seed)
        self.backend = resolve_backend(opt.backend, dev, opt.stem)
        if model is None:
            model = SupConResNet(opt.model, opt.head, opt.feat_dim, opt.stem)
            if opt.ckpt:
                st = ckpt_mod.load_checkpoint(opt.ckpt)
                ckpt_mod.load_model_state(model, st["model"])
                logging.info(f"loaded encoder from {opt.ckpt}")
            else:
                logging.warning("no --ckpt given: probing a randomly initialised encoder")
        model = model.to(dev)
        if dev.type == "cuda":
            model = model.to(memory_format=torch.channels_last)
        model.eval()
        for p in model.parameters():
            p.requires_grad_(False)
        self.model = model
        self.runner = ModelRunner(model, self.backend, opt.precision)
        self.train, self.val, self.resize, self.aug_val, opt.n_cls = probe_stores(opt, dev)
        # the reference DataLoader keeps the last partial batch (main_ce.py set_loader)
        self.sampler = DistributedIndexSampler(len(self.train), opt.batch_size, 1, 0, seed=opt.seed, drop_last=False)
        self.aug_train = AugConfig.linear_train(getattr(opt, "size", 32), opt.mean_t, opt.std_t)
        self.classifier = LinearClassifier(opt.model, opt.n_cls).to(dev)
        # the encoder is frozen: the native fold is computed once
        self.encode, _ = linear_probe.eval_encoder(model, self.backend, self.runner)
        self.folded = self.encode if self.backend == "native" else None      # the FoldedEncoder, when there is one
        self.native_ce = None
        # --head_gemm mfma: the classifier GEMMs on head_gemm.hip where they can run, else the
        # path of the default (fma) with one warning
        self.head_gemm = getattr(opt, "head_gemm", "fma")
        n_heads = len(getattr(opt, "sweep", None) or [None])
        if self.head_gemm == "mfma" and not (self.backend == "native" and
                                             linear_probe.sweep_supported(self.classifier, n_heads, gemm="mfma")):
            logging.warning("--head_gemm mfma cannot run here (backend %s, device %s, %d x %d classifier, %d heads): "
                            "using the fma path", self.backend, dev, self.classifier.fc.in_features,
                            self.classifier.fc.out_features, n_heads)
            self.head_gemm = "fma"
        if self.backend == "native" and linear_probe.supported(self.classifier, gemm=self.head_gemm):
            self.native_ce = linear_probe.NativeLinearCE(self.classifier, opt.momentum, opt.weight_decay,
                                                         gemm=self.head_gemm)
        self.criterion = torch.nn.CrossEntropyLoss()
        self.optimizer = torch.optim.SGD(self.classifier.parameters(), lr=opt.learning_rate, momentum=opt.momentum,
                                         weight_decay=opt.weight_decay)
        # --sweep_lr / --sweep_wd: G heads, every one a copy of the classifier above, trained on
        # the same features with their own lr schedule and weight decay
        self.sweep = getattr(opt, "sweep", None)
        self.sweep_results = None
        self.native_sweep = None
        if self.sweep:
            self.head_opts = sweep_head_opts(opt)
            self.head_lrs = [lr for lr, _ in self.sweep]
            wds = [wd for _, wd in self.sweep]
            if self.backend == "native" and linear_probe.sweep_supported(self.classifier, len(self.sweep),
                                                                         gemm=self.head_gemm):
                self.native_sweep = linear_probe.NativeLinearSweep(self.classifier, wds, opt.momentum,
                                                                   gemm=self.head_gemm)
            else:
                self.classifiers = [copy.deepcopy(self.classifier) for _ in self.sweep]
                self.optimizers = [torch.optim.SGD(c.parameters(), lr=lr, momentum=opt.momentum, weight_decay=wd)
                                   for c, (lr, wd) in zip(self.classifiers, self.sweep)]
        from ..utils.tb import Logger
        self.logger = Logger(opt.tb_folder, flush_secs=2)
        self.prof = PhaseTimer(getattr(opt, "profile", False), dev)
        # --cache_features: the banks are extracted by prepare_cache, before the first epoch
        self.cache = getattr(opt, "cache_features", "off")
        self.cache_views = getattr(opt, "cache_views", 0)
        self.val_bank: Optional[linear_probe.FeatureBank] = None
        self.bank: Optional[linear_probe.FeatureBank] = None

    @torch.no_grad()
    def _extract(self, store, cfg, batch: int, views: int, seeded: bool) -> linear_probe.FeatureBank:
        """The encoder's features of every image of ``store`` in index order, ``batch`` images per
        encoder pass, ``views`` times over (view v of batch i drawn with the seed that training
        step i of epoch v + 1 uses), written into one preallocated fp32 tensor."""
        n, k = len(store), self.classifier.fc.in_features
        feats = torch.empty(views * n, k, dtype=torch.float32, device=self.device)
        ph = self.prof.phase
        for v in range(views):
            for i, s in enumerate(range(0, n, batch)):
                idx = torch.arange(s, min(s + batch, n), device=self.device)
                with ph("augment"):
                    x = store.views(idx, cfg, step_seed(self.opt.seed, v + 1, i, 0) if seeded else 0)
                with ph("encoder"):
                    feats[v * n + s:v * n + s + idx.shape[0]] = self.encode(x)
        return linear_probe.FeatureBank(feats, store.labels.long().repeat(views), n, views)

    def prepare_cache(self):
        """--cache_features val / all: the extraction pass, once; refuses before it encodes anything
        when the banks do not fit the device."""
        if self.cache == "off" or self.val_bank is not None:
            return
        opt = self.opt
        k = self.classifier.fc.in_features
        views = max(self.cache_views, 1)
        shapes = [("val", len(self.val), 1)] + ([("train", len(self.train), views)] if self.cache == "all" else [])
        need = sum(linear_probe.FeatureBank.nbytes(n * v, k) for _, n, v in shapes)
        free = free_memory(self.device)
        if free is not None and need > free:
            raise RuntimeError(
                "--cache_features {}: the feature banks ({}) need {} bytes, the device has {} free; use {}".format(
                    self.cache, ", ".join(f"{nm} [{n * v}, {k}]" for nm, n, v in shapes), need, free,
                    "--cache_features val, fewer --cache_views or a smaller dataset" if self.cache == "all"
                    else "--cache_features off"))
        t0 = time.time()
        self.val_bank = self._extract(self.val, self.aug_val, opt.val_batch_size, 1, False)
        if self.cache == "all":
            cfg = self.aug_train if self.cache_views > 0 else self.aug_val
            self.bank = self._extract(self.train, cfg, opt.batch_size, views, self.cache_views > 0)
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        logging.info("feature cache ({}, {} views): {} fp32 + int64 labels, {} bytes, extracted in {:.2f}s".format(
            self.cache, self.cache_views, ", ".join(f"{nm} bank [{n * v}, {k}]" for nm, n, v in shapes), need,
            time.time() - t0))
        if self.prof.enabled:
            logging.info("phases (ms/batch, extraction): " + PhaseTimer.format(self.prof.summary()))

    def _bank_batch(self, view, idx):
        """(feats, labels, rows) of training batch ``idx`` of the bank view (feats [N, K], labels [N]):
        the native classifiers read the rows in place; elsewhere the batch is gathered here."""
        native = self.native_sweep if self.sweep else self.native_ce
        if native is not None:
            return view[0], view[1], idx
        return view[0][idx], view[1][idx], None

    def head_state(self, g: int):
        """``LinearClassifier`` state dict of sweep head ``g``."""
        if self.native_sweep is not None:
            return self.native_sweep.head_state(g)
        return {k: v.detach().clone() for k, v in self.classifiers[g].state_dict().items()}

    def _classify_sweep(self, feats, labels, train: bool, rows=None):
        """(logits [G, B, C], loss [G], acc1 [G], acc5 [G]) of a batch — device tensors; every
        value is computed as ``_classify`` computes a single classifier's."""
        bsz = labels.shape[0] if rows is None else rows.shape[0]
        if self.native_sweep is not None:
            if rows is not None:
                out, st = self.native_sweep.train_batch_rows(feats, labels, rows, self.head_lrs)
            elif train:
                out, st = self.native_sweep.train_batch(feats, labels, self.head_lrs)
            else:
                out, st = self.native_sweep.eval_batch(feats, labels)
            return out, st[:, 0] / bsz, st[:, 1] * (100.0 / bsz), st[:, 2] * (100.0 / bsz)
        outs, losses, a1s, a5s = [], [], [], []
        for clf, optim in zip(self.classifiers, self.optimizers):
            output = clf(feats.detach())
            loss = self.criterion(output, labels)
            acc1, acc5 = accuracy(output, labels, topk=(1, 5))
            if train:
                optim.zero_grad()
                loss.backward()
                optim.step()
            outs.append(output.detach())
            losses.append(loss.detach())
            a1s.append(acc1[0])
            a5s.append(acc5[0])
        return torch.stack(outs), torch.stack(losses), torch.stack(a1s), torch.stack(a5s)

    def _set_head_lrs(self, lrs):
        """``lrs[g]`` where it is not None becomes head g's learning rate."""
        for g, lr in enumerate(lrs):
            if lr is None:
                continue
            self.head_lrs[g] = lr
            if self.native_sweep is None:
                set_lr(self.optimizers[g], lr)

    def _train_epoch_sweep(self, epoch):
        """``train_epoch`` for G heads: per-head (loss, acc1, acc5) lists; the window line reports head 0."""
        opt = self.opt
        G = len(self.sweep)
        self.prepare_cache()
        view = self.bank.epoch_view(epoch) if self.bank is not None else None     # --cache_features all
        self.sampler.set_epoch(epoch)
        iters = len(self.sampler)
        if opt.max_steps:
            iters = min(iters, opt.max_steps)
        bt, dtm = AverageMeter(), AverageMeter()
        losses, top1, top5 = ([AverageMeter() for _ in range(G)] for _ in range(3))
        win = torch.zeros(G, 4, dtype=torch.float64, device=self.device)   # per head: Σloss·b, Σacc1·b, Σacc5·b, Σb
        end = time.time()
        for idx_i, idx in enumerate(self.sampler.batches(self.device)):
            if idx_i >= iters:
                break
            dtm.update(time.time() - end)
            ph = self.prof.phase
            rows = None
            if view is None:
                with ph("augment"):
                    x = self.train.views(idx, self.aug_train, step_seed(opt.seed, epoch, idx_i, 0))
                    labels = self.train.labels[idx]
            else:
                with ph("gather"):
                    feats, labels, rows = self._bank_batch(view, idx)
            bsz = idx.shape[0]
            self._set_head_lrs([warmup_lr(o, epoch, idx_i, iters) for o in self.head_opts])
            if view is None:
                with ph("encoder"):
                    feats = self.encode(x)
            with ph("classifier"):
                output, loss, acc1, acc5 = self._classify_sweep(feats, labels, True, rows)
                win += torch.stack([loss.double() * bsz, acc1.double() * bsz, acc5.double() * bsz,
                                    torch.full((G,), float(bsz), dtype=torch.float64, device=self.device)], dim=1)
            bt.update(time.time() - end)
            if (idx_i + 1) % opt.print_freq == 0 or idx_i + 1 == iters:
                # one host sync per print window: the sums and head 0's last batch together
                host = torch.cat([win.flatten(), loss[:1].double(), acc1[:1].double()]).tolist()
                win.zero_()
                for g in range(G):
                    sl, s1, s5, nb = host[4 * g:4 * g + 4]
                    losses[g].update(sl / nb, nb)
                    top1[g].update(s1 / nb, nb)
                    top5[g].update(s5 / nb, nb)
                losses[0].val, top1[0].val = host[4 * G], host[4 * G + 1]
                logging.info("Train: [{0}][{1}/{2}]\tBT {bt.val:.3f} ({bt.avg:.3f})\t"
                             "DT {dt.val:.3f} ({dt.avg:.3f})\tloss {loss.val:.3f} ({loss.avg:.3f})\t"
                             "Acc@1 {top1.val:.3f} ({top1.avg:.3f}) [h0 of {3}]".format(
                                 epoch, idx_i + 1, iters, G, bt=bt, dt=dtm, loss=losses[0], top1=top1[0]))
                if self.prof.enabled:
                    logging.info("phases (ms/step): " + PhaseTimer.format(self.prof.summary()))
                sys.stdout.flush()
            end = time.time()
        return [m.avg for m in losses], [m.avg for m in top1], [m.avg for m in top5]

    @torch.no_grad()
    def _validate_sweep(self):
        """``validate`` for G heads: per-head (loss, acc1, acc5) lists."""
        opt = self.opt
        G = len(self.sweep)
        n = len(self.val)
        losses, top1, top5 = ([AverageMeter() for _ in range(G)] for _ in range(3))
        vb = opt.val_batch_size
        self.prepare_cache()
        for i, s in enumerate(range(0, n, vb)):
            feats, labels = self._val_batch(s, min(s + vb, n))
            output, loss, acc1, acc5 = self._classify_sweep(feats, labels, False)
            bsz = labels.shape[0]
            host = torch.stack([loss, acc1, acc5], dim=1).tolist()
            for g in range(G):
                losses[g].update(host[g][0], bsz)
                top1[g].update(host[g][1], bsz)
                top5[g].update(host[g][2], bsz)
            if i % opt.print_freq == 0:
                logging.info("Test: [{0}/{1}]\tLoss {loss.val:.4f} ({loss.avg:.4f})\t"
                             "Acc@1 {top1.val:.3f} ({top1.avg:.3f}) [h0 of {2}]".format(
                                 i, (n + vb - 1) // vb, G, loss=losses[0], top1=top1[0]))
        for g in range(G):
            logging.info(" * h{0} Acc@1 {top1.avg:.3f}, Acc@5 {top5.avg:.3f}".format(g, top1=top1[g], top5=top5[g]))
        return [m.avg for m in losses], [m.avg for m in top1], [m.avg for m in top5]

    def _run_sweep(self):
        opt = self.opt
        G = len(self.sweep)
        res = [{"lr": lr, "wd": wd, "best_acc": 0.0, "best_acc5": 0.0, "best_epoch": 0} for lr, wd in self.sweep]
        if getattr(opt, "knn", False):
            self.knn_eval()
        self.prepare_cache()
        for epoch in range(1, opt.epochs + 1):
            self._set_head_lrs([lr_at_epoch(o, epoch) for o in self.head_opts])
            t1 = time.time()
            loss, acc, acc5 = self.train_epoch(epoch)
            logging.info("Train epoch {}, total time {:.2f}, accuracy:{}".format(
                epoch, time.time() - t1, " ".join("{:.2f}".format(a) for a in acc)))
            vloss, vacc, vacc5 = self.validate()
            for g in range(G):
                self.logger.log_value(f"classifier/train_loss/h{g}", loss[g], epoch)
                self.logger.log_value(f"classifier/train_acc1/h{g}", acc[g], epoch)
                self.logger.log_value(f"classifier/train_acc5/h{g}", acc5[g], epoch)
                self.logger.log_value(f"classifier/val_loss/h{g}", vloss[g], epoch)
                self.logger.log_value(f"classifier/val_acc1/h{g}", vacc[g], epoch)
                self.logger.log_value(f"classifier/val_acc5/h{g}", vacc5[g], epoch)
                if vacc[g] > res[g]["best_acc"]:
                    res[g].update(best_acc=vacc[g], best_acc5=vacc5[g], best_epoch=epoch)
        for g, r in enumerate(res):
            logging.info("head {} lr {:g} wd {:g}: best accuracy {:.2f}, accuracy5 {:.2f}".format(
                g, r["lr"], r["wd"], r["best_acc"], r["best_acc5"]))
        best = max(res, key=lambda r: r["best_acc"])      # the first of equals
        logging.info("best accuracy: {:.2f}, accuracy5: {:.2f}".format(best["best_acc"], best["best_acc5"]))
        self.sweep_results = res
        self.logger.close()
        return best["best_acc"], best["best_acc5"]

    def _classify(self, feats, labels, train: bool, rows=None):
        """(logits, loss, acc1, acc5) of a batch — device tensors; train: + the SGD step.
        ``rows`` (native training only, ``_bank_batch``): the batch is rows ``rows`` of the bank
        ``feats`` / ``labels``."""
        bsz = labels.shape[0] if rows is None else rows.shape[0]
        if self.native_ce is not None:
            if rows is not None:
                out, st = self.native_ce.train_batch_rows(feats, labels, rows, self.optimizer.param_groups[0]["lr"])
            elif train:
                out, st = self.native_ce.train_batch(feats, labels, self.optimizer.param_groups[0]["lr"])
            else:
                out, st = self.native_ce.eval_batch(feats, labels)
            return out, st[0] / bsz, st[1] * (100.0 / bsz), st[2] * (100.0 / bsz)
        output = self.classifier(feats.detach())
        loss = self.criterion(output, labels)
        acc1, acc5 = accuracy(output, labels, topk=(1, 5))
        if train:
            self.optimizer.zero_grad()
            loss.backward()
            self.optimizer.step()
        return output, loss.detach(), acc1[0], acc5[0]

    def train_epoch(self, epoch):
        if self.sweep:
            return self._train_epoch_sweep(epoch)
        opt = self.opt
        self.classifier.train()
        self.prepare_cache()
        view = self.bank.epoch_view(epoch) if self.bank is not None else None     # --cache_features all
        self.sampler.set_epoch(epoch)
        iters = len(self.sampler)
        if opt.max_steps:
            iters = min(iters, opt.max_steps)
        bt, dtm, losses, top1, top5 = AverageMeter(), AverageMeter(), AverageMeter(), AverageMeter(), AverageMeter()
        # every batch counts in the epoch meters (reference main_linear.py:151-155): the sums
        # stay on the device and reach the host once per print window
        win = torch.zeros(4, dtype=torch.float64, device=self.device)   # Σloss·b, Σacc1·b, Σacc5·b, Σb
        end = time.time()
        for idx_i, idx in enumerate(self.sampler.batches(self.device)):
            if idx_i >= iters:
                break
            dtm.update(time.time() - end)
            ph = self.prof.phase
            rows = None
            if view is None:
                with ph("augment"):
                    x = self.train.views(idx, self.aug_train, step_seed(opt.seed, epoch, idx_i, 0))
                    labels = self.train.labels[idx]
            else:
                with ph("gather"):
                    feats, labels, rows = self._bank_batch(view, idx)
            bsz = idx.shape[0]
            warmup_learning_rate(opt, epoch, idx_i, iters, self.optimizer)
            if view is None:
                with ph("encoder"):
                    feats = self.encode(x)
            with ph("classifier"):
                output, loss, acc1, acc5 = self._classify(feats, labels, True, rows)
                win += torch.stack([loss.double() * bsz, acc1.double() * bsz, acc5.double() * bsz,
                                    torch.tensor(float(bsz), dtype=torch.float64, device=self.device)])
            bt.update(time.time() - end)
            if (idx_i + 1) % opt.print_freq == 0 or idx_i + 1 == iters:
                sl, s1, s5, nb = win.tolist()       # one host sync per print window
                win.zero_()
                losses.update(sl / nb, nb)
                losses.val = loss.item()
                top1.update(s1 / nb, nb)
                top1.val = acc1.item()
                top5.update(s5 / nb, nb)
                logging.info("Train: [{0}][{1}/{2}]\tBT {bt.val:.3f} ({bt.avg:.3f})\t"
                             "DT {dt.val:.3f} ({dt.avg:.3f})\tloss {loss.val:.3f} ({loss.avg:.3f})\t"
                             "Acc@1 {top1.val:.3f} ({top1.avg:.3f})".format(
                                 epoch, idx_i + 1, iters, bt=bt, dt=dtm, loss=losses, top1=top1))
                if self.prof.enabled:
                    logging.info("phases (ms/step): " + PhaseTimer.format(self.prof.summary()))
                sys.stdout.flush()
            end = time.time()
        return losses.avg, top1.avg, top5.avg

    @torch.no_grad()
    def validate(self):
        if self.sweep:
            return self._validate_sweep()
        opt = self.opt
        self.classifier.eval()
        n = len(self.val)
        losses, top1, top5 = AverageMeter(), AverageMeter(), AverageMeter()
        vb = opt.val_batch_size
        self.prepare_cache()
        for i, s in enumerate(range(0, n, vb)):
            feats, labels = self._val_batch(s, min(s + vb, n))
            output, loss, acc1, acc5 = self._classify(feats, labels, False)
            bsz = labels.shape[0]
            losses.update(loss.item(), bsz)
            top1.update(acc1.item(), bsz)
            top5.update(acc5.item(), bsz)
            if i % opt.print_freq == 0:
                logging.info("Test: [{0}/{1}]\tLoss {loss.val:.4f} ({loss.avg:.4f})\t"
                             "Acc@1 {top1.val:.3f} ({top1.avg:.3f})".format(
                                 i, (n + vb - 1) // vb, loss=losses, top1=top1))
        logging.info(" * Acc@1 {top1.avg:.3f}, Acc@5 {top5.avg:.3f}".format(top1=top1, top5=top5))
        return losses.avg, top1.avg, top5.avg

    def _val_batch(self, s: int, e: int):
        """(feats, labels) of validation images s..e-1: encoded now, or (--cache_features) a slice
        of the features the same batch had in the extraction pass."""
        if self.val_bank is not None:
            return self.val_bank.feats[s:e], self.val_bank.labels[s:e]
        idx = torch.arange(s, e, device=self.device)
        x = self.val.views(idx, self.aug_val, 0)
        return self.encode(x), self.val.labels[idx]

    def knn_eval(self):
        """--knn: weighted k-NN accuracy of the loaded encoder (tags knn/val_acc1, knn/val_acc5 at step 0)."""
        from .knn import KnnEvaluator
        opt = self.opt
        t0 = time.time()
        ev = KnnEvaluator(self.model, self.backend, opt.precision, self.train, self.val, self.aug_val, opt.n_cls,
                          opt.knn_k, opt.knn_t, runner=self.runner if self.backend != "native" else None)
        acc1, acc5 = ev.evaluate()
        logging.info("kNN: epoch {} Acc@1 {:.2f} Acc@5 {:.2f} ({:.2f}s)".format(0, acc1, acc5, time.time() - t0))
        self.logger.log_value("knn/val_acc1", acc1, 0)
        self.logger.log_value("knn/val_acc5", acc5, 0)
        return acc1, acc5

    def run(self):
        if self.sweep:
            return self._run_sweep()
        opt = self.opt
        best_acc, best_acc5 = 0.0, 0.0
        if getattr(opt, "knn", False):
            self.knn_eval()
        self.prepare_cache()
        for epoch in range(1, opt.epochs + 1):
            adjust_learning_rate(opt, self.optimizer, epoch)
            t1 = time.time()
            loss, acc, acc5 = self.train_epoch(epoch)
            logging.info("Train epoch {}, total time {:.2f}, accuracy:{:.2f}".format(epoch, time.time() - t1, acc))
            self.logger.log_value("classifier/train_loss", loss, epoch)
            self.logger.log_value("classifier/train_acc1", acc, epoch)
            self.logger.log_value("classifier/train_acc5", acc5, epoch)
            vloss, vacc, vacc5 = self.validate()
            self.logger.log_value("classifier/val_loss", vloss, epoch)
            self.logger.log_value("classifier/val_acc1", vacc, epoch)
            self.logger.log_value("classifier/val_acc5", vacc5, epoch)
            if vacc > best_acc:
                best_acc, best_acc5 = vacc, vacc5
        logging.info("best accuracy: {:.2f}, accuracy5: {:.2f}".format(best_acc, best_acc5))
        self.logger.close()
        return best_acc, best_acc5
