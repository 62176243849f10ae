"""Contrastive pretraining engine (SimCLR / SupCon) — replaces main_supcon.py:155-406.

Per step (reference hot loop: main_supcon.py:253-349):

1. the rank's slice of the epoch permutation indexes the HBM-resident uint8 dataset and
   the fused GPU augmentation kernel writes both views (NHWC bf16) — no DataLoader
   workers, no H2D copy (reference: 8 CPU workers running PIL, main_supcon.py:200-207);
2. per-iteration warm-up lr (util.py:69-76) is written to the optimizer's device lr;
3. forward: native gfx950 encoder (or stock torch ops) + projection head;
4. loss: row-owned distributed SupCon/NT-Xent over globally gathered embeddings
   (losses/supcon.py) + the optional SEC / L2-reg feature-norm terms (main_supcon.py:295-317);
5. backward with bucketed gradient all-reduce overlapped on a comm stream
   (parallel/ddp.py), then one fused SGD/LARS kernel over the flat parameter buffer.

Logging keeps the reference's console format and TensorBoard tags; metric values stay on
device and are synchronised only every ``print_freq`` steps.
"""
from __future__ import annotations

import contextlib
import logging
import os
import sys
import time

import torch

from ..data.augment import AugConfig
from ..data.datasets import build_dataset
from ..data.sampler import DistributedIndexSampler
from ..data.store import DeviceStore, probe_stores
from ..losses.supcon import DistributedContrastiveLoss
from ..models.resnet import SupConResNet
from ..ops import _ext
from ..optim.flat import FusedSGD
from ..parallel import comm
from ..utils.faults import maybe_inject
from ..utils.meters import AverageMeter
from ..utils.profiling import PhaseTimer
from . import checkpoint as ckpt_mod
from .base import TrainEngine, resolve_backend, step_seed  # noqa: F401  (importable from here as before)

_NORM_SIDE = os.environ.get("SDX_NORM_SIDE", "1") != "0"


class PretrainEngine(TrainEngine):
    def _build_model(self):
        opt = self.opt
        model = SupConResNet(opt.model, opt.head, opt.feat_dim, opt.stem)
        if opt.ckpt:
            sd = ckpt_mod.load_checkpoint(opt.ckpt)["model"]
            ckpt_mod.load_model_state(model, sd)
            logging.info(f"load model from {opt.ckpt} ...")
        return model

    def _setup_more_comm(self, opt, dev):
        if self.world > 1 and self.backend == "native":
            self._setup_gather_comm(opt, dev)
        emu = int(os.environ.get("SDX_SYNCBN_EMU", "0") or 0)
        if emu > 1 and self.world == 1 and self.backend == "native" and dev.type == "cuda":
            # SyncBN over `emu` identical virtual ranks on this GPU (comm.EmulatedGroup):
            # SDX_SYNCBN_EMU_KIND=fused (default, the xGMI fused exchange) | emu (reduce ->
            # x·W -> finalize, the kernel sequence of the RCCL path minus the collective)
            self.sync_group = comm.EmulatedGroup(emu)
            m = _ext.require()
            kind = os.environ.get("SDX_SYNCBN_EMU_KIND", "fused")
            h = m.xgmi_emu_small_comm(emu) if kind == "fused" else m.emu_small_comm(emu)
            comm.set_native_small_comm(self.sync_group, h)
            self.syncbn_transport = f"emulated-{emu}-{kind}"
            logging.info(f"SyncBN emulated over {emu} virtual ranks ({kind})")

    def _early_step(self):
        # SDX_EARLY_STEP=1 (native SGD): each bucket's update runs as soon as its gradients are
        # final (after its collective with several ranks), overlapping the rest of backward.
        # Off by default: on one MI355X the step's tail shrinks by ~85 us but the update
        # kernels slow the concurrent critical-path backward kernels more (12.31 -> 12.44-12.60
        # ms/step same box, profiles/early_step_r3.txt)
        if (isinstance(self.optimizer, FusedSGD) and self.optimizer.native and not getattr(self.opt, "cuda_graph", False)
                and os.environ.get("SDX_EARLY_STEP", "0") == "1"):
            return self.optimizer.apply_range
        return None

    def _grad_scale(self):
        return super()._grad_scale() if self.opt.grad_semantics == "ref" else 1.0

    def _build_data(self):
        # data: whole uint8 dataset resident on the device; an ImageFolder as a native-resolution
        # ragged store (RandomResizedCrop on original pixels)
        opt = self.opt
        ds = build_dataset(opt.dataset, opt.data_folder, True, opt.synthetic, opt.synthetic_size, opt.size, opt.seed,
                           native=True, workers=opt.num_workers)
        self.train = DeviceStore.from_dataset(ds, self.device)
        self.sampler = DistributedIndexSampler(len(ds), opt.local_batch, self.world, self.rank, seed=opt.seed)
        self.aug = AugConfig.simclr(opt.size, opt.mean_t, opt.std_t, blur_p=getattr(opt, "blur_p", 0.0),
                                    blur_kernel=getattr(opt, "blur_kernel", 0),
                                    blur_sigma=getattr(opt, "blur_sigma", (0.1, 2.0)))

    def _init_state(self):
        opt, dev = self.opt, self.device
        self.criterion = DistributedContrastiveLoss(opt.method, opt.temp, opt.base_temperature, opt.contrast_mode,
                                                    backend="native" if self.backend == "native" else "torch")
        # device-resident step state (so the step body is graph-capturable)
        self.record_norm_mean = torch.zeros((), device=dev)
        self._rnm_valid = torch.zeros((), device=dev)
        self._ramp_t = torch.zeros((), device=dev)
        self._ns_sums = None
        self._graph = None
        self._graph_stats = None
        self._graph_failed = False
        self.knn = self._build_knn(self.train) if getattr(opt, "knn_freq", 0) > 0 else None

    def _build_knn(self, train: DeviceStore):
        """The weighted k-NN monitor (--knn_freq): bank = the training images already resident
        on the device, queries = the validation split, loaded here once. An ImageFolder's
        native-resolution ragged store is the bank in place (Resize + CenterCrop on the GPU at
        every evaluation, no second copy); its queries are --val_folder."""
        from .knn import KnnEvaluator
        opt = self.opt
        if train.ragged and not getattr(opt, "val_folder", None):
            raise ValueError("--knn_freq needs a fixed-size dataset with a validation split, or --val_folder")
        train, val, _, aug, n_cls = probe_stores(opt, self.device, train=train, n_cls_from_labels=True)
        return KnnEvaluator(self.model, self.backend, opt.precision, train, val, aug, n_cls, opt.knn_k, opt.knn_t,
                            runner=self.runner if self.backend != "native" else None)

    def knn_eval(self, epoch: int):
        """Run the k-NN monitor, log it and (rank 0) write knn/val_acc1, knn/val_acc5."""
        t0 = time.time()
        acc1, acc5 = self.knn.evaluate()
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        logging.info("kNN: epoch {} Acc@1 {:.2f} Acc@5 {:.2f} ({:.2f}s)".format(epoch, acc1, acc5, time.time() - t0))
        if self.rank == 0:
            self.logger.log_value("knn/val_acc1", acc1, epoch)
            self.logger.log_value("knn/val_acc5", acc5, epoch)
        return acc1, acc5

    def _setup_gather_comm(self, opt, dev):
        """Native transport of the contrastive loss's embedding all-gather / reduce-scatter
        (SURVEY §2.3 X5): the dedicated RCCL communicator (the SyncBN one when it is RCCL,
        else a new one; created and self-checked by all ranks together, 0 everywhere on
        failure -> c10d). gloo process groups keep the c10d path."""
        if dev.type != "cuda" or comm.backend() != "nccl" or os.environ.get("SDX_NATIVE_GATHER", "1") == "0":
            return
        m = _ext.require()
        h = comm.native_small_comm(None)
        if not (h and m.small_comm_kind(h) == 1):
            h = comm.create_rccl_small_comm(None, float(getattr(opt, "comm_timeout", 600.0)))
        if h:
            comm.set_native_gather_comm(None, h)
            logging.info("contrastive-loss embedding gather: dedicated RCCL communicator (native)")

    def _resume_extra(self, extra):
        rnm = extra.get("record_norm_mean")
        if rnm is not None:
            self.record_norm_mean.fill_(float(rnm))
            self._rnm_valid.fill_(1.0)

    def _extra_state(self, epoch):
        valid = float(self._rnm_valid) > 0
        return dict(super()._extra_state(epoch), record_norm_mean=float(self.record_norm_mean) if valid else None)

    def _state_tensors(self):
        return super()._state_tensors() + [self.record_norm_mean, self._rnm_valid]

    # ------------------------------------------------------------------------------
    def _host_prelude(self, epoch: int, it: int, iters: int):
        super()._host_prelude(epoch, it, iters)
        opt = self.opt
        if opt.sec or opt.l2reg:
            now_iter = (epoch - 1) * iters + it
            self._ramp_t.fill_(now_iter / (opt.epochs * iters))

    def _step_body(self, idx: torch.Tensor, epoch: int = 1, it: int = 0):
        """Device work of one step: no host syncs, no host-dependent control flow
        (capturable into a hipGraph)."""
        opt = self.opt
        mb = getattr(opt, "micro_batch", 0) or 0
        if 0 < mb < 2 * idx.numel():
            return self._step_body_gradcache(idx, epoch, it, mb)
        ph = self.prof.phase
        with ph("augment"):
            zeroed, x = self._start_step(idx, epoch, it)
            # (SimCLR ignores labels: no gather kernel in its step)
            labels = self.train.labels[idx] if opt.method == "SupCon" else None
        with ph("forward"):
            feats = self.runner.forward(x)
        with ph("loss"):
            loss = self.criterion(feats, labels if opt.method == "SupCon" else None)
            stats = self._norm_terms(feats)
            extra = stats.pop("extra_loss")
            if extra is not None:
                loss = loss + extra
        self._backward_and_update(loss, zeroed)
        stats["loss_local"] = loss.detach()
        return stats

    def _step_body_gradcache(self, idx: torch.Tensor, epoch: int, it: int, mb: int):
        """Gradient-cache step for contrastive batches larger than one encoder pass fits in
        HBM (e.g. BS 4096 at 224x224, BASELINE config 5): (1) encode all views in chunks of
        ``mb`` without autograd, (2) contrastive loss + norm terms on the full feature set,
        backward to the features only, (3) re-encode each chunk with autograd and backprop
        its slice of the feature gradient. Activation memory is one chunk's; the loss and
        its gradient are those of the full batch. BatchNorm statistics are per chunk (as
        in any micro-batched BN network); running statistics are updated once per chunk
        in the re-encode pass only. The update is therefore the EXACT gradient of the
        full-batch loss of the same network with ghost batch norm of ``mb`` views — not the
        reference's full-batch BN (tests/test_gradcache.py pins this equivalence); for
        full-batch BN semantics run the whole local batch in one pass (288 GB of HBM holds
        the config-5 batch: profiles/cfg5_slice_r2.json). The bucket reducer stays paused
        until the last chunk.
        """
        opt = self.opt
        ph = self.prof.phase
        with ph("augment"):
            x = self.make_views(idx, epoch, it)
            labels = self.train.labels[idx]
        chunks = list(torch.split(x, mb))
        bns = [m for m in self.model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
        saved = [(m.running_mean.clone(), m.running_var.clone(), m.num_batches_tracked.clone())
                 for m in bns if m.running_mean is not None]
        pend = self.runner._nbt_pending
        with ph("forward"), torch.no_grad():
            feats = torch.cat([self.runner.forward(c) for c in chunks])
        with torch.no_grad():          # undo the statistics updates of the no-grad pass
            for m, (rm, rv, nb) in zip([m for m in bns if m.running_mean is not None], saved):
                m.running_mean.copy_(rm)
                m.running_var.copy_(rv)
                m.num_batches_tracked.copy_(nb)
        self.runner._nbt_pending = pend
        feats = feats.detach().requires_grad_(True)
        with ph("loss"):
            loss = self.criterion(feats, labels if opt.method == "SupCon" else None)
            stats = self._norm_terms(feats)
            extra = stats.pop("extra_loss")
            if extra is not None:
                loss = loss + extra
            loss.backward()
        gfeat = feats.grad
        self.optimizer.zero_grad()
        with ph("backward"):
            off = 0
            for i, c in enumerate(chunks):
                n = c.shape[0]
                last = i == len(chunks) - 1
                ctx = self.reducer.no_sync() if (self.reducer is not None and not last) else contextlib.nullcontext()
                with ctx:
                    f = self.runner.forward(c)
                    f.backward(gfeat[off:off + n].to(f.dtype))
                off += n
        self._reduce_and_update()
        stats["loss_local"] = loss.detach()
        return stats

    def train_step(self, idx: torch.Tensor, epoch: int, it: int, iters: int):
        maybe_inject(self.rank, self.global_step)
        return super().train_step(idx, epoch, it, iters)

    def _step(self, idx, epoch, it):
        if self._graph is None:
            return self._step_body(idx, epoch, it)
        self._idx_buf.copy_(idx, non_blocking=True)
        self._graph.replay()
        self.runner._nbt_pending += self._graph_nbt
        return self._graph_stats

    def enable_cuda_graph(self, idx_example: torch.Tensor, warmup: int = 2) -> bool:
        """Capture the whole training step (aug → fwd → loss → bwd → SGD) in one hipGraph.

        Single-process only (the data-parallel path keeps eager launches; an emulated SyncBN
        group — SDX_SYNCBN_EMU — is captured too: the fused exchange takes its epoch from
        device-side counters, so every replay advances it, bn.hip xg_exchange). Capture needs
        warm-up steps run on a side stream; they execute real updates, so the training
        state they touch (parameters, optimizer buffers, BN running statistics, the norm
        EMA) is snapshotted first and restored after the capture — a graphed run follows
        exactly the eager trajectory."""
        if self.device.type != "cuda" or self.world > 1 or self.backend != "native":
            return False
        self._idx_buf = idx_example.clone()
        self._seed_dev = True
        with self._training_state_kept():
            self._host_prelude(1, 0, 1)
            # The step is captured as ONE chain: the weight gradients run in line on the capture
            # stream instead of forking to the wgrad side stream (SDX_GRAPH_SIDE=1 keeps the
            # fork). A captured two-stream DAG replays its branches on several hardware queues
            # with a cross-queue wait at every fork: 24.9 vs 11.9 ms eager at 256 images/GPU
            # (23.5 ms even with per-node priorities), while each kernel replayed on its own runs
            # at its eager speed (profiles/graph_probe_r6.txt, profiles/graph_ab_r6.txt).
            # In line, the dedicated wgrad kernels get the whole chip (their eager block target
            # keeps half of it for the concurrent critical path): SDX_GRAPH_WGRAD_BLOCKS, 256.
            from ..ops import streams
            side_prev = streams.ENABLED
            streams.ENABLED = os.environ.get("SDX_GRAPH_SIDE", "0") == "1"
            m = _ext.require()
            tgt_prev = m.wgrad_block_target_set(int(os.environ.get("SDX_GRAPH_WGRAD_BLOCKS", "256"))) \
                if not streams.ENABLED else None
            try:
                s = torch.cuda.Stream(device=self.device)
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    for _ in range(warmup):
                        self._step_body(self._idx_buf)
                torch.cuda.current_stream().wait_stream(s)
                g = torch.cuda.CUDAGraph()
                p0 = self.runner._nbt_pending
                # thread-local capture: the communicator watchdog thread (csrc/bindings/comm_ops.cpp)
                # keeps polling its events while this thread captures
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self._graph_stats = self._step_body(self._idx_buf)
            finally:
                streams.ENABLED = side_prev
                if tgt_prev is not None:
                    m.wgrad_block_target_set(tgt_prev)
            # BN passes of one step, counted on the host (ModelRunner.flush_bn_counters) per replay
            self._graph_nbt = self.runner._nbt_pending - p0
            self._graph = g
        return True

    def _norm_terms(self, feats):
        """SEC / L2-reg regularisers on un-normalised global features (main_supcon.py:295-317).
        The EMA ``record_norm_mean`` and the ramp live in device tensors."""
        opt = self.opt
        if not (opt.sec or opt.l2reg) and feats.is_cuda and feats.dim() == 2 and _ext.available():
            return self._norm_stats_native(feats)
        norms = feats.float().norm(dim=1)
        n_global = norms.numel() * self.world
        local = torch.stack([norms.sum(), (norms * norms).sum()])
        need_global = opt.sec or opt.l2reg
        if need_global and self.world > 1:
            g = local.detach().clone()
            comm.all_reduce_sum_(g)
        else:
            g = local.detach() * (self.world if self.world > 1 else 1)
        norm_mean = g[0] / n_global
        norm_var = g[1] / n_global - norm_mean * norm_mean
        m = opt.norm_momentum
        rec = self.record_norm_mean
        rec.copy_(torch.where(self._rnm_valid > 0, (1 - m) * rec + m * norm_mean, norm_mean))
        self._rnm_valid.fill_(1.0)
        extra = torch.zeros((), device=feats.device)
        loss_sec = ((norms - rec) ** 2).sum() / n_global
        loss_l2 = (norms ** 2).sum() / n_global
        if opt.sec:
            extra = extra + opt.sec_wei * self._ramp_t * loss_sec
        if opt.l2reg:
            extra = extra + opt.l2reg_wei * self._ramp_t * loss_l2
        return {"extra_loss": extra, "norm_mean": norm_mean.detach(), "norm_var": norm_var.detach(),
                "loss_sec": loss_sec.detach(), "loss_l2reg": loss_l2.detach(),
                "record_norm_mean": rec.detach().clone()}

    def _norm_stats_native(self, feats):
        """Logging-only norm statistics (no SEC / L2-reg term in the loss): one launch
        (csrc/kernels/featnorm.hip) computes them and advances the record_norm_mean EMA.
        Same semantics as the torch path: global sums are estimated as local·W (no
        collective) when no regulariser needs the exact global statistics."""
        from ..ops.streams import SideWork
        m = _ext.require()
        x = feats.detach().float().contiguous()
        n_global = float(x.shape[0] * self.world)
        mom = float(self.opt.norm_momentum)
        sums = self._ns_sums
        if sums is None or sums.device != x.device:
            sums = self._ns_sums = torch.zeros(2, dtype=torch.float64, device=x.device)
        # nothing in the step reads these: on the wgrad side stream (idle here), off the loss
        # -> backward path; the end-of-backward join orders every later reader behind them
        with (SideWork(x) if _NORM_SIDE else contextlib.nullcontext()):
            if self.world > 1:
                m.norm_stats(x, 0, sums, n_global, mom, self.record_norm_mean, self._rnm_valid)
                sums.mul_(float(self.world))
                out = m.norm_stats(x, 2, sums, n_global, mom, self.record_norm_mean, self._rnm_valid)
            else:
                out = m.norm_stats(x, 1, sums, n_global, mom, self.record_norm_mean, self._rnm_valid)
        return {"extra_loss": None, "norm_mean": out[0], "norm_var": out[1], "loss_sec": out[3],
                "loss_l2reg": out[4], "record_norm_mean": out[2]}

    # ------------------------------------------------------------------------------
    def train_epoch(self, epoch: int) -> float:
        opt = self.opt
        self.model.train()
        self.sampler.set_epoch(epoch)
        iters = len(self.sampler)
        if opt.max_steps:
            iters = min(iters, opt.max_steps)
        batch_time, data_time, losses = AverageMeter(), AverageMeter(), AverageMeter()
        loss_acc = torch.zeros((), device=self.device)
        window_loss = torch.zeros((), device=self.device)
        window_n = 0
        end = time.time()
        t_window = time.time()
        for it, idx in enumerate(self.sampler.batches(self.device)):
            if it >= iters:
                break
            if self._syncbn_pending:
                # --syncbn_comm auto: measure the transports on this batch (state restored)
                self.autotune_syncbn(idx)
            data_time.update(time.time() - end)
            if opt.cuda_graph and self._graph is None and not self._graph_failed:
                try:
                    ok = self.enable_cuda_graph(idx)
                    logging.info("hipGraph capture of the train step: " + ("enabled" if ok else "not applicable"))
                except Exception as e:  # noqa: BLE001
                    self._graph_failed = True
                    logging.warning(f"hipGraph capture failed, running eagerly: {e!r}")
            st = self.train_step(idx, epoch, it, iters)
            loss_acc += st["loss_local"]
            window_loss += st["loss_local"]
            window_n += 1
            batch_time.update(time.time() - end)
            end = time.time()
            if (it + 1) % opt.print_freq == 0 or it + 1 == iters:
                vals = torch.stack([window_loss, st["norm_mean"], st["record_norm_mean"], st["norm_var"],
                                    st["loss_sec"], st["loss_l2reg"], st["loss_local"]])
                vals[0] = vals[0] / max(window_n, 1)
                if self.world > 1:
                    red = vals[[0, 6]].clone()
                    comm.all_reduce_sum_(red)
                    vals[0], vals[6] = red[0], red[1]
                v = vals.tolist()    # one host sync per print window
                if self.device.type == "cuda":
                    torch.cuda.synchronize()
                dt = (time.time() - t_window) / window_n
                t_window = time.time()
                losses.update(v[0], window_n)
                losses.val = v[6]
                batch_time.val = dt
                if self.rank == 0:
                    now_iter = (epoch - 1) * iters + it
                    for tag, k in (("info/norm_mean", 1), ("info/norm_var", 3), ("info/record_norm_mean", 2),
                                   ("info/loss_sec", 4), ("info/loss_l2reg", 5)):
                        self.logger.log_value(tag, v[k], now_iter)
                    logging.info(
                        "Train: [{0}][{1}/{2}]\tBT {bt:.3f} ({bta:.3f})\tDT {dtv:.3f} ({dta:.3f})\t"
                        "loss {lv:.3f} ({la:.3f})\tnorm_mean {nm:.3f} (record: {rec:.3f}) var {var:.3f}\t"
                        "img/s {ips:.0f}".format(
                            epoch, it + 1, iters, bt=dt, bta=batch_time.avg, dtv=data_time.val, dta=data_time.avg,
                            lv=v[6], la=losses.avg, nm=v[1], rec=v[2], var=v[3],
                            ips=opt.batch_size / max(dt, 1e-9)))
                    if self.prof.enabled:
                        logging.info("phases (ms/step): " + PhaseTimer.format(self.prof.summary()))
                    sys.stdout.flush()
                window_loss = torch.zeros((), device=self.device)
                window_n = 0
        # BN num_batches_tracked is host-counted on the native path: visible in the buffers
        # from every epoch end on, not only through state_dict()
        self.runner.flush_bn_counters()
        return losses.avg

    def _epoch(self, epoch: int) -> dict:
        t1 = time.time()
        loss = self.train_epoch(epoch)
        logging.info("epoch {}, total time {:.2f}".format(epoch, time.time() - t1))
        return {"loss": loss}

    def _evaluate(self, epoch: int) -> dict:
        if self.knn is not None and (epoch % self.opt.knn_freq == 0 or epoch == self.opt.epochs):
            self.knn_eval(epoch)
        return {}
