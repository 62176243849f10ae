"""What the flat-buffer trainers share: :class:`TrainEngine`, the base of ``PretrainEngine``
(engine/pretrain.py) and ``SupervisedEngine`` (engine/supervised.py).

The base owns the process set-up (process group, priority stream, logging, seed, backend), the
SyncBN statistics transports, the flat parameter buffer with its optimizer, reducer and model
runner, the step / seed state, the augmentation call, the tail of a step (gradient zeroing,
backward, gradient reduction, update), checkpoint resume and the epoch loop of ``run()``.
A subclass supplies the model, the data and sampler, the loss part of ``_step_body``,
``train_epoch`` and what it logs per epoch.
"""
from __future__ import annotations

import contextlib
import logging
import os
import time
from typing import Optional

import torch
import torch.distributed as dist

from ..data.augment import nhwc8_to_nchw
from ..models.executor import ModelRunner
from ..ops import _ext
from ..optim.flat import FlatParams, build_optimizer
from ..optim.schedules import adjust_learning_rate, warmup_learning_rate
from ..parallel import comm
from ..parallel.ddp import GradBucketReducer
from ..utils.logging import setup_logging
from ..utils.profiling import PhaseTimer
from . import checkpoint as ckpt_mod

_ZERO_SIDE = os.environ.get("SDX_ZERO_SIDE", "1") != "0"


def resolve_backend(requested: str, device: torch.device, stem: str = "cifar") -> str:
    if requested == "torch":
        return "torch"
    native_ok = device.type == "cuda" and _ext.available()
    if requested == "native":
        if not native_ok:
            _ext.require()
            raise RuntimeError("native backend needs a GPU")
        return "native"
    return "native" if native_ok else "torch"


def step_seed(base: int, epoch: int, idx: int, rank: int) -> int:
    return (base * 1000003 + epoch * 100003 + idx * 17 + rank * 7919) & ((1 << 62) - 1)


_PRIO_STREAMS = {}


def _priority_stream(dev: torch.device) -> torch.cuda.Stream:
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    st = _PRIO_STREAMS.get(key)
    if st is None:
        st = _PRIO_STREAMS[key] = torch.cuda.Stream(device=dev, priority=-1)
    return st


class TrainEngine:
    # a subclass whose model depends on its data (the class count) loads the data first
    data_first = False

    def __init__(self, opt, device: Optional[torch.device] = None):
        self.opt = opt
        rank, local_rank, world, dev = comm.init_distributed(opt.dist_backend, getattr(opt, "comm_timeout", 600.0), device=device)
        self.rank, self.world, self.device = rank, world, dev
        self.stream = None
        if dev.type == "cuda" and os.environ.get("SDX_STREAM_PRIO", "1") != "0":
            # the whole step on a high-priority stream: the critical path (forward, BN,
            # dgrad chain) is dispatched ahead of the default-priority wgrad side stream.
            # 12.52 -> 12.43 ms/step same box, 4 alternating rounds (profiles/knob_sweep_r3.txt).
            # One stream per device and process, shared by every engine built in it.
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

        if self.data_first:
            self._build_data()
        model = self._build_model()
        # SyncBN statistics transport actually in use (bench.py reports it): none (W=1),
        # xgmi-fused, rccl-native, process-group (c10d collectives), emulated-W
        self.syncbn_transport = "none"
        self.syncbn_tune: Optional[dict] = None
        self._syncbn_cands: dict = {}
        self._syncbn_pending = False
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
        self._setup_more_comm(opt, dev)
        model = model.to(dev)
        if dev.type == "cuda":
            model = model.to(memory_format=torch.channels_last)
        self.model = model
        self.flat = FlatParams(model)
        self.optimizer = build_optimizer(opt.optimizer, self.flat, opt.learning_rate, opt.momentum,
                                         opt.weight_decay, backend="torch" if self.backend == "torch" else "auto")
        early = self._early_step()
        self.reducer = (GradBucketReducer(self.flat, early_step=early, compress=getattr(opt, "grad_compress", "none"))
                        if (world > 1 or early is not None) else None)
        self.optimizer.grad_scale = self._grad_scale()
        self.runner = ModelRunner(model, self.backend, opt.precision, self.sync_group, master=self.flat.flat)
        if not self.data_first:
            self._build_data()
        self.logger = None
        if rank == 0:
            from ..utils.tb import Logger
            self.logger = Logger(opt.tb_folder, flush_secs=2)
        self.start_epoch = 1
        self.global_step = 0
        self._seed_t = torch.zeros((1,), dtype=torch.int64, device=dev)
        self._seed_host = 0
        self._seed_dev = False     # True once a hipGraph of the step exists (the seed then lives in _seed_t)
        self._one_grad = None      # the persistent seed gradient of backward
        self._zg_ev = None         # the event behind the side-stream gradient zeroing
        self._cpu_store = None     # --gpu_aug 0: the host copy of the training store
        self.prof = PhaseTimer(getattr(opt, "profile", False), dev)
        self._init_state()
        if getattr(opt, "resume", ""):
            self._resume(opt.resume)

    # ---- what a subclass supplies ---------------------------------------------------
    def _build_model(self) -> torch.nn.Module:
        """The model on the host (its construction draws the initial weights), --ckpt loaded."""
        raise NotImplementedError

    def _build_data(self):
        """Set ``self.train`` (a DeviceStore), ``self.sampler`` and ``self.aug``."""
        raise NotImplementedError

    def _setup_more_comm(self, opt, dev):
        """Communicators besides the SyncBN transport, set up right after it."""

    def _early_step(self):
        """The per-bucket update the reducer runs as soon as a bucket is final, or None."""
        return None

    def _grad_scale(self) -> float:
        """The optimizer's factor on the ranks' gradient sum: 1/W, the mean of the local-batch means (DDP)."""
        return 1.0 / self.world

    def _init_state(self):
        """The subclass's own state, created before a --resume checkpoint is read."""

    def _epoch(self, epoch: int) -> dict:
        """Train epoch ``epoch``; returns the {tag: value} run() logs for it (rank 0)."""
        raise NotImplementedError

    def _evaluate(self, epoch: int) -> dict:
        """What follows an epoch's training; returns further {tag: value} to log."""
        return {}

    def _end_of_run(self):
        """After the last epoch, before the last checkpoint is written."""

    # ---- SyncBN statistics transport ------------------------------------------------
    def _setup_syncbn_comm(self, opt, dev):
        """SyncBN statistics transport for the native backend (SURVEY §2.3 X4/X6, §5.8;
        reference: main_supcon.py:222-224 converts the model to SyncBatchNorm).

        Candidates, each registered as a native handle so the C++ block executor exchanges
        each BN's sums itself on the compute stream:

        * ``xgmi-fused``: the one-shot IPC arena whose FUSED path reduces, exchanges and
          finalizes a BN's statistics in ONE launch (parallel/xgmi.py); all ranks must be
          peers on one node.
        * ``rccl-native``: a dedicated RCCL communicator (reduce -> ncclAllReduce ->
          finalize per BN).
        * ``process-group``: no native handle; the Python collective path (gloo runs).

        ``--syncbn_comm auto`` (default) sets up every candidate the job can have and MEASURES
        them on the first training batch (:meth:`autotune_syncbn`): all ranks agree on the
        fastest one (timings MAX-reduced over ranks, so the choice is identical everywhere).
        ``xgmi`` / ``rccl`` force one (RCCL is the fallback of both when the arena's self-check
        fails)."""
        want = getattr(opt, "syncbn_comm", "auto")
        self._syncbn_cands = {}
        if dev.type != "cuda":
            return
        timeout = float(getattr(opt, "comm_timeout", 600.0))
        if want in ("xgmi", "auto"):
            # set-up is agreed step by step across ranks (parallel/xgmi.py): either every
            # rank gets the arena or every rank raises here and falls back together
            try:
                from ..parallel.xgmi import OneShotAllReduce
                impl = OneShotAllReduce(timeout_s=timeout)
                self._xgmi = impl
                self._syncbn_cands["xgmi-fused"] = (impl.handle, impl)
            except Exception as e:  # noqa: BLE001
                (logging.warning if want == "xgmi" else logging.info)(
                    f"one-shot xGMI exchange unavailable ({e}); using RCCL")
        if (want == "auto" or not self._syncbn_cands) and comm.backend() == "nccl" \
                and os.environ.get("SDX_NATIVE_SYNCBN", "1") != "0":
            # 0 on every rank together when the dedicated communicator cannot be set up
            handle = comm.create_rccl_small_comm(None, timeout)
            if handle:
                self._syncbn_cands["rccl-native"] = (handle, None)
        if want == "auto" and comm.backend() != "nccl":
            self._syncbn_cands["process-group"] = (0, None)
        if not self._syncbn_cands:
            logging.warning("SyncBN statistics use the process-group all-reduce")
            return
        # until the measurement: RCCL when present (the conservative transport), else the first
        first = "rccl-native" if "rccl-native" in self._syncbn_cands else next(iter(self._syncbn_cands))
        self._activate_syncbn(first)
        self._syncbn_pending = want == "auto" and len(self._syncbn_cands) > 1
        logging.info(f"SyncBN statistics: {first} (candidates {list(self._syncbn_cands)})")

    def _activate_syncbn(self, name: str):
        handle, impl = self._syncbn_cands[name]
        comm.set_small_allreduce(None, impl)
        comm.set_native_small_comm(None, handle)
        self.syncbn_transport = name

    def autotune_syncbn(self, idx: torch.Tensor, steps: int = 3, baseline: bool = False) -> Optional[dict]:
        """Pick the SyncBN transport by timing real training steps on batch ``idx`` with each
        candidate (one untimed step each first). The training state the steps touch
        (parameters, optimizer and BN buffers, the norm EMA) is restored afterwards, so the
        run follows the trajectory it would have had. Every rank measures its own step
        time; the times are MAX-reduced over the ranks (the step is as slow as its slowest
        rank) and every rank takes the argmin of the SAME reduced vector, so the choice is
        identical everywhere. ``baseline``: also time the step with rank-local BN statistics
        (no exchange, timing only) to report each transport's cost per exchanged BN.
        SDX_SYNCBN_TUNE_SKEW="rank:name:ms[,...]" adds ms to a rank's measurement (tests)."""
        self._syncbn_pending = False
        names = list(self._syncbn_cands)
        if self.device.type != "cuda" or (len(names) < 2 and not baseline) or not names:
            return None
        if baseline:
            names = names + ["local-bn"]
        active = self.syncbn_transport
        group = self.runner.sync_group
        # two interleaved passes over the candidates, the faster of each candidate's two
        # timings kept: a drifting clock or a cold first candidate does not pick the transport
        ms = [float("inf")] * len(names)
        with self._training_state_kept():
            self._host_prelude(1, 0, 1)
            for _ in range(2):
                for k, nm in enumerate(names):
                    if nm == "local-bn":
                        self.runner.sync_group = None
                    else:
                        self._activate_syncbn(nm)
                    self._step_body(idx)
                    torch.cuda.synchronize()
                    comm.barrier()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        self._step_body(idx)
                    torch.cuda.synchronize()
                    comm.barrier()
                    ms[k] = min(ms[k], (time.perf_counter() - t0) / steps * 1e3)
                    self.runner.sync_group = group
        for item in filter(None, os.environ.get("SDX_SYNCBN_TUNE_SKEW", "").split(",")):
            r, nm, extra = item.split(":")
            if int(r) == self.rank and nm in names:
                ms[names.index(nm)] += float(extra)
        real = [i for i, nm in enumerate(names) if nm != "local-bn"]
        best, red = comm.agree_fastest(names, ms, eligible=real)
        self._activate_syncbn(best if best in self._syncbn_cands else active)
        n_bn = 2 * sum(1 for mod in self.model.encoder.modules() if isinstance(mod, torch.nn.BatchNorm2d))
        self.syncbn_tune = {"chosen": best, "step_ms": {nm: round(v, 3) for nm, v in zip(names, red)},
                            "exchanges_per_step": n_bn}
        if baseline:
            # (transport − local-BN step) per exchanged BN; within timing noise it can be ≤ 0
            base = red[names.index("local-bn")]
            self.syncbn_tune["us_per_bn"] = {names[i]: round((red[i] - base) * 1e3 / n_bn, 2) for i in real}
        logging.info(f"SyncBN transport measured: {self.syncbn_tune}")
        return self.syncbn_tune

    # ---- training state -------------------------------------------------------------
    def _state_tensors(self) -> list:
        """Every tensor a training step updates in place."""
        norms = getattr(self.optimizer, "norms", None)       # LARS
        return [self.flat.flat, self.optimizer.buf, *self.model.buffers()] + ([] if norms is None else [norms])

    @contextlib.contextmanager
    def _training_state_kept(self):
        """Steps run inside are real updates: snapshot the training state they touch and put it
        back on a normal exit, so the run follows the trajectory it would have had."""
        state = self._state_tensors()
        snap = [t.detach().clone() for t in state]
        pend = self.runner._nbt_pending
        yield
        with torch.no_grad():
            for t, v in zip(state, snap):
                t.copy_(v)
        self.runner._nbt_pending = pend

    def _resume(self, path):
        st = ckpt_mod.load_checkpoint(path)
        ckpt_mod.load_model_state(self.model, st["model"])
        self.optimizer.load_state_dict(st["optimizer"])
        self.start_epoch = int(st["epoch"]) + 1
        extra = st.get("sdx_state") or {}
        self.global_step = int(extra.get("global_step", 0))
        self._resume_extra(extra)
        logging.info(f"resumed from {path} at epoch {self.start_epoch}")

    def _resume_extra(self, extra: dict):
        """Take the subclass's own keys of a checkpoint's ``sdx_state``."""

    def _extra_state(self, epoch):
        return {"global_step": self.global_step, "epoch": epoch}

    # ---- one step -------------------------------------------------------------------
    def make_views(self, idx: torch.Tensor, epoch: int = 1, it: int = 0) -> torch.Tensor:
        if not getattr(self.opt, "gpu_aug", 1):
            return self._make_views_cpu(idx, epoch, it)
        if self.backend == "native":
            # eager: the seed is a kernel argument; a captured step reads it from _seed_t at replay
            return self.train.views_gpu(idx, self.aug, self._seed_host, self._seed_t if self._seed_dev else None)
        return nhwc8_to_nchw(self.train.views(idx, self.aug, step_seed(self.opt.seed, epoch, it, self.rank)))

    def _make_views_cpu(self, idx, epoch, it):
        """``--gpu_aug 0``: the torch CPU pipeline (same draws as the kernel) on a host copy
        of the dataset, ``--num_workers`` intra-op threads, then moved to the device."""
        if self._cpu_store is None:
            torch.set_num_threads(max(1, int(self.opt.num_workers)))
            self._cpu_store = self.train.to("cpu")
        x = self._cpu_store.views(idx.cpu(), self.aug, step_seed(self.opt.seed, epoch, it, self.rank))
        if self.backend == "native":
            return x.to(self.device, torch.bfloat16)
        return nhwc8_to_nchw(x).to(self.device)

    def _host_prelude(self, epoch: int, it: int, iters: int):
        """Per-step host-side scalars, written to device tensors the step body reads."""
        warmup_learning_rate(self.opt, epoch, it, iters, self.optimizer)
        self.optimizer._sync_lr()
        self._seed_host = step_seed(self.opt.seed, epoch, it, self.rank)
        if self._seed_dev:
            self._seed_t.fill_(self._seed_host)

    def _start_step(self, idx, epoch, it):
        """The head of a step: (what :meth:`_zero_grad_side` returned, the augmented views)."""
        self.runner.prefetch_weights()          # weight conversion overlaps the augmentation launch
        return self._zero_grad_side(), self.make_views(idx, epoch, it)

    def _zero_grad_side(self):
        """Zero the gradient buffer on the wgrad side stream at the start of the step (after
        the previous optimizer update), where it overlaps the forward instead of sitting on
        the compute stream before the backward (SDX_ZERO_SIDE=0: there). Returns the event
        the backward waits on, or None when it is left to the backward. The side stream's
        weight gradients are queued behind it anyway (FIFO)."""
        from ..ops import streams
        if not (_ZERO_SIDE and streams.ENABLED and self.device.type == "cuda"):
            return None
        main = torch.cuda.current_stream(self.device)
        s = streams.side(self.device)
        s.wait_stream(main)
        with torch.cuda.stream(s):
            self.optimizer.zero_grad()
        if self._zg_ev is None:
            self._zg_ev = torch.cuda.Event()
        self._zg_ev.record(s)
        return self._zg_ev

    def _backward_and_update(self, loss: torch.Tensor, zeroed):
        """The tail of a step. ``zeroed``: what :meth:`_zero_grad_side` returned at its start."""
        ph = self.prof.phase
        with ph("backward"):
            if zeroed is not None:
                torch.cuda.current_stream(self.device).wait_event(zeroed)
            else:
                self.optimizer.zero_grad()
            # a persistent seed gradient: no ones-fill kernel per step
            one = self._one_grad
            if one is None or one.device != loss.device or one.dtype != loss.dtype:
                one = self._one_grad = torch.ones((), device=loss.device, dtype=loss.dtype)
            loss.backward(one)
        self._reduce_and_update()

    def _reduce_and_update(self):
        ph = self.prof.phase
        if self.reducer is not None:
            with ph("grad_sync_wait"):
                self.reducer.finish()
        with ph("optimizer"):
            self.optimizer.step()

    def train_step(self, idx: torch.Tensor, epoch: int, it: int, iters: int):
        return self._train_step((idx,), epoch, it, iters)

    def _train_step(self, batch: tuple, epoch: int, it: int, iters: int):
        """One step on ``batch``, the leading arguments of the subclass's ``_step_body(*batch, epoch, it)``."""
        self._host_prelude(epoch, it, iters)
        st = self._step(*batch, epoch, it)
        self.global_step += 1
        return st

    def _step(self, *args):
        return self._step_body(*args)

    # ---- the run --------------------------------------------------------------------
    def _log_values(self, values: dict, epoch: int):
        if self.rank == 0:
            for tag, v in values.items():
                self.logger.log_value(tag, v, epoch)

    def _save(self, epoch: int, name: str):
        f = os.path.join(self.opt.save_folder, name)
        ckpt_mod.save_model(self.model, self.optimizer, self.opt, epoch, f, self._extra_state(epoch))

    def run(self):
        opt = self.opt
        for epoch in range(self.start_epoch, opt.epochs + 1):
            adjust_learning_rate(opt, self.optimizer, epoch)
            values = self._epoch(epoch)
            self._log_values(dict(values, learning_rate=self.optimizer.param_groups[0]["lr"]), epoch)
            self._log_values(self._evaluate(epoch), epoch)
            if epoch % opt.save_freq == 0 and self.rank == 0:
                self._save(epoch, f"ckpt_epoch_{epoch}.pth")
            comm.barrier()
        self._end_of_run()
        if self.rank == 0:
            self._save(opt.epochs, "last.pth")
            self.logger.close()
        comm.barrier()
        return os.path.join(opt.save_folder, "last.pth")
