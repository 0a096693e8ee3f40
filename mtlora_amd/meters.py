"""Device-side training meters: the reference's ``AverageMeter`` set of the train loop (main.py:318-321, 354-401) kept in device
memory, updated by ONE launch inside the train step (csrc/meter.hip) and read back once per ``PRINT_FREQ`` without a stall.

The reference reads back, every step, the loss scale (``loss_scaler.state_dict()["scale"]``), ``loss.item()``, the gradient norm,
every task's ``loss.item()`` and ``param_groups[0]["lr"]``: 2 + T host synchronisations in front of a step whose point, once it is
replayed from a graph, is that the host runs ahead.  Each of those values already sits at a fixed device address after a step;
``TrainMeters`` is a bank of ``AverageMeter`` slots that read them there.

    meters = TrainMeters.for_train_step(criterion.tasks, optimizer, loss_scaler, accumulation_steps=k)
    step = GraphedTrainStep(model, criterion, optimizer, images, targets, ..., meters=meters)   # or train_step(..., meters=meters)
    for idx, batch in enumerate(loader):
        ...; step()
        if idx % PRINT_FREQ == 0:
            meters.snapshot()                      # one async copy into pinned memory + an event
            m = meters.latest()                    # the newest snapshot that has ARRIVED (never synchronises): maybe the last one
            if m: print(m["loss"].val, m["loss"].avg, m["grad_norm"].avg, m["loss_scale"].val, m["lr"].val)
    meters.snapshot(); epoch = meters.latest(wait=True); meters.reset()

One deliberate difference from ``AverageMeter``: a value that is inf or nan becomes ``val`` and bumps ``skipped`` but enters neither
``sum`` nor ``count``.  Under the fp16 recipe a step overflows whenever the scale has grown too far; the scaler skips that step,
and one such step must not turn the epoch's average into inf.

``update_torch`` is the definition (fp64 arithmetic with torch operations, any device; the CPU path); ``update`` on a GPU is the
kernel, held to it bit for bit by tests/test_gpu_meters.py.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence

import torch

from . import _lib

WORDS = 4  # val, sum, count, skipped
VAL, SUM, COUNT, SKIPPED = range(WORDS)


class Meter(NamedTuple):
    """one slot as ``latest()`` returns it: ``AverageMeter``'s fields plus the number of non-finite values left out"""
    val: float
    avg: float
    sum: float
    count: float
    skipped: int


class TrainMeters:
    """a bank of at most 64 ``AverageMeter`` slots in device memory, each bound to a 0-d / 1-element fp32 or fp64 device tensor.

    ``add(name, tensor, n=1, period=1)`` binds a slot (``n``: ``AverageMeter.update``'s weight; ``period`` k: the slot is served at
    every k-th ``update`` only), ``seal()`` uploads the source table once, ``update()`` is one launch on the current stream (graph-
    capturable: every address is fixed from ``seal`` on), ``snapshot()`` / ``latest()`` read back, ``reset()`` starts a new epoch.
    The bound tensors are kept alive here; re-allocating one after ``seal`` is the caller's error, as for any captured address."""

    MAX_SLOTS = _lib.METER_MAX_SLOTS

    def __init__(self, device):
        self.device = torch.device(device)
        self.names: List[str] = []
        self.tasks: List[str] = []  # (for_train_step: the order of the staged per-task losses)
        self._src: List[torch.Tensor] = []
        self._n: List[float] = []
        self._period: List[int] = []
        self._staged: Dict[str, torch.Tensor] = {}  # slots whose source this object owns (stage())
        self._stage_buf: Optional[torch.Tensor] = None
        self._stage_names: List[str] = []
        self._sealed = False
        self._state: Optional[torch.Tensor] = None  # int64 words: the bank's 4 M doubles, then the counter
        self._table: Optional[torch.Tensor] = None
        self._pinned: List[Optional[torch.Tensor]] = [None, None]
        self._events: List[Optional["torch.cuda.Event"]] = [None, None]
        self._seq = [0, 0]  # snapshot number held by each buffer (0: none)
        self._snapshots = 0
        self._latest_seq, self._latest, self.latest_calls = 0, {}, 0

    # ---- construction -------------------------------------------------------------------------------------------------------
    def add(self, name: str, tensor: torch.Tensor, n: float = 1, period: int = 1) -> "TrainMeters":
        if self._sealed:
            raise RuntimeError("mtlora_amd: TrainMeters.add() after seal(): the source table is already on the device")
        if not isinstance(tensor, torch.Tensor) or tensor.numel() != 1:
            raise TypeError(f"mtlora_amd: meter {name!r} needs a 0-d or 1-element tensor, got "
                            f"{tuple(tensor.shape) if isinstance(tensor, torch.Tensor) else type(tensor).__name__}")
        if tensor.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"mtlora_amd: meter {name!r} needs an fp32 or fp64 tensor, got {tensor.dtype}")
        if tensor.device != self.device:
            raise TypeError(f"mtlora_amd: meter {name!r} lives on {tensor.device}, the bank on {self.device}")
        if isinstance(period, bool) or int(period) != period or period < 1:
            raise ValueError(f"mtlora_amd: meter {name!r}: period must be an integer >= 1, got {period!r}")
        if not float(n) > 0.0:
            raise ValueError(f"mtlora_amd: meter {name!r}: n must be positive, got {n!r}")
        if name in self.names:
            raise ValueError(f"mtlora_amd: meter {name!r} exists already")
        if len(self.names) >= self.MAX_SLOTS:
            raise ValueError(f"mtlora_amd: a TrainMeters bank holds at most {self.MAX_SLOTS} slots")
        self.names.append(name)
        self._src.append(tensor.detach())
        self._n.append(float(n))
        self._period.append(int(period))
        return self

    def add_staged(self, names: Sequence[str], n: float = 1, periods: Optional[Sequence[int]] = None) -> "TrainMeters":
        """slots whose sources are elements of ONE fp32 buffer owned by the bank: ``stage(values)`` writes them all with one small
        kernel (values that live at a new address every step, such as an eager step's loss)"""
        if self._stage_buf is not None:
            raise RuntimeError("mtlora_amd: TrainMeters.add_staged() was called already")
        buf = torch.zeros(len(names), dtype=torch.float32, device=self.device)
        for i, name in enumerate(names):
            self.add(name, buf[i], n, 1 if periods is None else periods[i])
            self._staged[name] = buf[i]
        self._stage_buf, self._stage_names = buf, list(names)
        return self

    @torch.no_grad()
    def stage(self, values: Sequence[torch.Tensor]) -> None:
        """write the first ``len(values)`` staged sources (in ``add_staged`` order) from 0-d device tensors: one device-to-device
        gather kernel (``torch.stack`` into the buffer), no host value, no memset"""
        if self._stage_buf is None or not 0 < len(values) <= len(self._stage_names):
            raise RuntimeError("mtlora_amd: TrainMeters.stage() needs 1 .. len(add_staged names) values")
        torch.stack([v.detach().reshape(()).to(torch.float32) for v in values], out=self._stage_buf[:len(values)])

    def seal(self) -> "TrainMeters":
        """allocate the bank and upload the source table (once); from here on every address the update reads or writes is fixed"""
        if self._sealed:
            return self
        if not self.names:
            raise RuntimeError("mtlora_amd: TrainMeters.seal() without a slot")
        M = len(self.names)
        self._state = torch.zeros(WORDS * M + 1, dtype=torch.int64, device=self.device)
        self._n_t = torch.tensor(self._n, dtype=torch.float64, device=self.device)
        self._period_t = torch.tensor(self._period, dtype=torch.int64, device=self.device)
        if self.device.type == "cuda":
            _lib.require_gpu(self._state)
            recs = (_lib.MeterSource * M)()
            for i, (t, n, k) in enumerate(zip(self._src, self._n, self._period)):
                recs[i].src, recs[i].dtype = t.data_ptr(), (_lib.METER_F64 if t.dtype == torch.float64 else _lib.METER_F32)
                recs[i].weight, recs[i].period = n, k
            host = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.int64).clone()
            self._table = host.to(self.device)  # (a synchronous copy: the table is complete before the first update)
            for b in range(2):
                self._pinned[b] = torch.zeros(WORDS * M + 1, dtype=torch.int64, pin_memory=True)
        else:
            for b in range(2):
                self._pinned[b] = torch.zeros(WORDS * M + 1, dtype=torch.int64)
        self._sealed = True
        return self

    def _need_sealed(self) -> None:
        if not self._sealed:
            raise RuntimeError("mtlora_amd: TrainMeters is not sealed (seal() after the last add())")

    # ---- views of the device state (no synchronisation) ---------------------------------------------------------------------
    @property
    def bank(self) -> torch.Tensor:
        """(M, 4) fp64 view of the device bank: val, sum, count, skipped"""
        self._need_sealed()
        return self._state[:-1].view(torch.float64).view(len(self.names), WORDS)

    @property
    def counter(self) -> torch.Tensor:
        """0-d int64 view of the device call counter"""
        self._need_sealed()
        return self._state[-1]

    # ---- the update ---------------------------------------------------------------------------------------------------------
    def update(self) -> None:
        """one call of every slot's ``AverageMeter.update`` (slots off their period are left alone): ONE launch on the current
        stream, nothing allocated or synchronised.  On a CPU bank this is ``update_torch``."""
        self._need_sealed()
        if self.device.type != "cuda":
            return self.update_torch()
        _lib.require_gpu(self._state)
        base = self._state.data_ptr()
        _lib.check(_lib.lib().mtlora_meter_update(base, self._table.data_ptr(), len(self.names), base + 8 * WORDS * len(self.names),
                                                  _lib.stream_ptr()), "meter_update")

    @torch.no_grad()
    def update_torch(self) -> None:
        """the definition of ``update``: the same arithmetic in fp64 with torch operations, on any device.  With c1 = counter + 1,
        a slot with c1 % period == 0 reads v: finite -> val = v, sum = sum + v * n, count = count + n; not finite -> val = v,
        skipped = skipped + 1; then counter = c1."""
        self._need_sealed()
        bank, c1 = self.bank, self.counter + 1
        v = torch.stack([t.reshape(()).to(torch.float64) for t in self._src])
        due = (c1 % self._period_t) == 0
        good = due & torch.isfinite(v)
        bad = due & ~torch.isfinite(v)
        new = torch.stack([torch.where(due, v, bank[:, VAL]),
                           torch.where(good, bank[:, SUM] + v * self._n_t, bank[:, SUM]),
                           torch.where(good, bank[:, COUNT] + self._n_t, bank[:, COUNT]),
                           torch.where(bad, bank[:, SKIPPED] + 1.0, bank[:, SKIPPED])], dim=1)
        bank.copy_(new)
        self.counter.copy_(c1)

    def reset(self, keep_phase: bool = True) -> None:
        """zero every slot: the reference's per-epoch re-creation of its ``AverageMeter``s.  ``keep_phase=True`` keeps the call
        counter, so a slot with a period stays in step with whatever it follows (an accumulation cycle); ``keep_phase=False``
        zeroes the counter as well.  One launch (a zero-fill kernel, never a memset); earlier snapshots stay readable."""
        self._need_sealed()
        if self.device.type != "cuda":
            (self._state[:-1] if keep_phase else self._state).zero_()
            return
        _lib.require_gpu(self._state)
        base = self._state.data_ptr()
        _lib.check(_lib.lib().mtlora_meter_reset(base, len(self.names), base + 8 * WORDS * len(self.names), int(bool(keep_phase)),
                                                 _lib.stream_ptr()), "meter_reset")

    # ---- reading back -------------------------------------------------------------------------------------------------------
    def snapshot(self) -> None:
        """enqueue ONE asynchronous copy of the bank and the counter into pinned host memory on the current stream and record an
        event behind it.  Two pinned buffers take turns, so the snapshot before this one stays readable while this one is in flight."""
        self._need_sealed()
        self._snapshots += 1
        b = self._snapshots & 1
        if self.device.type == "cuda":
            self._pinned[b].copy_(self._state, non_blocking=True)
            if self._events[b] is None:
                self._events[b] = torch.cuda.Event()
            self._events[b].record()
        else:
            self._pinned[b].copy_(self._state)
        self._seq[b] = self._snapshots

    def latest(self, wait: bool = False) -> Dict[str, Meter]:
        """``{name: Meter(val, avg, sum, count, skipped)}`` of the most recent snapshot whose copy has completed (``avg`` = sum /
        count, 0 while count is 0); ``{}`` before any has.  Never synchronises -- the events are only queried -- unless ``wait``:
        then the newest snapshot's event is waited for.  ``self.latest_calls`` is that snapshot's call counter."""
        self._need_sealed()
        for b in sorted(range(2), key=lambda i: -self._seq[i]):
            seq = self._seq[b]
            if seq <= self._latest_seq:
                break  # nothing newer than what was parsed before
            ev = self._events[b]
            if ev is not None:
                if wait:
                    ev.synchronize()
                elif not ev.query():
                    continue
            host = self._pinned[b]
            vals = host[:-1].view(torch.float64).tolist()
            self.latest_calls = int(host[-1])
            self._latest = {}
            for i, name in enumerate(self.names):
                val, s, cnt, skipped = vals[WORDS * i:WORDS * i + WORDS]
                self._latest[name] = Meter(val, s / cnt if cnt else 0.0, s, cnt, int(skipped))
            self._latest_seq = seq
            break
        return dict(self._latest)

    # ---- the train step's set -----------------------------------------------------------------------------------------------
    @classmethod
    def for_train_step(cls, criterion_tasks: Sequence[str], optimizer, loss_scaler=None, accumulation_steps: int = 1,
                       device=None) -> "TrainMeters":
        """the reference loop's meters under its names: ``loss``, ``tasks/<t>/loss``, ``grad_norm`` (period ``accumulation_steps``:
        the reference meters the norm on update steps only, main.py:363), ``loss_scale`` (with a ``loss_scaler``: the scaler's own
        device word) and ``lr`` (with a schedule attached to the optimizer: ``lr_used()[0]``, what the kernels used -- not
        ``param_groups``; attach it -- ``optimizer.attach_schedule(scheduler)`` -- before this call, ``GraphedTrainStep(lr_scheduler=)``
        attaching the same scheduler again changes nothing).  Loss, task losses and norm are staged sources: ``train_step`` / ``GraphedTrainStep`` write them with
        ``stage()`` and call ``update()``.  Sealed on return."""
        from .optim import accumulation_steps_of
        k = accumulation_steps_of(accumulation_steps)
        if device is None:
            device = optimizer.param_groups[0]["params"][0].device
        m = cls(device)
        tasks = list(criterion_tasks)
        m.tasks = tasks
        m.add_staged(["loss"] + [f"tasks/{t}/loss" for t in tasks] + ["grad_norm"], periods=[1] * (1 + len(tasks)) + [k])
        if loss_scaler is not None:
            loss_scaler._lazy_init(m.device)
            m.add("loss_scale", loss_scaler._scale)
        if getattr(optimizer, "_sched", None) is not None:
            m.add("lr", optimizer.lr_used()[0])
        return m.seal()

    def stage_train_step(self, loss: torch.Tensor, per: Dict[str, torch.Tensor], norm: Optional[torch.Tensor]) -> None:
        """what the harness calls at the end of a step: loss, the per-task losses and (on an update step) the gradient norm into
        the staged sources, then ``update()``"""
        vals = [loss] + [per[t] for t in self.tasks]
        if norm is not None:
            vals.append(norm)
        self.stage(vals)
        self.update()


for_train_step = TrainMeters.for_train_step
