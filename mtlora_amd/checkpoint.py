"""Checkpoint interop for the MI355X MTLoRA modules: vanilla Swin / reference MTLoRA checkpoints into
``mtlora_amd.swin_transformer_mtlora`` models, and LoRA merging for inference.

Mirrors reference ``utils.py:41-176`` (``load_checkpoint``: key mapping :125-149, ``attn_mask`` strip :60-63,
relative-position table / absolute position embedding re-interpolation :65-121) and ``models/lora.py:636-668``
(``merge_lora_weights``, ``map_old_state_dict_weights``) -- same arguments, same side effects on the state dict, same
``strict=False`` load -- so a maintainer can point the reference's ``main.py`` at it unchanged.

The other direction is here too: ``save_checkpoint`` and ``auto_resume_helper`` with the reference's signatures (utils.py:280-321),
``lora_state_dict`` / ``trainable_only=True`` for an adapter-only file, and ``TrainState``: everything a train step mutates,
enumerated once and gathered by ONE launch (csrc/snapshot.hip) into a staging buffer that one asynchronous copy moves to pinned
memory, so that a replayed loop (``mtl_harness.GraphedTrainStep``) saves between two replays without a ``state_dict()`` walk and
without waiting for the file.  Everything but ``TrainState`` is pure host code.
"""
from __future__ import annotations

import collections
import concurrent.futures
import ctypes
import logging
import os
import threading
from typing import Any, Dict, List, Mapping, MutableMapping, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .lora import MTLoRALinear, map_old_state_dict_weights
from .optim import FusedOptimizer, LossScaler

_LOG = logging.getLogger("mtlora_amd.checkpoint")


def _get(ns: Any, name: str, default=None):
    if ns is None:
        return default
    if isinstance(ns, Mapping):
        return ns.get(name, default)
    return getattr(ns, name, default)


def lora_key_mapping(model_state: Mapping[str, torch.Tensor], mtlora: Any) -> Dict[str, str]:
    """``{old key: new key}`` for the linears that the MTLoRA config turned into ``MTLoRALinear`` (their parameters live
    under ``.linear.``): reference utils.py:125-145."""
    layers: List[str] = []
    if _get(mtlora, "QKV_ENABLED"):
        layers += ["attn.qkv.weight", "attn.qkv.bias"]
    if _get(mtlora, "PROJ_ENABLED"):
        layers += ["attn.proj.weight", "attn.proj.bias"]
    if _get(mtlora, "FC1_ENABLED"):
        layers += ["mlp.fc1.weight", "mlp.fc1.bias"]
    if _get(mtlora, "FC2_ENABLED"):
        layers += ["mlp.fc2.weight", "mlp.fc2.bias"]
    if _get(mtlora, "DOWNSAMPLER_ENABLED"):
        layers += ["downsample.reduction.weight"]
    mapping = {}
    for k in model_state:
        parts = k.split(".")
        last_three, prefix = ".".join(parts[-3:]), ".".join(parts[:-3])
        if last_three in layers:
            wb = parts[-1]
            layer = ".".join(parts[-3:-1])
            mapping[f"{prefix}.{layer}.{wb}"] = f"{prefix}.{layer}.linear.{wb}"
    return mapping


def prepare_state_dict(model: nn.Module, model_state: MutableMapping[str, torch.Tensor], mtlora: Any = None,
                       update_relative_position: bool = False, skip_decoder: bool = False, split_qkv: bool = False,
                       logger: Optional[logging.Logger] = None) -> MutableMapping[str, torch.Tensor]:
    """everything reference ``load_checkpoint`` does to ``checkpoint["model"]`` before ``load_state_dict`` (in place)."""
    log = logger or _LOG
    if skip_decoder:  # utils.py:55-56
        for k in [k for k in model_state if k.startswith("decoders")]:
            del model_state[k]
    for k in [k for k in model_state if "attn_mask" in k]:  # re-initialised by the constructor (utils.py:59-62)
        del model_state[k]
    if update_relative_position:
        for pat in ("relative_position_index", "relative_coords_table"):  # utils.py:65-76
            for k in [k for k in model_state if pat in k]:
                del model_state[k]
        current = model.state_dict()
        for k in [k for k in model_state if "relative_position_bias_table" in k]:  # utils.py:78-98
            pre = model_state[k]
            if k not in current:
                continue
            L1, nH1 = pre.shape
            L2, nH2 = current[k].shape
            if nH1 != nH2:
                log.warning(f"Error in loading {k}, passing......")
            elif L1 != L2:
                S1, S2 = int(L1 ** 0.5), int(L2 ** 0.5)
                r = F.interpolate(pre.permute(1, 0).view(1, nH1, S1, S1), size=(S2, S2), mode="bicubic")
                model_state[k] = r.view(nH2, L2).permute(1, 0)
        for k in [k for k in model_state if "absolute_pos_embed" in k]:  # utils.py:100-121
            pre = model_state[k]
            if k not in current:
                continue
            _, L1, C1 = pre.shape
            _, L2, _ = current[k].shape
            if L1 != L2:
                S1, S2 = int(L1 ** 0.5), int(L2 ** 0.5)
                r = F.interpolate(pre.reshape(-1, S1, S1, C1).permute(0, 3, 1, 2), size=(S2, S2), mode="bicubic")
                model_state[k] = r.permute(0, 2, 3, 1).flatten(1, 2)
    if _get(mtlora, "ENABLED"):  # utils.py:123-149
        mapping = lora_key_mapping(model_state, mtlora)
        if not mapping:
            print("No keys needs to be mapped for LoRA")
        map_old_state_dict_weights(model_state, mapping, "", split_qkv)
    return model_state


def load_state(model: nn.Module, model_state: MutableMapping[str, torch.Tensor], mtlora: Any = None,
               update_relative_position: bool = False, skip_decoder: bool = False, split_qkv: bool = False,
               logger: Optional[logging.Logger] = None, quiet: bool = False) -> Tuple[List[str], List[str]]:
    """prepare + ``load_state_dict(strict=False)``; returns (missing, unexpected) and logs them like the reference."""
    log = logger or _LOG
    prepare_state_dict(model, model_state, mtlora, update_relative_position, skip_decoder, split_qkv, log)
    res = model.load_state_dict(model_state, strict=False)
    missing, unexpected = list(res.missing_keys), list(res.unexpected_keys)
    if not quiet:
        if missing:
            log.warning("=============Missing Keys==============")
            for k in missing:
                log.warning(k)
        if unexpected:
            log.warning("=============Unexpected Keys==============")
            for k in unexpected:
                log.warning(k)
    return missing, unexpected


def load_checkpoint(config, model, optimizer, lr_scheduler, loss_scaler, logger, backbone: bool = False, quiet: bool = False):
    """Drop-in for reference ``utils.load_checkpoint`` (utils.py:41-176): same signature, same config fields read
    (``MODEL.RESUME[_BACKBONE]``, ``MODEL.MTLORA``, ``MODEL.UPDATE_RELATIVE_POSITION``, ``TRAIN.SKIP_DECODER_CKPT``,
    ``EVAL_MODE``), returns ``max_accuracy``."""
    path = config.MODEL.RESUME if not backbone else config.MODEL.RESUME_BACKBONE
    logger.info(f"==============> Resuming form {path}....................")
    if str(path).startswith("https"):
        ckpt = torch.hub.load_state_dict_from_url(path, map_location="cpu", check_hash=True)
    else:
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
    mtlora = config.MODEL.MTLORA
    skip_decoder = bool(_get(config.TRAIN, "SKIP_DECODER_CKPT", False))
    adapter_only = bool(ckpt.get("trainable_only", False))  # save_checkpoint(trainable_only=True): no frozen tensors in the file
    missing, unexpected = load_state(model, ckpt["model"], mtlora, bool(_get(config.MODEL, "UPDATE_RELATIVE_POSITION", False)),
                                     skip_decoder, bool(_get(mtlora, "SPLIT_QKV", False)), logger, quiet or adapter_only)
    if adapter_only:
        if unexpected:
            raise RuntimeError(f"mtlora_amd: adapter-only checkpoint {path} holds keys this model does not have: {unexpected}")
        frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
        expected = [k for k in missing if k in frozen]
        logger.info(f"adapter-only checkpoint: {len(expected)} frozen tensors are not in the file, as expected; they keep their values")
        if not quiet:
            for k in (k for k in missing if k not in frozen):
                logger.warning(f"missing key (trainable or buffer): {k}")
    max_accuracy = 0.0
    if (not _get(config, "EVAL_MODE", False) and "optimizer" in ckpt and "lr_scheduler" in ckpt and "epoch" in ckpt
            and not skip_decoder):
        optimizer.load_state_dict(ckpt["optimizer"])
        lr_scheduler.load_state_dict(ckpt["lr_scheduler"])
        if hasattr(config, "defrost"):
            config.defrost()
        config.TRAIN.START_EPOCH = ckpt["epoch"] + 1
        if hasattr(config, "freeze"):
            config.freeze()
        if "scaler" in ckpt and loss_scaler is not None:
            loss_scaler.load_state_dict(ckpt["scaler"])
        logger.info(f"=> loaded successfully '{path}' (epoch {ckpt['epoch']})")
        max_accuracy = ckpt.get("max_accuracy", 0.0)
    del ckpt
    return max_accuracy


def merge_lora_weights(model: nn.Module) -> int:
    """Fold the low-rank updates into the frozen weights for inference (the role of reference lora.py:636-641, whose
    ``MTLoRALinear.merge`` is a stub): calls ``merge()`` on every ``MTLoRALinear``; returns how many layers merged.  Layers
    whose task outputs do not see the shared update (``shared_mode='matrix'`` with tasks) cannot be expressed by one weight
    and stay as they are."""
    return sum(1 for m in model.modules() if isinstance(m, MTLoRALinear) and m.merge())


def unmerge_lora_weights(model: nn.Module) -> int:
    return sum(1 for m in model.modules() if isinstance(m, MTLoRALinear) and m.unmerge())


# ---- saving: the reference's save_checkpoint / auto_resume_helper (utils.py:280-321), an adapter-only file, TrainState ----------
def _is_trainable(t: torch.Tensor) -> bool:
    """what a train step may write of a ``state_dict(keep_vars=True)`` value: a parameter with ``requires_grad``, or a buffer"""
    return t.requires_grad if isinstance(t, nn.Parameter) else True


def lora_state_dict(model: nn.Module) -> "collections.OrderedDict[str, torch.Tensor]":
    """the adapter-only state dict (the role of loralib's ``lora_state_dict``): ``model.state_dict()`` without the frozen
    parameters -- the trainable parameters and every buffer, under their ``state_dict`` keys, detached, not copied"""
    full = model.state_dict(keep_vars=True)
    out = collections.OrderedDict((k, v.detach()) for k, v in full.items() if _is_trainable(v))
    if hasattr(full, "_metadata"):
        out._metadata = full._metadata
    return out


def auto_resume_helper(output_dir: str) -> Optional[str]:
    """the newest ``*.pth`` of ``output_dir`` by modification time, or None (reference utils.py:310-321)"""
    found = [os.path.join(output_dir, f) for f in os.listdir(output_dir) if f.endswith("pth")]
    print(f"All checkpoints founded in {output_dir}: {[os.path.basename(f) for f in found]}")
    if not found:
        return None
    newest = max(found, key=os.path.getmtime)
    print(f"The latest checkpoint founded: {newest}")
    return newest


_ALIGN = 16  # packed offsets of a snapshot (csrc/snapshot.hip)


class _Slot:
    """one pinned host buffer of a TrainState: the event of the copy that last wrote it, a generation count (a handle of an older
    generation is stale) and a flag a background save holds while it still reads the buffer"""

    def __init__(self, nbytes: int):
        self.host = torch.empty(max(nbytes, _ALIGN), dtype=torch.uint8, pin_memory=True)
        self.done: Optional[torch.cuda.Event] = None
        self.generation = 0
        self.free = threading.Event()
        self.free.set()


class SnapshotHandle:
    """what ``TrainState.snapshot()`` returns: the training state as of that call, on its way to (or in) pinned host memory.  Valid
    until the second ``snapshot()`` after it -- the state has two pinned buffers and reuses them in turn; ``state()`` of a
    superseded handle raises."""

    def __init__(self, owner: "TrainState", slot: _Slot, layout, host_part: Dict[str, Any]):
        self._owner, self._slot, self._generation, self._done = owner, slot, slot.generation, slot.done
        self._layout, self._host = layout, host_part

    def ready(self) -> bool:
        """whether the copy has arrived (no waiting)"""
        return self._done.query()

    def wait(self) -> "SnapshotHandle":
        self._done.synchronize()
        return self

    def _view(self, name) -> torch.Tensor:
        off, nbytes, dtype, shape = self._layout.where[name]
        return self._slot.host[off:off + nbytes].view(dtype).reshape(shape)

    def state(self, copy: bool = False) -> Dict[str, Any]:
        """``{"model", "optimizer", "scaler"}`` (and ``"lr_scheduler"`` / ``"meters"`` where the TrainState has them): the dicts
        ``model.state_dict()``, ``optimizer.state_dict()`` and ``loss_scaler.state_dict()`` would have returned at the
        ``snapshot()`` call, key for key, with host tensors that are views of the pinned buffer (``copy=True``: copies in
        ordinary memory, which outlive the handle).  ``"lr_schedule_updates"``, ``"scale"`` and ``"_growth_tracker"`` are read
        from the snapshot, not from the device.  Waits for the copy."""
        if self._generation != self._slot.generation:
            raise RuntimeError("mtlora_amd: this snapshot was superseded (its pinned buffer holds a later one); take state() "
                               "before the second snapshot() after it, or state(copy=True)")
        self.wait()
        own, lay = self._owner, self._layout
        fix = (lambda t: t.clone()) if copy else (lambda t: t)
        model = collections.OrderedDict()
        for key in lay.model_keys:
            model[key] = fix(self._view(("model", key))) if ("model", key) in lay.where else own._frozen[key]
        if lay.model_metadata is not None:
            model._metadata = lay.model_metadata
        out: Dict[str, Any] = {"model": model, "optimizer": None, "scaler": None}
        opt = own.optimizer
        if isinstance(opt, FusedOptimizer):
            tensors = {n: fix(self._view(("optimizer", n))) for n in lay.fused_names}
            out["optimizer"] = opt.state_dict_from(tensors, self._host["optimizer"])
        elif opt is not None:
            sd = self._host["optimizer"]
            out["optimizer"] = {"state": {i: {k: (fix(self._view(("optimizer", i, k))) if ("optimizer", i, k) in lay.where else v)
                                              for k, v in s.items()} for i, s in sd["state"].items()},
                                "param_groups": sd["param_groups"]}
        sc = own.loss_scaler
        if isinstance(sc, LossScaler):
            words = {n: self._view(("scaler", n)) for n in ("scale", "growth_tracker")} if lay.scaler_words else None
            out["scaler"] = sc.state_dict_from(words)
        elif sc is not None:
            out["scaler"] = self._host["scaler"]
        if own.lr_scheduler is not None:
            out["lr_scheduler"] = self._host["lr_scheduler"]
        if own.meters is not None:
            out["meters"] = {"bank": self._view(("meters", "bank")).clone(), "counter": int(self._view(("meters", "counter")).item())}
        return out


class _Layout:
    """one enumeration of the live tensors: where each sits in the packed buffer, the uploaded table, the staging buffer"""

    def __init__(self, entries: List[Tuple[Any, torch.Tensor]], device):
        lib = _lib.lib()
        eb, n = lib.mtlora_snapshot_entry_bytes(), len(entries)
        host = (ctypes.c_ubyte * (eb * max(n, 1)))()
        self.where: Dict[Any, Tuple[int, int, torch.dtype, torch.Size]] = {}
        self.signature = tuple((name, t.data_ptr(), t.numel() * t.element_size()) for name, t in entries)
        self.keep = [t for _, t in entries]  # (the table holds their addresses)
        off = 0
        for i, (name, t) in enumerate(entries):
            if not t.is_contiguous():
                raise ValueError(f"mtlora_amd: TrainState needs contiguous tensors ({name}: strides {t.stride()})")
            if t.device != device:
                raise ValueError(f"mtlora_amd: TrainState needs every tensor on {device} ({name} is on {t.device})")
            nbytes = t.numel() * t.element_size()
            _lib.check(lib.mtlora_snapshot_entry(ctypes.byref(host, i * eb), _lib.ptr(t) if nbytes else None, nbytes, off),
                       "mtlora_snapshot_entry")
            self.where[name] = (off, nbytes, t.dtype, t.shape)
            off = -(-(off + nbytes) // _ALIGN) * _ALIGN
        self.n, self.extent = n, off
        self.n_chunks = lib.mtlora_snapshot_chunks(host, n)
        if self.n_chunks < 0:
            _lib.check(int(self.n_chunks), "mtlora_snapshot_chunks")
        _lib.check(lib.mtlora_snapshot_check(host, n, self.extent), "mtlora_snapshot_check")
        self.table = torch.frombuffer(host, dtype=torch.uint8).clone().to(device)
        self.staging = torch.empty(max(self.extent, _ALIGN), dtype=torch.uint8, device=device)
        self.model_keys: List[str] = []
        self.model_metadata = None
        self.fused_names: List[str] = []
        self.scaler_words = False


class TrainState:
    """Everything a train step mutates, enumerated ONCE: every parameter with ``requires_grad``, every module buffer, the
    optimizer's state (a fused optimizer's flat state buffers -- ``FusedAdamW``'s and ``FusedLAMB``'s two moment buffers, ``FusedSGD``'s
    momentum buffer --, its control block -- step count, accumulation counter -- and its
    schedule buffer; a torch optimizer's state tensors, enumerated at the first snapshot after a step), the ``LossScaler``'s two
    device words and the meters' bank.  GPU only.

    * ``snapshot()``: ONE ``mtlora_snapshot_pack`` launch on the current stream into a device staging buffer, then ONE asynchronous
      copy into one of two pinned host buffers on a side stream, behind an event.  Returns a ``SnapshotHandle`` at once.  The
      training stream is held for the pack launch only; later steps write the live tensors, not the staging buffer.  It waits
      only if both pinned buffers are still in flight (or a background save still reads the one whose turn it is).  The frozen
      tensors are copied to the host once, at the first snapshot, and shared by every handle after it.
    * ``restore(handle_or_state)``: back through the objects' own ``load_state_dict`` -- so with their rules: a ``FusedAdamW`` starts a
      new accumulation cycle and is written in place, into the buffers a live graph holds.
    * The table holds raw addresses: a tensor that was re-allocated (``p.data = ...``, ``model.to()``), or a changed set of
      trainable parameters, makes ``snapshot()`` raise; build a new ``TrainState`` then.
    ``lr_scheduler`` is host state; its ``state_dict()`` is taken at the ``snapshot()`` call."""

    def __init__(self, model: nn.Module, optimizer=None, lr_scheduler=None, loss_scaler=None, meters=None):
        self.model, self.optimizer, self.lr_scheduler, self.loss_scaler, self.meters = model, optimizer, lr_scheduler, loss_scaler, meters
        full = model.state_dict(keep_vars=True)
        live = [v for v in full.values() if _is_trainable(v)]
        if not live:
            raise ValueError("mtlora_amd: TrainState found neither a trainable parameter nor a buffer in the model")
        _lib.require_gpu(*live)
        self.device = live[0].device
        self._trainable = self._trainable_names()
        # (the parameters and buffers themselves, not detached aliases: a later ``p.data = ...`` shows in ``data_ptr()``)
        self._model_entries = [(("model", k), v) for k, v in full.items() if _is_trainable(v)]
        self._model_keys, self._model_metadata = list(full.keys()), getattr(full, "_metadata", None)
        self._frozen_live = {k: v for k, v in full.items() if not _is_trainable(v)}
        self._frozen: Optional[Dict[str, torch.Tensor]] = None
        self._layout: Optional[_Layout] = None
        self._slots: List[_Slot] = []
        self._turn = 0
        self._copy_stream = torch.cuda.Stream(device=self.device)
        self._staging_read: Optional[torch.cuda.Event] = None  # the copy that last read the staging buffer

    def _trainable_names(self) -> List[str]:
        return [n for n, p in self.model.named_parameters() if p.requires_grad]

    def _entries(self) -> Tuple[List[Tuple[Any, torch.Tensor]], Dict[str, Any]]:
        """the live tensors in packed order, and the host half of the state as of now.  The model's part was fixed at
        construction; the rest is a handful of tensors (FusedAdamW) or a walk over ``optimizer.state`` (torch)."""
        entries, host = list(self._model_entries), {}
        opt, sc = self.optimizer, self.loss_scaler
        fused_names: List[str] = []
        if isinstance(opt, FusedOptimizer):
            tensors = opt.state_tensors()
            fused_names = list(tensors)
            entries += [(("optimizer", n), t) for n, t in tensors.items()]
            host["optimizer"] = opt.state_meta()
        elif opt is not None:
            sd = opt.state_dict()  # torch: references to the live state tensors, no copy and no synchronisation
            for i, s in sd["state"].items():
                for k, v in s.items():
                    if torch.is_tensor(v) and v.is_cuda:
                        entries.append((("optimizer", i, k), v.detach()))
            host["optimizer"] = {"state": {i: {k: (v.clone() if torch.is_tensor(v) and not v.is_cuda else v) for k, v in s.items()}
                                           for i, s in sd["state"].items()}, "param_groups": sd["param_groups"]}
        words = sc.device_words() if isinstance(sc, LossScaler) else None
        if words is not None:
            entries += [(("scaler", n), t) for n, t in words.items()]
        elif sc is not None and not isinstance(sc, LossScaler):
            host["scaler"] = sc.state_dict()  # (another scaler's own state_dict(): it may synchronise)
        if self.lr_scheduler is not None:
            host["lr_scheduler"] = dict(self.lr_scheduler.state_dict())
        if self.meters is not None:
            entries += [(("meters", "bank"), self.meters.bank), (("meters", "counter"), self.meters.counter)]
        host["_fused_names"], host["_scaler_words"] = fused_names, words is not None
        return entries, host

    def _check_unchanged(self) -> None:
        if self._trainable_names() != self._trainable:
            raise RuntimeError("mtlora_amd: the set of trainable parameters changed after this TrainState was built; build a new one")

    def snapshot(self) -> SnapshotHandle:
        self._check_unchanged()
        entries, host = self._entries()
        signature = tuple((name, t.data_ptr(), t.numel() * t.element_size()) for name, t in entries)
        lay = self._layout
        if lay is None or lay.signature != signature:
            if lay is not None and lay.signature[:len(self._model_entries)] != signature[:len(self._model_entries)]:
                raise RuntimeError("mtlora_amd: a parameter or buffer of the model was re-allocated after this TrainState was built; "
                                   "build a new one")
            # the first snapshot, or the optimizer / scaler state came into being since the last one: a new table and new buffers
            for s in self._slots:
                s.free.wait()
            torch.cuda.synchronize(self.device)
            lay = _Layout(entries, self.device)
            lay.model_keys, lay.model_metadata = self._model_keys, self._model_metadata
            lay.fused_names, lay.scaler_words = host["_fused_names"], host["_scaler_words"]
            self._layout, self._staging_read = lay, None
            self._slots = [_Slot(lay.extent), _Slot(lay.extent)]
        if self._frozen is None:  # once: these never change
            self._frozen = {k: v.detach().cpu() for k, v in self._frozen_live.items()}
        slot = self._slots[self._turn]
        self._turn ^= 1
        slot.free.wait()  # a background save is still reading this buffer
        if slot.done is not None and not slot.done.query():
            slot.done.synchronize()  # both pinned buffers in flight
        with torch.cuda.device(self.device):
            main = torch.cuda.current_stream()
            if self._staging_read is not None:
                main.wait_event(self._staging_read)  # (a device-side wait) the previous copy has read the staging buffer
            _lib.check(_lib.lib().mtlora_snapshot_pack(_lib.ptr(lay.table), lay.n, lay.n_chunks, _lib.ptr(lay.staging), lay.extent,
                                                       _lib.stream_ptr()), "mtlora_snapshot_pack")
            packed = torch.cuda.Event()
            packed.record(main)
            self._copy_stream.wait_event(packed)
            with torch.cuda.stream(self._copy_stream):
                slot.host[:max(lay.extent, 1)].copy_(lay.staging[:max(lay.extent, 1)], non_blocking=True)
                done = torch.cuda.Event()
                done.record(self._copy_stream)
        slot.done, self._staging_read = done, done
        slot.generation += 1
        return SnapshotHandle(self, slot, lay, host)

    def restore(self, handle_or_state) -> None:
        """load a snapshot (or the dict ``SnapshotHandle.state()`` returns, or a checkpoint file's dict) back into the live
        objects through their ``load_state_dict``"""
        st = handle_or_state.state() if isinstance(handle_or_state, SnapshotHandle) else handle_or_state
        self.model.load_state_dict(st["model"], strict=not st.get("trainable_only", False))
        if self.optimizer is not None and st.get("optimizer") is not None:
            self.optimizer.load_state_dict(st["optimizer"])
        if self.lr_scheduler is not None and st.get("lr_scheduler") is not None:
            self.lr_scheduler.load_state_dict(st["lr_scheduler"])
        if self.loss_scaler is not None and st.get("scaler") is not None:
            self.loss_scaler.load_state_dict(st["scaler"])
        if self.meters is not None and st.get("meters") is not None:
            self.meters.bank.copy_(st["meters"]["bank"])
            self.meters.counter.fill_(int(st["meters"]["counter"]))


_writer: Optional[concurrent.futures.ThreadPoolExecutor] = None
_pending: List[concurrent.futures.Future] = []
_pending_lock = threading.Lock()


def _raise_failed(wait: bool) -> None:
    with _pending_lock:
        jobs = list(_pending)
    if wait:
        concurrent.futures.wait(jobs)
    failed = None
    with _pending_lock:
        for f in jobs:
            if f.done():
                _pending.remove(f)
                if failed is None and f.exception() is not None:
                    failed = f.exception()
    if failed is not None:
        raise RuntimeError(f"mtlora_amd: a background checkpoint write failed: {type(failed).__name__}: {failed}") from failed


def wait_for_saves() -> None:
    """wait for every ``save_checkpoint(..., blocking=False)`` made so far; raises if one of the writes failed"""
    _raise_failed(wait=True)


def _write(payload: Dict[str, Any], path: str, logger) -> None:
    tmp = path + ".tmp"  # (no "pth" ending: auto_resume_helper never sees a half-written file)
    torch.save(payload, tmp)
    os.replace(tmp, path)
    logger.info(f"{path} saved !!!")


def save_checkpoint(config, epoch, model, max_accuracy, optimizer, lr_scheduler, loss_scaler, logger, state: Optional[TrainState] = None,
                    blocking: bool = True, trainable_only: bool = False) -> str:
    """Drop-in for reference ``utils.save_checkpoint`` (utils.py:280-294): writes ``config.OUTPUT/ckpt_epoch_{epoch}.pth`` with the
    keys ``model, optimizer, lr_scheduler, max_accuracy, scaler, epoch, config`` and returns the path; ``load_checkpoint`` and
    plain ``torch.load`` read it.  A failed background write of an earlier call is raised here.

    * without ``state``: the reference's synchronous ``state_dict()`` + ``torch.save``.
    * ``state`` (the ``TrainState`` of these same objects): ``state.snapshot()`` -- one launch on the training stream -- and the file is
      written from the pinned copy; ``blocking=False`` hands that to ONE background thread and returns at once (``wait_for_saves()``
      before reading the file, and at the end of the run).
    * ``trainable_only=True``: ``"model"`` is ``lora_state_dict(model)`` -- trainable parameters and buffers only -- and the file
      carries ``"trainable_only": True``, which ``load_checkpoint`` reads as: missing frozen keys are expected."""
    _raise_failed(wait=False)
    path = os.path.join(config.OUTPUT, f"ckpt_epoch_{epoch}.pth")
    logger.info(f"{path} saving......")

    def payload_of(model_sd, opt_sd, sched_sd, scaler_sd):
        p = {"model": model_sd, "optimizer": opt_sd, "lr_scheduler": sched_sd, "max_accuracy": max_accuracy, "scaler": scaler_sd,
             "epoch": epoch, "config": config}
        if trainable_only:
            p["trainable_only"] = True
        return p

    if state is None:
        model_sd = lora_state_dict(model) if trainable_only else model.state_dict()
        _write(payload_of(model_sd, optimizer.state_dict(), lr_scheduler.state_dict(), loss_scaler.state_dict()), path, logger)
        return path
    if (state.model is not model or state.optimizer is not optimizer or state.lr_scheduler is not lr_scheduler
            or state.loss_scaler is not loss_scaler):
        raise ValueError("mtlora_amd: save_checkpoint(state=) needs the TrainState built from this model, optimizer, lr_scheduler "
                         "and loss_scaler")
    handle = state.snapshot()
    slot = handle._slot
    slot.free.clear()  # the next snapshot() whose turn this buffer is waits until the job below has copied it out

    def job():
        try:
            st = handle.state(copy=True)  # waits for the copy; ordinary memory from here on
        finally:
            slot.free.set()
        model_sd = st["model"]
        if trainable_only:
            keep = collections.OrderedDict((k, v) for k, v in model_sd.items() if ("model", k) in handle._layout.where)
            if hasattr(model_sd, "_metadata"):
                keep._metadata = model_sd._metadata
            model_sd = keep
        _write(payload_of(model_sd, st["optimizer"], st.get("lr_scheduler"), st["scaler"]), path, logger)

    if blocking:
        job()
        return path
    global _writer
    if _writer is None:
        _writer = concurrent.futures.ThreadPoolExecutor(max_workers=1, thread_name_prefix="mtlora-checkpoint")
    with _pending_lock:
        _pending.append(_writer.submit(job))
    return path
