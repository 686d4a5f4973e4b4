"""muP AdamW: `torch.optim.AdamW(groups, betas=(0.95, 0.99), fused=True)` of the reference
(train.py:335-344,433) as ONE multi-tensor HIP launch over every (sharded) fp32 parameter, which
also refreshes the bf16 compute copy (saving the cast pass of the next forward / all-gather).

Use exactly like the reference:
    groups, settings = dit.get_mup_setup(lr, 0.1, ["patch_proj", "context_kv", "positional_embedding"])
    opt = MuAdamW(groups, betas=(0.95, 0.99))
It is a torch.optim.Optimizer, so HF / torch LR schedulers drive `param_groups[i]["lr"]` as usual.

Guarded step (all three options default to off; with them off `step()` issues exactly the one launch above):
    opt = MuAdamW(groups, betas=(0.95, 0.99), max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.9999)
`step()` then runs, on the current stream and without reading anything on the host: a fixed-order sum of squares of
every gradient (`vds_grad_sumsq_multi`) -> when sharded, an all-reduce of that one float over the shard group -> a
finalize that leaves norm / coefficient / skipped flag / skipped count in a device record -> the guarded AdamW launch
that reads the record (and updates the EMA in the same pass).  So the whole thing replays from a captured graph.

  * max_grad_norm: global L2 clip with the arithmetic of `torch.nn.utils.clip_grad_norm_`
    (coefficient min(1, max_norm / (norm + 1e-6))).  The coefficient is applied INSIDE the kernel: `p.grad` is not
    modified.  `float("inf")` is legal (coefficient exactly 1: only the norm is measured).
  * skip_nonfinite: a step whose global gradient norm is inf / NaN writes nothing -- parameters, both moments, the
    bf16 shadows and the EMA keep every bit -- and the device count behind `skipped_steps()` goes up by one.
    UNLIKE torch's GradScaler, a skipped step STILL COUNTS as a step for the bias corrections and for the LR schedule:
    the host cannot know that it was skipped without a synchronisation, and a replayed step must not depend on it.
  * ema_decay: `state[p]["ema"]` (fp32, the shape of `p` -- the shard under sharding), initialised to a copy of `p`
    the first time `step()` sees the parameter (before that step's update), then ema = d * ema + (1 - d) * p_new.
    `opt.ema_decay = d` may be changed at any time, also between graph replays.  `swap_ema()` /
    `with opt.ema_weights():` exchange parameters and EMA in place (sampling, evaluation, `model_ema.pt`).
  * `opt.grad_norm`: 0-d DEVICE tensor, the pre-clip global norm of the last step (`.item()` it at logging time only).
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import List

import torch

from . import _lib, ops

CHUNK = 1 << 16


class MuAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.95, 0.99), eps=1e-8, weight_decay=1e-2, fused=True,
                 max_grad_norm=None, skip_nonfinite=False, ema_decay=None):
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:  # also refuses NaN
            raise ValueError(f"MuAdamW: max_grad_norm must be > 0 (inf allowed) or None, got {max_grad_norm}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._step = 0
        self._table_key = None
        self._chunk_key = None
        self._dev = {}
        self._dev_scalars = None  # device float[4]: see use_device_scalars
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._ema_decay = None
        self.ema_decay = ema_decay
        self._guard = None        # device record of the guarded step: float32[4] = vds_optim_guard
        self._skipped_seed = 0    # skipped count to start from (load_state_dict before the record exists)
        self._ema_swapped = False

    # ---- guarded step: options and what it leaves behind ---------------------------------------
    @property
    def ema_decay(self):
        return self._ema_decay

    @ema_decay.setter
    def ema_decay(self, d):
        if d is not None and not 0.0 <= float(d) < 1.0:
            raise ValueError(f"MuAdamW: ema_decay must be in [0, 1) or None, got {d}")
        if (d is None) != (self._ema_decay is None):
            self._table_key = None  # the EMA pointer table appears / disappears
        self._ema_decay = None if d is None else float(d)

    @property
    def guarded(self) -> bool:
        return self.max_grad_norm is not None or self.skip_nonfinite or self._ema_decay is not None

    @property
    def grad_norm(self):
        """0-d device tensor: global L2 norm of the gradients of the last `step()`, before clipping (None before the
        first guarded step).  Reading it on the host synchronises: do that at logging time only."""
        return None if self._guard is None else self._guard[0]

    def skipped_steps(self) -> int:
        """number of steps `skip_nonfinite` has skipped so far (reads the device count: synchronises)"""
        if self._guard is None:
            return self._skipped_seed
        return int(self._guard.view(torch.int32)[3].item())

    def _guard_record(self, device):
        if self._guard is None:
            rec = torch.zeros(4, dtype=torch.int32, device=device)
            rec[3] = self._skipped_seed
            self._guard = rec.view(torch.float32)
            self._dev["sumsq"] = torch.zeros(1, dtype=torch.float32, device=device)
        return self._guard

    @torch.no_grad()
    def swap_ema(self):
        """exchange every parameter with its EMA, in place (pointers stay: a captured step keeps working), and void the
        bf16 compute copies so that the next forward -- eager or replayed -- re-casts.  Twice = every bit restored."""
        groups = {}
        for group in self.param_groups:
            for p in group["params"]:
                ema = self.state.get(p, {}).get("ema")
                if ema is None or ema.numel() != p.numel():
                    continue
                tmp = p.data.clone()
                p.data.copy_(ema.view_as(p.data))
                ema.copy_(tmp.view_as(ema))
                g = getattr(p, "_vds_group", None)
                if g is not None:
                    groups[id(g)] = g
        for g in groups.values():
            g.invalidate_shadow()
        self._ema_swapped = not self._ema_swapped

    @contextlib.contextmanager
    def ema_weights(self):
        """`with opt.ema_weights(): sample / evaluate`: the model computes with the EMA inside the block"""
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    def ema_named(self, model):
        """{parameter name: this rank's EMA piece} for the parameters of `model` that carry one"""
        out = {}
        for n, p in model.named_parameters():
            ema = self.state.get(p, {}).get("ema")
            if ema is not None and ema.numel() == p.numel():
                out[n] = ema
        return out

    def use_device_scalars(self, device):
        """Keep the per-step scalars (bias corrections, LR multiplier) in device memory instead of kernel
        arguments, so that a captured step can be replayed (graph.py).  `step()` refreshes them with a
        stream-ordered copy unless the stream is capturing; a replay driver calls `advance()` itself."""
        if self._dev_scalars is None:
            self._dev_scalars = torch.zeros(4, dtype=torch.float32, device=device)
        return self._dev_scalars

    def _scalars(self, mult):
        import numpy as np
        b1, b2 = (np.float32(b) for b in self.param_groups[0]["betas"])
        one, st = np.float32(1), np.float32(self._step)
        bc1 = one - np.power(b1, st)
        bc2 = one - np.power(b2, st)
        # [3]: the EMA decay of the guarded step (read by vds_adamw_guarded_multi_dev only)
        return torch.tensor([bc1, one / np.sqrt(bc2), np.float32(mult), np.float32(self._ema_decay or 0.0)],
                            dtype=torch.float32)

    def advance(self):
        """host half of one captured step: count it and push its scalars (call before the replay)"""
        plist = [(p, g) for g in self.param_groups for p in g["params"] if p.grad is not None and p.numel() > 0]
        lrs, mult = self._lr_plan(plist)
        if self._table_key is not None and tuple(k[2] for k in self._table_key) != tuple(lrs):
            raise RuntimeError("MuAdamW: the base learning rates changed under a captured step; capture again")
        self._step += 1
        self._dev_scalars.copy_(self._scalars(mult))

    def _build_chunks(self, plist, device):
        chunk_t: List[int] = []
        chunk_s: List[int] = []
        for i, (p, _) in enumerate(plist):
            st = self.state[p]
            if "exp_avg" not in st or st["exp_avg"].numel() != p.numel():
                st["exp_avg"] = torch.zeros(p.numel(), dtype=torch.float32, device=device)
                st["exp_avg_sq"] = torch.zeros(p.numel(), dtype=torch.float32, device=device)
            n = p.numel()
            chunk_t.extend([i] * ((n + CHUNK - 1) // CHUNK))
            chunk_s.extend(range(0, n, CHUNK))
        self._dev["ct"] = torch.tensor(chunk_t, dtype=torch.int32, device=device)
        self._dev["cs"] = torch.tensor(chunk_s, dtype=torch.int64, device=device)
        self._dev["n"] = len(chunk_t)
        if self.guarded:  # the partials of the fixed-order sum of squares: one float per chunk
            nws = int(_lib.load().vds_grad_sumsq_workspace_floats(len(chunk_t)))
            self._dev["ws"] = torch.empty(nws, dtype=torch.float32, device=device)

    def _lr_plan(self, plist):
        """(per-param base lr list, common multiplier): LR schedulers scale every group's lr by the same
        factor of its `initial_lr` (train.py:349-364), so the descriptor table keeps the base lr and the
        factor travels as a kernel argument -- no table rebuild / H2D copy per step."""
        mult = None
        for _, g in plist:
            base = g.get("initial_lr", None)
            if base is None or base == 0.0:
                mult = None
                break
            r = g["lr"] / base
            if mult is None:
                mult = r
            elif abs(r - mult) > 1e-9 * max(abs(mult), 1e-30):
                mult = None
                break
        if mult is None:
            return [float(g["lr"]) for _, g in plist], 1.0
        return [float(g["initial_lr"]) for _, g in plist], float(mult)

    def _build_descs(self, plist, device, lrs):
        descs = (_lib.AdamWTensor * len(plist))()
        for i, (p, group) in enumerate(plist):
            st = self.state[p]
            shadow = getattr(p, "_vds_shadow", None)
            d = descs[i]
            d.p, d.g = p.data.data_ptr(), p.grad.data_ptr()
            d.m, d.v = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            d.p_bf16 = shadow.data_ptr() if shadow is not None and shadow.numel() == p.numel() else None
            d.numel = p.numel()
            d.lr, d.wd = lrs[i], float(group["weight_decay"])
        self._dev["desc"] = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(device)
        # the EMA pointers travel as a parallel array indexed by tensor (the descriptor keeps its 56 bytes)
        self._dev["ema"] = None
        if self._ema_decay is not None:
            self._dev["ema"] = torch.tensor([self.state[p]["ema"].data_ptr() for p, _ in plist],
                                            dtype=torch.int64).to(device)

    def state_dict(self):
        d = super().state_dict()
        d["vds_step"] = self._step
        if self.guarded:
            d["vds_skipped"] = self.skipped_steps()
        return d

    def load_state_dict(self, state_dict):
        state_dict = dict(state_dict)
        self._step = int(state_dict.pop("vds_step", 0))
        self._skipped_seed = int(state_dict.pop("vds_skipped", 0))
        if self._guard is not None:
            self._guard.view(torch.int32)[3] = self._skipped_seed
        super().load_state_dict(state_dict)
        self._table_key = self._chunk_key = None  # moments were replaced: rebuild the descriptor table

    @torch.no_grad()
    def step(self, closure=None):
        assert closure is None
        plist = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None or p.numel() == 0:
                    continue
                if not p.is_cuda:
                    raise RuntimeError("MuAdamW is a HIP kernel: parameters must be on the GPU")
                assert p.dtype == torch.float32 and p.grad.dtype == torch.float32
                assert p.data.is_contiguous() and p.grad.is_contiguous()
                plist.append((p, group))
        if not plist:
            return None
        self._step += 1
        device = plist[0][0].device
        if self._ema_decay is not None:
            if self._ema_swapped:
                raise RuntimeError("MuAdamW.step() while the EMA is swapped in: leave ema_weights() / swap_ema() back first")
            for p, _ in plist:  # first sight of a parameter: its EMA starts as a copy of it, before this step's update
                st = self.state[p]
                if "ema" not in st or st["ema"].numel() != p.numel():
                    st["ema"] = p.data.detach().clone()
                    self._table_key = None
        ckey = tuple(p.numel() for p, _ in plist)
        if ckey != self._chunk_key:
            self._build_chunks(plist, device)
            self._chunk_key, self._table_key = ckey, None
        lrs, mult = self._lr_plan(plist)
        key = tuple((p.data.data_ptr(), p.grad.data_ptr(), lr, g["weight_decay"]) for (p, g), lr in zip(plist, lrs))
        if self.guarded and "ws" not in self._dev:  # an option was switched on after the chunk table was built
            self._build_chunks(plist, device)
        if key != self._table_key:  # pointers or the base lr changed: refresh the descriptors
            self._build_descs(plist, device, lrs)
            self._table_key = key
        b1, b2 = self.param_groups[0]["betas"]
        eps = self.param_groups[0]["eps"]
        fresh_before = ()
        if self.guarded:
            fresh_before = self._step_guarded(plist, device, mult, b1, b2, eps)
        elif self._dev_scalars is not None:
            if not torch.cuda.is_current_stream_capturing():
                self._dev_scalars.copy_(self._scalars(mult))
            _lib.check(_lib.load().vds_adamw_multi_dev(self._dev["desc"].data_ptr(), self._dev["ct"].data_ptr(),
                                                       self._dev["cs"].data_ptr(), self._dev["n"], CHUNK, b1, b2, eps,
                                                       self._dev_scalars.data_ptr(), 1.0, ops._stream()),
                       "vds_adamw_multi_dev")
        else:
            _lib.check(_lib.load().vds_adamw_multi(self._dev["desc"].data_ptr(), self._dev["ct"].data_ptr(),
                                                   self._dev["cs"].data_ptr(), self._dev["n"], CHUNK, b1, b2, eps,
                                                   self._step, mult, 1.0, ops._stream()), "vds_adamw_multi")
        # the bf16 shadows of these flat groups are now current: the next forward skips its cast pass
        for g in {id(getattr(p, "_vds_group", None)): getattr(p, "_vds_group", None) for p, _ in plist}.values():
            if g is not None and (not self.skip_nonfinite or id(g) in fresh_before):
                g.mark_shadow_fresh()
        return None

    def _step_guarded(self, plist, device, mult, b1, b2, eps):
        """sum of squares -> (all-reduce over the shard group) -> finalize -> guarded AdamW, all on the current stream.
        Returns the ids of the flat groups whose bf16 shadow was current before the step: a step that may have been
        skipped has written no shadow, so it can only keep that claim, not establish it."""
        lib, stream = _lib.load(), ops._stream()
        rec = self._guard_record(device)
        ss, d = self._dev["sumsq"], self._dev
        max_norm = 0.0 if self.max_grad_norm is None else self.max_grad_norm  # 0 = clipping off
        skip = 1 if self.skip_nonfinite else 0
        shard = None  # the flat group whose communicator spans the ranks that own the other gradient elements
        fresh_before = set()
        for g in {id(getattr(p, "_vds_group", None)): getattr(p, "_vds_group", None) for p, _ in plist}.values():
            if g is None:
                continue
            if shard is None and (g.world > 1 or g.runtime is not None):
                shard = g
            if g.shadow_fresh:
                fresh_before.add(id(g))
        _lib.check(lib.vds_grad_sumsq_multi(d["desc"].data_ptr(), d["ct"].data_ptr(), d["cs"].data_ptr(), d["n"], CHUNK,
                                            d["ws"].data_ptr(), ss.data_ptr(), max_norm, skip,
                                            None if shard is not None else rec.data_ptr(), stream),
                   "vds_grad_sumsq_multi")
        if shard is not None:
            shard.all_reduce_scalar(ss)
            _lib.check(lib.vds_optim_guard_finalize(ss.data_ptr(), 1.0, max_norm, skip, rec.data_ptr(), stream),
                       "vds_optim_guard_finalize")
        ema = d["ema"].data_ptr() if d.get("ema") is not None else None
        if self._dev_scalars is not None:
            if not torch.cuda.is_current_stream_capturing():
                self._dev_scalars.copy_(self._scalars(mult))
            _lib.check(lib.vds_adamw_guarded_multi_dev(d["desc"].data_ptr(), d["ct"].data_ptr(), d["cs"].data_ptr(), d["n"],
                                                       CHUNK, b1, b2, eps, self._dev_scalars.data_ptr(), 1.0,
                                                       rec.data_ptr(), ema, stream), "vds_adamw_guarded_multi_dev")
        else:
            _lib.check(lib.vds_adamw_guarded_multi(d["desc"].data_ptr(), d["ct"].data_ptr(), d["cs"].data_ptr(), d["n"],
                                                   CHUNK, b1, b2, eps, self._step, mult, 1.0, rec.data_ptr(), ema,
                                                   self._ema_decay or 0.0, stream), "vds_adamw_guarded_multi")
        return fresh_before


# ---------------------------------------------------------------------------------------------- Muon ----
MUON_SLICE_BYTES = 256 << 20  # a bucket larger than this much workspace runs in slices of whole matrices


class MuonAdamW(MuAdamW):
    """Muon -- momentum, orthogonalised by a Newton-Schulz iteration (csrc/muon.hip) -- for the parameter groups that carry
    `use_muon=True`, `MuAdamW` for every other group:

        groups, table = dit.get_muon_setup(lr, 0.1, ["patch_proj", "context_kv", "positional_embedding"], muon_lr=0.02)
        opt = MuonAdamW(groups, betas=(0.95, 0.99))

    A Muon group holds 2-D parameters; `muon_split` = s says that each is s matrices stacked along its rows (qkv: 3,
    context_kv: 2), which are orthogonalised separately.  Group keys: `lr`, `weight_decay`, `momentum` (0.95), `nesterov`
    (True), `ns_steps` (5).  Per step and matrix W [rows, cols] with gradient G (coef = the clip coefficient, 1 without):
        buf = momentum * buf + coef * G;   u = coef * G + momentum * buf  (nesterov)  |  buf
        O = NewtonSchulz(u / (||u||_F + 1e-7), ns_steps)
        W = W * (1 - lr * weight_decay) - lr * sqrt(max(1, rows / cols)) * O
    The matrices are bucketed by (split) shape and every bucket runs momentum -> orthogonalize -> update as batched
    launches on the current stream, nothing read on the host: the step replays from a captured graph and follows the LR
    schedule through the device scalars of `use_device_scalars`.  `max_grad_norm`, `skip_nonfinite` and `ema_decay` work
    as documented for `MuAdamW`: the sum of squares covers EVERY gradient, Muon's included, and the Muon kernels read the
    same device record (a skipped step leaves parameters, momentum, shadows and EMA untouched).
    `state[p]["momentum_buffer"]` is fp32 in the shape of `p`.

    Whole matrices only: a parameter that is a shard of an `apply_fsdp`-wrapped model raises ValueError."""

    def __init__(self, params, lr=1e-3, betas=(0.95, 0.99), eps=1e-8, weight_decay=1e-2, fused=True,
                 max_grad_norm=None, skip_nonfinite=False, ema_decay=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, fused=fused,
                         max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, ema_decay=ema_decay)
        for group in self.param_groups:
            if not group.get("use_muon"):
                continue
            group.setdefault("momentum", 0.95)
            group.setdefault("nesterov", True)
            group.setdefault("ns_steps", 5)
            split = group.setdefault("muon_split", 1)
            if split not in (1, 2, 3):
                raise ValueError(f"MuonAdamW: muon_split must be 1, 2 or 3, got {split}")
            if not 0.0 <= float(group["momentum"]) < 1.0:
                raise ValueError(f"MuonAdamW: momentum must be in [0, 1), got {group['momentum']}")
            if int(group["ns_steps"]) != group["ns_steps"] or not 0 <= group["ns_steps"] <= 64:
                raise ValueError(f"MuonAdamW: ns_steps must be an integer in [0, 64], got {group['ns_steps']}")
            for p in group["params"]:
                g = getattr(p, "_vds_group", None)
                full = tuple(getattr(p, "_vds_full_shape", p.shape))
                if (g is not None and g.world > 1) or tuple(p.shape) != full:
                    raise ValueError("MuonAdamW: Muon needs whole matrices (the Newton-Schulz iteration multiplies a "
                                     f"matrix with its transpose); this parameter is a shard of a {full} tensor of an "
                                     "apply_fsdp-wrapped model")
                if p.dim() != 2:
                    raise ValueError(f"MuonAdamW: a Muon group takes 2-D parameters, got shape {tuple(p.shape)}")
                rows, cols = p.shape[0] // split, p.shape[1]
                if p.shape[0] % split or rows % 8 or cols % 8 or rows == 0:
                    raise ValueError(f"MuonAdamW: shape {tuple(p.shape)} with muon_split={split}: every matrix needs "
                                     "rows and columns that are multiples of 8")
        self._muon = {}        # bucket key -> dict(table, nmat, rows, cols, ...)
        self._muon_key = None
        self._muon_ws = None
        self._all = {}         # descriptor / chunk tables over EVERY gradient: the guarded step's sum of squares
        self._all_key = None
        self._guard_done = False
        self._muon_active = False

    # ---- the AdamW half sees the groups without `use_muon` only -------------------------------------
    @contextlib.contextmanager
    def _adam_groups_only(self):
        every = self.param_groups
        self.param_groups = [g for g in every if not g.get("use_muon")]
        try:
            yield
        finally:
            self.param_groups = every

    def _muon_plist(self):
        return [(p, g) for g in self.param_groups if g.get("use_muon") for p in g["params"]
                if p.grad is not None and p.numel() > 0]

    def _adam_plist(self):
        return [(p, g) for g in self.param_groups if not g.get("use_muon") for p in g["params"]
                if p.grad is not None and p.numel() > 0]

    def _muon_lr_plan(self, mlist):
        """(base lr per Muon parameter, multiplier): the AdamW half's plan when the Muon groups follow the same
        schedule (every scheduler of train.get_schedule does), else the current lr with multiplier 1 -- which a captured
        step cannot follow, since it reads the AdamW half's multiplier from the device scalars"""
        alist = self._adam_plist()
        lrs, mult = self._lr_plan(alist + mlist)  # (the AdamW half first: its ratio is the common multiplier, to the bit)
        if alist and self._dev_scalars is not None and self._lr_plan(alist)[1] != mult:
            raise RuntimeError("MuonAdamW: the Muon groups and the AdamW groups follow different LR schedules; a step "
                               "with device scalars (graph replay) needs one common multiplier")
        return lrs[len(alist):], mult

    def advance(self):
        mlist = self._muon_plist()
        if mlist and self._muon_key is not None:
            lrs, _ = self._muon_lr_plan(mlist)
            if tuple(lrs) != self._muon_key[1]:
                raise RuntimeError("MuonAdamW: the base learning rates changed under a captured step; capture again")
        if self._adam_plist():
            with self._adam_groups_only():
                super().advance()
        else:
            self._step += 1
            self._dev_scalars.copy_(self._scalars(self._muon_lr_plan(mlist)[1]))

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._muon_key = self._all_key = None  # momentum buffers / EMAs were replaced

    # ---- tables ---------------------------------------------------------------------------------------
    def _build_all(self, plist, device):
        """descriptor + chunk tables over every gradient (only .g and .numel are read)"""
        descs = (_lib.AdamWTensor * len(plist))()
        chunk_t: List[int] = []
        chunk_s: List[int] = []
        for i, (p, _) in enumerate(plist):
            descs[i].g, descs[i].numel = p.grad.data_ptr(), p.numel()
            chunk_t.extend([i] * ((p.numel() + CHUNK - 1) // CHUNK))
            chunk_s.extend(range(0, p.numel(), CHUNK))
        nws = int(_lib.load().vds_grad_sumsq_workspace_floats(len(chunk_t)))
        self._all = {"desc": torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(device),
                     "ct": torch.tensor(chunk_t, dtype=torch.int32, device=device),
                     "cs": torch.tensor(chunk_s, dtype=torch.int64, device=device), "n": len(chunk_t),
                     "ws": torch.empty(nws, dtype=torch.float32, device=device)}

    def _build_muon(self, mlist, lrs, device):
        buckets = {}
        for (p, group), lr in zip(mlist, lrs):
            st = self.state[p]
            split = group["muon_split"]
            rows, cols = p.shape[0] // split, p.shape[1]
            key = (rows, cols, lr, float(group["weight_decay"]), float(group["momentum"]), bool(group["nesterov"]),
                   int(group["ns_steps"]))
            shadow = getattr(p, "_vds_shadow", None)
            if shadow is not None and shadow.numel() != p.numel():
                shadow = None
            ema = st.get("ema") if self._ema_decay is not None else None
            for k in range(split):
                o = k * rows * cols
                buckets.setdefault(key, []).append((p.data.data_ptr() + 4 * o, p.grad.data_ptr() + 4 * o,
                                                    st["momentum_buffer"].data_ptr() + 4 * o,
                                                    None if shadow is None else shadow.data_ptr() + 2 * o,
                                                    None if ema is None else ema.data_ptr() + 4 * o))
        self._muon, ws_bytes = {}, 0
        for key, mats in buckets.items():
            rows, cols = key[0], key[1]
            per = max(1, MUON_SLICE_BYTES // ops.muon_workspace_bytes(1, rows, cols))
            slices = [(i, min(per, len(mats) - i)) for i in range(0, len(mats), per)]
            ws_bytes = max(ws_bytes, ops.muon_workspace_bytes(slices[0][1], rows, cols))
            self._muon[key] = {"table": ops.muon_table(mats, device), "slices": slices}
        if self._muon_ws is None or self._muon_ws.numel() < ws_bytes or self._muon_ws.device != device:
            self._muon_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)

    # ---- the step -----------------------------------------------------------------------------------------
    def _guard_all(self, device):
        """sum of squares over EVERY gradient -> (all-reduce over the shard group) -> record; once per step"""
        lib, stream = _lib.load(), ops._stream()
        rec = self._guard_record(device)
        d, ss = self._all, self._dev["sumsq"]
        max_norm = 0.0 if self.max_grad_norm is None else self.max_grad_norm
        skip = 1 if self.skip_nonfinite else 0
        _lib.check(lib.vds_grad_sumsq_multi(d["desc"].data_ptr(), d["ct"].data_ptr(), d["cs"].data_ptr(), d["n"], CHUNK,
                                            d["ws"].data_ptr(), ss.data_ptr(), max_norm, skip, rec.data_ptr(), stream),
                   "vds_grad_sumsq_multi")
        self._guard_done = True
        return rec

    def _step_guarded(self, plist, device, mult, b1, b2, eps):
        """the inherited guarded AdamW launch over the AdamW half, behind a record that covers every gradient"""
        if not self._muon_active:  # no Muon gradient this step: exactly the inherited sequence
            return super()._step_guarded(plist, device, mult, b1, b2, eps)
        lib, stream, d = _lib.load(), ops._stream(), self._dev
        rec = self._guard_all(device)
        fresh_before = {id(g) for g in {id(getattr(p, "_vds_group", None)): getattr(p, "_vds_group", None)
                                        for p, _ in plist}.values() if g is not None and g.shadow_fresh}
        ema = d["ema"].data_ptr() if d.get("ema") is not None else None
        if self._dev_scalars is not None:
            if not torch.cuda.is_current_stream_capturing():
                self._dev_scalars.copy_(self._scalars(mult))
            _lib.check(lib.vds_adamw_guarded_multi_dev(d["desc"].data_ptr(), d["ct"].data_ptr(), d["cs"].data_ptr(), d["n"],
                                                       CHUNK, b1, b2, eps, self._dev_scalars.data_ptr(), 1.0,
                                                       rec.data_ptr(), ema, stream), "vds_adamw_guarded_multi_dev")
        else:
            _lib.check(lib.vds_adamw_guarded_multi(d["desc"].data_ptr(), d["ct"].data_ptr(), d["cs"].data_ptr(), d["n"],
                                                   CHUNK, b1, b2, eps, self._step, mult, 1.0, rec.data_ptr(), ema,
                                                   self._ema_decay or 0.0, stream), "vds_adamw_guarded_multi")
        return fresh_before

    @torch.no_grad()
    def step(self, closure=None):
        assert closure is None
        mlist = self._muon_plist()
        self._muon_active = bool(mlist)
        if not mlist:
            with self._adam_groups_only():
                return super().step()
        alist = self._adam_plist()
        for p, _ in mlist:
            if not p.is_cuda:
                raise RuntimeError("MuonAdamW is a HIP kernel: parameters must be on the GPU")
            assert p.dtype == torch.float32 and p.grad.dtype == torch.float32
            assert p.data.is_contiguous() and p.grad.is_contiguous()
        device = mlist[0][0].device
        if self._ema_decay is not None and self._ema_swapped:
            raise RuntimeError("MuonAdamW.step() while the EMA is swapped in: leave ema_weights() / swap_ema() back first")
        for p, _ in mlist:  # first sight of a parameter: zero momentum; its EMA starts as a copy of it
            st = self.state[p]
            if "momentum_buffer" not in st or st["momentum_buffer"].shape != p.shape:
                st["momentum_buffer"] = torch.zeros_like(p.data, memory_format=torch.contiguous_format)
                self._muon_key = None
            if self._ema_decay is not None and ("ema" not in st or st["ema"].numel() != p.numel()):
                st["ema"] = p.data.detach().clone()
                self._muon_key = None
        groups = {id(getattr(p, "_vds_group", None)): getattr(p, "_vds_group", None) for p, _ in mlist}
        fresh_before = {i for i, g in groups.items() if g is not None and g.shadow_fresh}
        if self.guarded:
            akey = tuple((p.grad.data_ptr(), p.numel()) for p, _ in alist + mlist)
            if akey != self._all_key:
                self._build_all(alist + mlist, device)
                self._all_key = akey
        # ---- AdamW half (computes the guard record over every gradient on its way: _step_guarded above)
        self._guard_done = False
        if alist:
            with self._adam_groups_only():
                super().step()
        else:
            self._step += 1
        lrs, mult = self._muon_lr_plan(mlist)
        if not alist and self._dev_scalars is not None and not torch.cuda.is_current_stream_capturing():
            self._dev_scalars.copy_(self._scalars(mult))
        rec = None
        if self.guarded:
            rec = (self._guard_record(device) if self._guard_done else self._guard_all(device)).data_ptr()
        # ---- Muon half
        mkey = (tuple((p.data.data_ptr(), p.grad.data_ptr(), self.state[p]["momentum_buffer"].data_ptr(),
                       g["muon_split"], g["weight_decay"], g["momentum"], g["nesterov"], g["ns_steps"],
                       self._ema_decay is not None) for p, g in mlist), tuple(lrs))
        if mkey != self._muon_key:
            self._build_muon(mlist, lrs, device)
            self._muon_key = mkey
        sc = None if self._dev_scalars is None else self._dev_scalars.data_ptr()
        ws = self._muon_ws
        for (rows, cols, lr, wd, mu, nesterov, ns_steps), b in self._muon.items():
            for first, n in b["slices"]:
                tab = b["table"].data_ptr() + first * C.sizeof(_lib.MuonMat)
                ops.muon_momentum(tab, n, rows, cols, mu, nesterov, rec, ws)
                ops.muon_orthogonalize(ws, n, rows, cols, ns_steps)
                ops.muon_update(tab, n, rows, cols, lr, wd, mult, self._ema_decay or 0.0, sc, rec, ws)
        # the bf16 shadows of the Muon matrices are current again (same rule as the AdamW half: a step that may have
        # been skipped can only keep that claim, not establish it)
        for i, g in groups.items():
            if g is not None and (not self.skip_nonfinite or i in fresh_before):
                g.mark_shadow_fresh()
        return None
