"""Fused flat Adam for the BPMulT trunk.

The reference trains with `torch.optim.Adam(model.parameters(), lr=...)` (train.py:123-125), wraps it in
`ReduceLROnPlateau` (train.py:128-136), steps it after the backward pass (train.py:396-398) and stores
`optimizer.state_dict()` in its checkpoints (train.py:372-379).  Here every trunk parameter is a view into one flat fp32
master buffer and its gradient a view into one flat gradient buffer (engine.ParamStore), so the optimizer step for ~all
of the model is ONE streaming kernel (`bpm_adam_step_groups`) instead of a foreach loop over ~1700 tensors; the parameters
in no flat store -- the "tail": final GMU, head, front-ends, the BERT pooler, and by default all of `enc.*` -- go through an
ordinary torch.optim.Adam with the same hyper-parameters.  That tail is a few hundred KB with text features; with a real
text encoder it is ~109 M parameters in ~200 tensors unless `args.text_params = "flat"` puts the text parameters whose
gradients the HIP path produces into a flat store of their own (models/bert.py:build_text_store).  The optimizer steps EVERY
flat store of the model (`model._flat_stores()`) in one launch, `bpm_adam_step_sets`: one pair of moment buffers per
store, one segment table over all of them, one global gradient norm, one set of device step counters.  With one store the
launch is `bpm_adam_step_groups` as before.

`FusedAdam` IS a `torch.optim.Optimizer` (by default one param group holding every trainable model parameter), so LR
schedulers and the reference's checkpoint code accept it; every group's hyper-parameters are read at every step.

Parameter groups (per-group lr / betas / eps / weight decay, L2 or decoupled), parameters left out of every group, and a
step that skips itself when the gradient norm is not finite all stay that ONE launch over the flat buffers: the segment
table carries each segment's group, the groups' constants ride in the kernel arguments, and the skip decision is a device
float the norm reduction left behind.  The default construction is the same launch with one group.

Global-norm gradient clipping (`max_grad_norm`; upstream MulT calls `torch.nn.utils.clip_grad_norm_(model.parameters(), 0.8)`
before `optimizer.step()`) is part of the step: one reduction over the flat gradient buffer (`bpm_grad_sumsq`) leaves the
norm and the clip coefficient on the device, and the Adam kernel multiplies the coefficient into the gradients as it reads
them -- no second pass over the gradients, no host sync, no per-tensor loop.  `grad_norm(model)` is the readout alone.
"""
from __future__ import annotations

import math
from typing import List, Optional

import torch

from . import _lib, engine, ops


_HYPER = ("lr", "betas", "eps", "weight_decay", "decoupled_weight_decay")


class FusedAdam(torch.optim.Optimizer):
    """Drop-in for `torch.optim.Adam(params, lr, betas, eps, weight_decay, decoupled_weight_decay=...)` on a `bpmult_amd`
    model.

    Differences from torch.optim.Adam, all deliberate: trunk parameters that never receive a gradient keep a zero
    gradient instead of `None` (their update is exactly zero unless weight_decay > 0); `zero_grad()` clears the flat
    gradient buffer in place (fused into the step when `fused_zero_grad=True`); the moments are two flat buffers
    (`state_dict()["flat"]`; with a flat text store also `state_dict()["flat_text"]`: its moments and the names and offsets
    that say what lies where), not per-parameter tensors.  A checkpoint written with text_params = "torch" loads into an
    optimizer over a "flat" model: the per-parameter moments of its tail state are copied into the flat text moments by
    parameter name.  The reverse raises ValueError.

    `param_groups`: None (one group of every parameter that is trainable at construction), or torch-style dicts
    `{"params": [...], "lr": ..., "betas": ..., "eps": ..., "weight_decay": ..., "decoupled_weight_decay": ...}`; keys a
    dict leaves out take the constructor's values.  At most 16 groups; trunk and tail parameters may share one.  Every
    group keeps its own count of applied steps for the bias corrections (torch keeps one per parameter), so
    `add_param_group()` after `p.requires_grad_(True)` starts the new group at its step 1 with zero moments.  A model
    parameter that is in no group is NOT STEPPED: its master, both moments and every weight shadow derived from it keep
    their bits, and it does not count in the clip norm (its slice of the flat gradient buffer, which the backward
    launches still fill, is only cleared under `fused_zero_grad`).  `decoupled_weight_decay` (per group): p *= 1 - lr *
    wd first, then the Adam update on the undecayed gradient -- `torch.optim.AdamW`.  The trunk goes through ONE launch
    whatever the groups are (`bpm_adam_step_groups`: a block looks up its segment's group), the default construction's
    single group included.

    `max_grad_norm=c` clips the global gradient norm to c inside the step, as `torch.nn.utils.clip_grad_norm_(
    params, c)` in front of it would: ONE norm over the parameters of all groups, coefficient min(1, c / (norm + 1e-6)),
    a non-finite norm propagates as with error_if_nonfinite=False (unless `skip_nonfinite`).  `grad_scale` (GradSync's
    1 / world_size) acts BEFORE the clip: after a sum all-reduce the norm is that of the averaged gradient, the same on
    every rank.  The value lives in `param_groups[0]["max_grad_norm"]` (None: off) and travels with `state_dict()`; the
    copies torch's defaults place in the other groups are ignored.
    `last_grad_norm`: the norm before clipping of the latest step that took it, a 0-dim fp32 DEVICE tensor (None until
    then); reading it is the caller's sync -- `step()` itself never waits for the device.

    `skip_nonfinite=True`: every step takes the norm (so `last_grad_norm` is set without `max_grad_norm` too), and a
    step whose norm is NaN or +-inf changes nothing -- no parameter, moment or shadow of any group, trunk or tail, and no
    group's step count -- except that `skipped_steps` (a 0-dim int32 DEVICE tensor) goes up by one and the flat trunk
    gradients are still cleared under `fused_zero_grad` (the tail's `.grad`s are the caller's `zero_grad()`, as always;
    with clipping on they have been multiplied by the NaN / inf coefficient).  The flag is fixed at construction.  The decision, the counters and the bias corrections of later steps live on
    the device.  The tail then runs torch's FUSED Adam, which honours a device `found_inf` tensor and un-counts the
    step (what `torch.amp.GradScaler` uses); without the flag the tail is torch's default Adam as before."""

    def __init__(self, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 fused_zero_grad: bool = False, max_grad_norm: Optional[float] = None, decoupled_weight_decay: bool = False,
                 skip_nonfinite: bool = False, param_groups: Optional[List[dict]] = None):
        _check_max_norm(max_grad_norm)
        self.model = model
        self._name_of = {id(p): n for n, p in model.named_parameters()}
        self._group_steps: List[int] = []                    # applied steps per group, see _applied_steps(); add_param_group appends
        self._stale = True                                   # the groups changed: _regroup() before the next use
        if param_groups is None:
            groups = [p for p in model.parameters() if p.requires_grad]
        else:
            groups = [dict(g) for g in param_groups]
            if not groups:
                raise ValueError("param_groups is an empty list")
            if len(groups) > _lib.ADAM_MAX_GROUPS:
                raise ValueError(f"at most {_lib.ADAM_MAX_GROUPS} parameter groups, got {len(groups)}")
        super().__init__(groups, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                                      decoupled_weight_decay=bool(decoupled_weight_decay)))
        self.last_grad_norm: Optional[torch.Tensor] = None
        self.fused_zero_grad = fused_zero_grad
        self._skip_nonfinite = bool(skip_nonfinite)
        self.step_count = 0                                  # calls of step(), skipped ones included
        self.pending_grad_scale: Optional[float] = None      # set by distributed.GradSync.finish(): 1 / world_size
        # int32[16 + 1] on the device: under skip_nonfinite THE counts of applied steps (started from _group_steps, which
        # is not advanced from then on), and in its last word the skips
        self._counters: Optional[torch.Tensor] = None
        self._m: Optional[torch.Tensor] = None              # the trunk store's moments
        self._v: Optional[torch.Tensor] = None
        self._store_id = None
        # every flat store of the model (model._flat_stores(): the trunk's, then the text encoder's under text_params =
        # "flat"), one pair of moment buffers per store ([0] is _m / _v) and what the one launch over all of them takes
        self._stores: list = []
        self._ms: List[torch.Tensor] = []
        self._vs: List[torch.Tensor] = []
        self._store_ids: tuple = ()
        self._sets = None
        self._norm_multi = None
        self._tail_opt = None
        self._tail_gi: List[int] = []                        # tail group -> index of the group it mirrors

    # hyper-parameters live in the param groups (what schedulers write)
    @property
    def lr(self) -> float:
        return self.param_groups[0]["lr"]

    @property
    def skip_nonfinite(self) -> bool:
        """Fixed at construction: it decides where the step counts live and which torch Adam steps the tail."""
        return self._skip_nonfinite

    @property
    def skipped_steps(self) -> torch.Tensor:
        """Steps skipped for a non-finite gradient norm: a 0-dim int32 device tensor (reading it is the caller's sync)."""
        self._store()
        if self._counters is None:
            self._counters = torch.zeros(_lib.ADAM_MAX_GROUPS + 1, device=self._m.device, dtype=torch.int32)
        return self._counters[_lib.ADAM_MAX_GROUPS]

    def add_param_group(self, param_group: dict) -> None:
        """torch's add_param_group with this optimizer's rules (ValueError naming the offender): at most 16 groups, no
        empty group, parameters of the model only (by identity), each in one group, none with requires_grad == False.
        A group added after construction starts with zero moments and its own step count 0; the launch table is rebuilt
        at the next step."""
        if not isinstance(param_group, dict):
            raise TypeError(f"param_group must be a dict, got {type(param_group).__name__}")
        g = dict(param_group)
        ps = g.get("params")
        ps = [ps] if isinstance(ps, torch.Tensor) else list(ps if ps is not None else [])
        gi = len(self.param_groups)
        if gi >= _lib.ADAM_MAX_GROUPS:
            raise ValueError(f"at most {_lib.ADAM_MAX_GROUPS} parameter groups: group {gi} is one too many")
        if not ps:
            raise ValueError(f"parameter group {gi} is empty")
        seen = {id(p) for grp in self.param_groups for p in grp["params"]}
        for p in ps:
            name = self._name_of.get(id(p)) if isinstance(p, torch.Tensor) else None
            if name is None:
                what = f"a tensor of shape {tuple(p.shape)}" if isinstance(p, torch.Tensor) else repr(type(p).__name__)
                raise ValueError(f"parameter group {gi}: {what} is not a parameter of the model")
            if id(p) in seen:
                raise ValueError(f"parameter {name} (group {gi}) is in more than one parameter group")
            if not p.requires_grad:
                raise ValueError(f"parameter {name} (group {gi}) has requires_grad == False: leave it out of the groups")
            seen.add(id(p))
        g["params"] = ps
        if "betas" in g:
            g["betas"] = tuple(g["betas"])
        super().add_param_group(g)
        self._group_steps.append(0)
        self._stale = True

    # -- plumbing ---------------------------------------------------------------
    def _store(self):
        flat = getattr(self.model, "_flat_stores", None)
        stores = flat() if flat is not None else [self.model._ensure_store()]
        ids = tuple(id(st) for st in stores)
        if ids != self._store_ids:                         # (re)built after .to()/.cuda(): restart that store's moments
            ms, vs = [], []
            for i, st in enumerate(stores):
                if i < len(self._store_ids) and self._store_ids[i] == ids[i]:
                    ms.append(self._ms[i])
                    vs.append(self._vs[i])
                else:
                    ms.append(torch.zeros_like(st.master))
                    vs.append(torch.zeros_like(st.master))
            self._stores, self._ms, self._vs, self._store_ids = stores, ms, vs, ids
            self._m, self._v, self._store_id = ms[0], vs[0], ids[0]
            self._sets = self._norm_multi = None
            self._tail_opt, self._tail_gi, self._stale = None, [], True
        st = stores[0]
        if self._stale:
            self._regroup(st)
        if self.skip_nonfinite and self._counters is None:
            self._counters = torch.zeros(_lib.ADAM_MAX_GROUPS + 1, device=st.master.device, dtype=torch.int32)
            self._counters[:len(self._group_steps)] = torch.tensor(self._group_steps, dtype=torch.int32)
        return st

    def _regroup(self, st) -> None:
        """Flat stores: {name: group} per store for the grouped launch table and the norm's parameter set.  Tail (what is
        in no store): one torch.optim.Adam whose groups mirror the caller's (same membership order); a group added later
        is added there too, so the state of the earlier ones stays."""
        group_ofs = [{} for _ in self._stores]
        for gi, g in enumerate(self.param_groups):
            tail = []
            for p in g["params"]:
                n = self._name_of[id(p)]
                for group_of, store in zip(group_ofs, self._stores):
                    if n in store.params:
                        group_of[n] = gi
                        break
                else:
                    tail.append(p)
            if not tail or gi in self._tail_gi:
                continue
            tg = dict(params=tail, **{k: g[k] for k in _HYPER})
            if self._tail_opt is None:
                self._tail_opt = torch.optim.Adam([tg], fused=True) if self.skip_nonfinite else torch.optim.Adam([tg])
            else:
                self._tail_opt.add_param_group(tg)
            self._tail_gi.append(gi)
        if not any(group_ofs):
            raise ValueError("no parameter of the flat trunk buffers is in any parameter group: FusedAdam steps the trunk "
                             "(and the tail beside it); for tail parameters alone use torch.optim.Adam")
        self._group_ofs = group_ofs
        self._group_of = group_ofs[0]
        self._group_table = None                           # the segment table of the launch: built by the next step
        self._norm_multi = None
        self._trunk_set = frozenset(group_ofs[0])
        self._all_trunk = len(group_ofs[0]) == len(st.params)
        self._stale = False

    def _grad_sumsq(self, grad_scale: float, max_norm: float, extra: Optional[torch.Tensor]) -> torch.Tensor:
        """[total_norm, coef] on the device (ParamStore.grad_sumsq).  Several stores: ONE reduction whose table spans every
        store's gradient buffer (bpm_grad_sumsq takes absolute addresses), over the parameters this optimizer steps."""
        if len(self._stores) == 1:
            return self._stores[0].grad_sumsq(grad_scale, max_norm, extra, names=None if self._all_trunk else self._trunk_set)
        if self._norm_multi is None:
            self._norm_multi = _norm_over(self._stores, [lambda n, g=g: n in g for g in self._group_ofs])
        table, ws, out = self._norm_multi
        ops.grad_sumsq(*table, ws, out, grad_scale, max_norm, extra)
        return out

    def _applied_steps(self) -> List[int]:
        if self._counters is not None and self.skip_nonfinite:
            return [int(x) for x in self._counters[:len(self.param_groups)].tolist()]      # the caller's sync
        return list(self._group_steps)

    def zero_grad(self, set_to_none: bool = False) -> None:
        self._store()
        for st in self._stores:
            st.gflat.zero_()
        if self._tail_opt is not None:
            self._tail_opt.zero_grad(set_to_none=set_to_none)

    @torch.no_grad()
    def step(self, closure=None, grad_scale: Optional[float] = None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        st = self._store()
        g = self.param_groups[0]
        if grad_scale is None:
            grad_scale = self.pending_grad_scale if self.pending_grad_scale is not None else 1.0
        self.pending_grad_scale = None
        self.step_count += 1
        if any(s.master.numel() % 4 for s in self._stores):
            raise RuntimeError("flat parameter buffer is not a multiple of 4 elements")
        clip = g.get("max_grad_norm")
        tail = [p for tg in self._tail_opt.param_groups for p in tg["params"]] if self._tail_opt is not None else []
        coef = norm = None
        if clip is not None or self.skip_nonfinite:
            # the trunk's share: one reduction over gflat (the store's own table when every trunk parameter is stepped); the
            # tail's (PyTorch-owned parameters) through torch; one root.  Norm and coefficient stay on the device: the Adam
            # kernel and the tail read them there.
            _check_max_norm(clip)
            tail_grads = [p.grad for p in tail if p.grad is not None]
            res = self._grad_sumsq(grad_scale, float(clip) if clip is not None else 0.0, _sumsq(tail_grads))
            self.last_grad_norm = res[0].clone()
            coef = res[1:2] if clip is not None else None
            norm = res[0:1] if self.skip_nonfinite else None
        # one launch: the update of every trunk parameter AND the CT shadows of the plain weight matrices, written from
        # the updated masters as they are stored (no second pass over the flat master for the next forward's operands)
        if norm is None:                                   # (under skip_nonfinite the counts live on the device)
            self._group_steps = [s + 1 for s in self._group_steps]
        hyper = ops.adam_groups([dict(pg, step=s) for pg, s in zip(self.param_groups, self._group_steps)])
        dev = dict(scale_dev=coef, norm_dev=norm, steps_dev=None if norm is None else self._counters,
                   skipped_dev=None if norm is None else self._counters[_lib.ADAM_MAX_GROUPS:])
        if len(self._stores) == 1:
            if self._group_table is None:
                self._group_table = st.adam_group_table(self._group_of)
            st.adam_step_groups(self._m, self._v, self._group_table, hyper, grad_scale, self.fused_zero_grad, **dev)
        else:                                              # every store in the same launch: bpm_adam_step_sets
            if self._group_table is None:
                self._group_table = engine.adam_sets_table(self._stores, self._group_ofs)
            if self._sets is None:
                self._sets = ops.adam_sets([(s.master, s.gflat, m, v) for s, m, v in zip(self._stores, self._ms, self._vs)])
            engine.adam_step_sets(self._stores, self._group_table, self._sets, hyper, grad_scale, self.fused_zero_grad, **dev)
        if self._tail_opt is not None:
            for tg, gi in zip(self._tail_opt.param_groups, self._tail_gi):
                for k in _HYPER:
                    tg[k] = self.param_groups[gi][k]
            if coef is not None:
                if tail_grads:
                    torch._foreach_mul_(tail_grads, coef[0] * grad_scale)      # grad_scale and the clip in one multiply
            elif grad_scale != 1.0:
                for p in tail:
                    if p.grad is not None:
                        p.grad.mul_(grad_scale)
            if norm is not None:                           # torch's fused Adam: no update and the step un-counted when set
                self._tail_opt.found_inf = torch.isfinite(res[0]).logical_not().float()
            self._tail_opt.step()
        return loss

    def _load_tail(self, tail_sd) -> None:
        self._tail_opt.load_state_dict(tail_sd)
        _tail_flavour(self._tail_opt, self.skip_nonfinite)

    def _group_names(self, gi: int) -> List[str]:
        return [self._name_of[id(p)] for p in self.param_groups[gi]["params"]]

    def state_dict(self):
        """`step`: the applied steps of group 0; `group_steps`: of every group; `skipped`: the skip count (under
        skip_nonfinite reading them waits for the device: the caller's checkpoint, not the step); `step_calls`: calls of
        step(); `param_groups`: one dict per group, the hyper-parameters plus `param_names` (the model's names, in order)."""
        self._store()                                      # the moments exist (zeros) even before the first step
        steps = self._applied_steps()
        skipped = int(self._counters[_lib.ADAM_MAX_GROUPS]) if self._counters is not None else 0
        return {"step": steps[0], "group_steps": steps, "skipped": skipped, "step_calls": self.step_count,
                "flat": {"exp_avg": self._m, "exp_avg_sq": self._v},
                **self._flat_text_state(),
                "tail": self._tail_opt.state_dict() if self._tail_opt is not None else None,
                "dropout_step": int(getattr(self.model, "dropout_step", 0)),
                "param_groups": [dict({k: v for k, v in g.items() if k != "params"}, param_names=self._group_names(gi))
                                 for gi, g in enumerate(self.param_groups)]}

    def _flat_text_state(self) -> dict:
        """`flat_text`: the moments of the text encoder's flat store (text_params = "flat") with the names and offsets that
        say what lies where; absent without such a store."""
        if len(self._stores) < 2:
            return {}
        st = self._stores[1]
        return {"flat_text": {"exp_avg": self._ms[1], "exp_avg_sq": self._vs[1], "names": list(st.names),
                              "offsets": [st.off[n] for n in st.names]}}

    def _load_flat_text(self, sd) -> Optional[dict]:
        """Restores the text store's moments; returns the tail state to load (the checkpoint's, or what is left of it).
        A checkpoint written with text_params = "torch" holds them per parameter in its tail state: they are copied into
        the flat moments by parameter name and taken out of the tail state, so a run may turn the switch on at a resume."""
        tail_sd, ft = sd.get("tail"), sd.get("flat_text")
        if len(self._stores) < 2:
            if ft is not None:
                raise ValueError("the checkpoint was written with text_params='flat' (it holds 'flat_text' moments), this model "
                                 "runs text_params='torch': loading in that direction is not supported -- build the model with "
                                 "text_params='flat'")
            return tail_sd
        st, m, v = self._stores[1], self._ms[1], self._vs[1]
        if ft is not None:
            if list(ft["names"]) != list(st.names) or list(ft["offsets"]) != [st.off[n] for n in st.names]:
                raise ValueError("flat_text: the checkpoint's text parameters or their offsets differ from this model's text store")
            m.copy_(ft["exp_avg"])
            v.copy_(ft["exp_avg_sq"])
            return tail_sd
        m.zero_()
        v.zero_()
        if tail_sd is None:
            return None
        groups = sd["param_groups"]
        if any("param_names" not in g for g in groups):
            raise ValueError("the checkpoint names no parameters: its tail state cannot be moved into the flat text moments")
        trunk = self._stores[0].params
        saved = [[n for n in g["param_names"] if n not in trunk] for g in groups]          # the saving optimizer's tail groups
        saved = [names for names in saved if names]
        if len(saved) != len(tail_sd["param_groups"]) or any(len(a) != len(b["params"]) for a, b in zip(saved, tail_sd["param_groups"])):
            raise ValueError("the checkpoint's tail state does not match its parameter names")
        state, new_groups, new_state, k = tail_sd["state"], [], {}, 0
        for names, tg in zip(saved, tail_sd["param_groups"]):
            keep = []
            for n, idx in zip(names, tg["params"]):
                if n in st.params:
                    if idx in state:
                        a, cnt = st.off[n], st.params[n].numel()
                        m[a:a + cnt].copy_(state[idx]["exp_avg"].reshape(-1))
                        v[a:a + cnt].copy_(state[idx]["exp_avg_sq"].reshape(-1))
                else:
                    if idx in state:
                        new_state[k] = state[idx]
                    keep.append(k)
                    k += 1
            if keep:
                new_groups.append(dict(tg, params=keep))
        return {"state": new_state, "param_groups": new_groups} if new_groups else None

    def load_state_dict(self, sd) -> None:
        """Restores what state_dict() wrote.  A checkpoint written before parameter groups existed (no `param_names`, no
        `group_steps`) loads too: every group takes its `step`.  ValueError when the number of groups or a group's
        parameter names differ from this optimizer's."""
        groups = sd["param_groups"]
        if len(groups) != len(self.param_groups):
            raise ValueError(f"the checkpoint has {len(groups)} parameter groups, this optimizer {len(self.param_groups)}")
        for gi, theirs in enumerate(groups):
            if "param_names" in theirs and list(theirs["param_names"]) != self._group_names(gi):
                raise ValueError(f"parameter group {gi}: the checkpoint's parameter names differ from this optimizer's")
        steps = sd.get("group_steps")
        steps = [int(sd["step"])] * len(groups) if steps is None else [int(s) for s in steps]
        if len(steps) != len(groups):
            raise ValueError(f"the checkpoint has {len(steps)} group step counts for {len(groups)} parameter groups")
        self._store()
        self._group_steps = steps
        self.step_count = int(sd.get("step_calls", sd["step"]))
        if self._counters is not None or sd.get("skipped"):
            self.skipped_steps                             # (allocates the counters)
            self._counters.zero_()
            self._counters[:len(steps)] = torch.tensor(steps, dtype=torch.int32)
            self._counters[_lib.ADAM_MAX_GROUPS] = int(sd.get("skipped", 0))
        self._m.copy_(sd["flat"]["exp_avg"])
        self._v.copy_(sd["flat"]["exp_avg_sq"])
        tail_sd = self._load_flat_text(sd)
        if self._tail_opt is not None and tail_sd is not None:
            self._load_tail(tail_sd)
        if hasattr(self.model, "dropout_step"):
            self.model.dropout_step = int(sd.get("dropout_step", 0))
        for mine, theirs in zip(self.param_groups, groups):
            for k, v in theirs.items():
                if k != "param_names":
                    mine[k] = tuple(v) if k == "betas" else v


def _tail_flavour(opt: torch.optim.Adam, fused: bool) -> None:
    """torch's load_state_dict takes every group option from the saved groups, `fused` included, and leaves each `step`
    where that flavour keeps it.  Put the tail back to THIS optimizer's flavour: fused Adam with float32 device steps
    under skip_nonfinite, the default Adam with host steps otherwise."""
    for tg in opt.param_groups:
        tg["fused"], tg["foreach"] = (True if fused else None), None
        for p in tg["params"]:
            s = opt.state.get(p)
            if s and "step" in s:
                s["step"] = torch.as_tensor(s["step"], dtype=torch.float32).to(p.device if fused else "cpu")


def decay_groups(model, weight_decay: float, **overrides) -> List[dict]:
    """The usual two parameter groups over the model's TRAINABLE parameters: matrices and everything else with
    ndim >= 2 take `weight_decay`, vectors (ndim <= 1: biases, LayerNorm affines) take 0.  `overrides` (lr, betas, eps,
    decoupled_weight_decay, ...) go into both dicts."""
    ps = [p for p in model.parameters() if p.requires_grad]
    return [dict(overrides, params=[p for p in ps if p.ndim >= 2], weight_decay=weight_decay),
            dict(overrides, params=[p for p in ps if p.ndim <= 1], weight_decay=0.0)]


def _check_max_norm(x) -> None:
    if x is None:
        return
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or x <= 0:
        raise ValueError(f"max_grad_norm must be None or a finite number above 0, got {x!r}")


def _sumsq(grads: List[torch.Tensor]) -> Optional[torch.Tensor]:
    """Sum of squares of a list of gradients as one fp32 device scalar (None for an empty list), the way
    torch.nn.utils.clip_grad_norm_ takes it: per-tensor 2-norms (torch._foreach_norm), then their squares summed."""
    if not grads:
        return None
    return torch.stack(torch._foreach_norm(grads)).float().square().sum().reshape(1)


@torch.no_grad()
def grad_norm(model, grad_scale: float = 1.0) -> torch.Tensor:
    """Global 2-norm of the model's gradients times grad_scale, as a 0-dim fp32 device tensor: what
    `torch.nn.utils.clip_grad_norm_(model.parameters(), inf)` would return, without its per-tensor loop over the trunk
    (one reduction over the flat gradient buffer; the few tail parameters through torch) and without a host sync.
    Modifies nothing: for logging in loops that keep their own optimizer.  RuntimeError before the first backward."""
    flat = getattr(model, "_flat_stores", None)
    stores = flat() if flat is not None else [model._ensure_store()]
    st = stores[0]
    tail = [p.grad for n, p in model.named_parameters()
            if not any(n in s.params for s in stores) and p.requires_grad and p.grad is not None]
    if st._fresh():                                        # the flat gradient buffer holds nothing current
        raise RuntimeError("grad_norm: no gradients yet (call backward first)")
    if len(stores) == 1:
        return st.grad_sumsq(float(grad_scale), 0.0, _sumsq(tail))[0].clone()
    cached = getattr(model, "_grad_norm_tables", None)
    if cached is None or len(cached[0]) != len(stores) or any(a is not b for a, b in zip(cached[0], stores)):
        # one table over every store, built once per set of stores (which it keeps alive: the table holds their addresses)
        cached = model._grad_norm_tables = (stores, _norm_over(stores, [lambda n, s=s: s.params[n].requires_grad for s in stores]))
    table, ws, out = cached[1]
    ops.grad_sumsq(*table, ws, out, float(grad_scale), 0.0, _sumsq(tail))
    return out[0].clone()


def _norm_over(stores, counts):
    """(table, workspace, result) of one bpm_grad_sumsq launch over the gradient buffers of several stores: the slices of
    the parameters counts[i](name) admits in store i, in store order."""
    ranges = [r for s, c in zip(stores, counts) for r in s.norm_ranges(c)]
    if not ranges:
        raise RuntimeError("gradient norm: no trainable parameter in the flat buffers")
    table = ops.sumsq_table(ranges)
    dev = stores[0].device
    return (table, torch.empty(ops.grad_sumsq_ws_bytes(table[2]) // 4, device=dev, dtype=torch.float32),
            torch.zeros(2, device=dev, dtype=torch.float32))
