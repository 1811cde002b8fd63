"""Training-loop plumbing around the hot path, mirroring the reference's train.py so that a run can swap the model in
unchanged.  Data loading stays the caller's (out of scope): the loop takes an iterable
of batches, a `forward_loss(model, batch)` callable and an `evaluate(model)` callable that returns the tuning metric
(`make_evaluate` builds one over `model_eval`, the reference's evaluation on the HIP path).

Reference behaviour reproduced (file:line in /root/reference/bpmult):
* checkpoints: `save_checkpoint(state, is_best, path)` writes `checkpoint.pt` and copies it to `model_best.pt`
  (utils/utils.py:21-25); the dict holds epoch / state_dict / optimizer / scheduler / n_no_improve / best_metric
  (train.py:419-430); `load_checkpoint(model, path)` reads `["state_dict"]` (utils/utils.py:28-30).  A checkpoint saved
  from the reference's `nn.DataParallel` wrapper (train.py:354-356) prefixes every key with `module.`: stripped here.
* resume: `checkpoint.pt` in the save directory restores epoch, counters, model (strict=False), optimizer and scheduler
  (train.py:372-379).
* epoch loop: zero_grad, loss / accumulation steps, backward, step every `gradient_accumulation_steps` (train.py:382-398);
  `scheduler.step(tuning_metric)` with ReduceLROnPlateau (train.py:128-136, 410); improvement is `>=` (`<=` when the
  metric is minimised, train.py:411-414); a checkpoint is written on improvement only; stop when
  `n_no_improve >= patience` (train.py:432-439).
* the five-seed outer loop `for i in range(from_seed, 6)` with `inverse_seed` (train.py:490-503).
* the criterion: `get_criterion(args)` (train.py:99-120), torch's modules or, with `args.criterion = "hip"`, their
  subclasses in losses.py.
* evaluation: `model_eval` (train.py:165-280) with the reference's dict per task, over metrics.Evaluator.
"""
from __future__ import annotations

import os
import shutil
from typing import Callable, Dict, Iterable, Optional, Tuple

import torch


def strip_module_prefix(state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Keys of a DataParallel / DistributedDataParallel wrapper -> keys of the wrapped model."""
    if state_dict and all(k.startswith("module.") for k in state_dict):
        return {k[len("module."):]: v for k, v in state_dict.items()}
    return dict(state_dict)


def load_reference_checkpoint(model, src, strict: bool = True, map_location="cpu") -> Tuple[list, list]:
    """Load a reference `checkpoint.pt` / `model_best.pt` (a dict with "state_dict"), a bare state_dict, or a path to
    either, into a bpmult_amd model.  Returns (missing_keys, unexpected_keys)."""
    if isinstance(src, (str, os.PathLike)):
        src = torch.load(src, map_location=map_location, weights_only=False)
    sd = src["state_dict"] if isinstance(src, dict) and "state_dict" in src else src
    res = model.load_state_dict(strip_module_prefix(sd), strict=strict)
    return list(res.missing_keys), list(res.unexpected_keys)


def load_checkpoint(model, path) -> None:
    """utils/utils.py:28-30."""
    load_reference_checkpoint(model, path)


def save_checkpoint(state: dict, is_best: bool, checkpoint_path: str, filename: str = "checkpoint.pt") -> None:
    """utils/utils.py:21-25."""
    os.makedirs(checkpoint_path, exist_ok=True)
    filename = os.path.join(checkpoint_path, filename)
    torch.save(state, filename)
    if is_best:
        shutil.copyfile(filename, os.path.join(checkpoint_path, "model_best.pt"))


def get_scheduler(optimizer, lr_patience: int = 2, lr_factor: float = 0.5, mode: str = "max"):
    """train.py:128-136."""
    return torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode, patience=lr_patience, factor=lr_factor)


def get_criterion(args):
    """train.py:99-120: BCE-with-logits for multilabel tasks, cross-entropy otherwise, both weighted by the inverse label
    frequencies `(freqs / train_data_len) ** -1` under `args.weight_classes` -- except for cmu-mosi, which is never
    weighted and trains its non-multilabel form on L1.  `args.criterion`: "torch" (default) returns torch's own modules,
    "hip" the HIP-path subclasses of losses.py.  The weights are a buffer of the module: move it with `.to(device)` (the
    reference's `.cuda()` at construction is not reproduced)."""
    backend = getattr(args, "criterion", "torch")
    if backend not in ("torch", "hip"):
        raise ValueError(f"args.criterion: expected 'torch' or 'hip', got {backend!r}")
    if backend == "hip":
        from . import losses as L
    else:
        L = torch.nn
    weighted = bool(args.weight_classes) and args.task != "cmu-mosi"
    label_weights = None
    if weighted:
        freqs = [args.label_freqs[l] for l in args.labels]
        label_weights = (torch.FloatTensor(freqs) / args.train_data_len) ** -1
    if args.task_type == "multilabel":
        return L.BCEWithLogitsLoss(pos_weight=label_weights) if weighted else L.BCEWithLogitsLoss()
    if weighted:
        return L.CrossEntropyLoss(weight=label_weights)
    return L.L1Loss() if args.task == "cmu-mosi" else L.CrossEntropyLoss()


def fit(model, optimizer, scheduler, train_batches: Callable[[], Iterable], forward_loss: Callable, evaluate: Callable,
        savedir: str, max_epochs: int, patience: int, gradient_accumulation_steps: int = 1, minimise: bool = False,
        grad_sync=None, log: Optional[Callable[[str], None]] = None, process_group=None) -> dict:
    """The reference's train() epoch loop (train.py:370-439) around any model / optimizer pair.

    train_batches() yields the batches of one epoch; forward_loss(model, batch) returns the scalar loss;
    evaluate(model) returns the tuning metric of the validation split.  grad_sync: an optional
    distributed.GradSync -- only the last micro-step of an accumulation group exchanges gradients.

    process_group (data parallelism, one process per GPU, all ranks on one save directory): only rank 0 writes the
    checkpoints and every rank waits behind the write (a barrier per epoch); whether to resume is rank 0's decision,
    broadcast, every rank then restores from checkpoint.pt, and a barrier keeps the first write behind the last read.
    `evaluate` must return the same metric on every rank (make_evaluate(..., process_group=...) does): then
    scheduler, best metric, n_no_improve and the stop decision stay identical on all ranks."""
    log = log or (lambda s: None)
    writer = True
    if process_group is not None:
        import torch.distributed as dist
        writer = _eval_world(process_group)[1] == 0
    start_epoch, global_step, n_no_improve = 0, 0, 0
    best_metric = float("inf") if minimise else -float("inf")
    ck = os.path.join(savedir, "checkpoint.pt")
    resume = os.path.exists(ck)
    if process_group is not None:
        # whether to resume is rank 0's decision, taken before anybody can write: a rank that arrives late must not find
        # (and resume from) the file that rank 0 has written for the first epoch in the meantime
        flag = [resume]
        dist.broadcast_object_list(flag, src=dist.get_global_rank(process_group, 0), group=process_group)
        resume = flag[0]
    if resume:
        c = torch.load(ck, map_location="cpu", weights_only=False)
        start_epoch, n_no_improve, best_metric = c["epoch"], c["n_no_improve"], c["best_metric"]
        model.load_state_dict(strip_module_prefix(c["state_dict"]), strict=False)
        optimizer.load_state_dict(c["optimizer"])
        scheduler.load_state_dict(c["scheduler"])
    if process_group is not None:
        dist.barrier(group=process_group)           # every rank has read the file before rank 0 may replace it
    history = []
    for i_epoch in range(start_epoch, max_epochs):
        losses = []
        model.train()
        optimizer.zero_grad()
        for batch in train_batches():
            loss = forward_loss(model, batch)
            if gradient_accumulation_steps > 1:
                loss = loss / gradient_accumulation_steps
            losses.append(float(loss.detach()))
            last = (global_step + 1) % gradient_accumulation_steps == 0
            if grad_sync is not None:
                grad_sync.active = last
            loss.backward()
            if grad_sync is not None:
                grad_sync.finish()
            global_step += 1
            if last:
                optimizer.step()
                optimizer.zero_grad()
        model.eval()
        with torch.no_grad():
            tuning_metric = float(evaluate(model))
        log(f"epoch {i_epoch}: train loss {sum(losses) / max(len(losses), 1):.4f}, tuning metric {tuning_metric:.4f}")
        scheduler.step(tuning_metric)
        is_improvement = tuning_metric <= best_metric if minimise else tuning_metric >= best_metric
        if is_improvement:
            best_metric, n_no_improve = tuning_metric, 0
        else:
            n_no_improve += 1
        history.append({"epoch": i_epoch, "loss": sum(losses) / max(len(losses), 1), "metric": tuning_metric,
                        "lr": optimizer.param_groups[0]["lr"], "improved": is_improvement})
        if is_improvement and writer:
            save_checkpoint({"epoch": i_epoch + 1, "state_dict": model.state_dict(), "optimizer": optimizer.state_dict(),
                             "scheduler": scheduler.state_dict(), "n_no_improve": n_no_improve, "best_metric": best_metric},
                            is_improvement, savedir)
        if process_group is not None:
            dist.barrier(group=process_group)       # nobody runs ahead of (or resumes from) a file half written
        if n_no_improve >= patience:
            log("No improvement. Breaking out of loop.")
            break
    return {"best_metric": best_metric, "epochs_run": len(history), "history": history, "global_step": global_step}


def run_seeds(run_one: Callable[[int], object], from_seed: int = 1, inverse_seed: bool = False) -> Dict[int, object]:
    """train.py:490-503: seeds from_seed..5 (or 6 - i when inverse_seed)."""
    out = {}
    for i in range(from_seed, 6):
        seed = 6 - i if inverse_seed else i
        out[seed] = run_one(seed)
    return out


# ----------------------------------------------------------------------------
# batch formats (data/helpers.py:78-137, train.py:283-321): the loaders themselves are out of scope
# ----------------------------------------------------------------------------
def collate_fn(batch, model: str, task_type: str = "multilabel", with_poster: bool = True):
    """Rows as the reference's datasets yield them -- (tokens, segment, img, tgt, audio[, poster]) -- to the batch tuple
    of data/helpers.py:129-133: (text, segment, mask, img, tgt, audio[, poster]).  Text is right-padded with zeros to the
    longest row (mask = 1 on real tokens); audio is cropped to the batch-minimum length along its last axis
    (helpers.py:100-102, 106-110)."""
    bsz = len(batch)
    lens = [len(row[0]) for row in batch]
    max_len = max(lens)
    text = torch.zeros(bsz, max_len, dtype=torch.long)
    segment = torch.zeros(bsz, max_len, dtype=torch.long)
    mask = torch.zeros(bsz, max_len, dtype=torch.long)
    for i, (row, n) in enumerate(zip(batch, lens)):
        text[i, :n], segment[i, :n], mask[i, :n] = row[0], row[1], 1
    img = torch.stack([row[2] for row in batch])
    tgt = torch.stack([row[3] for row in batch]) if task_type == "multilabel" else torch.cat([row[3] for row in batch]).long()
    min_len = min(row[4].shape[1] for row in batch)
    audio = torch.stack([row[4][..., :min_len] for row in batch])
    if model == "mmtrvapt":
        poster = torch.stack([row[5] for row in batch]) if with_poster else None
        return text, segment, mask, img, tgt, audio, poster
    return text, segment, mask, img, tgt, audio


def model_forward(model, criterion, batch, model_name: str, gmu_gate: bool = False):
    """train.py:283-335 for the two hot-path models: note the argument order (txt, MASK, SEGMENT, ...) against the
    batch order (text, SEGMENT, MASK, ...).  Returns (loss, out, tgt[, gates])."""
    dev = next(model.parameters()).device
    if model_name == "mmtrvapt":
        txt, segment, mask, img, tgt, audio, poster = batch
        args = (txt.to(dev), mask.to(dev), segment.to(dev), img.to(dev), audio.to(dev), poster.to(dev))
    else:
        txt, segment, mask, img, tgt, audio = batch
        args = (txt.to(dev), mask.to(dev), segment.to(dev), img.to(dev), audio.to(dev))
    if gmu_gate:
        out, gates = model(*args, True)
    else:
        out, gates = model(*args), None
    tgt = tgt.to(dev)
    loss = criterion(out, tgt)
    return (loss, out, tgt, gates) if gmu_gate else (loss, out, tgt)


# ----------------------------------------------------------------------------
# evaluation (train.py:165-280) over metrics.Evaluator: one host read per evaluation
# ----------------------------------------------------------------------------
def eval_kind(args) -> str:
    """The metrics.Evaluator kind of a task: BCE tasks are "multilabel", cmu-mosi is "regression", the other
    cross-entropy tasks are "classes"."""
    if args.task_type == "multilabel":
        if args.task == "cmu-mosi":
            raise ValueError("task: cmu-mosi with task_type 'multilabel' is not evaluated here (the reference builds its targets "
                             "with a tensordot over 101 bins, train.py:324-326, which this library does not)")
        return "multilabel"
    return "regression" if args.task == "cmu-mosi" else "classes"


def arrange_metrics(args, m: dict) -> dict:
    """Evaluator.compute()'s primitives -> the reference's dict, with the reference's keys per task, mislabelled ones
    included: under mmimdb `micro_f1` holds the micro average precision and `auc_pr_macro` the weighted F1
    (train.py:206-211); under cmu-mosei `wacc_emos` holds the micro average precision and `auc_pr_micro` the mean weighted
    accuracy (train.py:254-255); in the else-branch `weight_f1` is the mean absolute error (train.py:270).

    Departures: a multilabel task for which the reference has no branch (iemocap: its model_eval returns the loss alone
    and train() then fails on the missing tuning metric) gets the cmu-mosei form over its C classes; the cross-entropy
    tasks also get `acc` (argmax == target); the argmax is taken over the logits, not over their fp32 softmax."""
    out = {"loss": m["loss"]}
    if args.task_type == "multilabel":
        eval_kind(args)
        f1, ap = m["f1"], m["ap"]
        if args.task == "moviescope":
            out.update(macro_f1=f1["macro"], micro_f1=f1["micro"], auc_pr_macro=ap["macro"], auc_pr_micro=ap["micro"],
                       auc_pr_samples=ap["samples"])
        elif args.task == "mmimdb":
            out.update(macro_f1=f1["macro"], micro_f1=ap["micro"], auc_pr_macro=f1["weighted"], auc_pr_micro=f1["micro"],
                       auc_pr_samples=f1["samples"])
        elif args.task == "counseling":
            if len(m["wf1"]) != 2:
                raise ValueError(f"n_classes: counseling is evaluated over exactly 2 classes, got {len(m['wf1'])}")
            out.update(f1_low=float(m["wf1"][1]), f1_high=float(m["wf1"][0]), acc=m["subset_accuracy"], auc_pr_micro=ap["micro"])
        else:
            n = len(m["wf1"])
            if args.task == "cmu-mosei" and n != 6:
                raise ValueError(f"n_classes: cmu-mosei is evaluated over exactly 6 classes, got {n}")
            for i in range(n):
                out[f"f1_emo{i + 1}"] = float(m["wf1"][i])
            for i in range(n):
                out[f"wacc_emo{i + 1}"] = float(m["wacc"][i])
            out["f1_emos"] = float(sum(m["wf1"]) / n)
            out["wacc_emos"] = ap["micro"]
            out["auc_pr_micro"] = float(sum(m["wacc"]) / n)
        return out
    out.update(mae=m["mae"], corr=m["corr"], accuracy_7=m["accuracy_7"], weighted_f1=m["weighted_f1"], weight_f1=m["mae"])
    if args.task != "cmu-mosi":
        out["acc"] = m["acc"]
    return out


def shard_range(n_batches: int, world: int, rank: int) -> Tuple[int, int]:
    """Rank `rank`'s share [lo, hi) of n_batches batches in a world of `world`: contiguous, in rank order, covering
    [0, n_batches) exactly once, sizes differing by at most one.  With fewer batches than ranks some shares are empty."""
    if n_batches < 0 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"shard_range: n_batches >= 0 and 0 <= rank < world, got {n_batches}, world {world}, rank {rank}")
    return n_batches * rank // world, n_batches * (rank + 1) // world


def _eval_world(process_group, presharded: bool = False) -> Tuple[int, int]:
    """(world, rank) of a sharded evaluation, (1, 0) without a group."""
    if process_group is None:
        if presharded:
            raise ValueError("presharded: needs a process_group (without one the batches are the whole evaluation)")
        return 1, 0
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        raise ValueError("process_group: torch.distributed is not initialised")
    return dist.get_world_size(process_group), dist.get_rank(process_group)


def model_eval(model, criterion, batches, args, evaluator=None, output_gates: bool = False, process_group=None,
               presharded: bool = False) -> dict:
    """The reference's model_eval (train.py:165-280) over model_forward and metrics.Evaluator: every batch is appended on
    the device (no loss.item(), no .cpu()), the metrics are computed there, and one buffer is read at the end.  Returns
    arrange_metrics' dict.  args: task, task_type, model, n_classes.  evaluator: a metrics.Evaluator to reuse (it is
    reset); without one, a store for exactly these batches is made.  With output_gates the GMU gates are kept in the
    evaluator (Evaluator.predictions()).  cmu-mosi: the logits [B, 1] are squeezed before the criterion, as
    train.py:330 does.

    process_group (data parallelism, one process per GPU): `batches` is the whole list, the same on every rank; this rank
    forwards only batches[shard_range(len(batches), world, rank)], the evaluator holds the global row count, and
    Evaluator.all_gather merges the shards in batch order with counts taken from the batch shapes (no further host
    read while every rank has a batch and output_gates is off; with it the gates' shape is exchanged, one small read).  Every rank returns the same dict, bit for bit that of the evaluation without
    a group.  presharded: `batches` is already this rank's share (a sharding loader); the merged order is then rank-major
    and the counts are exchanged (one small host read; two when the evaluator has to be sized here)."""
    from .metrics import Evaluator
    kind = eval_kind(args)
    crit = criterion if kind != "regression" else (lambda out, tgt: criterion(out.squeeze(1) if out.dim() == 2 else out, tgt))
    world, rank = _eval_world(process_group, presharded)
    counts = None
    if world > 1 or evaluator is None:
        batches = list(batches)
    if world > 1 and not presharded:
        sizes = [int(b[0].shape[0]) for b in batches]
        spans = [shard_range(len(batches), world, r) for r in range(world)]
        counts = [(sum(sizes[lo:hi]), hi - lo) for lo, hi in spans]
        rows, nb = sum(sizes), len(batches)
        batches = batches[spans[rank][0]:spans[rank][1]]
    elif evaluator is None:
        rows, nb = sum(int(b[0].shape[0]) for b in batches), len(batches)
        if world > 1:                           # presharded: the global size is the sum over the ranks
            import torch.distributed as dist
            t = torch.tensor([rows, nb], dtype=torch.int64).to(next(model.parameters()).device)
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=process_group)
            rows, nb = (int(v) for v in t.cpu())
    if evaluator is None:
        dev = next(model.parameters()).device
        evaluator = Evaluator(kind, 1 if kind == "regression" else int(args.n_classes), max(rows, 1), max(nb, 1), device=dev)
    else:
        evaluator.reset()
    with torch.no_grad():
        for batch in batches:
            r = model_forward(model, crit, batch, args.model, gmu_gate=output_gates)
            loss, out, tgt = r[0], r[1], r[2]
            evaluator.update(out, tgt, loss, r[3] if output_gates else None)
    if world > 1:
        evaluator.all_gather(process_group, counts, gates=output_gates)
    return arrange_metrics(args, evaluator.compute())


def make_evaluate(criterion, batches_fn: Callable[[], Iterable], args, key: str, process_group=None) -> Callable:
    """The `evaluate` callable of fit(): evaluate(model) runs model_eval over batches_fn() and returns metrics[key]
    (the reference tunes on "auc_pr_micro" for multilabel tasks and "weight_f1" otherwise, train.py:405-407).  One
    Evaluator is made at the first call, sized by that epoch's batches, and reused; `evaluate.metrics` keeps the last
    dict.  process_group: batches_fn() yields the whole validation split on every rank and model_eval shards it; the
    metric is then the same on every rank."""
    state = {"evaluator": None}
    _eval_world(process_group)

    def evaluate(model):
        from .metrics import Evaluator
        batches = batches_fn()
        if state["evaluator"] is None:
            batches = list(batches)
            kind = eval_kind(args)
            rows = sum(int(b[0].shape[0]) for b in batches)
            state["evaluator"] = Evaluator(kind, 1 if kind == "regression" else int(args.n_classes), max(rows, 1),
                                           max(len(batches), 1), device=next(model.parameters()).device)
        evaluate.metrics = model_eval(model, criterion, batches, args, evaluator=state["evaluator"], process_group=process_group)
        return evaluate.metrics[key]

    evaluate.metrics = None
    return evaluate
