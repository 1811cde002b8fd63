"""Captured launch sequences (hipGraph) of the model step: the cache half of a `_Trunk` (models/bpmult.py: its base class)."""
# The ~420 launches of a step are the same every step for a given (mode, input lengths): captured once per key and
# replayed.  What changes per step travels through device memory: the inputs (copied into static staging tensors),
# the dropout seed (BPM_SEED_INDIRECT: the kernels read it when they run) and the incoming logit gradients.  Host-side
# decisions stay outside the graph: the weight-shadow refresh, whether the gradients start from zero (part of the key),
# attaching .grad views.  Used when nothing needs the eager launch order: no gradient-exchange hook (GradSync runs
# eagerly: its all-reduces interleave with backward), launch profiler off.  The trunk (the subclass) composes the keys, names the inputs
# and keeps the host-side state of a forward; GraphCache counts, captures, bounds and replays.
from __future__ import annotations

import os
import warnings
from collections import OrderedDict
from typing import Callable, Optional

import torch

from . import engine, ops

_RETIRED_GRAPHS: list = []       # captured graphs of dropped trunks: kept alive, never replayed (see GraphCache.MAX_GRAPHS)


class GraphCache:
    GRAPH_WARMUP = 2            # eager runs of a forward key before it is captured (lazy allocations, stream creation)
    # Bounded caches.  The reference collate pads text to the batch's longest sentence and trims audio to its shortest
    # clip (data/helpers.py:83-102), so real training sees hundreds of (L, V, A) keys, and every captured graph pins its
    # static inputs / outputs and every allocation made during its capture.  At most MAX_GRAPHS keys are ever captured
    # (forward graph + its backward graphs): the first ones to recur GRAPH_WARMUP times; every other key runs as eager
    # launches (the step time is the same: DESIGN.md section 4).  Call counters are kept for MAX_TRACKED keys.
    # Captured graphs are NEVER DESTROYED while the process lives: on this stack (torch 2.10 + ROCm 7.0/7.2) destroying a
    # captured graph and then capturing / launching others ends in a host segfault inside hipGraphLaunch
    # (tools/graph_cache_probe.py, profiles/r04_graph_probe.json: 5 of 5 evicting variants crash -- shared or per-key pool,
    # with or without a device synchronise, either capture mode -- 0 of 2 non-evicting ones; round 3's capture_end crash
    # had the same ingredients).  So there is no LRU eviction, and a trunk that is dropped (another batch size, .to())
    # parks its graph objects in _RETIRED_GRAPHS after releasing their static tensors.
    MAX_GRAPHS = 4
    MAX_TRACKED = 64

    def __init__(self, device):
        self._fg, self._bg = OrderedDict(), OrderedDict()         # key -> {"calls", then "graph", "out" + staging | "failed"}
        self._gpool = None                                        # pool handle shared by this cache's graphs (first capture)
        self.graph_stats = {"captured": 0, "failed": 0}           # forward keys captured; captures (either kind) that failed
        self.MAX_GRAPHS = int(os.environ.get("BPMULT_MAX_GRAPHS", self.MAX_GRAPHS))
        self._seed_dev = torch.zeros(1, device=device, dtype=torch.int64)
        self.capturing = False

    def _seed_handle(self, seed: int) -> int:
        self._seed_dev.fill_(seed)
        return ops.DeviceSeed(self._seed_dev)

    def _forget_idle_counters(self) -> None:
        """Forget the oldest call counters of keys that hold no graph (see MAX_TRACKED); captured graphs stay."""
        idle = [k for k, e in self._fg.items() if "graph" not in e]
        for k in idle[:max(0, len(idle) - self.MAX_TRACKED)]:
            del self._fg[k]
            for bk in [bk for bk in self._bg if bk[0] == k]:
                del self._bg[bk]

    def retire_graphs(self) -> None:
        """The trunk is being dropped: park its captured graphs (never destroyed while the process lives, see above) and
        release everything else they pinned."""
        park = os.environ.get("BPMULT_GRAPH_DESTROY", "0") != "1"      # (=1: tools/graph_cache_probe.py reproduces the crash)
        for table in (self._fg, self._bg):
            for e in table.values():
                if "graph" in e and park:
                    _RETIRED_GRAPHS.append(e["graph"])
                e.clear()
            table.clear()

    def _capture(self, fn):
        """Capture fn() into a new graph.  thread_local error mode: the backward capture runs on the autograd thread while
        other threads (a DataLoader's pin_memory thread, an asynchronous checkpoint copy) may call into HIP.  Every side
        stream forked inside the capture must have been joined back when fn returns: an unjoined fork is joined here and
        reported as a Python error after the capture has ended -- not left for hipStreamEndCapture to trip over.
        Returns (graph, result) or raises; the caller marks the key non-capturable and goes on eagerly."""
        if self._gpool is None:
            self._gpool = torch.cuda.graph_pool_handle()
        g = torch.cuda.CUDAGraph()
        left = []
        engine._OPEN_FORKS.clear()                                # (forks of earlier eager runs are not this capture's)
        self.capturing = True
        try:
            with torch.cuda.graph(g, pool=self._gpool, capture_error_mode="thread_local"):
                try:
                    res = fn()
                finally:
                    left = engine.open_forks()
                    for st_ in left:                              # join, so that the capture can end cleanly
                        torch.cuda.current_stream().wait_stream(st_)
        finally:
            self.capturing = False
            engine._OPEN_FORKS.clear()
        if left:
            raise RuntimeError(f"graph capture: {len(left)} side stream(s) were still forked when the launch sequence ended "
                               "(a step table without its JOIN)")
        return g, res

    def replay(self, forward: bool, key, seed: int, inputs: dict, fn: Callable, warning: str,
            on_fail: Callable[[], None] = lambda: None) -> Optional[dict]:
        """One call of `key`.  None (the caller runs eagerly): while it warms up (a forward key GRAPH_WARMUP calls, a backward
        key one), when MAX_GRAPHS forward keys hold graphs already, after its capture failed (that marks the key, calls
        on_fail, warns once with `warning` % the reason and synchronises).  Otherwise: capture fn(static copies of
        `inputs`, seed handle) if that has not happened, copy the inputs (tensors or None) in, set the seed, replay;
        returns the key's entry, whose "out" is what fn returned inside the capture."""
        table, warmup = (self._fg, self.GRAPH_WARMUP) if forward else (self._bg, 1)
        ent = table.setdefault(key, {"calls": 0})
        table.move_to_end(key)
        ent["calls"] += 1
        if ent.get("failed"):
            return None
        if "graph" not in ent:
            full = forward and sum("graph" in e for e in self._fg.values()) >= self.MAX_GRAPHS
            if ent["calls"] <= warmup or full:
                self._forget_idle_counters()
                return None
            ent["in"] = {k: None if t is None else torch.empty_like(t) for k, t in inputs.items()}
            handle = self._seed_handle(seed)
            try:
                ent["graph"], ent["out"] = self._capture(lambda: fn(ent["in"], handle))
            except Exception as exc:                      # noqa: BLE001 -- any capture failure: this key runs eagerly from now on
                ent.clear()
                ent.update(calls=warmup + 1, failed=True)
                on_fail()
                self.graph_stats["failed"] += 1
                warnings.warn(warning % exc)
                torch.cuda.synchronize()
                return None
            if forward:
                self.graph_stats["captured"] += 1
            self._forget_idle_counters()
        for k, t in inputs.items():
            if t is not None:
                ent["in"][k].copy_(t)
        self._seed_handle(seed)
        ent["graph"].replay()
        return ent
