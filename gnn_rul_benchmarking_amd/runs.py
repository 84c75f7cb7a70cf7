"""Several independent training runs of one method stepped together on one device.

The reference protocol trains every (dataset, method) for five seeds, one after the other (``main.py --num_runs 5``).  For HAGCN that
is five times a step whose time is the Bi-LSTM recurrence: 3 584 dependent steps on 2 * num_patch of the 256 CUs (DESIGN.md section
3f).  ``HAGCN_runs`` holds one ordinary ``algorithms.HAGCN`` per run id and advances them through the same step side by side: the
three LSTM layers of all runs are three grouped calls (``hagcn.bilstm_sum_group``: the runs' recurrences share one launch), everything
else -- dropout, the graph stack, ``fc``, the loss, Adam -- runs per run as in ``HAGCN.update``.

A run computes what it would have computed alone: it is built under ``fix_randomness(run_id)`` and owns its generator states
(``RunGenerators``); whatever draws for run r -- its dropouts, its loader's sampler -- runs inside ``runs.active(r)``.

This is not a registry entry: ``--GNN_method`` names stay the reference's, the trainer asks ``get_runs_class(method)`` when
``--concurrent_runs`` is above 1.  Grouping the graph stack or ``fc``, LOGO and the one-direction LSTM users, data parallelism and hipGraph
capture are out of scope."""
from __future__ import annotations

import contextlib
import random

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .algorithms import HAGCN
from .hagcn import bilstm_sum_group, deferred_weight_gradients
from .utils import fix_randomness


def _capture(device):
    cuda = torch.cuda.get_rng_state(device) if device.type == "cuda" else None
    return random.getstate(), np.random.get_state(), torch.get_rng_state(), cuda


def _restore(state, device):
    py, npy, cpu, cuda = state
    random.setstate(py)
    np.random.set_state(npy)
    torch.set_rng_state(cpu)
    if cuda is not None:
        torch.cuda.set_rng_state(cuda, device)


class RunGenerators:
    """The generator states of one run (python, numpy, torch CPU and -- on a CUDA device -- that device's), as ``fix_randomness(run_id)``
    leaves them and as the run's own draws advance them.  ``with gen.active():`` installs them in the global generators and, on
    leaving, saves them and puts back what was there: code inside draws what the run would draw alone, code outside is not disturbed."""

    def __init__(self, run_id, device):
        self.run_id, self.device = int(run_id), torch.device(device)
        outer = _capture(self.device)
        fix_randomness(self.run_id)
        self.state = _capture(self.device)
        _restore(outer, self.device)

    @contextlib.contextmanager
    def active(self):
        outer = _capture(self.device)
        _restore(self.state, self.device)
        try:
            yield self
        finally:
            self.state = _capture(self.device)
            _restore(outer, self.device)


class HAGCN_runs:
    """``HAGCN_runs(configs, hparams, device, run_ids)``: ``.runs[r]`` is a plain ``algorithms.HAGCN`` with the initial weights the
    sequential protocol gives run ``run_ids[r]`` (``state_dict``, ``eval()``, ``model(x)`` per run work as always);
    ``update(Xs, ys, epoch)`` steps all of them once, run r on ``(Xs[r], ys[r])``, and returns their ``{'loss': ...}`` in order."""

    def __init__(self, configs, hparams, device, run_ids):
        self.run_ids = [int(r) for r in run_ids]
        if not self.run_ids:
            raise ValueError("HAGCN_runs needs at least one run id")
        limit = int(_lib.load().rulgnn_bilstm_max_groups())
        if len(self.run_ids) > limit:
            raise ValueError(f"HAGCN_runs steps at most {limit} runs together (rulgnn_bilstm_max_groups), got {len(self.run_ids)}")
        self.device = torch.device(device)
        self.generators = [RunGenerators(r, self.device) for r in self.run_ids]
        self.runs = []
        for gen in self.generators:
            with gen.active():                          # the trainer's order: fix_randomness(run_id), construct, move
                algo = HAGCN(configs, hparams, self.device)
                algo.to(self.device)
            self.runs.append(algo)

    def __len__(self):
        return len(self.runs)

    def active(self, r):
        """The context in which everything that draws random numbers for run ``r`` has to run."""
        return self.generators[r].active()

    def train(self, mode=True):
        for algo in self.runs:
            algo.train(mode)
        return self

    def eval(self):
        return self.train(False)

    def attach_data_parallel(self, dp):
        raise RuntimeError("HAGCN is not sample-shardable (its LSTM recurs along batch*nodes): run independent replicas")

    def update(self, Xs, ys, epoch=None):
        R = len(self.runs)
        if len(Xs) != R or len(ys) != R:
            raise ValueError(f"update() takes one batch per run: {R} runs, {len(Xs)} inputs, {len(ys)} labels")
        models = [algo.model for algo in self.runs]
        seqs, dims = [], []
        for m, X in zip(models, Xs):                    # HAGCN_model.forward: LSTM "batch" = patches, "sequence" = batch * nodes
            if not X.is_cuda:
                raise RuntimeError("HAGCN_model's graph stack runs on the HIP kernels only: input must be a CUDA (ROCm) tensor; "
                                   "there is no CPU fallback")
            bs, num_node, _ = X.size()
            v = torch.reshape(X.float(), [bs, num_node, m.num_patch, m.patch_size])
            seqs.append(torch.transpose(torch.reshape(v, [bs * num_node, m.num_patch, m.patch_size]), 1, 0))
            dims.append((bs, num_node, m.num_patch))
        # Bi_LSTM_Standard.forward, layer by layer over all runs; each run's dropouts draw from its own generators
        h = bilstm_sum_group([m.TD.bi_lstm1 for m in models], seqs)
        h = bilstm_sum_group([m.TD.bi_lstm2 for m in models], h)
        h = [self._drawn(r, lambda r=r: models[r].TD.drop2(h[r])) for r in range(R)]
        h = bilstm_sum_group([m.TD.bi_lstm3 for m in models], h)
        h = [self._drawn(r, lambda r=r: F.leaky_relu(models[r].TD.drop3(h[r]))) for r in range(R)]
        losses = []
        for algo, m, td, y, (bs, num_node, tlen) in zip(self.runs, models, h, ys, dims):
            v = torch.reshape(torch.transpose(td, 1, 0), [bs, num_node, tlen, -1])
            nodes = torch.reshape(torch.transpose(v, 1, 2), [bs * tlen, num_node, -1])
            feats, kl = m.graph_stack(nodes)
            pred = m.fc(torch.reshape(feats, [bs, -1]))
            losses.append(algo.mse(pred, y) + algo.alpha * kl)
        for algo in self.runs:
            algo.optimizer.zero_grad()
        # one backward over the sum: d sum / d loss_r is exactly 1, and each layer's BPTT of all runs is one grouped call
        with deferred_weight_gradients(self.device):
            sum(losses).backward()
        for algo in self.runs:
            algo.optimizer.step()
        return [algo._finish(loss.detach()) for algo, loss in zip(self.runs, losses)]

    def _drawn(self, r, fn):
        with self.generators[r].active():
            return fn()


_RUNS_CLASSES = {"HAGCN": HAGCN_runs}


def get_runs_class(method):
    """The class that steps several runs of ``--GNN_method method`` together; only HAGCN offers one."""
    if method not in _RUNS_CLASSES:
        raise NotImplementedError(f"--concurrent_runs: {method} has no runs class (only {', '.join(_RUNS_CLASSES)} steps several runs together)")
    return _RUNS_CLASSES[method]
