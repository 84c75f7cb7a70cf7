"""Several independent training runs of one method stepped together on one device.

The reference protocol trains every (dataset, method) for five seeds, one after the other (``main.py --num_runs 5``).  A runs class
holds one ordinary algorithm per run id and advances them through the same step side by side:

  * ``HAGCN_runs``: HAGCN's step is its Bi-LSTM recurrence, 3 584 dependent steps on 2 * num_patch of the 256 CUs (DESIGN.md section
    3f).  The three LSTM layers of all runs are three grouped calls (``hagcn.bilstm_sum_group``: the runs' recurrences share one
    launch), everything else -- dropout, the graph stack, ``fc``, the loss, Adam -- runs per run as in ``HAGCN.update``.
  * ``DVGTformer_runs`` and ``LOGO_runs`` (``_FusedRuns``): the whole step of every run is ONE C call,
    ``rulgnn_<family>_fwdbwd_group_f32`` on a host array of the runs' ordinary argument structs.  The kernels that dominate the step
    -- DVGTformer's fold, encoder forward, encoder backward and unfold, LOGO's two graph kernels and its six recurrences -- are
    launched once for all runs with the run index in ``blockIdx.y``; the heads, the sums and Adam follow per run (DESIGN.md
    sections 3p and 3q).  Each run's model and optimizer advance exactly as in the run's own ``update``.

A run computes what it would have computed alone, bit for bit: it is built under ``fix_randomness(run_id)`` and owns its generator
states (``RunGenerators``); whatever draws for run r -- its dropouts, its loader's sampler -- runs inside ``runs.active(r)``.

These are not registry entries: ``--GNN_method`` names stay the reference's, the trainer asks ``get_runs_class(method)`` when
``--concurrent_runs`` is above 1.  Grouping HAGCN's graph stack or the heads' GEMMs, LOGO_bearing and the one-direction LSTM users, data
parallelism and hipGraph capture are out of scope."""
from __future__ import annotations

import contextlib
import ctypes as C
import random

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .algorithms import DVGTformer, HAGCN, LOGO
from .flat import current_stream
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


class _Runs:
    """What the runs classes share: ``(configs, hparams, device, run_ids)`` builds ``.runs[r]``, a plain ``algorithm`` with the initial
    weights the sequential protocol gives run ``run_ids[r]`` (``state_dict``, ``eval()``, ``model(x)`` per run work as always), each
    under its own ``RunGenerators``; a subclass adds ``update(Xs, ys, epoch)``, which steps all of them once, run r on
    ``(Xs[r], ys[r])``, and returns their ``{'loss': ...}`` in order."""
    algorithm = None            # the plain algorithm class
    limit_entry = None          # the C entry that says how many runs one call takes
    not_shardable = None        # why attach_data_parallel is refused

    def __init__(self, configs, hparams, device, run_ids):
        name = type(self).__name__
        self.run_ids = [int(r) for r in run_ids]
        if not self.run_ids:
            raise ValueError(f"{name} needs at least one run id")
        limit = int(getattr(_lib.load(), self.limit_entry)())
        if len(self.run_ids) > limit:
            raise ValueError(f"{name} steps at most {limit} runs together ({self.limit_entry}), got {len(self.run_ids)}")
        self.device = torch.device(device)
        self.generators = [RunGenerators(r, self.device) for r in self.run_ids]
        self.runs = []
        for gen in self.generators:
            with gen.active():                          # the trainer's order: fix_randomness(run_id), construct, move
                algo = self.algorithm(configs, hparams, self.device)
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
        raise RuntimeError(self.not_shardable)

    def _one_batch_per_run(self, Xs, ys):
        R = len(self.runs)
        if len(Xs) != R or len(ys) != R:
            raise ValueError(f"update() takes one batch per run: {R} runs, {len(Xs)} inputs, {len(ys)} labels")
        return R


class HAGCN_runs(_Runs):
    """The three Bi-LSTM layers of all runs as grouped calls, the rest of ``HAGCN.update`` per run."""
    algorithm, limit_entry = HAGCN, "rulgnn_bilstm_max_groups"
    not_shardable = "HAGCN is not sample-shardable (its LSTM recurs along batch*nodes): run independent replicas"

    def update(self, Xs, ys, epoch=None):
        R = self._one_batch_per_run(Xs, ys)
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


class _FusedRuns(_Runs):
    """Runs of a fused-step family (``algorithms._FusedAlgorithm``) behind ``rulgnn_<c_family>_fwdbwd_group_f32``: ``update`` prepares
    every run's step as the run's own ``update`` would -- the model's dropout step, the optimizer's step count, the tape mark, the
    batch's workspace entry (``model.fused_mse_step_args``) -- and makes ONE C call for all of them.  All runs take the same batch size
    (one shape struct serves the call).  A subclass names the algorithm; ``step_fields(algo)`` are what its ``_eager_update`` passes to
    ``fused_mse_step`` on top of the batch."""
    limit_entry = "rulgnn_step_max_groups"

    def step_fields(self, algo):
        return {}

    def update(self, Xs, ys, epoch=None):
        R = self._one_batch_per_run(Xs, ys)
        for algo, X in zip(self.runs, Xs):              # every refusal of the python side before any run's counters move
            if algo.needs_train_mode and not algo.model.training:
                raise RuntimeError(f"update() needs algorithm.train() ({algo.needs_train_mode})")
            algo.model._require_device(X)
        fused_group_step([algo.model for algo in self.runs], [algo.optimizer for algo in self.runs], Xs, ys,
                         [self.step_fields(algo) for algo in self.runs])
        return [algo._finish(algo.model.bucket[algo.model.num_live]) for algo in self.runs]


def fused_group_step(models, optimizers, Xs, ys, fields=None):
    """One fused step of several models of one family and shape as ONE ``rulgnn_<c_family>_fwdbwd_group_f32`` call: model r on
    ``(Xs[r], ys[r])`` with ``optimizers[r]`` (all FusedAdam, or all None: gradients only) and ``fields[r]`` on top, each prepared by its
    own ``fused_mse_step_args``.  Fills every model's ``bucket`` = [grad | loss]; returns their ``(pred [B], loss 0-d)`` views."""
    R = len(models)
    if len({int(X.size(0)) for X in Xs}) != 1:          # one shape struct serves the call
        raise ValueError(f"a grouped step takes runs of one batch size, got {[int(X.size(0)) for X in Xs]}")
    fields = fields if fields is not None else [{}] * R
    steps = [m.fused_mse_step_args(X, y, opt, **kw) for m, opt, X, y, kw in zip(models, optimizers, Xs, ys, fields)]
    args = (models[0].Args * R)(*[step[1] for step in steps])
    blocks = [step[2] for step in steps]
    if any(b is None for b in blocks) and not all(b is None for b in blocks):
        raise ValueError("a grouped step takes an optimizer for every run or for none")
    opts = (_lib.AdamArgs * R)(*blocks) if blocks[0] is not None else None
    name = f"rulgnn_{models[0].c_family}_fwdbwd_group_f32"
    _lib.check(getattr(_lib.load(), name)(C.byref(steps[0][0]), args, opts, R, current_stream()), name)
    del steps                                           # (held the checked inputs the structs point to until the call was enqueued)
    return [(m._pred_buf, m.bucket[m.num_live]) for m in models]


class DVGTformer_runs(_FusedRuns):
    algorithm = DVGTformer
    not_shardable = "DVGTformer_runs steps independent runs on one device; data parallelism with concurrent runs is not built: run independent replicas"


class LOGO_runs(_FusedRuns):
    algorithm = LOGO
    not_shardable = "LOGO is not sample-shardable (its LSTMs recur along the batch): run independent replicas"

    def step_fields(self, algo):
        return {"theta": algo.theta}


_RUNS_CLASSES = {"HAGCN": HAGCN_runs, "DVGTformer": DVGTformer_runs, "LOGO": LOGO_runs}


def get_runs_class(method):
    """The class that steps several runs of ``--GNN_method method`` together; HAGCN, DVGTformer and LOGO offer one."""
    if method not in _RUNS_CLASSES:
        raise NotImplementedError(f"--concurrent_runs: {method} has no runs class (only {', '.join(_RUNS_CLASSES)} step several runs together)")
    return _RUNS_CLASSES[method]
