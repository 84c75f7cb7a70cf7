"""Base class of the model modules: flat fp32 parameter storage, the data-parallel bucket, workspace caches and the C-ABI call path
every flat-parameter family shares (argument struct, ``forward`` / ``backward`` / ``fwdbwd`` calls, Adam argument block, autograd).

A model module keeps the reference's ``nn.Module`` tree (same construction order => same RNG consumption => same initial
weights, same ``state_dict`` keys; the sub-modules only hold parameters) and runs on ONE flat device buffer:

  * ``_flat``       every parameter, in the order of the family's flat layout (include/rulgnn.h); the ``nn.Parameter``s are views
  * ``_grad_flat``  ``[gradient | loss | family extras]`` -- what the kernels write and one all-reduce carries (``bucket``)
  * ``_bufs``       per-batch-size workspaces (activations kept from forward to backward), a small LRU
  * ``_bn`` / ``_nbt``  the BatchNorm statistics / counters of the families that have them (``bn_modules``), the modules' buffers are views

``nn.Module._apply`` (``.to()``, ``.float()``...) converts tensors one by one: ``_apply`` below rebuilds the views when that
happened and leaves everything in place when it was a no-op (the per-epoch ``model.to(device)`` of the trainers; captured
hipGraphs and the optimizer state point into the buffers).

A family describes its C entries as data (``c_family``, ``Args``, ``not_covered``...) and keeps what is its own: ``_shape``, the shape
check of ``_check_input``, the family fields of ``_args``, its BatchNorm running-statistics entry and the ``forward`` the reference
pins.  ``DropoutStepModule`` (at the end) is the base of the families that draw dropout by sample index in the global batch: it holds
their step counter, the dropout fields of ``_args``, ``fused_mse_step`` and the train / eval ``forward``."""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _lib, params as PL


def current_stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _FlatFunction(torch.autograd.Function):
    """``model(x)`` with autograd through the family's ``forward`` / ``backward`` C entries.  ``state`` (training flag, dropout step)
    goes to both calls; the outputs are ``_run_forward``'s, the prediction first.  The backward reads the activations the forward left
    in the workspace of its batch size, which every later forward of that size overwrites: ``model._tape`` makes that an error."""

    @staticmethod
    def forward(ctx, model, x, state, *params):
        outs = model._run_forward(x, *state)
        ctx.model, ctx.x, ctx.state, ctx.token = model, x, state, model._tape.tokens[x.size(0)]
        return tuple(o.clone() for o in outs)

    @staticmethod
    def backward(ctx, *douts):
        model, B = ctx.model, ctx.x.size(0)
        model._tape.check(B, ctx.token, model._bufs, type(model).__name__)
        grads = model._run_backward(ctx.x, douts, *ctx.state)
        if model.consumes_tape:
            model._tape.consume(B, ctx.token)
        k = model.gradless_params
        return (None,) * (3 + k) + tuple(grads[off:off + n].view(shape).clone() for off, n, shape in model._slices[k:])


class FlatModule(nn.Module):
    bucket_tail = 1            # floats behind the gradient in ``_grad_flat``: the loss (+ what a family appends)
    flat_order = None          # parameter names in flat-layout order; None = ``named_parameters()`` order
    workspace_slots = 2        # batch sizes whose workspaces are kept (training batch + evaluation batch)
    output_buffers = 1         # [B] fp32 outputs cached with each workspace: the prediction (+ RGCNU's std head)

    # ---- the family's C entries: rulgnn_<c_family>_{<workspace_query>, forward_f32, backward_f32, fwdbwd_f32} ---------------
    c_family = None            # entry prefix ("sagcn", ...)
    Args = None                # their argument struct (_lib.SagcnArgs, ...)
    workspace_query = "workspace_bytes"
    not_covered = None         # RuntimeError text when the workspace query returns 0
    consumes_tape = False      # the backward reworks the forward's activations in place: one backward per forward
    gradless_params = 0        # leading parameters of the layout that never receive a gradient (autograd returns None)

    # ---- construction ----------------------------------------------------------------------------------
    def _init_flat(self, layout=None, count=None):
        """Call at the end of ``__init__``, once the parameter-holding sub-modules exist.  ``layout`` (name -> (offset, shape), with
        ``count`` floats in all) is the family's own table where the flat order is not the ``named_parameters()`` order."""
        table = dict(self.named_parameters())
        if layout is not None:
            self._layout, self._slices = OrderedDict(layout), []
            for name, (off, shape) in self._layout.items():
                if tuple(table[name].shape) != tuple(shape):
                    raise RuntimeError(f"flat layout of '{name}' is {tuple(shape)}, the parameter is {tuple(table[name].shape)}")
                self._slices.append((off, table[name].numel(), tuple(shape)))
            self._count = int(count)
        else:
            names = list(self.flat_order) if self.flat_order is not None else list(table)
            self._layout, self._slices, off = OrderedDict(), [], 0
            for name in names:
                p = table[name]
                self._layout[name] = (off, tuple(p.shape))
                self._slices.append((off, p.numel(), tuple(p.shape)))
                off += p.numel()
            self._count = off
        self._flat = self._grad_flat = None
        self._bufs, self._pin_bufs, self._step_state = {}, False, None
        self._tape = PL.ForwardTape()
        self._reflatten()

    def _named(self):
        table = dict(self.named_parameters())
        return [table[name] for name in self._layout]

    def _named_live(self):
        return list(zip(self._layout, self._named()))

    # ---- BatchNorm state --------------------------------------------------------------------------------
    # A family with BatchNorm names its modules in ``bn_modules``.  ``_bn`` holds every module's running_mean then running_var, module
    # after module: the fp32 buffer the kernels read.  ``_bn_batch`` has the same layout for the batch statistics of the latest training
    # forward, and the bucket carries one more such block behind the loss (data parallel: the batch moments, all-reduced with the
    # gradient).  num_batches_tracked: a fused step only counts (``_nbt_pending``); the int64 device tensor ``_nbt`` (one per module) is
    # brought up to date when somebody looks (state_dict, a move).  The modules' buffers are views of ``_bn`` / ``_nbt``.
    bn_modules = ()
    _bn = _bn_batch = _nbt = None
    _nbt_pending = 0

    def _track_batchnorm_counters(self):
        """Call in ``__init__`` before ``_init_flat``."""
        self._nbt_pending = 0
        self.register_state_dict_pre_hook(lambda module, prefix, keep_vars: module._flush_nbt())

    def _flush_nbt(self):
        if self._nbt_pending and self._nbt is not None:
            self._nbt += self._nbt_pending
            self._nbt_pending = 0

    def _reflatten_buffers(self, dev):
        """Move the statistics / counters of ``bn_modules`` into ``_bn`` / ``_nbt`` and allocate a zeroed ``_bn_batch``.  A family with
        another layout overrides this."""
        if not self.bn_modules:
            return
        bufs = dict(self.named_buffers())
        stats = [f"{m}.{leaf}" for m in self.bn_modules for leaf in ("running_mean", "running_var")]
        bn = torch.empty(sum(bufs[name].numel() for name in stats), dtype=torch.float32, device=dev)
        off = 0
        for name in stats:
            n = bufs[name].numel()
            bn[off:off + n].copy_(bufs[name].detach().float())
            self._set_buffer(name, bn[off:off + n])
            off += n
        nbt = torch.zeros(len(self.bn_modules), dtype=torch.int64, device=dev)
        for i, m in enumerate(self.bn_modules):
            nbt[i].copy_(bufs[m + ".num_batches_tracked"])
            self._set_buffer(m + ".num_batches_tracked", nbt[i])
        self._bn, self._nbt = bn, nbt
        self._bn_batch = torch.zeros_like(bn)

    def _bn_args(self, a, batch, moments_to_bucket=False):
        """The BatchNorm fields of ``a`` for a call at ``batch``: the running statistics (where the struct has them) and where a training
        forward leaves its batch statistics -- ``_bn_batch``, or with ``moments_to_bucket`` (data parallel) the bucket's block, as the
        moments (E[z], E[z^2]) weighted batch / global_batch, which the all-reduce sums to the global batch's."""
        if hasattr(self.Args, "bn_stats"):
            a.bn_stats = self._bn.data_ptr()
        if moments_to_bucket:
            a.bn_batch = self._bn_source(True)
            a.bn_moment_weight = batch / float(a.global_batch)
        else:
            a.bn_batch = self._bn_batch.data_ptr()
            a.bn_moment_weight = 0.0

    def _bn_source(self, in_bucket):
        """The batch statistics a running-statistics update reads: the bucket's block behind the loss, or ``_bn_batch``."""
        return self._grad_flat.data_ptr() + 4 * (self._count + self.bucket_tail) if in_bucket else self._bn_batch.data_ptr()

    # ---- flat storage ----------------------------------------------------------------------------------
    def _bucket_floats(self) -> int:
        return self._count + self.bucket_tail + (self._bn.numel() if self.bn_modules else 0)

    def _reset_caches(self):
        self._bufs, self._step_state = {}, None
        self._ws = self._pred_buf = None
        self._out_bufs = ()

    def _reflatten(self):
        self._flush_nbt()
        ps = self._named()
        dev = ps[0].device
        flat = torch.empty(self._count, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, (off, n, shape) in zip(ps, self._slices):
                flat[off:off + n].copy_(p.detach().reshape(-1).float())
                p.data = flat[off:off + n].view(shape)
        self._flat = flat
        self._reflatten_buffers(dev)
        self._grad_flat = torch.zeros(self._bucket_floats(), dtype=torch.float32, device=dev)
        self._reset_caches()
        PL.mark_flat_views(self)

    def _apply(self, fn, recurse=True):
        super()._apply(fn)
        if not PL.flat_views_intact(self):      # a no-op .to(device) (every epoch in the trainers) keeps the buffers
            self._reflatten()                   # a real move converts tensors one by one: rebuild the flat views
        return self

    def _set_buffer(self, dotted, tensor):
        mod = self
        parts = dotted.split(".")
        for a in parts[:-1]:
            mod = getattr(mod, a)
        mod._buffers[parts[-1]] = tensor

    @property
    def flat_params(self):
        return self._flat

    @property
    def bucket(self):
        """[gradient | loss]: what one all-reduce carries in data-parallel training."""
        return self._grad_flat

    @property
    def num_live(self):
        return self._count

    # ---- C-ABI plumbing --------------------------------------------------------------------------------
    def _workspace_entry(self, key, nbytes, unsupported: str, make=None):
        """The cached ``(workspace bytes, output buffers...)`` of batch size ``key``; allocates (and evicts the oldest entry
        beyond ``workspace_slots`` unless ``_pin_bufs``) on a miss.  ``nbytes`` is a callable: the family's
        ``rulgnn_*_workspace_bytes`` (0 = configuration not covered -> RuntimeError(unsupported))."""
        ent = self._bufs.get(key)
        if ent is None:
            n = nbytes()
            if n == 0:
                raise RuntimeError(unsupported)
            if len(self._bufs) >= self.workspace_slots and not self._pin_bufs:
                self._bufs.pop(next(iter(self._bufs)))
            dev = self._flat.device
            ent = (torch.empty(n, dtype=torch.uint8, device=dev),) + (make(dev) if make is not None else tuple(     # [B] views, never null
                torch.empty(max(int(key), 1), dtype=torch.float32, device=dev)[:int(key)] for _ in range(self.output_buffers)))
            self._bufs[key] = ent
        return ent

    def _adam_block(self, optimizer, bn=None):
        """The ``rulgnn_adam_args`` of a fused step with ``optimizer`` (optim.FusedAdam over this model), advancing its step count;
        None when the call should only produce gradients."""
        if optimizer is None:
            return None
        m, v = optimizer._state_buffers()
        optimizer._steps += 1
        g = optimizer.param_groups[0]
        return _lib.AdamArgs(self._flat.data_ptr(), m.data_ptr(), v.data_ptr(), bn.data_ptr() if bn is not None else None,
                             optimizer._steps, float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                             float(g["weight_decay"]), 0.1,
                             self._step_state.data_ptr() if self._step_state is not None else None)

    def _adam_args(self, optimizer, bn=None):
        """``byref`` of ``_adam_block``'s struct, or None."""
        block = self._adam_block(optimizer, bn=bn)
        return None if block is None else C.byref(block)

    def _require_device(self, x):
        """The input guard of every family: the model runs on its HIP kernels, on the device of its parameters."""
        if not x.is_cuda:
            raise RuntimeError(f"{type(self).__name__} runs on the HIP path only: input must be a CUDA (ROCm) tensor; "
                               "there is no CPU fallback")
        if x.device != self._flat.device:
            raise RuntimeError(f"input on {x.device} but model on {self._flat.device}")

    def _step_inputs(self, x, y):
        """``(x, flat fp32 target)`` of a training step: ``_check_input(x)`` and one target per sample."""
        x = self._check_input(x)
        yv = y.reshape(-1).contiguous().float()
        if yv.numel() != x.size(0):
            raise RuntimeError("target size mismatch")
        return x, yv

    def _args(self, shp, x, y=None, dpred=None, global_batch=None):
        """``Args`` of one call at ``x``'s batch size with the fields every family shares; a family's override sets its own on top.  The
        batch's cached workspace and output buffers become ``_ws`` / ``_out_bufs`` (``_pred_buf`` = the prediction's)."""
        B = x.size(0)
        ent = self._workspace_entry(B, lambda: getattr(_lib.load(), f"rulgnn_{self.c_family}_{self.workspace_query}")(C.byref(shp)),
                                    self.not_covered)
        # (plain instance attributes, written past nn.Module.__setattr__: its checks cost a microsecond apiece on every step)
        vars(self).update(_ws=ent[0], _out_bufs=ent[1:], _pred_buf=ent[1])
        a = self.Args()
        a.x = x.data_ptr()
        a.y = y.data_ptr() if y is not None else None
        a.dpred = dpred.data_ptr() if dpred is not None else None
        a.params, a.grads = self._flat.data_ptr(), self._grad_flat.data_ptr()
        a.pred = self._pred_buf.data_ptr()
        a.loss = self._grad_flat.data_ptr() + 4 * self._count
        a.workspace, a.workspace_bytes = self._ws.data_ptr(), self._ws.numel()
        a.global_batch = B if global_batch is None else int(global_batch)
        return a

    def _call(self, kind, shp, a, *more):
        """``rulgnn_<c_family>_<kind>_f32(shape, args, *more, stream)``; a non-zero code raises."""
        name = f"rulgnn_{self.c_family}_{kind}_f32"
        _lib.check(getattr(_lib.load(), name)(C.byref(shp), C.byref(a), *more, current_stream()), name)

    def _run_forward(self, x, *state):
        """One ``forward`` call; returns the output buffers' ``[B, 1]`` views (the prediction first), valid until the next call."""
        B = x.size(0)
        shp = self._shape(B)
        self._tape.mark(B)
        a = self._args(shp, x, *state)
        self._call("forward", shp, a)
        return tuple(t.view(-1, 1) for t in self._out_bufs)

    def _run_backward(self, x, douts, *state, **fields):
        """One ``backward`` call of the last forward at ``x``'s batch size with the outputs' incoming gradients ``douts``; fills
        ``_grad_flat``."""
        shp = self._shape(x.size(0))
        dpred = douts[0].reshape(-1).contiguous().float()
        a = self._args(shp, x, *state, dpred=dpred, **fields)
        self._call("backward", shp, a)
        return self._grad_flat

    def _fused_step(self, x, yv, optimizer, global_batch, *state, bn=None, **fields):
        """One ``fwdbwd`` call (forward + MSE + backward, + Adam with ``optimizer``) on checked inputs (``_step_inputs``)."""
        shp, a, opt = self._fused_step_args(x, yv, optimizer, global_batch, *state, bn=bn, **fields)
        self._call("fwdbwd", shp, a, None if opt is None else C.byref(opt))
        return self._pred_buf, self._grad_flat[self._count]

    def _fused_step_args(self, x, yv, optimizer, global_batch, *state, bn=None, **fields):
        """What one ``fwdbwd`` call takes, everything short of the call itself: ``(shape, args, rulgnn_adam_args or None)``.  The
        tape is marked, the batch's workspace entry becomes current and the optimizer's step count advances, as in ``_fused_step``
        (runs.py hands several models' triples to one grouped call)."""
        shp = self._shape(x.size(0))
        self._tape.mark(x.size(0))
        a = self._args(shp, x, *state, y=yv, global_batch=global_batch, **fields)
        return shp, a, self._adam_block(optimizer, bn=bn)

    def fused_mse_step(self, x, y, optimizer=None, global_batch=None):
        """forward + MSE + backward (+ Adam when ``optimizer`` is a FusedAdam over this model) in one C call; fills ``self.bucket`` =
        [grad | loss]; returns (pred [B], loss 0-d tensor) on the device, no host sync."""
        return self._fused_step(*self._step_inputs(x, y), optimizer, global_batch)

    def _forward_state(self, training):
        """``state`` of one forward of the shared BatchNorm-family paths below (what ``_args`` takes after ``x``): the training flag.  A
        family that draws dropout per step overrides this and advances its step here."""
        return (training,)

    def _bn_fused_mse_step(self, x, y, optimizer, global_batch, update_running_stats, moments_to_bucket, **fields):
        """``fused_mse_step`` of a BatchNorm family.  With ``optimizer`` the C call also updates the running statistics; without, they are
        updated here unless ``update_running_stats`` is False (data parallel: after the all-reduce, from the bucket)."""
        x, yv = self._step_inputs(x, y)
        out = self._fused_step(x, yv, optimizer, global_batch, *self._forward_state(True), bn=self._bn,
                               moments_to_bucket=moments_to_bucket, **fields)
        if optimizer is not None:
            self._nbt_pending += 1
        elif update_running_stats:
            self._after_train_forward(x.size(0))
        return out

    def _syncbn_step(self, entry, x, y, global_batch, bn_param_grad_scale, allreduce, *more, **fields):
        """``fused_mse_step_syncbn`` (dp.py, ``DataParallel(sync_bn=True)``): the step on this rank's shard with every BatchNorm
        normalising by the GLOBAL batch's statistics, one ``entry(shape, args, bn_param_grad_scale, callback, user, *more, stream)`` call.
        It calls ``allreduce(view)`` once per ``sync_bn_schedule()`` count with a float64 view of that many reduction cells inside the
        workspace, which must SUM it over the ranks in place, in stream order.  Fills ``self.bucket`` such that a SUM over the ranks is
        the global-batch gradient / loss (the BatchNorm scale / shift gradients are global sums on every rank and enter multiplied by
        ``bn_param_grad_scale``), and ``self._bn_batch`` with the global (mean, biased variance)."""
        x, yv = self._step_inputs(x, y)
        state = self._forward_state(True)
        shp = self._shape(x.size(0))
        self._tape.mark(x.size(0))
        a = self._args(shp, x, *state, y=yv, global_batch=global_batch, **fields)
        cb, user, failure = _lib.allreduce_callback(allreduce, self._ws)
        rc = getattr(_lib.load(), entry)(C.byref(shp), C.byref(a), float(bn_param_grad_scale), cb, user, *more, current_stream())
        if failure:
            raise failure[0]
        _lib.check(rc, entry)
        return self._pred_buf, self._grad_flat[self._count]

    def _bn_forward(self, x):
        """``forward`` of a BatchNorm family: the prediction [B, 1]; in training through autograd when grad mode is on, and the running
        statistics advance.  An empty batch gives an empty prediction in eval and raises in training, as BatchNorm does."""
        x = self._check_input(x)
        if x.size(0) == 0:
            if self.training:
                raise RuntimeError("training forward needs a non-empty batch")
            return torch.empty(0, 1, dtype=torch.float32, device=x.device)
        if not self.training:
            return self._predict(x, *self._forward_state(False), autograd=False)[0]
        pred = self._predict(x, *self._forward_state(True), autograd=torch.is_grad_enabled())[0]
        self._after_train_forward(x.size(0))
        return pred

    def _tap(self, batch, index, shape):
        """Tap ``index`` of the family's ``rulgnn_<c_family>_tap_offset`` in the workspace of the last forward at this batch size, as a new
        tensor of ``shape`` (the layout the kernels wrote: ``shape`` says where the batch sits)."""
        off = getattr(_lib.load(), f"rulgnn_{self.c_family}_tap_offset")(C.byref(self._shape(batch)), index)
        ws = self._bufs[batch][0].view(torch.float32)
        return ws[off:off + math.prod(shape)].view(shape).clone()

    def _needs_grad(self):
        return torch.is_grad_enabled() and any(p.requires_grad for p in self._named())

    def _predict(self, x, *state, autograd):
        """``_run_forward``'s outputs as new tensors; through the autograd Function (parameter gradients from the backward entry) when
        ``autograd``."""
        if autograd:
            return _FlatFunction.apply(self, x, state, *self._named())
        return tuple(o.clone() for o in self._run_forward(x, *state))


class DropoutStepModule(FlatModule):
    """A family without a BatchNorm path of FlatModule's whose dropout masks come from the package's counter hash, keyed by
    ``(seed, step, sample index in the global batch)``: the step counter, the five dropout fields of ``Args`` (``sample_offset``,
    ``dropout_p``, ``seed``, ``step``, ``training``), the fused step and the train / eval ``forward``.  ``state`` of a call is
    ``(training, step)``.  The family supplies ``dropout_p`` (what the struct's field takes: an attribute, or a property over the
    modules that hold the rates) and ``empty_batch``."""
    dropout_by_sample_offset = True          # dp.py: pass the shard's first global sample index to fused_mse_step
    eval_sample_independent = True           # no BatchNorm, no recurrence along the batch: a test set may be re-batched per shard
    empty_batch = None                       # RuntimeError text of a forward on an empty batch; None: it gives an empty prediction

    def _init_flat(self, layout=None, count=None):
        self._seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        self._step = 0
        super()._init_flat(layout, count)

    def _args(self, shp, x, training, step, y=None, dpred=None, global_batch=None, sample_offset=0):
        """``training`` and ``step`` of a backward must be the forward's: it redraws the forward's dropout masks from them."""
        a = super()._args(shp, x, y, dpred, global_batch)
        a.sample_offset = int(sample_offset)
        a.dropout_p = self.dropout_p
        a.seed, a.step = self._seed, int(step)
        a.training = 1 if training else 0
        return a

    def fused_mse_step(self, x, y, optimizer=None, global_batch=None, sample_offset=0, **fields):
        """forward (train mode) + MSE + backward (+ Adam when ``optimizer`` is a FusedAdam over this model) in one C call; fills
        ``self.bucket`` = [grad | loss]; returns (pred [B], loss 0-d tensor) on the device, no host sync.  ``fields`` go to the family's
        ``_args``."""
        x, yv = self._step_inputs(x, y)
        vars(self)["_step"] = step = self._step + 1          # (past nn.Module.__setattr__, as in FlatModule._args)
        return self._fused_step(x, yv, optimizer, global_batch, True, step, sample_offset=sample_offset, **fields)

    def fused_mse_step_args(self, x, y, optimizer=None, **fields):
        """What ``fused_mse_step(x, y, optimizer, **fields)`` would hand to its C call, short of calling: ``(shape, args,
        rulgnn_adam_args or None, the checked tensors the structs point to)``; the step counters advance as there."""
        x, yv = self._step_inputs(x, y)
        vars(self)["_step"] = step = self._step + 1
        return self._fused_step_args(x, yv, optimizer, None, True, step, **fields) + ((x, yv),)

    def _forward_outputs(self, x):
        """Every output of one forward; dropout follows ``self.training`` (a training forward advances the step), through autograd when
        grad mode is on."""
        x = self._check_input(x)
        if x.size(0) == 0:
            if self.empty_batch is None:
                return (torch.empty(0, 1, dtype=torch.float32, device=x.device),)
            raise RuntimeError(self.empty_batch)
        if self.training:
            self._step += 1
        return self._predict(x, self.training, self._step, autograd=self._needs_grad())

    def forward(self, x):
        return self._forward_outputs(x)[0]
