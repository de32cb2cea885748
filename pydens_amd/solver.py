""" `Solver`: same constructor, `fit`, `predict`, `losses` as the reference (pydens/model_torch.py:191-487); the
per-iteration arithmetic runs in the HIP kernels behind include/pinn.h.

Two step paths share every kernel:
  * fused   -- the equation was lowered to a residual program (trace.py): ONE call of pinn_residual_step does
               forward jets, ansatz, residual, MSE and the whole reverse sweep; then pinn_optim_step_at. No torch
               arithmetic and no host synchronisation inside the loop (losses stay on the device).
  * generic -- anything else the reference API allows (trainable `V` variables, callable ICs holding variables,
               constraint terms, user criteria): pinn_jet_forward hands the derivative streams to the user's own
               torch code, torch differentiates those few pointwise ops, pinn_jet_backward turns the upstream
               stream gradients into parameter gradients.
Data parallelism: if torch.distributed is initialised, every rank steps on its own `batch_size` points and the flat
gradient buffer (loss slot included) is summed with one all-reduce (RCCL) per iteration.
"""
import contextlib
import math
import os
from contextvars import copy_context

import numpy as np
import torch
from torch import nn
from tqdm import tqdm

from . import engine, trace
from .balance import LossBalancer
from .causal import CausalWeights
from .model import ConvBlockModel, InputProbe, PROBE
from . import tokens
from .tokens import current_model


UNSET = object()        # Solver._imap outside a step: a custom forward()'s input map has not been asked for


class FlatOptimizer:
    """ torch.optim semantics (reference model_torch.py:419-422, :461) on the flat kernel buffer for the rules the kernels carry
    (include/pinn.h pinn_optim_t): Adam and AdamW with weight decay, SGD, RMSprop -- two state arrays at most, the model's two moment
    buffers. `exp_avg` / `exp_avg_sq` name those buffers for every rule; the torch names of what a rule keeps in them are aliases. """
    # rule -> (code, the keywords it takes besides lr)
    needs_closure = False       # (FlatLBFGS, and TorchOptimizerAdapter around torch.optim.LBFGS: stepped as `step(closure)`)
    RULES = {'Adam': (engine.OPT_ADAM, ('betas', 'eps', 'weight_decay')),
             'AdamW': (engine.OPT_ADAMW, ('betas', 'eps', 'weight_decay')),
             'SGD': (engine.OPT_SGD, ('momentum', 'dampening', 'nesterov', 'weight_decay')),
             'RMSprop': (engine.OPT_RMSPROP, ('alpha', 'eps', 'weight_decay', 'momentum', 'centered'))}

    @classmethod
    def hyper(cls, name, lr, kwargs):
        """ the hyper-parameters torch resolves for `getattr(torch.optim, name)(params, lr=lr, **kwargs)` -- torch's own argument checks raise
        here as they do there -- if the kernels carry that call, else None: another name, another keyword (amsgrad, maximize, foreach,
        capturable, fused, differentiable), a tensor where torch also takes a number, RMSprop with momentum AND centered (three arrays) """
        if name not in cls.RULES or set(kwargs) - set(cls.RULES[name][1]):
            return None
        number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
        values = [lr] + [v for key, v in kwargs.items() if key not in ('betas', 'nesterov', 'centered')]
        betas = kwargs.get('betas', (0.0, 0.0))
        if not all(number(v) for v in values) or not (isinstance(betas, (tuple, list)) and len(betas) == 2 and all(number(b) for b in betas)):
            return None
        hyper = getattr(torch.optim, name)([torch.zeros(1, requires_grad=True)], lr=lr, **kwargs).defaults
        if name == 'RMSprop' and hyper['momentum'] > 0 and hyper['centered']:
            return None
        return {key: hyper[key] for key in ('lr', ) + cls.RULES[name][1]}

    def __init__(self, model, name, lr=0.005, **kwargs):
        hyper = self.hyper(name, lr, kwargs)
        if hyper is None:
            raise NotImplementedError(f'the HIP optimizer kernels do not carry torch.optim.{name}(lr={lr}, **{kwargs})')
        self.name, self.hyper_parameters = name, hyper
        self.torch_kwargs = dict(kwargs)            # (what `TorchOptimizerAdapter.continuing` hands torch.optim)
        self.optim = engine.Optim.build(self.RULES[name][0], **hyper)       # (None: FlatLBFGS, which has entry points of its own)
        self.model, self.lr = model, hyper['lr']
        self.betas, self.eps = tuple(hyper.get('betas', (0.0, 0.0))), hyper.get('eps', 0.0)
        self._take_state(model)

    # what the two buffers hold under a rule, by torch's names (torch.optim state keys)
    STATE_KEYS = {'Adam': ('exp_avg', 'exp_avg_sq'), 'AdamW': ('exp_avg', 'exp_avg_sq'), 'SGD': ('momentum_buffer', None)}

    def state_keys(self):
        """ (torch's state key of the first buffer, of the second); None: the rule does not use that buffer """
        if self.name == 'RMSprop':
            hyper = self.hyper_parameters
            return ('momentum_buffer' if hyper['momentum'] > 0 else ('grad_avg' if hyper['centered'] else None), 'square_avg')
        if self.name == 'SGD':
            return ('momentum_buffer' if self.hyper_parameters['momentum'] != 0 else None, None)
        return self.STATE_KEYS[self.name]

    def __getattr__(self, key):
        if key in ('momentum_buffer', 'grad_avg', 'square_avg') and key in self.state_keys():
            return self.exp_avg if self.state_keys()[0] == key else self.exp_avg_sq
        raise AttributeError(key)

    def _take_state(self, model):
        # the moment buffers and the device step counter belong to the MODEL and are zeroed here: every fit call builds a fresh
        # optimizer (reference :419-422) -- at the same device addresses, so that the launch graph a previous fit call recorded
        # (pinn_fit_steps keys on the addresses its nodes carry) is replayed instead of re-recorded. One live
        # optimizer per model: the Solver never keeps an old one.
        state = getattr(model, '_adam_state', None)
        if state is None or state[0].shape != model.flat.shape or state[0].device != model.flat.device:
            state = model._adam_state = (torch.zeros_like(model.flat), torch.zeros_like(model.flat),
                                         torch.zeros(1, dtype=torch.int32, device=model.flat.device))
        else:
            for t in state:
                t.zero_()
        self.exp_avg, self.exp_avg_sq, self.step_count = state
        self.t = 0                  # host copy of the step counter (the fused single-rank step passes it by value)
        self.mask = None
        self.members = None         # what this optimizer was built over (reference :420: the parameters that required grad THEN)
        # torch's Adam counts steps PER PARAMETER, and one the loss does not reach is not stepped; the kernel has one count for the whole
        # buffer. Per fit call and trainable scalar (log_scale, V(...) slots): was it reached? -> the step count it has in the reference
        self.calls = []             # (step count at its start, set of unreached offsets) per fit call this optimizer served

    def refresh(self, unreached=()):
        """ unreached: offsets of entries (log_scale, V(...) slots, the output bias) the loss terms of the coming fit call do not reach: the
        reference's backward leaves them without a gradient and torch's optimizers SKIP them -- moments, step count and value stay. Reached with
        a gradient that happens to be zero is something else: such an entry is stepped (Solver._unreached_scalars decides from the graph). """
        new = self.model.trainable_mask()
        if self.members is None:
            # (a buffer of the MODEL, like the mask and the moments: a fresh allocation per fit call shifted what the allocator hands the rest
            #  of the call and cost BASELINE config 4's fit 40 ms per call -- tools/fit_one.py, measured)
            kept = getattr(self.model, '_adam_members', None)
            if kept is None or kept.shape != new.shape or kept.device != new.device:
                self.model._adam_members = kept = torch.empty_like(new)
            kept.copy_(new)
            self.members = kept
        else:
            new = new & self.members        # (`fit(optimizer=None)` after unfreeze_trainable: the reused optimizer never heard of that parameter)
        for off in unreached:
            new[off] = 0
        buf = getattr(self.model, '_adam_mask', None)         # (same address from fit to fit, like the moment buffers)
        if buf is None or buf.shape != new.shape or buf.device != new.device:
            self.model._adam_mask = buf = new
        else:
            buf.copy_(new)
        self.mask = buf
        self.calls.append((self.t, set(unreached)))

    def _served(self):
        """ (iterations, unreached offsets) of every fit call so far; the running one last """
        ends = [t0 for t0, _ in self.calls[1:]] + [self.t]
        return [(end - t0, skipped) for (t0, skipped), end in zip(self.calls, ends)]

    def lagging(self, offsets):
        """ scalars that the coming call reaches but some earlier call of this optimizer did not: their step count in the reference is behind
        the buffer's (other bias corrections) -- what one count for the whole buffer cannot express (Solver._fit hands over to torch's Adam) """
        past = self._served()[:-1]
        return [off for off in offsets if off not in self.calls[-1][1] and any(off in skipped and n > 0 for n, skipped in past)]

    def steps_of(self, off):
        return sum(n for n, skipped in self._served() if off not in skipped)

    def set_lr(self, lr):
        """ the learning rate of the coming step(s) (a schedule, Solver.fit(lr_scheduler=...)): every eager call hands it to the library by
        value, through the `Optim` struct (L-BFGS: through `lr`) """
        self.lr = float(lr)
        if self.optim is not None:
            self.optim.lr = self.lr

    def shadow(self):
        """ the one-parameter host optimizer a learning-rate scheduler is built over: it carries `param_groups[0]['lr']` (and the momentum /
        betas a scheduler may look for) and never steps anything -- torch's own scheduler code computes every rate on it """
        if getattr(self, '_shadow', None) is None:
            weight = [torch.zeros(1, requires_grad=True)]
            hyper = self.hyper_parameters
            if 'betas' in hyper:
                self._shadow = torch.optim.Adam(weight, lr=self.lr, betas=tuple(hyper['betas']))
            else:
                self._shadow = torch.optim.SGD(weight, lr=self.lr, momentum=float(hyper.get('momentum', 0.0)))
        return self._shadow

    def step(self, grads, loss_out=None, stream=None):
        """ loss_out: device address that receives grads[off_loss] in the same launch (the fit's loss history) """
        self.t += 1
        self.model.net.optim_step(self.model.flat, grads, self.exp_avg, self.exp_avg_sq, self.mask, self.step_count, self.optim,
                                  at=self.t, loss_out=loss_out, stream=stream)


class FlatAdam(FlatOptimizer):
    """ plain torch.optim.Adam (lr, betas, eps): the default of `Solver.fit` -- the rule 'Adam' without weight decay """
    def __init__(self, model, lr=0.005, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, **kwargs):
        if weight_decay != 0 or amsgrad or kwargs:
            raise NotImplementedError('FlatAdam is plain Adam (lr, betas, eps); got '
                                      f'weight_decay={weight_decay}, amsgrad={amsgrad}, {kwargs}')
        super().__init__(model, 'Adam', lr=lr, betas=betas, eps=eps)


class FlatLBFGS(FlatOptimizer):
    """ torch.optim.LBFGS(lr, max_iter, max_eval, tolerance_grad, tolerance_change, history_size, line_search_fn in (None, 'strong_wolfe')) on
    the flat kernel buffer (include/pinn.h pinn_lbfgs_direction). `step(grads, closure=...)` is torch's `step(closure)`: the same stopping
    rules in the same order, `func_evals` and `n_iter` counted the same way. Per closure evaluation the direction costs three launches --
    whatever the history size -- and ONE read-back of sixteen doubles; without a line search the last launch also takes the step. The
    strong-Wolfe search is torch's own `torch.optim.lbfgs._strong_wolfe` over the flat buffers.
    State on the device, owned by the model like the Adam moments: the rings `S`, `Y` [history_size][p_total] (rows padded to 16 bytes),
    `prev_grad`, `d`, and the control block `ctrl` (ring head and count, H_diag, t, gtd, max|g|, max|t d|, losses, ys / yy of the last pair,
    the combination coefficients and the two Gram matrices). `fit(optimizer=None)` carries all of it on. """
    KEYWORDS = ('max_iter', 'max_eval', 'tolerance_grad', 'tolerance_change', 'history_size', 'line_search_fn')
    # the rings may take this many bytes (2 * history_size * p_total * 4); above it the fit keeps torch.optim.LBFGS, which allocates its
    # history pair by pair as the iterations accept them. 1 GiB: torch's default history of 100 up to 1.3 million parameters.
    HISTORY_BUDGET = 1 << 30
    needs_closure = True

    @classmethod
    def hyper(cls, name, lr, kwargs):
        """ torch's resolved hyper-parameters if the kernels carry `torch.optim.LBFGS(params, lr=lr, **kwargs)`, else None: another keyword, a
        tensor-valued hyper-parameter, an unknown line search. torch's own argument checks raise here as they do there. """
        if name != 'LBFGS' or set(kwargs) - set(cls.KEYWORDS):
            return None
        number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
        integer = lambda v: isinstance(v, int) and not isinstance(v, bool)
        if not number(lr) or not all(number(kwargs.get(key, 0.0)) for key in ('tolerance_grad', 'tolerance_change')):
            return None
        if not integer(kwargs.get('max_iter', 20)) or not integer(kwargs.get('history_size', 100)) or kwargs.get('history_size', 100) < 1:
            return None
        if not (kwargs.get('max_eval') is None or integer(kwargs['max_eval'])) or kwargs.get('line_search_fn') not in (None, 'strong_wolfe'):
            return None
        return dict(torch.optim.LBFGS([torch.zeros(1, requires_grad=True)], lr=lr, **kwargs).defaults)

    @classmethod
    def refusal(cls, model, hyper):
        """ why the kernels do not take this history, in words (None: they do) """
        history, p_total = hyper['history_size'], model.flat.numel()
        need = 2 * history * p_total * 4
        if need > cls.HISTORY_BUDGET:
            return (f'L-BFGS history on the device: 2 * history_size * p_total * 4 = 2 * {history} * {p_total} * 4 = {need} bytes exceed the '
                    f'budget of {cls.HISTORY_BUDGET} bytes (FlatLBFGS.HISTORY_BUDGET); this fit keeps torch.optim.LBFGS')
        if history > engine.LBFGS_MAX_HISTORY:
            return (f'L-BFGS history_size={history}: the kernels run the recursion on history_size x history_size scalars in the LDS of one '
                    f'workgroup, which holds {engine.LBFGS_MAX_HISTORY}; this fit keeps torch.optim.LBFGS')
        return None

    def __init__(self, model, lr=1, **kwargs):
        hyper = self.hyper('LBFGS', lr, kwargs)
        if hyper is None:
            raise NotImplementedError(f'the HIP optimizer kernels do not carry torch.optim.LBFGS(lr={lr}, **{kwargs})')
        message = self.refusal(model, hyper)
        if message is not None:
            raise NotImplementedError(message)
        self.name, self.hyper_parameters, self.optim = 'LBFGS', hyper, None
        self.torch_kwargs = dict(kwargs)
        self.model, self.lr = model, hyper['lr']
        history, flat = hyper['history_size'], model.flat
        ld = (flat.numel() + 3) // 4 * 4
        net = model.net
        state = getattr(model, '_lbfgs_state', None)
        if state is None or state['S'].shape != (history, ld) or state['S'].device != flat.device:
            # (the model's, at the same addresses from fit to fit, like the Adam moments)
            state = model._lbfgs_state = dict(
                S=torch.zeros((history, ld), dtype=torch.float32, device=flat.device), Y=torch.zeros((history, ld), dtype=torch.float32, device=flat.device),
                prev_grad=torch.zeros_like(flat), d=torch.zeros_like(flat),
                ctrl=torch.zeros(net.lbfgs_ctrl_doubles(history), dtype=torch.float64, device=flat.device),
                rows=torch.zeros(net.lbfgs_workspace_bytes(flat.numel(), history) // 8, dtype=torch.float64, device=flat.device))
        else:
            for buf in state.values():
                buf.zero_()
        self.S, self.Y, self.prev_grad, self.d, self.ctrl, self.rows = (state[key] for key in ('S', 'Y', 'prev_grad', 'd', 'ctrl', 'rows'))
        self.func_evals, self.n_iter, self.step_length = 0, 0, 0.0      # torch's state['func_evals'], ['n_iter'], ['t']
        self.closure_calls = 0                                          # ... of the last step
        self.last = None                                                # the control block's head as last read
        self.t, self.mask, self.members, self.calls = 0, None, None, []         # (FlatOptimizer.refresh: fit calls served, members, mask)

    def lagging(self, offsets):
        return []               # (one state for the whole buffer in torch too: nothing per parameter to fall behind)

    @property
    def state(self):
        """ torch's state dict entries that are scalars, read from the device """
        head = dict(zip(engine.LBFGS_CTRL, self.ctrl[:len(engine.LBFGS_CTRL)].tolist()))
        return dict(func_evals=self.func_evals, n_iter=self.n_iter, t=self.step_length, H_diag=head['H_diag'], history=int(head['count']),
                    prev_loss=head['prev_loss'])

    def _direction(self, grads, mode, apply, stream):
        hp = self.hyper_parameters
        self.model.net.lbfgs_direction(self.model.flat, grads, self.prev_grad, self.d, self.S, self.Y, self.mask, hp['history_size'], mode,
                                       apply, self.step_length, self.lr, hp['tolerance_grad'], hp['tolerance_change'], self.ctrl, self.rows,
                                       stream=stream)           # (self.lr: hp['lr'], or this iteration's rate of a schedule -- set_lr)
        self.last = dict(zip(engine.LBFGS_CTRL, self.ctrl[:len(engine.LBFGS_CTRL)].tolist()))       # the ONE read-back per evaluation
        return self.last

    def step(self, grads, loss_out=None, stream=None, closure=None):
        """ torch.optim.LBFGS.step(closure); `closure()` fills `grads` (loss slot included). Returns the first evaluation's loss (0-d, on the
        device). """
        if closure is None:
            raise TypeError("FlatLBFGS.step() needs the closure that re-evaluates loss and gradient")
        from torch.optim.lbfgs import _strong_wolfe
        hp, flat = self.hyper_parameters, self.model.flat
        off_loss = self.model.net.layout.off_loss
        max_iter, max_eval, search = hp['max_iter'], hp['max_eval'], hp['line_search_fn']
        self.closure_calls = 0

        def evaluate():
            closure()
            self.closure_calls += 1
        evaluate()
        first = grads[off_loss].clone()
        self.func_evals += 1
        evals, n_iter, mode, g = 1, 0, engine.LBFGS_START, grads
        live = None
        while n_iter < max_iter:
            c = self._direction(g, mode, search is None, stream)
            if c['stop'] in (1.0, 2.0, 3.0):            # optimality in front of the first direction; inside the loop also lack of progress
                break
            n_iter += 1
            self.n_iter += 1
            self.step_length = c['t']
            if c['stop'] == 4.0:                        # directional derivative above -tolerance_change: no step
                break
            ls_evals = 0
            if search is not None:
                x0, d = flat.clone(), self.d
                live = self.mask.bool() if live is None else live

                def objective(x, t, d):
                    # (masked entries keep their bits: d is zero there, but -0.0 + 0.0 is not -0.0)
                    flat.copy_(torch.where(live, torch.add(x, d, alpha=float(t)), x))
                    evaluate()
                    return float(grads[off_loss]), grads.clone()
                loss, g, t, ls_evals = _strong_wolfe(objective, x0, c['t'], d, c['loss'], g, c['gtd'], max_ls=max_eval - evals)
                flat.copy_(torch.where(live, torch.add(x0, d, alpha=float(t)), x0))
                self.step_length = float(t)
            elif n_iter != max_iter:                    # (the step was taken by the direction's last launch)
                evaluate()
                ls_evals, g = 1, grads
            evals += ls_evals
            self.func_evals += ls_evals
            if n_iter == max_iter or evals >= max_eval:
                break
            mode = engine.LBFGS_LOOP
        self.t += 1
        return first


class TorchOptimizerAdapter:
    """ any other `torch.optim` optimizer the reference accepts by name (model_torch.py:420): torch updates the
    parameter views in place; their .grad are views of the flat gradient buffer the kernels fill. """
    def __init__(self, model, name, lr, **kwargs):
        self.model = model
        self.params = model.optimizer_parameters()
        self.opt = getattr(torch.optim, name)(self.params, lr=lr, **kwargs)

    @property
    def name(self):
        return type(self.opt).__name__

    @classmethod
    def continuing(cls, flat):
        """ the torch optimizer of a FlatOptimizer's rule carrying on where it stands: same members, hyper-parameters, state arrays and -- per
        parameter -- step counts (FlatOptimizer.lagging); a parameter never stepped has no state (SGD: no momentum buffer yet) """
        model = flat.model
        self = cls.__new__(cls)
        self.model = model
        members = flat.members
        self.params = [p for p in model.parameters() if bool(members.as_strided(tuple(p.shape), tuple(p.stride()), p.storage_offset()).any())]
        self.opt = getattr(torch.optim, flat.name)(self.params, lr=flat.lr, **flat.torch_kwargs)
        first, second = flat.state_keys()
        for p in self.params:
            steps = flat.steps_of(p.storage_offset())       # (a fit call reaches a parameter as a whole: its first entry speaks for all)
            if steps > 0:
                view = lambda buf: buf.as_strided(tuple(p.shape), tuple(p.stride()), p.storage_offset()).clone()
                state = {} if flat.name == 'SGD' else {'step': torch.tensor(float(steps))}
                if first is not None:
                    state[first] = view(flat.exp_avg)
                if second is not None:
                    state[second] = view(flat.exp_avg_sq)
                if state:
                    self.opt.state[p] = state
        return self

    def refresh(self, unreached=()):
        """ unreached: offsets in the flat buffer the loss terms of the coming fit call do not reach (Solver._unreached_scalars, as for
        FlatOptimizer.refresh): a parameter that starts at one of them is bound without a gradient, and torch skips it """
        unreached = set(unreached)
        self.unreached = {id(p) for p in self.params if p.storage_offset() in unreached}

    @property
    def needs_closure(self):
        """ torch.optim.LBFGS: `step(closure)` re-evaluates loss and gradient on the same batch, as often as its rule asks """
        import inspect
        closure = inspect.signature(type(self.opt).step).parameters.get('closure')
        return closure is not None and closure.default is inspect.Parameter.empty

    def step(self, grads, loss_out=None, stream=None, closure=None):
        """ closure: the gradient part of the iteration on the batch already drawn; it fills `grads` (loss slot included). With one, the
        optimizer is stepped as `loss = opt.step(closure)` and that loss -- the first evaluation's -- is returned.
        Under torch.distributed the closure ends in the all-reduce, so every rank sees the same gradient and loss and holds the same
        parameters: every rank takes the same decisions (line search, stopping rules) and makes the same number of closure calls -- the
        collectives inside them pair up without any further agreement between the ranks. """
        if closure is not None:
            off_loss = self.model.net.layout.off_loss
            self.closure_calls = 0

            def evaluate():
                closure()
                self.closure_calls += 1
                self._bind(grads, contiguous=True)      # (torch.optim.LBFGS flattens every .grad with view(-1))
                return grads[off_loss].clone()          # (a copy: the slot is overwritten by the next evaluation)
            try:
                return self.opt.step(evaluate)
            finally:
                for p in self.params:
                    p.grad = None
        self._bind(grads)
        self.opt.step()
        for p in self.params:
            p.grad = None

    def _bind(self, grads, contiguous=False):
        # Parameters WITHOUT a gradient are skipped by torch's optimizers -- no weight decay, no momentum step, no step count -- and the
        # reference's backward leaves `.grad = None` on (a) a parameter frozen since this optimizer was built (`fit(optimizer=None)` after
        # freeze_trainable) and (b) a parameter the loss of this call does not reach: `log_scale` without an initial condition, a V(...) of the
        # equation in a constraint-only call, the output bias under a residual of derivatives alone. Which those are is a property of the
        # graph, settled once per fit call (`refresh`); a reached parameter whose gradient is zero gets that zero tensor and is stepped.
        skipped = getattr(self, 'unreached', ())
        for p in self.params:
            reached = p.requires_grad and id(p) not in skipped
            p.grad = grads.as_strided(tuple(p.shape), tuple(p.stride()), p.storage_offset()) if reached else None
            if contiguous and reached:
                p.grad = p.grad.contiguous()


class Solver:
    """ reference model_torch.py:191-487. Extra keyword `device` selects the HIP device (default: current). """
    def __init__(self, equation, ndims, initial_condition=None, boundary_condition=None, domain=(0, 1),
                 nparams=0, model=ConvBlockModel, constraints=None, **kwargs):
        self.equation = equation
        if constraints is None:
            self.constraints = ()
        elif isinstance(constraints, (tuple, list)):
            self.constraints = constraints
        else:
            self.constraints = (constraints, )
        self._losses = []
        self._pending = []
        self.use_fused = True       # diagnostic switch: False keeps every fit on the generic step path
        self.criterion_path = 'generic'     # set_criterion_path: closed-form criteria other than MSELoss() on the fused step or not
        self._crit_sum = False              # reduction='sum' in the fused steps of the running fit
        self.last_fit_criterion = None
        if os.environ.get('PYDENS_AMD_CRITERION'):
            self.set_criterion_path(os.environ['PYDENS_AMD_CRITERION'])
        self.optimizer = None
        self.lr_scheduler = None            # fit(lr_scheduler=...): the live torch.optim.lr_scheduler object
        self.lrs = []                       # the learning rate of every iteration stepped so far (host values; aligned with `losses`)
        self._lr_queue = []                 # rates drawn ahead of the device, one chunk at a time; the head is the next step's
        self.optimizer_path = 'torch'       # set_optimizer_path: optimizers other than plain Adam as torch.optim code or on the fused kernels
        self.last_fit_optimizer = None
        self.last_fit_balance = None        # fit(loss_weights=...): e.g. 'max_mean/fused', 'fixed/generic'; None: the plain sum of the terms
        self._balance = None                # the LossBalancer of the running / last weighted fit
        self._term_history, self._term_pending = [], []     # per weighted fit: (terms, losses [it, T], weights [it, T]) / the device histories
        self.last_fit_causal = None         # fit(causal=...): e.g. 'bins32/generic'; None: the equation term is the plain mean
        self._causal = None                 # the CausalWeights of the running / last causal fit
        self._causal_run = None             # ... and, while its fit runs, where the running iteration's rows of the histories are
        self._causal_history, self._causal_pending = [], []     # per causal fit: (weights [it, M], eps [it], mean r^2 [it]) / the device histories
        self.optimizer_refusal = None       # why the last `fit(optimizer='LBFGS')` under the 'fused' path kept torch.optim (None: it did not)
        if os.environ.get('PYDENS_AMD_OPTIMIZER'):
            self.set_optimizer_path(os.environ['PYDENS_AMD_OPTIMIZER'])

        self.model = model(**kwargs, ndims=ndims, initial_condition=initial_condition,
                           boundary_condition=boundary_condition, domain=domain, nparams=nparams)
        # the reference's plug-in seam (`Solver(model=...)`, model_torch.py:299-313): subclasses of ConvBlockModel that
        # change how the fully connected net / the ansatz parameters are set up run on the HIP kernels; a subclass that
        # replaces `forward` may put its own torch code AROUND the network -- `self.anzatc(self.conv_block(xs), xs) * g(xs)`, another
        # output transform, no ansatz at all: `self.conv_block(xs)` is then the bare network on the kernels and the rest runs as torch
        # ops on its value and derivative streams (generic step path; `D` applies the chain rule); a fixed map of each point onto as many
        # columns in front of the net is followed too (_input_map). Anything else -- a model that is not a ConvBlockModel, a map in front
        # of the net that is trainable, changes the number of columns or looks at the whole batch -- is refused
        if not isinstance(self.model, ConvBlockModel):
            raise NotImplementedError('Solver(model=...): only ConvBlockModel and its subclasses (fully connected layouts; a custom '
                                      'forward() may wrap torch code around self.conv_block(xs)) are backed by the HIP kernels')
        self.custom_forward = self.model.custom_forward
        self._imap = UNSET                                                # custom forward(): _input_map of the running step
        self._map_pattern, self._map_affine, self._map_scale = None, False, None       # ... and what _check_input_map found at construction
        current_model.set(self.model)                                     # :316-317
        self.ctx = copy_context()
        self.device = self.model.flat.device
        lay = self.model.net.layout
        self.grads = torch.zeros(lay.p_total, dtype=torch.float32, device=self.device)
        self._generator = None
        self._sample_seed, self._sample_calls = None, 0      # Philox key / batch counter of the device sampler
        self._broadcast_done = False
        self._comm = None                                    # data-parallel communicator (comm.Communicator)

        # "fake run" (:319-325): materialises V-variables and, here, tells which derivative streams D(...) needs
        if self.model.initial_condition is not None and self.model.ic_constant is None and not self.custom_forward:
            fake = torch.rand((3, self.model.total), device=self.device)
            self.ctx.run(self.model.ic_values, fake)
        self._trace_equation()
        # constraint terms (:451-457) the tracer can lower run as further residual programs over the value stream on
        # their own few points; the others keep the generic path (entry None, reason in constraint_errors)
        self.constraint_plans, self.constraint_errors = [], []
        self.constraint_specs = []           # per constraint: one StreamSpec per model call it makes (_discover_constraint)
        self.constraint_dry_run_errors = []  # ... or why that dry run failed (None: it did not)
        self._born_in_constraint = {}        # constraint number -> variables first created by tracing it (dormant until
        self._constraints_seen = set()       # a fit call has evaluated that constraint: reference :420 vs :457)
        for num, constraint in enumerate(self.constraints):
            before = set(self.model.variables)
            self._compile_constraint(num, constraint)
            self._born_in_constraint[num] = set(self.model.variables) - before
            self.model.dormant_variables |= self._born_in_constraint[num]
        self._traced_constraints = tuple(self.constraints)

    def set_gemm_mode(self, mode):
        """ arithmetic of the hidden-layer GEMMs of the fused step: 'fp32' (default; exact-fp32 MFMA) or 'bf16x3' (every fp32
        operand as three bf16, six partial products, fp32 accumulate -- the split-bf16 kernels where they are built, the fp32
        kernels elsewhere; include/pinn.h pinn_set_gemm_mode). Also settable for a whole process with PYDENS_AMD_GEMM. """
        self.model.net.set_gemm_mode(mode)

    CRITERION_PATHS = ('generic', 'fused')

    def set_criterion_path(self, path):
        """ where `fit(criterion=...)` other than `nn.MSELoss()` runs: 'generic' (default: the criterion module is called on the residual
        as torch code, between pinn_jet_forward and pinn_jet_backward) or 'fused' -- nn.L1Loss, nn.SmoothL1Loss, nn.HuberLoss and
        nn.MSELoss with reduction 'mean' or 'sum' are evaluated in closed form inside the point stage of the fused step (include/pinn.h
        PINN_CRIT_*), for the equation term and every lowered constraint term; everything else (other modules, subclasses, callables,
        reduction='none') keeps the generic path in either setting. Process-wide: PYDENS_AMD_CRITERION. """
        if path not in self.CRITERION_PATHS:
            raise ValueError(f'criterion path {path!r}: expected one of {sorted(self.CRITERION_PATHS)}')
        self.criterion_path = path

    OPTIMIZER_PATHS = ('torch', 'fused')

    def set_optimizer_path(self, path):
        """ where `fit(optimizer=...)` other than plain Adam runs: 'torch' (default: torch.optim updates views of the flat buffer, a train of
        launches behind the gradient reduction) or 'fused' -- Adam and AdamW with weight decay, SGD (momentum, dampening, nesterov, weight
        decay) and RMSprop (alpha, weight decay, momentum OR centered) are applied by the kernels (include/pinn.h pinn_optim_t): in the
        gradient reduction's launch, in the fit chunks and their launch graphs, in the one-CU chunk kernel. Matched by exact name and
        keywords; anything else (amsgrad, maximize, ..., other optimizers) stays on torch.optim in either setting. L-BFGS (lr, max_iter,
        max_eval, tolerance_grad, tolerance_change, history_size, line_search_fn None or 'strong_wolfe') becomes `FlatLBFGS`: direction
        kernels at three launches per closure evaluation; under data parallelism, with other keywords or with a history beyond
        `FlatLBFGS.HISTORY_BUDGET` bytes it stays torch.optim.LBFGS, which `fit` steps through a closure on either path.
        `last_fit_optimizer` tells, e.g. 'AdamW/fused'. Process-wide: PYDENS_AMD_OPTIMIZER. """
        if path not in self.OPTIMIZER_PATHS:
            raise ValueError(f'optimizer path {path!r}: expected one of {sorted(self.OPTIMIZER_PATHS)}')
        self.optimizer_path = path

    def _lbfgs_on_the_kernels(self, optimizer, lr, kwargs):
        """ does `fit(optimizer='LBFGS', ...)` take FlatLBFGS under the 'fused' optimizer path? Not with other keywords or tensor-valued
        hyper-parameters, not under data parallelism (every rank would keep a history of the same all-reduced gradients: torch.optim does that),
        not with a history beyond the memory budget -- `optimizer_refusal` then says why, with the byte count. """
        self.optimizer_refusal = None
        if optimizer != 'LBFGS':
            return False
        hyper = FlatLBFGS.hyper(optimizer, lr, kwargs)
        if hyper is None or self._world()[1] > 1:
            return False
        self.optimizer_refusal = FlatLBFGS.refusal(self.model, hyper)
        if self.optimizer_refusal is not None:
            import warnings
            warnings.warn('pydens_amd: ' + self.optimizer_refusal, RuntimeWarning)
        return self.optimizer_refusal is None

    def _lower_criterion(self, criterion):
        """ (code, parameter, sum) of a criterion the point stage has in closed form, else None. By EXACT type: a subclass may override
        forward(). `nn.MSELoss(reduction='mean')` is always lowerable (the fused step's own loss); the others only on the 'fused'
        criterion path. """
        reduction = getattr(criterion, 'reduction', None)
        if reduction not in ('mean', 'sum'):
            return None
        if isinstance(criterion, nn.MSELoss) and reduction == 'mean':      # (as before this switch existed: subclasses included)
            return (engine.CRIT_MSE, 0.0, False)
        if self.criterion_path != 'fused':
            return None
        kind = type(criterion)
        if kind is nn.MSELoss:
            return (engine.CRIT_MSE, 0.0, reduction == 'sum')
        if kind is nn.L1Loss:
            return (engine.CRIT_L1, 0.0, reduction == 'sum')
        if kind is nn.SmoothL1Loss:
            beta = float(criterion.beta)
            if beta < 0.0:
                return None
            # (beta = 0 is L1, as in torch)
            return (engine.CRIT_SMOOTH_L1, beta, reduction == 'sum') if beta > 0.0 else (engine.CRIT_L1, 0.0, reduction == 'sum')
        if kind is nn.HuberLoss:
            delta = float(criterion.delta)
            return (engine.CRIT_HUBER, delta, reduction == 'sum') if delta > 0.0 else None
        return None

    def _apply_criterion(self, lowered, nums_constraints):
        """ write the criterion of this fit call into the residual structs its fused steps hand to the library """
        code, param, reduce_sum = lowered
        self._crit_sum = reduce_sum
        if self.program is not None:
            self.program.set_criterion(code, param, reduce_sum)
        for num in nums_constraints:
            if num < len(self.constraint_plans) and self.constraint_plans[num] is not None:
                self.constraint_plans[num]['program'].set_criterion(code, param, reduce_sum)

    def set_tanh_mode(self, mode):
        """ 'fast' (default) or 'accurate': tanh of small arguments by a minimax polynomial in the kernels that have that form (the
        Poisson-box shape of BASELINE configs 1 / 2 at width 64) -- gradient error on trained models 0.6 - 1.2x the fp32 reference's own
        instead of 1.7 - 1.9x, for +2.5 % kernel time (include/pinn.h pinn_set_tanh_mode). Process-wide: PYDENS_AMD_TANH. """
        self.model.net.set_tanh_mode(mode)

    def _conv_block_argument(self, pts, inside=False):
        """ run the custom forward() up to its call of `self.conv_block` and return that call's argument """
        model = self.model
        model.raw_field = PROBE
        try:
            model.forward(pts) if inside else self.ctx.run(model.forward, pts)         # (inside: the caller runs in self.ctx already)
        except InputProbe as probe:
            ys = probe.arg
        else:
            raise NotImplementedError('Solver(model=...): this forward() never calls self.conv_block(xs) -- a model that is not the '
                                      'fully connected net of its layout is arbitrary torch code the HIP kernels cannot see')
        finally:
            model.raw_field = None
        if not torch.is_tensor(ys):
            raise NotImplementedError('a custom forward() must call self.conv_block on a tensor of points')
        return ys

    def _input_map(self, pts, inside=False, known_scale=False):
        """ custom forward(): what does it hand to `self.conv_block`? Asked in every step (a probe call of the forward()).
          None               the batch itself;
          (ys, scale, None)  a fixed per-column affine map `ys[:, k] = a_k * pts[:, k] + b_k` (input normalisation, `2 * xs - 1`): the kernels
                             evaluate the network and its derivative streams AT ys, and a derivative of multi-index alpha with respect to the
                             solver's own columns is the stream times prod_{k in alpha} a_k (_eval_equation);
          (ys, None, pattern) any other fixed map of a point onto as many columns (`torch.sin(xs)`, a time warp, columns mixed): streams at ys
                             with respect to the network's input columns, chain rule with the map's Jacobian by torch autograd
                             (trace.StreamContext._through_map; pattern[k][c] = "ys_k depends on column c", found at construction).
        What the reference's seam (model_torch.py:52-54) also takes and this does not: a map that depends on trainable parameters (its
        gradient would need the streams' own derivatives), on the batch as a whole, or that changes the number of columns (the reference
        builds `conv_block` for `total` inputs, :167): NotImplementedError.
        known_scale: the few points of a constraint's own model call, where a column often holds ONE value (`t0 = zeros`, a face `x = 1`):
        such a column takes the scale the construction found on its 64 random points; a batch of the equation is refused instead. """
        pts = pts.detach()
        ys = self._conv_block_argument(pts, inside)
        if (ys.data_ptr() == pts.data_ptr() and ys.shape == pts.shape and ys.stride() == pts.stride() and ys.dtype == pts.dtype
                and ys.device == pts.device):
            return None
        refusal = 'a custom forward() may call self.conv_block only on the batch of points it was given or on a fixed pointwise map of it '
        if ys.requires_grad:
            raise NotImplementedError(refusal + '(this one depends on trainable parameters)')
        if ys.shape != pts.shape:
            raise NotImplementedError(refusal + f'onto as many columns (shape {tuple(ys.shape)} from points of shape {tuple(pts.shape)})')
        ys32 = ys.detach().to(torch.float32).contiguous()
        if self._map_pattern is not None:                   # (known since construction to be more than a per-column affine map)
            return ys32, None, self._map_pattern
        x64, y64 = pts.double(), ys.detach().double()
        if not bool(torch.isfinite(y64).all()):
            raise NotImplementedError(refusal + '(not finite on this batch)')
        lo, hi = x64.argmin(dim=0), x64.argmax(dim=0)
        k = torch.arange(x64.shape[1], device=x64.device)
        span = x64[hi, k] - x64[lo, k]
        flat = span <= 0                                    # a column without two different values: only the identity is recognisable,
        known = torch.ones_like(span)                       # or the scale the construction found (a constraint's points: `t0 = zeros`)
        known_scale = known_scale and self._map_affine and self._map_scale is not None
        if known_scale:
            known = torch.tensor(self._map_scale, dtype=torch.float64, device=x64.device)
        a = torch.where(flat, known, (y64[hi, k] - y64[lo, k]) / torch.where(flat, torch.ones_like(span), span))
        b = y64[lo, k] - a * x64[lo, k]                     # (a flat column of an unknown map must come through unchanged: a = 1, b = 0)
        if not known_scale:
            b = torch.where(flat, torch.zeros_like(span), b)
        # (fp32 arithmetic of the user's map: a few ulp of its largest intermediate)
        err = (y64 - (a * x64 + b)).abs() - 1e-5 * ((a * x64).abs() + b.abs() + y64.abs())
        if float(err.max()) <= 0.0:
            return ys32, [float(v) for v in a.tolist()], None
        if self._map_affine:
            raise NotImplementedError(refusal + '(per-column affine on the points of the construction, not on this batch: a column without two '
                                      'different values cannot tell its scale)')
        return ys32, None, None

    def _check_input_map(self):
        """ construction: what kind of map does the custom forward() put in front of the network (refusals happen here and not in the first
        fit call), is it a map of each point by itself, and -- if it is not per-column affine -- which input column of the network depends
        on which column of the solver. """
        total = self.model.total
        self._map_pattern, self._map_affine, self._map_scale = None, False, None
        pts = torch.rand((64, total), device=self.device)
        imap = self._input_map(pts)
        if imap is None:
            return
        self._map_affine = imap[1] is not None
        self._map_scale = imap[1]
        part = self._input_map(pts[:23].contiguous())
        if part is None or not torch.allclose(part[0], imap[0][:23], rtol=1e-6, atol=1e-7):
            raise NotImplementedError('a custom forward() may call self.conv_block only on a map of each point by itself (this one depends on '
                                      'the batch as a whole: the reference differentiates such a map across the rows of the batch, the '
                                      'kernels see one point at a time)')
        if imap[1] is not None:
            return
        p = pts.clone().requires_grad_()
        ys = self._conv_block_argument(p)
        pattern = []
        for k in range(total):
            g = torch.autograd.grad(ys[:, k].sum(), p, retain_graph=True, allow_unused=True)[0] if ys.requires_grad else None
            pattern.append([False] * total if g is None else [bool(v) for v in (g != 0).any(dim=0).tolist()])
        self._map_pattern = pattern

    def _equation_of_the_network(self, net_value, *cols):
        """ custom forward(): the equation as a function of the BARE network's value (tagged: `D` finds its derivative streams)
        and the input columns -- u_hat = model.forward(points) is torch code around it (reference model_torch.py:437-447) """
        model = self.model
        pts = torch.cat(cols, dim=1)                        # = reshape_and_concat of [N,1] columns (:345-362)
        imap = self._imap
        if imap is UNSET:                                   # (the fake run of the tracer: no kernel has run, the question is asked here)
            imap = self._input_map(pts, inside=True)
        if imap is not None and imap[1] is None:
            # a general map in front of the net: the streams are derivatives with respect to the NETWORK's input columns; `D` goes through
            # the map's Jacobian (trace.StreamContext._through_map), taken from the graph this very forward() call builds
            trace.active_streams.get().ymap = {'cols': cols, 'pattern': imap[2], 'ys': None, 'jac': {}}
        model.raw_field = (pts, net_value, None if imap is None else imap[0])
        try:
            u_hat = model.forward(pts)
        finally:
            model.raw_field = None
        return self.equation(u_hat, *cols)

    def _trace_equation(self):
        """ which streams does the equation need, and can it be lowered to a residual program? (construction, and again at
        the start of a fit call whenever the cached lowering no longer reproduces the live callable) """
        self._eq = self._equation_of_the_network if self.custom_forward else self.equation
        if self.custom_forward:
            self._check_input_map()
        self.spec, self.needs_x_grad = trace.discover(self._eq, self.ctx.run, self.model.total, self.device,
                                                      hp=self.model.net.layout.hp, allact=self.model.net.allact)
        if self.custom_forward:
            # torch code between the network and the equation: generic step path only
            self.needs_x_grad = True
            self.ic_var_slot, self.ic_trainable, self.residual_plan = None, False, None
            self.program, self.program_error = None, 'the model has its own forward(): torch code around the network (generic path)'
            self._traced_equation = self.equation
            return
        # a callable initial condition that IS one scalar trainable variable (`lambda *a: V('init', ...)`, reference
        # examples notebook cells 80-88) stays on the fused path: the kernels read it from its user slot and return its
        # gradient there (pinn_residual_t::ic_var1); any other dependence on variables needs torch autograd (generic path)
        self.ic_var_slot = self._ic_variable_slot()
        self.ic_trainable = self.ic_var_slot is None and self._ic_depends_on_variables()
        self.residual_plan = None
        self.program, self.program_error = self._try_compile()
        self._traced_equation = self.equation

    def _refresh_traces(self, nums_constraints):
        """ The reference calls `equation(u_hat, *xs)` and the constraints in EVERY iteration (model_torch.py:448, :457), so
        a closure constant changed between two fit calls, a re-assigned `solver.equation` or new constraint points take
        effect there. Here they were lowered once: re-check the cached lowering against the live callables at the start of
        every fit call (17 random points, a few torch ops) and lower again on any mismatch. """
        if self.equation is not self._traced_equation:
            self._trace_equation()
        elif self.program is not None and self.residual_plan is not None:
            try:
                # (a callable initial condition lowered into the pre-pass is part of the cached lowering: the reference calls
                #  it in every iteration too, model_torch.py:125)
                ok = self._plan_matches(self.residual_plan) and self._ic_matches(self.residual_plan)
            except (trace.TraceUnsupported, NotImplementedError, RuntimeError, TypeError, ValueError):
                ok = False
            if not ok:
                self._trace_equation()
        if tuple(self.constraints) != self._traced_constraints or nums_constraints:
            for num, constraint in enumerate(self.constraints):
                if num < len(self.constraint_plans) and num not in nums_constraints and \
                        num < len(self._traced_constraints) and constraint is self._traced_constraints[num]:
                    continue
                known = num < len(self._traced_constraints) and constraint is self._traced_constraints[num]
                before = set(self.model.variables)
                self._compile_constraint(num, constraint)
                if not known:
                    # a constraint appended after construction: variables its tracing brings to life are dormant until a fit
                    # call has evaluated it, exactly as for the constraints __init__ saw (reference :420 vs :457)
                    born = set(self.model.variables) - before
                    self._born_in_constraint[num] = self._born_in_constraint.get(num, set()) | born
                    if num not in self._constraints_seen:
                        self.model.dormant_variables |= born
            self._traced_constraints = tuple(self.constraints)

    # ---- tracing ---------------------------------------------------------------------------------------------------
    def _ic_variable_slot(self):
        m = self.model
        if m.initial_condition is None or m.ic_constant is not None:
            return None
        cols = [torch.rand(3, device=self.device) for _ in range(m.ndims_spatial)]
        val = self.ctx.run(m.initial_condition, *cols)
        if isinstance(val, nn.Parameter) and val.numel() == 1 and val.requires_grad:
            return self._variable_slot(val)
        return None

    def _ic_depends_on_variables(self):
        m = self.model
        if m.initial_condition is None or m.ic_constant is not None:
            return False
        fake = torch.rand((3, m.total), device=self.device)
        return bool(self.ctx.run(m.ic_values, fake).requires_grad)

    def _plan_matches(self, plan):
        """ validation on random data: lowered residual (fp64 host interpreter) vs the user's callable on tagged tensors """
        total, n = self.model.total, 17
        streams = torch.rand((self.spec.n_streams, n), device=self.device) * 2 - 1
        pts = torch.rand((n, total), device=self.device) + 0.25
        # (an equation that differentiates composite expressions needs autograd over its own pointwise ops)
        probe = streams.clone().requires_grad_() if self.needs_x_grad else streams
        want = self._eval_equation(probe, pts, requires_grad=self.needs_x_grad)
        want = want.detach().reshape(-1).double().cpu().numpy()
        lay = self.model.net.layout
        var_values = self.model.flat[lay.off_extra:lay.off_extra + plan.n_vars].detach().cpu().numpy()
        got = trace.run_residual_numpy(plan, streams.cpu().numpy(), pts.cpu().numpy(), var_values)
        return bool(np.allclose(got, want, rtol=1e-4, atol=1e-5))

    def _ic_matches(self, plan):
        """ the initial-condition rows of the pre-pass against torch autograd over the live callable on random points """
        if plan.ic_row is None:
            return True
        pts = torch.rand((17, self.model.total), device=self.device) + 0.25
        want = self._ic_stream_tensor(pts, plan.comb_w)
        got = trace.run_ic_numpy(plan, pts.cpu().numpy().astype(np.float64))
        return got.shape == tuple(want.shape) and bool(np.allclose(got, want.double().cpu().numpy(), rtol=1e-4, atol=1e-5))

    def _try_compile(self):
        """ lower the equation to a residual program and cross-check it numerically against the callable. """
        total = self.model.total
        try:
            root = trace.symbolic(self.equation, self.ctx.run, total, variable_slot=self._variable_slot)
            ic_root = self._symbolic_initial_condition()
            if self.spec.mixed3 or self.spec.n4 > 0 or self.spec.mixed111:
                raise trace.TraceUnsupported('mixed third-order partials / fourth-order derivatives run on the generic path')
            plan = trace.lower_residual(root, self.spec, total, ic_root=ic_root)
            trace.combine_second_order(plan, self.spec)
            if not self._plan_matches(plan):
                raise trace.TraceUnsupported('traced program disagrees with the callable (data-dependent control flow?)')
            if plan.comb_w is None and not self.spec.single_call:
                raise trace.TraceUnsupported(f'{self.spec} needs several kernel calls (generic path)')
            self._attach_initial_condition(plan, ic_root)
            self.residual_plan = plan
            return self._with_ic_variable(plan.to_struct()), None
        except trace.TraceUnsupported as err:
            return None, str(err)

    def _symbolic_initial_condition(self):
        """ Sym DAG of a callable IC without trainable variables, or None (constant / trainable / untraceable IC) """
        m = self.model
        self.ic_lowering_error = None
        if m.initial_condition is None or m.ic_constant is not None or self.ic_var_slot is not None or self.ic_trainable:
            return None
        try:
            return trace.symbolic_initial_condition(m.initial_condition, self.ctx.run, m.ndims_spatial)
        except trace.TraceUnsupported as err:
            self.ic_lowering_error = str(err)
            return None

    def _attach_initial_condition(self, plan, ic_root):
        """ callable IC without trainable variables: IC(x) and its derivative streams join the x-only pre-pass (symbolic
        differentiation, trace.attach_initial_condition / lower_residual), so that a fused step holds no torch arithmetic
        at all; anything the tracer cannot lower keeps `_ic_streams` (torch autograd over the callable, per iteration). """
        if ic_root is None:
            return
        try:
            if plan.kind == trace.RES_AFFINE:
                trace.attach_initial_condition(plan, self.spec, ic_root)
            if plan.ic_row is None:
                raise trace.TraceUnsupported('initial condition does not fit the pre-pass')
            # validation against torch autograd over the callable on random points
            if not self._ic_matches(plan):
                raise trace.TraceUnsupported('lowered initial condition disagrees with the callable')
        except (trace.TraceUnsupported, NotImplementedError) as err:
            plan.ic_row, plan.ic_const = None, None          # (unused rows stay in the pre-pass: harmless)
            self.ic_lowering_error = str(err)

    def _try_compile_constraint(self, constraint):
        """ -> ({'program', 'plan', 'points', 'ic'}, None) or (None, reason). """
        model, total = self.model, self.model.total
        if self.custom_forward:
            return None, 'the model has its own forward()'
        if self.ic_trainable:
            return None, 'initial condition holds trainable variables'
        try:
            root, pts = trace.symbolic_constraint(
                constraint, self.ctx.run, total,
                lambda args: self.reshape_and_concat(args).numpy(), variable_slot=self._variable_slot)
            lay = model.net.layout
            # the streams the constraint's `D` asks of its one model call (none: a value constraint, as ever)
            try:
                spec = trace.StreamSpec(trace.requested_streams(root), hp=lay.hp, allact=model.net.allact)
            except NotImplementedError as err:      # (what the kernels do not carry at this width: the fit call that uses the term raises it)
                raise trace.TraceUnsupported(str(err)) from err
            # one call record per constraint: what one call of the constraint kernels cannot serve keeps the generic path
            if spec.n3 > 0 or spec.n4 > 0:
                raise trace.TraceUnsupported(f'{spec}: third- and fourth-order derivatives in a constraint run on the generic path')
            if not spec.single_call:
                raise trace.TraceUnsupported(f'{spec} needs several kernel calls (more than one direction group: generic path)')
            plan = trace.lower_residual(root, spec, total)
            # validation: the program (fp64 host interpreter) vs the callable fed with stand-ins for the model's value and every stream
            n_c = pts.shape[0]
            values = torch.rand((n_c, 1), device=self.device) * 2 - 1
            streams = values.reshape(1, -1)
            if spec.n_streams > 1:
                streams = torch.cat([streams, torch.rand((spec.n_streams - 1, n_c), device=self.device) * 2 - 1], dim=0)
            cols = [torch.from_numpy(pts[:, c:c + 1].copy()).to(self.device) for c in range(total)]

            def stand_in(*args):
                if spec.nd == 0:
                    return values
                sc = self._tag_streams(trace.StreamContext(total).bind_args(args), spec, streams)       # (`D` resolves to the stand-in streams)
                trace.active_streams.set(sc)
                return sc.tensors[()]
            try:
                want = self.ctx.run(trace.call_constraint, constraint, stand_in, *cols)
            except (TypeError, ValueError, AttributeError, RuntimeError, LookupError, NotImplementedError) as err:
                raise trace.TraceUnsupported(f'{type(err).__name__}: {err}') from err
            want = torch.as_tensor(want).detach().reshape(-1).double().cpu().numpy()
            var_values = model.flat[lay.off_extra:lay.off_extra + plan.n_vars].detach().cpu().numpy()
            got = trace.run_residual_numpy(plan, streams.cpu().numpy(), pts, var_values)
            if got.shape != want.shape or not np.allclose(got, want, rtol=1e-4, atol=1e-5):
                raise trace.TraceUnsupported('traced constraint disagrees with the callable')
        except trace.TraceUnsupported as err:
            return None, str(err)
        points = torch.from_numpy(pts).to(self.device).contiguous()
        # the callable initial condition at the constraint's points, one row per stream: computed once, the points are constants
        ic = None
        if model.initial_condition is not None and model.ic_constant is None and self.ic_var_slot is None:
            if spec.nd == 0:
                with torch.no_grad():
                    ic = self.ctx.run(model.ic_values, points).expand(points.shape[0], 1).reshape(1, -1).float().contiguous()
            else:
                ic = self._ic_stream_tensor(points, None, spec).contiguous()
        return dict(program=self._with_ic_variable(plan.to_struct()), plan=plan, points=points, ic=ic, spec=spec,
                    dir_cols=list(spec.dir_cols), n2p=spec.n2p), None

    def _with_ic_variable(self, residual):
        residual.ic_var1 = 0 if self.ic_var_slot is None else self.ic_var_slot + 1
        return residual

    def _constraint_step(self, num, world, accumulate):
        """ gradient + loss of constraint term `num` (the fit's criterion on its values, reference :457: their mean square by default),
        added to / stored in `self.grads`; every data-parallel rank evaluates it, hence the 1 / world in front of the all-reduce. """
        cp, model = self.constraint_plans[num], self.model
        n_c = 1 if self._crit_sum else cp['points'].shape[0]            # (reduction='sum': no division by the number of points)
        # (a constraint that differentiates the model carries the directions of its streams: one launch of that instantiation)
        spec = cp['spec']
        ws = model.workspace(n_c, 0, 0) if spec.nd == 0 else model.workspace(cp['points'].shape[0], spec.nd, cp['n2p'])
        model.net.residual_step(cp['program'], model.flat, cp['points'], self.grads, ws, cp['dir_cols'], cp['n2p'],
                                ic_streams=cp['ic'], ic_const=model.kernel_ic_const(),
                                inv_n_global=1.0 / (n_c * world), accumulate=accumulate)

    def _variable_slot(self, param):
        """ user slot (index behind `off_extra` in the flat buffer) of a scalar trainable V(...), else None. """
        if param.numel() != 1:
            return None
        lay = self.model.net.layout
        for name, (off, n) in self.model.variables.items():
            if getattr(self.model, name) is param and n == 1:
                return off - lay.off_extra
        return None

    @staticmethod
    def _tag_streams(sc, spec, streams, ic_streams=None, scale=None):
        """ the kernel streams of `spec` ([S, N], or a list of rows) as tagged [N, 1] tensors of the stream context `sc`, the
        user-visible mixed partials combined from their diagonals: what `D` picks from. For the equation on the batch and for every
        model call of a constraint alike. """
        def tag(t, alpha):
            # streams taken at an affine map of the points (custom forward(), _input_map): chain rule back to the solver's columns
            if scale is not None and alpha:
                t = t * math.prod(scale[c] for c in alpha)
            return sc.tag(t, alpha)
        full = {}
        for alpha, idx in spec.index.items():
            t = streams[idx].view(-1, 1)
            if ic_streams is not None and ic_streams[idx] is not None:
                t = t + ic_streams[idx]
            full[idx] = t
            if all(isinstance(c, int) for c in alpha):          # ('d', a, b) diagonal streams are not user-visible
                # (a node of its own in the autograd graph: the combinations below are built from `full`, NOT from tagged tensors -- `D` of an
                #  expression asks autograd for the partial derivative with respect to every tagged stream, and a mixed partial that hung
                #  below the tagged u_aa would be counted in d / d u_aa a second time)
                tag(t.view_as(t), alpha)
        for ab, (ivv, iaa, ibb) in spec.mixed.items():      # u_ab = (u_vv - u_aa - u_bb) / 2
            tag(0.5 * (full[ivv] - full[iaa] - full[ibb]), ab)
        for alpha, (ip, im, ia, ib) in spec.mixed4.items():         # u_aabb = (D4_{a+b} + D4_{a-b} - 2 u_aaaa - 2 u_bbbb) / 12
            tag((full[ip] + full[im] - 2.0 * full[ia] - 2.0 * full[ib]) / 12.0, alpha)
        for alpha, terms in list(spec.mixed31.items()) + list(spec.mixed111.items()):
            # u_aaab / u_abbb from D4 along a +- b and 2a +- b; u_abc from D3 along a +- b +- c (round 6)
            tag(sum(coef * full[idx] for idx, coef in terms), alpha)
        for alpha, (ip, im, i3, sign) in spec.mixed3.items():      # u_aab = (D3_{a+b} - D3_{a-b} - 2 u_bbb) / 6, u_abb: + D3_{a-b}, - 2 u_aaa
            tag((full[ip] + sign * full[im] - 2.0 * full[i3]) / 6.0, alpha)
        return sc

    def _streams_forward(self, kpts, spec, slot=0):
        """ the streams of `spec` at the points `kpts` [S, N] (no autograd): one pinn_jet_forward, or one per direction group.
        slot: which call of the step this is (the equation: 0) -- the cached row indices of the groups are kept per call """
        model = self.model
        if len(spec.groups) == 1:
            return model.net.jet_forward(model.flat, kpts, spec.dir_cols, spec.n2p, ic_const=model.kernel_ic_const())
        # more directions than one kernel call carries: one forward per group of directions (u comes with each)
        leaf = torch.empty((spec.n_streams, kpts.shape[0]), dtype=torch.float32, device=self.device)
        for num, (dirs_g, n2g, idx) in enumerate(spec.groups):
            part = model.net.jet_forward(model.flat, kpts, dirs_g, n2g, ic_const=model.kernel_ic_const())
            leaf.index_copy_(0, self._group_rows((slot, num), idx), part)
        return leaf

    def _streams_backward(self, kpts, spec, grad, slot=0):
        """ upstream gradients of the streams [S, N] -> parameter gradients, ADDED to `self.grads` (pinn_jet_backward, per group) """
        model = self.model
        if len(spec.groups) == 1:
            ws = model.workspace(kpts.shape[0], spec.nd, spec.n2p)
            model.net.jet_backward(model.flat, kpts, grad.contiguous(), self.grads, ws, spec.dir_cols, spec.n2p,
                                   ic_const=model.kernel_ic_const(), accumulate=True)
            return
        # the parameter gradient is linear in the upstream stream gradients: one backward per group, the
        # gradient of u itself rides with the first group only
        for num, (dirs_g, n2g, idx) in enumerate(spec.groups):
            gin = grad.index_select(0, self._group_rows((slot, num), idx))
            if num > 0:
                gin[0].zero_()
            ws = model.workspace(kpts.shape[0], len(dirs_g), n2g)
            model.net.jet_backward(model.flat, kpts, gin, self.grads, ws, dirs_g, n2g,
                                   ic_const=model.kernel_ic_const(), accumulate=True)

    def _eval_equation(self, streams, xs, ic_streams=None, requires_grad=True):
        """ run the user's callable on stream tensors [S,N] (+ optional IC streams), D resolves to streams. """
        total = self.model.total
        imap = self._imap if self.custom_forward else None
        scale = None if imap is None or imap is UNSET or imap[1] is None or all(a == 1.0 for a in imap[1]) else imap[1]
        sc = self._tag_streams(trace.StreamContext(total), self.spec, streams, ic_streams, scale)
        cols = []
        for c in range(total):
            col = xs[:, c:c + 1]
            if self.needs_x_grad and requires_grad:
                col = col.clone().requires_grad_()
            col._pinn_col = c
            cols.append(col)
        return self.ctx.run(trace.call_with_streams, sc, self._eq, sc.tensors[()], *cols)

    def _ic_streams(self, xs, create_graph, spec=None):
        """ IC(x_spatial) and its derivative streams as a list over stream indices ([N,1] tensors or None). spec: the equation's, or
        that of a constraint's model call. """
        own_points = spec is not None            # (a constraint's model call: often ONE point, `p = torch.tensor([[1.0]])`)
        m, spec = self.model, (self.spec if spec is None else spec)
        if own_points and xs.shape[0] == 1 and m.ic_constant is None:
            # (a callable IC that returns ONE value is taken for a constant below: a lone point is evaluated as two copies of itself)
            return [None if t is None else t[:1] for t in self._ic_streams(xs.repeat(2, 1), create_graph, spec)]
        cols = [xs[:, i].clone().requires_grad_() for i in range(m.ndims_spatial)]
        val = self.ctx.run(m.initial_condition, *cols)
        if not isinstance(val, torch.Tensor):
            val = torch.tensor(float(val), dtype=torch.float32, device=xs.device)
        val = val.to(xs.device).float()
        out = [None] * spec.n_streams
        out[0] = val.view(-1, 1) if val.numel() > 1 else val.reshape(1, 1).expand(xs.shape[0], 1)
        if val.numel() > 1 and val.requires_grad:
            def along(f, direction):
                """ directional derivative of f over the SPATIAL columns of a direction (IC ignores t / parameters) """
                total = None
                for c, weight in trace.dir_weights(direction):
                    if c < m.ndims_spatial and f is not None and f.requires_grad:
                        (g,) = torch.autograd.grad(f.sum(), cols[c], create_graph=True, retain_graph=True, allow_unused=True)
                        if g is not None:
                            g = g if weight == 1.0 else weight * g
                            total = g if total is None else total + g
                return total
            for k, direction in enumerate(spec.dirs):
                g1 = along(val, direction)
                if g1 is None:
                    continue
                out[1 + k] = g1.view(-1, 1)
                if k < spec.n2:
                    g2 = along(g1, direction)
                    if g2 is not None:
                        out[1 + spec.nd + k] = g2.view(-1, 1)
                        if k < spec.n3:
                            g3 = along(g2, direction)
                            if g3 is not None:
                                out[1 + spec.nd + spec.n2 + k] = g3.view(-1, 1)
                                if k < spec.n4:
                                    g4 = along(g3, direction)
                                    if g4 is not None:
                                        out[1 + spec.nd + spec.n2 + spec.n3 + k] = g4.view(-1, 1)
        if not create_graph:
            out = [None if t is None else t.detach() for t in out]
        return out

    def _ic_stream_tensor(self, xs, comb_w, spec=None):
        """ [S_kernel, N] IC streams by torch autograd over the callable (ICs the tracer could not lower) """
        spec = self.spec if spec is None else spec
        n2 = spec.n2 if comb_w is None else 1
        parts = self._ic_streams(xs, create_graph=False, spec=spec)
        ic_streams = torch.zeros((1 + spec.nd + n2 + (spec.n3 if comb_w is None else 0), xs.shape[0]), dtype=torch.float32,
                                 device=self.device)
        for i, t in enumerate(parts):
            if t is None:
                continue
            if comb_w is not None and i > spec.nd:
                ic_streams[1 + spec.nd] += comb_w[i - 1 - spec.nd] * t.reshape(-1)
            else:
                ic_streams[i] = t.reshape(-1)
        return ic_streams

    # ---- reference API -----------------------------------------------------------------------------------------------
    @property
    def losses(self):
        """ list of 0-d numpy arrays, one per iteration (reference model_torch.py:308, :464); device-side history is
        fetched lazily so that `fit` itself never synchronises. """
        if self._pending:
            for chunk, done in self._pending:       # `done`: iterations the fit call completed (all, unless interrupted)
                self._losses.extend(np.float32(v) for v in chunk.detach().cpu().numpy().reshape(-1)[:done[0]])
            self._pending = []
            self._losses = [np.asarray(v) for v in self._losses]
        return self._losses

    @losses.setter
    def losses(self, value):
        self._pending, self._losses = [], list(value)

    def _weight_histories(self):
        """ the device histories of the weighted fits so far, fetched lazily like `losses` """
        for terms, term_hist, weight_hist, done in self._term_pending:
            self._term_history.append((terms, term_hist[:done[0]].detach().cpu().numpy().copy(), weight_hist[:done[0]].detach().cpu().numpy().copy()))
        self._term_pending = []
        return self._term_history

    def _stacked_history(self, which):
        runs = self._weight_histories()
        if not runs:
            return np.zeros((0, 0), dtype=np.float32)
        terms = runs[-1][0]         # (fits over other terms have rows of another width: the rows of the latest set of terms are returned)
        return np.concatenate([run[which] for run in runs if run[0] == terms], axis=0)

    @property
    def term_losses(self):
        """ [iterations, T] float32: the UNWEIGHTED loss of every term of `loss_terms`, one row per iteration of the fits with
        `loss_weights` (those over the latest set of terms); `losses` holds the weighted sum, which is what is optimised """
        return self._stacked_history(1)

    @property
    def loss_weight_history(self):
        """ [iterations, T] float32: the weights each of those iterations was stepped with """
        return self._stacked_history(2)

    @property
    def loss_weights(self):
        """ {term: weight} of the last fit with `loss_weights`, read back from the device (None: there was none) """
        return None if self._balance is None else self._balance.weights

    @classmethod
    def reshape_and_concat(cls, tensors, device=None):
        """ Input casting of reference model_torch.py:327-362 -> float32 [N, D] (on `device` if given). """
        items = list(tensors)
        lengths = [int(np.prod(np.shape(t))) for t in items
                   if isinstance(t, (np.ndarray, torch.Tensor, tuple, list))]
        n = max(lengths) if lengths else 1
        cols = []
        for x in items:
            if isinstance(x, torch.Tensor):
                col = x.reshape(-1, 1).float()
            elif isinstance(x, np.ndarray):
                arr = x if x.size == n else np.tile(x.squeeze()[0], (n, 1))            # :355-356
                col = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32).reshape(n, 1))
            elif isinstance(x, (list, tuple)):
                col = torch.tensor(x, dtype=torch.float32).view(-1, 1)
            else:
                col = torch.full((n, 1), float(x), dtype=torch.float32)
            if device is not None:
                col = col.to(device)
            cols.append(col)
        return torch.cat(cols, dim=1)

    def _group_rows(self, num, idx):
        """ stream rows of direction group `num` as a device index tensor, built once (indexing with a Python list uploads it in every
        step, which a launch-graph recording refuses) """
        cache = self.__dict__.setdefault('_group_row_cache', {})
        key = (num, tuple(idx))
        if key not in cache:
            cache[key] = torch.tensor(list(idx), dtype=torch.long, device=self.device)
        return cache[key]

    def _points_on_device(self, pts):
        """ reshape_and_concat(pts) on the device. Small HOST constants -- the fixed points a constraint builds in every call,
        `f(torch.tensor([0.5]))` -- are looked up by content in a cache of device tensors: no host-to-device copy per iteration, and
        nothing in the step that a launch-graph recording would refuse (pageable-memory copies are not capturable). """
        key = []
        for x in pts:
            if isinstance(x, torch.Tensor):
                if x.is_cuda or x.requires_grad or x.numel() > 4096:
                    return self.reshape_and_concat(pts, device=self.device)
                try:
                    key.append(('t', str(x.dtype), tuple(x.shape), x.detach().contiguous().numpy().tobytes()))
                except (TypeError, RuntimeError):       # (a dtype numpy does not have: no cache entry, the plain upload)
                    return self.reshape_and_concat(pts, device=self.device)
            elif isinstance(x, np.ndarray):
                if x.size > 4096:
                    return self.reshape_and_concat(pts, device=self.device)
                key.append(('a', str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes()))
            elif isinstance(x, (list, tuple, int, float)):
                key.append(('v', repr(x)))
            else:
                return self.reshape_and_concat(pts, device=self.device)
        cache = self.__dict__.setdefault('_host_constants', {})
        key = tuple(key)
        if key not in cache:
            if len(cache) >= 64:
                cache.clear()
            cache[key] = self.reshape_and_concat(pts, device=self.device)
        return cache[key]

    def _world(self):
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            return dist.get_rank(), dist.get_world_size()
        return 0, 1

    def _device_guard(self):
        """ the library launches on the CURRENT device: make the model's device current where it is not """
        if self.device.type == 'cuda' and torch.cuda.current_device() != self.device.index:
            return torch.cuda.device(self.device)
        return contextlib.nullcontext()

    def _new_sample_seed(self):
        """ Philox key of the device sampler: drawn from torch's default generator, like the `torch.rand` calls of the
        reference's default sampler (model_torch.py:431) follow `torch.manual_seed`; per-rank offset under data parallelism """
        rank, _ = self._world()
        base = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        self._sample_seed = (base + 7919 * rank) & (2 ** 64 - 1)

    def _sample(self, batch_size, sampler, stream=None):
        """ reference model_torch.py:430-434: default U[0,1) columns (domain is ignored, trap 3 of SURVEY 8a),
        or `sampler.sample(batch_size)`. Products of independent uniform / normal / constant columns -- the default
        sampler and every `NumpySampler(...) & ...` of the reference's examples -- are drawn in HBM by ONE launch of the
        Philox kernel (pinn_sample_points); other samplers through `sample_device` or, last, numpy + a copy. """
        total = self.model.total
        columns = [(engine.SAMPLE_UNIFORM, 0.0, 1.0)] * total if sampler is None else \
            (sampler.columns() if hasattr(sampler, 'columns') else None)
        if columns is not None and len(columns) == total and total <= engine.MAX_INPUTS:
            if self._sample_seed is None:
                self._new_sample_seed()
            seed, call = self._sample_seed, self._sample_calls
            own = sampler.device_key() if hasattr(sampler, 'device_key') else None
            if own is not None:
                # `NumpySampler(..., seed=k)`: the reference draws from THAT seeded generator (model_torch.py:433), whatever
                # torch's seed is -- the sampler's seed keys the Philox stream and the sampler counts its own batches
                rank, _ = self._world()
                seed, call = (own + 7919 * rank) & (2 ** 64 - 1), sampler.next_device_call()
            xs = torch.empty((batch_size, total), dtype=torch.float32, device=self.device)
            self.model.net.sample_points(xs, columns, seed, call, stream=stream)
            self._sample_calls += 1
            return xs
        if self._generator is None:
            rank, _ = self._world()
            self._generator = torch.Generator(device=self.device)
            self._generator.manual_seed(torch.initial_seed() + 7919 * rank)
        if hasattr(sampler, 'sample_device'):
            xs = sampler.sample_device(batch_size, self.device, self._generator)
        else:
            xs = torch.from_numpy(np.asarray(sampler.sample(batch_size)).astype(np.float32)).to(self.device)
        if xs.shape[1] != total:
            raise ValueError(f'sampler produced {xs.shape[1]} columns, the problem has {total}')
        return xs.contiguous()

    # ---- data parallelism ---------------------------------------------------------------------------------
    def begin_data_parallel(self):
        """ once per process group: parameters of rank 0 everywhere, and a communicator whose all-reduce is enqueued on the
        COMPUTE stream (RCCL called directly -- no side stream, no event hops between the kernels of an iteration) """
        _, world = self._world()
        dist = torch.distributed
        if not (dist.is_available() and dist.is_initialized()):
            return
        if not self._broadcast_done:
            dist.broadcast(self.model.flat, src=0)
            self._broadcast_done = True
        if self._comm is None:
            from . import comm
            self._comm = comm.Communicator(self.device)

    def end_data_parallel(self):
        if self._comm is not None:
            self._comm.close()
            self._comm = None

    def _all_reduce(self, stream=None, tensor=None):
        if self._comm is None:
            self.begin_data_parallel()
        if self._comm is not None:              # (no process group: single process, nothing to exchange)
            self._comm.all_reduce_(self.grads if tensor is None else tensor, stream)

    def _dp_step(self, xs, world, stream=None, loss_out=None):
        """ one data-parallel iteration on this rank's shard `xs`: tile kernel + reduction, all-reduce of the flat gradient
        buffer (network, log_scale, loss slot, V slots) on the same stream, ONE Adam launch that also records the loss """
        self._fused_step(xs, world, stream=stream)
        self._all_reduce(stream)
        self.optimizer.step(self.grads, loss_out=loss_out, stream=stream)

    def _unreached_scalars(self, loss_terms, nums_constraints, criterion):
        """ offsets in the flat buffer of what the loss of these terms does not REACH, although it is trainable: log_scale without an initial
        condition, a V(...) of the equation in a constraint-only call, the output bias under a residual that holds derivatives of the
        network alone. The reference's backward leaves those without a gradient and torch's optimizers skip them (no decay, no momentum
        step, no step count); everything else is stepped, also where its gradient is zero -- a variable behind a zero co-factor, a
        coefficient that is switched on elsewhere in the domain, a sum that cancels on one batch. So the decision is taken from the GRAPH,
        never from a value: one dry evaluation of the terms through the generic step per fit call, asked for connectivity only
          * V(...):      `.grad is None` after the backward of the dry evaluation (all entries of a vector variable together);
          * log_scale:   reached exactly when an initial condition is bound (a model with its own forward(): torch autograd tells);
          * output bias: reached when the network's VALUE is -- through a constraint term, the equation's u, or a derivative stream along
                         a direction in which the ansatz factor varies (boundary binding: spatial columns; initial condition: time).
        The points of the dry evaluation are five U[0, 1) draws from a generator of its own: connectivity does not depend on where the
        terms are evaluated (nor on the sampler's domain), and the call's sampler is not asked for a batch it would then be short of.
        A dry evaluation that fails (the fit itself will say why) leaves everything reached. """
        model, lay = self.model, self.model.net.layout
        if not any(term == 'equation' or 'constraint' in term for term in loss_terms):
            return []
        probe = {}
        keep = self.grads.clone()
        try:
            gen = torch.Generator(device=self.device)           # (its own stream: the solver's sampling seeds come from torch's global one)
            gen.manual_seed(5)
            self._generic_step(torch.rand((5, model.total), device=self.device, generator=gen), loss_terms,
                               [num for num in nums_constraints if num < len(self.constraints)], criterion, 1, probe=probe)
        except Exception:
            return []
        finally:
            self.grads.copy_(keep)
        unreached = []
        if not (probe['log_scale'] if self.custom_forward else model.initial_condition is not None):
            unreached.append(lay.off_log_scale)
        for name, (off, n) in model.variables.items():
            if name not in probe['variables']:
                unreached.extend(range(off, off + n))
        if not self._value_reached(probe):
            bias = [m for m in model.conv_block][-1].bias
            unreached.extend(range(bias.storage_offset(), bias.storage_offset() + bias.numel()))
        return unreached

    def _value_reached(self, probe):
        """ does the loss of the dry evaluation hold the network's value (and with it the output bias, which the derivatives of the network
        do not hold)? `probe['streams']`: per kernel stream, whether the backward gave it a gradient. Stream 0 is u; the derivative streams
        along direction k hold the value through the product rule where the ansatz factor varies along k. """
        if probe.get('value') or not probe['streams']:
            return bool(probe.get('value'))
        return self._streams_reach_value(probe['streams'], self.spec)

    def _streams_reach_value(self, streams, spec):
        """ `streams`: per kernel stream of `spec`, whether the backward gave it a gradient -- the equation's on the batch, or those of a
        model call a constraint made at its own points """
        model = self.model
        if streams[0]:
            return True
        varying = set()
        if not self.custom_forward:             # (its ansatz is torch code around the value stream: autograd has told through stream 0)
            if model.boundary_condition is not None:
                varying |= set(range(model.ndims_spatial))
            if model.initial_condition is not None:
                varying.add(model.ndims - 1)
        for k, direction in enumerate(spec.dirs):
            rows = [1 + k] + [base + k for base, count in ((1 + spec.nd, spec.n2), (1 + spec.nd + spec.n2, spec.n3),
                                                           (1 + spec.nd + spec.n2 + spec.n3, spec.n4)) if k < count]
            if any(streams[row] for row in rows) and any(c in varying for c, _ in trace.dir_weights(direction)):
                return True
        return False

    def fit(self, niters, batch_size, sampler=None, loss_terms='equation', optimizer='Adam',
            criterion=nn.MSELoss(), lr=0.005, **kwargs):
        """ reference model_torch.py:364-464. Under torch.distributed `batch_size` stays the GLOBAL number of points per
        iteration (the reference's meaning); rank r steps on its share of it.
        `lr_scheduler`: the name of a class in torch.optim.lr_scheduler (built with `lr_scheduler_kwargs`) or a callable
        `factory(optimizer) -> scheduler`; the torch loop `opt.step(); sched.step()` once per iteration, on every step path
        (`_set_scheduler`). `fit(optimizer=None)` carries the running schedule on; a new optimizer without one has a constant rate. """
        lr_scheduler, lr_scheduler_kwargs = kwargs.pop('lr_scheduler', None), kwargs.pop('lr_scheduler_kwargs', None)
        loss_weights, causal = kwargs.pop('loss_weights', None), kwargs.pop('causal', None)
        with self._device_guard():
            return self._fit(niters, batch_size, sampler, loss_terms, optimizer, criterion, lr, lr_scheduler, lr_scheduler_kwargs,
                             loss_weights=loss_weights, causal=causal, **kwargs)

    # ---- causal training weights ----------------------------------------------------------------------------------------------------
    def _check_causal(self, causal, loss_terms, optimizer, criterion, lr, loss_weights, kwargs):
        """ `fit(causal=...)`: every refusal, raised before the call has changed anything. Served: the generic step with nn.MSELoss(), one
        process, an optimizer that steps once per batch. With `loss_weights` the combination is refused: the term rows would have to be
        evaluated with the causal weights inside the 'equation' row and recorded once per iteration, which is code of its own. """
        if not isinstance(causal, CausalWeights):
            raise ValueError(f'causal={causal!r}: a CausalWeights object (or None)')
        if 'equation' not in loss_terms:
            raise ValueError(f"causal: the weights act on the equation term, and 'equation' is not among loss_terms={list(loss_terms)}")
        if type(criterion) is not nn.MSELoss or criterion.reduction != 'mean':
            raise NotImplementedError(f'causal: the weighted equation term is mean_i w_i r_i^2, the form of nn.MSELoss() with mean '
                                      f'reduction; got {criterion!r}')
        if self._steps_by_closure(optimizer, lr, kwargs):
            raise NotImplementedError('causal: an optimizer that steps through a closure (L-BFGS) re-evaluates the batch inside one step, '
                                      'and the weights and the tolerance ladder must not move under its line search')
        if self._world()[1] > 1:
            raise NotImplementedError('causal: under torch.distributed every rank would weight its share of the batch by its own bin sums; '
                                      'the all-reduce of the bin sums is not built')
        if loss_weights is not None:
            raise NotImplementedError('causal: together with loss_weights -- the term rows of a weighted fit are evaluated apart, and the '
                                      "causal weights inside the 'equation' row are not built; use one of the two")
        resolved = causal.resolve(self.model)
        if causal.state is not None and causal.state.device != self.device:
            raise ValueError(f'causal: this CausalWeights lives on {causal.state.device}, the solver on {self.device}')
        if self.custom_forward:
            # (the bins are those of the batch's own time column: a forward() that hands the network another time is not followed)
            devices = [self.device] if self.device.type == 'cuda' else []
            with torch.random.fork_rng(devices=devices):
                pts = torch.rand((64, self.model.total), device=self.device)
                imap = self._input_map(pts)
            if imap is not None and not torch.equal(imap[0][:, resolved[0]], pts[:, resolved[0]]):
                raise NotImplementedError(f"causal: this model's forward() maps the time column {resolved[0]} before the network sees it; the "
                                          'bins would be those of another time than the network is trained on')

    @property
    def causal_weight_history(self):
        """ [iterations, M] float32: the bin weights w_k every iteration of the fits with `causal` was stepped with (those over the latest
        number of bins), fetched lazily like `losses` """
        return self._causal_stacked(1)

    @property
    def causal_eps_history(self):
        """ [iterations] float32: the tolerance of each of those iterations """
        return self._causal_stacked(2)

    @property
    def residual_mse_history(self):
        """ [iterations] float32: the UNWEIGHTED mean r^2 of the equation term of each of those iterations (`losses` holds the weighted loss) """
        return self._causal_stacked(3)

    def _causal_stacked(self, which):
        for bins, weight_hist, eps_hist, mse_hist, done in self._causal_pending:
            self._causal_history.append((bins, ) + tuple(h[:done[0]].detach().cpu().numpy().copy() for h in (weight_hist, eps_hist, mse_hist)))
        self._causal_pending = []
        runs = self._causal_history
        if not runs:
            return np.zeros((0, 0) if which == 1 else (0, ), dtype=np.float32)
        bins = runs[-1][0]
        return np.concatenate([run[which] for run in runs if run[0] == bins], axis=0)

    # ---- loss-term weights ---------------------------------------------------------------------------------------------------------
    def _steps_by_closure(self, optimizer, lr, kwargs):
        """ will the optimizer of the coming fit call re-evaluate the batch inside one step (`step(closure)`: L-BFGS)? """
        if optimizer is None:
            return bool(self.optimizer is not None and self.optimizer.needs_closure)
        import inspect
        cls = getattr(torch.optim, optimizer, None) if isinstance(optimizer, str) else None
        closure = inspect.signature(cls.step).parameters.get('closure') if cls is not None else None
        return closure is not None and closure.default is inspect.Parameter.empty

    def _resolve_loss_weights(self, loss_weights, loss_terms, by_closure):
        """ `fit(loss_weights=...)` -> the LossBalancer that serves the call (None: the plain sum, today's code), or the refusal, raised
        before the call has changed anything: a dict by term name or a sequence aligned with `loss_terms` (constant weights), or a
        LossBalancer (adaptive; the object owns its device state and carries it from fit to fit) """
        if loss_weights is None:
            return None
        terms = tuple(loss_terms)
        for term in terms:
            num = term.replace('constraint', '').replace('_', '') if isinstance(term, str) and 'constraint' in term else None
            if term != 'equation' and not (num is not None and num.isdigit() and int(num) < len(self.constraints)):
                raise ValueError(f"loss_weights: the loss term {term!r} is neither 'equation' nor one of the {len(self.constraints)} constraints of "
                                 'this solver; only those are evaluated term by term')
        if len(terms) > engine.BALANCE_MAX_TERMS:
            raise NotImplementedError(f'loss_weights: {len(terms)} loss terms; the kernels combine at most {engine.BALANCE_MAX_TERMS}')
        if isinstance(loss_weights, LossBalancer):
            balance = loss_weights
        elif isinstance(loss_weights, dict):
            balance = LossBalancer.fixed(loss_weights)
        elif isinstance(loss_weights, (tuple, list, np.ndarray)):
            if len(loss_weights) != len(terms):
                raise ValueError(f'loss_weights: {len(loss_weights)} weights for the {len(terms)} terms of loss_terms={list(terms)}')
            if len(set(terms)) != len(terms):
                raise ValueError(f'loss_weights: loss_terms={list(terms)} names a term twice')
            balance = LossBalancer.fixed(dict(zip(terms, [w.item() if isinstance(w, np.generic) else w for w in loss_weights])))
        else:
            raise ValueError(f'loss_weights={loss_weights!r}: a dict by term name, a sequence aligned with loss_terms, or a LossBalancer')
        refusal = balance.refusal(terms, by_closure)
        if refusal is not None:
            raise refusal
        return balance

    def _term_rows(self, n_terms):
        """ [T, ld] gradient rows of the weighted step, one per term (ld: p_total rounded up to a 16-byte piece), kept from fit to fit """
        ld = (self.grads.numel() + 3) // 4 * 4
        rows = getattr(self, '_balance_rows', None)
        if rows is None or rows.shape != (n_terms, ld) or rows.device != self.grads.device:
            rows = self._balance_rows = torch.zeros((n_terms, ld), dtype=torch.float32, device=self.device)
        return rows

    def _weighted_step(self, xs, loss_terms, criterion, world, fused, wb, it=None, stream=None):
        """ the gradient part of one iteration under loss weights: every term of `loss_terms` is evaluated by the code that evaluates it in
        the plain sum -- its gradient buffer pointed at row j of one [T, ld] tensor, accumulation off --, under torch.distributed the
        stacked rows are all-reduced in ONE call (every rank computes the same weights), and pinn_balance_terms writes `self.grads`:
        weighted gradient, weighted loss in the loss slot. `it`: the row of the term / weight histories this evaluation is recorded in
        (None: not recorded -- the later evaluations of a closure step). The generic step runs eagerly, once per term. """
        rows, n, grads = wb['rows'], self.grads.numel(), self.grads
        try:
            for j, term in enumerate(loss_terms):
                self.grads = rows[j, :n]
                if fused and term == 'equation':
                    self._fused_step(xs, world, stream=stream)
                elif fused:
                    self._constraint_step(wb['nums'][j], world, accumulate=False)
                else:
                    self._generic_step(xs, (term, ), [] if term == 'equation' else [wb['nums'][j]], criterion, world)
        finally:
            self.grads = grads
        if world > 1:
            self._all_reduce(stream, rows)
        record = it is not None
        wb['balance'].combine(self.model.net, rows, n, wb['mask'], self.grads,
                              term_loss_out=wb['term_ptr'] + 4 * len(loss_terms) * it if record else None,
                              weight_out=wb['weight_ptr'] + 4 * len(loss_terms) * it if record else None, count=record, stream=stream)

    # ---- learning-rate schedules -------------------------------------------------------------------------------------------------
    def _scheduled_optimizer(self):
        """ the torch optimizer a scheduler is built over: the real one (TorchOptimizerAdapter) or the flat optimizer's host shadow """
        opt = self.optimizer
        return opt.opt if isinstance(opt, TorchOptimizerAdapter) else opt.shadow()

    def _set_scheduler(self, spec, kwargs, fresh):
        """ `fit(lr_scheduler=spec, lr_scheduler_kwargs=kwargs)`. Semantics: torch's `opt.step(); sched.step()` per iteration; the rate of
        iteration k is what `param_groups[0]['lr']` reads in front of step k. The rates are torch's own: its scheduler code runs on the host,
        over the real optimizer on the torch path, over a one-parameter shadow optimizer for the flat optimizers -- there they are drawn a chunk
        ahead into a queue and travel to the kernels per iteration (include/pinn.h pinn_fit_steps, lr_steps). fresh: a new optimizer. """
        if spec is None:
            if fresh:
                self.lr_scheduler, self._lr_queue = None, []
            return
        target = self._scheduled_optimizer()
        if self._lr_queue:
            # (rates drawn ahead that no step used: the optimizer's rate is that of its NEXT step again before torch's rules look at it)
            target.param_groups[0]['lr'] = self._lr_queue[0]
        before = [(g['lr'], g.get('initial_lr')) for g in target.param_groups]
        cycled = [(g.get('momentum'), g.get('betas')) for g in target.param_groups]
        previous = (self.lr_scheduler, list(self._lr_queue))
        self.lr_scheduler, self._lr_queue = None, []

        def restore():
            # (the optimizer stays as it was: usable by a later fit(optimizer=None), at its own rate)
            del target.param_groups[len(before):]
            for g, (rate, initial) in zip(target.param_groups, before):
                g['lr'] = rate
                if initial is None:
                    g.pop('initial_lr', None)
                else:
                    g['initial_lr'] = initial
            for g, (momentum, betas) in zip(target.param_groups, cycled):
                if momentum is not None:
                    g['momentum'] = momentum
                if betas is not None:
                    g['betas'] = betas
            self.lr_scheduler, self._lr_queue = (None, []) if fresh else previous

        def refuse(error, message):
            restore()
            raise error(message)
        if isinstance(spec, str):
            cls = getattr(torch.optim.lr_scheduler, spec, None)
            if not (isinstance(cls, type) and (issubclass(cls, torch.optim.lr_scheduler.LRScheduler) or spec == 'ReduceLROnPlateau')):
                refuse(ValueError, f'lr_scheduler={spec!r}: torch.optim.lr_scheduler has no scheduler class of that name')
            build = lambda opt: cls(opt, **(kwargs or {}))
        elif callable(spec):
            if kwargs:
                refuse(ValueError, 'lr_scheduler_kwargs go with the NAME of a scheduler class; a factory builds its scheduler itself')
            build = spec
        else:
            refuse(ValueError, f'lr_scheduler must be the name of a class in torch.optim.lr_scheduler or a callable, got {spec!r}')
        try:
            sched = build(target)
        except Exception:           # (torch's own argument checks raise here as they do in the torch loop)
            restore()
            raise
        import inspect
        needs = [p.name for p in inspect.signature(sched.step).parameters.values()
                 if p.default is inspect.Parameter.empty and p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
        if needs:
            refuse(NotImplementedError, f'lr_scheduler {type(sched).__name__}: its step() needs {needs} -- a metric-driven schedule would read '
                                        'the loss back to the host every iteration, which Solver.fit never does; out of scope')
        self.lr_scheduler = sched
        message = self._rate_refusal()
        if message is not None:
            refuse(NotImplementedError, message)
        if not isinstance(self.optimizer, TorchOptimizerAdapter):
            if [(g.get('momentum'), g.get('betas')) for g in target.param_groups] != cycled:
                refuse(NotImplementedError, f'lr_scheduler {type(sched).__name__} also schedules momentum / betas, which the HIP optimizer '
                                            'kernels take as constants of a fit; pass cycle_momentum=False')
            target.step()       # (nothing to step: torch's order check then sees opt.step() in front of the first sched.step())

    def _rate_refusal(self):
        """ why the scheduler's current rate cannot be stepped with, in words (None: it can) """
        groups = self.lr_scheduler.optimizer.param_groups
        if len(groups) != 1:
            return f'lr_scheduler {type(self.lr_scheduler).__name__} leaves {len(groups)} param groups; the kernels step ONE flat buffer at one rate'
        rate = groups[0]['lr']
        if not isinstance(rate, (int, float)) or not math.isfinite(rate) or rate < 0:
            return f'lr_scheduler {type(self.lr_scheduler).__name__} gives the learning rate {rate!r}; a rate must be a finite number >= 0'
        return None

    def _draw_rates(self, k):
        """ the rates of the next k steps of a flat optimizer, in `_lr_queue`: read, then `sched.step()`, as often as needed """
        sched = self.lr_scheduler
        while len(self._lr_queue) < k:
            message = self._rate_refusal()
            if message is not None:
                raise NotImplementedError(message)
            self._lr_queue.append(float(sched.optimizer.param_groups[0]['lr']))
            sched.step()
        return self._lr_queue[:k]

    def _rate_begin(self):
        """ in front of ONE step of the per-iteration paths: the step's rate, handed to the optimizer (None: no schedule) """
        if self.lr_scheduler is None:
            return None
        opt = self.optimizer
        if isinstance(opt, TorchOptimizerAdapter):
            if self.lr_scheduler.optimizer is opt.opt:
                return float(opt.opt.param_groups[0]['lr'])
            # (TorchOptimizerAdapter.continuing took over from a flat optimizer in the middle of its schedule: the shadow goes on carrying it)
            rate = self._draw_rates(1)[0]
            for group in opt.opt.param_groups:
                group['lr'] = rate
            return rate
        rate = self._draw_rates(1)[0]
        opt.set_lr(rate)
        return rate

    def _rate_end(self, rate):
        """ behind that step: the schedule moves on, the rate is on record """
        if rate is None:
            opt = self.optimizer
            self.lrs.append(float(opt.opt.param_groups[0]['lr'] if isinstance(opt, TorchOptimizerAdapter) else opt.lr))
            return
        if self._lr_queue:
            self._lr_queue.pop(0)
        else:
            self.lr_scheduler.step()
            message = self._rate_refusal()
            if message is not None:
                raise NotImplementedError(message)
        self.lrs.append(rate)

    def _fit(self, niters, batch_size, sampler, loss_terms, optimizer, criterion, lr, lr_scheduler=None, lr_scheduler_kwargs=None,
             loss_weights=None, causal=None, **kwargs):
        model = self.model
        balance = None
        if causal is not None:                  # (refusals first: the call has changed nothing yet)
            self._check_causal(causal, loss_terms if isinstance(loss_terms, (tuple, list)) else (loss_terms, ), optimizer, criterion, lr,
                               loss_weights, kwargs)
            if optimizer is None and self.optimizer is None:
                raise ValueError('optimizer=None reuses the optimizer of a previous fit call; there is none yet')
        if loss_weights is not None:            # (refusals first: the call has changed nothing yet)
            balance = self._resolve_loss_weights(loss_weights, loss_terms if isinstance(loss_terms, (tuple, list)) else (loss_terms, ),
                                                 self._steps_by_closure(optimizer, lr, kwargs))
        for num in self._constraints_seen:          # variables an earlier fit call brought to life are trainable now
            model.dormant_variables -= self._born_in_constraint.get(num, set())
        if optimizer is not None:                                                          # :419-422
            plain_adam = optimizer == 'Adam' and not kwargs.get('weight_decay') and not kwargs.get('amsgrad') and \
                not (set(kwargs) - {'betas', 'eps', 'weight_decay', 'amsgrad'})
            if plain_adam:
                self.optimizer = FlatAdam(model, lr=lr, **kwargs)
            elif self.optimizer_path == 'fused' and FlatOptimizer.hyper(optimizer, lr, kwargs) is not None:
                self.optimizer = FlatOptimizer(model, optimizer, lr=lr, **kwargs)
            elif self.optimizer_path == 'fused' and self._lbfgs_on_the_kernels(optimizer, lr, kwargs):
                self.optimizer = FlatLBFGS(model, lr=lr, **kwargs)
            else:
                self.optimizer = TorchOptimizerAdapter(model, optimizer, lr, **kwargs)
        elif self.optimizer is None:
            raise ValueError('optimizer=None reuses the optimizer of a previous fit call; there is none yet')
        self._set_scheduler(lr_scheduler, lr_scheduler_kwargs, fresh=optimizer is not None)
        self._generic_graph = None          # launch graphs of the generic step are recorded per fit call (closure constants may have changed)
        model.train()
        loss_terms = loss_terms if isinstance(loss_terms, (tuple, list)) else (loss_terms, )
        nums_constraints = [int(term.replace('constraint', '').replace('_', ''))
                            for term in loss_terms if 'constraint' in term]
        self._refresh_traces(set(nums_constraints))
        if isinstance(self.optimizer, TorchOptimizerAdapter) or model.variables or not isinstance(self.optimizer, FlatAdam) or balance is not None:
            # (what the terms of THIS call reach decides what torch's optimizers do with a parameter: one dry evaluation per fit call, asked
            #  for graph connectivity -- _unreached_scalars. Plain Adam on a model without variables need not know: nothing changes from call
            #  to call there, and its update of an entry that never has a gradient is no move at all; weight decay would move it, and a
            #  variable's reach differs from call to call, so every other case asks)
            # (loss weights: an entry no term reaches is not a live entry of the statistics -- mean|g| divides by the live count)
            unreached = self._unreached_scalars(loss_terms, nums_constraints, criterion)
            self.optimizer.refresh(unreached)
            if optimizer is None and isinstance(self.optimizer, FlatOptimizer):
                lay = model.net.layout
                bias = [m for m in model.conv_block][-1].bias
                scalars = [lay.off_log_scale, bias.storage_offset()] + [off + i for off, n in model.variables.values() for i in range(n)]
                if self.optimizer.lagging(scalars):
                    self.optimizer = TorchOptimizerAdapter.continuing(self.optimizer)
                    self.optimizer.refresh(unreached)
        else:
            unreached = ()
            self.optimizer.refresh()
        self._constraints_seen |= {num for num in nums_constraints if num < len(self.constraints)}
        crit = self._lower_criterion(criterion)          # None: not lowerable (generic path)
        lowered = all(num < len(self.constraint_plans) and self.constraint_plans[num] is not None
                      for num in nums_constraints)
        only_known_terms = all(term == 'equation' or 'constraint' in term for term in loss_terms)
        fused = (self.use_fused and crit is not None and not self.ic_trainable and only_known_terms and lowered
                 and len(loss_terms) > 0 and (self.program is not None or 'equation' not in loss_terms))
        if causal is not None:
            fused = False                       # (the weights multiply the residual between the two halves of the generic step)
        rank, world = self._world()
        if world > 1:
            self.begin_data_parallel()
            # every rank must run the same step path (the validation of a lowering is a float comparison on random points and
            # may come out differently on one rank): fused only if fused everywhere
            flag = torch.tensor([1 if fused else 0], dtype=torch.int32, device=self.device)
            torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN)
            fused = bool(int(flag.item()))
        local_batch = batch_size // world + (1 if rank < batch_size % world else 0)
        self._global_batch = batch_size
        self._new_sample_seed()
        if hasattr(sampler, 'bind_solver'):         # (ResidualSampler: it asks this solver for the residual of its candidate pool)
            sampler.bind_solver(self)
        lay = model.net.layout
        history = torch.zeros(niters, dtype=torch.float32, device=self.device)
        done = [0]
        self._pending.append((history, done))       # registered up front: an interrupted fit keeps the losses it reached
        self.last_fit_path = 'fused' if fused else 'generic'
        self.last_fit_criterion = f'{type(criterion).__name__}/{self.last_fit_path}'
        self._apply_criterion(crit if fused else (engine.CRIT_MSE, 0.0, False), nums_constraints)
        flat_adam = isinstance(self.optimizer, FlatOptimizer)       # (any rule of the kernels; FlatAdam is the default one)
        self.last_fit_optimizer = f"{self.optimizer.name}/{'fused' if flat_adam else 'torch'}"
        # (an optimizer that steps through a closure -- L-BFGS -- re-evaluates the batch: no fit chunks, launch graphs or one-launch form)
        one_launch = (fused and world == 1 and flat_adam and tuple(loss_terms) == ('equation',) and not self.optimizer.needs_closure
                      and balance is None)            # (a fit with weights takes the per-iteration path, also for the equation alone)
        stream = engine.stream_of(model.flat)           # looked up once per call, not per iteration
        history_ptr = history.data_ptr()
        self.last_fit_balance, wb = None, None
        if balance is not None:
            terms = tuple(loss_terms)
            balance.bind(model.net, terms, self.grads.numel(), self.device)
            if flat_adam:
                mask = self.optimizer.mask
            else:                                       # (torch.optim steps the parameter views: the same entries -- trainable, reached -- are live)
                mask = model.trainable_mask()
                for off in unreached:
                    mask[off] = 0
            term_hist = torch.zeros((niters, len(terms)), dtype=torch.float32, device=self.device)
            weight_hist = torch.zeros((niters, len(terms)), dtype=torch.float32, device=self.device)
            self._term_pending.append((terms, term_hist, weight_hist, done))
            self._balance = balance
            self.last_fit_balance = f'{balance.kind}/{self.last_fit_path}'
            wb = dict(balance=balance, rows=self._term_rows(len(terms)), mask=mask, term_ptr=term_hist.data_ptr(), weight_ptr=weight_hist.data_ptr(),
                      nums=[None if term == 'equation' else int(term.replace('constraint', '').replace('_', '')) for term in terms],
                      keep=(term_hist, weight_hist))
        self.last_fit_causal = None
        if causal is not None:
            causal.bind(model.net, model, local_batch, self.device)
            hists = (torch.zeros((niters, causal.bins), dtype=torch.float32, device=self.device),
                     torch.zeros(niters, dtype=torch.float32, device=self.device), torch.zeros(niters, dtype=torch.float32, device=self.device))
            self._causal_pending.append((causal.bins, ) + hists + (done, ))
            self._causal = causal
            self.last_fit_causal = f'bins{causal.bins}/{self.last_fit_path}'
            self._causal_run = dict(causal=causal, it=0, ptrs=tuple(h.data_ptr() for h in hists), keep=hists, stream=stream)
        try:
            self._fit_loop(niters, local_batch, sampler, loss_terms, nums_constraints, criterion, world, fused, one_launch,
                           flat_adam, stream, history, history_ptr, done, wb)
        finally:
            self._global_batch = None
            self._causal_run = None

    def _fit_loop(self, niters, local_batch, sampler, loss_terms, nums_constraints, criterion, world, fused, one_launch,
                  flat_adam, stream, history, history_ptr, done, wb=None):
        lay = self.model.net.layout
        columns = self._device_columns(sampler) if one_launch else None
        if columns is not None and not self._needs_ic_streams():
            # the common case end to end on the device: chunks of iterations enqueued by ONE library call each
            # (pinn_fit_steps: sample, fused step, Adam per iteration; the interpreter is out of the per-iteration path)
            return self._fit_chunks(niters, local_batch, sampler, columns, stream, history, done)
        by_closure = self.optimizer.needs_closure
        for it in tqdm(range(niters), disable=None):
            xs = self._sample(local_batch, sampler, stream)
            if self._causal_run is not None:
                self._causal_run['it'] = it         # (the row of the causal histories this iteration writes)
            rate = self._rate_begin()               # (a schedule: this iteration's learning rate, by value through the calls below)
            if by_closure:
                # the batch is drawn ONCE; every closure call re-runs the gradient part of the iteration on it, and the iteration's loss is
                # what `step(closure)` returns: the loss at its first evaluation (`loss = opt.step(closure)`)
                recorded = []

                def closure(xs=xs, it=it, recorded=recorded):
                    if wb is not None:
                        # (constant weights: the same rows + combine in every evaluation; the histories take the first one's, as `losses` does)
                        self._weighted_step(xs, loss_terms, criterion, world, fused, wb, it=None if recorded else it, stream=stream)
                        recorded.append(it)
                        return
                    if fused:
                        self._fused_terms_step(xs, loss_terms, nums_constraints, world, stream=stream)
                    else:
                        self._generic_step(xs, loss_terms, nums_constraints, criterion, world)      # (eager: no launch graph across closure calls)
                    if world > 1:
                        self._all_reduce(stream)
                loss = self.optimizer.step(self.grads, stream=stream, closure=closure)
                history[it:it + 1].copy_(loss.reshape(1))
                done[0] = it + 1
                self._rate_end(rate)
                continue
            if one_launch:
                # Adam rides in the gradient-reduction launch, which also drops the loss into history[it]
                self._fused_step(xs, 1, adam=self.optimizer, loss_out=history_ptr + 4 * it, stream=stream)
                done[0] = it + 1
                self._rate_end(rate)
                continue
            if wb is not None:
                self._weighted_step(xs, loss_terms, criterion, world, fused, wb, it=it, stream=stream)
            elif fused:
                # (two to four launches per iteration: replaying them as a launch graph measured 0.048 -> 0.046 ms/it at batch 500 and
                #  0.072 -> 0.081 at 65 536 -- the eager loop stays)
                self._fused_terms_step(xs, loss_terms, nums_constraints, world, stream=stream)
            else:
                self._generic_step_auto(xs, loss_terms, nums_constraints, criterion, world, remaining=niters - it)
            if world > 1 and wb is None:
                self._all_reduce(stream)                # flat [p_total]: network, log_scale, loss slot, V slots
            if flat_adam:
                self.optimizer.step(self.grads, loss_out=history_ptr + 4 * it, stream=stream)
            else:
                self.optimizer.step(self.grads)
                history[it:it + 1].copy_(self.grads[lay.off_loss:lay.off_loss + 1])
            done[0] = it + 1
            self._rate_end(rate)

    FIT_CHUNK = 128             # iterations per pinn_fit_steps call (progress bar / KeyboardInterrupt granularity)
    FIT_CTRL_ON_HOST = False    # (tests on the CPU emulator: the control block of pinn_fit_steps in host memory)
    GRAPH_MAX_BATCH = 4096      # batches up to this size replay their chunks as one launch graph (+16 % at batch 100, +1 % at 4 096)

    def _device_columns(self, sampler):
        """ (kind, a, b) per input column if the Philox kernel can draw this sampler's batches, else None """
        total = self.model.total
        columns = [(engine.SAMPLE_UNIFORM, 0.0, 1.0)] * total if sampler is None else \
            (sampler.columns() if hasattr(sampler, 'columns') else None)
        if columns is not None and len(columns) == total and total <= engine.MAX_INPUTS:
            return columns
        return None

    def _needs_ic_streams(self):
        model = self.model
        lowered_ic = self.residual_plan is not None and self.residual_plan.ic_row is not None
        return (model.initial_condition is not None and model.ic_constant is None and self.ic_var_slot is None
                and not lowered_ic)

    def _fit_chunks(self, niters, batch, sampler, columns, stream, history, done):
        model, spec, adam = self.model, self.spec, self.optimizer
        comb_w = self.residual_plan.comb_w if self.residual_plan is not None else None
        n2 = spec.n2p if comb_w is None else 1
        ws = model.workspace(batch, spec.nd, spec.n2p)
        # (the batch buffer is kept per shape: its address is part of what a recorded chunk carries)
        xs = self.__dict__.setdefault('_fit_xs', {}).get((batch, model.total))
        if xs is None or xs.device != model.flat.device:
            xs = self._fit_xs[(batch, model.total)] = torch.empty((batch, model.total), dtype=torch.float32, device=self.device)
        own = sampler.device_key() if (sampler is not None and hasattr(sampler, 'device_key')) else None
        rank, _ = self._world()
        # small batches (the latency regime): each chunk as ONE replayable launch graph; the control block the kernels read their
        # per-iteration values from belongs to the solver (include/pinn.h pinn_fit_steps, ctrl)
        ctrl = None
        if batch <= self.GRAPH_MAX_BATCH and (xs.is_cuda or self.FIT_CTRL_ON_HOST) and os.environ.get('PYDENS_AMD_FIT_GRAPH', '1') != '0':
            if getattr(self, '_fit_ctrl', None) is None or self._fit_ctrl.device != xs.device:
                self._fit_ctrl = torch.zeros(int(model.net.lib.pinn_fit_ctrl_bytes()) + 64, dtype=torch.uint8, device=xs.device)
            ctrl = self._fit_ctrl
        with tqdm(total=niters, disable=None) as bar:
            it = 0
            while it < niters:
                k = min(self.FIT_CHUNK, niters - it)
                if own is not None:         # `NumpySampler(..., seed=k)`: the sampler's own key and batch counter (see _sample)
                    seed = (own + 7919 * rank) & (2 ** 64 - 1)
                    call0 = sampler.next_device_call(0)
                else:
                    seed, call0 = self._sample_seed, self._sample_calls
                t0, applied = adam.t, k
                # (a schedule: the chunk's rates, drawn ahead; how many of them leave the queue is decided by `applied` below)
                rates = self._draw_rates(k) if self.lr_scheduler is not None else None
                try:
                    model.net.fit_steps(self.program, model.flat, xs, columns, seed, call0, self.grads, ws, adam.exp_avg,
                                        adam.exp_avg_sq, adam.mask, adam.step_count, adam.t + 1, adam.optim,
                                        history[it:it + k], k, dir_cols=spec.dir_cols, n2=n2, ic_const=model.kernel_ic_const(),
                                        stream=stream, ctrl=ctrl, lr_steps=rates)
                    if os.environ.get('PYDENS_AMD_FIT_PERSIST') == '1' and model.net.lib.pinn_fit_chunk_status() != 0:
                        # the opt-in GRID form of the one-launch chunk gave up at its device-wide wait: nothing of the chunk was applied
                        # (include/pinn.h pinn_fit_chunk_status; the check synchronises with the device once per chunk)
                        raise RuntimeError('libpinn: ' + model.net.lib.pinn_last_error().decode())
                except BaseException:
                    # the library stopped inside the chunk (or an interrupt landed around the call): the device knows how many
                    # Adam steps it applied -- the host's step number and the batch counters follow IT, so that a later
                    # fit(optimizer=None) continues the bias correction and the point stream where the device left off
                    applied = max(0, min(k, int(adam.step_count.item()) - t0))
                    raise
                finally:
                    adam.t = t0 + applied
                    if rates is None:
                        self.lrs.extend([float(adam.lr)] * applied)
                    else:
                        self.lrs.extend(rates[:applied])
                        del self._lr_queue[:applied]
                    if own is not None:
                        sampler.next_device_call(applied)
                    else:
                        self._sample_calls += applied
                it += k
                done[0] = it
                bar.update(k)

    def _fused_step(self, xs, world, adam=None, loss_out=None, stream=None):
        model, spec = self.model, self.spec
        comb_w = self.residual_plan.comb_w if self.residual_plan is not None else None
        n2 = spec.n2p if comb_w is None else 1              # combined second-order stream: [u, firsts, sum_k c_k u_kk]
        ic_streams = None
        lowered_ic = self.residual_plan is not None and self.residual_plan.ic_row is not None
        if model.initial_condition is not None and model.ic_constant is None and self.ic_var_slot is None and not lowered_ic:
            ic_streams = self._ic_stream_tensor(xs, comb_w)
        ws = model.workspace(xs.shape[0], spec.nd, spec.n2p)
        if adam is not None:
            adam.t += 1
            model.net.residual_optim_step(self.program, model.flat, xs, self.grads, ws, adam.exp_avg, adam.exp_avg_sq,
                                          adam.mask, adam.step_count, adam.t, adam.optim, dir_cols=spec.dir_cols, n2=n2,
                                          ic_streams=ic_streams, ic_const=model.kernel_ic_const(), loss_out=loss_out, stream=stream)
            return
        # data parallel: this rank's share of a GLOBAL batch (shares may differ by one point: the true global count divides)
        n_global = self._global_batch if (world > 1 and getattr(self, '_global_batch', None)) else xs.shape[0] * world
        model.net.residual_step(self.program, model.flat, xs, self.grads, ws, spec.dir_cols, n2,
                                ic_streams=ic_streams, ic_const=model.kernel_ic_const(),
                                inv_n_global=1.0 if self._crit_sum else 1.0 / n_global, stream=stream)

    GENERIC_GRAPH_WARMUP = 3    # eager steps in front of the recording (instantiations, workspaces, autograd buffers settle)
    GENERIC_GRAPH_MIN_REPLAYS = 48      # a recording (device synchronise, gc, allocator trim inside torch.cuda.graph) is only made when at
                                        # least this many iterations of the fit call are left to replay it (short fits in a loop)
    GENERIC_GRAPH_CHECK_EVERY = 64      # every this many replays the step is ALSO run eagerly on the same batch and compared
    GENERIC_GRAPH_EARLY_CHECKS = (2, 8, 32)     # ... and soon after the recording, backing off (a recording that froze something is
                                                # noticed within a couple of iterations instead of 64; the steady state pays one check per 64)
    GENERIC_GRAPH_CHECK_RTOL = 1e-5     # relative L2 difference of the gradient buffers that still counts as "the same step" (torch code of
                                        # the user's that sums with atomics -- index_add / scatter backward -- differs in the last bits from run
                                        # to run; the library's own kernels are bit-repeatable)

    def _graph_step(self, xs, key, run, enabled=True, remaining=None):
        """ `run(points)` -- the gradient part of one iteration, everything between drawing the batch and the optimizer step -- replayed
        as ONE launch graph: recorded after a few eager iterations on a static copy of the batch (torch.cuda.graph; the library's
        launches go to the current stream, i.e. into the recording) and replayed with the next batch copied in. Same kernels, same
        order: bit-identical. A step whose torch code cannot be captured (data-dependent shapes, host reads) stays eager for good.

        What a recording FREEZES: the user's equation / constraint Python runs while the graph is recorded and not again -- host-side
        state it reads (closure scalars, numpy RNG used for arithmetic) keeps the value it had then, until the next fit call (graphs
        are per fit call). The reference re-evaluates that Python every iteration. Guard: 2, 8 and 32 replays after the recording and
        every GENERIC_GRAPH_CHECK_EVERY replays from then on the same batch is also stepped eagerly and the gradient buffers are compared
        (equal, or within GENERIC_GRAPH_CHECK_RTOL in relative L2: the library's kernels are bit-repeatable, the user's torch code need
        not be); on a mismatch the eager result is kept and the fit goes on eagerly. Up to GENERIC_GRAPH_CHECK_EVERY - 1 iterations can
        therefore run on frozen host-side state before it is noticed.
        `PYDENS_AMD_STEP_GRAPH=0` turns recording off altogether. """
        st = getattr(self, '_generic_graph', None)
        if not (enabled and xs.is_cuda and os.environ.get('PYDENS_AMD_STEP_GRAPH', os.environ.get('PYDENS_AMD_GENERIC_GRAPH', '1')) != '0'
                and not (st and st.get('failed') and st['key'] == key)):
            return run(xs)
        if st is None or st['key'] != key:
            st = self._generic_graph = dict(key=key, count=0, graph=None, xs=None, failed=False, replays=0)
        if st['graph'] is None:
            if st['count'] < self.GENERIC_GRAPH_WARMUP:
                st['count'] += 1
                before = tokens.AUTOGRAD_FALLBACKS[0]
                out = run(xs)
                if tokens.AUTOGRAD_FALLBACKS[0] != before:
                    # D(...) on something that is not a kernel stream (a constraint that differentiates the model at its point, a
                    # function of the inputs): torch.autograd.grad(create_graph=True) inside the step -- never recorded (see
                    # _generic_step_auto)
                    st['failed'], st['error'] = True, 'the step differentiates inside its torch code (D by autograd): kept eager'
                return out
            if remaining is not None and remaining < self.GENERIC_GRAPH_MIN_REPLAYS:
                return run(xs)                  # (too few iterations left to pay for a recording)
            try:
                st['xs'] = xs.clone()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    run(st['xs'])
                st['graph'] = graph
            except Exception as exc:         # noqa: BLE001 -- whatever the step's torch code does that a capture refuses
                st['failed'], st['graph'], st['error'] = True, None, repr(exc)
                torch.cuda.synchronize()
                return run(xs)
        st['xs'].copy_(xs)
        st['graph'].replay()
        st['replays'] += 1
        if st['replays'] in self.GENERIC_GRAPH_EARLY_CHECKS or st['replays'] % self.GENERIC_GRAPH_CHECK_EVERY == 0:
            replayed = self.grads.clone()
            run(xs)
            if not torch.equal(replayed, self.grads):
                rel = float((replayed - self.grads).norm() / self.grads.norm().clamp_min(1e-30))
                if not rel <= self.GENERIC_GRAPH_CHECK_RTOL:            # (also: NaN)
                    import warnings
                    warnings.warn('pydens_amd: the replayed launch graph and the eager step differ on the same batch (relative L2 '
                                  f'{rel:.1e}): host-side state the equation / constraint code reads may have changed during fit, or its '
                                  'torch code is not reproducible from run to run; continuing without the launch graph', RuntimeWarning)
                    st['failed'], st['graph'], st['error'] = True, None, f'replay differs from the eager step (relative L2 {rel:.1e})'

    def _generic_step_auto(self, xs, loss_terms, nums_constraints, criterion, world, remaining=None):
        """ the generic step -- pinn_jet_forward -> the user's torch code and its autograd sweep (a few dozen small kernels the
        interpreter launches one by one) -> pinn_jet_backward, constraint terms (the model on fixed points) included -- as a launch
        graph in a single process (direction groups included). Kept eager: data-parallel steps (the all-reduce sits between the halves)
        and every step that differentiates INSIDE its torch code with create_graph -- a callable initial condition's derivative
        streams, an equation that takes torch gradients with respect to its inputs, a model subclass's own forward(): recording those
        ends in a crash inside hipStreamEndCapture on ROCm 7.2 (not an exception: tools/graph_crash_probe.py), so they are never tried. """
        model = self.model
        # (a causal fit: pinn_causal_weights takes this iteration's rows of the histories and its `update` by value -- kept eager)
        ok = (world == 1 and not self.custom_forward and not self.needs_x_grad and self._causal_run is None
              and not (model.initial_condition is not None and model.ic_constant is None))
        return self._graph_step(xs, ('generic', tuple(xs.shape), id(criterion), id(self._eq), tuple(loss_terms)),
                                lambda pts: self._generic_step(pts, loss_terms, nums_constraints, criterion, world), enabled=ok,
                                remaining=remaining)

    def _fused_terms_step(self, xs, loss_terms, nums_constraints, world, stream=None):
        """ summed loss (:441-457) on the fused kernels: the equation term stores gradient + loss, every constraint term adds its own """
        first = True
        if 'equation' in loss_terms:
            self._fused_step(xs, world, stream=stream)
            first = False
        for num in nums_constraints:
            self._constraint_step(num, world, accumulate=not first)
            first = False

    def _model_at(self, args, spec, calls, probe=None, discover=False):
        """ `f(*args)` of a constraint (reference :451-454) on the generic step. spec: the streams the constraint's `D` asks of this call,
        known from the dry run (`_discover_constraint`); None or value only: the value-only forward with its autograd seam, as ever.
        Otherwise the value comes back TAGGED like the equation's field: a StreamContext of this call's own over the call's points, the
        kernel streams as its tensors, the arguments remembered by identity -- `D(value, arg)` picks a stream (tokens.D). The call is
        appended to `calls` (kernel points, spec, the stream leaf, slot): after `loss.backward()` the streams' gradients go back through
        pinn_jet_backward. A model with its own forward() runs that forward as torch code around the tagged network value.
        discover: the dry run -- no kernel, random stand-ins, `calls` receives the stream contexts (what was asked of each). """
        model, total = self.model, self.model.total
        if not discover and (spec is None or spec.nd == 0):
            out = model(self._points_on_device(args))
            if probe is not None and out.requires_grad:
                out.register_hook(lambda g: probe.__setitem__('value', True))
            return out
        sc = trace.StreamContext(total).bind_args(args)
        sc.discovering = discover
        imap = None
        if self.custom_forward:
            pts = self.reshape_and_concat(args, device=self.device)         # (keeps the autograd link to the arguments: the ansatz is torch code)
            imap = self._input_map(pts, inside=True, known_scale=True)
            if imap is not None and imap[1] is None:
                raise NotImplementedError('a constraint that differentiates a model whose forward() puts a map in front of the network that '
                                          'is not per-column affine: not built (the equation term follows such a map)')
            kpts = pts.detach().contiguous() if imap is None else imap[0]
        else:
            kpts = pts = self._points_on_device([a.detach() if torch.is_tensor(a) else a for a in args])
        if discover:
            sc.tag(torch.rand((kpts.shape[0], 1), device=self.device).requires_grad_(), ())
            calls.append((sc, ))
        else:
            slot = len(calls) + 1
            rows = leaf = self._streams_forward(kpts, spec, slot).requires_grad_()
            if probe is not None:
                rows = [row.detach().requires_grad_() for row in leaf.detach().unbind(0)]
            ic_streams = None
            if model.initial_condition is not None and model.ic_constant is None and not self.custom_forward:
                ic_streams = self._ic_streams(kpts, create_graph=True, spec=spec)
            scale = None if imap is None or all(a == 1.0 for a in imap[1]) else imap[1]
            self._tag_streams(sc, spec, rows, ic_streams, scale)
            calls.append((kpts, spec, rows, slot))
        trace.active_streams.set(sc)            # (until the constraint returns: trace.call_constraint)
        if not self.custom_forward:
            return sc.tensors[()]
        model.raw_field = (pts, sc.tensors[()], None if imap is None else imap[0])
        try:
            return model.forward(pts)
        finally:
            model.raw_field = None

    def _discover_constraint(self, constraint):
        """ dry run of a constraint (as trace.discover is the equation's): one StreamSpec per model call, in call order -- which streams
        its `D` asks of the model at the constraint's own points. None: the dry run failed for a reason of its own, kept in
        `constraint_dry_run_errors` (the step then evaluates the model by value, as it always did, and says what is wrong); an exception
        object: an order or partial the kernels do not carry, raised by the fit call that uses the constraint.
        -> (specs, why the dry run failed or None) """
        calls = []
        lay = self.model.net.layout
        try:
            # (stand-in values on a fork of the generators: a later fit samples what it would have sampled without this dry run)
            with torch.random.fork_rng(devices=[self.device] if self.device.type == 'cuda' else []):
                cols = [torch.rand((3, 1), device=self.device).requires_grad_() for _ in range(self.model.total)]
                self.ctx.run(trace.call_constraint, constraint, lambda *args: self._model_at(args, None, calls, discover=True), *cols)
            specs = [trace.StreamSpec(sc.requested, hp=lay.hp, allact=self.model.net.allact) for sc, in calls]
            if self.custom_forward and len(specs) > 1 and any(spec.nd for spec in specs):
                raise NotImplementedError('a constraint that differentiates a model with its own forward() may call the model once: `D` of '
                                          'an expression of its value finds the streams of ONE call')
            return specs, None
        except NotImplementedError as err:
            return err, None
        except Exception as err:        # noqa: BLE001 -- whatever the user's code does with stand-in values
            return None, f'{type(err).__name__}: {err}'         # (kept per constraint in `constraint_dry_run_errors`)

    def _compile_constraint(self, num, constraint):
        """ lower constraint `num` where the fused step can serve it, and find the streams its model calls need on the generic step """
        plan, err = self._try_compile_constraint(constraint)
        specs, dry_run_error = self._discover_constraint(constraint)
        for values, value in ((self.constraint_plans, plan), (self.constraint_errors, err), (self.constraint_specs, specs),
                              (self.constraint_dry_run_errors, dry_run_error)):
            if num < len(values):
                values[num] = value
            else:
                values.append(value)

    def _generic_step(self, xs, loss_terms, nums_constraints, criterion, world, probe=None):
        """ probe: a dict -- the step is a DRY evaluation that is asked which parts of the graph the loss reaches (_unreached_scalars): every
        kernel stream is a leaf of its own, the backward stops at the streams, and `probe` receives 'streams' (per stream: did it get a
        gradient), 'variables' (names of the V(...) that did), 'log_scale', 'value' (a constraint term's model value did) """
        model, spec = self.model, self.spec
        lay = model.net.layout
        self.grads.zero_()
        model.grad_sink = self.grads
        for name in model.variables:
            getattr(model, name).grad = None
        model.log_scale.grad = None
        try:
            loss = 0
            leaf = None
            # data parallel: the all-reduce SUMS the ranks' buffers, so the equation term (a mean over this rank's share of
            # the global batch) is weighted by that share and the constraint terms, which every rank evaluates, by 1 / world
            n_global = self._global_batch if (world > 1 and getattr(self, '_global_batch', None)) else xs.shape[0] * world
            w_eq, w_con = xs.shape[0] / n_global, 1.0 / world
            kpts = xs                              # where the kernels evaluate the network: the batch, or what a custom forward() maps it to
            if 'equation' in loss_terms:
                if self.custom_forward:
                    self._imap = self._input_map(xs)
                    if self._imap is not None:
                        kpts = self._imap[0]
                leaf = self._streams_forward(kpts, spec).requires_grad_()
                if probe is not None:
                    leaf = [row.detach().requires_grad_() for row in leaf.detach().unbind(0)]
                ic_streams = None
                if model.initial_condition is not None and model.ic_constant is None and not self.custom_forward:
                    ic_streams = self._ic_streams(xs, create_graph=True)       # (custom forward(): the IC is torch code of the model)
                r = self._eval_equation(leaf, xs, ic_streams)
                run = self._causal_run if probe is None else None
                if run is not None:
                    # causal weights of this batch from its own residuals (three launches, include/pinn.h pinn_causal_weights), held
                    # constant under the gradient: the equation term is mean_i w_i r_i^2
                    it, ptrs = run['it'], run['ptrs']
                    w = run['causal'].point_weights(model.net, xs, r.detach().reshape(-1).float().contiguous(),
                                                    bin_weight_out=ptrs[0] + 4 * run['causal'].bins * it, eps_out=ptrs[1] + 4 * it,
                                                    mean_sq_out=ptrs[2] + 4 * it, stream=run['stream'])
                    term = (w.view_as(r) * r * r).mean()
                else:
                    term = criterion(r, torch.zeros_like(xs[:, :1]))                        # :448
                loss = loss + (term if world == 1 else term * w_eq)

            calls = []          # model calls of the constraint terms that carry derivative streams (_model_at)
            cols = [xs[:, c:c + 1] for c in range(model.total)]
            for num in nums_constraints:                                                  # :456-457
                specs = self.constraint_specs[num] if num < len(self.constraint_specs) else None
                if isinstance(specs, Exception):
                    raise specs                 # (what the dry run of this constraint met: an order or partial the kernels do not carry)
                todo = list(specs) if specs is not None else None
                differentiates = specs is not None and any(spec_c.nd for spec_c in specs)
                cols_c = cols
                if differentiates:
                    # (leaves of the constraint's own: `D(x * f(x, t), x)` has an explicit partial derivative with respect to the batch
                    #  column, and the ansatz of a custom forward() is torch code of the points. `D` finds them by identity all the same.)
                    cols_c = [col.clone().requires_grad_() for col in cols]

                def _forward(*pts):                                                      # :451-454
                    if differentiates and not todo:
                        raise NotImplementedError(f'constraint {num} calls the model more often in the step than in its dry run on stand-in '
                                                  f'values ({len(specs)} calls): which derivative streams the further calls need is not known')
                    spec_c = todo.pop(0) if todo else None
                    return self._model_at(pts, spec_c, calls, probe)
                value = self.ctx.run(trace.call_constraint, self.constraints[num], _forward, *cols_c)
                term = criterion(value, torch.zeros(1, device=self.device))
                loss = loss + (term if world == 1 else term * w_con)
            loss.backward()
            if probe is not None:
                probe['streams'] = [] if leaf is None else [row.grad is not None for row in leaf]
                probe['variables'] = {name for name in model.variables if getattr(model, name).grad is not None}
                probe['log_scale'] = model.log_scale.grad is not None
                for _, spec_c, rows, _ in calls:
                    if self._streams_reach_value([row.grad is not None for row in rows], spec_c):
                        probe['value'] = True
            else:
                if leaf is not None and leaf.grad is not None:
                    self._streams_backward(kpts, spec, leaf.grad)
                for kpts_c, spec_c, rows, slot in calls:
                    if rows.grad is not None:
                        self._streams_backward(kpts_c, spec_c, rows.grad, slot)
            for name, (off, n) in model.variables.items():
                p = getattr(model, name)
                if p.grad is not None:
                    self.grads[off:off + n] += p.grad.reshape(-1)
                    p.grad = None
            if self.custom_forward and model.log_scale.grad is not None:
                # (the ansatz of a custom forward() is torch code: its log_scale gradient comes from autograd, not from the kernels)
                self.grads[lay.off_log_scale] += model.log_scale.grad.reshape(())
                model.log_scale.grad = None
            self.grads[lay.off_loss] = loss.detach()
        finally:
            model.grad_sink = None
            self._imap = UNSET

    RESIDUAL_SLICE = 1 << 20    # points per forward pass of `residual`: bounds the stream buffers ([streams, N] floats) of a large pool

    def residual(self, *xs):
        """ the value of the equation callable at the given points with the current parameters -> ndarray [N, 1]; arguments as for
        `predict`. Forward only: the jet kernels hand the derivative streams to the equation (the forward half of the generic step, so
        every equation `fit` accepts is served, lowered to a residual program or not). Nothing is written to `grads`, no `.grad` is
        touched, the launch graphs of a fit stay as they are, the model's train / eval mode is restored. """
        with self._device_guard():
            pts = self.reshape_and_concat(xs, device=self.device).contiguous()
            # the traces as `fit` builds them (a re-assigned equation, a changed closure constant); the validation draws random points:
            # on a fork of the generators, so that a later fit samples what it would have sampled without this call
            devices = [self.device] if self.device.type == 'cuda' else []
            with torch.random.fork_rng(devices=devices):
                self._refresh_traces(set())
            return self._residual_device(pts).view(-1, 1).cpu().numpy()

    def _residual_device(self, pts):
        """ `residual` on a device tensor [N, total] -> device tensor [N]; no host copy, no synchronisation (ResidualSampler) """
        model = self.model
        was_training = model.training
        model.eval()
        try:
            n = pts.shape[0]
            if n == 1 and model.initial_condition is not None and model.ic_constant is None:
                # (`_ic_streams` takes a callable IC that returns ONE value for a constant and skips its derivative streams: a lone
                #  point is evaluated as two copies of itself)
                return self._residual_slice(pts.repeat(2, 1))[:1]
            if n <= self.RESIDUAL_SLICE:
                return self._residual_slice(pts)
            out = torch.empty(n, dtype=torch.float32, device=self.device)
            for lo in range(0, n, self.RESIDUAL_SLICE):
                out[lo:lo + self.RESIDUAL_SLICE] = self._residual_slice(pts[lo:lo + self.RESIDUAL_SLICE])
            return out
        finally:
            model.train(was_training)

    def _residual_slice(self, xs):
        """ the forward half of `_generic_step` on one slice of points: jet_forward per direction group, IC streams, the input map of a
        custom forward(), the equation. Equations that differentiate inside their torch code run with grad enabled and are detached.
        Nested-skip nets need forward scratch: a buffer of this method's own (engine.Net.jet_forward `ws_slot`), never the step's, whose
        address a recorded launch graph of the generic step carries. """
        model, spec = self.model, self.spec
        with_grad = bool(self.needs_x_grad)
        kpts = xs
        try:
            if self.custom_forward:
                self._imap = self._input_map(xs)
                if self._imap is not None:
                    kpts = self._imap[0]
            with torch.no_grad():
                if len(spec.groups) == 1:
                    leaf = model.net.jet_forward(model.flat, kpts, spec.dir_cols, spec.n2p, ic_const=model.kernel_ic_const(), ws_slot='_residual_fwd_ws')
                else:
                    leaf = torch.empty((spec.n_streams, xs.shape[0]), dtype=torch.float32, device=self.device)
                    for num, (dirs_g, n2g, idx) in enumerate(spec.groups):
                        part = model.net.jet_forward(model.flat, kpts, dirs_g, n2g, ic_const=model.kernel_ic_const(), ws_slot='_residual_fwd_ws')
                        leaf.index_copy_(0, self._group_rows(num, idx), part)
            ic_streams = None
            if model.initial_condition is not None and model.ic_constant is None and not self.custom_forward:
                with torch.enable_grad():           # (the IC's derivative streams are torch autograd over the callable)
                    ic_streams = self._ic_streams(xs, create_graph=with_grad)
            with (torch.enable_grad() if with_grad else torch.no_grad()):
                if with_grad:
                    leaf.requires_grad_()
                r = self._eval_equation(leaf, xs, ic_streams, requires_grad=with_grad)
            return r.detach().reshape(-1).float()
        finally:
            self._imap = UNSET

    def predict(self, *xs):
        """ reference model_torch.py:466-487 -> ndarray [N,1]. """
        with self._device_guard():
            return self._predict(*xs)

    def _predict(self, *xs):
        model = self.model
        pts = self.reshape_and_concat(xs, device=self.device).contiguous()
        model.eval()
        with torch.no_grad():
            if self.custom_forward:
                u = self.ctx.run(model.forward, pts).view(-1, 1)          # bare network on the kernels, the rest is the model's torch code
            else:
                u = model.net.jet_forward(model.flat, pts, ic_const=model.kernel_ic_const()).view(-1, 1)
                if model.initial_condition is not None and model.ic_constant is None:
                    u = u + self.ctx.run(model.ic_values, pts).expand_as(u)
        return u.detach().cpu().numpy()
