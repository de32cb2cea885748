""" Loss-term weights of `Solver.fit(loss_weights=...)`: constant, or balanced by the gradient statistics of the terms on the device
(include/pinn.h pinn_balance_terms; pydens_amd/csrc/pinn_balance_kernels.h). Nothing is read back per iteration. """
import math

import numpy as np
import torch

from . import engine


class LossBalancer:
    """ weights of the loss terms of a fit, adapted from the terms' gradients every `period` iterations:
      kind='max_mean'  the learning-rate annealing of Wang, Teng and Perdikaris (2021): the `reference` term has hat = 1, every other term
                       hat_i = max|grad L_ref| / mean|grad L_i|
      kind='norm'      its L2-norm form: hat_i = sum_j |grad L_j|_2 / |grad L_i|_2 for every term
    and w_i <- momentum * w_i + (1 - momentum) * hat_i, clipped to `clip` (`momentum` is the weight of the OLD value). A term whose
    statistic is zero or not finite keeps its weight for that iteration. `initial`: the weights before the first update -- a number for
    all terms, or a dict by term name. The object owns the device state: handed to a later `fit(optimizer=None, loss_weights=balancer)` it
    carries the weights (and the period's count) on; a new object starts from `initial`. """
    KINDS = {'max_mean': engine.BALANCE_MAX_MEAN, 'norm': engine.BALANCE_NORM}

    def __init__(self, kind='max_mean', momentum=0.9, period=1, reference='equation', initial=1.0, clip=(0.0, 1e6)):
        if kind not in self.KINDS and kind != 'fixed':
            raise ValueError(f"LossBalancer(kind={kind!r}): one of {sorted(self.KINDS)}")
        if not (isinstance(momentum, (int, float)) and 0.0 <= momentum <= 1.0):
            raise ValueError(f'LossBalancer(momentum={momentum!r}): a number in [0, 1] (the weight of the old value)')
        if not (isinstance(period, int) and not isinstance(period, bool) and period >= 1):
            raise ValueError(f'LossBalancer(period={period!r}): an integer >= 1')
        lo, hi = (float(v) for v in clip)
        if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 <= lo <= hi):
            raise ValueError(f'LossBalancer(clip={clip!r}): finite bounds with 0 <= lo <= hi')
        self.kind, self.momentum, self.period, self.reference, self.initial, self.clip = kind, float(momentum), period, reference, initial, (lo, hi)
        self.terms = None           # the loss terms the state was built for, in the order of the rows
        self.state = None           # float64 device tensor (engine.BALANCE_STATE)
        self.workspace = None
        self.calls = 0              # iterations served so far: the weights are updated where calls % period == 0

    @property
    def adaptive(self):
        return self.kind != 'fixed'

    @classmethod
    def fixed(cls, weights):
        """ constant weights (a dict by term name): PINN_BALANCE_FIXED through the same three launches """
        return cls(kind='fixed', momentum=1.0, initial=dict(weights))

    def initial_weights(self, terms):
        """ one checked weight per term, from `initial` """
        initial = self.initial
        if isinstance(initial, dict):
            extra, missing = [t for t in initial if t not in terms], [t for t in terms if t not in initial]
            if extra:
                raise ValueError(f'loss_weights: a weight for {extra}, which is not among loss_terms={list(terms)}')
            if missing:
                raise ValueError(f'loss_weights: no weight for {missing} of loss_terms={list(terms)}')
            values = [initial[t] for t in terms]
        else:
            values = [initial] * len(terms)
        for term, w in zip(terms, values):
            if isinstance(w, bool) or not isinstance(w, (int, float, np.integer, np.floating)) or not math.isfinite(w) or w < 0:
                raise ValueError(f'loss_weights: the weight {w!r} of {term!r} must be a finite number >= 0')
        return [float(w) for w in values]

    def refusal(self, terms, by_closure):
        """ why these terms cannot be served, as an exception (None: they can) """
        if len(terms) > engine.BALANCE_MAX_TERMS:
            return NotImplementedError(f'loss_weights: {len(terms)} loss terms; the kernels combine at most {engine.BALANCE_MAX_TERMS}')
        if len(set(terms)) != len(terms):
            return ValueError(f'loss_weights: loss_terms={list(terms)} names a term twice; which weight belongs to which is not defined')
        if self.adaptive:
            if len(terms) < 2:
                return ValueError(f"loss_weights: LossBalancer('{self.kind}') balances terms against each other; loss_terms={list(terms)} is a single term")
            if self.reference not in terms:
                return ValueError(f'loss_weights: reference={self.reference!r} is not among loss_terms={list(terms)}')
            if by_closure:
                return NotImplementedError("loss_weights: an adaptive LossBalancer with an optimizer that steps through a closure (L-BFGS) -- it "
                                           're-evaluates the batch inside one step, and the weights must not move under its line search; '
                                           'constant weights are served there')
        if self.terms is not None and tuple(terms) != self.terms:
            return ValueError(f'loss_weights: this LossBalancer holds the weights of loss_terms={list(self.terms)}; it cannot go on with {list(terms)}')
        try:
            self.initial_weights(terms)
        except ValueError as err:
            return err
        return None

    def bind(self, net, terms, n, device):
        """ the device state for these terms: built from `initial` on first use, carried on afterwards """
        if self.state is None or self.state.device != torch.device(device):
            if self.state is not None:
                raise ValueError(f'loss_weights: this LossBalancer lives on {self.state.device}, the solver on {device}')
            self.state = net.balance_state(len(terms), self.initial_weights(terms), device)
            self.terms = tuple(terms)
        need = int(net.lib.pinn_balance_workspace_bytes(int(n), len(terms))) // 8
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = net.balance_workspace(n, len(terms), device)

    def combine(self, net, rows, n, mask, out, term_loss_out=None, weight_out=None, count=True, stream=None):
        """ one iteration: weights updated if this is an iteration of the period, out <- sum_j w_j rows[j] """
        update = self.adaptive and self.calls % self.period == 0
        ref = self.terms.index(self.reference) if self.adaptive else 0
        net.balance_terms(rows, n, mask, self.KINDS.get(self.kind, engine.BALANCE_FIXED), ref, update, self.momentum, self.clip[0],
                          self.clip[1], self.state, out, self.workspace, term_loss_out=term_loss_out, weight_out=weight_out, stream=stream)
        if count:
            self.calls += 1

    def read(self, field):
        first, count = engine.BALANCE_STATE[field]
        values = self.state[first:first + count].cpu().numpy()
        return values[:len(self.terms)] if count > 1 else values[0]

    @property
    def weights(self):
        """ {term: weight} as it stands on the device (read back when asked) """
        if self.state is None:
            return None
        return {term: float(w) for term, w in zip(self.terms, self.read('weights'))}
