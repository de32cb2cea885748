""" Causal training weights of `Solver.fit(causal=...)`: the equation residual of a time slice is held down until the slices before it are
resolved (Wang, Sankaran, Perdikaris 2022), over time bins of the batch, on the device (include/pinn.h pinn_causal_weights;
pydens_amd/csrc/pinn_causal_kernels.h). Nothing is read back per iteration. """
import math

import numpy as np
import torch

from . import engine


class CausalWeights:
    """ the batch is cut into `bins` equal time bins over the model's domain of the time column; with L_k the mean squared residual of bin
    k, the points of bin k are weighted by w_k = exp(-eps * sum_{j<k} L_j), held constant under the gradient, and the equation term of
    the loss is mean_i w_i r_i^2 = sum_k (n_k / N) w_k L_k -- the paper's 1/M sum_k w_k L_k where the bins are equally filled.
      eps     a tolerance, or the ladder of the paper's annealing (at most 8): once min_k w_k > delta the next tolerance takes over with
              the next iteration; at the last one `converged` is set. The decision is taken on the device.
      time    index of the time column (default: the last of the model's `ndims` columns, the one the ansatz treats as time)
      period  the ladder decision runs every `period`-th iteration only
    The object owns the device state: handed to a later `fit(optimizer=None, causal=obj)` it carries the ladder on; a new object starts at
    the first tolerance. """

    def __init__(self, bins=32, eps=(1e-2, 1e-1, 1.0, 1e1, 1e2), delta=0.99, time=None, period=1):
        if not (isinstance(bins, (int, np.integer)) and not isinstance(bins, bool) and 1 <= bins <= engine.CAUSAL_MAX_BINS):
            raise ValueError(f'CausalWeights(bins={bins!r}): an integer in [1, {engine.CAUSAL_MAX_BINS}]')
        ladder = [eps] if isinstance(eps, (int, float, np.integer, np.floating)) and not isinstance(eps, bool) else list(eps)
        if not 1 <= len(ladder) <= engine.CAUSAL_MAX_EPS:
            raise ValueError(f'CausalWeights(eps=...): a ladder of {len(ladder)} tolerances; 1 to {engine.CAUSAL_MAX_EPS}')
        for e in ladder:
            if isinstance(e, bool) or not isinstance(e, (int, float, np.integer, np.floating)) or not math.isfinite(e) or e < 0:
                raise ValueError(f'CausalWeights(eps=...): the tolerance {e!r} must be a finite number >= 0')
        if isinstance(delta, bool) or not isinstance(delta, (int, float, np.integer, np.floating)) or math.isnan(delta):
            raise ValueError(f'CausalWeights(delta={delta!r}): a number')
        if not (isinstance(period, int) and not isinstance(period, bool) and period >= 1):
            raise ValueError(f'CausalWeights(period={period!r}): an integer >= 1')
        if time is not None and not (isinstance(time, (int, np.integer)) and not isinstance(time, bool) and time >= 0):
            raise ValueError(f'CausalWeights(time={time!r}): the index of the time column')
        self.bins, self.ladder, self.delta, self.time, self.period = int(bins), [float(e) for e in ladder], float(delta), time, period
        self.state = None           # float64 device tensor (engine.CAUSAL_STATE)
        self.workspace = None
        self.weights = None         # [n] float32: the point weights of the running batch
        self.column = None          # the time column and its domain, as bound to a solver
        self.t_lo = self.t_hi = None
        self.calls = 0              # iterations served so far: the ladder decision runs where calls % period == 0

    def resolve(self, model):
        """ (time column, t_lo, t_hi) for this model; raises the refusal, before anything of this object has changed """
        time = self.time
        if time is None:
            if model.ndims < 2:
                raise ValueError(f'causal: a problem with ndims={model.ndims} has no time column beside a space column; name it with '
                                 'CausalWeights(time=...) if the single column is the time')
            time = model.ndims - 1
        if time >= model.ndims:
            raise ValueError(f'causal: time={time} is not one of the {model.ndims} columns of the domain')
        lo, hi = (float(v) for v in model.domain[time])
        if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
            raise ValueError(f'causal: the domain {model.domain[time]} of the time column {time} is not an interval t_lo < t_hi')
        if self.column is not None and (self.column, self.t_lo, self.t_hi) != (int(time), lo, hi):
            raise ValueError(f'causal: this CausalWeights is bound to the time column {self.column} over [{self.t_lo}, {self.t_hi}]; it cannot '
                             f'go on with column {time} over [{lo}, {hi}]')
        return int(time), lo, hi

    def bind(self, net, model, n, device):
        """ the device state: built from the ladder on first use, carried on afterwards; buffers for batches of n points """
        if self.state is not None and self.state.device != torch.device(device):
            raise ValueError(f'causal: this CausalWeights lives on {self.state.device}, the solver on {device}')
        self.column, self.t_lo, self.t_hi = self.resolve(model)
        if self.state is None:
            self.state = net.causal_state(self.ladder, self.delta, device)
        need = int(net.lib.pinn_causal_workspace_bytes(int(n), self.bins)) // 8
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = net.causal_workspace(n, self.bins, device)
        if self.weights is None or self.weights.numel() < n:
            self.weights = torch.empty(int(n), dtype=torch.float32, device=device)

    def point_weights(self, net, xs, r, bin_weight_out=None, eps_out=None, mean_sq_out=None, stream=None):
        """ one iteration: the weights of the batch `xs` from its residuals `r` (detached), the ladder decision if this is an iteration of
        the period -> [n] float32 (a view of this object's buffer) """
        n = xs.shape[0]
        net.causal_weights(xs, self.column, r, self.bins, self.t_lo, self.t_hi, self.calls % self.period == 0, self.state, self.weights,
                           self.workspace, bin_weight_out=bin_weight_out, eps_out=eps_out, mean_sq_out=mean_sq_out, stream=stream)
        self.calls += 1
        return self.weights[:n]

    def read(self, field):
        """ a field of the state block as it stands on the device (engine.CAUSAL_STATE), read back when asked """
        if self.state is None:
            return None
        first, count = engine.CAUSAL_STATE[field]
        values = self.state[first:first + count].cpu().numpy()
        if field == 'ladder':
            return values[:len(self.ladder)]
        return values[:self.bins] if count > 1 else values[0]

    @property
    def eps(self):
        """ the tolerance the next iteration uses """
        return self.ladder[0] if self.state is None else float(self.read('ladder')[int(self.read('index'))])

    @property
    def converged(self):
        """ min_k w_k > delta was reached at the last tolerance of the ladder """
        return False if self.state is None else bool(self.read('converged') != 0)

    @property
    def non_finite(self):
        """ an iteration so far met a NaN or infinite residual (it entered its bin's sum as 0) """
        return False if self.state is None else bool(self.read('non_finite') != 0)
