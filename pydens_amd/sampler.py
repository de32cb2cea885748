""" Point samplers with the `batchflow.sampler` surface pydens re-exports (reference pydens/__init__.py:5):
`NumpySampler(name, **kwargs)`, `a & b` = column concatenation, `.sample(size) -> ndarray [size, dim]`
(call site reference model_torch.py:433; README.md:82 `NumpySampler('uniform') & NumpySampler('uniform', low=1, high=5)`).

`batchflow` itself is third-party and not vendored by the reference; only the numpy-distribution samplers and
`&` are restated. On top of the numpy surface every sampler offers `sample_device(size, device)`, which draws the
batch directly in HBM (uniform / normal), so that `Solver.fit` keeps the host out of the step path, and `columns()`:
the per-column description (kind, a, b) of include/pinn.h `pinn_sample_points` when the sampler is a product of
independent uniform / normal / constant columns -- `Solver.fit` then draws the whole batch with ONE launch of the
Philox kernel instead of a handful of torch ops per iteration.
"""
import numbers
import operator

import numpy as np
import torch

__all__ = ['Sampler', 'NumpySampler', 'ConstantSampler', 'NS', 'ResidualSampler']

_ALIASES = {'u': 'uniform', 'n': 'normal', 'e': 'exponential', 'g': 'gamma'}


class Sampler:
    dim = 1

    def sample(self, size):
        raise NotImplementedError

    def sample_device(self, size, device, generator=None):
        """ default: numpy draw + one host-to-device copy. """
        return torch.from_numpy(np.asarray(self.sample(size), dtype=np.float32)).to(device)

    def columns(self):
        """ [(kind, a, b)] per column for the device sampler kernel (0 uniform on [a, b), 1 normal a + b z, 2 constant a),
        or None when the sampler is not such a product (then `sample_device` / `sample` are used). """
        return None

    def seeds(self):
        """ seeds of the random leaves of this sampler, None for an unseeded leaf (constants contribute nothing) """
        return []

    def device_key(self):
        """ Philox key for the device sampler when EVERY random leaf was given a seed (`NumpySampler(..., seed=k)`: the
        reference then draws a sequence that depends on those seeds alone, model_torch.py:433), else None: the solver
        keys the stream by torch's generator instead. """
        seeds = self.seeds()
        if not seeds or any(s is None for s in seeds):
            return None
        key = 0x9E3779B97F4A7C15
        try:
            for s in seeds:                       # splitmix64-style fold
                key = (key ^ (int(s) & (2 ** 64 - 1))) * 0xBF58476D1CE4E5B9 & (2 ** 64 - 1)
                key ^= key >> 31
        except (TypeError, ValueError):           # array-like seeds (numpy accepts them): no single integer to key a stream with
            return None
        return key

    def next_device_call(self, count=1):
        """ batches this sampler object has drawn on the device so far (its own call counter, like its own numpy state);
        reserves `count` consecutive batch numbers and returns the first """
        n = getattr(self, '_device_calls', 0)
        self._device_calls = n + count
        return n

    def __and__(self, other):
        if isinstance(other, (int, float)):
            other = ConstantSampler(other)
        return _ConcatSampler(self, other)


class _ConcatSampler(Sampler):
    def __init__(self, left, right):
        self.left, self.right = left, right
        self.dim = left.dim + right.dim

    def sample(self, size):
        return np.concatenate([self.left.sample(size), self.right.sample(size)], axis=1)

    def sample_device(self, size, device, generator=None):
        return torch.cat([self.left.sample_device(size, device, generator),
                          self.right.sample_device(size, device, generator)], dim=1)

    def columns(self):
        left, right = self.left.columns(), self.right.columns()
        return None if left is None or right is None else left + right

    def seeds(self):
        return self.left.seeds() + self.right.seeds()


class ConstantSampler(Sampler):
    def __init__(self, value, dim=1):
        self.value, self.dim = float(value), dim

    def sample(self, size):
        return np.full((size, self.dim), self.value, dtype=np.float64)

    def sample_device(self, size, device, generator=None):
        return torch.full((size, self.dim), self.value, dtype=torch.float32, device=device)

    def columns(self):
        return [(2, self.value, 0.0)] * self.dim


class NumpySampler(Sampler):
    """ sampler named after a `numpy.random` distribution ('uniform'/'u', 'normal'/'n', ...).

    `seed=`: `sample()` (host numpy) replays numpy's own stream, as batchflow's sampler does. Inside `Solver.fit` products of
    uniform / normal / constant columns are drawn ON THE DEVICE by a counter-based Philox generator keyed with the seeds
    (`device_key`): runs are reproducible for a given seed, rank and batch count, but the points are NOT numpy's -- two
    leaves with the same seed give independent columns there, every rank draws its own points -- so a seeded run does not
    reproduce the reference's point sets bit for bit. For that, hand `fit` a sampler object without `columns()` (e.g. a
    thin wrapper exposing only `sample`): it then takes the host path of the reference (model_torch.py:433). """
    def __init__(self, name, dim=1, seed=None, **kwargs):
        self.name = _ALIASES.get(name, name)
        self.dim = dim
        self.kwargs = kwargs
        self.seed = seed
        self.rng = np.random.RandomState(seed)
        if not hasattr(self.rng, self.name):
            raise ValueError(f'unknown numpy distribution {name!r}')

    def seeds(self):
        return [self.seed] * self.dim

    def sample(self, size):
        draw = getattr(self.rng, self.name)
        return np.asarray(draw(size=(size, self.dim), **self.kwargs), dtype=np.float64)

    def sample_device(self, size, device, generator=None):
        if self.name == 'uniform' and not (set(self.kwargs) - {'low', 'high'}):
            low, high = float(self.kwargs.get('low', 0.0)), float(self.kwargs.get('high', 1.0))
            out = torch.rand((size, self.dim), dtype=torch.float32, device=device, generator=generator)
            if low != 0.0 or high != 1.0:
                out = out * (high - low) + low
            return out
        if self.name == 'normal' and not (set(self.kwargs) - {'loc', 'scale'}):
            out = torch.randn((size, self.dim), dtype=torch.float32, device=device, generator=generator)
            return out * float(self.kwargs.get('scale', 1.0)) + float(self.kwargs.get('loc', 0.0))
        return super().sample_device(size, device, generator)

    def columns(self):
        if self.name == 'uniform' and not (set(self.kwargs) - {'low', 'high'}):
            low, high = self.kwargs.get('low', 0.0), self.kwargs.get('high', 1.0)
            if np.ndim(low) == 0 and np.ndim(high) == 0:
                return [(0, float(low), float(high))] * self.dim
        if self.name == 'normal' and not (set(self.kwargs) - {'loc', 'scale'}):
            loc, scale = self.kwargs.get('loc', 0.0), self.kwargs.get('scale', 1.0)
            if np.ndim(loc) == 0 and np.ndim(scale) == 0:
                return [(1, float(loc), float(scale))] * self.dim
        return None


class ResidualSampler(Sampler):
    """ residual-based adaptive collocation sampling (RAD: Wu, Zhu, Tan, Kartha, Lu, CMAME 2023; RAR-D with replacement): every `period`
    iterations `base` draws a pool of `pool * batch_size` candidates, the solver evaluates the equation residual r on them (forward only)
    and the batch is drawn from the pool with probability proportional to |r|^power / mean(|r|^power) + floor -- on the device, by the
    resampler kernels of include/pinn.h pinn_resample_points (three launches; one for the iterations that reuse the pool).

    base    any sampler `Solver.fit` accepts; None: U[0, 1) columns. Products of uniform / normal / constant columns are drawn by the
            Philox kernel, others through `sample_device` / `sample`.
    pool    candidates per batch point (>= 1);  period: iterations one pool serves (>= 1): pool evaluation amortised over `period` batches
    power   1 or 2;  floor: the c of RAD (>= 0): 0 is purely residual-proportional, large values approach the base distribution
    seed    keys the draw stream (per-rank offset under data parallelism, like `NumpySampler(seed=)`); None: the solver's per-fit key

    `Solver.fit(sampler=...)` binds the sampler to the solver; `columns()` is None, so the fit takes the per-iteration path of any
    external sampler. For inspection: `last_pool` [M, d], `last_residual` [M], `last_indices` int32 [batch] (device tensors of the last
    call) and `evaluations`, the number of pool evaluations so far. The sampler numbers its draws itself, like a NumpySampler its batches:
    the count runs on from one fit call to the next (fresh uniforms in every call), only the iteration count that decides when a pool is
    due starts again at every fit. """
    MAX_FLOOR = 1e100

    def __init__(self, base=None, pool=4, period=1, power=1, floor=1.0, seed=None):
        def integer(value, name, meaning):
            try:
                if isinstance(value, bool):
                    raise TypeError
                value = operator.index(value)           # (Python and numpy integers alike)
            except TypeError:
                value = 0
            if value < 1:
                raise ValueError(f'ResidualSampler: {name} must be an integer >= 1 ({meaning})')
            return value
        pool = integer(pool, f'pool={pool!r}', 'candidates per batch point')
        period = integer(period, f'period={period!r}', 'iterations per pool')
        if power not in (1, 2):
            raise ValueError(f'ResidualSampler: power={power!r} must be 1 or 2')
        if not (isinstance(floor, numbers.Real) and not isinstance(floor, bool) and 0.0 <= float(floor) <= self.MAX_FLOOR):
            raise ValueError(f'ResidualSampler: floor={floor!r} must be a number in [0, {self.MAX_FLOOR:g}] (include/pinn.h PINN_RESAMPLE_MAX_FLOOR)')
        self.base, self.pool, self.period, self.power, self.floor, self.seed = base, pool, period, int(power), float(floor), seed
        if base is not None:
            self.dim = base.dim
        self.solver = None
        self.evaluations = 0
        self.last_pool = self.last_residual = self.last_indices = None
        self._iteration, self._draws, self._workspace, self._pool_size = 0, 0, None, None

    def columns(self):
        return None

    def seeds(self):
        return [self.seed]

    def bind_solver(self, solver):
        """ called by `Solver.fit` at the start of the call: iteration 0 of this fit draws a fresh pool """
        self.solver = solver
        self.dim = solver.model.total
        self._iteration = 0

    def _key(self):
        solver = self.solver
        if self.seed is None:
            if solver._sample_seed is None:
                solver._new_sample_seed()
            return solver._sample_seed              # (per fit call, per rank)
        rank, _ = solver._world()
        return (self.device_key() + 7919 * rank) & (2 ** 64 - 1)

    def sample_device(self, size, device=None, generator=None):
        solver = self.solver
        if solver is None:
            raise RuntimeError('ResidualSampler draws by the residual of a solver: pass it to Solver.fit(sampler=...) (or call '
                               'bind_solver(solver)) before sampling')
        net = solver.model.net
        m = self.pool * size
        fresh = self._iteration % self.period == 0 or self._pool_size != m or self.last_pool is None
        if fresh:
            self.last_pool = solver._sample(m, self.base)
            self.last_residual = solver._residual_device(self.last_pool)
            self.evaluations += 1
            self._pool_size = m
            if self._workspace is None or self._workspace.device != self.last_pool.device or \
                    self._workspace.numel() * 8 < int(net.lib.pinn_resample_workspace_bytes(m)):
                self._workspace = net.resample_workspace(m, self.last_pool.device)
        xs, self.last_indices, _ = net.resample_points(self.last_pool, self.last_residual, size, self.power, self.floor, self._key(),
                                                       self._draws, workspace=self._workspace, redraw=not fresh)
        self._draws += 1
        self._iteration += 1
        return xs

    def sample(self, size):
        return self.sample_device(size).detach().cpu().numpy().astype(np.float64)


NS = NumpySampler
