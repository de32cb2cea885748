""" A zero gradient is not an unreached scalar.

torch's optimizers skip a parameter WITHOUT a gradient (`.grad is None`: the loss of this call does not reach it) and step one whose gradient
is a zero-valued tensor like any other: its step count advances, it decays, its momentum carries on. The reference (model_torch.py:419-461)
inherits both. `Solver.fit` decides per fit call which trainable scalars (log_scale, V(...) slots, the output bias) the loss terms reach and
clears the others' bits in the mask the optimizer kernels read (`FlatOptimizer.refresh`, `TorchOptimizerAdapter.refresh`); this file pins that
the decision follows the GRAPH and not the gradient's value:

  a. zero_cofactor       u_xx - V('amp', 0) sin(V('freq', 1) x) - 1: d loss / d freq is exactly 0 on the first batch and not afterwards
  b. zero_variable       the scalar itself starts at 0, its gradient does not (control)
  c. off_probe_domain    a coefficient switched on only outside U[0, 1), batches from [2, 3)
  d. truly unreached     a V of the equation in a constraint-only call, log_scale without an initial condition: skipped, bit for bit (control)
  e. reused optimizer    fit(AdamW) then fit(optimizer=None): per-parameter step counts against torch's state
  f. chunk forms         eager loop, chunk entry point / launch graphs, one-CU chunk on the BASELINE config 1 net at batch 100
  g. two-team kernel     the 4 x 64 shape: both V gradients of one kernel step, the mask bit, three iterations
  h. one-entry layer parameters on the torch path: `p.grad is None` per parameter as the oracle has it

The reference is oracle.pinn_oracle.OracleSolver (torch autograd and the real torch.optim rule) stepped from the same fp32 start on the same
pre-drawn batches, in fp32 and -- where the bar is missed -- in fp64. Bars: helpers.fit_close (FIT_LOSS_RTOL, FIT_PARAM_RTOL, the fp64 arbiter
at k = 2, adam_move = lr * steps); a scalar's own value at the same bar against the oracle's scalar. One optimizer step on a zero gradient is
one or two fp32 roundings of a value near 1 (the decay; SGD's p - lr (wd p)): "equal after iteration 1" is 2 ulp (DECAY_ULPS).
CPU tier on the emulator build, `-m gpu` twins on the HIP library. """
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import params_close
from helpers import (FIT_PARAM_RTOL, FixedBatches, GRAD_RTOL, close_or_arbitrated, fit_close, linear_modules, load_params, record_margin)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'emu'))

STANDING = dict(ndims=1, layout='fafaf', features=[8, 8, 1], activation='Tanh')
BATCH, NITERS, LR = 37, 20, 0.01           # two full tiles and a tail of 5
DECAY_ULPS = 2


@pytest.fixture(scope='module')
def emu_lib():
    import build_emu
    from pydens_amd import engine
    lib = engine.bind(ctypes.CDLL(build_emu.build()))
    assert lib.pinn_backend() == b'emu-host'
    return lib


@pytest.fixture(scope='module')
def pa():
    import pydens_amd
    return pydens_amd


@pytest.fixture(scope='module')
def gpu_lib(pa):
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    lib = pa.engine.load_library()
    assert lib.pinn_backend() == b'hip-gfx950'
    return lib


def emu_kwargs(lib):
    return dict(_lib=lib, device='cpu')


# ---- the problems: make(D, V, dtype) -> (equation, constraints or None) ---------------------------------------------------------------------
def zero_cofactor(D, V, dtype):
    return (lambda u, x: D(D(u, x), x) - V('amp', data=torch.Tensor([0.0])) * torch.sin(V('freq', data=torch.Tensor([1.0])) * x) - 1), None


def zero_cofactor_2d(D, V, dtype):
    return (lambda u, x, y: D(D(u, x), x) + D(D(u, y), y)
            - V('amp', data=torch.Tensor([0.0])) * torch.sin(V('freq', data=torch.Tensor([1.0])) * x) - 1), None


def zero_variable(D, V, dtype):
    return (lambda u, x: D(u, x) - V('k', data=torch.Tensor([0.0])) * u - 1), None


def off_probe_domain(D, V, dtype):
    return (lambda u, x: D(D(u, x), x) - V('c', data=torch.Tensor([1.0])) * torch.relu(x - 1.5) - 1), None


def equation_only_variable(D, V, dtype):
    eq = lambda u, x: D(u, x) - 2 * np.pi * torch.cos(2 * np.pi * x) + V('new_var', data=torch.Tensor([1.0]))
    return eq, (lambda f, x: f(torch.tensor([0.5], dtype=dtype)))


def vector_variable(D, V, dtype):
    def eq(u, x):
        w = V('w', data=torch.zeros(2))
        return D(D(u, x), x) - w[0] * torch.sin(x) - w[1] * torch.cos(x) - 1
    return eq, (lambda f, x: f(torch.tensor([0.5], dtype=dtype)) - 0.2)


class Pair:
    """ the oracle (fp32; fp64 from the same fp32 start on demand) and the solver, given the same fit calls """
    def __init__(self, pa, extra, make, kw, path=None, seed=0, edit_start=None):
        from oracle import pinn_oracle as po
        self.po, self.make, self.kw, self.calls, self._o64 = po, make, kw, [], None
        torch.manual_seed(seed)
        self.oracle = self._oracle(torch.float32)
        self.start = [np.asarray(p, dtype=np.float32) for p in self.oracle.export_params()]
        if edit_start is not None:
            edit_start(self.start)
            self.oracle.import_params(self.start)
        eq, con = make(pa.D, pa.V, torch.float32)
        self.solver = pa.Solver(eq, constraints=con, **kw, **extra)
        load_params(self.solver, self.start)
        if path == 'fused':
            self.solver.set_optimizer_path('fused')

    def _oracle(self, dtype):
        eq, con = self.make(self.po.D, self.po.V, dtype)
        return self.po.OracleSolver(eq, constraints=con, dtype=dtype, **self.kw)

    def fit(self, pts, sampler=None, **call):
        self.calls.append((pts, call))
        self.oracle.fit(niters=len(pts), batch_size=pts.shape[1], points=pts, **call)
        self.solver.fit(niters=len(pts), batch_size=pts.shape[1], sampler=FixedBatches(pts) if sampler is None else sampler, **call)

    def oracle64(self):
        if self._o64 is None:
            self._o64 = self._oracle(torch.float64)
            self._o64.import_params(self.start)
            for pts, call in self.calls:
                self._o64.fit(niters=len(pts), batch_size=pts.shape[1], points=pts, **call)
        return self._o64

    def values(self, name):
        """ (ours, fp32 oracle) of a V(...) """
        return (getattr(self.solver.model, name).detach().cpu().numpy().astype(np.float64).ravel(),
                getattr(self.oracle.model, name).detach().numpy().astype(np.float64).ravel())

    def scalar_close(self, test, case, name, steps, lr=LR):
        """ a V(...)'s own value at the bar of fit_close's parameters against the oracle's """
        got, want = self.values(name)
        ok, err, arb = close_or_arbitrated(got, want, lambda: getattr(self.oracle64().model, name).detach().numpy().ravel(), FIT_PARAM_RTOL,
                                           atol=2e-6, adam_move=lr * steps)
        record_margin(test, f'{case}[V {name}]', 'scalar', err, FIT_PARAM_RTOL, arb)
        print(f'{test} {case}: V({name}) ours {got} oracle {want} err {err:.2e}{" (fp64 arbiter)" if arb else ""}')
        assert ok, (case, name, got, want, err)

    def close(self, test, case, steps, lr=LR):
        fit_close(test, case, self.solver, self.oracle, self.oracle64, adam_move=lr * steps)


def _points(seed, niters, batch, dims=1, low=0.0, high=1.0):
    return (low + (high - low) * np.random.RandomState(seed).rand(niters, batch, dims)).astype(np.float32)


def _ulps(got, want):
    return abs(float(got) - float(want)) / (2.0 ** -23 * abs(float(want)))


# ---- a. zero_cofactor ----------------------------------------------------------------------------------------------------------------------------
WD_RULES = {'adamw': ('AdamW', dict(weight_decay=0.1)), 'sgd': ('SGD', dict(momentum=0.9, dampening=0.3, weight_decay=0.1)),
            'rmsprop': ('RMSprop', dict(momentum=0.9, weight_decay=0.1))}
COFACTOR_RUNS = [('adam', None)] + [(rule, path) for path in ('fused', 'torch') for rule in WD_RULES]
COFACTOR_IDS = [rule if path is None else f'{rule}-{path}' for rule, path in COFACTOR_RUNS]
COFACTOR_KW = dict(boundary_condition=0.0, **STANDING)


def _cofactor_case(pa, extra, test, rule, path):
    name, okw = ('Adam', {}) if rule == 'adam' else WD_RULES[rule]
    case = f'zero_cofactor/{rule}/{path or "default"}'
    pts = _points(40, NITERS, BATCH)
    if okw.get('weight_decay'):
        # the reference decays a reached parameter whose gradient is a zero tensor: freq after ONE iteration against the oracle's
        one = Pair(pa, extra, zero_cofactor, COFACTOR_KW, path)
        one.fit(pts[:1], optimizer=name, lr=LR, **okw)
        got, want = one.values('freq')
        print(f'{test} {case}: freq after iteration 1 ours {got[0]!r} oracle {want[0]!r}')
        assert want[0] != 1.0                                   # (the oracle did decay it)
        assert got[0] != 1.0 and _ulps(got[0], want[0]) <= DECAY_ULPS, (got, want)
    pair = Pair(pa, extra, zero_cofactor, COFACTOR_KW, path)
    pair.fit(pts, optimizer=name, lr=LR, **okw)
    expected = 'Adam/fused' if rule == 'adam' else f'{name}/{path}'
    assert pair.solver.last_fit_optimizer == expected
    pair.close(test, case, NITERS)
    assert pair.values('freq')[1][0] != 1.0                     # the reference moved it ...
    assert pair.values('freq')[0][0] != 1.0                     # ... and so did we
    pair.scalar_close(test, case, 'freq', NITERS)
    pair.scalar_close(test, case, 'amp', NITERS)


@pytest.mark.parametrize('rule,path', COFACTOR_RUNS, ids=COFACTOR_IDS)
def test_zero_cofactor_on_the_emulator(pa, emu_lib, rule, path):
    _cofactor_case(pa, emu_kwargs(emu_lib), 'zero_gradient_a_emu', rule, path)


@pytest.mark.gpu
@pytest.mark.parametrize('rule,path', COFACTOR_RUNS, ids=COFACTOR_IDS)
def test_zero_cofactor_on_the_gpu(pa, gpu_lib, rule, path):
    _cofactor_case(pa, {}, 'zero_gradient_a_gpu', rule, path)


# ---- b. zero_variable (control) ------------------------------------------------------------------------------------------------------------------
def _zero_variable_case(pa, extra, test):
    for path, (name, okw) in [(None, ('Adam', {})), ('fused', WD_RULES['adamw']), ('torch', WD_RULES['adamw'])]:
        pair = Pair(pa, extra, zero_variable, dict(initial_condition=1.0, **STANDING), path)
        pair.fit(_points(41, NITERS, BATCH), optimizer=name, lr=LR, **okw)
        case = f'zero_variable/{name}/{path or "default"}'
        pair.close(test, case, NITERS)
        assert pair.values('k')[0][0] != 0.0
        pair.scalar_close(test, case, 'k', NITERS)


def test_zero_variable_on_the_emulator(pa, emu_lib):
    _zero_variable_case(pa, emu_kwargs(emu_lib), 'zero_gradient_b_emu')


@pytest.mark.gpu
def test_zero_variable_on_the_gpu(pa, gpu_lib):
    _zero_variable_case(pa, {}, 'zero_gradient_b_gpu')


# ---- c. off_probe_domain ---------------------------------------------------------------------------------------------------------------------------
def _off_domain_case(pa, extra, test, draw):
    from oracle import philox
    kw = dict(boundary_condition=0.0, domain=(2, 3), **STANDING)
    sampler = None
    if draw == 'fixed_batches':
        pts = _points(42, NITERS, BATCH, low=2.0, high=3.0)
    else:
        # the sampler's batches, drawn on the device by the Philox kernel, restated on the host for the oracle (bit-exact for uniform columns)
        sampler = pa.NumpySampler('uniform', low=2, high=3, seed=3)
        pts = np.stack([philox.sample_points(BATCH, [(philox.UNIFORM, 2.0, 3.0)], sampler.device_key(), i) for i in range(NITERS)])
    assert pts.min() >= 2.0 and pts.max() <= 3.0
    for path, (name, okw) in [(None, ('Adam', {})), ('fused', WD_RULES['adamw']), ('torch', WD_RULES['sgd'])]:
        if sampler is not None:
            sampler = pa.NumpySampler('uniform', low=2, high=3, seed=3)
        pair = Pair(pa, extra, off_probe_domain, kw, path)
        pair.fit(pts, sampler=sampler, optimizer=name, lr=LR, **okw)
        case = f'off_probe_domain/{draw}/{name}/{path or "default"}'
        pair.close(test, case, NITERS)
        assert pair.values('c')[1][0] != 1.0 and pair.values('c')[0][0] != 1.0
        pair.scalar_close(test, case, 'c', NITERS)


@pytest.mark.parametrize('draw', ['fixed_batches', 'numpy_sampler'])
def test_off_probe_domain_on_the_emulator(pa, emu_lib, draw):
    _off_domain_case(pa, emu_kwargs(emu_lib), 'zero_gradient_c_emu', draw)


@pytest.mark.gpu
@pytest.mark.parametrize('draw', ['fixed_batches', 'numpy_sampler'])
def test_off_probe_domain_on_the_gpu(pa, gpu_lib, draw):
    _off_domain_case(pa, {}, 'zero_gradient_c_gpu', draw)


# ---- d. truly unreached stays skipped (control) --------------------------------------------------------------------------------------------
def _nonzero_log_scale(start):
    start[-1] = np.float32(0.25)            # (0.0 would hide a decay)


def _truly_unreached_case(pa, extra, path):
    """ constraint-only call, no initial condition: the equation's V and log_scale have no gradient in the reference -- value, moments and
    step count stay, bit for bit, and torch keeps no (or an unchanged) state for them """
    from pydens_amd.solver import FlatOptimizer, TorchOptimizerAdapter
    pair = Pair(pa, extra, equation_only_variable, dict(boundary_condition=1.0, **STANDING), path, edit_start=_nonzero_log_scale)
    pts = _points(43, 3, BATCH)
    pair.fit(pts, optimizer='AdamW', lr=LR, weight_decay=0.1, loss_terms=['constraint_0'])
    assert pair.solver.last_fit_optimizer == f'AdamW/{path}'
    solver, oracle = pair.solver, pair.oracle
    for ours, theirs, start in ((solver.model.new_var, oracle.model.new_var, 1.0), (solver.model.log_scale, oracle.model.log_scale, 0.25)):
        assert theirs.grad is None and len(oracle.optimizer.state.get(theirs, {})) == 0
        assert float(theirs.detach()) == start
        assert float(ours.detach()) == start
        off = ours.storage_offset()
        opt = solver.optimizer
        if path == 'fused':
            assert isinstance(opt, FlatOptimizer)
            assert float(opt.exp_avg[off]) == 0.0 and float(opt.exp_avg_sq[off]) == 0.0 and opt.steps_of(off) == 0
            assert int(opt.mask[off]) == 0
        else:
            assert isinstance(opt, TorchOptimizerAdapter)
            assert len(opt.opt.state.get(ours, {})) == 0
    # the network WAS stepped and decayed, as in the reference
    w0 = linear_modules(solver)[0].weight
    assert not np.array_equal(w0.detach().cpu().numpy(), pair.start[0])
    for got, want in zip([m.weight.detach().cpu().numpy() for m in linear_modules(solver)], oracle.export_params()[0::2]):
        assert params_close(got, want, FIT_PARAM_RTOL, atol=2e-6)


@pytest.mark.parametrize('path', ['fused', 'torch'])
def test_truly_unreached_stays_skipped_on_the_emulator(pa, emu_lib, path):
    _truly_unreached_case(pa, emu_kwargs(emu_lib), path)


@pytest.mark.gpu
@pytest.mark.parametrize('path', ['fused', 'torch'])
def test_truly_unreached_stays_skipped_on_the_gpu(pa, gpu_lib, path):
    _truly_unreached_case(pa, {}, path)


# ---- e. reused optimizer --------------------------------------------------------------------------------------------------------------------------
def _steps(pair, param_ours, param_theirs):
    """ (our step count of a parameter, torch's in the oracle) """
    from pydens_amd.solver import FlatOptimizer
    opt = pair.solver.optimizer
    want = pair.oracle.optimizer.state.get(param_theirs, {}).get('step')
    want = 0 if want is None else int(want)
    if isinstance(opt, FlatOptimizer):
        return opt.steps_of(param_ours.storage_offset()), want
    got = opt.opt.state.get(param_ours, {}).get('step')
    return (0 if got is None else int(got)), want


def _reused_case(pa, extra, test, path):
    from pydens_amd.solver import FlatOptimizer
    pair = Pair(pa, extra, zero_cofactor, COFACTOR_KW, path)
    pts = _points(44, 10, BATCH)
    pair.fit(pts[:5], optimizer='AdamW', lr=LR, weight_decay=0.1)
    first = pair.solver.optimizer
    if path == 'fused':
        lagging, seen = FlatOptimizer.lagging, []

        def watched(self, offsets):
            seen.append(lagging(self, offsets))
            return seen[-1]
        FlatOptimizer.lagging = watched
    try:
        pair.fit(pts[5:], optimizer=None, lr=LR)
    finally:
        if path == 'fused':
            FlatOptimizer.lagging = lagging
    if path == 'fused':
        assert seen == [[]], seen                               # amp and freq were reached all along: nothing lags
        assert pair.solver.optimizer is first and pair.solver.last_fit_optimizer == 'AdamW/fused'
    for name in ('amp', 'freq'):
        got, want = _steps(pair, getattr(pair.solver.model, name), getattr(pair.oracle.model, name))
        assert got == want == 10, (name, got, want)
    case = f'reused_optimizer/{path}'
    pair.close(test, case, 10)
    pair.scalar_close(test, case, 'freq', 10)
    pair.scalar_close(test, case, 'amp', 10)


def _reused_vector_case(pa, extra, test):
    """ a two-entry V that a constraint-only call does not reach lags behind the buffer in the next call: torch's optimizer takes over
    (TorchOptimizerAdapter.continuing) and the vector's step count is its own, not the buffer's """
    from pydens_amd.solver import TorchOptimizerAdapter
    pair = Pair(pa, extra, vector_variable, COFACTOR_KW, 'fused')
    pts = _points(45, 6, BATCH)
    pair.fit(pts[:3], optimizer='AdamW', lr=LR, weight_decay=0.1, loss_terms=['constraint_0'])
    assert np.array_equal(pair.values('w')[0], [0.0, 0.0])
    got, want = _steps(pair, pair.solver.model.w, pair.oracle.model.w)
    assert got == want == 0
    pair.fit(pts[3:], optimizer=None, lr=LR, loss_terms=['equation', 'constraint_0'])
    assert isinstance(pair.solver.optimizer, TorchOptimizerAdapter)
    got, want = _steps(pair, pair.solver.model.w, pair.oracle.model.w)
    assert got == want == 3, (got, want)
    w0 = linear_modules(pair.solver)[0].weight
    got, want = _steps(pair, w0, pair.oracle.model.linears()[0].weight)
    assert got == want == 6, (got, want)
    pair.close(test, 'reused_optimizer/vector', 6)
    pair.scalar_close(test, 'reused_optimizer/vector', 'w', 6)


@pytest.mark.parametrize('path', ['fused', 'torch'])
def test_reused_optimizer_on_the_emulator(pa, emu_lib, path):
    _reused_case(pa, emu_kwargs(emu_lib), 'zero_gradient_e_emu', path)


def test_reused_optimizer_vector_variable_on_the_emulator(pa, emu_lib):
    _reused_vector_case(pa, emu_kwargs(emu_lib), 'zero_gradient_e_emu')


@pytest.mark.gpu
@pytest.mark.parametrize('path', ['fused', 'torch'])
def test_reused_optimizer_on_the_gpu(pa, gpu_lib, path):
    _reused_case(pa, {}, 'zero_gradient_e_gpu', path)


@pytest.mark.gpu
def test_reused_optimizer_vector_variable_on_the_gpu(pa, gpu_lib):
    _reused_vector_case(pa, {}, 'zero_gradient_e_gpu')


# ---- f. chunk forms ---------------------------------------------------------------------------------------------------------------------------------
CFG1 = dict(ndims=2, boundary_condition=1, layout='fa fa fa f', features=[10, 12, 15, 1], activation='Tanh')     # BASELINE config 1's net
CHUNK_ITERS = 140           # one full chunk of 128 and a tail


def _chunk_run(pa, extra, lib, monkeypatch, graph, persist, eager_loop=False, rounds=None):
    monkeypatch.setenv('PYDENS_AMD_FIT_GRAPH', '1' if graph else '0')
    monkeypatch.setenv('PYDENS_AMD_FIT_PERSIST', str(persist))
    if rounds is not None:
        monkeypatch.setenv('PYDENS_AMD_FIT_ROUNDS', str(rounds))
    torch.manual_seed(21)
    solver = pa.Solver(zero_cofactor_2d(pa.D, pa.V, torch.float32)[0], **CFG1, **extra)
    if eager_loop:
        solver._device_columns = lambda sampler: None           # the per-iteration loop
    solver.fit(niters=CHUNK_ITERS, batch_size=100, lr=0.005)
    assert solver.last_fit_path == 'fused' and solver.last_fit_optimizer == 'Adam/fused', solver.program_error
    opt = solver.optimizer
    return dict(losses=np.array([float(v) for v in solver.losses]), params=solver.model.flat.detach().cpu().numpy().copy(),
                m=opt.exp_avg.cpu().numpy().copy(), v=opt.exp_avg_sq.cpu().numpy().copy(), t=int(opt.step_count.item()),
                kernel=lib.pinn_last_kernel_name().decode(), freq=float(solver.model.freq.detach()), amp=float(solver.model.amp.detach()),
                mask=int(opt.mask[solver.model.freq.storage_offset()]))


def _moved(run):
    assert run['t'] == CHUNK_ITERS and np.isfinite(run['losses']).all()
    assert run['mask'] == 1 and run['amp'] != 0.0
    assert run['freq'] != 1.0, run['freq']


def _chunk_forms_case(pa, extra, lib, monkeypatch):
    eager = _chunk_run(pa, extra, lib, monkeypatch, False, 0, eager_loop=True)
    _moved(eager)
    for graph in (False, True):                                 # the chunk entry point: its own loop, its launch graphs
        run = _chunk_run(pa, extra, lib, monkeypatch, graph, 0)
        _moved(run)
        for key in ('losses', 'params', 'm', 'v'):
            assert np.array_equal(run[key], eager[key]), (graph, key)
    return eager


def _one_cu_case(pa, extra, lib, monkeypatch):
    """ the one-CU chunk against the eager loop at the bounds of test_fused_optimizers._one_cu_case (another summation order: not bits) """
    a = _chunk_run(pa, extra, lib, monkeypatch, True, 0, rounds=4)
    b = _chunk_run(pa, extra, lib, monkeypatch, True, 2, rounds=4)
    assert b['kernel'].startswith('pinn_fit_kernel<') and not b['kernel'].endswith(',1>'), b['kernel']
    _moved(a)
    _moved(b)
    np.testing.assert_allclose(b['losses'][:8], a['losses'][:8], rtol=2e-6)
    np.testing.assert_allclose(b['losses'], a['losses'], rtol=2e-4)
    assert params_close(b['params'], a['params'], 2e-4)
    assert abs(b['freq'] - a['freq']) <= 2e-4 * abs(a['freq'])


def test_chunk_forms_move_a_zero_gradient_scalar_on_the_emulator(pa, emu_lib, monkeypatch):
    monkeypatch.setattr(pa.Solver, 'FIT_CTRL_ON_HOST', True)
    _chunk_forms_case(pa, emu_kwargs(emu_lib), emu_lib, monkeypatch)


def test_one_cu_chunk_moves_a_zero_gradient_scalar_on_the_emulator(pa, emu_lib, monkeypatch):
    monkeypatch.setattr(pa.Solver, 'FIT_CTRL_ON_HOST', True)
    _one_cu_case(pa, emu_kwargs(emu_lib), emu_lib, monkeypatch)


@pytest.mark.gpu
def test_chunk_forms_move_a_zero_gradient_scalar_on_the_gpu(pa, gpu_lib, monkeypatch):
    _chunk_forms_case(pa, {}, gpu_lib, monkeypatch)


@pytest.mark.gpu
def test_one_cu_chunk_moves_a_zero_gradient_scalar_on_the_gpu(pa, gpu_lib, monkeypatch):
    _one_cu_case(pa, {}, gpu_lib, monkeypatch)


# ---- g. two-team kernel ------------------------------------------------------------------------------------------------------------------------------
def two_team_term(D, V, dtype):
    # test_residual_program_ops.ANSATZ['two_team_4x64'] with k = V('k', 0) in front of a term that holds a second V at 1.0
    return (lambda u, x, y: D(D(u, x), x) + D(D(u, y), y) + V('k', data=torch.Tensor([0.0])) * torch.sin(V('freq', data=torch.Tensor([1.0])) * x + u)
            - 5 * torch.sin(np.pi * (x + y))), None


def _two_team_case(pa, extra, test):
    from test_residual_program_ops import ANSATZ
    kw = ANSATZ['two_team_4x64'][0]
    pair = Pair(pa, extra, two_team_term, kw, seed=5)
    solver = pair.solver
    pts = _points(46, 3, 97, dims=2)
    # one kernel step: both V slots' gradients against the oracle (d loss / d freq = k * (...) is exactly zero)
    grads = {}
    for dtype in (torch.float32, torch.float64):
        o = pair._oracle(dtype)
        o.import_params(pair.start)
        o.evaluate(pts[0])
        grads[dtype] = {n: float(getattr(o.model, n).grad) for n in ('k', 'freq')}
        assert getattr(o.model, 'freq').grad is not None
    solver._fused_step(torch.from_numpy(pts[0]).to(solver.device), 1)
    kernel = solver.model.net.lib.pinn_last_kernel_name().decode()
    var = int(kernel.rstrip('>').split(',')[-1])
    assert kernel.startswith('pinn_tile_kernel<') and var & 256 and var & 2048, kernel
    for n in ('k', 'freq'):
        got = float(solver.grads[solver.model.variables[n][0]])
        ok, err, arb = close_or_arbitrated([got], [grads[torch.float32][n]], lambda n=n: [grads[torch.float64][n]], GRAD_RTOL)
        record_margin(test, f'two_team[V {n}]', 'grad', err, GRAD_RTOL, arb)
        print(f'{test}: V({n}) gradient ours {got:.9g} f32 {grads[torch.float32][n]:.9g} f64 {grads[torch.float64][n]:.9g}')
        assert ok, (n, got, grads)
    assert grads[torch.float32]['freq'] == 0.0 and grads[torch.float32]['k'] != 0.0
    pair.fit(pts, optimizer='Adam', lr=LR)
    assert solver.last_fit_path == 'fused' and solver.last_fit_optimizer == 'Adam/fused', solver.program_error
    for n in ('k', 'freq'):
        assert int(solver.optimizer.mask[solver.model.variables[n][0]]) == 1, n        # the mask handed to the Adam launch
    pair.close(test, 'two_team', 3)
    assert pair.values('freq')[1][0] != 1.0 and pair.values('freq')[0][0] != 1.0
    pair.scalar_close(test, 'two_team', 'freq', 3)
    pair.scalar_close(test, 'two_team', 'k', 3)


def test_two_team_kernel_on_the_emulator(pa, emu_lib):
    _two_team_case(pa, emu_kwargs(emu_lib), 'zero_gradient_g_emu')


@pytest.mark.gpu
def test_two_team_kernel_on_the_gpu(pa, gpu_lib):
    _two_team_case(pa, {}, 'zero_gradient_g_gpu')


# ---- h. one-entry layer parameters on the torch path ------------------------------------------------------------------------------------------
ONE_UNIT = dict(ndims=1, layout='faf', features=[1, 1], activation='Tanh')
ONE_UNIT_EQUATIONS = {
    # the output bias is outside the double-backward graph: u_x, u_xx of W2 tanh(W1 x + b1) + b2 do not hold b2
    'derivatives_only': lambda D, V, dtype: ((lambda u, x: D(D(u, x), x) + 0.5 * D(u, x) - torch.sin(2.0 * x)), None),
    'ordinary': lambda D, V, dtype: ((lambda u, x: D(u, x) - 0.5 * u - torch.sin(2.0 * x)), None),
}
# what the oracle showed when this test was written (asserted below, so that a change of the reference's graph is noticed):
# `p.grad is None` after backward for W1, b1, W2, b2, log_scale
ORACLE_GRAD_IS_NONE = {'derivatives_only': [False, False, False, True, True], 'ordinary': [False, False, False, False, True]}


def _one_unit_case(pa, extra, test, which, monkeypatch):
    from pydens_amd.solver import TorchOptimizerAdapter
    pair = Pair(pa, extra, ONE_UNIT_EQUATIONS[which], ONE_UNIT, 'torch', seed=3, edit_start=_nonzero_log_scale)
    bound, bind = [], TorchOptimizerAdapter._bind

    def recording(self, grads, contiguous=False):
        bind(self, grads, contiguous)
        bound.append({id(p): p.grad is None for p in self.params})
    monkeypatch.setattr(TorchOptimizerAdapter, '_bind', recording)
    pair.fit(_points(47, 5, BATCH), optimizer='SGD', lr=LR, momentum=0.9, weight_decay=0.1)
    assert pair.solver.last_fit_optimizer == 'SGD/torch' and len(bound) == 5
    theirs = [p for lin in pair.oracle.model.linears() for p in (lin.weight, lin.bias)] + [pair.oracle.model.log_scale]
    ours = [p for lin in linear_modules(pair.solver) for p in (lin.weight, lin.bias)] + [pair.solver.model.log_scale]
    assert all(p.numel() == 1 for p in ours)
    table = [p.grad is None for p in theirs]
    print(f'{test} one_unit/{which}: oracle p.grad is None for W1, b1, W2, b2, log_scale: {table}')
    assert table == ORACLE_GRAD_IS_NONE[which]
    for step in bound:
        assert [step[id(p)] for p in ours] == table, (which, step, table)
    pair.close(test, f'one_unit/{which}', 5)
    for p, q in zip(ours, theirs):
        if q.grad is None:
            assert float(p.detach()) == float(q.detach())       # neither decayed nor moved: bit for bit


@pytest.mark.parametrize('which', list(ONE_UNIT_EQUATIONS))
def test_one_entry_layer_parameters_on_the_emulator(pa, emu_lib, monkeypatch, which):
    _one_unit_case(pa, emu_kwargs(emu_lib), 'zero_gradient_h_emu', which, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize('which', list(ONE_UNIT_EQUATIONS))
def test_one_entry_layer_parameters_on_the_gpu(pa, gpu_lib, monkeypatch, which):
    _one_unit_case(pa, {}, 'zero_gradient_h_gpu', which, monkeypatch)
