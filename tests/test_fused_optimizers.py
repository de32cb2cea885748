""" The optimizer family of the kernels (`Solver.set_optimizer_path('fused')`; include/pinn.h pinn_optim_t): Adam and AdamW with weight decay,
SGD and RMSprop with torch.optim semantics applied in the gradient reduction's launch, in the fit chunks, their launch graphs and the one-CU
chunk kernel instead of as torch.optim code behind the step (reference model_torch.py:419-422, :461). CPU tier on the emulator build of the
product sources, `-m gpu` twins on the device.

Tolerances are the suite's own. Kernel against torch.optim: masked entries untouched, live ones within 1e-6 relative L2
(test_adam_matches_torch). `Solver.fit` against the oracle: losses 1e-5 relative, parameters through `close_or_arbitrated` at 3e-5, a trainable
V(...) within 2e-5 absolute (test_fused_criteria). Sequences of fit calls on the tutorial's trainable-variable problem: the 5e-5 / 5e-5 / 2e-5 of
the tests on that problem in test_emu_engine (test_constraint_terms_as_residual_programs, test_freeze_and_unfreeze). Chunk forms: launch graphs
bit for bit, the one-CU kernel at the bounds of test_emu_engine._one_launch_case. Data parallel: the 1e-5 of test_data_parallel.

`adam_move` of `close_or_arbitrated` (the farthest an entry whose gradient is fp32 noise can be moved by the rule, used only when the fp64
oracle arbitrates): Adam and AdamW lr per step; RMSprop divides by sqrt(square_avg) with square_avg = (1 - alpha) g^2 after the first step,
so at most lr / sqrt(1 - alpha) per step, and its momentum buffer sums those moves with weight momentum^j: step k moves at most
(1 + ... + momentum^(k-1)) times that.
SGD is linear in the gradient and amplifies nothing: no allowance. """
import ctypes
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
from torch import nn

from conftest import params_close, rel_l2
from helpers import FixedBatches, close_or_arbitrated, export_params, load_params, make_solver

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'emu'))

LOSS_RTOL, PARAM_RTOL, VAR_ATOL = 1e-5, 3e-5, 2e-5
NITERS, LR = 4, 0.005


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


def emu_kwargs(lib):
    return dict(_lib=lib, device='cpu')


# ---- 1. the rules against torch.optim, kernel only ---------------------------------------------------------------------------------------
RULE_CASES = [('Adam', dict(weight_decay=0.01)), ('Adam', dict(weight_decay=0.1, betas=(0.8, 0.95), eps=1e-6)),
              ('AdamW', {}), ('AdamW', dict(weight_decay=0.1)),
              ('SGD', {}), ('SGD', dict(momentum=0.9)), ('SGD', dict(momentum=0.9, dampening=0.3, weight_decay=0.01)),
              ('SGD', dict(momentum=0.9, nesterov=True, weight_decay=0.01)),
              ('RMSprop', {}), ('RMSprop', dict(alpha=0.9, weight_decay=0.01)), ('RMSprop', dict(momentum=0.9)), ('RMSprop', dict(centered=True))]
RULE_IDS = [name + ''.join(f'-{k}={v}' for k, v in kw.items()) for name, kw in RULE_CASES]


def _optim_struct(pa, name, lr, kw):
    from pydens_amd.solver import FlatOptimizer
    hyper = FlatOptimizer.hyper(name, lr, kw)
    assert hyper is not None, (name, kw)
    return pa.engine.Optim.build(FlatOptimizer.RULES[name][0], **hyper)


def _rule_case(pa, lib, device, name, kw, n, steps=20):
    """ test_adam_matches_torch for every rule: random parameters and gradients, every seventh entry masked, the two standalone forms
    (step counted on the device / passed by value) alternating """
    engine = pa.engine
    torch.manual_seed(0)
    p = torch.randn(n, device=device)
    ref = p.clone().requires_grad_()
    opt = getattr(torch.optim, name)([ref], lr=0.01, **kw)
    optim = _optim_struct(pa, name, 0.01, kw)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step = torch.zeros(1, dtype=torch.int32, device=device)
    mask = torch.ones(n, dtype=torch.uint8, device=device)
    mask[::7] = 0
    keep = p.clone()
    net = engine.Net([2, 16, 1], 'tanh', 2, lib=lib)
    for k in range(steps):
        grad = torch.randn(n, device=device)
        ref.grad = grad.clone()
        opt.step()
        net.optim_step(p, grad, m, v, mask, step, optim, at=0 if k % 2 == 0 else k + 1)
    live = mask.bool()
    err = rel_l2(p[live].cpu().numpy(), ref.detach()[live].cpu().numpy())
    print(f'{name} {kw}: relative L2 against torch.optim after {steps} steps {err:.2e}')
    assert torch.equal(p[~live], keep[~live])                    # a masked entry keeps its value: it is not decayed either
    assert torch.equal(m[~live], torch.zeros_like(m[~live])) and torch.equal(v[~live], torch.zeros_like(v[~live]))     # ... and its state
    assert err < 1e-6
    assert int(step) == steps
    # the state arrays are torch's, under torch's names (not exp_avg_sq at this bound: Adam's kernel forms 1 - beta2 in fp32, 4.7e-5 off
    # torch's double for 0.999, which the bias correction undoes in the update -- the arithmetic of plain Adam, which may not move a bit)
    state = opt.state[ref]
    for key, buf in (('exp_avg', m), ('square_avg', v), ('grad_avg', m), ('momentum_buffer', m)):
        if state.get(key) is not None:
            assert rel_l2(buf[live].cpu().numpy(), state[key].detach()[live].cpu().numpy()) < 1e-5, key


@pytest.mark.parametrize('name,kw', RULE_CASES, ids=RULE_IDS)
def test_rules_match_torch_optim(pa, emu_lib, name, kw):
    _rule_case(pa, emu_lib, 'cpu', name, kw, 700)


@pytest.mark.gpu
@pytest.mark.parametrize('name,kw', RULE_CASES, ids=RULE_IDS)
def test_rules_match_torch_optim_on_the_gpu(pa, name, kw):
    _rule_case(pa, pa.engine.load_library(), 'cuda', name, kw, 5000)


def _plain_adam_case(pa, lib, device, n):
    """ plain Adam() as torch resolves it (FlatOptimizer.hyper) is `Net.adam_step`'s struct of the bare numbers: the same update, bit for bit
    (both standalone forms) """
    engine = pa.engine
    torch.manual_seed(1)
    net = engine.Net([2, 16, 1], 'tanh', 2, lib=lib)
    optim = _optim_struct(pa, 'Adam', 0.01, {})
    start = torch.randn(n, device=device)
    mask = torch.ones(n, dtype=torch.uint8, device=device)
    mask[::7] = 0
    grads = [torch.randn(n, device=device) for _ in range(20)]
    out = []
    for new in (False, True):
        p, m, v = start.clone(), torch.zeros_like(start), torch.zeros_like(start)
        step = torch.zeros(1, dtype=torch.int32, device=device)
        for k, grad in enumerate(grads):
            at = 0 if k % 2 == 0 else k + 1
            if new:
                net.optim_step(p, grad, m, v, mask, step, optim, at=at)
            else:
                net.adam_step(p, grad, m, v, mask, step, 0.01, at=at)
        out.append((p, m, v, int(step)))
    assert out[0][3] == out[1][3] == 20
    for a, b in zip(out[0][:3], out[1][:3]):
        assert torch.equal(a, b)


def test_plain_adam_through_the_family_is_the_adam_entry_point(pa, emu_lib):
    _plain_adam_case(pa, emu_lib, 'cpu', 700)


@pytest.mark.gpu
def test_plain_adam_through_the_family_is_the_adam_entry_point_on_the_gpu(pa):
    _plain_adam_case(pa, pa.engine.load_library(), 'cuda', 5000)


# ---- 2. Solver.fit against the oracle --------------------------------------------------------------------------------------------------------
def _problem(which, D, V, dtype=torch.float32):
    """ the problems of test_fused_criteria: AFFINE residuals (Poisson box; heat with IC + BC), a residual PROGRAM (Burgers with V('nu')), a
    constraint term -> (equation, solver kwargs, loss_terms) """
    if which == 'poisson':
        eq = lambda u, x, y: D(D(u, x), x) + D(D(u, y), y) - 5.0 * torch.sin(np.pi * (x + y))
        return eq, dict(ndims=2, boundary_condition=1.0, layout='fa fa f', features=[16, 16, 1], activation='Tanh'), 'equation'
    if which == 'heat':
        eq = lambda u, x, t: D(u, t) - 0.1 * D(D(u, x), x) - 2.0 * torch.cos(3.0 * x + t)
        return eq, dict(ndims=2, boundary_condition=0.0, initial_condition=lambda x: torch.sin(np.pi * x), layout='fa fa f',
                        features=[16, 16, 1], activation='Tanh'), 'equation'
    eq = lambda u, x, t: D(u, t) - V('nu', data=torch.Tensor([0.3])) * D(D(u, x), x) + u * D(u, x) - 1.5 * torch.cos(2.0 * x - t)
    kw = dict(ndims=2, boundary_condition=0.0, initial_condition=lambda x: torch.sin(np.pi * x), layout='fafaf', features=[16, 16, 1],
              activation='Tanh')
    if which == 'burgers':
        return eq, kw, 'equation'
    assert which == 'constraint'
    con = lambda f, x, t: f(torch.tensor([0.4], dtype=dtype), torch.tensor([0.6], dtype=dtype)) - 0.2      # (dtype: the fp64 oracle's)
    return eq, dict(kw, constraints=con), ['equation', 'constraint_0']


PROBLEMS = ('poisson', 'heat', 'burgers', 'constraint')
# one optimizer per rule -> (name, keywords, adam_move over the NITERS steps in units of lr: see the module docstring)
RMSPROP_MOVE = sum(sum(0.9 ** j for j in range(k + 1)) / np.sqrt(1 - 0.99) for k in range(NITERS))        # 80.5
FIT_OPTIMIZERS = {'adam_wd': ('Adam', dict(weight_decay=0.01), float(NITERS)), 'adamw': ('AdamW', {}, float(NITERS)),
                  'sgd_nesterov': ('SGD', dict(momentum=0.9, nesterov=True), None),
                  'rmsprop_momentum': ('RMSprop', dict(momentum=0.9), RMSPROP_MOVE)}


def _oracle_run(which, opt, seed, batch, dtype, start=None):
    from oracle import pinn_oracle as po
    name, kw, _ = FIT_OPTIMIZERS[opt]
    eq, skw, terms = _problem(which, po.D, po.V, dtype)
    torch.manual_seed(seed)
    oracle = po.OracleSolver(eq, dtype=dtype, **skw)
    if start is not None:
        oracle.import_params(start)
    pts = np.random.RandomState(1000 + seed).rand(NITERS, batch, 2).astype(np.float32)
    begin = [np.asarray(p, dtype=np.float32) for p in oracle.export_params()]
    oracle.fit(niters=NITERS, batch_size=batch, points=pts, lr=LR, loss_terms=terms, criterion=nn.MSELoss(), optimizer=name, **kw)
    return oracle, pts, begin


def _fit_case(pa, extra, which, opt, batch):
    name, kw, move = FIT_OPTIMIZERS[opt]
    seed = 0
    oracle, pts, start = _oracle_run(which, opt, seed, batch, torch.float32)
    want = np.array([float(v) for v in oracle.losses])
    oracle64 = []

    def fp64():
        if not oracle64:
            oracle64.append(_oracle_run(which, opt, seed, batch, torch.float64, start))
        return oracle64[0]
    eq, skw, terms = _problem(which, pa.D, pa.V)
    for path in ('fused', 'torch'):
        torch.manual_seed(seed)
        solver = pa.Solver(eq, **skw, **extra)
        load_params(solver, start)
        assert solver.optimizer_path == 'torch'                   # the default: opt-in
        if path == 'fused':
            solver.set_optimizer_path('fused')
        solver.fit(niters=NITERS, batch_size=batch, sampler=FixedBatches(pts), lr=LR, loss_terms=terms, criterion=nn.MSELoss(),
                   optimizer=name, **kw)
        assert solver.last_fit_path == 'fused', (solver.program_error, solver.constraint_errors)
        assert solver.last_fit_optimizer == f'{name}/{path}'
        got = np.array([float(v) for v in solver.losses])
        print(f'{which}/{opt}/{path}: loss rel err vs oracle {np.abs(got / want - 1).max():.2e}')
        np.testing.assert_allclose(got, want, rtol=LOSS_RTOL, err_msg=path)
        for i, (p, w) in enumerate(zip(export_params(solver), oracle.export_params())):
            ok, err, arb = close_or_arbitrated(p, w, lambda i=i: fp64()[0].export_params()[i], PARAM_RTOL, atol=3e-7,
                                               adam_move=None if move is None else move * LR)
            print(f'{which}/{opt}/{path}: tensor {i} rel err {err:.2e}{" (fp64 arbiter)" if arb else ""}')
            assert ok, (path, i, err, arb)
        if hasattr(solver.model, 'nu'):
            assert abs(float(solver.model.nu.detach()) - float(oracle.model.nu.detach())) < VAR_ATOL, path


@pytest.mark.parametrize('opt', list(FIT_OPTIMIZERS))
@pytest.mark.parametrize('which', PROBLEMS)
def test_fused_optimizers_follow_the_oracle(pa, emu_lib, which, opt):
    _fit_case(pa, emu_kwargs(emu_lib), which, opt, 40)


@pytest.mark.gpu
@pytest.mark.parametrize('opt', list(FIT_OPTIMIZERS))
@pytest.mark.parametrize('which', PROBLEMS)
def test_fused_optimizers_follow_the_oracle_on_the_gpu(pa, which, opt):
    _fit_case(pa, {}, which, opt, 523)


def _path_case(pa, extra, monkeypatch):
    """ what takes the kernels' rules under 'fused', and that nothing does without the call """
    from pydens_amd.solver import FlatAdam, FlatOptimizer, TorchOptimizerAdapter
    eq, kw, terms = _problem('poisson', pa.D, pa.V)
    pts = np.random.RandomState(3).rand(1, 24, 2).astype(np.float32)
    solver = pa.Solver(eq, **kw, **extra)
    fit = lambda name, **okw: solver.fit(niters=1, batch_size=24, sampler=FixedBatches(pts), lr=LR, optimizer=name, **okw)
    carried = [('Adam', dict(weight_decay=0.01)), ('AdamW', {}), ('SGD', dict(momentum=0.9)), ('RMSprop', dict(centered=True))]
    for name, okw in carried:
        fit(name, **okw)
        assert solver.last_fit_optimizer == f'{name}/torch' and isinstance(solver.optimizer, TorchOptimizerAdapter)
    fit('Adam')
    assert solver.last_fit_optimizer == 'Adam/fused' and type(solver.optimizer) is FlatAdam      # plain Adam: fused under either setting
    solver.set_optimizer_path('fused')
    for name, okw in carried:
        fit(name, **okw)
        assert solver.last_fit_optimizer == f'{name}/fused' and type(solver.optimizer) is FlatOptimizer
    fit('Adam', betas=(0.8, 0.99))
    assert type(solver.optimizer) is FlatAdam and solver.last_fit_optimizer == 'Adam/fused'
    # out of scope: stays on torch.optim
    for name, okw in (('Adam', dict(amsgrad=True)), ('AdamW', dict(maximize=True)), ('SGD', dict(foreach=False)), ('Adagrad', {}),
                      ('RMSprop', dict(momentum=0.9, centered=True)), ('Adam', dict(weight_decay=0.01, capturable=False))):
        fit(name, **okw)
        assert solver.last_fit_optimizer == f'{name}/torch' and isinstance(solver.optimizer, TorchOptimizerAdapter), (name, okw)
    # torch's argument checks raise as torch raises
    for name, okw in (('SGD', dict(nesterov=True)), ('SGD', dict(momentum=0.9, dampening=0.1, nesterov=True)), ('AdamW', dict(weight_decay=-1.0)),
                      ('RMSprop', dict(alpha=-0.5))):
        with pytest.raises(ValueError):
            fit(name, **okw)
    with pytest.raises(ValueError):
        solver.set_optimizer_path('quick')
    monkeypatch.setenv('PYDENS_AMD_OPTIMIZER', 'fused')
    assert pa.Solver(eq, **kw, **extra).optimizer_path == 'fused'


def test_optimizers_take_the_fused_path_when_asked_to(pa, emu_lib, monkeypatch):
    _path_case(pa, emu_kwargs(emu_lib), monkeypatch)


@pytest.mark.gpu
def test_optimizers_take_the_fused_path_on_the_gpu(pa, monkeypatch):
    _path_case(pa, {}, monkeypatch)


# ---- 3. sequences of fit calls -------------------------------------------------------------------------------------------------------------------
def _variable_problem(D, V):
    def odevar(f, x):                               # tutorial cell 50: a trainable V in the equation, a constraint that does not see it
        return D(f, x) - 2 * np.pi * torch.cos(2 * np.pi * x) + V('new_var', data=torch.Tensor([1.0]))
    return odevar, (lambda f, x: f(torch.tensor([0.5])))


def _paired(pa, extra):
    from oracle import pinn_oracle as po
    kw = dict(ndims=1, initial_condition=1, layout='fafaf', features=[12, 10, 1], activation='Tanh')
    eq_o, con_o = _variable_problem(po.D, po.V)
    torch.manual_seed(11)
    oracle = po.OracleSolver(eq_o, constraints=con_o, **kw)
    eq_p, con_p = _variable_problem(pa.D, pa.V)
    solver = pa.Solver(eq_p, constraints=con_p, **kw, **extra)
    load_params(solver, oracle.export_params())
    solver.set_optimizer_path('fused')
    return oracle, solver


class Sequence:
    """ the same fit calls on the oracle and on the solver, compared at the end """
    def __init__(self, pa, extra, lr=0.02, batch=40):
        self.oracle, self.solver = _paired(pa, extra)
        self.pts = np.random.RandomState(8).rand(64, batch, 1).astype(np.float32)
        self.at, self.lr, self.batch = 0, lr, batch

    def fit(self, niters, terms='equation', **kw):
        pts = self.pts[self.at:self.at + niters]
        self.at += niters
        self.oracle.fit(niters=niters, batch_size=self.batch, points=pts, lr=self.lr, loss_terms=terms, **kw)
        self.solver.fit(niters=niters, batch_size=self.batch, sampler=FixedBatches(pts), lr=self.lr, loss_terms=terms, **kw)
        assert self.solver.last_fit_path == 'fused', (self.solver.program_error, self.solver.constraint_errors)

    def freeze(self, frozen):
        self.oracle.model.new_var.requires_grad = not frozen                    # reference freeze_trainable(variables=...)
        (self.solver.model.freeze_trainable if frozen else self.solver.model.unfreeze_trainable)(variables=['new_var'])

    def var(self):
        return float(self.solver.model.new_var.detach()), float(self.oracle.model.new_var.detach())

    def check(self):
        got, want = [float(v) for v in self.solver.losses], [float(v) for v in self.oracle.losses]
        print(f'sequence: loss rel err vs oracle {np.abs(np.array(got) / np.array(want) - 1).max():.2e}, V {self.var()}')
        np.testing.assert_allclose(got, want, rtol=5e-5)
        assert abs(self.var()[0] - self.var()[1]) < VAR_ATOL
        for p, w in zip(export_params(self.solver), self.oracle.export_params()):
            assert params_close(p, w, 5e-5)


def _continue_case(pa, extra):
    """ fit(AdamW) then fit(optimizer=None): state and step count (the bias corrections) continue on the kernels """
    from pydens_amd.solver import FlatOptimizer
    seq = Sequence(pa, extra)
    seq.fit(4, optimizer='AdamW', weight_decay=0.1)
    first = seq.solver.optimizer
    seq.fit(3, optimizer=None)
    assert seq.solver.optimizer is first and type(first) is FlatOptimizer and first.t == 7 and int(first.step_count.item()) == 7
    assert seq.solver.last_fit_optimizer == 'AdamW/fused'
    assert seq.var()[0] != 1.0
    seq.check()
    state = seq.oracle.optimizer.state[seq.oracle.model.new_var]
    off = seq.solver.model.variables['new_var'][0]
    assert abs(float(first.exp_avg[off]) - float(state['exp_avg'])) < 1e-5 * max(1.0, abs(float(state['exp_avg'])))


def _freeze_case(pa, extra):
    """ frozen when the optimizer is built: never a member -- not decayed, not trained by fit(optimizer=None) after unfreezing (reference :420);
    a fresh optimizer takes it in; frozen again under the SAME optimizer: skipped, value and state stay """
    seq = Sequence(pa, extra)
    seq.freeze(True)
    seq.fit(3, optimizer='AdamW', weight_decay=0.1)
    assert seq.var() == (1.0, 1.0)
    seq.freeze(False)
    seq.fit(2, optimizer=None)
    assert seq.var() == (1.0, 1.0)
    seq.fit(3, optimizer='AdamW', weight_decay=0.1)
    moved = seq.var()[0]
    assert moved != 1.0
    seq.freeze(True)
    seq.fit(2, optimizer=None)
    assert seq.var()[0] == moved
    assert seq.solver.last_fit_optimizer == 'AdamW/fused'
    seq.check()


def _unreached_case(pa, extra):
    """ a constraint-only call does not reach the equation's V: torch skips a parameter without a gradient -- no decay (round 6's fuzz caught
    AdamW decaying it); then a call that reaches it makes it LAG (its step count is behind the buffer's): torch's optimizer carries on with
    the kernels' state, the variable without any """
    from pydens_amd.solver import TorchOptimizerAdapter
    for name, kw in (('AdamW', dict(weight_decay=0.1)), ('SGD', dict(momentum=0.9, dampening=0.3, weight_decay=0.1)),
                     ('RMSprop', dict(momentum=0.9, weight_decay=0.1))):
        seq = Sequence(pa, extra)
        seq.fit(3, terms=['constraint_0'], optimizer=name, **kw)
        assert seq.solver.last_fit_optimizer == f'{name}/fused'
        assert seq.var() == (1.0, 1.0), name                               # == its start: not decayed
        flat = seq.solver.optimizer
        seq.fit(3, terms=['equation', 'constraint_0'], optimizer=None)
        assert isinstance(seq.solver.optimizer, TorchOptimizerAdapter) and seq.solver.last_fit_optimizer == f'{name}/torch'
        handed = seq.solver.optimizer.opt
        assert type(handed).__name__ == name and handed.defaults['weight_decay'] == 0.1
        # the network's parameters went over with the kernels' state and step count, the variable with none
        w0 = seq.solver.model.conv_block[0].weight
        first, second = flat.state_keys()
        assert set(handed.state[w0]) == {k for k in (first, second) if k} | (set() if name == 'SGD' else {'step'})
        if name != 'SGD':
            assert float(handed.state[w0]['step']) == 6.0
            steps = handed.state[seq.solver.model.new_var]['step']
            assert float(steps) == 3.0
        assert seq.var()[0] != 1.0
        seq.check()


def _sgd_reuse_case(pa, extra):
    """ SGD(momentum, dampening) sets the momentum buffer to the gradient on step 1 (no 1 - dampening); a reused optimizer is past step 1 """
    seq = Sequence(pa, extra, lr=0.05)
    seq.fit(3, optimizer='SGD', momentum=0.9, dampening=0.3)
    seq.fit(3, optimizer=None)
    seq.fit(2, terms=['equation', 'constraint_0'], optimizer=None)
    opt = seq.solver.optimizer
    assert seq.solver.last_fit_optimizer == 'SGD/fused' and opt.t == 8
    seq.check()
    w0 = seq.solver.model.conv_block[0].weight
    ow0 = next(p for p in seq.oracle.model.parameters() if tuple(p.shape) == tuple(w0.shape))        # (the first layer's weight)
    buf = opt.momentum_buffer.as_strided(tuple(w0.shape), tuple(w0.stride()), w0.storage_offset())
    want = seq.oracle.optimizer.state[ow0]['momentum_buffer']
    assert tuple(buf.shape) == tuple(want.shape) and params_close(buf.cpu().numpy(), want.detach().numpy(), 5e-5, atol=1e-7)


SEQUENCES = {'continue': _continue_case, 'freeze': _freeze_case, 'unreached_then_lagging': _unreached_case, 'sgd_reuse': _sgd_reuse_case}


@pytest.mark.parametrize('which', list(SEQUENCES))
def test_fit_sequences_follow_the_oracle(pa, emu_lib, which):
    SEQUENCES[which](pa, emu_kwargs(emu_lib))


@pytest.mark.gpu
@pytest.mark.parametrize('which', list(SEQUENCES))
def test_fit_sequences_follow_the_oracle_on_the_gpu(pa, which):
    SEQUENCES[which](pa, {})


# ---- 4. chunk forms ----------------------------------------------------------------------------------------------------------------------------------
CHUNK_OPTIMIZERS = {'sgd_momentum': ('SGD', dict(momentum=0.9)), 'adamw': ('AdamW', {})}


def _chunk_run(pa, extra, lib, monkeypatch, opt, niters, graph, persist, eager_loop=False, rounds=None):
    """ cfg1 at batch 100, on-device sampler: fit(optimizer) then fit(optimizer=None) through the chunk entry points """
    name, kw = CHUNK_OPTIMIZERS[opt]
    monkeypatch.setenv('PYDENS_AMD_FIT_GRAPH', '1' if graph else '0')
    monkeypatch.setenv('PYDENS_AMD_FIT_PERSIST', str(persist))
    if rounds is not None:
        monkeypatch.setenv('PYDENS_AMD_FIT_ROUNDS', str(rounds))
    torch.manual_seed(21 if rounds is None else 31)
    cfg, solver = make_solver('cfg1', pa, **extra)
    solver.set_optimizer_path('fused')
    if eager_loop:
        solver._device_columns = lambda sampler: None          # the per-iteration loop (pinn_residual_optim_step)
    st0 = (ctypes.c_int32 * 4)()
    lib.pinn_debug_fit_graph_stats(st0)
    solver.fit(niters=niters[0], batch_size=100, lr=0.005, optimizer=name, **kw)
    solver.fit(niters=niters[1], batch_size=100, lr=0.005, optimizer=None)
    assert solver.last_fit_path == 'fused' and solver.last_fit_optimizer == f'{name}/fused'
    st = (ctypes.c_int32 * 4)()
    lib.pinn_debug_fit_graph_stats(st)
    opt_ = solver.optimizer
    return dict(losses=np.array([float(v) for v in solver.losses]), params=solver.model.flat.detach().cpu().numpy().copy(),
                m=opt_.exp_avg.cpu().numpy().copy(), v=opt_.exp_avg_sq.cpu().numpy().copy(), t=int(opt_.step_count.item()), host_t=opt_.t,
                kernel=lib.pinn_last_kernel_name().decode(), stats=[st[i] - st0[i] for i in range(4)], solver=solver)


def _graph_case(pa, extra, lib, monkeypatch, opt, niters):
    """ the chunks through pinn_fit_steps with a control block (launch graphs on the device; the emulator refuses capture and runs the entry
    point's eager loop) against pinn_fit_steps without one: the same kernels with the same arguments -- every loss, parameter and both state arrays equal """
    a = _chunk_run(pa, extra, lib, monkeypatch, opt, niters, False, 0)
    b = _chunk_run(pa, extra, lib, monkeypatch, opt, niters, True, 0)
    assert a['t'] == b['t'] == a['host_t'] == b['host_t'] == sum(niters)
    assert np.isfinite(b['losses']).all()
    for key in ('losses', 'params', 'm', 'v'):
        assert np.array_equal(a[key], b[key]), key
    if CHUNK_OPTIMIZERS[opt][0] == 'SGD':
        assert b['m'].any() and not b['v'].any()                 # SGD keeps a momentum buffer and nothing else
        assert b['solver'].optimizer.momentum_buffer is b['solver'].optimizer.exp_avg
    # ... and the per-iteration loop (pinn_residual_optim_step) is the same trajectory too
    c = _chunk_run(pa, extra, lib, monkeypatch, opt, niters, False, 0, eager_loop=True)
    for key in ('losses', 'params', 'm', 'v'):
        assert np.array_equal(a[key], c[key]), key
    return b


@pytest.mark.parametrize('opt', list(CHUNK_OPTIMIZERS))
def test_chunk_entry_points_follow_the_eager_loop_bit_for_bit(pa, emu_lib, monkeypatch, opt):
    monkeypatch.setattr(pa.Solver, 'FIT_CTRL_ON_HOST', True)
    _graph_case(pa, emu_kwargs(emu_lib), emu_lib, monkeypatch, opt, (5, 3))


@pytest.mark.gpu
@pytest.mark.parametrize('opt', list(CHUNK_OPTIMIZERS))
def test_fit_chunks_as_launch_graphs_follow_the_eager_loop_bit_for_bit_on_the_gpu(pa, monkeypatch, opt):
    """ 300 iterations = eager chunk + capture, one replay, an eager tail; 260 more with optimizer=None: two replays at once """
    run = _graph_case(pa, {}, pa.engine.load_library(), monkeypatch, opt, (300, 260))
    assert run['t'] == 560
    assert run['stats'][1] >= 1 and run['stats'][0] >= 3, run['stats']
    assert run['kernel'].startswith('pinn_tile_kernel<'), run['kernel']


def _one_cu_case(pa, extra, lib, monkeypatch, opt, niters):
    """ test_emu_engine._one_launch_case with an optimizer: every chunk as ONE launch on one CU (mode 2) against the eager loop """
    a = _chunk_run(pa, extra, lib, monkeypatch, opt, niters, True, 0, rounds=4)
    b = _chunk_run(pa, extra, lib, monkeypatch, opt, niters, True, 2, rounds=4)
    assert a['kernel'].startswith('pinn_tile_kernel<'), a['kernel']
    assert b['kernel'].startswith('pinn_fit_kernel<') and not b['kernel'].endswith(',1>'), b['kernel']
    chunks = sum((n + 127) // 128 for n in niters)
    assert b['stats'][0] >= chunks                    # every chunk went out as one launch
    assert a['t'] == b['t'] == sum(niters) and np.isfinite(b['losses']).all()
    rel = np.abs(b['losses'] / a['losses'] - 1)
    print(f'one-CU chunk against the eager loop ({opt}): loss rel err first 8 {rel[:8].max():.2e}, all {rel.max():.2e}')
    np.testing.assert_allclose(b['losses'][:8], a['losses'][:8], rtol=2e-6)
    np.testing.assert_allclose(b['losses'], a['losses'], rtol=2e-4)
    assert params_close(b['params'], a['params'], 2e-4)
    assert params_close(b['m'], a['m'], 2e-3, atol=1e-7) and params_close(b['v'], a['v'], 2e-3, atol=1e-9)


@pytest.mark.parametrize('opt', list(CHUNK_OPTIMIZERS))
def test_fit_chunk_on_one_cu_follows_the_eager_loop(pa, emu_lib, monkeypatch, opt):
    monkeypatch.setattr(pa.Solver, 'FIT_CTRL_ON_HOST', True)
    _one_cu_case(pa, emu_kwargs(emu_lib), emu_lib, monkeypatch, opt, (5, 3))


@pytest.mark.gpu
@pytest.mark.parametrize('opt', list(CHUNK_OPTIMIZERS))
def test_fit_chunk_on_one_cu_follows_the_eager_loop_on_the_gpu(pa, monkeypatch, opt):
    _one_cu_case(pa, {}, pa.engine.load_library(), monkeypatch, opt, (300, 130))


def _interrupted_case(pa, extra, monkeypatch):
    """ a chunk that stops part way: optimizer.t follows the device's step count, and the next fit(optimizer=None) goes on from there """
    monkeypatch.setenv('PYDENS_AMD_FIT_GRAPH', '0')
    monkeypatch.setenv('PYDENS_AMD_FIT_PERSIST', '0')
    torch.manual_seed(21)
    cfg, solver = make_solver('cfg1', pa, **extra)
    solver.set_optimizer_path('fused')
    solver.fit(niters=4, batch_size=100, lr=0.005, optimizer='SGD', momentum=0.9, dampening=0.3)
    opt = solver.optimizer
    real = solver.model.net.fit_steps

    def stopping(*args, **kw):
        args = list(args)
        args[15] = 3                                            # k_steps: the library applies three of the six iterations ...
        real(*args, **kw)
        raise KeyboardInterrupt                                 # ... and the call does not come back
    monkeypatch.setattr(solver.model.net, 'fit_steps', stopping)
    with pytest.raises(KeyboardInterrupt):
        solver.fit(niters=6, batch_size=100, lr=0.005, optimizer=None)
    assert opt.t == 7 == int(opt.step_count.item())
    monkeypatch.setattr(solver.model.net, 'fit_steps', real)
    solver.fit(niters=2, batch_size=100, lr=0.005, optimizer=None)
    assert opt.t == 9 == int(opt.step_count.item()) and solver.last_fit_optimizer == 'SGD/fused'


def test_interrupted_chunk_leaves_the_step_count_where_the_device_says(pa, emu_lib, monkeypatch):
    _interrupted_case(pa, emu_kwargs(emu_lib), monkeypatch)


@pytest.mark.gpu
def test_interrupted_chunk_leaves_the_step_count_where_the_device_says_on_the_gpu(pa, monkeypatch):
    _interrupted_case(pa, {}, monkeypatch)


# ---- 5. data parallel ------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


DP_OPTIMIZERS = {'sgd_momentum': ('SGD', dict(momentum=0.9)), 'adamw': ('AdamW', {})}


def _dp_problem(pa, lib, opt):
    torch.manual_seed(21)
    eq, kw, terms = _problem('constraint', pa.D, pa.V)
    solver = pa.Solver(eq, **kw, _lib=lib, device='cpu')
    solver.set_optimizer_path('fused')
    rng = np.random.RandomState(3)
    start = [np.asarray(rng.randn(*p.shape) * 0.5, dtype=np.float32) for p in export_params(solver)]
    name, okw = DP_OPTIMIZERS[opt]
    return solver, rng.rand(3, 33, 2).astype(np.float32), dict(lr=0.01, loss_terms=terms, optimizer=name, **okw), start


def _dp_worker(rank, world, port, out_dir, opt):
    sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.join(HERE, 'emu'))
    import torch.distributed as dist
    import build_emu
    import pydens_amd as pa
    from pydens_amd import engine
    torch.set_num_threads(1)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    lib = engine.bind(ctypes.CDLL(build_emu.build()))
    solver, points, fit_kw, start = _dp_problem(pa, lib, opt)
    if rank == 0:
        load_params(solver, start)
    shard = points[:, rank::world]
    solver.fit(niters=points.shape[0], batch_size=points.shape[1], sampler=FixedBatches(shard), **fit_kw)
    assert solver.last_fit_path == 'fused' and solver.last_fit_optimizer.endswith('/fused')
    np.savez(os.path.join(out_dir, f'rank{rank}.npz'), losses=np.array([float(v) for v in solver.losses]),
             nu=float(solver.model.nu.detach()), **{f'p{i}': p for i, p in enumerate(export_params(solver))})
    dist.destroy_process_group()


@pytest.mark.parametrize('opt', list(DP_OPTIMIZERS))
def test_two_ranks_follow_the_single_process(pa, emu_lib, opt):
    """ gloo, world 2, uneven shares (33 points), equation + constraint term: all-reduce, then the standalone update with the loss slot -- as
    tests/test_data_parallel.py, same bounds """
    from oracle import pinn_oracle as po
    single, points, fit_kw, start = _dp_problem(pa, emu_lib, opt)
    load_params(single, start)
    single.fit(niters=points.shape[0], batch_size=points.shape[1], sampler=FixedBatches(points), **fit_kw)
    assert single.last_fit_path == 'fused' and single.last_fit_optimizer.endswith('/fused')
    want_losses, want = np.array([float(v) for v in single.losses]), export_params(single)
    # (the single process itself against the oracle, same optimizer)
    eq, kw, terms = _problem('constraint', po.D, po.V)
    oracle = po.OracleSolver(eq, **kw)
    oracle.import_params(start)
    okw = {k: v for k, v in fit_kw.items() if k != 'loss_terms'}
    oracle.fit(niters=points.shape[0], batch_size=points.shape[1], points=points, loss_terms=terms, **okw)
    np.testing.assert_allclose(want_losses, [float(v) for v in oracle.losses], rtol=LOSS_RTOL)
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_dp_worker, args=(2, _free_port(), tmp, opt), nprocs=2, join=True)
        for rank in range(2):
            z = np.load(os.path.join(tmp, f'rank{rank}.npz'))
            np.testing.assert_allclose(z['losses'], want_losses, rtol=1e-5)
            assert abs(float(z['nu']) - float(single.model.nu.detach())) < 1e-5
            for i, w in enumerate(want):
                assert rel_l2(z[f'p{i}'], w) < 1e-5, (rank, i)


# ---- 6. C-ABI ------------------------------------------------------------------------------------------------------------------------------------------
def _abi_case(pa, lib, device):
    engine = pa.engine
    n = 300
    torch.manual_seed(2)
    start, grad = torch.randn(n, device=device), torch.randn(n, device=device)
    mask = torch.ones(n, dtype=torch.uint8, device=device)
    mask[::5] = 0
    vp = lambda t: ctypes.c_void_p(t.data_ptr())

    def buffers():
        return start.clone(), torch.zeros_like(start), torch.zeros_like(start), torch.zeros(1, dtype=torch.int32, device=device)
    # a zeroed struct with Adam's four numbers is plain Adam: torch.optim.Adam's update, restated here in fp64 on the numbers the struct
    # carries (floats) -- and the same bits as the struct Optim.build makes of those numbers with everything else at its default
    zeroed = engine.Optim()
    assert (zeroed.rule, zeroed.weight_decay, zeroed.momentum, zeroed.dampening, zeroed.alpha, zeroed.nesterov, zeroed.centered) == (0, 0, 0, 0, 0, 0, 0)
    zeroed.lr, zeroed.beta1, zeroed.beta2, zeroed.eps = 0.01, 0.9, 0.999, 1e-8
    built = engine.Optim.build(engine.OPT_ADAM, 0.01, betas=(0.9, 0.999), eps=1e-8)
    p0, m0, v0, s0 = buffers()
    p1, m1, v1, s1 = buffers()
    loss0, loss1 = torch.zeros(1, device=device), torch.zeros(1, device=device)
    live = mask.bool().cpu().numpy()
    g64 = grad.double().cpu().numpy()
    p64, m64, v64 = start.double().cpu().numpy().copy(), np.zeros(n), np.zeros(n)
    lr, b1, b2, eps = float(zeroed.lr), float(zeroed.beta1), float(zeroed.beta2), float(zeroed.eps)
    for step in (1, 2, 3):
        assert lib.pinn_optim_step_at(vp(p0), vp(grad), vp(m0), vp(v0), vp(mask), n, vp(s0), step, ctypes.byref(built), vp(loss0), 7,
                                      engine.stream_of(p0)) == 0
        assert lib.pinn_optim_step_at(vp(p1), vp(grad), vp(m1), vp(v1), vp(mask), n, vp(s1), step, ctypes.byref(zeroed), vp(loss1), 7,
                                      engine.stream_of(p1)) == 0
        m64[live] += (1 - b1) * (g64[live] - m64[live])
        v64[live] = b2 * v64[live] + (1 - b2) * g64[live] ** 2
        p64[live] -= lr / (1 - b1 ** step) * m64[live] / (np.sqrt(v64[live]) / np.sqrt(1 - b2 ** step) + eps)
    assert torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1) and int(s0) == int(s1) == 3
    assert float(loss1) == float(grad[7]) == float(loss0) and not torch.equal(p1, start)
    # (three steps of at most a handful of fp32 roundings each, 6e-8 apiece, on values that do not cancel: the bound of the rule test)
    for got, want in ((p1, p64), (m1, m64), (v1, v64)):
        assert rel_l2(got.cpu().numpy().astype(np.float64), want) < 1e-6
    assert torch.equal(p1[~mask.bool()], start[~mask.bool()]) and not m1[~mask.bool()].any() and not v1[~mask.bool()].any()
    # refusals: non-zero, a message, nothing launched
    build = engine.Optim.build
    bad = [build(4, 0.01), build(-1, 0.01), build(engine.OPT_ADAMW, 0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=-0.01),
           build(engine.OPT_SGD, 0.01, nesterov=True), build(engine.OPT_SGD, 0.01, momentum=0.9, dampening=0.1, nesterov=True),
           build(engine.OPT_RMSPROP, 0.01, eps=1e-8, alpha=0.99, momentum=0.9, centered=True), build(engine.OPT_ADAM, -0.01, betas=(0.9, 0.999)),
           build(engine.OPT_RMSPROP, 0.01, eps=-1.0, alpha=0.99)]
    for optim in bad:
        for at in (0, 1):
            p, m, v, s = buffers()
            if at:
                rc = lib.pinn_optim_step_at(vp(p), vp(grad), vp(m), vp(v), vp(mask), n, vp(s), 1, ctypes.byref(optim), None, 0, engine.stream_of(p))
            else:
                rc = lib.pinn_optim_step(vp(p), vp(grad), vp(m), vp(v), vp(mask), n, vp(s), ctypes.byref(optim), engine.stream_of(p))
            assert rc != 0 and b'optimizer' in lib.pinn_last_error(), (optim.rule, lib.pinn_last_error())
            assert torch.equal(p, start) and not m.any() and not v.any() and int(s) == 0
    assert lib.pinn_optim_step(vp(p0), vp(grad), vp(m0), vp(v0), vp(mask), n, vp(s0), None, engine.stream_of(p0)) != 0
    # ... and through the fused iteration and the chunk: the step is not taken, the buffers stay
    net = engine.Net([2, 16, 16, 1], 'tanh', ndims=2, has_bc=True, bc_value=1.0, lib=lib)
    lay = net.layout
    flat = torch.zeros(lay.p_total, dtype=torch.float32)
    rng = np.random.RandomState(7)
    for w, b in net.param_views(flat):
        w.copy_(torch.as_tensor(rng.randn(*w.shape).astype(np.float32) * 0.5))
        b.copy_(torch.as_tensor(rng.randn(*b.shape).astype(np.float32) * 0.5))
    flat = flat.to(device)
    xs = torch.as_tensor(rng.rand(64, 2).astype(np.float32)).to(device)
    ws = torch.zeros((net.workspace_bytes(64, 2, 2) + 3) // 4, dtype=torch.float32, device=device)
    res = engine.Residual.build(engine.RES_AFFINE, 0, None, coef=[0.0, 0.0, 0.0, 1.0, 1.0], src_const=-0.7)
    fmask = torch.ones(lay.p_total, dtype=torch.uint8, device=device)
    for optim in bad[:3]:
        keep = flat.clone()
        grads, m, v = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros_like(flat)
        step = torch.zeros(1, dtype=torch.int32, device=device)
        history = torch.zeros(4, device=device)
        with pytest.raises(RuntimeError, match='optimizer'):
            net.residual_optim_step(res, flat, xs, grads, ws, m, v, fmask, step, 1, optim, dir_cols=(0, 1), n2=2)
        with pytest.raises(RuntimeError, match='optimizer'):
            net.fit_steps(res, flat, xs, [(0, 0.0, 1.0)] * 2, 5, 0, grads, ws, m, v, fmask, step, 1, optim, history, 4, dir_cols=(0, 1), n2=2)
        assert torch.equal(flat, keep) and not grads.any() and not m.any() and int(step) == 0 and not history.any()
    # a good one: the fused iteration is the plain step followed by the standalone update
    optim = build(engine.OPT_SGD, 0.01, momentum=0.9, weight_decay=0.01)
    a, b = flat.clone(), flat.clone()
    ga, gb = torch.zeros_like(flat), torch.zeros_like(flat)
    ma, va, mb, vb = (torch.zeros_like(flat) for _ in range(4))
    sa, sb = (torch.zeros(1, dtype=torch.int32, device=device) for _ in range(2))
    for step in (1, 2, 3):
        net.residual_optim_step(res, a, xs, ga, ws, ma, va, fmask, sa, step, optim, dir_cols=(0, 1), n2=2)
        net.residual_step(res, b, xs, gb, ws, dir_cols=(0, 1), n2=2)
        net.optim_step(b, gb, mb, vb, fmask, sb, optim, at=step)
    # (two kernels around one expression tree: the bound of the rule test, not bits)
    assert torch.equal(ga, gb) and not torch.equal(a, flat)
    assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < 1e-6 and rel_l2(ma.cpu().numpy(), mb.cpu().numpy()) < 1e-6


def test_optimizer_struct_of_the_abi(pa, emu_lib):
    _abi_case(pa, emu_lib, 'cpu')


@pytest.mark.gpu
def test_optimizer_struct_of_the_abi_on_the_gpu(pa):
    _abi_case(pa, pa.engine.load_library(), 'cuda')
