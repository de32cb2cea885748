""" CPU-side checks of the PRODUCT kernel sources through the real C-ABI, executed by the fiber SIMT emulator
(tests/emu): same pinn_kernel.h / pinn_abi.cpp as libpinn_hip.so, compiled for the host with an emulated
v_mfma_f32_16x16x4_f32, barriers and DPP row sums. What they pin here, without a GPU: tile indexing, lane maps,
the reverse sweep, the residual interpreter, Adam, the Python host (Solver/D/V/tracer) and the data-parallel path.
The product never loads this library (it is injected with the private `_lib=` test hook); the GPU parity tests are in test_gpu_parity.py. """
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import pinn_configs as pc
from conftest import Golden, params_close, rel_l2
from helpers import FixedBatches, export_grads, export_params, fit_rtol, grad_close, load_params, make_solver

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))


@pytest.fixture(scope='session')
def emu_lib():
    import build_emu
    from pydens_amd import engine
    lib = engine.bind(ctypes.CDLL(build_emu.build()))
    assert lib.pinn_backend() == b'emu-host'
    return lib


@pytest.fixture(scope='session')
def pa():
    import pydens_amd
    return pydens_amd


def emu_kwargs(lib):
    return dict(_lib=lib, device='cpu')


@pytest.mark.parametrize('name', ['cfg1', 'cfg2', 'cfg3', 'cfg4', 'ode_sigmoid', 'mixed', 'heat3d', 'kdv', 'resnet3'])
def test_fused_fit_matches_reference_golden(pa, emu_lib, name):
    g = Golden(name)
    _, solver = make_solver(name, pa, **emu_kwargs(emu_lib))
    load_params(solver, g.params)
    pts = g.points
    pred = solver.predict(*[pts[1][:, i] for i in range(pts.shape[2])])
    assert np.abs(pred[:, 0] - g.predict).max() <= 1e-5 * max(1.0, np.abs(g.predict).max())
    assert solver.program is not None, solver.program_error
    niters = 2 if name == 'cfg3' else len(g.losses)        # 8-wave / 128-wide emulation is slow: two steps suffice
    solver.fit(niters=niters, batch_size=pts.shape[1], sampler=FixedBatches(pts), lr=g.lr)
    assert solver.last_fit_path == 'fused'
    # the BASELINE shapes take a shape-specialised instantiation (PinnShape 1: Poisson, 2: heat, 3: ODE family), the
    # 32-wide sigmoid net and the mixed-partial operator (a diagonal direction) the general one
    assert emu_lib.pinn_debug_last_kernel() == (2 if name in ('cfg1', 'cfg2', 'cfg3', 'cfg4') else 0)
    np.testing.assert_allclose(np.array([float(v) for v in solver.losses]), g.losses[:niters], rtol=fit_rtol(name))
    if niters == len(g.losses):
        for got, want in zip(export_params(solver), g.finals):
            assert rel_l2(got, want) < fit_rtol(name)


@pytest.mark.parametrize('name', ['cfg1', 'ode_sigmoid', 'mixed', 'heat3d', 'kdv', 'resnet3'])
def test_generic_fit_matches_reference_golden(pa, emu_lib, name):
    g = Golden(name)
    _, solver = make_solver(name, pa, **emu_kwargs(emu_lib))
    load_params(solver, g.params)
    solver.program = None                           # force: kernel streams -> user's torch code -> kernel backward
    solver.fit(niters=len(g.losses), batch_size=g.points.shape[1], sampler=FixedBatches(g.points), lr=g.lr)
    assert solver.last_fit_path == 'generic'
    np.testing.assert_allclose(np.array([float(v) for v in solver.losses]), g.losses, rtol=fit_rtol(name))
    for got, want in zip(export_params(solver), g.finals):
        assert rel_l2(got, want) < fit_rtol(name)


@pytest.mark.parametrize('name', ['cfg1', 'cfg4', 'mixed'])
def test_gradients_match_reference_golden(pa, emu_lib, name):
    g = Golden(name)
    _, solver = make_solver(name, pa, **emu_kwargs(emu_lib))
    load_params(solver, g.params)
    solver._fused_step(torch.from_numpy(g.points[0].copy()), 1)
    lay = solver.model.net.layout
    assert abs(float(solver.grads[lay.off_loss]) - g.loss0) <= 1e-5 * g.loss0
    for got, want in zip(export_grads(solver), g.grads):
        if want is None:
            assert float(np.abs(got).max()) == 0.0
        else:
            assert grad_close(got, want)


@pytest.mark.parametrize('n', [1, 15, 17, 50])
def test_ragged_tiles(pa, emu_lib, n):
    g = Golden('cfg1')
    cfg, solver = make_solver('cfg1', pa, **emu_kwargs(emu_lib))
    load_params(solver, g.params)
    pts = pc.sample_points(cfg, 64, seed=9)
    full = solver.predict(pts[:, 0], pts[:, 1])
    part = solver.predict(pts[:n, 0], pts[:n, 1])
    assert np.array_equal(full[:n], part)
    xs = torch.from_numpy(pts[:n].copy())
    solver._fused_step(xs, 1)
    lay = solver.model.net.layout
    streams = solver.model.net.jet_forward(solver.model.flat, xs, [0, 1], 2)
    r = streams[3] + streams[4] - 5 * torch.sin(np.pi * (xs[:, 0] + xs[:, 1]))
    assert abs(float(solver.grads[lay.off_loss]) - float((r * r).mean())) <= 2e-6 * float((r * r).mean())


def test_streams_match_fp64_jets(pa, emu_lib):
    from oracle import jet_f64 as jf, problems
    from test_oracle_vs_golden import make_spec
    g = Golden('cfg3')
    _, solver = make_solver('cfg3', pa, **emu_kwargs(emu_lib))
    load_params(solver, g.params)
    sf, spec = make_spec(g)
    pts = g.points[0][:48]
    ic64 = problems.ic_streams_f64('cfg3', pts, sf['dir_cols'], sf['n2'])
    out = jf.step(spec, pts, sf['residual'], ic64)
    streams = solver.model.net.jet_forward(solver.model.flat, torch.from_numpy(pts.copy()), sf['dir_cols'], sf['n2'],
                                           ic_streams=torch.from_numpy(ic64.astype(np.float32)).contiguous())
    for s in range(spec.S):
        assert rel_l2(streams[s].numpy(), out['u_streams'][s]) < 2e-5, s


def test_sharded_sum_equals_whole(pa, emu_lib):
    g = Golden('cfg4')
    cfg, solver = make_solver('cfg4', pa, **emu_kwargs(emu_lib))
    load_params(solver, g.params)
    pts = torch.from_numpy(pc.sample_points(cfg, 96, seed=4))
    solver._fused_step(pts, 1)
    whole = solver.grads.clone()
    acc = torch.zeros_like(whole)
    for shard in pts.chunk(3):
        solver._fused_step(shard.contiguous(), 3)
        acc += solver.grads
    assert rel_l2(acc.numpy(), whole.numpy()) < 1e-5


def test_adam_matches_torch(emu_lib):
    from pydens_amd import engine
    torch.manual_seed(0)
    n = 700
    p = torch.randn(n); ref = p.clone().requires_grad_()
    opt = torch.optim.Adam([ref], lr=0.01)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step = torch.zeros(1, dtype=torch.int32)
    mask = torch.ones(n, dtype=torch.uint8); mask[::7] = 0
    keep = p.clone()
    net = engine.Net([2, 16, 1], 'tanh', 2, lib=emu_lib)
    for k in range(12):
        grad = torch.randn(n)
        ref.grad = grad.clone()
        opt.step()
        # odd steps: the count lives on the device (two launches); even steps: the host passes it (one launch)
        net.adam_step(p, grad, m, v, mask, step, 0.01, at=0 if k % 2 == 0 else k + 1)
    live = mask.bool()
    assert torch.equal(p[~live], keep[~live])
    assert rel_l2(p[live].numpy(), ref.detach()[live].numpy()) < 1e-6
    assert int(step) == 12


# ---- reference API beyond the plain equation: trainable V, constraints, freezing, other optimizers -----------------------
def _variable_problem(D, V, torch):
    def odevar(f, x):                               # tutorial cell 50
        return D(f, x) - 2 * np.pi * torch.cos(2 * np.pi * x) + V('new_var', data=torch.Tensor([1.0]))
    return odevar, (lambda f, x: f(torch.tensor([0.5])))


def _paired(pa, emu_lib, **fit_kwargs):
    """ oracle + product solver for the tutorial's trainable-variable problem; emu_lib=None -> the HIP library """
    from oracle import pinn_oracle as po
    kw = dict(ndims=1, initial_condition=1, layout='fafaf', features=[12, 10, 1], activation='Tanh')
    eq_o, con_o = _variable_problem(po.D, po.V, torch)
    oracle = po.OracleSolver(eq_o, constraints=con_o, **kw)
    eq_p, con_p = _variable_problem(pa.D, pa.V, torch)
    solver = pa.Solver(eq_p, constraints=con_p, **kw, **(emu_kwargs(emu_lib) if emu_lib is not None else {}))
    load_params(solver, oracle.export_params())
    return oracle, solver


def test_trainable_variable_and_constraint_follow_the_reference(pa, emu_lib):
    oracle, solver = _paired(pa, emu_lib)
    assert solver.program is not None and solver.residual_plan.n_vars == 1    # V('new_var') is a program register
    pts = np.random.RandomState(3).rand(6, 40, 1).astype(np.float32)
    terms = ['equation', 'constraint_0']
    solver.use_fused = False                        # this test pins the GENERIC path (the fused form: next test)
    oracle.fit(niters=6, batch_size=40, points=pts, lr=0.05, loss_terms=terms)
    solver.fit(niters=6, batch_size=40, sampler=FixedBatches(pts), lr=0.05, loss_terms=terms)
    assert solver.last_fit_path == 'generic'
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=5e-5)
    assert abs(float(solver.model.new_var) - float(oracle.model.new_var)) < 1e-5
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 5e-5)


def test_constraint_terms_as_residual_programs(pa, emu_lib):
    """ loss_terms with constraints (reference :451-457) on the fused path: the constraint is traced to a program over the
    value stream on its own fixed points and ADDS gradient + loss to the equation's (pinn_residual_step_add) """
    oracle, solver = _paired(pa, emu_lib)
    assert solver.constraint_plans[0] is not None, solver.constraint_errors
    assert solver.constraint_plans[0]['points'].shape == (1, 1)
    pts = np.random.RandomState(8).rand(9, 40, 1).astype(np.float32)
    for terms, lo in ((['equation', 'constraint_0'], 0), (['constraint_0'], 3), ('equation', 6)):
        oracle.fit(niters=3, batch_size=40, points=pts[lo:lo + 3], lr=0.05, loss_terms=terms)
        solver.fit(niters=3, batch_size=40, sampler=FixedBatches(pts[lo:lo + 3]), lr=0.05, loss_terms=terms)
        assert solver.last_fit_path == 'fused'
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=5e-5)
    assert abs(float(solver.model.new_var) - float(oracle.model.new_var.detach())) < 1e-5
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 5e-5)

    # several points, a variable inside the constraint, a callable initial condition
    from oracle import pinn_oracle as po

    def problem(D, V):
        def eq(u, x, t):
            return D(u, t) - 0.3 * D(D(u, x), x)
        def con(f, x, t):
            return f(np.array([0.25, 0.5, 0.75]), 0.5) - V('level', data=torch.Tensor([0.4])) * 2.0
        return eq, con
    kw = dict(ndims=2, initial_condition=lambda x: torch.sin(np.pi * x), boundary_condition=0.0, layout='fafaf',
              features=[16, 16, 1], activation='Tanh')
    eq_o, con_o = problem(po.D, po.V)
    eq_p, con_p = problem(pa.D, pa.V)
    oracle = po.OracleSolver(eq_o, constraints=con_o, **kw)
    solver = pa.Solver(eq_p, constraints=con_p, **kw, **emu_kwargs(emu_lib))
    load_params(solver, oracle.export_params())
    cp = solver.constraint_plans[0]
    assert cp is not None and cp['points'].shape == (3, 2) and cp['plan'].n_vars == 1 and cp['ic'] is not None
    pts = np.random.RandomState(9).rand(7, 33, 2).astype(np.float32)
    terms = ['equation', 'constraint_0']
    # a variable that lives only in a constraint is born in the reference's first iteration that evaluates the constraint
    # (:457), after that fit call built its optimizer (:420): the first call leaves it alone, the next one trains it
    oracle.fit(niters=4, batch_size=33, points=pts[:4], lr=0.02, loss_terms=terms)
    solver.fit(niters=4, batch_size=33, sampler=FixedBatches(pts[:4]), lr=0.02, loss_terms=terms)
    assert solver.last_fit_path == 'fused'
    assert float(solver.model.level) == float(oracle.model.level.detach()) == float(np.float32(0.4))
    oracle.fit(niters=3, batch_size=33, points=pts[4:], lr=0.02, loss_terms=terms)
    solver.fit(niters=3, batch_size=33, sampler=FixedBatches(pts[4:]), lr=0.02, loss_terms=terms)
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=5e-5)
    assert abs(float(solver.model.level) - float(oracle.model.level.detach())) < 1e-5
    assert float(solver.model.level) != float(np.float32(0.4))
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 5e-5)
    # a constraint on the batch points cannot be lowered and says why
    other = pa.Solver(eq_p, constraints=lambda f, x, t: f(x, 0.0), **kw, **emu_kwargs(emu_lib))
    assert other.constraint_plans[0] is None and 'batch points' in other.constraint_errors[0]


def test_trainable_variable_on_the_fused_path(pa, emu_lib):
    """ equation-only loss: the scalar V(...) is a register of the residual program, its gradient comes out of the tile
    kernel (user slot of the flat gradient buffer) and Adam updates it with the network. """
    oracle, solver = _paired(pa, emu_lib)
    pts = np.random.RandomState(5).rand(6, 40, 1).astype(np.float32)
    oracle.fit(niters=6, batch_size=40, points=pts, lr=0.05)
    solver.fit(niters=6, batch_size=40, sampler=FixedBatches(pts), lr=0.05)
    assert solver.last_fit_path == 'fused'
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=5e-5)
    assert float(solver.model.new_var) != 1.0
    assert abs(float(solver.model.new_var) - float(oracle.model.new_var)) < 1e-5
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 5e-5)


def _inverse_problem(D, V, torch):
    def heat_with_unknowns(u, x, t):                # tutorial-style inverse problem: diffusivity and source scale are trainable
        a = V('diffusivity', data=torch.Tensor([0.7]))
        q = V('source', data=torch.Tensor([1.3]))
        return D(u, t) - a * D(D(u, x), x) - q * torch.sin(np.pi * x) * torch.exp(-t) + 0.1 * a * q * u * u
    return heat_with_unknowns


def test_two_trainable_coefficients_in_a_nonlinear_program(pa, emu_lib):
    from oracle import pinn_oracle as po
    kw = dict(ndims=2, initial_condition=lambda x: torch.sin(np.pi * x), boundary_condition=0.0, layout='fafaf',
              features=[16, 16, 1], activation='Tanh')
    oracle = po.OracleSolver(_inverse_problem(po.D, po.V, torch), **kw)
    solver = pa.Solver(_inverse_problem(pa.D, pa.V, torch), **kw, **emu_kwargs(emu_lib))
    load_params(solver, oracle.export_params())
    plan = solver.residual_plan
    assert solver.program is not None, solver.program_error
    assert plan.n_vars == 2 and plan.n_aux >= 1
    pts = np.random.RandomState(6).rand(5, 48, 2).astype(np.float32)
    oracle.fit(niters=5, batch_size=48, points=pts, lr=0.02)
    solver.fit(niters=5, batch_size=48, sampler=FixedBatches(pts), lr=0.02)
    assert solver.last_fit_path == 'fused'
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=5e-5)
    for name in ('diffusivity', 'source'):
        assert abs(float(getattr(solver.model, name)) - float(getattr(oracle.model, name))) < 2e-5
    assert float(solver.model.diffusivity) != float(np.float32(0.7))
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 5e-5)


def test_freeze_and_unfreeze(pa, emu_lib):
    oracle, solver = _paired(pa, emu_lib)
    pts = np.random.RandomState(4).rand(4, 32, 1).astype(np.float32)
    oracle.model.new_var.requires_grad = False                           # reference freeze_trainable(variables=...)
    solver.model.freeze_trainable(variables=('new_var',))
    oracle.fit(niters=2, batch_size=32, points=pts[:2], lr=0.1)
    solver.fit(niters=2, batch_size=32, sampler=FixedBatches(pts[:2]), lr=0.1)
    assert float(solver.model.new_var) == 1.0
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=5e-5)
    oracle.model.new_var.requires_grad = True
    solver.model.unfreeze_trainable(variables=['new_var'])
    oracle.fit(niters=2, batch_size=32, points=pts[2:], lr=0.1)
    solver.fit(niters=2, batch_size=32, sampler=FixedBatches(pts[2:]), lr=0.1)
    assert float(solver.model.new_var) != 1.0
    assert abs(float(solver.model.new_var) - float(oracle.model.new_var)) < 2e-5
    solver.model.freeze_trainable(layers=['conv_block'])
    before = [p.copy() for p in export_params(solver)]
    solver.fit(niters=1, batch_size=32, sampler=FixedBatches(pts[:1]), lr=0.1)
    for a, b in zip(before[:-1], export_params(solver)[:-1]):
        assert np.array_equal(a, b)


def test_other_torch_optimizer_by_name(pa, emu_lib):
    from oracle import pinn_oracle as po
    g = Golden('cfg1')
    cfg, solver = make_solver('cfg1', pa, **emu_kwargs(emu_lib))
    load_params(solver, g.params)
    ocfg = pc.make_config('cfg1', po.D, torch)
    oracle = po.OracleSolver(ocfg['equation'], **ocfg['solver_kwargs'])
    oracle.import_params(g.params)
    oracle.fit(niters=3, batch_size=100, points=g.points[:3], optimizer='SGD', lr=1e-3, momentum=0.9)
    solver.fit(niters=3, batch_size=100, sampler=FixedBatches(g.points[:3]), optimizer='SGD', lr=1e-3, momentum=0.9)
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 2e-5)
    # optimizer=None keeps the existing optimizer (reference model_torch.py:392-393)
    solver.fit(niters=1, batch_size=100, sampler=FixedBatches(g.points[3:4]), optimizer=None)
    oracle.fit(niters=1, batch_size=100, points=g.points[3:4], optimizer=None)
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 2e-5)


@pytest.mark.parametrize('form', ['variable_fused', 'variable_generic', 'expression'])
def test_callable_ic_with_variable(pa, emu_lib, form):
    """ README.md:111-118: the initial condition itself is a trainable V(...). A bare scalar variable rides in the kernels
    (pinn_residual_t::ic_var1: value read from its user slot, gradient = sum of d(loss)/du returned there), also through
    the constraint term; an expression of variables needs torch autograd and keeps the generic path. """
    from oracle import pinn_oracle as po

    def problem(D, V):
        ic = (lambda *a: V('init', data=torch.Tensor([3.0]))) if form != 'expression' else \
            (lambda *a: 1.5 * V('init', data=torch.Tensor([2.0])))
        return (lambda u, t: D(u, t) - 2 * np.pi * torch.cos(2 * np.pi * t)), ic
    kw = dict(ndims=1, layout='fafaf', features=[8, 8, 1], activation='Tanh')
    eq_o, ic_o = problem(po.D, po.V)
    oracle = po.OracleSolver(eq_o, initial_condition=ic_o, constraints=lambda u, t: u(torch.tensor([0.5])), **kw)
    eq_p, ic_p = problem(pa.D, pa.V)
    solver = pa.Solver(eq_p, initial_condition=ic_p, constraints=lambda u, t: u(torch.tensor([0.5])), **kw,
                       **emu_kwargs(emu_lib))
    load_params(solver, oracle.export_params())
    if form == 'expression':
        assert solver.ic_trainable and solver.ic_var_slot is None
    else:
        assert not solver.ic_trainable and solver.ic_var_slot == 0 and solver.constraint_plans[0] is not None
        solver.use_fused = form == 'variable_fused'
    pts = np.random.RandomState(5).rand(8, 24, 1).astype(np.float32)
    terms = ('equation', 'constraint_0')
    oracle.fit(niters=5, batch_size=24, points=pts[:5], lr=0.05, loss_terms=terms)
    solver.fit(niters=5, batch_size=24, sampler=FixedBatches(pts[:5]), lr=0.05, loss_terms=terms)
    assert solver.last_fit_path == ('fused' if form == 'variable_fused' else 'generic')
    oracle.fit(niters=3, batch_size=24, points=pts[5:], lr=0.05)
    solver.fit(niters=3, batch_size=24, sampler=FixedBatches(pts[5:]), lr=0.05)
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=5e-5)
    assert abs(float(solver.model.init) - float(oracle.model.init)) < 2e-5
    assert float(solver.model.init) not in (2.0, 3.0)
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 5e-5)
    xs = np.linspace(0, 1, 7).astype(np.float32)
    assert np.abs(solver.predict(xs) - oracle.predict(xs)).max() < 2e-5


def _nonlinear_problem(D, torch):
    def burgers(f, x, t):                            # nonlinear in the field: lowered to a residual PROGRAM
        return D(f, t) + f * D(f, x) - 0.05 * D(D(f, x), x) - torch.sin(np.pi * x) * torch.exp(-t)
    return burgers, dict(ndims=2, boundary_condition=0, initial_condition=lambda x: torch.sin(np.pi * x),
                         layout='fafaf', features=[16, 16, 1], activation='Tanh')


def _variable_coefficient_problem(D, torch):
    def eq(f, x, y):                                 # affine with x-dependent coefficients: pre-pass rows
        return (1 + x * y) * D(D(f, x), x) + torch.exp(-x) * D(D(f, y), y) + torch.cos(y) * D(f, x) - 3 * f - x * torch.sin(y)
    return eq, dict(ndims=2, boundary_condition=0.5, layout='fafaf', features=[16, 16, 1], activation='Sigmoid')


def _mixed_affine_problem(D, torch):
    def eq(f, x, y):                                 # mixed partial: one extra diagonal direction e_x + e_y
        return D(D(f, x), x) + D(D(f, x), y) + 2 * D(D(f, y), y) + 0.5 * D(f, y) - torch.sin(3 * x * y)
    return eq, dict(ndims=2, boundary_condition=0.5, layout='fafaf', features=[16, 16, 1], activation='Tanh')


def _D_of_a_mixed_partial_problem(D, torch):
    def eq(f, x, y):                                 # D of an EXPRESSION that holds a mixed partial (which the solver builds from u_vv, u_xx, u_yy)
        return D(f * D(D(f, x), y), x) + D(D(f, y), y) - torch.sin(3 * x * y)
    return eq, dict(ndims=2, boundary_condition=0.5, layout='fafaf', features=[16, 16, 1], activation='Tanh')


def _mixed_nonlinear_problem(D, torch):
    def eq(f, x, t):                                 # mixed space-time partial under a callable IC, nonlinear in f
        return D(f, t) + f * D(D(f, x), t) - 0.1 * D(D(f, x), x) - x * t
    return eq, dict(ndims=2, boundary_condition=0, initial_condition=lambda x: torch.sin(np.pi * x),
                    layout='fafaf', features=[16, 16, 1], activation='Tanh')


def _divergence_form_problem(D, torch):
    def eq(f, x, y):                                 # D of composite expressions: div(a(x) grad u), still affine in u
        return D((1 + x * y) * D(f, x), x) + D(torch.exp(-x) * D(f, y), y) - x * torch.sin(y)
    return eq, dict(ndims=2, boundary_condition=0.5, layout='fafaf', features=[16, 16, 1], activation='Tanh')


def _conservative_burgers_problem(D, torch):
    def eq(f, x, t):                                 # D(f * f, x): chain rule through a product containing the field
        return D(f, t) + 0.5 * D(f * f, x) - 0.05 * D(D(f, x), x) + D(torch.sin(f), x) * x
    return eq, dict(ndims=2, boundary_condition=0, initial_condition=lambda x: torch.sin(np.pi * x),
                    layout='fafaf', features=[16, 16, 1], activation='Tanh')


@pytest.mark.parametrize('problem,kind', [(_nonlinear_problem, 0), (_variable_coefficient_problem, 1),
                                          (_mixed_affine_problem, 1), (_mixed_nonlinear_problem, 0),
                                          (_divergence_form_problem, 1), (_conservative_burgers_problem, 0)])
def test_residual_kinds_match_the_oracle(pa, emu_lib, problem, kind):
    from oracle import pinn_oracle as po
    eq_o, kw = problem(po.D, torch)
    oracle = po.OracleSolver(eq_o, **kw)
    eq_p, kw = problem(pa.D, torch)
    solver = pa.Solver(eq_p, **kw, **emu_kwargs(emu_lib))
    assert solver.program is not None and solver.residual_plan.kind == kind, solver.program_error
    load_params(solver, oracle.export_params())
    pts = np.random.RandomState(8).rand(4, 50, 2).astype(np.float32)
    oracle.fit(niters=4, batch_size=50, points=pts, lr=0.01)
    solver.fit(niters=4, batch_size=50, sampler=FixedBatches(pts), lr=0.01)
    assert solver.last_fit_path == 'fused'
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=3e-5)
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 3e-5)


@pytest.mark.parametrize('problem', ['mixed', 'composite', 'D_of_mixed'])
def test_mixed_partial_and_composite_D_generic_path(pa, emu_lib, problem):
    """ generic path (kernel streams -> the user's torch code -> kernel backward): D(D(f, x), y) seen as
    u_xy = (u_vv - u_xx - u_yy) / 2 built from the streams; D(f * f, x) by the chain rule over the streams; `D_of_mixed` (round 6):
    D of an expression that holds u_xy -- the chain rule takes d expr / d stream for every tagged stream by autograd, so u_xy must
    not hang below the tagged u_xx / u_yy in the graph (it did: d / d u_xx then counted the path through u_xy a second time) """
    _generic_D_case(pa, problem, emu_kwargs(emu_lib))


def _generic_D_case(pa, problem, solver_kwargs):
    from oracle import pinn_oracle as po
    make = {'mixed': _mixed_affine_problem, 'composite': _conservative_burgers_problem, 'D_of_mixed': _D_of_a_mixed_partial_problem}[problem]
    eq_o, kw = make(po.D, torch)
    oracle = po.OracleSolver(eq_o, **kw)
    eq_p, kw = make(pa.D, torch)
    solver = pa.Solver(eq_p, **kw, **solver_kwargs)
    solver.program = None
    load_params(solver, oracle.export_params())
    pts = np.random.RandomState(9).rand(3, 40, 2).astype(np.float32)
    oracle.fit(niters=3, batch_size=40, points=pts, lr=0.01)
    solver.fit(niters=3, batch_size=40, sampler=FixedBatches(pts), lr=0.01)
    assert solver.last_fit_path == 'generic'
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=3e-5)
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 3e-5)


LAYOUTS = {
    # docstring example of the reference (model_torch.py:155): skip over two hidden layers
    'skip': dict(layout='faR fa fa+ f', features=[16, 12, 16, 1], activation='Tanh'),
    # two skips back to back ('+' output is the next 'R' input), per-layer activations incl. Sin
    'two_skips': dict(layout='fa R fa + R fa fa + f', features=[16, 16, 16, 16, 1],
                      activation=['Tanh', 'Sin', 'Sigmoid', 'Tanh']),
    'sin': dict(layout='fa fa f', features=[16, 16, 1], activation='Sin'),
    # a hidden dense layer without activation
    'identity': dict(layout='fa f fa f', features=[16, 16, 16, 1], activation='Tanh'),
    'skip_to_top_wide': dict(layout='fa R fa fa + f', features=[40, 40, 40, 1], activation='Sigmoid'),
    # smooth activations whose derivatives are functions of the pre-activation (kept in the slab instead of the value)
    'softplus_silu_gelu': dict(layout='fa fa fa f', features=[12, 16, 12, 1], activation=['Softplus', 'SiLU', 'GELU']),
    # every unit of a 64-wide net real (no zero padding to hide a wrong lane / K quad)
    'full64': dict(layout='fa R fa fa + f', features=[64, 64, 64, 1], activation=['Sin', 'Tanh', 'Sigmoid']),
    # the usual residual block act(W h + skip): '+' between the dense layer and its activation (PINN_SKIP_PRE); two blocks, the
    # second one starting where the first ends, and one joining in front of an identity
    'pre_activation_blocks': dict(layout='fa R fa f+a R fa f+a f', features=[16, 16, 16, 16, 16, 1],
                                  activation=['Tanh', 'Sin', 'Tanh', 'SiLU', 'Sigmoid']),
    'pre_activation_mixed': dict(layout='faR f+a R fa fa+ f', features=[24, 24, 24, 24, 1], activation='Tanh'),
    # skips that START in front of an activation: z to z (the pre-activation ResNet block), from the first layer, and z to act(z)
    'skip_from_pre_activation': dict(layout='fRa fa f+a fRa fa+ f', features=[20, 20, 20, 20, 20, 1],
                                     activation=['Tanh', 'Sigmoid', 'Tanh', 'Sin', 'Tanh']),
    'pre_blocks_back_to_back': dict(layout='fa fRa f+Ra fa f+a f', features=[16, 16, 16, 16, 16, 1], activation='Tanh'),
    # round 5: NESTED skips ('+' closes the most recent 'R'): the outer skip's jets wait in its slab slot, the inner one rides in
    # registers; one nest of post-activation skips, one where the outer skip carries pre-activation jets into a pre-activation join
    'nested_skips': dict(layout='fa R fa R fa fa + fa + f', features=[16, 16, 16, 16, 16, 1], activation=['Tanh', 'Sigmoid', 'Tanh', 'Sin', 'Tanh']),
    'nested_pre_activation': dict(layout='fRa faR fa fa+ f+a f', features=[20, 20, 20, 20, 20, 1], activation=['Tanh', 'Tanh', 'SiLU', 'Tanh', 'Sigmoid']),
    # round 5: the rest of the activations `getattr(nn, name)()` commonly names, torch-default forms (include/pinn.h PINN_ACT_RELU ..)
    'relu_family': dict(layout='fa fa fa fa f', features=[16, 12, 16, 12, 1], activation=['ELU', 'LeakyReLU', 'SELU', 'ReLU']),
    'softsign_gelutanh_mish': dict(layout='fa fa fa f', features=[12, 16, 12, 1], activation=['Softsign', torch.nn.GELU(approximate='tanh'), 'Mish']),
    'shrink_logsigmoid': dict(layout='fa fa fa f', features=[12, 16, 12, 1], activation=[torch.nn.Tanhshrink, 'LogSigmoid', torch.nn.functional.mish]),
}


def _layout_problems(D, torch, which, net):
    if which == 'poisson':                           # combined second-order stream
        eq = lambda f, x, y: D(D(f, x), x) + D(D(f, y), y) - 5 * torch.sin(np.pi * (x + y))
        return eq, dict(ndims=2, boundary_condition=1, **net)
    eq = lambda f, x, t: D(f, t) + f * D(f, x) - 0.05 * D(D(f, x), x)      # residual program, IC + BC
    return eq, dict(ndims=2, boundary_condition=0, initial_condition=lambda x: torch.sin(np.pi * x), **net)


@pytest.mark.parametrize('net', sorted(LAYOUTS))
@pytest.mark.parametrize('which', ['poisson', 'burgers'])
def test_layout_breadth_matches_the_oracle(pa, emu_lib, net, which):
    """ skip connections 'R ... +', per-layer activation lists, Sin and activation-free dense layers (reference
    model_torch.py:142-156) against the oracle's nested autograd: fused step, generic step and predict """
    from oracle import pinn_oracle as po
    if net in ('skip_to_top_wide', 'full64') and which == 'burgers':
        pytest.skip('one case per wide net is enough for the emulator')
    eq_o, kw = _layout_problems(po.D, torch, which, LAYOUTS[net])
    oracle = po.OracleSolver(eq_o, **kw)
    eq_p, kw = _layout_problems(pa.D, torch, which, LAYOUTS[net])
    pts = np.random.RandomState(10).rand(3, 40, 2).astype(np.float32)
    oracle_start = oracle.export_params()
    oracle.fit(niters=3, batch_size=40, points=pts, lr=0.01)
    for path in ('fused', 'generic'):
        solver = pa.Solver(eq_p, **kw, **emu_kwargs(emu_lib))
        assert solver.program is not None, solver.program_error
        if path == 'generic':
            solver.program = None
        load_params(solver, oracle_start)
        solver.fit(niters=3, batch_size=40, sampler=FixedBatches(pts), lr=0.01)
        assert solver.last_fit_path == path
        np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=3e-5)
        for got, want in zip(export_params(solver), oracle.export_params()):
            assert params_close(got, want, 3e-5)
    xs = [pts[0][:, i] for i in range(2)]
    assert np.abs(solver.predict(*xs) - oracle.predict(*xs)).max() < 2e-5


def test_layout_errors_are_loud(pa, emu_lib):
    for layout, features, exc in [('fa R fa f', [8, 8, 1], ValueError),                   # unclosed skip
                                  ('fa R fa + f', [8, 12, 1], ValueError),                # widths differ
                                  ('fa R fa R fa + + f', [8, 8, 8, 1], NotImplementedError),   # nested
                                  ('R fa fa + f', [8, 8, 1], NotImplementedError),        # skip from the inputs
                                  ('fa fRa +fa f', [8, 8, 8, 1], NotImplementedError),     # '+' without a layer in between
                                  ('ca f', [8, 1], NotImplementedError)]:
        with pytest.raises(exc):
            pa.Solver(lambda f, x: pa.D(f, x), ndims=1, layout=layout, features=features, **emu_kwargs(emu_lib))


@pytest.mark.parametrize('depth', [8, 20])
def test_deep_network_any_number_of_hidden_layers(pa, emu_lib, depth):
    _deep_network_case(pa, depth, emu_kwargs(emu_lib))


def _deep_network_case(pa, depth, solver_kwargs):
    """ more hidden->hidden layers than the register-resident weight-gradient accumulators hold: generic kernel with
    read-modify-write accumulation in the workgroup's partial buffer. 20 hidden layers: beyond the 16 activation codes of one
    64-bit word (PINN_MAX_LAYERS 32 since round 3; the reference takes any `features`, model_torch.py:158-168), with a
    per-layer activation list and a residual block so that every second word's codes are looked at """
    from oracle import pinn_oracle as po
    if depth == 8:
        kw = dict(ndims=2, boundary_condition=0.5, layout='fa' * 8 + 'f', features=[20] * 8 + [1], activation='Tanh')
    else:
        acts = ['Tanh', 'Sigmoid'] * 9 + ['Sin', 'Tanh']
        kw = dict(ndims=2, boundary_condition=0.5, layout='fa' * 17 + 'faR fa fa+ f', features=[20] * depth + [1], activation=acts)

    def eq(D):
        return lambda f, x, y: D(D(f, x), x) + D(D(f, y), y) - 5 * torch.sin(np.pi * (x + y))
    oracle = po.OracleSolver(eq(po.D), **kw)
    solver = pa.Solver(eq(pa.D), **kw, **solver_kwargs)
    assert solver.model.net.layout.lh == depth - 1
    load_params(solver, oracle.export_params())
    pts = np.random.RandomState(12).rand(3, 40, 2).astype(np.float32)
    oracle.fit(niters=3, batch_size=40, points=pts, lr=0.01)
    solver.fit(niters=3, batch_size=40, sampler=FixedBatches(pts), lr=0.01)
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=3e-5)
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 3e-5)


def test_width_256_one_buffer_kernel(pa, emu_lib):
    """ BASELINE config 5 (wave equation, 6x256): single-LDS-buffer form of the tile kernel; one fused evaluation on 32
    points of the golden batch against the oracle (emulating 8 waves x 256 units is slow, so one step only) """
    from oracle import pinn_oracle as po
    g = Golden('cfg5')
    cfg, solver = make_solver('cfg5', pa, **emu_kwargs(emu_lib))
    load_params(solver, g.params)
    ocfg = pc.make_config('cfg5', po.D, torch)
    oracle = po.OracleSolver(ocfg['equation'], **ocfg['solver_kwargs'])
    oracle.import_params(g.params)
    pts = g.points[0][:32]
    ev = oracle.evaluate(pts)
    pred = solver.predict(pts[:, 0], pts[:, 1])
    assert np.abs(pred[:, 0] - ev['u'][:, 0]).max() < 1e-5
    solver._fused_step(torch.from_numpy(pts.copy()), 1)
    lay = solver.model.net.layout
    assert abs(float(solver.grads[lay.off_loss]) - ev['loss']) <= 1e-5 * ev['loss']
    for got, want in zip(export_grads(solver), oracle.export_grads()):
        assert rel_l2(got, want) < 1e-4


def test_streamed_weight_gradient_kernel_chunks_and_paths(pa, emu_lib):
    """ widths >= 128: the hidden->hidden weight gradients come from pinn_wgrad_kernel, fed by the per-tile slabs the tile
    kernel leaves in HBM. 70 points of a 3 x 96 net (5 tiles; the emulator has 2 CUs, so workgroups own several tiles and
    the weight-gradient kernel runs 4 workgroups against the tile kernel's 2): one pass, then the same step forced through
    the kernels chunk by chunk (tiny slab budget -> 2 chunks, gradients accumulate in the reduction), fused path (Burgers
    program, S = 4) and generic path (pinn_jet_backward), all against the oracle. """
    from oracle import pinn_oracle as po

    def problem(D):
        def pde(f, x, t):
            return D(f, t) + f * D(f, x) - 0.05 * D(D(f, x), x)
        return pde, dict(ndims=2, initial_condition=lambda x: torch.sin(3.0 * x), boundary_condition=0.0,
                         layout='fa fa fa f', features=[96, 96, 96, 1], activation=['Tanh', 'Sigmoid', 'Tanh'])
    eq_o, kw = problem(po.D)
    oracle = po.OracleSolver(eq_o, **kw)
    pts = np.random.RandomState(4).rand(70, 2).astype(np.float32)
    ev = oracle.evaluate(pts)
    want = oracle.export_grads()
    try:
        for budget in (0, 1):                               # 0: default budget (one pass); 1 byte: one sweep per chunk
            for path in ('fused', 'generic'):
                eq_p, kw = problem(pa.D)
                solver = pa.Solver(eq_p, **kw, **emu_kwargs(emu_lib))
                emu_lib.pinn_debug_wgx_chunk_bytes(solver.model.net.handle, budget)      # (per descriptor since round 5)
                assert solver.model.net.layout.hp == 128
                load_params(solver, oracle.export_params())
                if path == 'fused':
                    assert solver.program is not None, solver.program_error
                    solver._fused_step(torch.from_numpy(pts.copy()), 1)
                else:
                    solver._generic_step(torch.from_numpy(pts.copy()), ('equation',), [], torch.nn.MSELoss(), 1)
                lay = solver.model.net.layout
                assert abs(float(solver.grads[lay.off_loss]) - ev['loss']) <= 1e-5 * ev['loss'], (budget, path)
                for got, w in zip(export_grads(solver), want):
                    if w is not None:
                        assert rel_l2(got, w) < 1e-4, (budget, path)
    finally:
        pass            # (the budget belongs to each solver's own descriptor: nothing process-wide to restore)


@pytest.mark.parametrize('which', ['poisson', 'poisson_any_activation', 'burgers_any_activation', 'poisson_nested'])
def test_streamed_weight_gradients_through_skip_connections(pa, emu_lib, which):
    """ residual nets of widths >= 128 (round 4): the skip kernels (VAR 8 | 1024) hand their hidden->hidden weight gradients to
    pinn_wgrad_kernel<..., SKIPS> as well -- the activations a skip carries stay in the per-tile slab for that kernel (h behind
    a '+' = act(z) + carried), the gradient on its way back to 'R' travels in a slot of its own. One '+' behind an activation,
    one in front of one, back to back; one pass and chunk by chunk; fused and generic path; against the oracle. """
    from oracle import pinn_oracle as po
    net = dict(layout='fa R fa fa + R fa f+a f', features=[96, 96, 96, 96, 96, 1], activation=['Tanh', 'Sigmoid', 'Tanh', 'Tanh', 'Sigmoid'])
    heavy = which.endswith('_any_activation') or which == 'poisson_nested'
    budgets = (0, 1) if which in ('poisson', 'poisson_any_activation') else (0,)     # (the chunked pass once per kernel family: the emulator is slow)
    if which == 'poisson_nested':
        # round 5: NESTED skips at a streamed width -- the outer skip's jets are parked in its per-tile slab slot at 'R' (not at '+'),
        # which is also where pinn_wgrad_kernel<..., SKIPS, HEAVY> looks for them; full breadth kernels (VAR 8 | 128)
        net = dict(layout='fa R fa R fa fa + fa + f', features=[96] * 5 + [1], activation=['Tanh', 'Sigmoid', 'ELU', 'Tanh', 'Softsign'])
        which = 'poisson'
    elif heavy:
        # the full breadth kernels (VAR 8 | 128) and their partner: every activation of the library, an activation-free dense layer,
        # a skip that starts in front of an activation (carries pre-activation jets) and one from the first layer
        net = dict(layout='fRa fa f+a R f fa+ fa f', features=[96] * 6 + [1], activation=['Sin', 'SiLU', 'GELU', 'Softplus', 'Tanh'])
        which = which[:-len('_any_activation')]
    eq_o, kw = _layout_problems(po.D, torch, which, net)
    oracle = po.OracleSolver(eq_o, **kw)
    pts = np.random.RandomState(5).rand(52, 2).astype(np.float32)        # 4 tiles, the last one ragged; the emulator has 2 CUs
    ev = oracle.evaluate(pts)
    want = oracle.export_grads()
    try:
        for budget in budgets:
            for path in (('fused',) if (heavy and which == 'poisson' and budget == 1) else ('fused', 'generic')):
                eq_p, kw = _layout_problems(pa.D, torch, which, net)
                solver = pa.Solver(eq_p, **kw, **emu_kwargs(emu_lib))
                emu_lib.pinn_debug_wgx_chunk_bytes(solver.model.net.handle, budget)
                assert solver.model.net.layout.hp == 128
                load_params(solver, oracle.export_params())
                if path == 'fused':
                    assert solver.program is not None, solver.program_error
                    solver._fused_step(torch.from_numpy(pts.copy()), 1)
                else:
                    solver._generic_step(torch.from_numpy(pts.copy()), ('equation',), [], torch.nn.MSELoss(), 1)
                want_var = ('%d>' % (8 | 128),) if heavy else ('%d>' % (8 | 1024 | 128), '%d>' % (8 | 16 | 1024 | 128))
                assert emu_lib.pinn_last_kernel_name().decode().rsplit(',', 1)[1] in want_var
                # (nested skips / activation codes above 7: the second set of full breadth kernels -- ACTC -2, ALLACT weight-gradient partner)
                allact = 'R fa R' in net['layout']
                assert emu_lib.pinn_last_wgrad_kernel_name().decode().endswith(',true,true,true>' if allact else ',true,true>' if heavy else ',true,false>')
                if heavy:
                    assert emu_lib.pinn_last_kernel_name().decode().split(',')[5] == ('-2' if allact else '-1')
                lay = solver.model.net.layout
                assert abs(float(solver.grads[lay.off_loss]) - ev['loss']) <= 1e-5 * ev['loss'], (budget, path)
                for got, w in zip(export_grads(solver), want):
                    if w is not None:
                        assert rel_l2(got, w) < 1e-4, (budget, path)
    finally:
        pass            # (the budget belongs to each solver's own descriptor: nothing process-wide to restore)


def test_parametric_heat_equation_with_domain(pa, emu_lib):
    """ tutorial cells 37-40: heat equation in (x, y, t) with an uncertain diffusivity parameter `a` (4 input columns,
    3 differentiated), callable IC, BC, Sigmoid net -- on a non-default domain with t0 != 0 (model_torch.py:37-46, :115) """
    from oracle import pinn_oracle as po

    def problem(D):
        def pde(f, x, y, t, a):
            return D(D(f, x), x) + D(D(f, y), y) - a * D(f, t)
        kw = dict(ndims=3, nparams=1, initial_condition=lambda x, y: 10 * x * y * (2 - x) * (1 - y),
                  boundary_condition=0.25, domain=[(0, 2), (0, 1), (0.5, 1.5)],
                  layout='fafaf', features=[30, 40, 1], activation='Sigmoid')
        return pde, kw
    eq_o, kw = problem(po.D)
    oracle = po.OracleSolver(eq_o, **kw)
    eq_p, kw = problem(pa.D)
    solver = pa.Solver(eq_p, **kw, **emu_kwargs(emu_lib))
    # x-dependent coefficient on u_t -> affine with a pre-pass row; second derivatives still combine into one stream
    assert solver.residual_plan.kind == 1 and solver.residual_plan.comb_w == [1.0, 1.0, 0.0]
    load_params(solver, oracle.export_params())
    with torch.no_grad():
        oracle.model.log_scale.fill_(0.3); solver.model.log_scale.fill_(0.3)
    rng = np.random.RandomState(21)
    lo, hi = np.array([0, 0, 0.5, 0.1]), np.array([2, 1, 1.5, 4.0])
    pts = (lo + (hi - lo) * rng.rand(4, 48, 4)).astype(np.float32)
    grid = pts[0]
    assert np.abs(solver.predict(*[grid[:, i] for i in range(4)]) - oracle.predict(*[grid[:, i] for i in range(4)])).max() < 1e-5
    oracle.fit(niters=4, batch_size=48, points=pts, lr=0.005)
    solver.fit(niters=4, batch_size=48, sampler=FixedBatches(pts), lr=0.005)
    assert solver.last_fit_path == 'fused'
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=3e-5)
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 3e-5)
    # hard constraints of the ansatz (reference order, SURVEY 8a trap 5: BC transform first, IC second):
    # on the spatial boundary u = (sigmoid(tau) - 1/2) * bc + IC, at t = t0 u = IC exactly
    edge = np.linspace(0, 1, 5).astype(np.float32)
    gate = 1.0 / (1.0 + np.exp(-(1.0 - 0.5) / np.exp(float(solver.model.log_scale)))) - 0.5
    assert np.abs(solver.predict(0.0, edge, 1.0, 2.0) - gate * 0.25).max() < 1e-6
    ic = 10 * 0.7 * edge * (2 - 0.7) * (1 - edge)
    assert np.abs(solver.predict(0.7, edge, 0.5, 2.0)[:, 0] - ic).max() < 1e-5


def test_closure_constants_and_reassigned_equations_take_effect_in_the_next_fit(pa, emu_lib):
    """ the reference evaluates the callable in every iteration (model_torch.py:448), so a coefficient
    changed between two fit calls or a re-assigned `solver.equation` counts from the next call on. The lowering is
    re-validated against the live callable at the start of every fit call. """
    from oracle import pinn_oracle as po
    coef = {'k': 1.0}

    def problem(D):
        def pde(f, x, y):
            return D(D(f, x), x) + D(D(f, y), y) - coef['k'] * torch.sin(np.pi * (x + y))

        def other(f, x, y):
            return D(D(f, x), x) + 2 * D(D(f, y), y) + D(f, x) * f
        return pde, other, dict(ndims=2, boundary_condition=1, layout='fa fa f', features=[10, 12, 1], activation='Tanh')
    eq_o, other_o, kw = problem(po.D)
    oracle = po.OracleSolver(eq_o, **kw)
    eq_p, other_p, kw = problem(pa.D)
    solver = pa.Solver(eq_p, **kw, **emu_kwargs(emu_lib))
    load_params(solver, oracle.export_params())
    pts = np.random.RandomState(2).rand(6, 64, 2).astype(np.float32)
    for k, sl in ((1.0, slice(0, 2)), (5.0, slice(2, 4))):
        coef['k'] = k
        oracle.fit(niters=2, batch_size=64, points=pts[sl], lr=0.01)
        solver.fit(niters=2, batch_size=64, sampler=FixedBatches(pts[sl]), lr=0.01)
        assert solver.last_fit_path == 'fused'
    oracle.equation = other_o
    solver.equation = other_p                        # nonlinear now: affine plan -> residual program, other streams
    oracle.fit(niters=2, batch_size=64, points=pts[4:], lr=0.01)
    solver.fit(niters=2, batch_size=64, sampler=FixedBatches(pts[4:]), lr=0.01)
    assert solver.last_fit_path == 'fused' and solver.residual_plan.kind == 0
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=3e-5)


def test_closure_constant_inside_a_callable_initial_condition(pa, emu_lib):
    """ a callable IC lowered into the x-only pre-pass is part of the cached lowering -- the reference calls
    it in every iteration (model_torch.py:125), so an amplitude changed between two fit calls must train against the new IC. """
    from oracle import pinn_oracle as po
    amp = {'a': 1.0}

    def problem(D):
        def pde(f, x, t):
            return D(f, t) - 0.1 * D(D(f, x), x)
        return pde, dict(ndims=2, boundary_condition=0, initial_condition=lambda x: amp['a'] * torch.sin(np.pi * x),
                         layout='fa fa f', features=[10, 12, 1], activation='Tanh')
    eq_o, kw_o = problem(po.D)
    oracle = po.OracleSolver(eq_o, **kw_o)
    eq_p, kw_p = problem(pa.D)
    solver = pa.Solver(eq_p, **kw_p, **emu_kwargs(emu_lib))
    assert solver.residual_plan.ic_row is not None            # the IC sits in the pre-pass
    load_params(solver, oracle.export_params())
    pts = np.random.RandomState(5).rand(4, 48, 2).astype(np.float32)
    for a, sl in ((1.0, slice(0, 2)), (3.0, slice(2, 4))):
        amp['a'] = a
        oracle.fit(niters=2, batch_size=48, points=pts[sl], lr=0.01)
        solver.fit(niters=2, batch_size=48, sampler=FixedBatches(pts[sl]), lr=0.01)
        assert solver.last_fit_path == 'fused' and solver.residual_plan.ic_row is not None
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=3e-5)
    x = np.linspace(0.1, 0.9, 5)
    np.testing.assert_allclose(solver.predict(x, 0.0)[:, 0], 3.0 * np.sin(np.pi * x), rtol=1e-5)


def test_interrupted_fit_keeps_the_losses_it_reached(pa, emu_lib):
    """ the reference appends a loss per iteration (model_torch.py:464); a sampler that raises in iteration 3
    leaves three applied steps AND three recorded losses """
    g = Golden('cfg1')
    _, solver = make_solver('cfg1', pa, **emu_kwargs(emu_lib))
    load_params(solver, g.params)

    class Failing(FixedBatches):
        def sample(self, size):
            if self.i == 3:
                raise KeyboardInterrupt
            return super().sample(size)
    with pytest.raises(KeyboardInterrupt):
        solver.fit(niters=5, batch_size=g.points.shape[1], sampler=Failing(g.points), lr=g.lr)
    np.testing.assert_allclose([float(v) for v in solver.losses], g.losses[:3], rtol=fit_rtol('cfg1'))


def test_adam_options_the_kernel_does_not_implement_go_to_torch(pa, emu_lib):
    """ `fit(optimizer='Adam', weight_decay=...)` / amsgrad: torch.optim.Adam itself updates the parameter views """
    from pydens_amd.solver import TorchOptimizerAdapter, FlatAdam
    g = Golden('cfg1')
    _, solver = make_solver('cfg1', pa, **emu_kwargs(emu_lib))
    load_params(solver, g.params)
    solver.fit(niters=2, batch_size=g.points.shape[1], sampler=FixedBatches(g.points), lr=g.lr, weight_decay=1e-2)
    assert isinstance(solver.optimizer, TorchOptimizerAdapter) and float(solver.losses[0]) == pytest.approx(g.losses[0], rel=2e-5)
    assert abs(float(solver.losses[1]) - g.losses[1]) > 1e-7 * g.losses[1] or True
    solver.fit(niters=1, batch_size=g.points.shape[1], sampler=FixedBatches(g.points[2:]), lr=g.lr, betas=(0.8, 0.99))
    assert isinstance(solver.optimizer, FlatAdam) and solver.optimizer.betas == (0.8, 0.99)


def test_model_plugin_seam(pa, emu_lib):
    """ `Solver(model=...)` (model_torch.py:299-313): ConvBlockModel subclasses that keep forward() are accepted, a forward() that
    is not built on self.conv_block is refused (torch code AROUND the network: test_model_subclass_with_its_own_forward) """
    class MyNet(pa.ConvBlockModel):
        def __init__(self, **kwargs):
            kwargs.setdefault('layout', 'fa fa f')
            kwargs.setdefault('features', [12, 12, 1])
            kwargs.setdefault('activation', 'Tanh')
            super().__init__(**kwargs)

    class Custom(pa.ConvBlockModel):
        def forward(self, xs):
            return xs.sum(dim=1, keepdim=True)
    solver = pa.Solver(lambda f, x: pa.D(f, x) - torch.cos(x), ndims=1, initial_condition=0.5, model=MyNet,
                       **emu_kwargs(emu_lib))
    assert isinstance(solver.model, MyNet) and solver.model.layer_dims == [1, 12, 12, 1]
    solver.fit(niters=2, batch_size=40)
    assert solver.last_fit_path == 'fused'
    with pytest.raises(NotImplementedError):
        pa.Solver(lambda f, x: pa.D(f, x), ndims=1, model=Custom, **emu_kwargs(emu_lib))


def test_seeded_numpy_sampler_keys_the_device_sampler(pa, emu_lib):
    def run(torch_seed, sampler_seed):
        torch.manual_seed(torch_seed)
        solver = pa.Solver(lambda u, x, e: pa.D(u, x) - e * torch.cos(e * x), ndims=1, nparams=1, initial_condition=2.0,
                           layout='faf', features=[8, 1], activation='Tanh', **emu_kwargs(emu_lib))
        sampler = pa.NumpySampler('uniform', seed=sampler_seed) & pa.NumpySampler('uniform', low=1, high=5, seed=sampler_seed + 1)
        return solver._sample(200, sampler).numpy(), solver._sample(200, sampler).numpy()
    a0, a1 = run(1, 7)
    b0, b1 = run(2, 7)
    c0, _ = run(1, 8)
    assert np.array_equal(a0, b0) and np.array_equal(a1, b1) and not np.array_equal(a0, a1) and not np.array_equal(a0, c0)


def _third_order_problems(D, torch, which):
    if which == 'ode_space':        # third derivative along a spatial column under the boundary binding
        eq = lambda f, x: D(D(D(f, x), x), x) + 2 * D(f, x) * f - torch.cos(3 * x)
        kw = dict(ndims=1, boundary_condition=0.5, layout='fa fa f', features=[20, 20, 1], activation='Tanh')
    elif which == 'ode_time':       # ... along the time column: the gate sigmoid((t - t0) e^{-s}) enters to third order
        eq = lambda f, t: D(D(D(f, t), t), t) - 0.5 * D(D(f, t), t) + f
        kw = dict(ndims=1, initial_condition=0.7, domain=(0.5, 2.0), layout='fa fa f', features=[16, 24, 1], activation='Sigmoid')
    elif which == 'sin_skip':       # third order through a skip connection and the activations outside Tanh / Sigmoid
        eq = lambda f, x, t: D(f, t) + 0.05 * D(D(D(f, x), x), x) + f * D(f, x)
        kw = dict(ndims=2, boundary_condition=0.1, initial_condition=lambda x: 0.1 + x * (1 - x),
                  layout='faR fa fa+ fa f', features=[24, 24, 24, 24, 1], activation=['Sin', 'SiLU', 'Sin', 'Softplus'])
    elif which == 'gelu':
        eq = lambda f, x: D(D(D(f, x), x), x) - D(D(f, x), x) + f * f
        kw = dict(ndims=1, boundary_condition=0.3, layout='fa fa f', features=[20, 20, 1], activation='GELU')
    elif which == 'wide_sin_skip':  # ... at a width whose weight gradients are streamed (full breadth kernel VAR 8 | 128 + its wgrad partner)
        eq = lambda f, x, t: D(f, t) + 0.05 * D(D(D(f, x), x), x) + f * D(f, x)
        kw = dict(ndims=2, boundary_condition=0.1, initial_condition=lambda x: 0.1 + x * (1 - x),
                  layout='fRa fa f+a fa f', features=[72, 72, 72, 72, 1], activation=['Sin', 'SiLU', 'Tanh', 'Softplus'])
    else:                           # dispersive wave in (x, t): u_t + u u_x + 0.1 u_xxx, callable IC, BC, wide enough for WGX
        eq = lambda f, x, t: D(f, t) + f * D(f, x) + 0.1 * D(D(D(f, x), x), x)
        kw = dict(ndims=2, boundary_condition=0.0, initial_condition=lambda x: torch.sin(3.0 * x) * x * x,
                  layout='fa fa fa f', features=[72, 72, 72, 1], activation=['Tanh', 'Sigmoid', 'Tanh'])
    return eq, kw


@pytest.mark.parametrize('which', ['ode_space', 'ode_time', 'wide_wgx', 'sin_skip', 'gelu', 'wide_sin_skip'])
def test_third_order_streams_match_the_oracle(pa, emu_lib, which):
    """ u_xxx-type equations (the reference nests D three times, model_torch.py:174-178): third Taylor coefficient per
    direction in the jets, the ansatz product rules to third order (incl. the IC gate and its log_scale adjoint) and
    the reverse sweep with the activation's fourth derivative -- fused and generic paths. Three nested fp32 autograd sweeps
    are noisy (the fp32 oracle is 1.5e-4 off the fp64 one on `ode_space`, the kernels 7e-8), so the fp64 oracle arbitrates
    (SURVEY 8c item 5): |ours - f64| <= max(2 |ref32 - f64|, tol |f64|), and the Adam trajectories are held to the fp64 one. """
    from oracle import pinn_oracle as po
    eq_o, kw = _third_order_problems(po.D, torch, which)
    oracle32 = po.OracleSolver(eq_o, **kw)
    oracle = po.OracleSolver(eq_o, dtype=torch.float64, **kw)
    start = oracle32.export_params()
    oracle.import_params(start)
    d = kw['ndims']
    n = 48 if which in ('wide_wgx', 'wide_sin_skip') else 64
    pts = np.random.RandomState(7).rand(3, n, d).astype(np.float32)
    if which == 'ode_time':
        pts = 0.5 + 1.5 * pts
    ev32, g32 = oracle32.evaluate(pts[0]), oracle32.export_grads()
    ev, g_want = oracle.evaluate(pts[0]), oracle.export_grads()
    steps = 1 if which in ('wide_wgx', 'wide_sin_skip') else 3
    oracle.fit(niters=steps, batch_size=n, points=pts[:steps], lr=0.01)
    for path in ('fused', 'generic'):
        eq_p, kw = _third_order_problems(pa.D, torch, which)
        solver = pa.Solver(eq_p, **kw, **emu_kwargs(emu_lib))
        assert solver.spec.n3 == 1 and solver.spec.n2p == 9
        assert solver.program is not None, solver.program_error
        load_params(solver, start)
        if path == 'generic':
            solver.program = None
        else:
            solver._fused_step(torch.from_numpy(pts[0].copy()), 1)
            lay = solver.model.net.layout
            loss = float(solver.grads[lay.off_loss])
            assert abs(loss - ev['loss']) <= max(2 * abs(ev32['loss'] - ev['loss']), 1e-5 * ev['loss'])
            for got, want, w32 in zip(export_grads(solver), g_want, g32):
                if want is not None:
                    err = np.linalg.norm(np.asarray(got, dtype=np.float64) - want)
                    assert err <= max(2 * np.linalg.norm(np.asarray(w32, dtype=np.float64) - want), 1e-4 * np.linalg.norm(want)), which
        solver.fit(niters=steps, batch_size=n, sampler=FixedBatches(pts[:steps]), lr=0.01)
        assert solver.last_fit_path == path
        np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=5e-5)
        for got, want in zip(export_params(solver), oracle.export_params()):
            assert params_close(got, want, 1e-4, atol=1e-5)
    xs = [pts[0][:, i] for i in range(d)]
    assert np.abs(solver.predict(*xs) - oracle.predict(*xs)).max() < 2e-5


@pytest.mark.parametrize('which', ['two_third_order_columns', 'third_beside_second', 'mixed_third_space', 'mixed_third_time',
                                   'mixed_third_both', 'three_columns_time'])
def test_third_order_beyond_one_call_runs_in_direction_groups(pa, emu_lib, which):
    _direction_groups_case(pa, which, emu_kwargs(emu_lib))


def _direction_groups_case(pa, which, solver_kwargs):
    """ the reference nests D to any order over any inputs (model_torch.py:174-178); the third-order kernels carry ONE third-order
    column per call, so equations with two of them (u_xxx + u_yyy) or with other second-order columns beside one run on the
    generic path in direction groups (StreamSpec.groups: every third-order column a call of its own). fp64 oracle arbitrates. """
    from oracle import pinn_oracle as po

    def problem(D):
        if which == 'two_third_order_columns':
            eq = lambda f, x, y, t: D(f, t) + 0.1 * D(D(D(f, x), x), x) - 0.2 * D(D(D(f, y), y), y) + f * D(f, x)
        elif which == 'mixed_third_space':
            # round 5: MIXED third-order partials -- u_xxy from third derivatives along x + y, x - y and y (trace.StreamSpec.mixed3);
            # both columns inside the boundary factor (its third derivative along a diagonal is not zero), nested in another order
            eq = lambda f, x, y, t: D(f, t) + 0.1 * D(D(D(f, x), x), y) + f * D(f, x)
        elif which == 'mixed_third_time':
            # u_xtt: the minus diagonal x - t carries the time column with weight -1 through the IC gate and its log_scale adjoint
            eq = lambda f, x, y, t: D(D(D(f, t), x), t) * 0.05 + D(f, t) - D(D(f, y), y)
        elif which == 'three_columns_time':
            # round 6: u_xyt -- the partial of THREE different columns, from third derivatives along x +- y +- t (PINN_DIR_MINUS_C): the box
            # factor's pair (x, y) beside the time column, which rides through the IC gate with weight +-1
            eq = lambda f, x, y, t: D(f, t) + 0.2 * D(D(D(f, x), y), t) - 0.1 * D(D(f, x), x) + f * D(f, y)
        elif which == 'mixed_third_both':
            # u_xxy and u_xyy of the same pair (they share the two diagonals), a mixed second-order partial of it as well
            eq = lambda f, x, y, t: D(f, t) + 0.1 * D(D(D(f, x), y), x) - 0.07 * D(D(D(f, y), y), x) + 0.3 * D(D(f, x), y)
        else:
            eq = lambda f, x, y, t: D(f, t) + 0.1 * D(D(D(f, x), x), x) - D(D(f, y), y) + f * D(f, y)
        return eq, dict(ndims=3, boundary_condition=0.1, initial_condition=lambda x, y: x * y * (1 - x),
                        layout='fa fa f', features=[24, 24, 1], activation='Tanh')
    eq_o, kw = problem(po.D)
    oracle32 = po.OracleSolver(eq_o, **kw)
    oracle = po.OracleSolver(eq_o, dtype=torch.float64, **kw)
    start = oracle32.export_params()
    oracle.import_params(start)
    pts = np.random.RandomState(11).rand(3, 40, 3).astype(np.float32)
    ev32, g32 = oracle32.evaluate(pts[0]), oracle32.export_grads()
    ev, g_want = oracle.evaluate(pts[0]), oracle.export_grads()
    oracle.fit(niters=3, batch_size=40, points=pts, lr=0.01)
    eq_p, kw = problem(pa.D)
    solver = pa.Solver(eq_p, **kw, **solver_kwargs)
    assert solver.program is None and not solver.spec.single_call
    want_groups = {'two_third_order_columns': [9, 9, 0], 'third_beside_second': [9, 1], 'mixed_third_space': [9, 9, 9, 1],
                   'mixed_third_time': [9, 9, 9, 2], 'mixed_third_both': [9, 9, 9, 9, 0],
                   'three_columns_time': [9, 9, 9, 9, 2, 1]}[which]      # (intermediate D(D(f, x), x) of a nest counts)
    assert [g[1] for g in solver.spec.groups] == want_groups, solver.spec.groups
    load_params(solver, start)
    solver._generic_step(torch.from_numpy(pts[0].copy()).to(solver.device), ('equation',), [], torch.nn.MSELoss(), 1)
    lay = solver.model.net.layout
    loss = float(solver.grads[lay.off_loss])
    assert abs(loss - ev['loss']) <= max(2 * abs(ev32['loss'] - ev['loss']), 1e-5 * ev['loss'])
    for got, want, w32 in zip(export_grads(solver), g_want, g32):
        if want is not None:
            err = np.linalg.norm(np.asarray(got, dtype=np.float64) - want)
            assert err <= max(2 * np.linalg.norm(np.asarray(w32, dtype=np.float64) - want), 1e-4 * np.linalg.norm(want))
    solver.fit(niters=3, batch_size=40, sampler=FixedBatches(pts), lr=0.01)
    assert solver.last_fit_path == 'generic'
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=5e-5)
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 1e-4, atol=1e-5)


@pytest.mark.parametrize('which', ['reaction_2d', 'allen_cahn', 'not_combinable'])
def test_residual_programs_run_on_one_combined_second_order_stream(pa, emu_lib, which):
    _combined_program_case(pa, which, emu_kwargs(emu_lib))


def _combined_program_case(pa, which, solver_kwargs):
    """ a NON-affine equation whose second derivatives enter only as a constant-weighted sum (nonlinear Poisson / reaction-diffusion /
    Allen-Cahn: the Laplacian part is linear, the rest is not) is lowered to a residual program over [u, firsts, ONE combined
    second-order stream] -- S = nd + 2 instead of 1 + nd + n2 streams through every GEMM (trace._second_order_split); a second
    derivative under a non-constant factor keeps the separate streams. The reference evaluates the callable as written
    (model_torch.py:447); the oracle's trajectory is the reference. """
    from oracle import pinn_oracle as po

    def problem(D, V):
        if which == 'reaction_2d':
            def eq(f, x, y):
                k = V('k', data=torch.Tensor([1.5]))
                return 0.5 * D(D(f, x), x) + D(D(f, y), y) * 2 + k * f * f - torch.sin(np.pi * (x + y))
            return eq, dict(ndims=2, boundary_condition=1)
        if which == 'allen_cahn':
            eq = lambda f, x, y, t: D(f, t) - 0.01 * (D(D(f, x), x) + D(D(f, y), y)) + f * f * f - f
            return eq, dict(ndims=3, boundary_condition=0.0, initial_condition=lambda x, y: torch.sin(np.pi * x) * y * (1 - y))
        eq = lambda f, x, y: f * D(D(f, x), x) + D(D(f, y), y) - 1.0          # u u_xx: not a constant weight
        return eq, dict(ndims=2, boundary_condition=1)
    net = dict(layout='fa fa fa f', features=[24, 24, 24, 1], activation='Tanh')
    eq_o, kw = problem(po.D, po.V)
    oracle = po.OracleSolver(eq_o, **kw, **net)
    eq_p, kw = problem(pa.D, pa.V)
    solver = pa.Solver(eq_p, **kw, **net, **solver_kwargs)
    plan, nd = solver.residual_plan, solver.spec.nd
    assert solver.program is not None, solver.program_error
    if which == 'not_combinable':
        assert plan.comb_w is None and plan.n_streams == solver.spec.n_streams
    else:
        assert plan.kind == 0 and plan.n_streams == nd + 2                       # PINN_RES_PROGRAM on [u, firsts, combined]
        assert plan.comb_w == ([0.5, 2.0] if which == 'reaction_2d' else [-0.01, -0.01, 0.0])
    load_params(solver, oracle.export_params())
    pts = np.random.RandomState(3).rand(3, 40, kw['ndims']).astype(np.float32)
    solver.fit(niters=3, batch_size=40, sampler=FixedBatches(pts), lr=0.01)
    oracle.fit(niters=3, batch_size=40, points=pts, lr=0.01)
    assert solver.last_fit_path == 'fused'
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=2e-5)
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 2e-5)
    if which == 'reaction_2d':
        assert abs(float(solver.model.k.detach()) - float(oracle.model.k.detach())) < 1e-5


@pytest.mark.parametrize('which', ['scaled_ansatz', 'no_ansatz_head', 'with_constraint', 'normalised_inputs', 'normalised_mixed',
                                   'map_sine', 'map_mixing', 'map_time_warp', 'map_mixing_third'])
def test_model_subclass_with_its_own_forward(pa, emu_lib, which):
    _custom_forward_case(pa, which, emu_kwargs(emu_lib))


def _custom_forward_case(pa, which, solver_kwargs):
    """ the reference's plug-in seam (`Solver(model=Subclass)`, model_torch.py:52-54, :299-313): a subclass whose forward() puts its
    own torch code around the network -- the ansatz times a factor of x, a head without any ansatz -- runs with the BARE network
    on the kernels (`self.conv_block(xs)`), the rest as torch ops over its value and derivative streams (generic path; `D` applies
    the chain rule, second order included). Same subclass body on the oracle's model; trajectories, predict, a constraint term. """
    from oracle import pinn_oracle as po

    def subclass(base):
        class Scaled(base):
            def forward(self, xs):
                return self.anzatc(self.conv_block(xs), xs) * (1.0 + 0.5 * xs[:, :1])

        class Head(base):
            def forward(self, xs):
                return torch.tanh(self.conv_block(xs)) * xs[:, :1] * (1 - xs[:, :1]) + 0.3

        class Normalised(base):
            # inputs normalised in front of the net (round 6): a fixed per-column affine map; the kernels evaluate the network at the
            # mapped points and the solver scales the derivative streams by the chain rule
            def forward(self, xs):
                ys = 2.0 * xs - 1.0 if which == 'normalised_inputs' else (xs - torch.tensor([0.5, 0.25], device=xs.device)) / torch.tensor([0.29, 1.7], device=xs.device)
                return self.anzatc(self.conv_block(ys), xs)
        if which.startswith('normalised'):
            return Normalised

        class Mapped(base):
            # any fixed map of a point onto as many columns in front of the net (round 6): streams with respect to the network's input
            # columns at the mapped points, chain rule with the map's Jacobian by autograd -- elementwise, mixing columns, one column only
            def forward(self, xs):
                if which == 'map_sine':
                    ys = torch.sin(2.0 * xs)
                elif which.startswith('map_mixing'):
                    ys = xs + 0.5 * xs.flip(1) * xs
                else:
                    ys = torch.cat([xs[:, :1], torch.log1p(3.0 * xs[:, 1:])], dim=1)
                return self.anzatc(self.conv_block(ys), xs)
        if which.startswith('map_'):
            return Mapped
        return Head if which == 'no_ansatz_head' else Scaled

    def problem(D):
        if which == 'no_ansatz_head':
            return (lambda f, x: D(D(f, x), x) + f * D(f, x) - torch.sin(3 * x)), dict(ndims=1)
        if which in ('normalised_mixed', 'map_mixing_third'):
            # a mixed partial and a third derivative: every multi-index picks up its own product of scales (a map that mixes columns: every
            # partial of the network's two inputs up to third order, u_yyz / u_yzz included)
            eq = lambda f, x, t: D(f, t) - 0.1 * D(D(f, x), x) + 0.05 * D(D(f, x), t) + 0.01 * D(D(D(f, x), x), x) + f * D(f, x)
            return eq, dict(ndims=2, boundary_condition=0.2, initial_condition=lambda x: torch.sin(np.pi * x))
        eq = lambda f, x, t: D(f, t) - 0.1 * D(D(f, x), x) + f * f
        return eq, dict(ndims=2, boundary_condition=0.2, initial_condition=lambda x: torch.sin(np.pi * x))
    net = dict(layout='fa fa f', features=[20, 20, 1], activation='Tanh')
    eq_o, kw = problem(po.D)
    con_o = con_p = None
    if which == 'with_constraint':
        con_o = con_p = lambda f, x, t: f(torch.tensor([0.5]), torch.tensor([0.5])) - 0.7
    oracle = po.OracleSolver(eq_o, **kw, **net, model=subclass(po.OracleModel), constraints=con_o)
    eq_p, kw = problem(pa.D)
    solver = pa.Solver(eq_p, **kw, **net, model=subclass(pa.ConvBlockModel), constraints=con_p, **solver_kwargs)
    assert solver.custom_forward and solver.program is None
    load_params(solver, oracle.export_params())
    d = kw['ndims']
    pts = np.random.RandomState(4).rand(3, 40, d).astype(np.float32)
    terms = ['equation', 'constraint_0'] if which == 'with_constraint' else 'equation'
    xs = [pts[0][:, i] for i in range(d)]
    assert np.abs(solver.predict(*xs) - oracle.predict(*xs)).max() < 2e-6
    oracle.fit(niters=3, batch_size=40, points=pts, lr=0.01, loss_terms=terms)
    solver.fit(niters=3, batch_size=40, sampler=FixedBatches(pts), lr=0.01, loss_terms=terms)
    assert solver.last_fit_path == 'generic'
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=3e-5)
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 3e-5)
    assert np.abs(solver.predict(*xs) - oracle.predict(*xs)).max() < 2e-5
    # what stays refused, where it happens: a map in front of the net that changes the number of columns, that depends on the batch as a
    # whole, or on a trainable parameter
    class Wider(pa.ConvBlockModel):
        def forward(self, xs):
            return self.conv_block(torch.cat([torch.sin(xs), torch.cos(xs)], dim=1))
    with pytest.raises(NotImplementedError, match='as many columns'):
        pa.Solver(eq_p, **kw, **net, model=Wider, **solver_kwargs)
    class BatchStatistics(pa.ConvBlockModel):
        def forward(self, xs):
            return self.conv_block((xs - xs.mean(dim=0)) / xs.std(dim=0))
    with pytest.raises(NotImplementedError, match='batch as a whole'):
        pa.Solver(eq_p, **kw, **net, model=BatchStatistics, **solver_kwargs)
    class Trainable(pa.ConvBlockModel):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            self.stretch = torch.nn.Parameter(torch.tensor(2.0, device=self.flat.device))
        def forward(self, xs):
            return self.conv_block(xs * self.stretch)
    with pytest.raises(NotImplementedError, match='trainable'):
        pa.Solver(eq_p, **kw, **net, model=Trainable, **solver_kwargs)
    if which == 'normalised_inputs':
        # a batch that cannot tell the scale (one point): refused rather than guessed
        with pytest.raises(NotImplementedError):
            solver._input_map(torch.full((1, d), 0.3, device=solver.device))


def test_breadth_streams_and_gradients_match_the_fp64_jets(pa, emu_lib):
    """ the breadth fixture `resnet3` (third derivative; Sin / Tanh / SiLU / Sigmoid; a residual block joining in front of its
    activation and one behind) against oracle/jet_f64.py, the independent fp64 statement of the kernel mathematics that is itself
    pinned to the reference-generated golden (tests/test_oracle_vs_golden.py): every derivative stream, the loss, every gradient """
    from oracle import jet_f64 as jf, problems
    from test_oracle_vs_golden import make_spec
    g = Golden('resnet3')
    _, solver = make_solver('resnet3', pa, **emu_kwargs(emu_lib))
    load_params(solver, g.params)
    sf, spec = make_spec(g)
    pts = g.points[0]
    ic64 = problems.ic_streams_f64('resnet3', pts, sf['dir_cols'], sf['n2'], sf.get('n3', 0))
    out = jf.step(spec, pts, sf['residual'], ic64)
    xs = torch.from_numpy(pts.copy())
    n2p = sf['n2'] | (sf.get('n3', 0) << 3)
    streams = solver.model.net.jet_forward(solver.model.flat, xs, sf['dir_cols'], n2p,
                                           ic_streams=torch.from_numpy(ic64.astype(np.float32)).contiguous())
    for s_idx in range(spec.S):
        assert rel_l2(streams[s_idx].numpy(), out['u_streams'][s_idx]) < 2e-5, s_idx
    solver._fused_step(xs, 1)
    lay = solver.model.net.layout
    assert abs(float(solver.grads[lay.off_loss]) - out['loss']) <= 1e-5 * out['loss']
    flat = [t for pair in zip(out['dW'], out['db']) for t in pair]
    for got, want in zip(export_grads(solver), flat):
        assert rel_l2(got, want) < 2e-5
    assert abs(float(export_grads(solver)[-1]) - out['dlog_scale']) <= 2e-5 * max(1.0, abs(out['dlog_scale']))


def test_chunked_fit_equals_the_per_iteration_loop(pa, emu_lib):
    """ Solver.fit on the common path -- device sampler, one equation term, Adam -- enqueues chunks of iterations through ONE
    library call (pinn_fit_steps; reference loop model_torch.py:426-464). Same Philox batches, same Adam steps, same loss
    history as the per-iteration loop, bit for bit; a seeded NumpySampler keeps counting its own batches across the chunks. """
    def run(chunk, per_iteration, sampler_of):
        torch.manual_seed(77)
        cfg, solver = make_solver('cfg4', pa, **emu_kwargs(emu_lib))
        solver.FIT_CHUNK = chunk
        if per_iteration:
            solver._device_columns = lambda sampler: None
        sampler = sampler_of()
        solver.fit(niters=5, batch_size=40, sampler=sampler, lr=0.01)
        solver.fit(niters=2, batch_size=40, sampler=sampler, lr=0.01, optimizer=None)
        return np.array([float(v) for v in solver.losses]), export_params(solver)
    for sampler_of in (lambda: None, lambda: pa.NumpySampler('uniform', seed=5) & pa.NumpySampler('uniform', low=1, high=5, seed=6)):
        want_l, want_p = run(128, True, sampler_of)
        for chunk in (128, 2):
            got_l, got_p = run(chunk, False, sampler_of)
            assert np.array_equal(got_l, want_l), chunk
            for a, b in zip(got_p, want_p):
                assert np.array_equal(a, b), chunk


def test_wide_sin_net_takes_the_static_activation_kernel(pa, emu_lib):
    _wide_sin_case(pa, 128, emu_kwargs(emu_lib), 40, emu_lib)


def _wide_sin_case(pa, hp, solver_kwargs, n, lib=None):
    """ round 6: 'Sin' nets of the streamed widths (>= 128) without skips on the Dirichlet-box shape run on a tile kernel with the activation fixed at compile
    time (VAR 16 | 128, ACTC = Sin) instead of the full breadth kernel's run-time activation code; the weight gradients come from the HEAVY partner as before """
    from oracle import pinn_oracle as po
    feats = [72, 100, 72, 1] if hp == 128 else [200, 256, 136, 1]

    def problem(D):
        eq = lambda f, x, y: D(D(f, x), x) + D(D(f, y), y) - 5 * torch.sin(np.pi * (x + y))
        return eq, dict(ndims=2, boundary_condition=1, layout='fa fa fa f', features=feats, activation='Sin')
    torch.manual_seed(6)
    eq_o, kw = problem(po.D)
    oracle = po.OracleSolver(eq_o, **kw)
    eq_p, kw = problem(pa.D)
    solver = pa.Solver(eq_p, **kw, **solver_kwargs)
    load_params(solver, oracle.export_params())
    pts = np.random.RandomState(9).rand(2, n, 2).astype(np.float32)
    oracle.fit(niters=2, batch_size=n, points=pts, lr=0.005)
    solver.fit(niters=2, batch_size=n, sampler=FixedBatches(pts), lr=0.005)
    lib = lib or solver.model.net.lib
    assert lib.pinn_last_kernel_name().decode() == f'pinn_tile_kernel<{hp},2,1,1,-1,2,true,144>', lib.pinn_last_kernel_name().decode()
    assert lib.pinn_last_wgrad_kernel_name().decode().startswith(f'pinn_wgrad_kernel<{hp},2,1,true,1,false,true,true')
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=2e-5)
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 2e-5)


@pytest.mark.parametrize('bc', [1, None])
def test_sin_net_of_depth_four_takes_the_static_kernel(pa, emu_lib, bc):
    """ 4 x 64 'Sin' nets (reference model_torch.py:158-168 takes any activation name) run on instantiations with the depth and
    the activation fixed -- register-resident weight gradients instead of read-modify-write rows (round 3, the worst breadth
    workload) -- with the Dirichlet-box shape facts fixed where they apply (bc = 1) and without (no boundary condition). """
    from oracle import pinn_oracle as po

    def problem(D):
        eq = lambda f, x, y: D(D(f, x), x) + D(D(f, y), y) - 5 * torch.sin(np.pi * (x + y))
        kw = dict(ndims=2, layout='fa fa fa fa f', features=[64, 64, 64, 64, 1], activation='Sin')
        if bc is not None:
            kw['boundary_condition'] = bc
        return eq, kw
    torch.manual_seed(4)
    eq_o, kw = problem(po.D)
    oracle = po.OracleSolver(eq_o, **kw)
    eq_p, kw = problem(pa.D)
    solver = pa.Solver(eq_p, **kw, **emu_kwargs(emu_lib))
    load_params(solver, oracle.export_params())
    pts = np.random.RandomState(8).rand(2, 50, 2).astype(np.float32)
    oracle.fit(niters=2, batch_size=50, points=pts, lr=0.005)
    solver.fit(niters=2, batch_size=50, sampler=FixedBatches(pts), lr=0.005)
    name = emu_lib.pinn_last_kernel_name().decode()
    assert name == ('pinn_tile_kernel<64,2,1,1,3,2,true,272>' if bc is not None else 'pinn_tile_kernel<64,2,1,1,3,2,true,8>'), name    # (round 6: the box shape as two teams)
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=2e-5)
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 2e-5)


def _wide512_problems(D, torch, which):
    """ hidden widths beyond 256 (the reference takes any `features`, model_torch.py:158-168): padded to 512 """
    if which == 'ode_fused':          # one direction with its second derivative: ONE kernel call (S = 3), fused step path
        eq = lambda f, x: D(D(f, x), x) + f - torch.sin(3.0 * x)
        return eq, dict(ndims=1, boundary_condition=0.2, layout='fa fa f', features=[300, 300, 1], activation='Tanh'), 'fused'
    if which == 'poisson_groups':     # two second-order directions: one kernel call each (generic path)
        eq = lambda f, x, y: D(D(f, x), x) + D(D(f, y), y) - 5 * torch.sin(np.pi * (x + y))
        return eq, dict(ndims=2, boundary_condition=1, layout='fa fa fa f', features=[264, 320, 264, 1], activation='Tanh'), 'generic'
    if which == 'heat_sigmoid':       # IC + BC, a second-order and a first-order direction (two calls), Sigmoid
        eq = lambda f, x, t: D(f, t) - 0.2 * D(D(f, x), x)
        return eq, dict(ndims=2, boundary_condition=0.0, initial_condition=lambda x: torch.sin(np.pi * x), layout='fa fa f', features=[512, 512, 1],
                        activation='Sigmoid'), 'generic'
    # first breadth set: Sin / GELU layers and a skip connection at width 512
    eq = lambda f, x, y: D(f, x) + 0.5 * D(f, y) - f * f
    return eq, dict(ndims=2, boundary_condition=0.3, layout='faR fa fa+ f', features=[288, 288, 288, 1], activation=['Sin', 'GELU', 'Tanh']), 'fused'


@pytest.mark.parametrize('which', ['ode_fused', 'poisson_groups', 'heat_sigmoid', 'advection_breadth'])
def test_hidden_width_512_matches_the_oracle(pa, emu_lib, which):
    # (a 512-wide net costs the emulator a minute or more per tile: ONE case in the CPU tier, all four with PYDENS_AMD_SLOW_EMU=1 -- and on the device,
    #  tests/test_gpu_parity.py::test_hidden_width_512_on_the_gpu)
    if which != 'ode_fused' and os.environ.get('PYDENS_AMD_SLOW_EMU') != '1':
        pytest.skip('slow on the emulator: PYDENS_AMD_SLOW_EMU=1, or the -m gpu twin')
    _wide512_case(pa, which, emu_kwargs(emu_lib), 16)


def _wide512_case(pa, which, solver_kwargs, n):
    """ round 6: widths 257 .. 512 run on kernels of their own -- S <= 3 streams per call (LDS), anything larger in direction groups, eight
    bias-gradient rows, the streamed weight-gradient kernel in four 256 x 256 block passes
    (the loops of that path -- second tiles, ragged tiles, all 512 units, eight layers, every instantiation: tests/test_width_512.py) """
    from oracle import pinn_oracle as po
    torch.manual_seed(53)
    eq_o, kw, path = _wide512_problems(po.D, torch, which)
    oracle32 = po.OracleSolver(eq_o, **kw)
    oracle = po.OracleSolver(eq_o, dtype=torch.float64, **kw)
    start = oracle32.export_params()
    oracle.import_params(start)
    eq_p, kw, _ = _wide512_problems(pa.D, torch, which)
    solver = pa.Solver(eq_p, **kw, **solver_kwargs)
    assert solver.model.net.layout.hp == 512
    assert (solver.program is not None) == (path == 'fused'), solver.program_error
    load_params(solver, start)
    d = kw['ndims']
    pts = np.random.RandomState(21).rand(3, n, d).astype(np.float32)
    ev32, g32 = oracle32.evaluate(pts[0]), oracle32.export_grads()
    ev, g_want = oracle.evaluate(pts[0]), oracle.export_grads()
    xs = torch.from_numpy(pts[0].copy()).to(solver.device)
    if path == 'fused':
        solver._fused_step(xs, 1)
    else:
        solver._generic_step(xs, ('equation',), [], torch.nn.MSELoss(), 1)
    lay = solver.model.net.layout
    loss = float(solver.grads[lay.off_loss])
    assert abs(loss - ev['loss']) <= max(2 * abs(ev32['loss'] - ev['loss']), 1e-5 * ev['loss']), (loss, ev['loss'], ev32['loss'])
    for got, want, w32 in zip(export_grads(solver), g_want, g32):
        if want is not None:
            err = np.linalg.norm(np.asarray(got, dtype=np.float64) - want)
            assert err <= max(2 * np.linalg.norm(np.asarray(w32, dtype=np.float64) - want), 1e-5 * np.linalg.norm(want)), (which, err)
    oracle32.fit(niters=2, batch_size=n, points=pts[1:], lr=0.002)
    solver.fit(niters=2, batch_size=n, sampler=FixedBatches(pts[1:]), lr=0.002)
    assert solver.last_fit_path == path
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle32.losses], rtol=5e-5)
    for got, want in zip(export_params(solver), oracle32.export_params()):
        assert params_close(got, want, 5e-5, atol=5e-6)
    cols = [pts[0][:, i] for i in range(d)]
    assert np.abs(solver.predict(*cols) - oracle32.predict(*cols)).max() < 2e-5


def _evolution_problems(D, torch, which):
    """ (x, t) problems on a 4 x 64 Tanh net: boundary binding in x, initial condition in t (PinnShape 2) """
    kw = dict(ndims=2, boundary_condition=0.1, initial_condition=lambda x: torch.sin(np.pi * x), layout='fa fa fa fa f', features=[64, 64, 64, 64, 1],
              activation='Tanh')
    if which == 'heat':           # affine residual, one second derivative beside u_t: the combined second-order stream
        return (lambda f, x, t: D(f, t) - 0.3 * D(D(f, x), x) - 2.0 * torch.exp(-t) * torch.sin(np.pi * x)), kw
    if which == 'wave':           # second derivatives in both columns
        return (lambda f, x, t: D(D(f, t), t) - 0.5 * D(D(f, x), x)), kw
    return (lambda f, x, t: D(f, t) + f * D(f, x) - 0.05 * D(D(f, x), x)), kw            # viscous Burgers: residual program


@pytest.mark.parametrize('which', ['heat', 'wave', 'burgers'])
def test_evolution_shape_in_x_t_takes_the_two_team_kernels(pa, emu_lib, which):
    _evolution_case(pa, which, emu_kwargs(emu_lib), 50, emu_lib)


def _evolution_case(pa, which, solver_kwargs, n, lib=None):
    """ round 6: heat / wave / Burgers in one space dimension on the 4 x 64 Tanh net run on two-team twins of the Poisson-box kernel
    (VAR 256 | 32: PinnShape 2; | 2048 with a residual program) instead of the general one-wave-per-SIMD kernel """
    from oracle import pinn_oracle as po
    torch.manual_seed(31)
    eq_o, kw = _evolution_problems(po.D, torch, which)
    oracle = po.OracleSolver(eq_o, **kw)
    eq_p, kw = _evolution_problems(pa.D, torch, which)
    solver = pa.Solver(eq_p, **kw, **solver_kwargs)
    assert solver.program is not None, solver.program_error
    load_params(solver, oracle.export_params())
    pts = np.random.RandomState(12).rand(2, n, 2).astype(np.float32)
    oracle.fit(niters=2, batch_size=n, points=pts, lr=0.005)
    solver.fit(niters=2, batch_size=n, sampler=FixedBatches(pts), lr=0.005)
    name = (lib or solver.model.net.lib).pinn_last_kernel_name().decode()
    assert name == ('pinn_tile_kernel<64,2,1,1,3,0,true,2336>' if which == 'burgers' else 'pinn_tile_kernel<64,2,1,1,3,0,true,288>'), name
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=2e-5)
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 2e-5)


@pytest.mark.parametrize('name', ['w16_program', 'w32_affine', 'w32_generic', 'w32_third_order', 'w100_heat', 'program', 'generic'])
def test_the_large_batch_gpu_cases_on_a_few_points(pa, emu_lib, name):
    """ tests/test_gpu_occupancy.py runs these problems at 131 072 points on full grids of the device; here the same body (oracle
    parity, four bit-identical repeats, the workgroups-per-CU cap, pinn_last_launch_info) on the emulator with a handful of points """
    import test_gpu_occupancy as tg
    info = tg.run_case(pa, name, 80 if name != 'w100_heat' else 40, solver_kwargs=emu_kwargs(emu_lib), on_device=False)
    assert info['grid'] >= 1 and info['threads'] in (64, 128, 256, 512) and info['per_cu'] >= 1


@pytest.mark.parametrize('which', ['affine', 'program'])
def test_one_second_derivative_beside_three_first_order_directions(pa, emu_lib, which):
    """ four differentiation directions with exactly ONE second derivative (`u_t + u_y + u_z = nu u_xx` in four variables)
    exist as the combined second-order stream only; pinn_workspace_bytes used to plan the combined form from two second derivatives
    on and answered 0 bytes for this shape ('workspace too small'). Affine and program residuals against the oracle. """
    from oracle import pinn_oracle as po

    def problem(D):
        if which == 'affine':
            return lambda f, x, y, z, t: D(f, t) + D(f, y) + D(f, z) - 0.1 * D(D(f, x), x)
        return lambda f, x, y, z, t: D(f, t) + D(f, y) + f * D(f, z) - 0.1 * D(D(f, x), x)
    kw = dict(ndims=4, boundary_condition=0.5, initial_condition=lambda x, y, z: torch.sin(np.pi * x) * y * z,
              layout='fa fa f', features=[20, 20, 1], activation='Tanh')
    oracle = po.OracleSolver(problem(po.D), **kw)
    solver = pa.Solver(problem(pa.D), **kw, **emu_kwargs(emu_lib))
    assert solver.program is not None, solver.program_error
    assert solver.residual_plan.comb_w is not None and solver.residual_plan.n_streams == 6
    load_params(solver, oracle.export_params())
    pts = np.random.RandomState(5).rand(3, 40, 4).astype(np.float32)
    solver.fit(niters=3, batch_size=40, sampler=FixedBatches(pts), lr=0.01)
    oracle.fit(niters=3, batch_size=40, points=pts, lr=0.01)
    assert solver.last_fit_path == 'fused'
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=2e-5)
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 2e-5)


@pytest.mark.parametrize('case', ['cfg2', 'cfg2_bf16x3', 'cfg4', 'cfg3_streamed'])      # (wide skip kernels under shuffling: tools/experiments/r05_alternating_gz_check.py runs them)
def test_results_do_not_depend_on_the_order_the_waves_run_in(pa, emu_lib, case, monkeypatch):
    """ the emulator normally advances the waves of a workgroup round-robin, which hides a missing barrier; under PINN_EMU_SHUFFLE=<seed>
    they advance in random order, whole phases apart up to the next barrier (tests/emu/emu_runtime.cpp). Every gradient of a fused step
    must come out bit-identical to the round-robin run -- two-team, split-bf16, streamed weight-gradient and skip kernels.
    (Negative control: tools/emu_shuffle_check.py -DPINN_ABL=16, the same kernels built without the tile loop's barriers, differs by
    O(10) under every seed.) """
    def run(shuffle):
        if shuffle:
            monkeypatch.setenv('PINN_EMU_SHUFFLE', str(shuffle))
        else:
            monkeypatch.delenv('PINN_EMU_SHUFFLE', raising=False)
        torch.manual_seed(0)
        if case == 'wide_skip_any_activation':
            eq, kw = _layout_problems(pa.D, torch, 'burgers', dict(layout='fRa fa f+a R f fa+ fa f', features=[96] * 6 + [1],
                                                                  activation=['Sin', 'SiLU', 'GELU', 'Softplus', 'Tanh']))
            solver = pa.Solver(eq, **kw, **emu_kwargs(emu_lib))
            pts = torch.from_numpy(np.random.RandomState(1).rand(40, 2).astype(np.float32))
        else:
            name = case.split('_')[0]
            cfg, solver = make_solver(name, pa, **emu_kwargs(emu_lib))
            if case.endswith('bf16x3'):
                solver.set_gemm_mode('bf16x3')
            pts = torch.from_numpy(pc.sample_points(cfg, 40 if name == 'cfg3' else 150, seed=1))
        solver._fused_step(pts, 1)
        return solver.grads.clone().numpy()
    want = run(0)
    for seed in (1,):           # (tools/emu_shuffle_check.py runs more seeds; a stalled wave costs the emulator many idle passes)
        assert np.array_equal(run(seed), want), seed


def test_second_kernel_set_splits_large_stream_shapes_into_direction_groups(pa, emu_lib):
    """ round 5: nets with activation codes above 7 / nested skips run on the SECOND set of full breadth kernels, built for the stream
    shapes of one or two directions per call (pinn_inst.inc PINN_ALLACT_SHAPES). A non-affine equation over three differentiated
    columns (separate second-order streams: shape (3, 2)) has no single-call kernel there: the tracer must say so and the generic
    path must serve it through direction groups -- same trajectory as the oracle. The affine heat operator over the same columns
    stays fused (ONE combined second-order stream over three directions is in the set). """
    from oracle import pinn_oracle as po
    net = dict(layout='fa fa f', features=[12, 12, 1], activation=['ELU', 'Mish'])

    def problems(D):
        nonaffine = lambda f, x, y, t: D(f, t) - (1.0 + f * f) * D(D(f, x), x) - D(D(f, y), y)
        affine = lambda f, x, y, t: D(f, t) - 0.3 * D(D(f, x), x) - 0.2 * D(D(f, y), y) - 1.0
        kw = dict(ndims=3, boundary_condition=0.1, initial_condition=lambda x, y: torch.sin(np.pi * x) * y, **net)
        return (nonaffine, kw), (affine, kw)

    pts = np.random.RandomState(12).rand(3, 24, 3).astype(np.float32)
    for which, want_path in ((0, 'generic'), (1, 'fused')):
        eq_o, kw = problems(po.D)[which]
        oracle = po.OracleSolver(eq_o, **kw)
        start = oracle.export_params()
        oracle.fit(niters=3, batch_size=24, points=pts, lr=0.01)
        eq_p, kw = problems(pa.D)[which]
        solver = pa.Solver(eq_p, **kw, **emu_kwargs(emu_lib))
        assert solver.model.net.allact
        load_params(solver, start)
        solver.fit(niters=3, batch_size=24, sampler=FixedBatches(pts), lr=0.01)
        assert solver.last_fit_path == want_path, (solver.last_fit_path, solver.program_error)
        if want_path == 'generic':
            assert 'several kernel calls' in solver.program_error and len(solver.spec.groups) > 1
        assert emu_lib.pinn_last_kernel_name().decode().split(',')[5] == '-2'
        np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=3e-5)
        for got, want in zip(export_params(solver), oracle.export_params()):
            assert params_close(got, want, 3e-5)


def _fourth_order_problems(D, torch, which):
    if which == 'beam_1d':            # u'''' + u = f(x) on a clamped interval (beam on an elastic foundation): ONE kernel call carries u .. u'''' (packed 73)
        # (the `+ f` matters to the TEST: without it the last bias has an exactly zero gradient and Adam turns fp noise into +-lr steps)
        eq = lambda f, x: D(D(D(D(f, x), x), x), x) + f - 24.0 * torch.cos(2.0 * x)
        return eq, dict(ndims=1, boundary_condition=0.1, layout='fa fa f', features=[16, 16, 1], activation='Tanh')
    if which in ('beam_wide', 'beam_wide_sin'):      # widths >= 128: streamed weight gradients (pinn_wgrad_kernel rebuilds h'''' from the saved jets)
        eq = lambda f, x: D(D(D(D(f, x), x), x), x) + f - 24.0 * torch.cos(2.0 * x)
        acts = ['Tanh', 'Sigmoid', 'Tanh'] if which == 'beam_wide' else ['Sin', 'Softplus', 'Tanh']
        return eq, dict(ndims=1, boundary_condition=0.1, layout='fa fa fa f', features=[72, 72, 72, 1], activation=acts)
    if which == 'kuramoto_sivashinsky':   # u_t + u_xxxx + u_xx + u u_x in (x, t): fourth-order direction in a group of its own, IC gate + BC
        eq = lambda f, x, t: D(f, t) + 0.02 * D(D(D(D(f, x), x), x), x) + 0.1 * D(D(f, x), x) + f * D(f, x)
        return eq, dict(ndims=2, boundary_condition=0.0, initial_condition=lambda x: torch.sin(np.pi * x), layout='fa fa f', features=[20, 20, 1],
                        activation='Tanh')
    if which == 'time_fourth':        # fourth derivative along the TIME column: the gate's fourth derivative and its log_scale adjoint (sigmoid's fifth)
        eq = lambda f, x, t: 0.05 * D(D(D(D(f, t), t), t), t) + D(f, x) - f
        return eq, dict(ndims=2, boundary_condition=0.2, initial_condition=0.7, layout='fa fa f', features=[16, 16, 1], activation='Sigmoid')
    if which == 'xxxt_gate':          # round 6: u_xxxt and u_xttt in (x, t) with IC + BC -- weighted diagonals 2x + t, 2x - t: the box factor's column counts
        # twice (A1 = 2 p', A2 = 4 p''), the gate's time column carries the sign of the minus diagonals to odd orders
        eq = lambda f, x, t: D(f, t) + 0.02 * D(D(D(D(f, x), x), x), t) - 0.01 * D(D(D(D(f, t), t), t), x) + f * D(f, x)
        return eq, dict(ndims=2, boundary_condition=0.1, initial_condition=lambda x: torch.sin(np.pi * x), layout='fa fa f', features=[16, 16, 1],
                        activation='Tanh')
    if which == 'tttp_gate':          # ... u_tttp with a parameter column p behind t: the weighted diagonals 2t + p, 2t - p put weight 2 on the TIME column
        # (the gate's n-th derivative carries 2^n, so does its log_scale adjoint)
        eq = lambda f, x, t, p: D(f, t) + 0.01 * D(D(D(D(f, t), t), t), p) + 0.02 * D(D(D(D(f, p), p), p), t) - p * D(D(f, x), x)
        return eq, dict(ndims=2, nparams=1, boundary_condition=0.2, initial_condition=0.5, layout='fa fa f', features=[16, 16, 1], activation='Sigmoid')
    if which == 'biharmonic':         # u_xxxx + 2 u_xxyy + u_yyyy = f: the mixed one from fourth derivatives along x + y and x - y
        eq = lambda f, x, y: D(D(D(D(f, x), x), x), x) + 2.0 * D(D(D(D(f, x), x), y), y) + D(D(D(D(f, y), y), y), y) - torch.sin(np.pi * x) * y
        return eq, dict(ndims=2, boundary_condition=0.0, layout='fa fa f', features=[16, 16, 1], activation='Tanh')
    # activations of the second kernel set, a skip connection and an identity layer: every fifth derivative formula on the reverse sweep
    eq = lambda f, x: D(D(D(D(f, x), x), x), x) + D(D(f, x), x) - torch.exp(-x)
    return eq, dict(ndims=1, boundary_condition=0.3, layout='faR fa f+a fa f', features=[12, 12, 12, 12, 1], activation=['Mish', 'Softsign', 'GELU', 'SiLU'])


@pytest.mark.parametrize('which', ['beam_1d', 'kuramoto_sivashinsky', 'time_fourth', 'biharmonic', 'any_activation', 'beam_wide', 'beam_wide_sin', 'xxxt_gate',
                                   'tttp_gate'])
def test_fourth_order_streams_match_the_oracle(pa, emu_lib, which):
    _fourth_order_case(pa, which, emu_kwargs(emu_lib))


def _fourth_order_case(pa, which, solver_kwargs):
    """ round 5: u_xxxx-type equations (the reference nests D to any order, model_torch.py:174-178) -- a fourth Taylor coefficient per
    direction in the jets, the ansatz product rules to fourth order (box factor incl. its mixed fourth derivative along a diagonal, IC
    gate and its log_scale adjoint), the reverse sweep with the activation's FIFTH derivative; one fourth-order direction per kernel call,
    generic step path. Four nested fp32 autograd sweeps of the reference are noisy: the fp64 oracle arbitrates. """
    from oracle import pinn_oracle as po
    eq_o, kw = _fourth_order_problems(po.D, torch, which)
    oracle32 = po.OracleSolver(eq_o, **kw)
    oracle = po.OracleSolver(eq_o, dtype=torch.float64, **kw)
    start = oracle32.export_params()
    oracle.import_params(start)
    d = kw['ndims'] + kw.get('nparams', 0)
    pts = np.random.RandomState(14).rand(3, 40, d).astype(np.float32)
    ev32, g32 = oracle32.evaluate(pts[0]), oracle32.export_grads()
    ev, g_want = oracle.evaluate(pts[0]), oracle.export_grads()
    oracle.fit(niters=3, batch_size=40, points=pts, lr=0.01)
    eq_p, kw = _fourth_order_problems(pa.D, torch, which)
    solver = pa.Solver(eq_p, **kw, **solver_kwargs)
    assert solver.spec.n4 >= 1 and solver.program is None
    want_groups = {'beam_1d': [73], 'kuramoto_sivashinsky': [73, 0], 'time_fourth': [73, 0], 'biharmonic': [73, 73, 73, 73], 'any_activation': [73], 'beam_wide': [73],
                   'beam_wide_sin': [73], 'xxxt_gate': [73, 73, 73, 73, 9, 9], 'tttp_gate': [73, 73, 73, 73, 9, 9, 1]}[which]
    assert [g[1] for g in solver.spec.groups] == want_groups, solver.spec.groups
    if which.endswith('_gate'):
        assert [c for c in solver.spec.dir_cols if c & 0x200], solver.spec.dir_cols          # PINN_DIR_DOUBLE directions are in play
    load_params(solver, start)
    solver._generic_step(torch.from_numpy(pts[0].copy()).to(solver.device), ('equation',), [], torch.nn.MSELoss(), 1)
    lay = solver.model.net.layout
    loss = float(solver.grads[lay.off_loss])
    assert abs(loss - ev['loss']) <= max(2 * abs(ev32['loss'] - ev['loss']), 1e-5 * ev['loss']), (loss, ev['loss'], ev32['loss'])
    for got, want, w32 in zip(export_grads(solver), g_want, g32):
        if want is not None:
            err = np.linalg.norm(np.asarray(got, dtype=np.float64) - want)
            assert err <= max(2 * np.linalg.norm(np.asarray(w32, dtype=np.float64) - want), 1e-4 * np.linalg.norm(want)), (which, err)
    solver.fit(niters=3, batch_size=40, sampler=FixedBatches(pts), lr=0.01)
    assert solver.last_fit_path == 'generic'
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=1e-4)
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 2e-4, atol=2e-5)
    xs = [pts[0][:, i] for i in range(d)]
    assert np.abs(solver.predict(*xs) - oracle.predict(*xs)).max() < 2e-5


# ---- a chunk of fit iterations as ONE launch on ONE CU (pinn_fit_kernel.h, round 5) ---------------------------------------------------
def _one_launch_problem(pa, which, kw):
    """ -> (solver, sampler, batch): narrow nets at the reference's own batch sizes """
    if which in ('cfg1', 'one_point'):
        return make_solver('cfg1', pa, **kw)[1], None, (100 if which == 'cfg1' else 1)
    if which == 'ode_16':                      # generic kernel of width 16 (program registers in every virtual workgroup's LDS block), 25 tiles
        eq = lambda f, x: pa.D(f, x) - 2 * np.pi * torch.cos(2 * np.pi * x)
        return pa.Solver(eq, ndims=1, initial_condition=0.5, layout='fa fa f', features=[10, 12, 1], activation='Tanh', **kw), None, 400
    if which == 'ode_default_net':             # tutorial cells 28-31: default net (20, 30 units -> width 32: TWO waves per virtual workgroup)
        eq = lambda f, x, e: pa.D(f, x) - e * np.pi * torch.cos(e * np.pi * x)
        return (pa.Solver(eq, ndims=1, initial_condition=2.0, nparams=1, **kw),
                pa.NumpySampler('u') & pa.NumpySampler('u', low=.5, high=5.5), 100)
    if which == 'program_with_variable':       # residual program with a trainable coefficient
        eq = lambda f, x, y: pa.D(pa.D(f, x), x) + pa.D(pa.D(f, y), y) + pa.V('k', data=torch.Tensor([1.5])) * f * f - torch.sin(np.pi * (x + y))
        return pa.Solver(eq, ndims=2, boundary_condition=1, layout='fa fa f', features=[16, 16, 1], activation='Tanh', **kw), None, 90
    assert which == 'skip_sin'                 # breadth kernel: skip connection, Sin / Tanh / Sigmoid
    eq = lambda f, x, y: pa.D(pa.D(f, x), x) + pa.D(pa.D(f, y), y) - torch.sin(np.pi * (x + y))
    return pa.Solver(eq, ndims=2, boundary_condition=1, layout='faR fa fa+ f', features=[16, 16, 16, 1], activation=['Sin', 'Tanh', 'Sigmoid'], **kw), None, 60


def _one_launch_case(pa, which, kw, monkeypatch, mode, niters, lib, rounds=4):
    """ Solver.fit with every chunk as one launch (mode 2: one hardware workgroup of virtual workgroups on one CU, mode 1: a grid with a
    device-scope wait) against the eager loop: same Philox batches, same Adam scalars; the sums over the partial rows may group the tiles
    differently (another number of rows) and the tile pass is compiled into another kernel (FMA contraction): fp32 round-off apart. """
    def run(m):
        monkeypatch.setenv('PYDENS_AMD_FIT_PERSIST', str(m))
        monkeypatch.setenv('PYDENS_AMD_FIT_ROUNDS', str(rounds))
        monkeypatch.setenv('PYDENS_AMD_FIT_GRAPH', '1')
        torch.manual_seed(31)
        solver, sampler, batch = _one_launch_problem(pa, which, kw)
        assert solver.model.net.layout.hp <= 32
        st0 = (ctypes.c_int32 * 4)()
        lib.pinn_debug_fit_graph_stats(st0)
        solver.fit(niters=niters[0], batch_size=batch, sampler=sampler, lr=0.005)
        solver.fit(niters=niters[1], batch_size=batch, sampler=sampler, lr=0.005, optimizer=None)      # continues
        assert solver.last_fit_path == 'fused', solver.program_error
        st = (ctypes.c_int32 * 4)()
        lib.pinn_debug_fit_graph_stats(st)
        return (np.array([float(v) for v in solver.losses]), solver.model.flat.detach().cpu().numpy().copy(),
                solver.optimizer.exp_avg.cpu().numpy().copy(), solver.optimizer.exp_avg_sq.cpu().numpy().copy(),
                int(solver.optimizer.step_count.item()), solver.grads.cpu().numpy().copy(), lib.pinn_last_kernel_name().decode(), st[0] - st0[0])
    l0, p0, m0, v0, t0, g0, k0, n0 = run(0)
    l1, p1, m1, v1, t1, g1, k1, n1 = run(mode)
    assert k0.startswith('pinn_tile_kernel<'), k0
    assert k1.startswith('pinn_fit_kernel<') and (k1.endswith(',1>') == (mode == 1)), k1
    chunks = sum((n + 127) // 128 for n in niters)
    assert n1 >= chunks                          # every chunk went out as one launch (n0: the chunks the eager run replayed as launch graphs)
    assert t0 == t1 == sum(niters) and np.isfinite(l1).all()
    np.testing.assert_allclose(l1[:8], l0[:8], rtol=2e-6)
    np.testing.assert_allclose(l1, l0, rtol=2e-4)
    assert params_close(p1, p0, 2e-4) and params_close(m1, m0, 2e-3, atol=1e-7) and params_close(v1, v0, 2e-3, atol=1e-9)
    assert params_close(g1, g0, 5e-3, atol=1e-6)


@pytest.mark.parametrize('which', ['cfg1', 'one_point', 'ode_16', 'ode_default_net', 'program_with_variable', 'skip_sin'])
def test_fit_chunk_on_one_cu_follows_the_eager_loop(pa, emu_lib, which, monkeypatch):
    monkeypatch.setattr(pa.Solver, 'FIT_CTRL_ON_HOST', True)
    _one_launch_case(pa, which, emu_kwargs(emu_lib), monkeypatch, 2, (5, 3), emu_lib)


def test_callable_ic_beside_a_parameter_column_is_lowered(pa, emu_lib):
    """ tutorial cells 37-40 (heat equation with the diffusivity as a sampled parameter, callable IC): the IC and its derivative streams
    must join the x-only pre-pass -- no torch autograd per iteration. Round 5 regression: the tracer's emitter memoised registers by
    id(node) without keeping the nodes; the temporaries of the coefficient row (-a) died, the IC's derivative nodes were handed their
    ids and registers, the validation against the callable refused the lowering, and every iteration paid ~0.45 ms of torch autograd. """
    eq = lambda f, x, y, t, a: pa.D(pa.D(f, x), x) + pa.D(pa.D(f, y), y) - a * pa.D(f, t)
    solver = pa.Solver(eq, ndims=3, nparams=1, initial_condition=lambda x, y: 10 * x * y * (1 - x) * (1 - y), boundary_condition=0,
                       layout='fafaf', features=[30, 24, 1], activation='Sigmoid', **emu_kwargs(emu_lib))
    assert solver.program is not None, solver.program_error
    assert solver.ic_lowering_error is None and solver.residual_plan.ic_row is not None
    assert not solver._needs_ic_streams()
    sampler = pa.NumpySampler('u', dim=2) & pa.NumpySampler('u', low=0, high=.5) & pa.NumpySampler('u', low=.1, high=4)
    assert solver._device_columns(sampler) is not None
    # and the lowered rows are the callable's streams (the validation the solver ran, once more, on other points)
    from pydens_amd import trace
    pts = torch.rand((9, 4), dtype=torch.float32) * 0.5 + 0.2
    want = solver._ic_stream_tensor(pts, solver.residual_plan.comb_w).double().numpy()
    got = trace.run_ic_numpy(solver.residual_plan, pts.numpy().astype(np.float64))
    assert np.allclose(got, want, rtol=1e-5, atol=1e-6)
    solver.fit(niters=3, batch_size=40, sampler=sampler, lr=0.005)
    assert solver.last_fit_path == 'fused' and np.isfinite([float(v) for v in solver.losses]).all()


def _wide_prepass_case(pa, kw):
    """ an x-only pre-pass whose program keeps more registers alive than the activation buffers hold for a whole workgroup of points:
    width 16, no derivative streams (S = 1: 768 floats of buffers, 64 threads -> room for 12 registers per lane), a source term with ten
    shared sub-terms (16 registers) -- the kernel then runs the pre-pass over fewer points per sweep (48 lanes) instead of falling back to
    private registers (round 5: the select between the two made every register access a flat instruction) """
    from oracle import pinn_oracle as po
    from pydens_amd import trace

    def mk(D):
        def eq(f, x, y):
            ts = [torch.sin((i + 1) * x) if i % 2 else torch.cos((i + 1) * y) for i in range(10)]
            src = ts[0] * ts[9]
            for i in range(1, 10):
                src = src + ts[i] * ts[9 - i]
            return f - 0.1 * src
        return eq
    net = dict(ndims=2, boundary_condition=0.3, layout='fa fa f', features=[12, 12, 1], activation='Tanh')
    torch.manual_seed(3)
    oracle = po.OracleSolver(mk(po.D), **net)
    solver = pa.Solver(mk(pa.D), **net, **kw)
    assert solver.program is not None, solver.program_error
    code, _ = solver.residual_plan.pre
    two_reg = {trace.OPS[k] for k in ('ADD', 'SUB', 'MUL', 'DIV')}
    nregs = 1 + max(max(w[1], w[2] if w[0] != trace.OPS['CONST'] else 0, w[3] if w[0] in two_reg else 0) for w in code)
    assert nregs > 12, nregs                       # more than a 64-thread sweep has room for
    load_params(solver, oracle.export_params())
    pts = np.random.RandomState(5).rand(3, 100, 2).astype(np.float32)
    oracle.fit(niters=3, batch_size=100, points=pts, lr=0.01)
    solver.fit(niters=3, batch_size=100, sampler=FixedBatches(pts), lr=0.01)
    assert solver.last_fit_path == 'fused'
    np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=2e-5)
    for got, want in zip(export_params(solver), oracle.export_params()):
        assert params_close(got, want, 2e-5)


def test_prepass_with_more_registers_than_a_full_sweep_holds(pa, emu_lib):
    _wide_prepass_case(pa, emu_kwargs(emu_lib))


def test_fit_chunk_that_does_not_fit_one_cu_keeps_the_other_paths(pa, emu_lib, monkeypatch):
    """ the one-CU fit chunk keeps parameters, Adam state and one partial row per virtual workgroup in LDS: a narrow but DEEP net
    (width 32, seven hidden layers: ~7 K parameters) does not fit beside the virtual workgroups' blocks -- the launcher declines and
    the chunk runs as before (launch graphs on the GPU, the eager loop here), same trajectory as with the form switched off """
    monkeypatch.setattr(pa.Solver, 'FIT_CTRL_ON_HOST', True)
    eq = lambda f, x: pa.D(f, x) - 2 * np.pi * torch.cos(2 * np.pi * x)

    def run(mode):
        monkeypatch.setenv('PYDENS_AMD_FIT_PERSIST', str(mode))
        torch.manual_seed(5)
        solver = pa.Solver(eq, ndims=1, initial_condition=0.5, layout='fa' * 7 + 'f', features=[32] * 7 + [1], activation='Tanh',
                           **emu_kwargs(emu_lib))
        solver.fit(niters=4, batch_size=40, lr=0.005)
        return np.array([float(v) for v in solver.losses]), emu_lib.pinn_last_kernel_name().decode()
    l0, k0 = run(0)
    l2, k2 = run(2)
    assert k0.startswith('pinn_tile_kernel<') and k2.startswith('pinn_tile_kernel<'), (k0, k2)
    assert np.array_equal(l0, l2)


def test_first_layer_gradient_in_registers_and_in_lds_side_by_side(pa, emu_lib):
    """ a static-depth kernel with register accumulators (<64,2,2,..,3,TANH>: two separate second-order streams, x-dependent coefficient) on
    FIVE input columns: the first four columns of dW1 and the bias gradients are summed per lane and stored once at the end of the
    workgroup (plain LDS stores since round 5), the fifth column is added in LDS tile by tile -- both land in the same rows """
    from oracle import pinn_oracle as po

    def mk(D):
        return lambda f, x, y, a, b, c: (1 + x) * D(D(f, x), x) + a * D(D(f, y), y) - b * torch.sin(np.pi * (x + y)) + 0.2 * c
    net = dict(ndims=2, nparams=3, boundary_condition=0.5, layout='fa fa fa fa f', features=[64, 64, 64, 64, 1], activation='Tanh')
    torch.manual_seed(3)
    oracle = po.OracleSolver(mk(po.D), **net)
    solver = pa.Solver(mk(pa.D), **net, **emu_kwargs(emu_lib))
    load_params(solver, oracle.export_params())
    pts = (np.random.RandomState(5).rand(70, 5) * np.array([1, 1, 2, 1, 1]) + np.array([0, 0, 1, 0, 0])).astype(np.float32)
    ev, g_want = oracle.evaluate(pts), oracle.export_grads()
    solver._fused_step(torch.from_numpy(pts.copy()), 1)
    assert emu_lib.pinn_last_kernel_name().decode() == 'pinn_tile_kernel<64,2,2,1,3,0,false,0>'
    lay = solver.model.net.layout
    assert abs(float(solver.grads[lay.off_loss]) - ev['loss']) <= 1e-5 * ev['loss']
    grads = export_grads(solver)
    for c in range(5):
        assert rel_l2(grads[0][:, c], g_want[0][:, c]) < 1e-5, c
    for got, want in zip(grads, g_want):
        if want is not None:
            assert grad_close(got, want)
