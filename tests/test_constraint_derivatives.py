""" Constraints that DIFFERENTIATE the model at points of their own choosing (reference model_torch.py:451-457 with `D` inside the
constraint): soft Neumann and Robin conditions, the initial velocity u_t(x, 0) = g(x).

Two routes, both checked against `oracle.pinn_oracle.OracleSolver` (the reference's autograd `D`, fp32 and the fp64 arbiter) at the
project's own bars (helpers.fit_close, GRAD_RTOL):
  * fused   -- constant points: the constraint is lowered to a residual program over the derivative streams of ONE kernel call
               (`constraint_plans[num]` carries `dir_cols` / `n2p` / the IC rows of every stream);
  * generic -- batch points, several direction groups, a model with its own forward(): `f(*args)` comes back tagged, `D` picks kernel
               streams by the identity of its second argument, pinn_jet_backward takes the streams' gradients.
Every case runs on the emulator tier and, marked gpu, on the device. Problems are built by factories `problem(D, V, dtype, device)`, so that
the constraint's own tensors have the engine's dtype (fp64 for the arbiter) and live where the engine computes. """
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch
from torch import nn

from helpers import (FIT_PARAM_RTOL, FixedBatches, GRAD_RTOL, close_or_arbitrated, export_grads, export_params, fit_close, load_params, record_margin)


@pytest.fixture(scope='module')
def emu_lib():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
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


EMU, GPU = ('emu', 'cpu'), ('gpu', 'cuda')


# ---- problems ------------------------------------------------------------------------------------------------------------------------------
ODE = dict(ndims=1, initial_condition=1, layout='fafaf', features=[12, 10, 1], activation='Tanh')
WAVE = dict(ndims=2, initial_condition=lambda x: torch.sin(np.pi * x), boundary_condition=0.0, layout='fafaf', features=[16, 16, 1],
            activation='Tanh')
HEAT = dict(ndims=2, initial_condition=0.5, layout='fafaf', features=[16, 16, 1], activation='Tanh')
DEEP = dict(ndims=2, boundary_condition=0.5, layout='faR fa f+a fa f', features=[64, 64, 64, 64, 1],
            activation=['Tanh', 'Mish', 'Tanh', 'Tanh'])


def neumann_ode(D, V, dtype, device='cpu'):
    """ case 1: u'(1) = 2 at one fixed point """
    def eq(f, x):
        return D(f, x) - 2 * np.pi * torch.cos(2 * np.pi * x)

    def neumann(f, x):
        p = torch.tensor([[1.0]], dtype=dtype, device=device, requires_grad=True)
        return D(f(p), p) - 2.0
    return eq, neumann


def wave_velocity(D, V, dtype, device='cpu'):
    """ case 2: initial velocity u_t(x, 0) = v0 * x on a fixed grid of 5 x; t0 is a leaf of zeros -- on the face t = 0 the gate
    sigmoid(0) - 1/2 vanishes and only the derivative stream holds the network and log_scale """
    xg = torch.linspace(0.1, 0.9, 5, dtype=dtype, device=device).reshape(-1, 1)

    def eq(u, x, t):
        return D(D(u, t), t) - 0.5 * D(D(u, x), x)

    def velocity(f, x, t):
        t0 = torch.zeros((5, 1), dtype=dtype, device=device, requires_grad=True)
        return D(f(xg, t0), t0) - V('v0', data=torch.tensor([0.3], dtype=dtype, device=device)) * xg
    return eq, velocity


def wave_robin(D, V, dtype, device='cpu'):
    """ case 3: u_x + 2 u = 1 on the face x = 1 at three times, one model call: under the hard Dirichlet ansatz the value stream is the
    boundary constant there, the derivative stream is not """
    tg = torch.tensor([[0.2], [0.5], [0.8]], dtype=dtype, device=device)

    def eq(u, x, t):
        return D(D(u, t), t) - 0.5 * D(D(u, x), x)

    def robin(f, x, t):
        x1 = torch.ones((3, 1), dtype=dtype, device=device, requires_grad=True)
        u = f(x1, tg)
        return D(u, x1) + 2 * u - 1
    return eq, robin


def _face_terms(which):
    def problem(D, V, dtype, device='cpu'):
        """ two directions in ONE lowered call, on 70 points of the face x = 1 (more than four tiles of 16, the last one ragged; t = 0, the
        corner where the gate vanishes too, included): `laplacian` u_xx + u_tt = 1 (nd = 2, n2 = 2), `oblique` u_x + 0.5 u_t + u = 1
        (nd = 2, n2 = 0) """
        tg = torch.linspace(0.0, 1.0, 70, dtype=dtype, device=device).reshape(-1, 1)

        def eq(u, x, t):
            return D(D(u, t), t) - 0.5 * D(D(u, x), x)

        def con(f, x, t):
            x1 = torch.ones((70, 1), dtype=dtype, device=device, requires_grad=True)
            t1 = tg.clone().requires_grad_()
            u = f(x1, t1)
            if which == 'laplacian':
                return D(D(u, x1), x1) + D(D(u, t1), t1) - 1.0
            return D(u, x1) + 0.5 * D(u, t1) + u - 1.0
        return eq, con
    return problem


def periodic_flux(D, V, dtype, device='cpu'):
    """ `D` of an expression of TWO model calls: the chain rule runs over the streams of both """
    def eq(u, x, t):
        return D(u, t) - 0.3 * D(D(u, x), x)

    def con(f, x, t):
        a, b = f(0.2 * torch.ones_like(x), t), f(0.8 * torch.ones_like(x), t)
        return D(a - b, t) + 0.5 * D(a * b, t)
    return eq, con


def coordinate_coefficients(D, V, dtype, device='cpu'):
    """ `D` of an expression that holds the batch column ITSELF beside the model's value: the explicit partial derivative counts
    (d/dt [t u] = u + t u_t; a flux with a coefficient of the coordinate, d/dx [(1 + x) u_x]) """
    def eq(u, x, t):
        return D(u, t) - 0.3 * D(D(u, x), x)

    def growth(f, x, t):
        return D(f(x, t) * t, t) - 0.1

    def flux(f, x, t):
        u = f(x, t)
        return D((1 + x) * D(u, x), x) + D(x * u, x)
    return eq, (growth, flux)


def _second_order(mixed):
    def problem(D, V, dtype, device='cpu'):
        """ case 4: a second derivative at two fixed points, pure (one direction: lowered) or mixed (the diagonal: three directions) """
        def eq(u, x, y):
            return D(D(u, x), x) + D(D(u, y), y) - 5 * torch.sin(np.pi * (x + y))

        def con(f, x, y):
            px = torch.tensor([[0.3], [0.7]], dtype=dtype, device=device, requires_grad=True)
            py = torch.tensor([[0.6], [0.2]], dtype=dtype, device=device, requires_grad=True)
            u = f(px, py)
            return (D(D(u, px), py) if mixed else D(D(u, px), px)) - 1.0
        return eq, con
    return problem


def heat_on_the_batch(D, V, dtype, device='cpu'):
    """ case 5: the initial velocity on the batch's x and the flux on the batch itself """
    def eq(u, x, t):
        return D(u, t) - 0.3 * D(D(u, x), x)

    def velocity(f, x, t):                       # u_t(x, 0) = 0 on the batch's x
        t0 = torch.zeros_like(t).requires_grad_()
        return D(f(x, t0), t0)

    def flux(f, x, t):
        return D(f(x, t), x) - 0.1
    return eq, (velocity, flux)


def normalised(base):
    class Normalised(base):
        def forward(self, xs):
            return self.anzatc(self.conv_block(2 * xs - 1), xs)
    return Normalised


# ---- the harness -----------------------------------------------------------------------------------------------------------------------------
def _pair(pa, tier, problem, kw, extra, model=False):
    """ (fp32 oracle, its start, the product solver loaded with that start, a maker of further oracles) """
    from oracle import pinn_oracle as po
    torch.manual_seed(11)
    eq_o, con_o = problem(po.D, po.V, torch.float32)
    okw = dict(kw, model=normalised(po.OracleModel)) if model else kw
    oracle = po.OracleSolver(eq_o, constraints=con_o, **okw)
    start = oracle.export_params()

    def another(dtype):
        eq, con = problem(po.D, po.V, dtype)
        o = po.OracleSolver(eq, constraints=con, dtype=dtype, **okw)
        o.import_params(start)
        return o
    eq_p, con_p = problem(pa.D, pa.V, torch.float32, tier[1])
    pkw = dict(kw, model=normalised(pa.ConvBlockModel)) if model else kw
    solver = pa.Solver(eq_p, constraints=con_p, **pkw, **extra)
    load_params(solver, start)
    return oracle, start, solver, another


def _fit_case(pa, tier, extra, name, problem, kw, terms, batch, path, steps=3, lr=0.01, model=False, fit_kwargs=None, oracle_kwargs=None,
              before=None, calls=1):
    """ calls: that many fit calls in a row, each of `steps` iterations on points of its own; losses of all of them and the parameters at
    the end are judged. Returns (fp32 oracle, solver, the fp64 arbiter's maker). """
    oracle, start, solver, another = _pair(pa, tier, problem, kw, extra, model)
    if before is not None:
        before(solver)
    d = kw['ndims']
    pts = np.random.RandomState(21).rand(calls, steps, batch, d).astype(np.float32)
    okw = dict(oracle_kwargs or fit_kwargs or {})
    arbiter = {}

    def oracle64():
        if 'o' not in arbiter:
            o = arbiter['o'] = another(torch.float64)
            for part in pts:
                o.fit(niters=steps, batch_size=batch, points=part, lr=lr, loss_terms=terms, **okw)
        return arbiter['o']
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)            # (the reference's own target of size [1] against [n, 1] values)
        for part in pts:
            oracle.fit(niters=steps, batch_size=batch, points=part, lr=lr, loss_terms=terms, **okw)
            solver.fit(niters=steps, batch_size=batch, sampler=FixedBatches(part), lr=lr, loss_terms=terms, **(fit_kwargs or {}))
            assert solver.last_fit_path == path, solver.constraint_errors
        print(f'{tier[0]} {name} {terms}: path {solver.last_fit_path}, errors {solver.constraint_errors}, losses {[float(v) for v in solver.losses]} '
              f'oracle {[float(v) for v in oracle.losses]}')
        fit_close(f'{tier[0]}_constraint_derivatives', f'{name}/{"+".join(terms)}', solver, oracle, oracle64, adam_move=lr * steps * calls)
    return oracle, solver, oracle64


def _tier(request, tier):
    return {} if tier is GPU else emu_kwargs(request.getfixturevalue('emu_lib'))


def both_tiers(fn):
    """ the case on the emulator and, marked gpu, on the device """
    return pytest.mark.parametrize('tier', [pytest.param(EMU, id='emu'), pytest.param(GPU, id='gpu', marks=pytest.mark.gpu)])(fn)


@pytest.fixture
def extra(request, pa, tier):
    if tier is GPU:
        request.getfixturevalue('gpu_lib')
    return _tier(request, tier)


# ---- 1. Neumann at one fixed point -------------------------------------------------------------------------------------------------------------
@both_tiers
@pytest.mark.parametrize('terms', [['equation', 'constraint_0'], ['constraint_0']], ids=['with_equation', 'alone'])
def test_neumann_at_a_fixed_point_is_lowered(pa, tier, extra, terms):
    _, solver, _ = _fit_case(pa, tier, extra, 'neumann_ode', neumann_ode, ODE, terms, 40, 'fused', steps=4, lr=0.05)
    cp = solver.constraint_plans[0]
    assert cp is not None, solver.constraint_errors
    assert cp['points'].shape == (1, 1) and float(cp['points'][0, 0]) == 1.0
    assert list(cp['dir_cols']) == [0] and cp['n2p'] == 0


# ---- 2. initial velocity of a wave -------------------------------------------------------------------------------------------------------------
@both_tiers
def test_initial_velocity_on_a_fixed_grid(pa, tier, extra):
    """ the callable IC adds its own rows to every stream (cp['ic']), the V born in the constraint stays dormant for the first fit call,
    and log_scale -- which t = 0 reaches through the derivative stream alone -- gets the reference's gradient """
    terms = ['equation', 'constraint_0']
    oracle, start, solver, another = _pair(pa, tier, wave_velocity, WAVE, extra)
    cp = solver.constraint_plans[0]
    assert cp is not None, solver.constraint_errors
    assert cp['points'].shape == (5, 2) and list(cp['dir_cols']) == [1] and cp['plan'].n_vars == 1
    assert cp['ic'] is not None and tuple(cp['ic'].shape) == (2, 5)         # u and u_t: the IC's value row and its (zero) time derivative
    np.testing.assert_allclose(cp['ic'][0].cpu().numpy(), np.sin(np.pi * np.linspace(0.1, 0.9, 5)), rtol=1e-6)
    assert float(cp['ic'][1].abs().max()) == 0.0
    # one evaluation of the constraint term alone: every gradient against the oracle's (lr = 0: its backward, no move)
    pts = np.random.RandomState(22).rand(1, 33, 2).astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        oracle.fit(niters=1, batch_size=33, points=pts, lr=0.0, loss_terms=['constraint_0'])
        o64 = another(torch.float64)
        o64.fit(niters=1, batch_size=33, points=pts, lr=0.0, loss_terms=['constraint_0'])
    solver._apply_criterion((pa.engine.CRIT_MSE, 0.0, False), [0])
    solver._fused_terms_step(torch.from_numpy(pts[0]).to(solver.device), ['constraint_0'], [0], 1)
    want, want64 = oracle.export_grads(), o64.export_grads()
    for i, got in enumerate(export_grads(solver)):
        ok, err, arb = close_or_arbitrated(got, want[i], lambda i=i: want64[i], GRAD_RTOL)
        record_margin(f'{tier[0]}_constraint_derivatives', 'wave_velocity/gradient', f'grad_{i}', err, GRAD_RTOL, arb)
        assert ok, (i, err)
    assert abs(float(want[-1])) > 1e-6 and abs(float(export_grads(solver)[-1])) > 1e-6      # log_scale: reached, not zero
    # trajectories: the first call leaves v0 alone (reference :420 vs :457), the second trains it; both at the bars of fit_close
    oracle, solver, _ = _fit_case(pa, tier, extra, 'wave_velocity', wave_velocity, WAVE, terms, 33, 'fused', steps=3, lr=0.02)
    assert float(solver.model.v0.detach()) == float(oracle.model.v0.detach()) == float(np.float32(0.3))
    oracle, solver, oracle64 = _fit_case(pa, tier, extra, 'wave_velocity_two_calls', wave_velocity, WAVE, terms, 33, 'fused', steps=3, lr=0.02,
                                         calls=2)
    got, want = float(solver.model.v0.detach()), float(oracle.model.v0.detach())
    assert got != float(np.float32(0.3))
    ok, err, arb = close_or_arbitrated([got], [want], lambda: [float(oracle64().model.v0.detach())], FIT_PARAM_RTOL, atol=2e-6)
    record_margin(f'{tier[0]}_constraint_derivatives', 'wave_velocity_two_calls', 'v0', err, FIT_PARAM_RTOL, arb)
    assert ok, (got, want, err)


# ---- 3. Robin on a face ------------------------------------------------------------------------------------------------------------------------
@both_tiers
def test_robin_on_a_face_with_one_model_call(pa, tier, extra):
    _, solver, _ = _fit_case(pa, tier, extra, 'wave_robin', wave_robin, WAVE, ['equation', 'constraint_0'], 33, 'fused', steps=3, lr=0.02)
    cp = solver.constraint_plans[0]
    assert cp['points'].shape == (3, 2) and list(cp['dir_cols']) == [0]
    # on the face the ansatz factor is exactly zero: the value stream is the boundary constant plus IC(1)
    u = solver.predict(np.ones(3), np.array([0.2, 0.5, 0.8]))
    assert float(np.abs(u).max()) < 1e-6


# ---- 3b. two directions in one lowered call on 70 face points ----------------------------------------------------------------------------------
@both_tiers
@pytest.mark.parametrize('which, n2p', [('laplacian', 2), ('oblique', 0)])
def test_two_directions_on_seventy_face_points(pa, tier, extra, which, n2p):
    for terms in (['equation', 'constraint_0'], ['constraint_0']):          # (accumulate mode, and the term storing on its own)
        _, solver, _ = _fit_case(pa, tier, extra, 'face_' + which, _face_terms(which), WAVE, terms, 33, 'fused', steps=3, lr=0.02)
        cp = solver.constraint_plans[0]
        assert cp['points'].shape == (70, 2) and list(cp['dir_cols']) == [0, 1] and cp['n2p'] == n2p
        assert tuple(cp['ic'].shape) == (3 + n2p, 70)


# ---- 4. second order at a point, deep net with a skip and an activation of the second set -------------------------------------------------------
@both_tiers
@pytest.mark.parametrize('mixed', [False, True], ids=['pure', 'mixed'])
def test_second_order_at_two_points(pa, tier, extra, mixed):
    path = 'generic' if mixed else 'fused'
    _, solver, _ = _fit_case(pa, tier, extra, 'second_order_' + ('mixed' if mixed else 'pure'), _second_order(mixed), DEEP,
                          ['equation', 'constraint_0'], 33, path, steps=3, lr=0.005)
    assert solver.model.net.allact
    if mixed:
        # three directions (x, y, the diagonal) on the second set of kernels: more than one call, hence not lowered -- and says so
        assert solver.constraint_plans[0] is None and 'several kernel calls' in solver.constraint_errors[0]
        assert len(solver.constraint_specs[0][0].groups) > 1
    else:
        cp = solver.constraint_plans[0]
        assert cp['points'].shape == (2, 2) and list(cp['dir_cols']) == [0] and cp['n2p'] == 1


# ---- 5. the generic path on batch points --------------------------------------------------------------------------------------------------------
@both_tiers
@pytest.mark.parametrize('model', [False, True], ids=['kernel_ansatz', 'own_forward'])
def test_batch_points_on_the_generic_path(pa, tier, extra, model):
    terms = ['equation', 'constraint_0', 'constraint_1']
    _, solver, _ = _fit_case(pa, tier, extra, 'heat_on_the_batch' + ('_own_forward' if model else ''), heat_on_the_batch, HEAT, terms, 40,
                          'generic', steps=3, lr=0.01, model=model)
    assert solver.constraint_plans == [None, None]
    # (a model with its own forward() is refused for lowering as such, before the tracer looks at the points: that reason comes first and
    #  stands in for 'batch points' there, on purpose)
    reason = 'its own forward()' if model else 'batch points'
    assert all(reason in err for err in solver.constraint_errors), solver.constraint_errors
    assert [[spec.dirs for spec in specs] for specs in solver.constraint_specs] == [[[(1,)]], [[(0,)]]]


@both_tiers
def test_derivative_of_an_expression_of_two_model_calls(pa, tier, extra):
    """ `D(f(a, t) - f(b, t), t)`: not a stream pick but the chain rule, over the streams of BOTH calls (the dry run asks both for u_t) """
    _, solver, _ = _fit_case(pa, tier, extra, 'periodic_flux', periodic_flux, HEAT, ['constraint_0'], 40, 'generic', steps=3, lr=0.01)
    assert [spec.dirs for spec in solver.constraint_specs[0]] == [[(1,)], [(1,)]]
    assert solver.constraint_dry_run_errors == [None]


@both_tiers
@pytest.mark.parametrize('model', [False, True], ids=['kernel_ansatz', 'own_forward'])
def test_batch_column_inside_the_differentiated_expression(pa, tier, extra, model):
    """ the batch columns a differentiating constraint gets are leaves: `D(t * f(x, t), t)` keeps its `u` term """
    terms = ['constraint_0', 'constraint_1']
    _, solver, _ = _fit_case(pa, tier, extra, 'coordinate_coefficients' + ('_own_forward' if model else ''), coordinate_coefficients, HEAT,
                             terms, 40, 'generic', steps=3, lr=0.01, model=model)
    assert solver.constraint_dry_run_errors == [None, None]
    assert [[spec.dirs for spec in specs] for specs in solver.constraint_specs] == [[[(1,)]], [[(0,)]]]
    assert solver.constraint_specs[1][0].n2 == 1


# ---- 6. fused criterion and fused optimizer -------------------------------------------------------------------------------------------------------
@both_tiers
@pytest.mark.parametrize('which', ['l1_criterion', 'adamw'])
def test_fused_criterion_and_optimizer(pa, tier, extra, which):
    terms = ['equation', 'constraint_0']
    if which == 'l1_criterion':
        crit = nn.L1Loss()
        _, solver, _ = _fit_case(pa, tier, extra, 'neumann_ode_l1', neumann_ode, ODE, terms, 40, 'fused', steps=4, lr=0.05,
                              fit_kwargs=dict(criterion=crit), before=lambda s: s.set_criterion_path('fused'))
        assert solver.last_fit_criterion == 'L1Loss/fused'
    else:
        kwargs = dict(optimizer='AdamW', weight_decay=0.05)
        _, solver, _ = _fit_case(pa, tier, extra, 'neumann_ode_adamw', neumann_ode, ODE, terms, 40, 'fused', steps=4, lr=0.05,
                              fit_kwargs=kwargs, before=lambda s: s.set_optimizer_path('fused'))
        assert solver.last_fit_optimizer == 'AdamW/fused'


# ---- 7. refusals, and what stays untouched ---------------------------------------------------------------------------------------------------------
@both_tiers
def test_refusals(pa, tier, extra):
    dev = tier[1]
    eq = neumann_ode(pa.D, pa.V, torch.float32, dev)[0]
    pts = np.random.RandomState(5).rand(2, 33, 1).astype(np.float32)

    def fifth(f, x):
        p = torch.tensor([[0.5]], device=dev, requires_grad=True)
        return pa.D(pa.D(pa.D(pa.D(pa.D(f(p), p), p), p), p), p)
    solver = pa.Solver(eq, constraints=fifth, **ODE, **extra)
    assert solver.constraint_plans[0] is None
    with pytest.raises(NotImplementedError, match=r'\(0, 0, 0, 0, 0\).*orders above four are not built'):
        solver.fit(niters=2, batch_size=33, sampler=FixedBatches(pts), loss_terms=['equation', 'constraint_0'])

    def unrelated(f, x):
        p = torch.tensor([[0.5]], device=dev, requires_grad=True)
        q = torch.tensor([[0.5]], device=dev, requires_grad=True)
        return pa.D(f(p), q)
    solver = pa.Solver(eq, constraints=unrelated, **ODE, **extra)
    assert solver.constraint_plans[0] is None
    with pytest.raises(RuntimeError, match='not have been used in the graph'):
        solver.fit(niters=2, batch_size=33, sampler=FixedBatches(pts), loss_terms=['equation', 'constraint_0'])

    # the dry run's own failures are on record; a width that does not carry the order leaves a reason and raises in the fit call
    assert solver.constraint_dry_run_errors[0] is not None and 'q is none' not in solver.constraint_dry_run_errors[0]

    def third(f, x):
        p = torch.tensor([[0.5]], device=dev, requires_grad=True)
        return pa.D(pa.D(pa.D(f(p), p), p), p)
    wide = dict(ODE, layout='faf', features=[512, 1])
    solver = pa.Solver(eq, constraints=third, **wide, **extra)
    assert solver.constraint_plans[0] is None and 'width 512' in solver.constraint_errors[0]
    with pytest.raises(NotImplementedError, match='width 512'):
        solver.fit(niters=1, batch_size=33, sampler=FixedBatches(pts), loss_terms=['constraint_0'])

    def through_a_map(f, x):
        p = torch.tensor([[0.5]], device=dev, requires_grad=True)
        return pa.D(f(2 * p), p)
    solver = pa.Solver(eq, constraints=through_a_map, **ODE, **extra)
    with pytest.raises(NotImplementedError, match='FUNCTION of x'):
        solver.fit(niters=2, batch_size=33, sampler=FixedBatches(pts), loss_terms=['equation', 'constraint_0'])


@both_tiers
def test_predict_and_residual_do_not_see_the_constraint(pa, tier, extra):
    eq, con = neumann_ode(pa.D, pa.V, torch.float32, tier[1])
    torch.manual_seed(3)
    with_term = pa.Solver(eq, constraints=con, **ODE, **extra)
    plain = pa.Solver(eq, **ODE, **extra)
    x = np.linspace(0.0, 1.0, 19).astype(np.float32)
    pts = np.random.RandomState(6).rand(3, 33, 1).astype(np.float32)
    for after_fit in (False, True):
        if after_fit:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', UserWarning)
                with_term.fit(niters=3, batch_size=33, sampler=FixedBatches(pts), loss_terms=['equation', 'constraint_0'])
        load_params(plain, export_params(with_term))
        assert np.array_equal(with_term.predict(x), plain.predict(x))
        assert np.array_equal(with_term.residual(x), plain.residual(x))


# ---- 8. the generic step with a differentiating constraint is recorded as a launch graph -----------------------------------------------------------
@pytest.mark.gpu
def test_generic_step_is_recorded_as_a_launch_graph(pa, gpu_lib, monkeypatch):
    """ `D` served from a stream is no autograd fallback: the step of case 5 is recorded, warns nothing, and gives the eager step's losses """
    terms = ['equation', 'constraint_0', 'constraint_1']
    steps = pa.Solver.GENERIC_GRAPH_WARMUP + pa.Solver.GENERIC_GRAPH_MIN_REPLAYS + 4
    pts = np.random.RandomState(24).rand(steps, 40, 2).astype(np.float32)
    losses = {}
    for graph in ('1', '0'):
        monkeypatch.setenv('PYDENS_AMD_STEP_GRAPH', graph)
        _, start, solver, _ = _pair(pa, GPU, heat_on_the_batch, HEAT, {})
        before = pa.tokens.AUTOGRAD_FALLBACKS[0]
        with warnings.catch_warnings():
            warnings.simplefilter('error', RuntimeWarning)
            warnings.simplefilter('ignore', UserWarning)
            solver.fit(niters=steps, batch_size=40, sampler=FixedBatches(pts), lr=0.01, loss_terms=terms)
        assert solver.last_fit_path == 'generic' and pa.tokens.AUTOGRAD_FALLBACKS[0] == before
        st = solver._generic_graph
        if graph == '1':
            assert st is not None and st['graph'] is not None and not st['failed'], st
            assert st['replays'] > 0
        else:
            assert st is None or st['graph'] is None
        losses[graph] = [float(v) for v in solver.losses]
    assert losses['1'] == losses['0']
