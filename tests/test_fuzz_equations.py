""" Random residual equations end to end: expression trees over u, u_x, u_t, u_xx, the coordinates and constants
(arithmetic, sin / cos / tanh / sigmoid / abs / exp, squares and cubes), each handed to the product and to the oracle as a
pydens equation callable under an IC + BC ansatz; two Adam iterations must agree (losses, every parameter). Exercises the
tracer, both residual kinds, the in-kernel interpreter with its reverse sweep and the pre-pass on shapes nobody wrote by
hand -- and, with use_fused = False, the generic path (kernel streams, the user's torch code, D's stream chain rule).
CPU: emulated kernels; -m gpu: the HIP library. """
import os

import numpy as np
import pytest
import torch

from conftest import params_close, rel_l2
from helpers import (FIT_LOSS_RTOL, FIT_PARAM_RTOL, FixedBatches, close_or_arbitrated, export_params, fit_close, load_params,
                     record_margin)

SCALE = int(os.environ.get('PINN_FUZZ_SCALE', '1'))       # soak runs: PINN_FUZZ_SCALE=8 pytest tests/test_fuzz_equations.py -m gpu
LEAVES = ['u', 'ux', 'ut', 'uxx', 'x', 't', 'c']
UNARY = ['sin', 'cos', 'tanh', 'neg', 'sq', 'cube', 'sigmoid', 'abs', 'exps']
BINARY = ['add', 'sub', 'mul', 'divc', 'mulc']


def _gen(rng, depth, leaves=None, unary=None):
    leaves, unary = leaves or LEAVES, unary or UNARY
    if depth == 0 or rng.rand() < 0.25:
        leaf = leaves[rng.randint(len(leaves))]
        return ('c', float(np.round(rng.uniform(-2, 2), 3))) if leaf == 'c' else (leaf,)
    if rng.rand() < 0.4:
        return (unary[rng.randint(len(unary))], _gen(rng, depth - 1, leaves, unary))
    op = BINARY[rng.randint(len(BINARY))]
    if op in ('divc', 'mulc'):
        return (op, _gen(rng, depth - 1, leaves, unary), float(np.round(rng.uniform(0.5, 3), 3)))
    return (op, _gen(rng, depth - 1, leaves, unary), _gen(rng, depth - 1, leaves, unary))


def _ev(tree, env):
    kind = tree[0]
    if kind == 'c':
        return tree[1]
    if kind in env:
        return env[kind]
    a = _ev(tree[1], env)
    if kind in UNARY:
        if isinstance(a, float):
            a = torch.tensor(a)
        if kind == 'neg':
            return -a
        if kind == 'sq':
            return a ** 2
        if kind == 'cube':
            return a * a * a
        if kind == 'exps':
            return torch.exp(0.3 * torch.tanh(a))               # bounded exponent: no overflow on random inputs
        return getattr(torch, kind)(a)
    if kind == 'divc':
        return a / tree[2]
    if kind == 'mulc':
        return tree[2] * a
    b = _ev(tree[2], env)
    return {'add': a + b, 'sub': a - b, 'mul': a * b}[kind]


LOSS_RTOL, PARAM_RTOL = FIT_LOSS_RTOL, FIT_PARAM_RTOL          # (helpers.fit_close: shared with test_residual_program_ops.py)
_fit_close = fit_close


def _uses(tree, name):
    return tree[0] == name or any(isinstance(c, tuple) and _uses(c, name) for c in tree[1:])


def _equation(tree, D, keep=0.0):
    def equation(u, x, t):
        env = {'u': u, 'x': x, 't': t}
        if _uses(tree, 'ux') or _uses(tree, 'uxx') or _uses(tree, 'uxxx'):
            env['ux'] = D(u, x)
        if _uses(tree, 'uxx') or _uses(tree, 'uxxx'):
            env['uxx'] = D(env['ux'], x)
        if _uses(tree, 'uxxx'):
            env['uxxx'] = D(env['uxx'], x)
        if _uses(tree, 'ut'):
            env['ut'] = D(u, t)
        # keeps the field in and the residual away from zero. keep > 0: every parameter gets a gradient that is not EXACTLY
        # zero (u_xxx alone does not see the last bias under the boundary binding: fp64 says 0, fp32 says 1e-9, and Adam turns
        # that into a step of 0.1 lr)
        return _ev(tree, env) + keep * u + 0.37
    return equation


def _run(pa, extra, n_trees, batch, fused=True, third=False):
    """ third: u_xxx joins the leaves and every tree uses it. Three nested fp32 autograd sweeps are noisy, so the oracle runs in
    fp64 from the same fp32 start (the arbiter of SURVEY 8c item 5) and the tolerances are those of an fp32 computation against
    the exact one. """
    from oracle import pinn_oracle as po
    rng = np.random.RandomState(11 if third else 1)
    leaves = LEAVES + ['uxxx', 'uxxx'] if third else LEAVES
    kw = dict(ndims=2, initial_condition=lambda x: torch.sin(np.pi * x), boundary_condition=0.0, layout='fafaf',
              features=[16, 16, 1], activation='Tanh')
    kinds = {'program': 0, 'affine': 0}
    for trial in range(n_trees):
        tree = _gen(rng, 3, leaves)
        if not any(_uses(tree, name) for name in (('uxxx',) if third else ('u', 'ux', 'ut', 'uxx'))):
            continue
        torch.manual_seed(trial)
        oracle = po.OracleSolver(_equation(tree, po.D, 0.05 if third else 0.0), **kw)
        start = oracle.export_params()
        pts = np.random.RandomState(trial).rand(2, batch, 2).astype(np.float32)

        def oracle64(tree=tree, start=start, pts=pts):
            o = po.OracleSolver(_equation(tree, po.D, 0.05 if third else 0.0), dtype=torch.float64, **kw)
            o.import_params(start)
            o.fit(niters=2, batch_size=batch, points=pts, lr=0.01)
            return o
        if third:
            oracle = po.OracleSolver(_equation(tree, po.D, 0.05 if third else 0.0), dtype=torch.float64, **kw)
            oracle.import_params(start)
        solver = pa.Solver(_equation(tree, pa.D, 0.05 if third else 0.0), **kw, **extra)
        solver.use_fused = fused
        load_params(solver, oracle.export_params())
        oracle.fit(niters=2, batch_size=batch, points=pts, lr=0.01)
        solver.fit(niters=2, batch_size=batch, sampler=FixedBatches(pts), lr=0.01)
        want = np.array([float(v) for v in oracle.losses])
        if not np.all(np.isfinite(want)):
            continue
        assert solver.last_fit_path == ('fused' if fused else 'generic'), (tree, solver.program_error)
        if third:
            assert solver.spec.n3 == 1, tree
        if third:       # (against the fp64 trajectory itself: three nested fp32 sweeps of the reference are 1e-4 noisy)
            np.testing.assert_allclose([float(v) for v in solver.losses], want, rtol=1e-4, err_msg=str(tree))
            for got, ref in zip(export_params(solver), oracle.export_params()):
                assert params_close(got, ref, 2e-4, atol=1e-5), tree
        else:
            _fit_close('random_equations_' + ('fused' if fused else 'generic'), tree, solver, oracle, oracle64, adam_move=2 * 0.01)
        kinds['program' if solver.residual_plan.kind == 0 else 'affine'] += 1
    assert (kinds['program'] >= 5 and kinds['affine'] >= 5) or (third and sum(kinds.values()) >= 10), kinds


@pytest.mark.parametrize('path', ['fused', 'generic'])
def test_random_equations_on_the_emulated_kernels(path):
    import ctypes
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
    import build_emu
    import pydens_amd as pa
    from pydens_amd import engine
    _run(pa, dict(_lib=engine.bind(ctypes.CDLL(build_emu.build())), device='cpu'), n_trees=40, batch=23, fused=path == 'fused')


@pytest.mark.gpu
@pytest.mark.parametrize('path', ['fused', 'generic'])
def test_random_equations_on_the_gpu(path):
    import pydens_amd as pa
    _run(pa, {}, n_trees=40 * SCALE, batch=523, fused=path == 'fused')


@pytest.mark.parametrize('path', ['fused', 'generic'])
def test_random_third_order_equations_on_the_emulated_kernels(path):
    import ctypes
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
    import build_emu
    import pydens_amd as pa
    from pydens_amd import engine
    _run(pa, dict(_lib=engine.bind(ctypes.CDLL(build_emu.build())), device='cpu'), n_trees=40, batch=23, fused=path == 'fused', third=True)


@pytest.mark.gpu
def test_random_third_order_equations_on_the_gpu():
    import pydens_amd as pa
    _run(pa, {}, n_trees=40 * SCALE, batch=523, third=True)


def _composite_equation(trees, cols, D):
    """ D of EXPRESSIONS (round 6): residual = D(E1, a) + D(D(E2, b), c) + E0 with random trees E1 over (u, u_x, u_t, x, t), E2 over (u, x, t) --
    the chain rule of `D` over the streams (symbolic on the fused path, torch autograd over the tagged streams on the generic one), mixed
    second and third partials of two columns included; the reference nests torch.autograd.grad (model_torch.py:174-178) """
    e0, e1, e2 = trees
    a, b, c = cols

    def equation(u, x, t):
        env = {'u': u, 'x': x, 't': t}
        xs = {'x': x, 't': t}
        if any(_uses(e, 'ux') for e in trees):
            env['ux'] = D(u, x)
        if any(_uses(e, 'ut') for e in trees):
            env['ut'] = D(u, t)
        first = D(_ev(e1, env) + u, xs[a])
        second = D(D(_ev(e2, env) + 0.3 * u * u, xs[b]), xs[c])
        return 0.5 * first + 0.1 * second + _ev(e0, env) + 0.05 * u + 0.37
    return equation


def _run_composite(pa, extra, n_trees, batch, test):
    from oracle import pinn_oracle as po
    rng = np.random.RandomState(23)
    kw = dict(ndims=2, initial_condition=lambda x: torch.sin(np.pi * x), boundary_condition=0.0, layout='fafaf',
              features=[16, 16, 1], activation='Tanh')
    paths, done = {'fused': 0, 'generic': 0}, 0
    for trial in range(n_trees):
        # (no `abs` under a D: its derivative jumps where the argument crosses zero, and a point whose u_t is 1e-8 in fp64 and -1e-8 in fp32
        #  moves a gradient entry by a whole term -- first met on the GPU at 523 points per batch)
        smooth = [name for name in UNARY if name != 'abs']
        trees = (_gen(rng, 2, ['u', 'ux', 'ut', 'x', 't', 'c']), _gen(rng, 2, ['u', 'ux', 'ut', 'x', 't', 'c'], smooth), _gen(rng, 2, ['u', 'x', 't', 'c'], smooth))
        cols = tuple('xt'[rng.randint(2)] for _ in range(3))
        torch.manual_seed(trial)
        # (the reference's arithmetic in fp64 from the same fp32 start: two and three nested fp32 autograd sweeps of a random expression
        #  are 1e-4 noisy -- as for the third-order trees above)
        oracle = po.OracleSolver(_composite_equation(trees, cols, po.D), dtype=torch.float64, **kw)
        start = [np.asarray(p, dtype=np.float32) for p in po.OracleSolver(_composite_equation(trees, cols, po.D), **kw).export_params()]
        oracle.import_params(start)
        pts = np.random.RandomState(trial).rand(2, batch, 2).astype(np.float32)
        solver = pa.Solver(_composite_equation(trees, cols, pa.D), **kw, **extra)
        load_params(solver, start)
        oracle.fit(niters=2, batch_size=batch, points=pts, lr=0.01)
        want = np.array([float(v) for v in oracle.losses])
        if not np.all(np.isfinite(want)) or want.max() > 1e4:
            continue
        solver.fit(niters=2, batch_size=batch, sampler=FixedBatches(pts), lr=0.01)
        np.testing.assert_allclose([float(v) for v in solver.losses], want, rtol=1e-4, err_msg=str((trees, cols, solver.last_fit_path)))
        for got, ref in zip(export_params(solver), oracle.export_params()):
            assert params_close(got, ref, 2e-4, atol=1e-5), (trees, cols, solver.last_fit_path)
        paths[solver.last_fit_path] += 1
        done += 1
    assert done >= n_trees * 3 // 4 and paths['generic'] >= 3, (done, paths)


def test_random_composite_D_on_the_emulated_kernels():
    import ctypes
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
    import build_emu
    import pydens_amd as pa
    from pydens_amd import engine
    _run_composite(pa, dict(_lib=engine.bind(ctypes.CDLL(build_emu.build())), device='cpu'), n_trees=24, batch=23, test='emu')


@pytest.mark.gpu
def test_random_composite_D_on_the_gpu():
    import pydens_amd as pa
    _run_composite(pa, {}, n_trees=40 * SCALE, batch=523, test='gpu')


def _all_activations(rng, depth):
    """ one activation per hidden layer out of the whole vocabulary of the kernels (round 6): names, module instances configured away from torch's
    defaults (LeakyReLU slope, ELU alpha, Softplus beta, GELU tanh form), the smooth ones more often than the kinked ones """
    from torch import nn
    smooth = ['Tanh', 'Sigmoid', 'Sin', 'Softplus', 'SiLU', 'GELU', 'Softsign', 'Mish', 'Tanhshrink', 'LogSigmoid', 'SELU', 'ELU']
    made = []
    for _ in range(depth):
        r = rng.rand()
        if r < 0.55:
            made.append(smooth[rng.randint(len(smooth))])
        elif r < 0.85:
            made.append([lambda: nn.Softplus(beta=float(np.round(rng.uniform(0.5, 3.0), 2))), lambda: nn.ELU(alpha=float(np.round(rng.uniform(0.3, 2.0), 2))),
                         lambda: nn.GELU(approximate='tanh'), lambda: nn.LeakyReLU(float(np.round(rng.uniform(0.05, 0.4), 2)))][rng.randint(4)]())
        else:
            made.append(['ReLU', 'LeakyReLU'][rng.randint(2)])
    return made


def _random_net(rng, wmax=41):
    """ a random fully connected layout of the reference's Block vocabulary: 1-5 hidden layers of 5-40 units (padded to
    16 / 32 / 64 inside), Tanh / Sigmoid / Sin / Softplus / SiLU / GELU per layer (or one name), sometimes a hidden layer without activation,
    sometimes one skip connection 'R ... +' over layers of equal width (joining behind or in front of the activation) """
    depth = rng.randint(1, 6)
    widths = [int(rng.randint(5, wmax)) for _ in range(depth)]
    names = ['Tanh', 'Sigmoid', 'Sin', 'Softplus', 'SiLU', 'GELU']
    acts = [names[rng.randint(len(names))] for _ in range(depth)]
    letters = ['fa'] * depth
    no_act = depth >= 3 and rng.rand() < 0.3
    skip = depth >= 3 and not no_act and rng.rand() < 0.5
    if no_act:
        k = rng.randint(1, depth - 1)
        letters[k] = 'f'
        del acts[k]
    if skip:
        a = rng.randint(0, depth - 2)
        b = rng.randint(a + 1, depth - 1) if a + 1 < depth - 1 else a + 1
        for i in range(a, b + 1):
            widths[i] = widths[a]
        letters[a] = 'faR' if rng.rand() < 0.6 else 'fRa'          # the skip carries act(z) or z itself
        letters[b] = 'fa+' if rng.rand() < 0.5 else 'f+a'      # sum behind the activation, or the residual block act(W h + skip)
    activation = acts[0] if rng.rand() < 0.4 and not no_act else acts
    if isinstance(activation, str):
        acts = [activation] * len(acts)
    return dict(layout=' '.join(letters) + ' f', features=widths + [1], activation=activation if isinstance(activation, str) else acts)


def _run_layouts(pa, extra, n_nets, batch, wide=False, all_acts=False):
    """ wide: widths up to 200 (the 128- and 256-wide kernels with the streamed weight gradient; the device only); all_acts: the activations
    drawn from the whole vocabulary incl. configured instances (_all_activations) """
    from oracle import pinn_oracle as po
    rng = np.random.RandomState(44 if all_acts else 4)

    def problems(D):
        return [
            (lambda u, x, y: D(D(u, x), x) + D(D(u, y), y) - 5 * torch.sin(np.pi * (x + y)), dict(ndims=2, boundary_condition=1)),
            (lambda u, x, t: D(u, t) + u * D(u, x) - 0.05 * D(D(u, x), x),
             dict(ndims=2, boundary_condition=0, initial_condition=lambda x: torch.sin(np.pi * x))),
            (lambda u, x, e: D(u, x) - e * torch.cos(e * x), dict(ndims=1, nparams=1, initial_condition=1.0)),
        ]
    seen = set()
    for trial in range(n_nets):
        net = _random_net(rng, 201 if wide and trial % 4 == 3 else 41)
        if all_acts:
            net['activation'] = _all_activations(rng, net['layout'].count('a'))
        which = trial % 3
        eq_o, kw = problems(po.D)[which]
        eq_p, _ = problems(pa.D)[which]
        torch.manual_seed(trial)
        oracle = po.OracleSolver(eq_o, **kw, **net)
        solver = pa.Solver(eq_p, **kw, **net, **extra)
        start = oracle.export_params()
        load_params(solver, start)
        pts = np.random.RandomState(trial).rand(2, batch, 2).astype(np.float32)

        def oracle64(eq_o=eq_o, kw=kw, net=net, start=start, pts=pts):
            o = po.OracleSolver(eq_o, dtype=torch.float64, **kw, **net)
            o.import_params(start)
            o.fit(niters=2, batch_size=batch, points=pts, lr=0.01)
            return o
        oracle.fit(niters=2, batch_size=batch, points=pts, lr=0.01)
        solver.fit(niters=2, batch_size=batch, sampler=FixedBatches(pts), lr=0.01)
        assert solver.last_fit_path == 'fused', (net, solver.program_error)
        _fit_close('random_layouts' + ('_wide' if wide else '') + ('_all_acts' if all_acts else ''), str(net), solver, oracle, oracle64, adam_move=2 * 0.01)
        grid = [np.linspace(0.1, 0.9, 5).astype(np.float32)] * 2
        assert np.abs(solver.predict(*grid) - oracle.predict(*grid)).max() < 2e-5, net
        seen.add(('R' in net['layout'], isinstance(net['activation'], list)))
    assert len(seen) >= (2 if all_acts else 3)                     # with / without skips, one name / per-layer lists


def test_random_layouts_on_the_emulated_kernels():
    import ctypes
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
    import build_emu
    import pydens_amd as pa
    from pydens_amd import engine
    _run_layouts(pa, dict(_lib=engine.bind(ctypes.CDLL(build_emu.build())), device='cpu'), n_nets=20, batch=21)


def test_random_layouts_with_every_activation_on_the_emulated_kernels():
    import ctypes
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
    import build_emu
    import pydens_amd as pa
    from pydens_amd import engine
    _run_layouts(pa, dict(_lib=engine.bind(ctypes.CDLL(build_emu.build())), device='cpu'), n_nets=12, batch=23, all_acts=True)


@pytest.mark.gpu
def test_random_layouts_with_every_activation_on_the_gpu():
    import pydens_amd as pa
    _run_layouts(pa, {}, n_nets=30 * SCALE, batch=523, wide=True, all_acts=True)


@pytest.mark.gpu
def test_random_layouts_on_the_gpu():
    import pydens_amd as pa
    _run_layouts(pa, {}, n_nets=24 * SCALE, batch=311, wide=True)



def _random_problem(rng, D):
    """ a random problem SHAPE: 1-3 differentiated variables, with / without time, box or no boundary binding, constant or
    callable initial condition, 0-2 extra parameters, a random domain, a random net, a ragged batch size """
    ndims = int(rng.randint(1, 4))
    nparams = int(rng.randint(0, 3)) if ndims < 3 else 0
    has_ic = bool(rng.rand() < 0.6)
    has_bc = bool(rng.rand() < 0.6) and (ndims > 1 or not has_ic)
    lo = [float(np.round(rng.uniform(-1, 0.5), 2)) for _ in range(ndims)]
    hi = [float(np.round(l + rng.uniform(0.5, 2.0), 2)) for l in lo]
    kw = dict(ndims=ndims, nparams=nparams, domain=list(zip(lo, hi)) if ndims > 1 else (lo[0], hi[0]))
    if has_bc:
        kw['boundary_condition'] = float(np.round(rng.uniform(-1, 1), 2))
    if has_ic:
        nsp = ndims - 1
        if nsp >= 1 and rng.rand() < 0.5:
            kw['initial_condition'] = (lambda x: torch.sin(2.0 * x) + 0.3) if nsp == 1 else (lambda x, y: x * y + torch.cos(x))
        else:
            kw['initial_condition'] = float(np.round(rng.uniform(-1, 1), 2))
    order2 = bool(rng.rand() < 0.6)
    c = float(np.round(rng.uniform(0.1, 1.5), 2))

    def equation(u, *args):
        xs, ps = args[:ndims], args[ndims:]
        r = 0.37 + 0.1 * u
        for i, x in enumerate(xs):
            ux = D(u, x)
            r = r + (1.0 + 0.5 * i) * ux * (u if i == 0 else 1.0)
            if order2 and (i < ndims - 1 or not has_ic):
                r = r - c * D(ux, x)
            r = r + torch.sin(x)
        for p in ps:
            r = r + p * u
        return r
    depth = int(rng.randint(1, 5))
    net = dict(layout='fa' * depth + 'f', features=[int(rng.randint(4, 70)) for _ in range(depth)] + [1],
               activation=['Tanh', 'Sigmoid', 'Sin'][rng.randint(3)])
    batch = int(rng.choice([1, 7, 16, 17, 63, 64, 65, 200, 513, 1500, 2999]))
    return equation, {**kw, **net}, batch, ndims + nparams, lo + [0.5] * nparams, hi + [1.5] * nparams


def _run_problems(pa, extra, n_problems, max_batch):
    from oracle import pinn_oracle as po
    paths = set()
    for trial in range(n_problems):
        eq_o, kw, batch, d, lo, hi = _random_problem(np.random.RandomState(100 + trial), po.D)
        eq_p = _random_problem(np.random.RandomState(100 + trial), pa.D)[0]
        batch = min(batch, max_batch)
        torch.manual_seed(trial)
        oracle = po.OracleSolver(eq_o, **kw)
        solver = pa.Solver(eq_p, **kw, **extra)
        start = oracle.export_params()
        load_params(solver, start)
        u = np.random.RandomState(trial).rand(2, batch, d)
        pts = (np.asarray(lo) + (np.asarray(hi) - np.asarray(lo)) * u).astype(np.float32)

        def oracle64(trial=trial, start=start, pts=pts, batch=batch):
            eq64, kw64 = _random_problem(np.random.RandomState(100 + trial), po.D)[:2]
            o = po.OracleSolver(eq64, dtype=torch.float64, **kw64)
            o.import_params(start)
            o.fit(niters=2, batch_size=batch, points=pts, lr=0.01)
            return o
        oracle.fit(niters=2, batch_size=batch, points=pts, lr=0.01)
        solver.fit(niters=2, batch_size=batch, sampler=FixedBatches(pts), lr=0.01)
        want = [float(v) for v in oracle.losses]
        if not np.all(np.isfinite(want)):
            continue
        _fit_close('random_problem_shapes', (trial, batch), solver, oracle, oracle64, adam_move=2 * 0.01)
        paths.add(solver.last_fit_path)
    assert 'fused' in paths


def test_random_problem_shapes_on_the_emulated_kernels():
    import ctypes
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
    import build_emu
    import pydens_amd as pa
    from pydens_amd import engine
    _run_problems(pa, dict(_lib=engine.bind(ctypes.CDLL(build_emu.build())), device='cpu'), n_problems=6, max_batch=65)


@pytest.mark.gpu
def test_random_problem_shapes_on_the_gpu():
    import pydens_amd as pa
    _run_problems(pa, {}, n_problems=40 * SCALE, max_batch=3000)


def _random_ic_problem(rng, D):
    """ a random CALLABLE initial condition (round 6): a smooth expression tree of the spatial columns -- the tracer lowers it, with its
    derivatives along every direction of the equation, to rows of the x-only pre-pass (fused path), the generic path differentiates it by
    torch autograd -- under an evolution equation with first, second and (sometimes) mixed space-time derivatives; boundary binding or not """
    nsp = int(rng.randint(1, 3))
    smooth = [name for name in UNARY if name != 'abs']
    tree = _gen(rng, 3, ['x', 'y', 'c'][:nsp] + ['x', 'c'], smooth)
    if not any(_uses(tree, name) for name in ('x', 'y')):
        tree = ('add', tree, ('sin', ('x',)))
    mixed, burgers = bool(rng.rand() < 0.4), bool(rng.rand() < 0.5)
    c = float(np.round(rng.uniform(0.05, 0.5), 2))

    def ic(*cols):
        return _ev(tree, dict(zip('xy', cols)))

    def equation(u, *args):
        xs, t = args[:nsp], args[nsp]
        r = D(u, t) + 0.37
        for i, x in enumerate(xs):
            ux = D(u, x)
            r = r - c * D(ux, x) + (u * ux if burgers and i == 0 else 0.3 * ux)
            if mixed and i == 0:
                r = r + 0.2 * D(ux, t)
        return r
    kw = dict(ndims=nsp + 1, initial_condition=ic, layout='fafaf', features=[16, 16, 1], activation='Tanh')
    if rng.rand() < 0.6:
        kw['boundary_condition'] = float(np.round(rng.uniform(-1, 1), 2))
    return equation, kw, tree


def _run_ics(pa, extra, n_problems, batch):
    from oracle import pinn_oracle as po
    paths = {'fused': 0, 'generic': 0}
    for trial in range(n_problems):
        eq_o, kw, tree = _random_ic_problem(np.random.RandomState(500 + trial), po.D)
        eq_p, kw_p, _ = _random_ic_problem(np.random.RandomState(500 + trial), pa.D)
        torch.manual_seed(trial)
        oracle = po.OracleSolver(eq_o, **kw)
        solver = pa.Solver(eq_p, **kw_p, **extra)
        start = oracle.export_params()
        load_params(solver, start)
        if trial % 3 == 2:
            solver.use_fused = False            # every third problem on the generic path: the IC's derivative streams by torch autograd
        pts = np.random.RandomState(trial).rand(2, batch, kw['ndims']).astype(np.float32)

        def oracle64(trial=trial, start=start, pts=pts):
            eq64, kw64, _ = _random_ic_problem(np.random.RandomState(500 + trial), po.D)
            o = po.OracleSolver(eq64, dtype=torch.float64, **kw64)
            o.import_params(start)
            o.fit(niters=2, batch_size=batch, points=pts, lr=0.01)
            return o
        oracle.fit(niters=2, batch_size=batch, points=pts, lr=0.01)
        want = [float(v) for v in oracle.losses]
        if not np.all(np.isfinite(want)) or max(want) > 1e4:
            continue
        solver.fit(niters=2, batch_size=batch, sampler=FixedBatches(pts), lr=0.01)
        _fit_close('random_initial_conditions', (trial, tree), solver, oracle, oracle64, adam_move=2 * 0.01)
        paths[solver.last_fit_path] += 1
    assert paths['fused'] >= n_problems // 2 and paths['generic'] >= n_problems // 4, paths


def test_random_initial_conditions_on_the_emulated_kernels():
    import ctypes
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
    import build_emu
    import pydens_amd as pa
    from pydens_amd import engine
    _run_ics(pa, dict(_lib=engine.bind(ctypes.CDLL(build_emu.build())), device='cpu'), n_problems=16, batch=23)


@pytest.mark.gpu
def test_random_initial_conditions_on_the_gpu():
    import pydens_amd as pa
    _run_ics(pa, {}, n_problems=40 * SCALE, batch=523)


def _random_forward_problem(rng, D, base):
    """ a random model subclass with its own forward() (round 6; the reference's plug-in seam, model_torch.py:52-54): a random fixed map of
    each point in FRONT of the network (none / per-column affine / an expression tree per column / columns mixed) and a random smooth
    head around it (an expression tree of the network value and the columns, inside or instead of the ansatz) """
    smooth = [name for name in UNARY if name != 'abs']
    kind = ['none', 'affine', 'columns', 'mixing'][rng.randint(4)]
    a, b = rng.uniform(0.5, 2.5, size=2).round(2), rng.uniform(-1, 1, size=2).round(2)
    col_trees = [_gen(rng, 2, ['x', 'x', 'c'], smooth) for _ in range(2)]
    mix = float(np.round(rng.uniform(0.2, 0.8), 2))
    head = _gen(rng, 2, ['n', 'n', 'x', 't', 'c'], smooth)
    if not _uses(head, 'n'):
        head = ('add', head, ('n',))
    with_ansatz = bool(rng.rand() < 0.6)

    class Model(base):
        def forward(self, xs):
            if kind == 'none':
                ys = xs
            elif kind == 'affine':
                ys = xs * torch.tensor([float(a[0]), float(a[1])], device=xs.device) + torch.tensor([float(b[0]), float(b[1])], device=xs.device)
            elif kind == 'columns':
                ys = torch.cat([_ev(col_trees[k], {'x': xs[:, k:k + 1]}) + 0.5 * xs[:, k:k + 1] for k in range(2)], dim=1)
            else:
                ys = xs + mix * xs.flip(1) * xs
            n = self.conv_block(ys)
            out = _ev(head, {'n': n, 'x': xs[:, :1], 't': xs[:, 1:2]})
            return self.anzatc(out, xs) if with_ansatz else out
    mixed = bool(rng.rand() < 0.4)
    c = float(np.round(rng.uniform(0.05, 0.5), 2))

    def equation(u, x, t):
        ux = D(u, x)
        r = D(u, t) - c * D(ux, x) + u * ux + 0.37
        return r + 0.2 * D(ux, t) if mixed else r
    kw = dict(ndims=2, initial_condition=lambda x: torch.sin(np.pi * x), boundary_condition=0.2, layout='fafaf', features=[16, 16, 1],
              activation='Tanh', model=Model)
    return equation, kw, (kind, head, col_trees if kind == 'columns' else None, with_ansatz, mixed)


def _run_forwards(pa, extra, n_problems, batch):
    from oracle import pinn_oracle as po
    kinds = {}
    for trial in range(n_problems):
        eq_o, kw, what = _random_forward_problem(np.random.RandomState(900 + trial), po.D, po.OracleModel)
        eq_p, kw_p, _ = _random_forward_problem(np.random.RandomState(900 + trial), pa.D, pa.ConvBlockModel)
        torch.manual_seed(trial)
        oracle = po.OracleSolver(eq_o, **kw)
        solver = pa.Solver(eq_p, **kw_p, **extra)
        start = oracle.export_params()
        load_params(solver, start)
        pts = np.random.RandomState(trial).rand(2, batch, 2).astype(np.float32)

        def oracle64(trial=trial, start=start, pts=pts):
            eq64, kw64, _ = _random_forward_problem(np.random.RandomState(900 + trial), po.D, po.OracleModel)
            o = po.OracleSolver(eq64, dtype=torch.float64, **kw64)
            o.import_params(start)
            o.fit(niters=2, batch_size=batch, points=pts, lr=0.01)
            return o
        oracle.fit(niters=2, batch_size=batch, points=pts, lr=0.01)
        want = [float(v) for v in oracle.losses]
        if not np.all(np.isfinite(want)) or max(want) > 1e4:
            continue
        solver.fit(niters=2, batch_size=batch, sampler=FixedBatches(pts), lr=0.01)
        assert solver.last_fit_path == 'generic'
        _fit_close('random_forwards', (trial, what), solver, oracle, oracle64, adam_move=2 * 0.01)
        xs = [pts[0][:, i] for i in range(2)]
        assert np.abs(solver.predict(*xs) - oracle.predict(*xs)).max() < 2e-5, what
        kinds[what[0]] = kinds.get(what[0], 0) + 1
    assert len(kinds) == 4, kinds


def test_random_forwards_on_the_emulated_kernels():
    import ctypes
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
    import build_emu
    import pydens_amd as pa
    from pydens_amd import engine
    _run_forwards(pa, dict(_lib=engine.bind(ctypes.CDLL(build_emu.build())), device='cpu'), n_problems=16, batch=23)


@pytest.mark.gpu
def test_random_forwards_on_the_gpu():
    import pydens_amd as pa
    _run_forwards(pa, {}, n_problems=40 * SCALE, batch=523)


def _random_variable_problem(rng, D, V):
    """ random trainable variables and constraint terms (round 6; reference model_torch.py:180-188, :441-457): 1-3 scalar V(...) in random places
    of a random residual tree (program registers on the fused path, torch autograd on the generic one), sometimes as the initial value,
    0-2 constraint terms on fixed points (values of the solution, sometimes against a variable), several fit calls with different
    loss_terms -- the reference creates a variable where it is first met and hands it to the optimizer of the NEXT fit call """
    n_vars = int(rng.randint(1, 4))
    names = ['va', 'vb', 'vc'][:n_vars]
    # start values 0.3 .. 1.5, and exactly 0.0 for one draw in four: a variable (or its co-factor) that starts at zero has a zero gradient on
    # the first batch and must still be stepped -- reached is a property of the graph (tests/test_zero_gradient_scalars.py)
    init = {name: float(np.round(rng.uniform(0.3, 1.5), 2)) * float(rng.rand() >= 0.25) for name in names}
    smooth = [name for name in UNARY if name != 'abs']
    tree = _gen(rng, 3, ['u', 'ux', 'ut', 'uxx', 'x', 't', 'c'] + names + names, smooth)
    if not any(_uses(tree, name) for name in names):
        tree = ('add', tree, ('mul', (names[0],), ('u',)))
    ic_var = bool(rng.rand() < 0.3)
    n_con = int(rng.randint(0, 3))
    con_pts = [(float(np.round(rng.uniform(0.1, 0.9), 2)), float(np.round(rng.uniform(0.1, 0.9), 2))) for _ in range(n_con)]
    con_var = [bool(rng.rand() < 0.5) for _ in range(n_con)]
    con_tgt = [float(np.round(rng.uniform(-0.5, 0.5), 2)) for _ in range(n_con)]

    def var(name):
        return V(name, data=torch.Tensor([init[name]]))

    def equation(u, x, t):
        env = {'u': u, 'x': x, 't': t}
        env.update({name: var(name) for name in names if _uses(tree, name)})
        env['ux'] = D(u, x)
        if _uses(tree, 'uxx'):
            env['uxx'] = D(env['ux'], x)
        if _uses(tree, 'ut'):
            env['ut'] = D(u, t)
        return _ev(tree, env) + 0.05 * u + 0.1 * env['ux'] + 0.37

    def constraint(k):
        def con(f, x, t):
            value = f(torch.tensor([con_pts[k][0]]), torch.tensor([con_pts[k][1]]))
            return value - (var(names[k % n_vars]) * 0.5 if con_var[k] else con_tgt[k])
        return con
    kw = dict(ndims=2, boundary_condition=0.0, layout='fafaf', features=[16, 16, 1], activation='Tanh',
              initial_condition=(lambda x: V('v_init', data=torch.Tensor([0.6]))) if ic_var else (lambda x: torch.sin(np.pi * x)),
              constraints=[constraint(k) for k in range(n_con)] or None)
    terms = [['equation'] + [f'constraint_{k}' for k in range(n_con)], 'equation'] + ([[f'constraint_{n_con - 1}']] if n_con else [])
    return equation, kw, terms, names + (['v_init'] if ic_var else []), (tree, ic_var, n_con, con_var)


def _run_variables(pa, extra, n_problems, batch):
    from oracle import pinn_oracle as po
    paths = {'fused': 0, 'generic': 0}
    for trial in range(n_problems):
        eq_o, kw, terms, names, what = _random_variable_problem(np.random.RandomState(1300 + trial), po.D, po.V)
        eq_p, kw_p, _, _, _ = _random_variable_problem(np.random.RandomState(1300 + trial), pa.D, pa.V)
        torch.manual_seed(trial)
        oracle = po.OracleSolver(eq_o, **kw)
        solver = pa.Solver(eq_p, **kw_p, **extra)
        load_params(solver, oracle.export_params())
        if trial % 2:
            solver.use_fused = False            # every other problem on the generic path (the tracer lowers nearly all of them)
        pts = np.random.RandomState(trial).rand(2 * len(terms), batch, 2).astype(np.float32)
        bad = False
        for k, lt in enumerate(terms):
            oracle.fit(niters=2, batch_size=batch, points=pts[2 * k:2 * k + 2], lr=0.01, loss_terms=lt)
            if not np.all(np.isfinite([float(v) for v in oracle.losses])) or max(float(v) for v in oracle.losses) > 1e4:
                bad = True
                break
            solver.fit(niters=2, batch_size=batch, sampler=FixedBatches(pts[2 * k:2 * k + 2]), lr=0.01, loss_terms=lt)
            paths[solver.last_fit_path] += 1
        if bad:
            continue
        np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=5e-5, err_msg=str((trial, what)))
        for name in names:
            if hasattr(oracle.model, name) or hasattr(solver.model, name):
                assert abs(float(getattr(solver.model, name).detach()) - float(getattr(oracle.model, name).detach())) < 2e-5, (trial, name, what)
        for got, want in zip(export_params(solver), oracle.export_params()):
            assert params_close(got, want, 1e-4, atol=2e-5), (trial, what)
    assert paths['fused'] >= 3 and paths['generic'] >= 3, paths


def test_random_variables_and_constraints_on_the_emulated_kernels():
    import ctypes
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
    import build_emu
    import pydens_amd as pa
    from pydens_amd import engine
    _run_variables(pa, dict(_lib=engine.bind(ctypes.CDLL(build_emu.build())), device='cpu'), n_problems=16, batch=23)


@pytest.mark.gpu
def test_random_variables_and_constraints_on_the_gpu():
    import pydens_amd as pa
    _run_variables(pa, {}, n_problems=40 * SCALE, batch=523)


HIGH = {2: [('x', 'x', 'x'), ('x', 'x', 'y'), ('x', 'y', 'y'), ('y', 'y', 'y'), ('x', 'x', 'x', 'x'), ('x', 'x', 'y', 'y'), ('x', 'x', 'x', 'y'), ('x', 'y', 'y', 'y')],
        3: [('x', 'y', 'z'), ('x', 'x', 'z'), ('y', 'z', 'z'), ('x', 'x', 'x')]}


def _random_high_order_problem(rng, D):
    """ random equations over third- and fourth-order partials (round 6: u_xxxy / u_xyyy / u_xyz joined u_xxx, u_xxy, u_xxxx, u_xxyy): 1-3 of
    them as leaves of a smooth expression tree beside u and the coordinates, D nested in a random order of the columns, on a random
    activation, with or without the boundary binding; direction groups and polarisation identities of the generic path """
    nd = int(rng.choice([2, 2, 3]))
    picks = [HIGH[nd][i] for i in rng.choice(len(HIGH[nd]), size=int(rng.randint(1, 4)), replace=False)]
    names = ['d%d' % i for i in range(len(picks))]
    smooth = [name for name in UNARY if name not in ('abs', 'exps', 'cube')]
    tree = _gen(rng, 2, ['u', 'x', 'y', 'c'] + names + names, smooth)
    orders = [list(rng.permutation(len(p))) for p in picks]

    def equation(u, *cols):
        col = dict(zip('xyz', cols))
        env = {'u': u, 'x': cols[0], 'y': cols[1]}
        total = 0.0
        for name, alpha, order in zip(names, picks, orders):
            v = u
            for i in order:
                v = D(v, col[alpha[i]])
            env[name] = v
            total = total + 0.01 * v
        return _ev(tree, env) + total + 0.1 * u + 0.37
    kw = dict(ndims=nd, layout='fafaf', features=[12, 12, 1], activation=['Tanh', 'Sin', 'Sigmoid', 'SiLU'][rng.randint(4)])
    if rng.rand() < 0.5:
        kw['boundary_condition'] = float(np.round(rng.uniform(-1, 1), 2))
    return equation, kw, (picks, tree)


def _run_high_order(pa, extra, n_problems, batch):
    from oracle import pinn_oracle as po
    seen = set()
    for trial in range(n_problems):
        eq_o, kw, what = _random_high_order_problem(np.random.RandomState(1700 + trial), po.D)
        eq_p = _random_high_order_problem(np.random.RandomState(1700 + trial), pa.D)[0]
        torch.manual_seed(trial)
        start = [np.asarray(p, dtype=np.float32) for p in po.OracleSolver(eq_o, **kw).export_params()]
        oracle = po.OracleSolver(eq_o, dtype=torch.float64, **kw)             # (four nested fp32 sweeps of the reference are noise: fp64 from the same start)
        oracle.import_params(start)
        solver = pa.Solver(eq_p, **kw, **extra)
        load_params(solver, start)
        pts = np.random.RandomState(trial).rand(2, batch, kw['ndims']).astype(np.float32)
        oracle.fit(niters=2, batch_size=batch, points=pts, lr=0.01)
        want = np.array([float(v) for v in oracle.losses])
        if not np.all(np.isfinite(want)) or want.max() > 1e4:
            continue
        solver.fit(niters=2, batch_size=batch, sampler=FixedBatches(pts), lr=0.01)
        np.testing.assert_allclose([float(v) for v in solver.losses], want, rtol=2e-4, err_msg=str((trial, what, solver.last_fit_path)))
        for got, ref in zip(export_params(solver), oracle.export_params()):
            assert params_close(got, ref, 5e-4, atol=2e-5), (trial, what, solver.last_fit_path)
        seen.update(what[0])
    assert len(seen) >= 8, seen


def test_random_high_order_equations_on_the_emulated_kernels():
    import ctypes
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
    import build_emu
    import pydens_amd as pa
    from pydens_amd import engine
    _run_high_order(pa, dict(_lib=engine.bind(ctypes.CDLL(build_emu.build())), device='cpu'), n_problems=16, batch=17)


@pytest.mark.gpu
def test_random_high_order_equations_on_the_gpu():
    import pydens_amd as pa
    _run_high_order(pa, {}, n_problems=30 * SCALE, batch=311)


def _run_fit_sequences(pa, extra, n_sequences, batch):
    """ random SEQUENCES of fit calls on one solver (round 6; reference model_torch.py:364-464): optimizer by name with keyword arguments
    (plain Adam on the HIP kernel, everything else through the adapter), `optimizer=None` (the optimizer of the call before keeps its
    moments), lr, criterion (MSE on the fused path, anything else generic), loss_terms, a variable frozen / unfrozen in between (the
    reference hands the optimizer the parameters that require grad when the call starts, :420) """
    from torch import nn
    from oracle import pinn_oracle as po

    def problem(D, V, nu0):
        def eq(u, x, t):
            return D(u, t) - V('nu', data=torch.Tensor([nu0])) * D(D(u, x), x) + u * D(u, x)

        def con(f, x, t):
            return f(torch.tensor([0.4]), torch.tensor([0.6])) - 0.2
        return eq, con
    kw = dict(ndims=2, initial_condition=lambda x: torch.sin(np.pi * x), boundary_condition=0.0, layout='fafaf', features=[16, 16, 1],
              activation='Tanh')
    optimizers = [('Adam', {}), ('Adam', {}), ('Adam', dict(weight_decay=0.01)), ('Adam', dict(amsgrad=True)), ('Adam', dict(betas=(0.8, 0.95))),
                  ('SGD', dict(momentum=0.9)), ('RMSprop', {}), ('AdamW', {}), ('Adagrad', {}), (None, {}), (None, {})]
    seen = set()
    for trial in range(n_sequences):
        rng = np.random.RandomState(2100 + trial)
        nu0 = 0.0 if trial % 4 == 3 else 0.3             # every fourth sequence starts the variable at exactly zero
        eq_o, con_o = problem(po.D, po.V, nu0)
        eq_p, con_p = problem(pa.D, pa.V, nu0)
        torch.manual_seed(trial)
        oracle = po.OracleSolver(eq_o, constraints=con_o, **kw)
        solver = pa.Solver(eq_p, constraints=con_p, **kw, **extra)
        load_params(solver, oracle.export_params())
        n_calls = int(rng.randint(3, 6))
        pts = np.random.RandomState(trial).rand(2 * n_calls, batch, 2).astype(np.float32)
        frozen, log = False, []
        for k in range(n_calls):
            name, okw = optimizers[rng.randint(len(optimizers))] if k > 0 else optimizers[rng.randint(len(optimizers) - 2)]
            crit = [nn.MSELoss, nn.MSELoss, nn.L1Loss, nn.SmoothL1Loss][rng.randint(4)]
            terms = [['equation', 'constraint_0'], 'equation', ['equation', 'constraint_0'], ['constraint_0']][rng.randint(4)]
            lr = float([0.01, 0.003, 0.02][rng.randint(3)])
            if rng.rand() < 0.3:
                frozen = not frozen
                oracle.model.nu.requires_grad = not frozen
                (solver.model.freeze_trainable if frozen else solver.model.unfreeze_trainable)(variables=['nu'])
            call = dict(loss_terms=terms, optimizer=name, criterion=crit(), lr=lr, **okw)
            log.append((name, okw, crit.__name__, terms, lr, frozen))
            oracle.fit(niters=2, batch_size=batch, points=pts[2 * k:2 * k + 2], **{**call, 'criterion': crit()})
            solver.fit(niters=2, batch_size=batch, sampler=FixedBatches(pts[2 * k:2 * k + 2]), **call)
            seen.add((name, tuple(okw), crit.__name__, solver.last_fit_path))
        np.testing.assert_allclose([float(v) for v in solver.losses], [float(v) for v in oracle.losses], rtol=1e-4, err_msg=str((trial, log)))
        assert abs(float(solver.model.nu.detach()) - float(oracle.model.nu.detach())) < 5e-5, (trial, log)
        for got, want in zip(export_params(solver), oracle.export_params()):
            assert params_close(got, want, 2e-4, atol=4e-5), (trial, log)
    assert len({s[0] for s in seen}) >= 5 and {'fused', 'generic'} <= {s[3] for s in seen}, seen


def test_random_fit_call_sequences_on_the_emulated_kernels():
    import ctypes
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))
    import build_emu
    import pydens_amd as pa
    from pydens_amd import engine
    _run_fit_sequences(pa, dict(_lib=engine.bind(ctypes.CDLL(build_emu.build())), device='cpu'), n_sequences=12, batch=23)


@pytest.mark.gpu
def test_random_fit_call_sequences_on_the_gpu():
    import pydens_amd as pa
    _run_fit_sequences(pa, {}, n_sequences=20 * SCALE, batch=523)
