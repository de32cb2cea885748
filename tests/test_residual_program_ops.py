""" The residual program on the field, one operation at a time.

`pydens_amd/trace.py` compiles a user's equation into straight-line register code; `pinn_prog_forward` / `pinn_prog_backward`
(pinn_kernel.h) interpret it per point inside the tile kernels and `pinn_prepass_point` evaluates its x-only part in fp64. The fuzzer
(test_fuzz_equations.py) never divides by the field and never takes its log, root, reciprocal or a power other than 2; this file does:

  1. one equation per opcode whose argument holds u, u_x (some u_xx) and x: loss, EVERY parameter tensor's gradient and the gradient of
     the trainable V(...) slot of one kernel step against the oracle in fp32 and in fp64 (helpers.close_or_arbitrated, GRAD_RTOL);
  2. the values torch defines at a kink: abs'(0) = 0, d/dx x**3 at 0, x ** 1, x ** 0;
  3. `D` of an expression through each rule of trace._differentiate (host, fp64) and three nonlinear PDEs end to end;
  4. the fp64 pre-pass in both of its forms (tile-kernel prologue, separate launch) against numpy fp64, point by point.

Every kernel test runs on the emulator (CPU tier) and has an `-m gpu` twin on the HIP library. """
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from helpers import (FixedBatches, GRAD_RTOL, close_or_arbitrated, export_grads, export_params, fit_close, linear_modules, load_params,
                     record_margin)
from pydens_amd import trace
from pydens_amd.engine import OPS, RES_PROGRAM

PI = float(np.pi)


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


# ---- 1. one opcode at a time -------------------------------------------------------------------------------------------------------------
# name: (opcode the compiled program must contain, term T(D, u, x, c)). `c` lies inside the range of u under the case's ansatz (C_INSIDE),
# so that `u - c` takes both signs within a batch (asserted). Non-integer powers and logarithms get arguments bounded away from zero --
# also for u in (-1, 1), where the solver validates a lowering on random streams.
TERMS = {
    'div_field_in_denominator': ('DIV', lambda D, u, x, c: D(u, x) / (1 + u * u)),
    'div_field_on_both_sides': ('DIV', lambda D, u, x, c: (u + x) / (2 + D(u, x) * D(u, x))),
    'recip_torch_reciprocal': ('RECIP', lambda D, u, x, c: torch.reciprocal(3 + u + 0.5 * D(u, x))),
    'recip_spelled_one_over': ('DIV', lambda D, u, x, c: 1 / (2 + u + 0.5 * D(u, x))),          # 1 / expr compiles to CONST, DIV
    'log': ('LOG', lambda D, u, x, c: torch.log(1 + u * u + x * D(u, x) ** 2)),
    'sqrt': ('SQRT', lambda D, u, x, c: torch.sqrt(1 + D(u, x) ** 2 + 0.5 * u * u)),
    'pow_3_negative_argument': ('POW', lambda D, u, x, c: (u - 2 + 0.5 * D(u, x)) ** 3),
    'pow_3_both_signs': ('POW', lambda D, u, x, c: (u - c['u']) ** 3 + 0.1 * D(u, x)),
    'pow_1p5': ('POW', lambda D, u, x, c: (2 + u + 0.5 * D(u, x)) ** 1.5),
    'pow_0p5': ('POW', lambda D, u, x, c: (2 + u * x + 0.5 * D(u, x)) ** 0.5),
    'pow_minus_1': ('POW', lambda D, u, x, c: (2 + u + 0.5 * D(u, x)) ** -1),
    'pow_minus_2': ('POW', lambda D, u, x, c: (2 + u + x * D(u, x)) ** -2),
    'abs_both_signs': ('ABS', lambda D, u, x, c: torch.abs(D(u, x) - c['ux']) * (1 + u)),
    'sigmoid_with_second_derivative': ('SIGMOID', lambda D, u, x, c: torch.sigmoid(D(D(u, x), x) + 2 * u)),
    'tanh_with_second_derivative': ('TANH', lambda D, u, x, c: torch.tanh(u * D(D(u, x), x) + x)),
    'exp': ('EXP', lambda D, u, x, c: torch.exp(0.5 * u - D(u, x))),
    'sin': ('SIN', lambda D, u, x, c: torch.sin(2 * u + D(u, x))),
    'cos': ('COS', lambda D, u, x, c: torch.cos(u - x * D(u, x))),
    'neg': ('NEG', lambda D, u, x, c: -(u * u) * D(u, x)),
}
FIVE = ('div_field_in_denominator', 'sqrt', 'pow_1p5', 'log', 'abs_both_signs')       # also on the 4 x 64 kernel and in the fit chunk

# ansatz: (solver kwargs, input columns, equation around the term). k = V('k'): d(loss)/dk = sum 2 r T / N pins the term's VALUE as well.
SMALL = dict(layout='fafaf', features=[16, 16, 1], activation='Tanh')
ANSATZ = {
    'ic_1d': (dict(ndims=1, initial_condition=1.0, **SMALL), 1,
              lambda D, V, T, c: (lambda u, x: D(u, x) - 0.3 * u + V('k', torch.tensor(0.7)) * T(D, u, x, c) + 0.37)),
    'bc_2d': (dict(ndims=2, boundary_condition=0.5, **SMALL), 2,
              lambda D, V, T, c: (lambda u, x, y: D(u, x) + 0.5 * y * D(u, y) + V('k', torch.tensor(0.7)) * T(D, u, x, c) + 0.37)),
    # the `program` workload shape of bench.py: Laplacian as ONE combined stream, 4 x 64 Tanh, Dirichlet box -- the two-team kernel
    'two_team_4x64': (dict(ndims=2, boundary_condition=1, layout='fa' * 4 + 'f', features=[64] * 4 + [1], activation='Tanh'), 2,
                      lambda D, V, T, c: (lambda u, x, y: D(D(u, x), x) + D(D(u, y), y) + V('k', torch.tensor(1.5)) * T(D, u, x, c)
                                          - 5 * torch.sin(PI * (x + y)))),
}
# values inside the range of u and of u_x on every batch of the tests, chosen where the fp64 oracle keeps the difference away from zero in
# every point (no point may change sides between the precisions); the tests assert that, and that the difference takes both signs.
# (abs takes u_x - c, not u - c: under a Dirichlet box u stays within 1e-3 of the boundary value, and fp32 cancellation in u - c would
# be what the case measures)
C_INSIDE = {'ic_1d': dict(u=1.0453439950942993, ux=0.0675939992070198), 'bc_2d': dict(u=0.49950501322746277, ux=-0.00028300000121816993),
            'two_team_4x64': dict(u=1.0000849962234497, ux=0.0009009999921545386)}      # (fp32 numbers)
BOTH_SIGNS = {'pow_3_both_signs': ('u', lambda D, u, x: u), 'abs_both_signs': ('ux', lambda D, u, x: D(u, x))}


def _opcodes(solver):
    prog = solver.program.program
    return {int(prog.code[i]) & 255 for i in range(prog.n_ops)}


def _assert_is_program_with(solver, opname):
    assert solver.program is not None, solver.program_error
    assert solver.residual_plan.kind == RES_PROGRAM and solver.program.kind == RES_PROGRAM      # not an affine residual
    assert OPS[opname] in _opcodes(solver), (opname, sorted(_opcodes(solver)))


def _oracles(make_eq, kw, start, pts, names=('k',)):
    """ fp32 and fp64 oracle from the same fp32 start on the same points: {dtype: (loss, [grad per tensor], {V name: grad}, u)} """
    from oracle import pinn_oracle as po
    out = {}
    for dtype in (torch.float32, torch.float64):
        o = po.OracleSolver(make_eq(po.D, po.V), dtype=dtype, **kw)
        o.import_params(start)
        ev = o.evaluate(pts)
        out[dtype] = (ev['loss'], o.export_grads(), {n: float(getattr(o.model, n).grad) for n in names}, ev['u'])
    return out


def _check_step(test, case, solver, refs, names=('k',)):
    """ loss, every parameter tensor's gradient and every V slot's against the fp32 oracle at GRAD_RTOL, or arbitrated in fp64 """
    (l32, g32, v32, _), (l64, g64, v64, _) = refs[torch.float32], refs[torch.float64]
    lay = solver.model.net.layout
    loss = float(solver.grads[lay.off_loss])
    ok, err, arb = close_or_arbitrated([loss], [l32], lambda: [l64], 1e-5, atol=0.0)
    record_margin(test, case, 'loss', err, 1e-5, arb)
    print(f'{test} {case}: loss ours {loss:.9g} f32 {l32:.9g} f64 {l64:.9g} err {err:.2e}{" (fp64 arbiter)" if arb else ""}')
    assert ok, (case, loss, l32, l64)
    for i, (got, a32, a64) in enumerate(zip(export_grads(solver), g32, g64)):
        if a64 is None:                                     # (log_scale without an initial condition)
            assert float(np.abs(got).max()) == 0.0, (case, i)
            continue
        ok, err, arb = close_or_arbitrated(got, a32, lambda a64=a64: a64, GRAD_RTOL)
        record_margin(test, f'{case}[{i}]', 'grad', err, GRAD_RTOL, arb)
        print(f'{test} {case}: tensor {i} err {err:.2e}{" (fp64 arbiter)" if arb else ""} |f64| {np.linalg.norm(a64):.3e}')
        assert ok, (case, i, err)
    for n in names:
        off = solver.model.variables[n][0]
        got = float(solver.grads[off])
        ok, err, arb = close_or_arbitrated([got], [v32[n]], lambda n=n: [v64[n]], GRAD_RTOL)
        record_margin(test, f'{case}[V {n}]', 'grad', err, GRAD_RTOL, arb)
        print(f'{test} {case}: V({n}) ours {got:.9g} f32 {v32[n]:.9g} f64 {v64[n]:.9g}{" (fp64 arbiter)" if arb else ""}')
        assert ok, (case, n, got, v32[n], v64[n])


def _opcode_case(pa, extra, test, name, ansatz, batches):
    from oracle import pinn_oracle as po
    opname, T = TERMS[name]
    kw, d, wrap = ANSATZ[ansatz]
    c = C_INSIDE[ansatz]
    make_eq = lambda D, V: wrap(D, V, T, c)
    torch.manual_seed(5)
    start = po.OracleSolver(make_eq(po.D, po.V), **kw).export_params()
    solver = pa.Solver(make_eq(pa.D, pa.V), **kw, **extra)
    load_params(solver, start)
    _assert_is_program_with(solver, opname)
    for batch in batches:
        pts = np.random.RandomState(100 + batch).rand(batch, d).astype(np.float32)
        refs = _oracles(make_eq, kw, start, pts)
        if batch > 1 and name in BOTH_SIGNS:
            key, inner = BOTH_SIGNS[name]
            probe = po.OracleSolver((lambda u, *xs: inner(po.D, u, xs[0])), dtype=torch.float64, **kw)
            probe.import_params(start)
            vals = probe.evaluate(pts)['r'].ravel()
            arg = vals - c[key]
            assert arg.min() < 0 < arg.max() and np.abs(arg).min() > 20 * 2.0 ** -23 * np.abs(vals).max(), (arg.min(), arg.max(), np.abs(arg).min())
        solver._fused_step(torch.from_numpy(pts).to(solver.device), 1)
        kernel = solver.model.net.lib.pinn_last_kernel_name().decode()
        if ansatz == 'two_team_4x64':                       # two teams (VAR 256) of the residual-program instantiation (VAR 2048)
            var = int(kernel.rstrip('>').split(',')[-1])
            assert kernel.startswith('pinn_tile_kernel<') and var & 256 and var & 2048, kernel
        _check_step(test, f'{name}/{ansatz}/n{batch}', solver, refs)
    solver.fit(niters=1, batch_size=batches[-1], sampler=FixedBatches([pts]), lr=1e-3)      # the path a fit call of this solver takes
    assert solver.last_fit_path == 'fused', solver.program_error


OPCODE_CASES = [(n, a) for n in sorted(TERMS) for a in ('ic_1d', 'bc_2d')] + [(n, 'two_team_4x64') for n in FIVE]
# below one tile, a ragged tile, an odd tile count on two teams
EMU_BATCHES = (1, 37, 97)


@pytest.mark.parametrize('name,ansatz', OPCODE_CASES)
def test_opcode_forward_and_reverse_sweep_on_the_emulated_kernels(pa, emu_lib, name, ansatz):
    _opcode_case(pa, emu_kwargs(emu_lib), 'emu_program_ops', name, ansatz, EMU_BATCHES)


@pytest.mark.gpu
@pytest.mark.parametrize('name,ansatz', OPCODE_CASES)
def test_opcode_forward_and_reverse_sweep_on_the_gpu(pa, gpu_lib, name, ansatz):
    _opcode_case(pa, {}, 'gpu_program_ops', name, ansatz, (1000,))


def test_which_opcode_the_reciprocal_spellings_compile_to(pa, emu_lib):
    """ torch.reciprocal(expr) is PINN_OP_RECIP; 1 / expr is a CONST and a DIV (Sym.__rtruediv__), never RECIP """
    seen = {}
    for name in ('recip_torch_reciprocal', 'recip_spelled_one_over'):
        kw, d, wrap = ANSATZ['ic_1d']
        solver = pa.Solver(wrap(pa.D, pa.V, TERMS[name][1], None), **kw, **emu_kwargs(emu_lib))
        seen[name] = _opcodes(solver)
    assert OPS['RECIP'] in seen['recip_torch_reciprocal'] and OPS['DIV'] not in seen['recip_torch_reciprocal']
    assert OPS['DIV'] in seen['recip_spelled_one_over'] and OPS['RECIP'] not in seen['recip_spelled_one_over']


# the one-launch fit chunk (pinn_fit_kernel.h inherits the interpreter through pinn_tile_body). Solver.fit hands that path a DEVICE sampler
# only -- it refuses FixedBatches (Solver._device_columns) --, so the batch is the Philox batch of a seeded sampler, restated on the host
# (oracle/philox.py, bit-exact). One iteration: the gradient buffer then holds the gradient at the start parameters.
def _fit_chunk_case(pa, extra, lib, monkeypatch, test, name, batch):
    from oracle import philox
    from oracle import pinn_oracle as po
    opname, T = TERMS[name]
    kw, d, wrap = ANSATZ['ic_1d']
    c = C_INSIDE['ic_1d']
    make_eq = lambda D, V: wrap(D, V, T, c)
    monkeypatch.setenv('PYDENS_AMD_FIT_PERSIST', '2')
    monkeypatch.setenv('PYDENS_AMD_FIT_ROUNDS', '4')
    monkeypatch.setenv('PYDENS_AMD_FIT_GRAPH', '1')
    torch.manual_seed(5)
    start = po.OracleSolver(make_eq(po.D, po.V), **kw).export_params()
    solver = pa.Solver(make_eq(pa.D, pa.V), **kw, **extra)
    load_params(solver, start)
    _assert_is_program_with(solver, opname)
    sampler = pa.NumpySampler('uniform', dim=1, seed=3)
    pts = philox.sample_points(batch, [(philox.UNIFORM, 0.0, 1.0)], sampler.device_key(), 0)
    refs = _oracles(make_eq, kw, start, pts)
    solver.fit(niters=1, batch_size=batch, sampler=sampler, lr=1e-3)
    assert solver.last_fit_path == 'fused', solver.program_error
    kernel = lib.pinn_last_kernel_name().decode()
    assert kernel.startswith('pinn_fit_kernel<'), kernel
    _check_step(test, f'{name}/fit_chunk/n{batch}', solver, refs)
    assert abs(float(solver.losses[0]) - refs[torch.float64][0]) <= 1e-5 * refs[torch.float64][0]


@pytest.mark.parametrize('name', FIVE)
def test_opcode_in_the_one_launch_fit_chunk_on_the_emulator(pa, emu_lib, monkeypatch, name):
    monkeypatch.setattr(pa.Solver, 'FIT_CTRL_ON_HOST', True)
    _fit_chunk_case(pa, emu_kwargs(emu_lib), emu_lib, monkeypatch, 'emu_program_ops_fit_chunk', name, 37)


@pytest.mark.gpu
@pytest.mark.parametrize('name', FIVE)
def test_opcode_in_the_one_launch_fit_chunk_on_the_gpu(pa, gpu_lib, monkeypatch, name):
    # (the one-CU chunk takes batches of a few tiles -- at most eight virtual workgroups times four rounds, pinn_abi.cpp --; 1 000 points
    #  would go to the eager loop, which the tests above cover)
    _fit_chunk_case(pa, {}, gpu_lib, monkeypatch, 'gpu_program_ops_fit_chunk', name, 100)


# ---- 2. values torch defines at a kink ---------------------------------------------------------------------------------------------------
KINK_KW = dict(ndims=1, initial_condition=1.0, layout='fafaf', features=[8, 8, 1], activation='Tanh')


def _kink_step(pa, extra, make_eq, test, case, program=True):
    """ one step of 64 points; -> (solver, gradient in the slot of V('a'), fp32 / fp64 oracle) """
    from oracle import pinn_oracle as po
    torch.manual_seed(7)
    start = po.OracleSolver(make_eq(po.D, po.V), **KINK_KW).export_params()
    solver = pa.Solver(make_eq(pa.D, pa.V), **KINK_KW, **extra)
    load_params(solver, start)
    assert solver.program is not None and (solver.program.kind == RES_PROGRAM) == program, solver.program_error
    pts = np.random.RandomState(8).rand(64, 1).astype(np.float32)
    refs = _oracles(make_eq, KINK_KW, start, pts, names=('a',))
    solver._fused_step(torch.from_numpy(pts).to(solver.device), 1)
    got = float(solver.grads[solver.model.variables['a'][0]])
    print(f'{test} {case}: d(loss)/da ours {got:.9g}, torch fp32 {refs[torch.float32][2]["a"]:.9g}, fp64 {refs[torch.float64][2]["a"]:.9g}; '
          f'loss ours {float(solver.grads[solver.model.net.layout.off_loss]):.9g}, torch fp32 {refs[torch.float32][0]:.9g}')
    return solver, got, refs


def _kink_cases(pa, extra, test):
    # abs at an argument that is exactly zero in EVERY point: torch's abs backward is sign(x) with sign(0) = 0
    eq = lambda a0: (lambda D, V: (lambda u, x: D(u, x) - u + torch.abs(V('a', torch.tensor(a0)) - 0.5)))
    solver, got, refs = _kink_step(pa, extra, eq(0.5), test, 'abs at zero')
    assert refs[torch.float32][2]['a'] == 0.0 and refs[torch.float64][2]['a'] == 0.0
    assert OPS['ABS'] in _opcodes(solver)
    assert got == 0.0, got
    _check_step(test, 'abs_at_zero', solver, refs, names=('a',))
    # ... and one fp32 step to its right, where the gradient is the sum of d(loss)/dr
    solver, got, refs = _kink_step(pa, extra, eq(0.5 + 2.0 ** -20), test, 'abs at 2^-20')
    assert abs(refs[torch.float64][2]['a']) > 0.1
    _check_step(test, 'abs_right_of_zero', solver, refs, names=('a',))
    # x ** 3 at zero: 3 x^2 = 0
    cube = lambda D, V: (lambda u, x: D(u, x) - u + (V('a', torch.tensor(0.5)) - 0.5) ** 3)
    solver, got, refs = _kink_step(pa, extra, cube, test, 'cube at zero')
    assert OPS['POW'] in _opcodes(solver) and refs[torch.float64][2]['a'] == 0.0
    assert got == 0.0, got
    _check_step(test, 'cube_at_zero', solver, refs, names=('a',))
    # x ** 1 is the argument itself (no POW)
    first = lambda D, V: (lambda u, x: D(u, x) - u + (V('a', torch.tensor(0.5)) - 0.5) ** 1)
    solver, got, refs = _kink_step(pa, extra, first, test, 'first power at zero')
    assert OPS['POW'] not in _opcodes(solver) and abs(refs[torch.float64][2]['a']) > 0.1
    _check_step(test, 'first_power_at_zero', solver, refs, names=('a',))
    # x ** 0: torch gives the value 1 and the gradient 0, at x = 0 as well. The interpreter's e * powf(x, e - 1) would be 0 * inf there:
    # the tracer folds the power into the constant 1, so that no POW with exponent 0 reaches a kernel (this residual is affine then)
    zeroth = lambda D, V: (lambda u, x: D(u, x) - u + (V('a', torch.tensor(0.5)) - 0.5) ** 0)
    solver, got, refs = _kink_step(pa, extra, zeroth, test, 'zeroth power at zero', program=False)
    assert refs[torch.float64][2]['a'] == 0.0
    assert OPS['POW'] not in _opcodes(solver)
    assert got == 0.0, got
    _check_step(test, 'zeroth_power_at_zero', solver, refs, names=('a',))


def test_kinks_follow_torch_on_the_emulated_kernels(pa, emu_lib):
    _kink_cases(pa, emu_kwargs(emu_lib), 'emu_program_kinks')


@pytest.mark.gpu
def test_kinks_follow_torch_on_the_gpu(pa, gpu_lib):
    _kink_cases(pa, {}, 'gpu_program_kinks')


def test_tracer_never_emits_a_power_with_exponent_zero():
    from pydens_amd.tokens import D
    run = lambda fn, *args: fn(*args)
    for eq in (lambda f, x: D(f, x) + f ** 0, lambda f, x: D(f, x) + torch.pow(f * f, 0.0), lambda f, x: D(f ** 1, x) + (f * x).pow(0)):
        spec, _ = trace.discover(eq, run, 1)
        code, consts = trace.compile_program(trace.symbolic(eq, run, 1), spec, 1)
        assert all(op != OPS['POW'] for op, _, _, _ in code), code


# ---- 3. D of an expression through each rule of trace._differentiate (host, fp64) ----------------------------------------------------------
# g(f, f_x, x) on f in [0.5, 1.5], f_x in [-1, 1], x in [0.5, 1.5]: denominators >= 1, arguments of roots and logarithms >= 0.5
D_RULES = {
    'div_field_in_numerator': lambda f, fx, x: f * fx / (1 + x * x),
    'div_field_in_denominator': lambda f, fx, x: x / (1 + f * f + fx * fx),
    'div_field_in_both': lambda f, fx, x: (f + x) / (2 + fx * fx),
    'log': lambda f, fx, x: torch.log(1 + f * f + x * fx * fx),
    'sqrt': lambda f, fx, x: torch.sqrt(1 + fx ** 2 + 0.5 * f * x),
    'recip': lambda f, fx, x: torch.reciprocal(3 + f * x + 0.5 * fx),
    'pow_3': lambda f, fx, x: (f - 2 + fx * x) ** 3,
    'pow_1p5': lambda f, fx, x: (2 + f + 0.3 * fx * x) ** 1.5,
    'pow_minus_1': lambda f, fx, x: (2 + f * x + 0.3 * fx) ** -1,
    'tanh': lambda f, fx, x: torch.tanh(f * fx + x),
    'sigmoid': lambda f, fx, x: torch.sigmoid(fx * x - f),
    'exp': lambda f, fx, x: torch.exp(0.5 * f - fx * x),
    'sin': lambda f, fx, x: torch.sin(2 * f * x + fx),
    'cos': lambda f, fx, x: torch.cos(f - x * fx),
}


@pytest.mark.parametrize('rule', sorted(D_RULES))
def test_D_of_an_expression_through_each_differentiation_rule(rule):
    """ D(g(f, f_x, x), x) = g_x + g_f f_x + g_{f_x} f_xx: the symbolic rule, lowered and run by the fp64 host interpreter, against torch
    double autograd of the same g with f, f_x, x as independent leaves. rtol 1e-6 as in test_trace.py (program constants may be fp32). """
    from pydens_amd.tokens import D
    g = D_RULES[rule]
    run = lambda fn, *args: fn(*args)
    eq = lambda f, x: D(g(f, D(f, x), x), x)
    spec, _ = trace.discover(eq, run, 1)
    assert (spec.dir_cols, spec.n2) == ([0], 1)
    code, consts = trace.compile_program(trace.symbolic(eq, run, 1), spec, 1)
    rng = np.random.RandomState(3)
    n = 33
    streams = np.stack([rng.rand(n) + 0.5, rng.rand(n) * 2 - 1, rng.rand(n) * 2 - 1])
    assert [spec.index[()], spec.index[(0,)], spec.index[(0, 0)]] == [0, 1, 2]
    xs = rng.rand(n, 1) + 0.5
    got = trace.run_program_numpy(code, consts, streams, xs)
    f, fx, x = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (streams[0], streams[1], xs[:, 0])]
    fxx = torch.tensor(streams[2], dtype=torch.float64)
    g_f, g_fx, g_x = torch.autograd.grad(g(f, fx, x).sum(), [f, fx, x])
    want = (g_x + g_f * fx + g_fx * fxx).detach().numpy()
    assert np.abs(want).min() > 1e-4                       # (no entry is a cancelling sum: the relative bound means something)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0.0)


# three nonlinear PDEs end to end, two Adam steps, the bars of helpers.fit_close (the fuzzer's); (equation, solver kwargs, columns, path,
# stated reason when the path is the generic one)
def _pdes(D):
    def surface_2d(u, x, y):
        ux, uy = D(u, x), D(u, y)
        w = torch.sqrt(1 + ux ** 2 + uy ** 2)
        return D(ux / w, x) + D(uy / w, y) - 0.3
    return {
        'minimal_surface_1d': (lambda u, x: D(D(u, x) / torch.sqrt(1 + D(u, x) ** 2), x) - 0.3,
                               dict(ndims=1, initial_condition=1.0, **SMALL), 1, 'fused', None),
        # (u ** 1.5 is NaN on the random streams in (-1, 1) the solver validates a lowering on: refused, generic path)
        'porous_medium': (lambda u, x, t: D(u, t) - D(u ** 1.5 * D(u, x), x),
                          dict(ndims=2, initial_condition=lambda x: 1 + 0.3 * torch.sin(PI * x), **SMALL), 2, 'generic',
                          'traced program disagrees with the callable'),
        'bratu': (lambda u, x, y: D(D(u, x), x) + D(D(u, y), y) + 1.5 * torch.exp(u),
                  dict(ndims=2, boundary_condition=0.0, **SMALL), 2, 'fused', None),
        'minimal_surface_2d': (surface_2d, dict(ndims=2, boundary_condition=0.5, **SMALL), 2, 'generic', 'residual program too long'),
    }


def _pde_case(pa, extra, test, name, batch):
    from oracle import pinn_oracle as po
    eq_o, kw, d, path, reason = _pdes(po.D)[name]
    torch.manual_seed(9)
    oracle = po.OracleSolver(eq_o, **kw)
    start = oracle.export_params()
    pts = np.random.RandomState(10).rand(2, batch, d).astype(np.float32)

    def oracle64():
        o = po.OracleSolver(_pdes(po.D)[name][0], dtype=torch.float64, **kw)
        o.import_params(start)
        o.fit(niters=2, batch_size=batch, points=pts, lr=0.01)
        return o
    solver = pa.Solver(_pdes(pa.D)[name][0], **kw, **extra)
    load_params(solver, start)
    oracle.fit(niters=2, batch_size=batch, points=pts, lr=0.01)
    solver.fit(niters=2, batch_size=batch, sampler=FixedBatches(pts), lr=0.01)
    print(f'{test} {name}: path {solver.last_fit_path}, program_error {solver.program_error!r}')
    assert solver.last_fit_path == path, solver.program_error
    if path == 'generic':
        assert reason in solver.program_error, solver.program_error
    else:
        assert solver.residual_plan.kind == RES_PROGRAM
    fit_close(test, name, solver, oracle, oracle64, adam_move=2 * 0.01)


@pytest.mark.parametrize('name', ['minimal_surface_1d', 'porous_medium', 'bratu', 'minimal_surface_2d'])
def test_nonlinear_pde_on_the_emulated_kernels(pa, emu_lib, name):
    _pde_case(pa, emu_kwargs(emu_lib), 'emu_program_pdes', name, 37)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['minimal_surface_1d', 'porous_medium', 'bratu', 'minimal_surface_2d'])
def test_nonlinear_pde_on_the_gpu(pa, gpu_lib, name):
    _pde_case(pa, {}, 'gpu_program_pdes', name, 1000)


# ---- 4. the fp64 pre-pass, both forms ------------------------------------------------------------------------------------------------------
# A net without ansatz whose last layer is zero: every stream is exactly 0, D(u, x) - F(x) + c has the residual fl32(c - F(x)) (the whole
# x-only part is ONE pre-pass row) and the loss slot is the mean of fl32(c - F)^2 -- the aux row, seen through the loss. c = 0 shows the
# magnitude of F to the last bit, also where F is small; the square hides its SIGN (a cosine negated in two quadrants passed unnoticed,
# and so would an odd function with the wrong sign at negative arguments), so every source runs with c = 2 as well.
SOURCES = {     # name: (torch form, numpy fp64 form, argument of the single-point launch(es), range of the 256-point batch)
    'sin': (torch.sin, np.sin, None, (-3e5, 3e5)),
    'cos': (torch.cos, np.cos, None, (-3e5, 3e5)),
    'exp_neg': (lambda x: torch.exp(-x), lambda x: np.exp(-x), (1.3,), (0.0, 3.0)),
    'log': (lambda x: torch.log(x + 2), lambda x: np.log(x + 2), (0.7,), (0.0, 3.0)),
    'tanh': (torch.tanh, np.tanh, (0.6,), (-2.0, 2.0)),
    'sqrt': (lambda x: torch.sqrt(x + 1), lambda x: np.sqrt(x + 1), (0.9,), (0.0, 3.0)),
    'pow_1p5': (lambda x: (x + 1) ** 1.5, lambda x: (x + 1) ** 1.5, (0.9,), (0.0, 3.0)),
    'abs': (lambda x: torch.abs(x - 0.5), lambda x: np.abs(x - 0.5), (0.3, 0.8), (0.0, 1.0)),
    'sigmoid': (torch.sigmoid, lambda x: 1 / (1 + np.exp(-x)), (0.4,), (-3.0, 3.0)),
    'recip': (lambda x: 1 / (x + 3), lambda x: 1 / (x + 3), (0.2,), (0.0, 3.0)),
    'div': (lambda x: x / (1 + x * x), lambda x: x / (1 + x * x), (1.7,), (-2.0, 2.0)),
}
# (c - |x - 0.5| is EXACT in double on fp32 arguments, in numpy and in the kernel alike: where it lands on a rounding tie of fp32 both round
#  it to even, so the two checks that keep F away from ties do not apply to it)
EXACT_IN_DOUBLE = ('abs',)


def _trig_arguments():
    """ fp32 arguments of sin / cos: k pi/2 +- 2^-m for k in {1, 2, 3, 4, 1001, 63661} (every quadrant parity; 63661 pi/2 = 99998.5 sits
    under the switch to the library forms at 1e5), both sides of that switch with both signs, and 1e7 """
    out = []
    for k, m in ((1, 10), (2, 10), (3, 10), (4, 10), (1001, 6), (63661, 3)):
        out += [np.float32(k * np.pi / 2 + 2.0 ** -m), np.float32(k * np.pi / 2 - 2.0 ** -m)]
    out += [np.float32(s * v) for v in (99999.0, 100000.0, 100001.0) for s in (1, -1)] + [np.float32(1e7)]
    return out


def _prepass_solver(pa, extra, name, offset):
    F = SOURCES[name][0]
    solver = pa.Solver(lambda u, x: pa.D(u, x) - F(x) + offset, ndims=1, layout='fafaf', features=[8, 8, 1], activation='Tanh', **extra)
    assert solver.program is not None and solver.residual_plan.n_aux == 1, solver.program_error
    with torch.no_grad():
        last = linear_modules(solver)[-1]
        last.weight.zero_()
        last.bias.zero_()
    return solver


def _prepass_loss(solver, xs, in_kernel):
    net = solver.model.net
    assert net.lib.pinn_debug_prepass_in_kernel(net.handle, 1 if in_kernel else 0) == 0
    try:
        solver._fused_step(torch.from_numpy(np.asarray(xs, dtype=np.float32).reshape(-1, 1)).to(solver.device), 1)
        return np.float32(float(solver.grads[net.layout.off_loss]))
    finally:
        net.lib.pinn_debug_prepass_in_kernel(net.handle, 1)


def _half_ulps_from_a_tie(v):
    """ distance of the double v from the nearest midpoint between two floats, in half ulps of fp32 (0: v IS a tie) """
    f = np.float32(v)
    half = float(np.spacing(np.abs(f))) / 2
    return 1.0 - abs(float(v) - float(f)) / half


# Roundings between the fp64 value F and the loss slot of ONE point: (1) the STORE rounds F to fp32 -- the same float as np.float32(F64)
# unless F sits on a rounding tie: the kernel's fp64 F is good to about 1e-13 relative (Cody-Waite with a two-part pi/2 on fp32 arguments
# below 1e5; the library forms elsewhere), and every argument below keeps F more than 1e-4 half ulps (6e-12 relative) away from a tie
# (asserted); (2) r * r rounds once (half an ulp); (3) the scale 1 / N = 1 is exact; (4) the row sum is taken in double and rounded to fp32
# once (half an ulp). Against the exact square of fl32(F): at most ONE ulp of fp32.
SINGLE_POINT_ULPS = 1.0


def _prepass_cases(pa, extra, test):
    bit_equal = True
    for name, (_, F64, single, span) in SOURCES.items():
        for offset in (0.0, 2.0):
            solver = _prepass_solver(pa, extra, name, offset)
            args = _trig_arguments() if single is None else [np.float32(v) for v in single]
            for x in args:
                f64 = offset - float(F64(np.float64(x)))
                assert name in EXACT_IN_DOUBLE or _half_ulps_from_a_tie(f64) > 1e-4, (name, offset, x)
                want = float(np.float32(f64)) ** 2
                ulp = float(np.spacing(np.float32(want)))
                got = [_prepass_loss(solver, [x], form) for form in (True, False)]
                bit_equal &= got[0] == got[1]
                for form, g in zip(('prologue', 'launch'), got):
                    err = abs(float(g) - want) / ulp
                    record_margin(test, f'{offset:g} - {name}({float(x)!r}) {form}', 'ulps', err, SINGLE_POINT_ULPS)
                    assert err <= SINGLE_POINT_ULPS, (name, offset, float(x), form, float(g), want, err)
            # one batch of 256 points: a single point in the wrong quadrant moves the mean by far more than 1e-5
            rng = np.random.RandomState(12)
            xs = (np.linspace(span[0], span[1], 256) + rng.uniform(-0.4, 0.4, 256) * (span[1] - span[0]) / 256).astype(np.float32)
            want = float(np.mean(np.float32(offset - F64(xs.astype(np.float64))).astype(np.float64) ** 2))
            # the fp64 reference itself. (The arguments are fp32 numbers and exact: moving THEM by an ulp moves a sine at 3e5 by 0.03 and
            # says nothing.) What can move is the rounding of each F to fp32: with every F nudged by a few ulps of fp64 either way no
            # point may round to another float -- the mean then stays within 1e-12 --, and the same mean in extended precision
            # (80-bit where numpy has it) agrees to 1e-12 as well: numpy's large-argument sine is good to an ulp of the RESULT here.
            f64 = offset - F64(xs.astype(np.float64))
            for nudge in (() if name in EXACT_IN_DOUBLE else (1 - 1e-15, 1 + 1e-15)):
                moved = float(np.mean(np.float32(f64 * nudge).astype(np.float64) ** 2))
                assert abs(moved - want) <= 1e-12 * abs(want), (name, offset, nudge, moved, want)
            ext = float(np.mean((offset - F64(xs.astype(np.longdouble))).astype(np.float32).astype(np.longdouble) ** 2))
            assert abs(want - ext) <= 1e-12 * abs(ext), (name, offset, want, ext)
            got = [_prepass_loss(solver, xs, form) for form in (True, False)]
            bit_equal &= got[0] == got[1]
            for form, g in zip(('prologue', 'launch'), got):
                err = abs(float(g) - want) / want
                record_margin(test, f'{offset:g} - {name} batch 256 {form}', 'loss', err, 1e-5)
                assert err <= 1e-5, (name, offset, form, float(g), want)
    print(f'{test}: pre-pass in the kernel prologue and as its own launch bit-equal on every case: {bit_equal}')


def test_fp64_prepass_in_both_forms_on_the_emulator(pa, emu_lib):
    _prepass_cases(pa, emu_kwargs(emu_lib), 'emu_prepass')


@pytest.mark.gpu
def test_fp64_prepass_in_both_forms_on_the_gpu(pa, gpu_lib):
    _prepass_cases(pa, {}, 'gpu_prepass')
