""" The one-launch fit chunk (`pinn_fit_kernel`, pydens_amd/csrc/pinn_fit_kernel.h), iteration by iteration.

The other tests of this kernel follow a trajectory against the eager loop at loose bounds (test_emu_engine._one_launch_case and its copies:
losses 2e-4, parameters 2e-4, moments 2e-3, gradients 5e-3), where a wrong row sum, a missed tile or a stale batch in a late iteration fits.
Here:

  1. `_per_iteration`: K = 4 iterations as four one-iteration chunks. Before each call the parameters are exported and the iteration's batch is
     restated on the host (oracle/philox.py: same key, call index i); after it the loss (1e-5) and EVERY gradient tensor (helpers.GRAD_RTOL
     relative L2, floor 1e-9 per entry, fp64 arbiter with k = 2) are held to the oracle at those parameters on that batch, and the parameters
     and both state arrays to the update rule restated in fp64 (torch.optim on doubles) from the kernel's own fp32 gradient -- the contract
     test_fused_optimizers._rule_case holds for the reduction launch: live parameters 1e-6 relative L2, state arrays 1e-5, masked entries bit
     for bit. (Adam's exp_avg_sq is not part of that contract at 1e-5 against torch's double 1 - beta2, because the kernel forms 1 - beta2 in
     fp32, 4.7e-5 off; it is held at the same 1e-5 to the restatement with THAT factor.)
  2. `_split_identity`: fit(niters=4) as ONE chunk, as 2 + 2 and (SGD with momentum: `first`) as 1 + 3 equals the four one-iteration chunks
     BIT FOR BIT in losses, parameters, both state arrays, the gradient buffer, the step count and the batch left in xs. Derivable: the same
     kernel binary with k_steps a run-time argument, the same row order, the same Philox counters, state crossing calls as exact fp32. What
     differs between the two is `draw(k + 1)` at the end of sweep (d), the resident row / batch buffers reused across iterations and the
     barrier that closes (d).
  3. the cases: BASELINE config 1 (batch 100 and 1); width 16 with the in-kernel fp64 pre-pass at VW - 1, VW, VW + 1 tiles, a ragged last
     tile, exactly VW * rounds tiles and one more (declined: the tile kernel); width 32 with three hidden layers, where p_core > 4 * threads
     and sweep (d) takes a second pass, all trainable and with the middle layer frozen, Adam and SGD with momentum; a 2-D residual program
     with a trainable V(...); eight input columns at the residency limit of the LDS; the grid form (device only).
  4. a pre-pass that keeps more registers than the in-kernel form has room for (the separate pinn_aux_kernel launch): the chunk must not take
     the one-launch form, whose tile body would read pre-pass rows nobody wrote for its batches.

CPU tier on the emulator, `-m gpu` twins on the device. The emulator twin of the eight-column case (nine seconds) sits behind
PYDENS_AMD_SLOW_EMU=1. """
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import pinn_configs as pc
from helpers import GRAD_RTOL, close_or_arbitrated, load_params, record_margin

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'emu'))

K, LR, TILE = 4, 0.005, 16
LOSS_RTOL = 1e-5
PARAM_RTOL, STATE_RTOL = 1e-6, 1e-5         # test_fused_optimizers._rule_case
LDS_LIMIT = 160 * 1024 - 128
SLOW = os.environ.get('PYDENS_AMD_SLOW_EMU') == '1'
PI = float(np.pi)


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


# ---- the problems: name -> (equation from the tokens D, V; solver keywords; sampler columns (low, high); names of V slots) -----------------
def _wide_source(x, y, terms):
    """ a source term in the manner of test_emu_engine._wide_prepass_case: `terms` sub-terms, each live until its partner from the other end
    of the list is through -- one register each, two program words a term (the program holds 64) """
    ts = [torch.sin(x), torch.cos(y)]
    for i in range(2, terms):
        ts.append(ts[i - 1] * (x if i % 2 else y))
    src = ts[0] * ts[terms - 1]
    for i in range(1, terms // 2):
        src = src + ts[i] * ts[terms - 1 - i]
    return src


# width 16 without a derivative stream: PinnCfg::PREPASS_FLOATS_PER_LANE = 2 * (16 + 8) floats, room for 24 double registers; 24 sub-terms keep
# 28 alive. (Width 32 has no such window: 2 * (32 + 8) floats hold 40 registers, and PINN_MAX_REGS is 40.)
WIDE_TERMS = {'wide_prepass_16': 24}


def _problem(name, D, V):
    ode = lambda f, x: D(f, x) - 2 * PI * torch.cos(2 * PI * x)
    if name == 'cfg1':
        cfg = pc.make_config('cfg1', D, torch)
        return cfg['equation'], cfg['solver_kwargs'], [(0.0, 1.0)] * 2, ()
    if name == 'ode_16':            # x-dependent source: one fp64 pre-pass row, evaluated in the kernel and resident in aux_res
        return ode, dict(ndims=1, initial_condition=0.5, layout='fa fa f', features=[16, 16, 1], activation='Tanh'), [(0.0, 1.0)], ()
    if name == 'ode_32x3':          # 32 + 32 + 2 (32 * 32 + 32) + 32 + 1 + log_scale: more core parameters than 4 * 512 threads
        return ode, dict(ndims=1, initial_condition=0.5, layout='fa fa fa f', features=[32, 32, 32, 1], activation='Tanh'), [(0.0, 1.0)], ()
    if name == 'program_with_variable':     # test_emu_engine._one_launch_problem
        eq = lambda f, x, y: D(D(f, x), x) + D(D(f, y), y) + V('k', data=torch.Tensor([1.5])) * f * f - torch.sin(PI * (x + y))
        return eq, dict(ndims=2, boundary_condition=1, layout='fa fa f', features=[16, 16, 1], activation='Tanh'), [(0.0, 1.0)] * 2, ('k',)
    if name == 'eight_columns':     # ndims + nparams = 8: the batch takes 8 floats a point of the resident LDS
        eq = lambda f, x, a, b, c, d, e, g, h: D(f, x) - a * PI * torch.cos(b * PI * x) + c * f - d * e + 0.5 * g * h
        return (eq, dict(ndims=1, nparams=7, initial_condition=0.5, layout='fa fa f', features=[32, 32, 1], activation='Tanh'),
                [(0.0, 1.0)] + [(0.5, 1.5)] * 7, ())
    if name in WIDE_TERMS:          # no derivative stream (S = 1), a pre-pass with more live registers than the in-kernel form holds
        eq = lambda f, x, y: f - 0.1 * _wide_source(x, y, WIDE_TERMS[name])
        return eq, dict(ndims=2, boundary_condition=0.3, layout='fa fa f', features=[12, 12, 1], activation='Tanh'), [(0.0, 1.0)] * 2, ()
    raise KeyError(name)


def _sampler(pa, columns, seed):
    out = None
    for lo, hi in columns:
        leaf = pa.NumpySampler('uniform', seed=seed, low=lo, high=hi)
        out = leaf if out is None else out & leaf
    return out


class Run:
    """ one solver from the problem's start with a seeded device sampler; `fit(k)` runs k iterations as one Solver.fit call """
    def __init__(self, pa, extra, lib, problem, batch, seed, opt=('Adam', {}), frozen=(), start=None):
        from oracle import pinn_oracle as po
        self.pa, self.lib, self.problem, self.batch, self.opt = pa, lib, problem, batch, opt
        eq, kw, self.columns, self.names = _problem(problem, pa.D, pa.V)
        self.kw = kw
        if start is None:
            torch.manual_seed(seed)
            eq_o, _, _, _ = _problem(problem, po.D, po.V)
            start = po.OracleSolver(eq_o, **kw).export_params()
        self.start = start
        self.solver = pa.Solver(eq, **kw, **extra)
        load_params(self.solver, start)
        self.flat_start = self.solver.model.flat.detach().cpu().numpy().copy()
        if opt[0] != 'Adam':
            self.solver.set_optimizer_path('fused')
        self.frozen = tuple(frozen)
        for i in self.frozen:
            for p in self.linears()[i].parameters():
                p.requires_grad = False
        self.sampler = _sampler(pa, self.columns, seed)
        self.key = self.sampler.device_key()
        assert self.key is not None and self.solver._device_columns(self.sampler) is not None
        self.calls = 0
        self.kernels = []

    def linears(self):
        return [m for m in self.solver.model.conv_block if hasattr(m, 'weight')]

    def points(self, call):
        from oracle import philox
        return philox.sample_points(self.batch, [(philox.UNIFORM, lo, hi) for lo, hi in self.columns], self.key, call)

    def fit(self, k):
        name, kw = self.opt
        first = self.calls == 0
        self.solver.fit(niters=k, batch_size=self.batch, sampler=self.sampler, lr=LR, optimizer=(name if first else None), **(kw if first else {}))
        assert self.solver.last_fit_path == 'fused', self.solver.program_error
        self.calls += k
        self.kernels.append(self.lib.pinn_last_kernel_name().decode())
        return self.kernels[-1]

    def launch_info(self):
        info = (ctypes.c_int32 * 4)()
        assert self.lib.pinn_last_launch_info(info) == 0
        return [int(v) for v in info]

    def state(self):
        s, o = self.solver, self.solver.optimizer
        host = lambda t: t.detach().cpu().numpy().copy()
        return dict(losses=np.array([float(v) for v in s.losses], dtype=np.float32), params=host(s.model.flat), m=host(o.exp_avg),
                    v=host(o.exp_avg_sq), grads=host(s.grads), step=int(o.step_count.item()), host_step=int(o.t),
                    xs=host(s._fit_xs[(self.batch, s.model.total)]))

    # ---- the views of the flat buffers the oracle speaks of -----------------------------------------------------------------------------
    def tensors(self, flat):
        """ [W1, b1, ..., log_scale] of a flat buffer (helpers.export_params order) and the V slots by name """
        net, lay = self.solver.model.net, self.solver.model.net.layout
        flat = torch.as_tensor(flat)
        out = []
        for w, b in net.param_views(flat):
            out += [w.numpy().copy(), b.numpy().copy()]
        out.append(flat[lay.off_log_scale].numpy().copy())
        return out, {n: float(flat[self.solver.model.variables[n][0]]) for n in self.names}


def _vw(kernel):
    return int(kernel.rstrip('>').split(',')[-1])


def _oracle_pair(run):
    from oracle import pinn_oracle as po
    eq_o = lambda: _problem(run.problem, po.D, po.V)[0]
    return {dtype: po.OracleSolver(eq_o(), dtype=dtype, **run.kw) for dtype in (torch.float32, torch.float64)}


def _evaluate(oracle, tensors, variables, pts):
    oracle.import_params(tensors)
    with torch.no_grad():
        for n, value in variables.items():
            getattr(oracle.model, n).fill_(value)
    ev = oracle.evaluate(pts)
    return ev['loss'], oracle.export_grads(), {n: float(getattr(oracle.model, n).grad) for n in variables}


def _rule_restated(run, before, grad, step):
    """ the update rule in doubles (torch.optim itself, as in test_fused_optimizers._rule_case) on the live entries: from the kernel's state
    before the call and the kernel's own fp32 gradient -> (parameters, first state array, second state array or None) """
    name, kw = run.opt
    live = run.solver.optimizer.mask.cpu().numpy().astype(bool)
    ref = torch.tensor(before['params'][live], dtype=torch.float64, requires_grad=True)
    opt = getattr(torch.optim, name)([ref], lr=LR, **kw)
    m, v = (torch.tensor(before[key][live], dtype=torch.float64) for key in ('m', 'v'))
    if name == 'Adam':
        opt.state[ref] = dict(step=torch.tensor(float(step - 1)), exp_avg=m, exp_avg_sq=v)
    elif step > 1:
        opt.state[ref] = dict(momentum_buffer=m)
    ref.grad = torch.tensor(grad[live], dtype=torch.float64)
    opt.step()
    state = opt.state[ref]
    second = None
    if name == 'Adam':
        b2 = np.float32(kw.get('betas', (0.9, 0.999))[1])
        g = grad[live].astype(np.float64)
        second = float(b2) * before['v'][live].astype(np.float64) + float(np.float32(1.0) - b2) * g * g      # (1 - beta2 formed in fp32: the kernel's)
    first = state['exp_avg' if name == 'Adam' else 'momentum_buffer']
    return live, ref.detach().numpy(), first.numpy(), second


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _per_iteration(test, case, run, form, k=K):
    """ k one-iteration chunks; -> the state after each. form: 'onecu' / 'grid' / 'tile' -- what the case claims its kernel to be """
    oracles = _oracle_pair(run)
    states, margins = [], dict(loss=0.0, grad=0.0, arb=0)
    for i in range(k):
        before = run.state() if i else None
        flat0 = run.solver.model.flat.detach().cpu().numpy().copy()
        tensors, variables = run.tensors(flat0)
        pts = run.points(i)
        kernel = run.fit(1)
        after = run.state()
        if before is None:
            zero = np.zeros_like(flat0)
            before = dict(params=flat0, m=zero, v=zero)
        assert np.array_equal(after['xs'], pts), (case, i)             # the batch the chunk left is the restated one, bit for bit
        assert after['step'] == after['host_step'] == i + 1
        l32, g32, v32 = _evaluate(oracles[torch.float32], tensors, variables, pts)
        l64, g64, v64 = _evaluate(oracles[torch.float64], tensors, variables, pts)
        lay = run.solver.model.net.layout
        loss = float(after['grads'][lay.off_loss])
        assert loss == float(after['losses'][i])                       # the history's entry is the loss slot of the gradient buffer
        ok, err, arb = close_or_arbitrated([loss], [l32], lambda: [l64], LOSS_RTOL, atol=0.0)
        record_margin(test, f'{case}/it{i}', 'loss', err, LOSS_RTOL, arb)
        margins['loss'], margins['arb'] = max(margins['loss'], err), margins['arb'] + int(arb)
        print(f'{test} {case} it {i}: {kernel} loss ours {loss:.9g} f32 {l32:.9g} f64 {l64:.9g} err {err:.2e}{" (fp64 arbiter)" if arb else ""}')
        assert ok, (case, i, loss, l32, l64)
        got_tensors, got_vars = run.tensors(after['grads'])
        for j, (got, a32, a64) in enumerate(zip(got_tensors, g32, g64)):
            if a64 is None:                                             # (log_scale without an initial condition)
                assert float(np.abs(got).max()) == 0.0, (case, i, j)
                continue
            assert float(np.linalg.norm(a64)) > 1e-9 * np.sqrt(a64.size), (case, i, j, 'reference tensor at its floor')
            ok, err, arb = close_or_arbitrated(got, a32, lambda a64=a64: a64, GRAD_RTOL)
            record_margin(test, f'{case}/it{i}[{j}]', 'grad', err, GRAD_RTOL, arb)
            margins['grad'], margins['arb'] = max(margins['grad'], err), margins['arb'] + int(arb)
            print(f'{test} {case} it {i}: tensor {j} err {err:.2e}{" (fp64 arbiter)" if arb else ""} |f64| {np.linalg.norm(a64):.3e}')
            assert ok, (case, i, j, err)
        for n in run.names:
            assert abs(v64[n]) > 1e-9, (case, i, n, 'reference slot at its floor')
            ok, err, arb = close_or_arbitrated([got_vars[n]], [v32[n]], lambda n=n: [v64[n]], GRAD_RTOL)
            record_margin(test, f'{case}/it{i}[V {n}]', 'grad', err, GRAD_RTOL, arb)
            margins['grad'], margins['arb'] = max(margins['grad'], err), margins['arb'] + int(arb)
            print(f'{test} {case} it {i}: V({n}) ours {got_vars[n]:.9g} f32 {v32[n]:.9g} f64 {v64[n]:.9g}{" (fp64 arbiter)" if arb else ""}')
            assert ok, (case, i, n, got_vars[n], v32[n], v64[n])
        # the update: the rule restated in doubles from the kernel's own gradient
        live, p_want, m_want, v_want = _rule_restated(run, before, after['grads'], i + 1)
        for key in ('params', 'm', 'v'):
            assert np.array_equal(after[key][~live], before[key][~live]), (case, i, key, 'a masked entry moved')
        for n in run.names:
            assert live[run.solver.model.variables[n][0]], (case, n)
        errs = dict(params=_rel(after['params'][live], p_want), m=_rel(after['m'][live], m_want))
        if v_want is not None:
            errs['v'] = _rel(after['v'][live], v_want)
        else:
            assert not after['v'].any()                                 # SGD keeps a momentum buffer and nothing else
        for key, err in errs.items():
            bound = PARAM_RTOL if key == 'params' else STATE_RTOL
            record_margin(test, f'{case}/it{i}', f'rule {key}', err, bound)
            assert err < bound, (case, i, key, err)
        print(f'{test} {case} it {i}: update rule against doubles ' + ', '.join(f'{key} {err:.2e}' for key, err in errs.items()))
        # the form the case claims (after the numbers, so that a wrong form shows what it computed)
        if form == 'tile':
            assert kernel.startswith('pinn_tile_kernel<'), kernel
        else:
            assert kernel.startswith('pinn_fit_kernel<') and (_vw(kernel) == 1) == (form == 'grid'), kernel
        states.append(after)
    print(f'{test} {case}: SUMMARY kernel {run.kernels[-1]} VW {_vw(run.kernels[-1]) if form != "tile" else "-"} worst loss {margins["loss"]:.2e} '
          f'worst grad {margins["grad"]:.2e} arbitrated {margins["arb"]}')
    return states


BITS = ('losses', 'params', 'm', 'v', 'grads', 'step', 'host_step', 'xs')


def _same_bits(got, want, what):
    for key in BITS:
        assert np.array_equal(got[key], want[key]), (what, key)


def _split_identity(test, case, make_run, want, splits, form):
    """ the same K iterations as fewer, longer chunks end in the very bits of the one-iteration chunks """
    for split in splits:
        run = make_run()
        for k in split:
            kernel = run.fit(k)
            assert kernel.startswith('pinn_fit_kernel<') and (_vw(kernel) == 1) == (form == 'grid'), kernel
        _same_bits(run.state(), want, (case, split))
        print(f'{test} {case}: chunks of {split} end in the bits of {sum(split)} one-iteration chunks')


def _env(monkeypatch, persist, rounds):
    monkeypatch.setenv('PYDENS_AMD_FIT_PERSIST', str(persist))
    monkeypatch.setenv('PYDENS_AMD_FIT_ROUNDS', str(rounds))
    monkeypatch.setenv('PYDENS_AMD_FIT_GRAPH', '1')


def _both_checks(test, case, make_run, form='onecu', splits=((4,), (2, 2))):
    run = make_run()
    states = _per_iteration(test, case, run, form)
    if form != 'tile':
        _split_identity(test, case, make_run, states[-1], splits, form)
    return run, states


# seeds: chosen on the CPU so that no reference tensor of any iteration sits at its floor (test_no_reference_gradient_sits_at_the_floor)
SEEDS = {'cfg1': 31, 'ode_16': 5, 'ode_32x3': 5, 'program_with_variable': 31, 'eight_columns': 5, 'wide_prepass_16': 3}
SGD = ('SGD', dict(momentum=0.9))


def _maker(pa, extra, lib, problem, batch, **kw):
    return lambda: Run(pa, extra, lib, problem, batch, SEEDS[problem], **kw)


# ---- (a) BASELINE config 1 -------------------------------------------------------------------------------------------------------------------
def _case_a(pa, extra, lib, monkeypatch, test, batch, persist=2):
    _env(monkeypatch, persist, 4)
    form = 'onecu' if persist == 2 else 'grid'
    _both_checks(test, f'cfg1/n{batch}', _maker(pa, extra, lib, 'cfg1', batch), form)
    # SGD with momentum: the step-1 flag `first` inside a longer chunk
    if batch == 100:
        _both_checks(test, f'cfg1/n{batch}/sgd', _maker(pa, extra, lib, 'cfg1', batch, opt=SGD), form, splits=((4,), (1, 3)))


# ---- (b) width 16, in-kernel pre-pass, tile counts around VW and VW * rounds ------------------------------------------------------------------
B_CASES = {     # name: (tiles and extra points as a function of VW, rounds, form)
    'vw_minus_1': (lambda vw: (vw - 1) * TILE, 1, 'onecu'),
    'vw': (lambda vw: vw * TILE, 1, 'onecu'),
    'vw_plus_1': (lambda vw: (vw + 1) * TILE, 2, 'onecu'),
    'ragged': (lambda vw: vw * TILE + 3, 2, 'onecu'),
    'vw_times_2': (lambda vw: 2 * vw * TILE, 2, 'onecu'),
    'vw_times_4': (lambda vw: 4 * vw * TILE, 4, 'onecu'),
    'vw_times_2_plus_1': (lambda vw: (2 * vw + 1) * TILE, 2, 'tile'),
}


def _probe_vw(pa, extra, lib, monkeypatch, problem):
    """ VW of the problem's instantiation: a static figure (PinnFitVw), read from the kernel name of a one-tile chunk """
    _env(monkeypatch, 2, 1)
    kernel = Run(pa, extra, lib, problem, TILE, SEEDS[problem]).fit(1)
    assert kernel.startswith('pinn_fit_kernel<') and kernel.split('<')[1].split(',')[3] == '1', kernel      # (MT = 1: tiles of 16 points)
    assert 2 <= _vw(kernel) <= 8, kernel
    return _vw(kernel)


def _case_b(pa, extra, lib, monkeypatch, test, name):
    vw = _probe_vw(pa, extra, lib, monkeypatch, 'ode_16')
    points, rounds, form = B_CASES[name]
    _env(monkeypatch, 2, rounds)
    run, _ = _both_checks(test, f'ode_16/{name}/vw{vw}/n{points(vw)}', _maker(pa, extra, lib, 'ode_16', points(vw)), form)
    assert run.solver.residual_plan.n_aux >= 1                           # the source term IS a pre-pass row


# ---- (c) width 32, three hidden layers: the second pass of sweep (d) ---------------------------------------------------------------------------
def _case_c(pa, extra, lib, monkeypatch, test, opt, frozen):
    _env(monkeypatch, 2, 4)
    which = f'ode_32x3/{opt[0].lower()}/{"frozen_middle" if frozen else "all_trainable"}'
    splits = ((4,), (2, 2)) if opt[0] == 'Adam' else ((4,), (1, 3))
    run, states = _both_checks(test, which, _maker(pa, extra, lib, 'ode_32x3', 40, opt=opt, frozen=frozen), splits=splits)
    threads = run.launch_info()[2]
    p_core = int(run.solver.model.net.layout.p_total)
    assert threads == 128 * _vw(run.kernels[-1]) and p_core > 4 * threads, (p_core, threads)
    if frozen:
        # mask 0 in BOTH passes of the p0 loop, and the frozen layer keeps value and state bit for bit
        live = run.solver.optimizer.mask.cpu().numpy().astype(bool)
        dead = np.flatnonzero(~live[:p_core])
        lin = run.linears()[frozen[0]]
        assert dead.size >= lin.weight.numel() and (dead < 4 * threads).any() and (dead >= 4 * threads).any()
        off = np.flatnonzero(run.flat_start != states[-1]['params'])
        assert off.size and live[off].all()
        assert not states[-1]['m'][~live].any() and not states[-1]['v'][~live].any()


# ---- (d) a 2-D residual program with a trainable V(...) ----------------------------------------------------------------------------------------
def _case_d(pa, extra, lib, monkeypatch, test):
    _env(monkeypatch, 2, 4)
    run, states = _both_checks(test, 'program_with_variable/n90', _maker(pa, extra, lib, 'program_with_variable', 90))
    off = run.solver.model.variables['k'][0]
    assert states[-1]['params'][off] != np.float32(1.5) and states[-1]['m'][off] != 0.0      # the slot was updated


# ---- (e) the residency limit ---------------------------------------------------------------------------------------------------------------------
def _case_e(pa, extra, lib, monkeypatch, test):
    vw = _probe_vw(pa, extra, lib, monkeypatch, 'eight_columns')
    _env(monkeypatch, 2, 4)
    tiles = 4 * vw
    while tiles > 1:                        # walk down until the resident figure fits and the launcher accepts the chunk
        if Run(pa, extra, lib, 'eight_columns', tiles * TILE, SEEDS['eight_columns']).fit(1).startswith('pinn_fit_kernel<'):
            break
        tiles -= 1
    run, _ = _both_checks(test, f'eight_columns/tiles{tiles}/vw{vw}', _maker(pa, extra, lib, 'eight_columns', tiles * TILE))
    lds = run.launch_info()[3]
    print(f'{test} eight_columns: VW {vw}, {tiles} tiles of {4 * vw} accepted, LDS {lds} bytes of {LDS_LIMIT}')
    assert run.launch_info()[2] == 128 * vw and 0 < lds <= LDS_LIMIT, (lds, run.launch_info())
    if tiles + 1 <= 4 * vw:                 # one tile more is within the rounds and does NOT fit: declined, the tile kernel, same contract
        _both_checks(test, f'eight_columns/tiles{tiles + 1}/declined', _maker(pa, extra, lib, 'eight_columns', (tiles + 1) * TILE), 'tile')


# ---- section 4: a pre-pass that does not go into the kernel ------------------------------------------------------------------------------------
def _prepass_registers(solver):
    from pydens_amd import trace
    code, _ = solver.residual_plan.pre
    two_reg = {trace.OPS[k] for k in ('ADD', 'SUB', 'MUL', 'DIV')}
    return 1 + max(max(w[1], w[2] if w[0] != trace.OPS['CONST'] else 0, w[3] if w[0] in two_reg else 0) for w in code)


def _case_wide_prepass(pa, extra, lib, monkeypatch, test, problem, room):
    """ three iterations in ONE fit call, every one of them against the oracle on its own Philox batch: the losses from the history, the
    gradient of the last, the trajectory's parameters through the per-iteration check of three more one-iteration calls """
    from pydens_amd.engine import MAX_REGS
    _env(monkeypatch, 2, 4)
    run = Run(pa, extra, lib, problem, 3 * TILE + 5, SEEDS[problem])
    nregs = _prepass_registers(run.solver)
    assert room < nregs <= MAX_REGS, nregs          # more doubles than the in-kernel pre-pass has LDS for: the separate launch
    oracles = _oracle_pair(run)
    # the one-iteration calls first (any form that runs the pre-pass per iteration passes them) ...
    singles = _per_iteration(test, f'{problem}/nregs{nregs}/singles', run, 'tile', k=3)
    # ... then the same three iterations as one call
    chunk = Run(pa, extra, lib, problem, run.batch, SEEDS[problem])
    kernel = chunk.fit(3)
    got = chunk.state()
    print(f'{test} {problem}: nregs {nregs}, three iterations in one call ran {kernel}')
    for i in range(3):
        tensors, variables = run.tensors(singles[i - 1]['params'] if i else run.flat_start)
        l32 = _evaluate(oracles[torch.float32], tensors, variables, chunk.points(i))[0]
        l64 = _evaluate(oracles[torch.float64], tensors, variables, chunk.points(i))[0]
        ok, err, arb = close_or_arbitrated([float(got['losses'][i])], [l32], lambda: [l64], LOSS_RTOL, atol=0.0)
        record_margin(test, f'{problem}/chunk/it{i}', 'loss', err, LOSS_RTOL, arb)
        print(f'{test} {problem} chunk it {i}: loss ours {float(got["losses"][i]):.9g} f32 {l32:.9g} f64 {l64:.9g} err {err:.2e}')
        assert ok, (problem, i, float(got['losses'][i]), l32, l64)
    assert kernel.startswith('pinn_tile_kernel<'), kernel              # the chunk declined the one-launch form
    _same_bits(got, singles[-1], problem)                               # same kernels, same arguments as the one-iteration calls


# ---- the tests: emulator (CPU tier) and device twins ---------------------------------------------------------------------------------------------
slow_emu = pytest.mark.skipif(not SLOW, reason='nine seconds on the emulator: PYDENS_AMD_SLOW_EMU=1')
C_CASES = [(opt, frozen) for opt in (('Adam', {}), SGD) for frozen in ((), (1,))]
C_IDS = [f'{opt[0].lower()}-{"frozen_middle" if frozen else "all_trainable"}' for opt, frozen in C_CASES]


def _emu(pa, emu_lib, monkeypatch):
    monkeypatch.setattr(pa.Solver, 'FIT_CTRL_ON_HOST', True)
    return dict(_lib=emu_lib, device='cpu')


@pytest.mark.parametrize('batch', [100, 1])
def test_config_1_every_iteration_and_every_split_on_the_emulator(pa, emu_lib, monkeypatch, batch):
    _case_a(pa, _emu(pa, emu_lib, monkeypatch), emu_lib, monkeypatch, 'emu_fit_chunk', batch)


@pytest.mark.gpu
@pytest.mark.parametrize('batch', [100, 1])
def test_config_1_every_iteration_and_every_split_on_the_gpu(pa, gpu_lib, monkeypatch, batch):
    _case_a(pa, {}, gpu_lib, monkeypatch, 'gpu_fit_chunk', batch)


@pytest.mark.parametrize('name', list(B_CASES))
def test_tile_counts_around_the_virtual_workgroups_on_the_emulator(pa, emu_lib, monkeypatch, name):
    _case_b(pa, _emu(pa, emu_lib, monkeypatch), emu_lib, monkeypatch, 'emu_fit_chunk', name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(B_CASES))
def test_tile_counts_around_the_virtual_workgroups_on_the_gpu(pa, gpu_lib, monkeypatch, name):
    _case_b(pa, {}, gpu_lib, monkeypatch, 'gpu_fit_chunk', name)


@pytest.mark.parametrize('opt,frozen', C_CASES, ids=C_IDS)
def test_second_pass_of_the_update_sweep_on_the_emulator(pa, emu_lib, monkeypatch, opt, frozen):
    _case_c(pa, _emu(pa, emu_lib, monkeypatch), emu_lib, monkeypatch, 'emu_fit_chunk', opt, frozen)


@pytest.mark.gpu
@pytest.mark.parametrize('opt,frozen', C_CASES, ids=C_IDS)
def test_second_pass_of_the_update_sweep_on_the_gpu(pa, gpu_lib, monkeypatch, opt, frozen):
    _case_c(pa, {}, gpu_lib, monkeypatch, 'gpu_fit_chunk', opt, frozen)


def test_program_with_a_trainable_variable_on_the_emulator(pa, emu_lib, monkeypatch):
    _case_d(pa, _emu(pa, emu_lib, monkeypatch), emu_lib, monkeypatch, 'emu_fit_chunk')


@pytest.mark.gpu
def test_program_with_a_trainable_variable_on_the_gpu(pa, gpu_lib, monkeypatch):
    _case_d(pa, {}, gpu_lib, monkeypatch, 'gpu_fit_chunk')


@slow_emu
def test_residency_limit_on_the_emulator(pa, emu_lib, monkeypatch):
    _case_e(pa, _emu(pa, emu_lib, monkeypatch), emu_lib, monkeypatch, 'emu_fit_chunk')


@pytest.mark.gpu
def test_residency_limit_on_the_gpu(pa, gpu_lib, monkeypatch):
    _case_e(pa, {}, gpu_lib, monkeypatch, 'gpu_fit_chunk')


@pytest.mark.gpu
def test_grid_form_every_iteration_and_every_split_on_the_gpu(pa, gpu_lib, monkeypatch):
    """ (f) PYDENS_AMD_FIT_PERSIST=1: resident workgroups with a device-scope wait -- the form and shape
    test_fit_chunk_as_one_launch_follows_the_eager_loop runs with 430 iterations, here with 8 and every one of them checked """
    _case_a(pa, {}, gpu_lib, monkeypatch, 'gpu_fit_chunk_grid', 100, persist=1)


def test_declined_chunk_leaves_no_timeout_flag_of_an_earlier_chunk_on_the_emulator(pa, emu_lib, monkeypatch):
    """ pinn_fit_chunk_status reads the flag of the LAST grid-form chunk of the thread. A later chunk that declines the one-launch form must
    not leave it pointing at the earlier chunk's flag: that workspace memory has another use by then. (One tile: the emulator runs the grid
    form on a grid of one workgroup.) The workspace stays allocated throughout; nothing is freed. """
    _env(monkeypatch, 1, 4)
    run = Run(pa, _emu(pa, emu_lib, monkeypatch), emu_lib, 'ode_16', TILE, SEEDS['ode_16'])
    kernel = run.fit(1)
    assert kernel.startswith('pinn_fit_kernel<') and _vw(kernel) == 1, kernel          # the grid form
    assert emu_lib.pinn_fit_chunk_status() == 0
    workspaces = list(run.solver.model._workspaces.values())
    assert workspaces
    for ws in workspaces:
        ws.view(torch.uint8).fill_(0xA5)
    monkeypatch.setenv('PYDENS_AMD_FIT_PERSIST', '2')       # (Solver.fit asks for the status itself under '1')
    net = run.solver.model.net
    assert net.lib.pinn_debug_fit_persistent(net.handle, 0) == 1
    kernel = run.fit(1)
    assert kernel.startswith('pinn_tile_kernel<'), kernel                               # declined: the launch graphs
    assert emu_lib.pinn_fit_chunk_status() == 0


# (room: registers the in-kernel pre-pass holds = PinnCfg::PREPASS_FLOATS_PER_LANE / 2 of the problem's kernel)
WIDE_ROOM = {'wide_prepass_16': 24}


@pytest.mark.parametrize('problem', list(WIDE_ROOM))
def test_prepass_outside_the_kernel_declines_the_one_launch_chunk_on_the_emulator(pa, emu_lib, monkeypatch, problem):
    _case_wide_prepass(pa, _emu(pa, emu_lib, monkeypatch), emu_lib, monkeypatch, 'emu_fit_chunk', problem, WIDE_ROOM[problem])


@pytest.mark.gpu
@pytest.mark.parametrize('problem', list(WIDE_ROOM))
def test_prepass_outside_the_kernel_declines_the_one_launch_chunk_on_the_gpu(pa, gpu_lib, monkeypatch, problem):
    _case_wide_prepass(pa, {}, gpu_lib, monkeypatch, 'gpu_fit_chunk', problem, WIDE_ROOM[problem])


# ---- no reference tensor at its floor (CPU tier, fp64 oracle alone: also for the cases whose kernels run on the device only) --------------------
# (the batch sizes the kernel cases arrive at with VW = 8 at width 16 and VW = 3 at width 32; those cases assert the floors again themselves)
FLOOR_CASES = ([('cfg1', n, ('Adam', {}), ()) for n in (100, 1)] + [('cfg1', 100, SGD, ())] +
               [('ode_16', n, ('Adam', {}), ()) for n in (16, 112, 128, 144, 131, 256, 512, 272)] +
               [('ode_32x3', 40, opt, frozen) for opt, frozen in C_CASES] + [('program_with_variable', 90, ('Adam', {}), ())] +
               [('eight_columns', n * TILE, ('Adam', {}), ()) for n in (1, 12)] + [('wide_prepass_16', 3 * TILE + 5, ('Adam', {}), ())])


@pytest.mark.parametrize('problem,batch,opt,frozen', FLOOR_CASES, ids=[f'{p}-n{n}-{o[0].lower()}-{len(f)}' for p, n, o, f in FLOOR_CASES])
def test_no_reference_gradient_sits_at_the_floor(problem, batch, opt, frozen):
    """ a tensor whose fp64 gradient is below the rule's floor 1e-9 sqrt(size) would pass whatever the kernel wrote: along the fp64 oracle's
    own K iterations on the Philox batches of the case's seed there is none (the kernel cases assert it again on their trajectories) """
    import pydens_amd as pa
    from oracle import philox
    from oracle import pinn_oracle as po
    seed = SEEDS[problem]
    torch.manual_seed(seed)
    eq, kw, columns, names = _problem(problem, po.D, po.V)
    start = po.OracleSolver(eq, **kw).export_params()
    oracle = po.OracleSolver(_problem(problem, po.D, po.V)[0], dtype=torch.float64, **kw)
    oracle.import_params(start)
    linears = list(oracle.model.linears())
    frozen_ids = {id(p) for i in frozen for p in linears[i].parameters()}
    live = [p for p in oracle.model.parameters() if id(p) not in frozen_ids]
    optim = getattr(torch.optim, opt[0])(live, lr=LR, **opt[1])
    key = _sampler(pa, columns, seed).device_key()
    for i in range(K):
        pts = philox.sample_points(batch, [(philox.UNIFORM, lo, hi) for lo, hi in columns], key, i)
        oracle.evaluate(pts)
        for j, g in enumerate(oracle.export_grads()):
            if g is not None:
                assert float(np.linalg.norm(g)) > 1e-9 * np.sqrt(g.size), (problem, batch, i, j)
        for n in names:
            assert abs(float(getattr(oracle.model, n).grad)) > 1e-9, (problem, batch, i, n)
        optim.step()
