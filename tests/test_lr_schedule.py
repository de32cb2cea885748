""" Learning-rate schedules in `Solver.fit` (`lr_scheduler=`, `lr_scheduler_kwargs=`): torch's own scheduler objects compute every rate on the
host; the rates reach the kernels per iteration -- by value on the eager paths, through the control block of the fit chunks (include/pinn.h
lr_steps of pinn_fit_steps), whose launch graph and one-CU kernel go on running while the rate changes under them. CPU tier on the emulator
build of the product sources, `-m gpu` twins on the device.

Tolerances are the suite's own. Chunk forms against the per-iteration calls: the eager chunk and the launch-graph chunk bit for bit, the
one-CU kernel at the bounds of test_emu_engine._one_launch_case. `Solver.fit` against a torch loop (torch.optim + the real scheduler object on
the same kernel gradients): LOSS_RTOL / PARAM_RTOL of test_fused_optimizers -- both sides take their gradients from the same kernels, so only
the update arithmetic differs. L-BFGS: the bounds of test_lbfgs. Data parallel: the 1e-5 of test_data_parallel. `solver.lrs` against the
scheduler's own rates: equal as Python floats. """
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

from conftest import params_close
from helpers import FixedBatches, export_params, load_params, make_solver

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'emu'))

LOSS_RTOL, PARAM_RTOL = 1e-5, 3e-5
LR = 0.005


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


def _poisson(D):
    eq = lambda u, x, y: D(D(u, x), x) + D(D(u, y), y) - 5.0 * torch.sin(np.pi * (x + y))
    return eq, dict(ndims=2, boundary_condition=1.0, layout='fa f', features=[16, 1], activation='Tanh')       # the net [2, 16, 1]


def _stats(lib):
    st = (ctypes.c_int32 * 4)()
    lib.pinn_debug_fit_graph_stats(st)
    return [int(v) for v in st]


def scheduler_rates(build, lr, n, optimizer=torch.optim.SGD):
    """ what `param_groups[0]['lr']` reads in front of step k = 0 .. n-1 of the torch loop `opt.step(); sched.step()` """
    opt = optimizer([torch.zeros(1, requires_grad=True)], lr=lr)
    sched = build(opt)
    rates = []
    for _ in range(n):
        rates.append(float(opt.param_groups[0]['lr']))
        opt.step()
        sched.step()
    return rates


# ---- 1. kernel contract: a chunk with a table of rates is the per-iteration calls with lr_k by value --------------------------------------------
RULES = {'adam': ('Adam', {}), 'adam_wd': ('Adam', dict(weight_decay=0.01)), 'adamw': ('AdamW', dict(weight_decay=0.1)),
         'sgd_nesterov': ('SGD', dict(momentum=0.9, nesterov=True)), 'rmsprop_momentum': ('RMSprop', dict(momentum=0.9)),
         'rmsprop_centered': ('RMSprop', dict(centered=True))}


def rate_table(k, scale=1.0):
    """ non-monotone: warm-up over four steps, then decay, one entry exactly 0.0 """
    table = [scale * LR * (i + 1) / 4 for i in range(min(4, k))] + [scale * LR * 0.97 ** i for i in range(max(0, k - 4))]
    if k > 6:
        table[6] = 0.0
    return table


def _contract_run(pa, extra, monkeypatch, rule, tables, form):
    """ cfg1 at batch 100 on buffers of the test's own. form: 'steps' -- sample_points + residual_optim_step per iteration with the
    rate in the struct; 'eager' -- fit_steps(lr_steps=) without a control block; 'graph' / 'one_cu' -- with one, the narrow net's one-launch
    form off / on """
    from pydens_amd.solver import FlatOptimizer
    monkeypatch.setenv('PYDENS_AMD_FIT_PERSIST', '2' if form == 'one_cu' else '0')
    monkeypatch.setenv('PYDENS_AMD_FIT_ROUNDS', '4')
    torch.manual_seed(21)
    cfg, solver = make_solver('cfg1', pa, **extra)
    model, spec = solver.model, solver.spec
    net, flat = model.net, model.flat
    name, kw = RULES[rule]
    optim = pa.engine.Optim.build(FlatOptimizer.RULES[name][0], **FlatOptimizer.hyper(name, LR, kw))
    comb_w = solver.residual_plan.comb_w if solver.residual_plan is not None else None
    n2 = spec.n2p if comb_w is None else 1
    batch, total = 100, sum(len(t) for t in tables)
    ws = model.workspace(batch, spec.nd, spec.n2p)
    xs = torch.empty((batch, model.total), dtype=torch.float32, device=flat.device)
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    step = torch.zeros(1, dtype=torch.int32, device=flat.device)
    mask = model.trainable_mask()
    history = torch.zeros(total, dtype=torch.float32, device=flat.device)
    columns = solver._device_columns(None)
    ctrl = None
    if form in ('graph', 'one_cu'):
        ctrl = torch.zeros(int(net.lib.pinn_fit_ctrl_bytes()) + 64, dtype=torch.uint8, device=flat.device)
    common = dict(dir_cols=spec.dir_cols, n2=n2, ic_const=model.kernel_ic_const())
    seed, at = 1234, 0
    st0 = _stats(net.lib)
    for table in tables:
        k = len(table)
        if form == 'steps':
            for j, rate in enumerate(table):
                net.sample_points(xs, columns, seed, at + j)
                optim.lr = rate
                net.residual_optim_step(solver.program, flat, xs, solver.grads, ws, m, v, mask, step, at + j + 1, optim,
                                        loss_out=history.data_ptr() + 4 * (at + j), **common)
        else:
            net.fit_steps(solver.program, flat, xs, columns, seed, at, solver.grads, ws, m, v, mask, step, at + 1, optim,
                          history[at:at + k], k, ctrl=ctrl, lr_steps=table, **common)
        at += k
    st = _stats(net.lib)
    return dict(params=flat.detach().clone(), m=m, v=v, step=step.clone(), losses=history, kernel=net.lib.pinn_last_kernel_name().decode(),
                stats=[b - a for a, b in zip(st0, st)])


def _contract_case(pa, extra, monkeypatch, rule, lengths, on_gpu):
    tables = [rate_table(k, scale=1.0 - 0.3 * i) for i, k in enumerate(lengths)]
    want = _contract_run(pa, extra, monkeypatch, rule, tables, 'steps')
    assert np.isfinite(want['losses'].cpu().numpy()).all() and int(want['step']) == sum(lengths)
    for form in ('eager', 'graph'):
        got = _contract_run(pa, extra, monkeypatch, rule, tables, form)
        for key in ('params', 'm', 'v', 'step', 'losses'):
            assert torch.equal(got[key], want[key]), (form, key)
        if on_gpu and form == 'graph':
            assert got['stats'][1] == 1 and got['stats'][0] >= 1 and got['stats'][2] == 0, got['stats']
    got = _contract_run(pa, extra, monkeypatch, rule, tables, 'one_cu')
    assert got['kernel'].startswith('pinn_fit_kernel<') and not got['kernel'].endswith(',1>'), got['kernel']
    assert got['stats'][0] >= len(tables) and int(got['step']) == sum(lengths)
    a, b = want['losses'].cpu().numpy(), got['losses'].cpu().numpy()
    rel = np.abs(b / a - 1)
    print(f'{rule}: one-CU chunk under a schedule against the per-iteration calls: loss rel err first 8 {rel[:8].max():.2e}, all {rel.max():.2e}')
    np.testing.assert_allclose(b[:8], a[:8], rtol=2e-6)
    np.testing.assert_allclose(b, a, rtol=2e-4)
    assert params_close(got['params'].cpu().numpy(), want['params'].cpu().numpy(), 2e-4)
    assert params_close(got['m'].cpu().numpy(), want['m'].cpu().numpy(), 2e-3, atol=1e-7)
    assert params_close(got['v'].cpu().numpy(), want['v'].cpu().numpy(), 2e-3, atol=1e-9)


@pytest.mark.parametrize('rule', list(RULES))
def test_chunk_with_a_rate_table_is_the_per_iteration_calls(pa, emu_lib, monkeypatch, rule):
    _contract_case(pa, emu_kwargs(emu_lib), monkeypatch, rule, (9, 4), False)


@pytest.mark.gpu
@pytest.mark.parametrize('rule', list(RULES))
def test_chunk_with_a_rate_table_is_the_per_iteration_calls_on_the_gpu(pa, monkeypatch, rule):
    """ two whole chunks (the second replays the recording of the first under other rates) and a tail """
    _contract_case(pa, {}, monkeypatch, rule, (128, 128, 5), True)


def test_rate_tables_are_validated(pa, emu_lib, monkeypatch):
    with pytest.raises(RuntimeError, match='invalid learning rate'):
        _contract_run(pa, emu_kwargs(emu_lib), monkeypatch, 'adam', [[LR, -LR, LR]], 'eager')
    with pytest.raises(RuntimeError, match='invalid learning rate'):
        _contract_run(pa, emu_kwargs(emu_lib), monkeypatch, 'sgd_nesterov', [[LR, float('nan')]], 'graph')


# ---- 2. a recorded chunk survives a change of rate ------------------------------------------------------------------------------------------
def _fit_run(pa, extra, monkeypatch, graph, persist, niters, chunk=None, per_iteration=False, optimizer='Adam', okw=None, seeded=False, small=False, **sched):
    monkeypatch.setenv('PYDENS_AMD_FIT_GRAPH', '1' if graph else '0')
    monkeypatch.setenv('PYDENS_AMD_FIT_PERSIST', str(persist))
    monkeypatch.setenv('PYDENS_AMD_FIT_ROUNDS', '4')
    if chunk is not None:
        monkeypatch.setattr(pa.Solver, 'FIT_CHUNK', chunk)
    torch.manual_seed(21)
    if small:                   # the net [2, 16, 1] at batch 32: one tile per iteration
        eq, skw = _poisson(pa.D)
        solver, batch = pa.Solver(eq, **skw, **extra), 32
    else:
        solver, batch = make_solver('cfg1', pa, **extra)[1], 100
    solver.set_optimizer_path('fused')
    if per_iteration:
        solver._device_columns = lambda sampler: None           # the per-iteration loop (pinn_residual_optim_step)
    st0 = _stats(solver.model.net.lib)
    first = True
    # (seeded: the sampler's own Philox key and batch counter -- the point stream does not depend on how the fit calls cut it)
    sampler = pa.NumpySampler('uniform', dim=2, seed=7) if seeded else None
    for n in niters:
        solver.fit(niters=n, batch_size=batch, sampler=sampler, lr=LR, optimizer=optimizer if first else None, **(okw or {}) if first else {},
                   **(sched if first else {}))
        first = False
    assert solver.last_fit_path == 'fused'
    st = _stats(solver.model.net.lib)
    opt = solver.optimizer
    return dict(losses=np.array([float(v) for v in solver.losses]), params=solver.model.flat.detach().cpu().numpy().copy(),
                m=opt.exp_avg.cpu().numpy().copy(), v=opt.exp_avg_sq.cpu().numpy().copy(), t=int(opt.step_count.item()), host_t=opt.t,
                lrs=list(solver.lrs), stats=[b - a for a, b in zip(st0, st)], solver=solver)


def _same(a, b):
    for key in ('losses', 'params', 'm', 'v'):
        assert np.array_equal(a[key], b[key]), key
    assert a['lrs'] == b['lrs'] and a['t'] == b['t'] == a['host_t'] == b['host_t']


def _replay_case(pa, extra, monkeypatch, chunk, on_gpu):
    """ three whole chunks, another rate in each: ONE recording, replayed; the eager loop's trajectory bit for bit """
    sched = dict(lr_scheduler='StepLR', lr_scheduler_kwargs=dict(step_size=chunk, gamma=0.5))
    for optimizer, okw in (('Adam', {}), ('SGD', dict(momentum=0.9))):
        eager = _fit_run(pa, extra, monkeypatch, False, 0, (3 * chunk, ), chunk=chunk, optimizer=optimizer, okw=okw, **sched)
        graph = _fit_run(pa, extra, monkeypatch, True, 0, (3 * chunk, ), chunk=chunk, optimizer=optimizer, okw=okw, **sched)
        assert graph['lrs'] == [LR] * chunk + [LR * 0.5] * chunk + [LR * 0.25] * chunk
        assert np.isfinite(graph['losses']).all()
        _same(eager, graph)
        if on_gpu:
            assert graph['stats'][1] == 1 and graph['stats'][0] >= 1 and graph['stats'][2] == 0, graph['stats']
            assert eager['stats'][:3] == [0, 0, 0], eager['stats']


def test_chunks_with_another_rate_each_follow_the_eager_loop(pa, emu_lib, monkeypatch):
    """ (the emulator records nothing: the entry point with a control block against the one without, four iterations per chunk) """
    monkeypatch.setattr(pa.Solver, 'FIT_CTRL_ON_HOST', True)
    _replay_case(pa, emu_kwargs(emu_lib), monkeypatch, 4, False)


@pytest.mark.gpu
def test_recorded_chunk_is_replayed_under_another_rate_on_the_gpu(pa, monkeypatch):
    _replay_case(pa, {}, monkeypatch, 128, True)


# ---- 3. a constant schedule is no schedule ------------------------------------------------------------------------------------------------------
def _constant_case(pa, extra, monkeypatch, niters):
    const = dict(lr_scheduler='LambdaLR', lr_scheduler_kwargs=dict(lr_lambda=lambda e: 1.0))
    for per_iteration in (False, True):
        for optimizer, okw in (('Adam', {}), ('AdamW', dict(weight_decay=0.1))):
            plain = _fit_run(pa, extra, monkeypatch, True, 2, niters, per_iteration=per_iteration, optimizer=optimizer, okw=okw)
            sched = _fit_run(pa, extra, monkeypatch, True, 2, niters, per_iteration=per_iteration, optimizer=optimizer, okw=okw, **const)
            assert plain['solver'].lr_scheduler is None and sched['solver'].lr_scheduler is not None
            assert sched['lrs'] == [LR] * sum(niters)
            _same(plain, sched)


def test_constant_schedule_is_no_schedule(pa, emu_lib, monkeypatch):
    monkeypatch.setattr(pa.Solver, 'FIT_CTRL_ON_HOST', True)
    _constant_case(pa, emu_kwargs(emu_lib), monkeypatch, (5, 3))


@pytest.mark.gpu
def test_constant_schedule_is_no_schedule_on_the_gpu(pa, monkeypatch):
    _constant_case(pa, {}, monkeypatch, (140, 20))


# ---- 4. Solver.fit against the torch loop ---------------------------------------------------------------------------------------------------------
NITERS = 12
SCHEDULERS = {
    'ExponentialLR': ('ExponentialLR', dict(gamma=0.9)),
    'MultiStepLR': ('MultiStepLR', dict(milestones=[3, 7], gamma=0.3)),
    'CosineAnnealingWarmRestarts': ('CosineAnnealingWarmRestarts', dict(T_0=5, eta_min=1e-4)),
    'OneCycleLR': ('OneCycleLR', dict(max_lr=0.02, total_steps=NITERS, cycle_momentum=False)),
    'SequentialLR': (lambda opt: torch.optim.lr_scheduler.SequentialLR(
        opt, [torch.optim.lr_scheduler.LinearLR(opt, start_factor=0.2, total_iters=4), torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.8)],
        milestones=[4]), None)}
TORCH_OPTIMIZERS = {'adam': ('Adam', {}), 'adamw': ('AdamW', dict(weight_decay=0.1)), 'sgd': ('SGD', dict(momentum=0.9, nesterov=True))}


def _builder(which):
    spec, kw = SCHEDULERS[which]
    return (lambda opt: getattr(torch.optim.lr_scheduler, spec)(opt, **kw)) if isinstance(spec, str) else spec


def _torch_loop(pa, extra, start, pts, name, okw, build):
    """ torch.optim.<name> and the real scheduler object on a twin's parameters, fed with the gradients of the gradient-only residual step """
    eq, skw = _poisson(pa.D)
    twin = pa.Solver(eq, **skw, **extra)
    load_params(twin, start)
    unreached = set(twin._unreached_scalars(('equation', ), [], nn.MSELoss()))
    params = [p for p in twin.model.optimizer_parameters()]
    opt = getattr(torch.optim, name)(params, lr=LR, **okw)
    sched = build(opt)
    off_loss = twin.model.net.layout.off_loss
    losses, rates = [], []
    for batch in pts:
        twin._fused_step(torch.from_numpy(batch).to(twin.device), 1)
        losses.append(float(twin.grads[off_loss]))
        for p in params:
            reached = p.storage_offset() not in unreached
            p.grad = twin.grads.as_strided(tuple(p.shape), tuple(p.stride()), p.storage_offset()).clone() if reached else None
        rates.append(float(opt.param_groups[0]['lr']))
        opt.step()
        sched.step()
    return np.array(losses), export_params(twin), rates


def _torch_case(pa, extra, which, opt, batch):
    name, okw = TORCH_OPTIMIZERS[opt]
    spec, skw_ = SCHEDULERS[which]
    eq, skw = _poisson(pa.D)
    torch.manual_seed(5)
    solver = pa.Solver(eq, **skw, **extra)
    start = export_params(solver)
    pts = np.random.RandomState(17).rand(NITERS, batch, 2).astype(np.float32)
    want_losses, want_params, want_rates = _torch_loop(pa, extra, start, pts, name, okw, _builder(which))
    solver.set_optimizer_path('fused')
    solver.fit(niters=NITERS, batch_size=batch, sampler=FixedBatches(pts), lr=LR, optimizer=name, lr_scheduler=spec, lr_scheduler_kwargs=skw_, **okw)
    assert solver.last_fit_path == 'fused' and solver.last_fit_optimizer == f'{name}/fused'
    assert solver.lrs == want_rates and len(set(want_rates)) > 2
    got = np.array([float(v) for v in solver.losses])
    print(f'{which}/{opt}: loss rel err vs the torch loop {np.abs(got / want_losses - 1).max():.2e}')
    np.testing.assert_allclose(got, want_losses, rtol=LOSS_RTOL)
    for i, (p, w) in enumerate(zip(export_params(solver), want_params)):
        assert params_close(p, w, PARAM_RTOL), (i, p, w)


@pytest.mark.parametrize('opt', list(TORCH_OPTIMIZERS))
@pytest.mark.parametrize('which', list(SCHEDULERS))
def test_fit_with_a_scheduler_follows_the_torch_loop(pa, emu_lib, which, opt):
    _torch_case(pa, emu_kwargs(emu_lib), which, opt, 40)


@pytest.mark.gpu
@pytest.mark.parametrize('opt', list(TORCH_OPTIMIZERS))
@pytest.mark.parametrize('which', list(SCHEDULERS))
def test_fit_with_a_scheduler_follows_the_torch_loop_on_the_gpu(pa, which, opt):
    _torch_case(pa, {}, which, opt, 97)


# ---- 5. chunk boundary, continuation, interruption ------------------------------------------------------------------------------------------------
EXP = dict(lr_scheduler='ExponentialLR', lr_scheduler_kwargs=dict(gamma=0.99))


WHOLE = {}      # fit(131) per device: computed once, shared, left unchanged


def _boundary_case(pa, extra, monkeypatch, per_iteration):
    """ fit(131) crosses a chunk boundary; fit(70) + fit(61, optimizer=None) is the same trajectory, on the eager chunk and on the
    per-iteration loop """
    device = extra.get('device', 'cuda')
    if device not in WHOLE:
        want_rates = scheduler_rates(lambda opt: torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.99), LR, 131)
        WHOLE[device] = whole = _fit_run(pa, extra, monkeypatch, False, 0, (131, ), seeded=True, small=True, **EXP)
        assert whole['lrs'] == want_rates and whole['t'] == 131
    split = _fit_run(pa, extra, monkeypatch, False, 0, (70, 61), per_iteration=per_iteration, seeded=True, small=True, **EXP)
    _same(WHOLE[device], split)
    return WHOLE[device]


@pytest.mark.parametrize('per_iteration', [False, True], ids=['chunks', 'per_iteration'])
def test_schedule_crosses_chunks_and_fit_calls(pa, emu_lib, monkeypatch, per_iteration):
    _boundary_case(pa, emu_kwargs(emu_lib), monkeypatch, per_iteration)


@pytest.mark.gpu
def test_schedule_crosses_chunks_and_fit_calls_on_the_gpu(pa, monkeypatch):
    _boundary_case(pa, {}, monkeypatch, False)
    whole = _boundary_case(pa, {}, monkeypatch, True)
    # ... and the default forms on the device (one-CU chunks) follow it at their bound
    one_cu = _fit_run(pa, {}, monkeypatch, True, 2, (70, 61), seeded=True, small=True, **EXP)
    assert one_cu['lrs'] == whole['lrs']
    np.testing.assert_allclose(one_cu['losses'], whole['losses'], rtol=2e-4)


def _interrupted_case(pa, extra, monkeypatch, chunk):
    """ an interrupt on the host between two chunks: the rates drawn for the chunk that never ran stay queued """
    monkeypatch.setenv('PYDENS_AMD_FIT_GRAPH', '0')
    monkeypatch.setenv('PYDENS_AMD_FIT_PERSIST', '0')
    monkeypatch.setattr(pa.Solver, 'FIT_CHUNK', chunk)
    want = scheduler_rates(lambda opt: torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.99), LR, 2 * chunk + 3, torch.optim.Adam)
    torch.manual_seed(21)
    cfg, solver = make_solver('cfg1', pa, **extra)
    real, calls = solver.model.net.fit_steps, []

    def second_call_never_starts(*args, **kw):
        calls.append(1)
        if len(calls) == 2:
            raise KeyboardInterrupt
        real(*args, **kw)
    monkeypatch.setattr(solver.model.net, 'fit_steps', second_call_never_starts)
    sampler = pa.NumpySampler('uniform', dim=2, seed=7)           # (its own key and batch counter, across fit calls)
    with pytest.raises(KeyboardInterrupt):
        solver.fit(niters=2 * chunk, batch_size=100, sampler=sampler, lr=LR, **EXP)
    opt = solver.optimizer
    assert opt.t == chunk == int(opt.step_count.item())
    assert solver.lrs == want[:chunk] and solver._lr_queue == want[chunk:2 * chunk]
    monkeypatch.setattr(solver.model.net, 'fit_steps', real)
    solver.fit(niters=3, batch_size=100, sampler=sampler, lr=LR, optimizer=None)
    assert opt.t == chunk + 3 == int(opt.step_count.item())
    assert solver.lrs == want[:chunk + 3] and len(solver.losses) == chunk + 3
    # the same steps without the interruption
    torch.manual_seed(21)
    cfg, twin = make_solver('cfg1', pa, **extra)
    twin.fit(niters=chunk + 3, batch_size=100, sampler=pa.NumpySampler('uniform', dim=2, seed=7), lr=LR, **EXP)
    assert torch.equal(twin.model.flat, solver.model.flat)
    # a NEW scheduler over the same optimizer: torch's initial_lr rules, from the rate of the next step
    solver.fit(niters=2, batch_size=100, optimizer=None, lr_scheduler='ExponentialLR', lr_scheduler_kwargs=dict(gamma=0.5))
    # (ExponentialLR's chainable form starts from the group's CURRENT rate -- that of step chunk + 4 of the first schedule -- as in torch)
    assert solver.lrs[-2:] == scheduler_rates(lambda opt: torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.5), want[chunk + 3], 2)
    assert solver.lr_scheduler.base_lrs == [LR]                 # (initial_lr of the group stays the first scheduler's: torch's setdefault)


def test_interrupt_between_chunks_keeps_the_queue(pa, emu_lib, monkeypatch):
    _interrupted_case(pa, emu_kwargs(emu_lib), monkeypatch, 4)


@pytest.mark.gpu
def test_interrupt_between_chunks_keeps_the_queue_on_the_gpu(pa, monkeypatch):
    _interrupted_case(pa, {}, monkeypatch, 128)


# ---- 6. every other step path ---------------------------------------------------------------------------------------------------------------------
def _heat(D, V):
    eq = lambda u, x, t: D(u, t) - 0.1 * D(D(u, x), x) - 2.0 * torch.cos(3.0 * x + t)
    kw = dict(ndims=2, boundary_condition=0.0, initial_condition=lambda x: torch.sin(np.pi * x), layout='fa f', features=[16, 1], activation='Tanh')
    con = lambda f, x, t: f(torch.tensor([0.4]), torch.tensor([0.6])) - 0.2
    return eq, dict(kw, constraints=con)


class LogCosh(nn.Module):
    """ a criterion the kernels do not carry: the generic step """
    def forward(self, got, target):
        return torch.log(torch.cosh(got - target)).mean()


PATHS = {'torch_adagrad': dict(optimizer='Adagrad'), 'generic_step': dict(criterion=LogCosh()),
         'constraint_term': dict(loss_terms=['equation', 'constraint_0']),
         'lbfgs': dict(optimizer='LBFGS', max_iter=3, history_size=4, lr=0.5)}
PATH_STEPS = 6
PATH_SCHED = dict(lr_scheduler='StepLR', lr_scheduler_kwargs=dict(step_size=2, gamma=0.5))


def _poke(solver, rate):
    """ the workaround a schedule replaces: the optimizer's rate set from outside between two fit calls of one iteration """
    from pydens_amd.solver import TorchOptimizerAdapter
    opt = solver.optimizer
    if isinstance(opt, TorchOptimizerAdapter):
        for group in opt.opt.param_groups:
            group['lr'] = rate
    else:
        opt.lr = rate
        if opt.optim is not None:
            opt.optim.lr = rate


def _path_case(pa, extra, which):
    from pydens_amd.solver import FlatLBFGS, TorchOptimizerAdapter
    fit_kw = dict(PATHS[which])
    lr = fit_kw.pop('lr', LR)
    want_rates = scheduler_rates(lambda opt: torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5), lr, PATH_STEPS)
    pts = np.random.RandomState(23).rand(PATH_STEPS, 40, 2).astype(np.float32)
    eq, skw = _heat(pa.D, pa.V)
    torch.manual_seed(9)
    solver = pa.Solver(eq, **skw, **extra)
    start = export_params(solver)
    solver.set_optimizer_path('fused')
    solver.fit(niters=PATH_STEPS, batch_size=40, sampler=FixedBatches(pts), lr=lr, **fit_kw, **PATH_SCHED)
    assert solver.lrs == want_rates
    expect = {'torch_adagrad': ('fused', 'Adagrad/torch'), 'generic_step': ('generic', 'Adam/fused'),
              'constraint_term': ('fused', 'Adam/fused'), 'lbfgs': ('fused', 'LBFGS/fused')}[which]
    assert (solver.last_fit_path, solver.last_fit_optimizer) == expect
    assert isinstance(solver.optimizer, FlatLBFGS) == (which == 'lbfgs')
    assert (solver.lr_scheduler.optimizer is getattr(solver.optimizer, 'opt', None)) == isinstance(solver.optimizer, TorchOptimizerAdapter)
    # the twin: torch's own optimizer where there is one to compare with (L-BFGS), one-iteration fit calls with the rate set from outside
    twin = pa.Solver(eq, **skw, **extra)
    load_params(twin, start)
    if which != 'lbfgs':
        twin.set_optimizer_path('fused')
    for k, rate in enumerate(want_rates):
        if k == 0:
            twin.fit(niters=1, batch_size=40, sampler=FixedBatches(pts[:1]), lr=rate, **fit_kw)
        else:
            _poke(twin, rate)
            kw = {key: v for key, v in fit_kw.items() if key in ('criterion', 'loss_terms')}
            twin.fit(niters=1, batch_size=40, sampler=FixedBatches(pts[k:k + 1]), optimizer=None, **kw)
    got, want = np.array([float(v) for v in solver.losses]), np.array([float(v) for v in twin.losses])
    print(f'{which}: loss rel err vs its twin {np.abs(got / want - 1).max():.2e}')
    np.testing.assert_allclose(got, want, rtol=LOSS_RTOL)
    for p, w in zip(export_params(solver), export_params(twin)):
        assert params_close(p, w, PARAM_RTOL)
    assert not np.array_equal(got[1:], np.array([float(v) for v in _constant_twin(pa, extra, eq, skw, start, pts, lr, fit_kw).losses])[1:])


def _constant_twin(pa, extra, eq, skw, start, pts, lr, fit_kw):
    """ the same fit at a constant rate: what the schedule must NOT be """
    twin = pa.Solver(eq, **skw, **extra)
    load_params(twin, start)
    twin.set_optimizer_path('fused')
    twin.fit(niters=PATH_STEPS, batch_size=40, sampler=FixedBatches(pts), lr=lr, **fit_kw)
    return twin


@pytest.mark.parametrize('which', list(PATHS))
def test_every_step_path_follows_the_schedule(pa, emu_lib, which):
    _path_case(pa, emu_kwargs(emu_lib), which)


@pytest.mark.gpu
@pytest.mark.parametrize('which', list(PATHS))
def test_every_step_path_follows_the_schedule_on_the_gpu(pa, which):
    _path_case(pa, {}, which)


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _dp_problem(pa, lib):
    torch.manual_seed(21)
    eq, kw = _heat(pa.D, pa.V)
    solver = pa.Solver(eq, **kw, _lib=lib, device='cpu')
    solver.set_optimizer_path('fused')
    rng = np.random.RandomState(3)
    start = [np.asarray(rng.randn(*p.shape) * 0.5, dtype=np.float32) for p in export_params(solver)]
    fit_kw = dict(lr=0.01, loss_terms=['equation', 'constraint_0'], optimizer='SGD', momentum=0.9,
                  lr_scheduler='ExponentialLR', lr_scheduler_kwargs=dict(gamma=0.7))
    return solver, rng.rand(4, 33, 2).astype(np.float32), fit_kw, start


def _dp_worker(rank, world, port, out_dir):
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
    solver, points, fit_kw, start = _dp_problem(pa, lib)
    if rank == 0:
        load_params(solver, start)
    shard = points[:, rank::world]
    solver.fit(niters=points.shape[0], batch_size=points.shape[1], sampler=FixedBatches(shard), **fit_kw)
    assert solver.last_fit_path == 'fused' and solver.last_fit_optimizer == 'SGD/fused'
    np.savez(os.path.join(out_dir, f'rank{rank}.npz'), losses=np.array([float(v) for v in solver.losses]), lrs=np.array(solver.lrs),
             **{f'p{i}': p for i, p in enumerate(export_params(solver))})
    dist.destroy_process_group()


def test_two_ranks_follow_the_schedule_of_the_single_process(pa, emu_lib):
    """ gloo, world 2, uneven shares (33 points): every rank computes the same rates on its host -- as tests/test_data_parallel.py, same bounds """
    single, points, fit_kw, start = _dp_problem(pa, emu_lib)
    load_params(single, start)
    single.fit(niters=points.shape[0], batch_size=points.shape[1], sampler=FixedBatches(points), **fit_kw)
    want_losses, want = np.array([float(v) for v in single.losses]), export_params(single)
    assert single.lrs == scheduler_rates(lambda opt: torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.7), 0.01, points.shape[0])
    with tempfile.TemporaryDirectory() as out_dir:
        mp.spawn(_dp_worker, args=(2, _free_port(), out_dir), nprocs=2, join=True)
        for rank in range(2):
            z = np.load(os.path.join(out_dir, f'rank{rank}.npz'))
            assert list(z['lrs']) == single.lrs
            np.testing.assert_allclose(z['losses'], want_losses, rtol=1e-5)
            for i, w in enumerate(want):
                assert params_close(z[f'p{i}'], w, 1e-5), (rank, i)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------------
def _refusal_case(pa, extra):
    eq, skw = _poisson(pa.D)
    pts = np.random.RandomState(3).rand(8, 24, 2).astype(np.float32)
    solver = pa.Solver(eq, **skw, **extra)
    solver.set_optimizer_path('fused')
    fit = lambda **kw: solver.fit(niters=1, batch_size=24, sampler=FixedBatches(pts), lr=LR, **kw)
    fit(lr_scheduler='ExponentialLR', lr_scheduler_kwargs=dict(gamma=0.5))
    running, first = solver.lr_scheduler, solver.optimizer
    refused = [(NotImplementedError, 'metric-driven', dict(lr_scheduler='ReduceLROnPlateau')),
               (NotImplementedError, 'finite number >= 0', dict(lr_scheduler='LambdaLR', lr_scheduler_kwargs=dict(lr_lambda=lambda e: -1.0))),
               (ValueError, 'no scheduler class of that name', dict(lr_scheduler='HalveEveryFullMoon')),
               (NotImplementedError, 'cycle_momentum=False', dict(lr_scheduler='OneCycleLR', lr_scheduler_kwargs=dict(max_lr=0.1, total_steps=9))),
               (NotImplementedError, 'param groups', dict(lr_scheduler=lambda opt: _second_group(opt)))]
    for error, message, kw in refused:
        with pytest.raises(error, match=message):
            fit(optimizer=None, **kw)
        assert solver.optimizer is first and solver.lr_scheduler is running         # the running schedule goes on ...
    fit(optimizer=None)
    assert solver.lrs == [LR, LR * 0.5]
    for error, message, kw in refused:                                                    # ... a fresh optimizer is left at its constant rate
        for optimizer, okw in (('Adam', {}), ('SGD', dict(momentum=0.9)), ('Adagrad', {})):
            if optimizer == 'Adagrad' and 'cycle_momentum' in message:
                continue                        # (torch's own optimizer: torch itself says what it cannot cycle)
            with pytest.raises(error, match=message):
                fit(optimizer=optimizer, **okw, **kw)
            assert solver.lr_scheduler is None
            before = len(solver.lrs)
            fit(optimizer=None)
            assert solver.lrs[before:] == [LR]
    with pytest.raises(ValueError, match='lr_scheduler_kwargs'):
        fit(lr_scheduler=lambda opt: torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.5), lr_scheduler_kwargs=dict(gamma=0.5))
    # a rate that turns negative in the middle of a fit stops it there
    with pytest.raises(NotImplementedError, match='finite number >= 0'):
        solver.fit(niters=6, batch_size=24, sampler=FixedBatches(pts), lr=LR,
                   lr_scheduler='LambdaLR', lr_scheduler_kwargs=dict(lr_lambda=lambda e: 1.0 - 0.4 * e))
    assert solver.optimizer.t == 3 and solver.lrs[-3:] == pytest.approx([LR, LR * 0.6, LR * 0.2])


def _second_group(opt):
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.5)
    opt.add_param_group(dict(params=[torch.zeros(1, requires_grad=True)]))
    return sched


def test_refused_schedulers_leave_the_optimizer_usable(pa, emu_lib):
    _refusal_case(pa, emu_kwargs(emu_lib))


@pytest.mark.gpu
def test_refused_schedulers_leave_the_optimizer_usable_on_the_gpu(pa):
    _refusal_case(pa, {})
