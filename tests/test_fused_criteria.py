""" Closed-form criteria on the fused step (`Solver.set_criterion_path('fused')`; include/pinn.h PINN_CRIT_*): nn.L1Loss, nn.SmoothL1Loss,
nn.HuberLoss and nn.MSELoss(reduction='sum') evaluated in the point stage of the tile kernels instead of as torch code between
pinn_jet_forward and pinn_jet_backward (reference model_torch.py:396-410, :448, :457: ONE criterion for every term of the loss).
CPU tier on the emulator build of the product sources, `-m gpu` twins on the device.

Tolerances are the suite's own: losses within 1e-5 relative of the oracle, parameters through `close_or_arbitrated` at the 3e-5 of
test_emu_engine.test_residual_kinds_match_the_oracle (the fp64 oracle arbitrates where the fp32 reference is the noisy side), a trainable
V(...) within 2e-5 absolute (test_fuzz_equations._run_variables).

The L1 condition: sign(r) is discontinuous, so a point whose |r| sits at fp32 round-off may flip between two correct fp32 implementations and
move the gradient by 1/N. The L1 cases therefore run on seeds for which the FP64 oracle's residuals satisfy min |r| > 1e-4 max |r| on every
batch of the trajectory -- asserted, no point excluded (seeds scanned on the CPU: SEEDS below). """
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

CRITERIA = {'l1': lambda: nn.L1Loss(), 'smooth_l1': lambda: nn.SmoothL1Loss(beta=0.3), 'huber': lambda: nn.HuberLoss(delta=0.5),
            'mse_sum': lambda: nn.MSELoss(reduction='sum')}
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


# ---- problems: AFFINE residuals (Poisson box; heat with IC + BC), a residual PROGRAM (Burgers with V('nu')), a constraint term ----------
def _problem(which, D, V, dtype=torch.float32):
    """ -> (equation, solver kwargs, loss_terms); untrained nets, O(1) source terms """
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
# seeds (net initialisation and batches) for which the fp64 oracle's L1 trajectory keeps min |r| > 1e-4 max |r| on every batch, per
# (problem, batch size): scanned on the CPU from 0 upwards, first seed with a ratio above 3e-4 (the test asserts the condition again)
SEEDS = {('poisson', 40): 0, ('heat', 40): 1, ('burgers', 40): 0, ('constraint', 40): 0,
         ('poisson', 523): 0, ('heat', 523): 0, ('burgers', 523): 4, ('constraint', 523): 14}


class Recording(nn.Module):
    """ a criterion that notes the residuals it is handed (the oracle takes any callable) """
    def __init__(self, inner):
        super().__init__()
        self.inner, self.seen = inner, []

    def forward(self, value, target):
        self.seen.append(value.detach().cpu().numpy().astype(np.float64).ravel().copy())
        return self.inner(value, target)


def _oracle_run(which, crit_name, seed, batch, dtype, start=None):
    from oracle import pinn_oracle as po
    eq, kw, terms = _problem(which, po.D, po.V, dtype)
    torch.manual_seed(seed)
    oracle = po.OracleSolver(eq, dtype=dtype, **kw)
    if start is not None:
        oracle.import_params(start)
    pts = np.random.RandomState(1000 + seed).rand(NITERS, batch, 2).astype(np.float32)
    rec = Recording(CRITERIA[crit_name]())
    begin = [np.asarray(p, dtype=np.float32) for p in oracle.export_params()]
    oracle.fit(niters=NITERS, batch_size=batch, points=pts, lr=LR, loss_terms=terms, criterion=rec)
    return oracle, pts, rec.seen, begin


def l1_condition(seen):
    """ worst min |r| / max |r| over the batches a criterion saw (terms of one point -- a constraint -- count as they are) """
    return min(float(np.abs(r).min() / max(np.abs(r).max(), 1e-300)) for r in seen)


def _parity_case(pa, extra, which, crit_name, batch):
    seed = SEEDS[(which, batch)]
    oracle, pts, seen32, start = _oracle_run(which, crit_name, seed, batch, torch.float32)
    want = np.array([float(v) for v in oracle.losses])
    oracle64 = []

    def fp64():
        if not oracle64:
            oracle64.append(_oracle_run(which, crit_name, seed, batch, torch.float64, start))
        return oracle64[0]
    if crit_name == 'l1':
        ratio = l1_condition(fp64()[2])
        print(f'{which}/{crit_name}/batch {batch}: fp64 oracle min|r| / max|r| over the trajectory = {ratio:.3e}')
        assert ratio > 1e-4, (which, seed, ratio)
    if crit_name in ('smooth_l1', 'huber') and which == 'poisson':
        # C1 criteria need no such condition; here residuals on BOTH sides of beta / delta, so that both branches are exercised
        edge = 0.3 if crit_name == 'smooth_l1' else 0.5
        for r in seen32:
            assert np.abs(r).min() < edge < np.abs(r).max(), (np.abs(r).min(), np.abs(r).max())
    eq, kw, terms = _problem(which, pa.D, pa.V)
    results = {}
    for path in ('fused', 'generic'):
        torch.manual_seed(seed)
        solver = pa.Solver(eq, **kw, **extra)
        load_params(solver, start)
        solver.set_criterion_path(path)
        solver.fit(niters=NITERS, batch_size=batch, sampler=FixedBatches(pts), lr=LR, loss_terms=terms, criterion=CRITERIA[crit_name]())
        assert solver.last_fit_path == path, (solver.program_error, solver.constraint_errors)
        assert solver.last_fit_criterion == f'{type(CRITERIA[crit_name]()).__name__}/{path}'
        got = np.array([float(v) for v in solver.losses])
        print(f'{which}/{crit_name}/{path}: loss rel err vs oracle {np.abs(got / want - 1).max():.2e}')
        results[path] = (got, export_params(solver), float(solver.model.nu.detach()) if hasattr(solver.model, 'nu') else None)
    for path, (got, params, nu) in results.items():
        np.testing.assert_allclose(got, want, rtol=LOSS_RTOL, err_msg=path)
        for i, (p, w) in enumerate(zip(params, oracle.export_params())):
            ok, err, arb = close_or_arbitrated(p, w, lambda i=i: fp64()[0].export_params()[i], PARAM_RTOL, atol=3e-7, adam_move=LR * NITERS)
            print(f'{which}/{crit_name}/{path}: tensor {i} rel err {err:.2e}{" (fp64 arbiter)" if arb else ""}')
            assert ok, (path, i, err, arb)
        if nu is not None:
            assert abs(nu - float(oracle.model.nu.detach())) < VAR_ATOL, path
    # ... and the two paths of the same build against each other, same rules
    np.testing.assert_allclose(results['fused'][0], results['generic'][0], rtol=LOSS_RTOL)
    for i, (p, w) in enumerate(zip(results['fused'][1], results['generic'][1])):
        ok, err, arb = close_or_arbitrated(p, w, lambda i=i: fp64()[0].export_params()[i], PARAM_RTOL, atol=3e-7, adam_move=LR * NITERS)
        assert ok, ('fused vs generic', i, err, arb)
    if results['fused'][2] is not None:
        assert abs(results['fused'][2] - results['generic'][2]) < VAR_ATOL


# ---- 1. path -----------------------------------------------------------------------------------------------------------------------
def _path_case(pa, extra, monkeypatch):
    eq, kw, terms = _problem('constraint', pa.D, pa.V)
    pts = np.random.RandomState(3).rand(8, 24, 2).astype(np.float32)
    solver = pa.Solver(eq, **kw, **extra)
    fit = lambda crit, k: solver.fit(niters=1, batch_size=24, sampler=FixedBatches(pts[k:k + 1]), lr=LR, loss_terms=terms, criterion=crit)
    assert solver.criterion_path == 'generic'
    for k, name in enumerate(CRITERIA):
        fit(CRITERIA[name](), k)
        assert solver.last_fit_path == 'generic', name           # opt-in: without the call nothing changes
        assert solver.last_fit_criterion == f'{type(CRITERIA[name]()).__name__}/generic'
    solver.set_criterion_path('fused')
    for k, name in enumerate(CRITERIA):
        fit(CRITERIA[name](), k)
        assert solver.last_fit_path == 'fused', name
        assert solver.last_fit_criterion == f'{type(CRITERIA[name]()).__name__}/fused'
    fit(nn.MSELoss(), 0)
    assert solver.last_fit_criterion == 'MSELoss/fused'

    class MyL1(nn.L1Loss):                                        # a subclass may override forward(): by exact type only
        def forward(self, value, target):
            return 2.0 * super().forward(value, target)
    for crit in (MyL1(), lambda value, target: (value - target).abs().mean(), nn.SmoothL1Loss(beta=0.3, reduction='none'), nn.SoftMarginLoss()):
        if getattr(crit, 'reduction', None) == 'none':
            assert solver._lower_criterion(crit) is None          # (the reference cannot call backward() on it either)
            continue
        fit(crit, 4)
        assert solver.last_fit_path == 'generic', crit
    solver.set_criterion_path('generic')
    fit(nn.L1Loss(), 5)
    assert solver.last_fit_path == 'generic'
    fit(nn.MSELoss(), 6)
    assert solver.last_fit_path == 'fused'
    with pytest.raises(ValueError):
        solver.set_criterion_path('quick')
    monkeypatch.setenv('PYDENS_AMD_CRITERION', 'fused')
    assert pa.Solver(eq, **kw, **extra).criterion_path == 'fused'


def test_closed_form_criteria_take_the_fused_path_when_asked_to(pa, emu_lib, monkeypatch):
    _path_case(pa, emu_kwargs(emu_lib), monkeypatch)


@pytest.mark.gpu
def test_closed_form_criteria_take_the_fused_path_on_the_gpu(pa, monkeypatch):
    _path_case(pa, {}, monkeypatch)


# ---- 2. / 3. parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('crit_name', list(CRITERIA))
@pytest.mark.parametrize('which', PROBLEMS)
def test_fused_criteria_follow_the_oracle_and_the_generic_path(pa, emu_lib, which, crit_name):
    _parity_case(pa, emu_kwargs(emu_lib), which, crit_name, 40)


@pytest.mark.gpu
@pytest.mark.parametrize('crit_name', list(CRITERIA))
@pytest.mark.parametrize('which', PROBLEMS)
def test_fused_criteria_follow_the_oracle_and_the_generic_path_on_the_gpu(pa, which, crit_name):
    _parity_case(pa, {}, which, crit_name, 523)


def _specialised_shape_case(pa, extra, lib, n):
    """ BASELINE config 2's shape (4 x 64 Tanh net, Poisson box): MSE keeps its shape-specialised kernel, L1 takes the general kernel of the
    same stream shape (the specialised affine instantiations are compiled for MSE alone) and follows the oracle """
    from oracle import pinn_oracle as po
    import pinn_configs as pc
    torch.manual_seed(2)
    ocfg = pc.make_config('cfg2', po.D, torch)
    oracle = po.OracleSolver(ocfg['equation'], **ocfg['solver_kwargs'])
    cfg, solver = make_solver('cfg2', pa, **extra)
    start = oracle.export_params()
    load_params(solver, start)
    solver.set_criterion_path('fused')
    pts = pc.sample_points(cfg, n, seed=5, steps=3)
    solver.fit(niters=1, batch_size=n, sampler=FixedBatches(pts[:1]), lr=LR)
    assert solver.last_fit_path == 'fused' and lib.pinn_debug_last_kernel() == 2
    name_mse = lib.pinn_last_kernel_name().decode()
    load_params(solver, start)
    rec = Recording(nn.L1Loss())
    oracle64 = po.OracleSolver(ocfg['equation'], dtype=torch.float64, **ocfg['solver_kwargs'])
    oracle64.import_params(start)
    oracle64.fit(niters=2, batch_size=n, points=pts[1:], lr=LR, criterion=rec)
    assert l1_condition(rec.seen) > 1e-4, l1_condition(rec.seen)
    oracle.fit(niters=2, batch_size=n, points=pts[1:], lr=LR, criterion=nn.L1Loss())
    solver.fit(niters=2, batch_size=n, sampler=FixedBatches(pts[1:]), lr=LR, criterion=nn.L1Loss())
    assert solver.last_fit_path == 'fused' and lib.pinn_debug_last_kernel() == 0
    assert lib.pinn_last_kernel_name().decode() != name_mse
    np.testing.assert_allclose([float(v) for v in solver.losses][1:], [float(v) for v in oracle.losses], rtol=LOSS_RTOL)
    for i, (got, want) in enumerate(zip(export_params(solver), oracle.export_params())):
        ok, err, arb = close_or_arbitrated(got, want, lambda i=i: oracle64.export_params()[i], PARAM_RTOL, atol=3e-7, adam_move=LR * 2)
        assert ok, (i, err, arb)
    # back to MSE: the specialised kernel again
    solver.fit(niters=1, batch_size=n, sampler=FixedBatches(pts[:1]), lr=LR)
    assert lib.pinn_debug_last_kernel() == 2 and lib.pinn_last_kernel_name().decode() == name_mse


def test_non_mse_criterion_leaves_the_shape_specialised_kernel_to_mse(pa, emu_lib):
    _specialised_shape_case(pa, emu_kwargs(emu_lib), emu_lib, 48)


@pytest.mark.gpu
def test_non_mse_criterion_leaves_the_shape_specialised_kernel_to_mse_on_the_gpu(pa):
    _specialised_shape_case(pa, {}, pa.engine.load_library(), 523)


# ---- 4. C-ABI ------------------------------------------------------------------------------------------------------------------------
def _abi_net(engine, lib, device):
    net = engine.Net([2, 16, 16, 1], 'tanh', ndims=2, has_bc=True, bc_value=1.0, lib=lib)
    lay = net.layout
    flat = torch.zeros(lay.p_total, dtype=torch.float32)
    rng = np.random.RandomState(7)
    for w, b in net.param_views(flat):
        w.copy_(torch.as_tensor(rng.randn(*w.shape).astype(np.float32) * 0.5))
        b.copy_(torch.as_tensor(rng.randn(*b.shape).astype(np.float32) * 0.5))
    n = 64
    xs = torch.as_tensor(rng.rand(n, 2).astype(np.float32))
    flat, xs = flat.to(device), xs.to(device)
    ws = torch.zeros((net.workspace_bytes(n, 2, 2) + 3) // 4, dtype=torch.float32, device=device)
    # r = u_xx + u_yy - 0.7 (streams u, u_x, u_y, u_xx, u_yy)
    make = lambda: engine.Residual.build(engine.RES_AFFINE, 0, None, coef=[0.0, 0.0, 0.0, 1.0, 1.0], src_const=-0.7)
    return net, flat, xs, ws, make


def _abi_step(net, res, flat, xs, ws, inv_n=None):
    grads = torch.zeros_like(flat)
    net.residual_step(res, flat, xs, grads, ws, dir_cols=(0, 1), n2=2, inv_n_global=inv_n)
    return grads.cpu().numpy().copy()


def _abi_case(engine, lib, device):
    net, flat, xs, ws, make = _abi_net(engine, lib, device)
    lay, n = net.layout, xs.shape[0]
    zero = make()                                                 # criterion fields untouched: zero-initialised
    assert (zero.criterion, zero.crit_param, zero.crit_sum) == (0, 0.0, 0)
    g_zero = _abi_step(net, zero, flat, xs, ws)
    # MSELoss(reduction='mean') through the generic entry points: forward streams, d(mean r^2)/d(streams) = 2 r C_s / N, backward
    streams = net.jet_forward(flat, xs, (0, 1), 2)
    r = streams[3] + streams[4] - 0.7
    gin = torch.zeros_like(streams)
    gin[3] = gin[4] = 2.0 * r / n
    g_ref = torch.zeros_like(flat)
    net.jet_backward(flat, xs, gin.contiguous(), g_ref, ws, (0, 1), 2)
    g_ref = g_ref.cpu().numpy()
    assert rel_l2(g_zero[:lay.off_loss], g_ref[:lay.off_loss]) < 1e-5
    assert abs(g_zero[lay.off_loss] / float((r * r).mean()) - 1) < 1e-5
    # explicit MSE code, a stray parameter: the same bits
    assert np.array_equal(_abi_step(net, make().set_criterion(engine.CRIT_MSE, 123.0), flat, xs, ws), g_zero)
    # pinn_residual_step takes its scale from the caller: N * (1 / N) = 1 is a power of two here, so the sum is the mean times N, bit for bit
    assert np.array_equal(_abi_step(net, make().set_criterion(engine.CRIT_MSE, 0.0, True), flat, xs, ws, inv_n=1.0), g_zero * n)
    # the other criteria against torch's own backward of the module on the streams
    for crit, code, par in ((nn.L1Loss(), engine.CRIT_L1, 0.0), (nn.SmoothL1Loss(beta=0.3), engine.CRIT_SMOOTH_L1, 0.3),
                            (nn.HuberLoss(delta=0.5), engine.CRIT_HUBER, 0.5), (nn.SmoothL1Loss(beta=0.0), engine.CRIT_SMOOTH_L1, 0.0)):
        leaf = streams.detach().clone().requires_grad_()
        value = crit(leaf[3] + leaf[4] - 0.7, torch.zeros_like(leaf[3]))
        value.backward()
        want = torch.zeros_like(flat)
        net.jet_backward(flat, xs, leaf.grad.contiguous(), want, ws, (0, 1), 2)
        got = _abi_step(net, make().set_criterion(code, par), flat, xs, ws)
        assert rel_l2(got[:lay.off_loss], want.cpu().numpy()[:lay.off_loss]) < 1e-5, crit
        assert abs(got[lay.off_loss] / float(value.detach()) - 1) < 1e-5, crit
    # refusals: unknown code, Huber without a positive delta
    for code, par in ((4, 0.0), (-1, 0.0), (engine.CRIT_HUBER, 0.0), (engine.CRIT_HUBER, -1.0), (engine.CRIT_SMOOTH_L1, -0.5)):
        bad = make().set_criterion(code, par)
        grads = torch.zeros_like(flat)
        dirs, nd = net._dirs((0, 1))
        rc = lib.pinn_residual_step(net.handle, ctypes.byref(bad), ctypes.c_void_p(flat.data_ptr()), ctypes.c_void_p(xs.data_ptr()), n, dirs, nd, 2,
                                    None, 0.0, 1.0 / n, ctypes.c_void_p(grads.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 4,
                                    engine.stream_of(xs))
        assert rc != 0 and lib.pinn_last_error(), (code, par)
        assert b'criterion' in lib.pinn_last_error() or b'Loss' in lib.pinn_last_error()
        assert not grads.any()


def test_criterion_fields_of_the_residual_struct(emu_lib):
    from pydens_amd import engine
    _abi_case(engine, emu_lib, 'cpu')


@pytest.mark.gpu
def test_criterion_fields_of_the_residual_struct_on_the_gpu():
    from pydens_amd import engine
    _abi_case(engine, engine.load_library(), 'cuda')


# ---- 4. / 5. one-launch forms: L1 after MSE on one net, chunks against the eager loop ----------------------------------------------------
def _l1_after_mse_case(pa, extra, lib, monkeypatch, name, batch, niters, persist, exact):
    """ Solver.fit(MSE) then Solver.fit(L1) on ONE net, every chunk through pinn_fit_steps with a control block, against the per-iteration loop on the same
    Philox batches: a launch graph (or one-CU chunk) recorded for MSE must not be replayed for L1. Rule of the existing chunk tests: launch
    graphs bit for bit (test_gpu_parity.test_fit_chunks_as_launch_graphs_follow_the_eager_loop_bit_for_bit), the one-launch kernel to fp32
    round-off (test_emu_engine._one_launch_case). """
    def run(chunks):
        monkeypatch.setenv('PYDENS_AMD_FIT_GRAPH', '1' if chunks else '0')
        monkeypatch.setenv('PYDENS_AMD_FIT_PERSIST', str(persist if chunks else 0))
        torch.manual_seed(21)
        cfg, solver = make_solver(name, pa, **extra)
        solver.set_criterion_path('fused')
        if not chunks:
            solver._device_columns = lambda sampler: None          # the per-iteration loop (pinn_residual_optim_step)
        st0 = (ctypes.c_int32 * 4)()
        lib.pinn_debug_fit_graph_stats(st0)
        solver.fit(niters=niters, batch_size=batch, lr=0.005)
        solver.fit(niters=niters, batch_size=batch, lr=0.005, optimizer=None, criterion=nn.L1Loss())
        assert solver.last_fit_path == 'fused' and solver.last_fit_criterion == 'L1Loss/fused'
        kernel = lib.pinn_last_kernel_name().decode()
        solver.fit(niters=niters, batch_size=batch, lr=0.005, optimizer=None)
        st = (ctypes.c_int32 * 4)()
        lib.pinn_debug_fit_graph_stats(st)
        return (np.array([float(v) for v in solver.losses]), solver.model.flat.detach().cpu().numpy().copy(),
                solver.optimizer.exp_avg.cpu().numpy().copy(), [st[i] - st0[i] for i in range(4)], kernel)
    l0, p0, m0, _, _ = run(False)
    l1, p1, m1, stats, kernel = run(True)
    assert np.isfinite(l1).all()
    if exact:
        assert np.array_equal(l0, l1) and np.array_equal(p0, p1) and np.array_equal(m0, m1)
    else:
        np.testing.assert_allclose(l1[:8], l0[:8], rtol=2e-6)
        np.testing.assert_allclose(l1, l0, rtol=2e-4)
        assert params_close(p1, p0, 2e-4) and params_close(m1, m0, 2e-3, atol=1e-7)
    return stats, kernel


def test_l1_after_mse_through_the_chunk_entry_point_eager_fallback(pa, emu_lib, monkeypatch):
    """ the emulator refuses capture: pinn_fit_steps with a control block runs its eager loop, which must honour the criterion """
    monkeypatch.setattr(pa.Solver, 'FIT_CTRL_ON_HOST', True)
    _l1_after_mse_case(pa, emu_kwargs(emu_lib), emu_lib, monkeypatch, 'cfg4', 40, 5, 0, True)


# sampler seeds of the one-CU cases per trajectory length (iterations per fit call): scanned on the CPU from 0 upwards, first seed whose fp64
# oracle trajectory keeps min |r| > 3e-4 max |r| on every L1 batch (the case asserts the 1e-4 of the L1 condition again)
ONE_CU_SEEDS = {5: 0, 8: 2}


def _one_cu_batches(pa, sampler_seed, count, batch=100):
    """ the Philox batches a fresh seeded sampler hands the device sampler, restated on the host (oracle/philox.py: bit-exact) """
    from oracle import philox
    sampler = pa.NumpySampler('uniform', dim=2, seed=sampler_seed)
    key = sampler.device_key()
    assert key is not None and sampler.columns() == [(0, 0.0, 1.0)] * 2
    return sampler, [philox.sample_points(batch, [(philox.UNIFORM, 0.0, 1.0)] * 2, key, call) for call in range(count)]


def _one_cu_oracle(niters, sampler_seed, pa):
    """ fp64 oracle on the same start and batches: MSE stretch, then the L1 stretch with its residuals noted """
    import pinn_configs as pc
    from oracle import pinn_oracle as po
    torch.manual_seed(21)
    ocfg = pc.make_config('cfg1', po.D, torch)
    start = [np.asarray(p, dtype=np.float32) for p in po.OracleSolver(ocfg['equation'], **ocfg['solver_kwargs']).export_params()]
    oracle = po.OracleSolver(ocfg['equation'], dtype=torch.float64, **ocfg['solver_kwargs'])
    oracle.import_params(start)
    pts = np.stack(_one_cu_batches(pa, sampler_seed, 2 * niters)[1])
    rec = Recording(nn.L1Loss())
    oracle.fit(niters=niters, batch_size=100, points=pts[:niters], lr=0.005)
    oracle.fit(niters=niters, batch_size=100, points=pts[niters:], lr=0.005, optimizer=None, criterion=rec)
    return start, np.array([float(v) for v in oracle.losses]), l1_condition(rec.seen)


def _one_cu_l1_case(pa, extra, lib, monkeypatch, niters):
    """ batch 100 on the narrow net of BASELINE config 1: fit(MSE), fit(L1), fit(MSE) on one net with every chunk as ONE launch on one CU
    (pinn_fit_kernel.h inherits the point stage through pinn_tile_body) against the per-iteration loop, under the rule of
    test_emu_engine._one_launch_case: first eight losses within 2e-6, all within 2e-4, parameters 2e-4, first moments 2e-3.
    The two sides are two fp32 implementations of the tile pass (another kernel, another FMA contraction), so the L1 condition of this file
    applies: a residual at round-off level may take another sign on either side, and from then on Adam walks two trajectories. The batches
    come from a SEEDED sampler, are restated on the host and the fp64 oracle's L1 residuals on them must keep min |r| > 1e-4 max |r|, every
    point counted. That bounds the length: a trajectory of K L1 iterations has 100 K residuals, each below 1e-4 of the largest with a
    probability of about 1e-4 -- a handful of iterations can meet the condition, the 300 of the MSE chunk test cannot (one such point in 30 000
    is all but certain). The one-CU form takes chunks of any length up to 128, so a short fit runs the same kernel. """
    start, want, ratio = _one_cu_oracle(niters, ONE_CU_SEEDS[niters], pa)
    print(f'one-CU L1 case, {niters} iterations per fit: fp64 oracle min|r| / max|r| over the L1 stretch = {ratio:.3e}')
    assert ratio > 1e-4, ratio

    def run(chunks):
        monkeypatch.setenv('PYDENS_AMD_FIT_GRAPH', '1' if chunks else '0')
        monkeypatch.setenv('PYDENS_AMD_FIT_PERSIST', '2' if chunks else '0')
        monkeypatch.setenv('PYDENS_AMD_FIT_ROUNDS', '4')
        torch.manual_seed(21)
        cfg, solver = make_solver('cfg1', pa, **extra)
        load_params(solver, start)
        solver.set_criterion_path('fused')
        sampler, _ = _one_cu_batches(pa, ONE_CU_SEEDS[niters], 0)
        if not chunks:
            solver._device_columns = lambda sampler: None          # the per-iteration loop (pinn_residual_optim_step)
        st0 = (ctypes.c_int32 * 4)()
        lib.pinn_debug_fit_graph_stats(st0)
        solver.fit(niters=niters, batch_size=100, sampler=sampler, lr=0.005)
        solver.fit(niters=niters, batch_size=100, sampler=sampler, lr=0.005, optimizer=None, criterion=nn.L1Loss())
        assert solver.last_fit_path == 'fused' and solver.last_fit_criterion == 'L1Loss/fused'
        kernel = lib.pinn_last_kernel_name().decode()
        solver.fit(niters=niters, batch_size=100, sampler=sampler, lr=0.005, optimizer=None)
        st = (ctypes.c_int32 * 4)()
        lib.pinn_debug_fit_graph_stats(st)
        return (np.array([float(v) for v in solver.losses]), solver.model.flat.detach().cpu().numpy().copy(),
                solver.optimizer.exp_avg.cpu().numpy().copy(), st[0] - st0[0], kernel)
    l0, p0, m0, _, k0 = run(False)
    l1, p1, m1, launched, k1 = run(True)
    rel = np.abs(l1 / l0 - 1)
    print(f'one-CU chunk against the eager loop: loss rel err first 8 {rel[:8].max():.2e}, all {rel.max():.2e}; eager against the fp64 oracle '
          f'{np.abs(l0[:2 * niters] / want - 1).max():.2e}')
    assert k0.startswith('pinn_tile_kernel<') and k1.startswith('pinn_fit_kernel<'), (k0, k1)
    assert launched >= 3                                           # every fit call went out as one-launch chunks
    # the restated batches are the ones the device drew: both stretches follow the fp64 oracle on them (the suite's 5e-5 of a few Adam steps)
    np.testing.assert_allclose(l0[:2 * niters], want, rtol=5e-5)
    assert np.isfinite(l1).all()
    np.testing.assert_allclose(l1[:8], l0[:8], rtol=2e-6)
    np.testing.assert_allclose(l1, l0, rtol=2e-4)
    assert params_close(p1, p0, 2e-4) and params_close(m1, m0, 2e-3, atol=1e-7)


def test_l1_fit_chunk_on_one_cu_follows_the_eager_loop(pa, emu_lib, monkeypatch):
    monkeypatch.setattr(pa.Solver, 'FIT_CTRL_ON_HOST', True)
    _one_cu_l1_case(pa, emu_kwargs(emu_lib), emu_lib, monkeypatch, 5)


@pytest.mark.gpu
def test_l1_fit_chunk_on_one_cu_follows_the_eager_loop_on_the_gpu(pa, monkeypatch):
    _one_cu_l1_case(pa, {}, pa.engine.load_library(), monkeypatch, 8)


@pytest.mark.gpu
def test_l1_after_mse_replays_its_own_launch_graph_on_the_gpu(pa, monkeypatch):
    """ batch 2 048 on the 4 x 64 net: 128-iteration chunks as launch graphs. 300 iterations per fit = eager chunk + capture, one replay, an
    eager tail; the L1 fit behind the MSE fit must capture a graph of its own (the criterion is part of the cache key) and replay THAT """
    lib = pa.engine.load_library()
    stats, kernel = _l1_after_mse_case(pa, {}, lib, monkeypatch, 'cfg2', 2048, 300, 0, True)
    assert stats[1] >= 3 and stats[0] >= 3, stats          # three captures (MSE, L1, MSE again), a replay behind each
    assert kernel.startswith('pinn_tile_kernel<'), kernel


# ---- 6. data parallel ----------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _dp_problem(pa, lib, reduction):
    torch.manual_seed(21)
    eq, kw, terms = _problem('constraint', pa.D, pa.V)
    solver = pa.Solver(eq, **kw, _lib=lib, device='cpu')
    solver.set_criterion_path('fused')
    rng = np.random.RandomState(3)
    start = [np.asarray(rng.randn(*p.shape) * 0.5, dtype=np.float32) for p in export_params(solver)]
    return solver, rng.rand(3, 33, 2).astype(np.float32), dict(lr=0.01, loss_terms=terms, criterion=nn.L1Loss(reduction=reduction)), start


def _dp_worker(rank, world, port, out_dir, reduction):
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
    solver, points, fit_kw, start = _dp_problem(pa, lib, reduction)
    if rank == 0:
        load_params(solver, start)
    shard = points[:, rank::world]
    solver.fit(niters=points.shape[0], batch_size=points.shape[1], sampler=FixedBatches(shard), **fit_kw)
    assert solver.last_fit_path == 'fused'
    np.savez(os.path.join(out_dir, f'rank{rank}.npz'), losses=np.array([float(v) for v in solver.losses]),
             nu=float(solver.model.nu.detach()), **{f'p{i}': p for i, p in enumerate(export_params(solver))})
    dist.destroy_process_group()


@pytest.mark.parametrize('reduction', ['mean', 'sum'])
def test_two_ranks_follow_the_single_process_with_l1(pa, emu_lib, reduction):
    """ gloo, world 2, uneven shares (33 points), equation + constraint term: as tests/test_data_parallel.py, same bounds """
    from oracle import pinn_oracle as po
    single, points, fit_kw, start = _dp_problem(pa, emu_lib, reduction)
    load_params(single, start)
    single.fit(niters=points.shape[0], batch_size=points.shape[1], sampler=FixedBatches(points), **fit_kw)
    assert single.last_fit_path == 'fused'
    want_losses, want = np.array([float(v) for v in single.losses]), export_params(single)
    # (the single process itself against the oracle: the loss of the first iteration, before any update)
    eq, kw, terms = _problem('constraint', po.D, po.V)
    oracle = po.OracleSolver(eq, **kw)
    oracle.import_params(start)
    oracle.fit(niters=1, batch_size=points.shape[1], points=points, lr=0.01, loss_terms=terms, criterion=nn.L1Loss(reduction=reduction))
    np.testing.assert_allclose(want_losses[0], float(oracle.losses[0]), rtol=LOSS_RTOL)
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_dp_worker, args=(2, _free_port(), tmp, reduction), nprocs=2, join=True)
        for rank in range(2):
            z = np.load(os.path.join(tmp, f'rank{rank}.npz'))
            np.testing.assert_allclose(z['losses'], want_losses, rtol=1e-5)
            assert abs(float(z['nu']) - float(single.model.nu.detach())) < 1e-5
            for i, w in enumerate(want):
                assert rel_l2(z[f'p{i}'], w) < 1e-5, (rank, i)
