""" L-BFGS in `Solver.fit`: closure steps of torch.optim.LBFGS on the default optimizer path, `FlatLBFGS` with the direction kernels
(include/pinn.h pinn_lbfgs_direction) under `set_optimizer_path('fused')`. CPU tier on the emulator build of the product sources, `-m gpu`
twins on the device.

Reference of every end-to-end case: `oracle.OracleSolver` stepped by torch.optim.LBFGS over its trainable parameters, in fp32, and in fp64 as
arbiter. Bounds are the suite's own through `close_or_arbitrated`: parameters 3e-5, losses 1e-5, k = 2 where the fp32 reference is the noisy
side; no entries set aside (L-BFGS has no g / sqrt(g^2) amplification).

What can be compared: without a line search L-BFGS is chaotic in fp32 -- the reference's own fp32 run sits O(1) from its fp64 run after three
iterations -- so the fixed-step form is compared over ONE iteration with max_iter = 2 (the fp32 reference is checked against fp64 at the same
bound first). With 'strong_wolfe', history_size 4, max_iter 5, three iterations the fp32 reference stays within 1.1e-4 of fp64 on the losses
and 1.6e-5 on the parameters: that is the end-to-end case.

Direction kernels: against an fp64 two-loop recursion in numpy over the very pairs the ring holds; the bound is the error of torch's own fp32
recursion on the same pairs, with the 1e-6 relative L2 of test_adam_matches_torch as floor. """
import ctypes
import inspect
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import pinn_configs as pc
from conftest import Golden, rel_l2
from helpers import FixedBatches, close_or_arbitrated, export_params, load_params, make_solver, record_margin

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'emu'))

LOSS_RTOL, PARAM_RTOL = 1e-5, 3e-5
WOLFE = dict(lr=1, max_iter=5, history_size=4, line_search_fn='strong_wolfe')
FIXED = dict(lr=1, max_iter=2, history_size=4)
BATCH, NITERS = 64, 3


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


# ---- the reference: the oracle stepped by torch.optim.LBFGS, computed once per (fixture, setting, precision) ---------------------------------
_ORACLE = {}


def _points(name, niters=NITERS):
    d = Golden(name).points.shape[-1]
    return np.random.RandomState(77).rand(niters, BATCH, d).astype(np.float32)


def _oracle_run(name, setting, dtype, niters=NITERS):
    from oracle import pinn_oracle as po
    key = (name, tuple(sorted(setting.items(), key=str)), dtype, niters)
    if key not in _ORACLE:
        cfg = pc.make_config(name, po.D, torch)
        oracle = po.OracleSolver(cfg['equation'], dtype=dtype, **cfg['solver_kwargs'])
        oracle.import_params(Golden(name).params)
        opt = torch.optim.LBFGS([p for p in oracle.model.parameters() if p.requires_grad], **setting)
        losses, evals = [], []
        for pts in _points(name, niters):
            calls = [0]

            def closure():
                calls[0] += 1
                return torch.tensor(oracle.evaluate(pts)['loss'], dtype=dtype)
            losses.append(float(opt.step(closure)))
            evals.append(calls[0])
        _ORACLE[key] = dict(losses=np.array(losses), evals=evals, params=oracle.export_params())
    return _ORACLE[key]


def _against_oracle(solver, name, setting, case, niters=NITERS, evals=None):
    want, want64 = _oracle_run(name, setting, torch.float32, niters), _oracle_run(name, setting, torch.float64, niters)
    got = np.array([float(v) for v in solver.losses])[-niters:]
    for i in range(niters):
        ok, err, arb = close_or_arbitrated(got[i], want['losses'][i], lambda i=i: want64['losses'][i], LOSS_RTOL, atol=0.0)
        print(f'{case}: loss {i} rel err {err:.2e}{" (fp64 arbiter)" if arb else ""}')
        record_margin('test_lbfgs', case, f'loss{i}', err, LOSS_RTOL, arb)
        assert ok, (case, i, got[i], want['losses'][i], want64['losses'][i])
    for i, (p, w) in enumerate(zip(export_params(solver), want['params'])):
        ok, err, arb = close_or_arbitrated(p, w, lambda i=i: want64['params'][i], PARAM_RTOL, atol=3e-7, adam_move=None)
        print(f'{case}: tensor {i} rel err {err:.2e}{" (fp64 arbiter)" if arb else ""}')
        record_margin('test_lbfgs', case, f'param{i}', err, PARAM_RTOL, arb)
        assert ok, (case, i, err, arb)
    if evals is not None and want['evals'] == want64['evals']:          # (asserted only where the two references agree on it)
        assert evals == want['evals'], (case, evals, want['evals'])


def _fit_lbfgs(pa, extra, name, setting, path, use_fused=True, niters=NITERS):
    cfg, solver = make_solver(name, pa, **extra)
    load_params(solver, Golden(name).params)
    solver.use_fused = use_fused
    solver.set_optimizer_path(path)
    evals = []
    for pts in _points(name, niters):           # one fit call per iteration: the number of closure evaluations of each is on the optimizer
        solver.fit(niters=1, batch_size=BATCH, sampler=FixedBatches(pts[None]), optimizer='LBFGS' if not evals else None, **setting)
        evals.append(solver.optimizer.closure_calls)
    assert solver.last_fit_path == ('fused' if use_fused else 'generic'), solver.program_error
    assert solver.last_fit_optimizer == f'LBFGS/{path}'
    return solver, evals


def _wolfe_case(pa, extra, name, path, use_fused):
    solver, evals = _fit_lbfgs(pa, extra, name, WOLFE, path, use_fused)
    _against_oracle(solver, name, WOLFE, f'{name}/wolfe/{path}/{"fused" if use_fused else "generic"}', evals=evals)


def _fixed_case(pa, extra, name, path):
    """ one iteration of the fixed-step form; the fp32 reference itself must hold the bound against fp64 there """
    r32, r64 = _oracle_run(name, FIXED, torch.float32, 1), _oracle_run(name, FIXED, torch.float64, 1)
    for a, b in zip(r32['params'], r64['params']):
        assert rel_l2(a, b) <= PARAM_RTOL or np.linalg.norm(np.asarray(a, np.float64) - b) <= 3e-7 * np.sqrt(a.size)
    solver, evals = _fit_lbfgs(pa, extra, name, FIXED, path, niters=1)
    _against_oracle(solver, name, FIXED, f'{name}/fixed/{path}', niters=1, evals=evals)


STEP_PATHS = [True, False]


# ---- 1. the default ('torch') optimizer path: fails with TypeError before closure steps existed ----------------------------------------------
@pytest.mark.parametrize('use_fused', STEP_PATHS, ids=['fused_step', 'generic_step'])
@pytest.mark.parametrize('name', ['cfg1', 'cfg2'])
def test_lbfgs_by_name_follows_the_oracle(pa, emu_lib, name, use_fused):
    _wolfe_case(pa, emu_kwargs(emu_lib), name, 'torch', use_fused)


@pytest.mark.gpu
@pytest.mark.parametrize('use_fused', STEP_PATHS, ids=['fused_step', 'generic_step'])
@pytest.mark.parametrize('name', ['cfg1', 'cfg2'])
def test_lbfgs_by_name_follows_the_oracle_on_the_gpu(pa, name, use_fused):
    _wolfe_case(pa, {}, name, 'torch', use_fused)


@pytest.mark.parametrize('path', ['torch', 'fused'])
def test_fixed_step_lbfgs_follows_the_oracle_for_one_iteration(pa, emu_lib, path):
    _fixed_case(pa, emu_kwargs(emu_lib), 'cfg1', path)


@pytest.mark.gpu
@pytest.mark.parametrize('path', ['torch', 'fused'])
def test_fixed_step_lbfgs_follows_the_oracle_for_one_iteration_on_the_gpu(pa, path):
    _fixed_case(pa, {}, 'cfg1', path)


def _adam_then_lbfgs_case(pa, extra, path):
    """ "Adam to get close, L-BFGS to converge" on one solver, against the same calls on the oracle """
    from oracle import pinn_oracle as po
    g = Golden('cfg1')
    cfg = pc.make_config('cfg1', po.D, torch)
    oracle = po.OracleSolver(cfg['equation'], **cfg['solver_kwargs'])
    oracle.import_params(g.params)
    pts = _points('cfg1', 4)
    oracle.fit(niters=2, batch_size=BATCH, points=pts[:2], lr=0.005)
    opt = torch.optim.LBFGS([p for p in oracle.model.parameters() if p.requires_grad], **WOLFE)
    want = [float(opt.step(lambda p=p: torch.tensor(oracle.evaluate(p)['loss']))) for p in pts[2:]]
    _, solver = make_solver('cfg1', pa, **extra)
    load_params(solver, g.params)
    solver.set_optimizer_path(path)
    solver.fit(niters=2, batch_size=BATCH, sampler=FixedBatches(pts[:2]), lr=0.005)
    assert solver.last_fit_optimizer == 'Adam/fused'
    solver.fit(niters=2, batch_size=BATCH, sampler=FixedBatches(pts[2:]), optimizer='LBFGS', **WOLFE)
    assert solver.last_fit_optimizer == f'LBFGS/{path}' and len(solver.losses) == 4
    np.testing.assert_allclose([float(v) for v in solver.losses[2:]], want, rtol=5e-5)       # (behind two Adam steps: the 5e-5 of the fit sequences)
    for p, w in zip(export_params(solver), oracle.export_params()):
        assert rel_l2(p, w) < 5e-5 or np.abs(p - w).max() < 3e-7


@pytest.mark.parametrize('path', ['torch', 'fused'])
def test_adam_then_lbfgs_on_one_solver(pa, emu_lib, path):
    _adam_then_lbfgs_case(pa, emu_kwargs(emu_lib), path)


@pytest.mark.gpu
@pytest.mark.parametrize('path', ['torch', 'fused'])
def test_adam_then_lbfgs_on_one_solver_on_the_gpu(pa, path):
    _adam_then_lbfgs_case(pa, {}, path)


# ---- 2. the direction kernels against an fp64 two-loop recursion ---------------------------------------------------------------------------------
def _two_loop(g, S, Y, H, dtype):
    """ torch.optim.LBFGS's recursion (lbfgs.py) over the pairs oldest first, in `dtype` torch ops """
    g, S, Y = torch.as_tensor(g, dtype=dtype), [torch.as_tensor(s, dtype=dtype) for s in S], [torch.as_tensor(y, dtype=dtype) for y in Y]
    ro = [1.0 / y.dot(s) for s, y in zip(S, Y)]
    al = [None] * len(S)
    q = g.neg()
    for i in range(len(S) - 1, -1, -1):
        al[i] = S[i].dot(q) * ro[i]
        q.add_(Y[i], alpha=-al[i])
    r = torch.mul(q, torch.as_tensor(H, dtype=dtype))
    for i in range(len(S)):
        be = Y[i].dot(r) * ro[i]
        r.add_(S[i], alpha=al[i] - be)
    return r.double().numpy()


class Direction:
    """ pinn_lbfgs_direction on its own buffers """
    def __init__(self, pa, lib, device, p, m, seed=0):
        engine = pa.engine
        self.engine, self.p, self.m, self.device = engine, p, m, device
        self.net = engine.Net([2, 16, 1], 'tanh', 2, lib=lib)
        rng = np.random.RandomState(seed)
        self.rng = rng
        ld = (p + 3) // 4 * 4
        dev = lambda a: torch.as_tensor(a).to(device)
        self.params = dev(rng.randn(p).astype(np.float32))
        self.mask = torch.ones(p, dtype=torch.uint8, device=device)
        self.mask[::7] = 0
        self.live = self.mask.bool().cpu().numpy()
        # state as a fresh FlatLBFGS has it, except d and prev_grad at masked entries: a bit pattern that must survive
        self.d = dev(np.where(self.live, 0.0, 7.25).astype(np.float32))
        self.prev = dev(np.where(self.live, 0.0, -3.5).astype(np.float32))
        # (the rings need no initialisation: NaN everywhere must never reach a product, and stays where no entry takes part)
        self.S, self.Y = torch.full((m, ld), float('nan'), device=device), torch.full((m, ld), float('nan'), device=device)
        self.ctrl = torch.zeros(self.net.lbfgs_ctrl_doubles(m), dtype=torch.float64, device=device)
        self.rows = torch.zeros(self.net.lbfgs_workspace_bytes(p, m) // 8, dtype=torch.float64, device=device)
        self.t, self.lr = 0.0, 0.7
        self.off_loss = 0               # (entry 0 is masked: it plays the loss slot)

    def call(self, g, mode, apply=True, tol_grad=1e-7, tol_change=1e-9):
        self.g = torch.as_tensor(g).to(self.device)
        self.net.lbfgs_direction(self.params, self.g, self.prev, self.d, self.S, self.Y, self.mask, self.m, mode, apply, self.t, self.lr,
                                 tol_grad, tol_change, self.ctrl, self.rows, off_loss=self.off_loss)
        head = dict(zip(self.engine.LBFGS_CTRL, self.ctrl[:16].tolist()))
        if head['stop'] == 0.0 or head['stop'] == 4.0:
            self.t = head['t']
        return head

    def pairs(self, head):
        """ the ring's pairs oldest first, live entries only, as stored """
        n, first = int(head['count']), int(head['head'])
        S, Y = self.S.cpu().numpy()[:, :self.p], self.Y.cpu().numpy()[:, :self.p]
        order = [(first + c) % self.m for c in range(n)]
        return [S[j] for j in order], [Y[j] for j in order], order

    def gram(self):
        m = self.m
        rest = self.ctrl[16 + 2 * m:].cpu().numpy()
        return rest[:m * m].reshape(m, m), rest[m * m:].reshape(m, m)


def _direction_case(pa, lib, device, p, m, updates, check_every=1):
    D = Direction(pa, lib, device, p, m)
    live, rng = D.live, D.rng
    keep = dict(params=D.params.cpu().numpy().copy(), d=D.d.cpu().numpy().copy(), prev=D.prev.cpu().numpy().copy())
    g = rng.randn(p).astype(np.float32)
    p0 = D.params.cpu().numpy().copy()
    head = D.call(g, D.engine.LBFGS_START)
    # fill level 0: steepest descent and torch's first step length
    d = D.d.cpu().numpy()
    assert head['stop'] == 0.0 and head['count'] == 0.0 and head['n_iter'] == 1.0 and head['H_diag'] == 1.0
    assert np.array_equal(d[live], -g[live])
    t0 = min(1.0, 1.0 / np.abs(g[live].astype(np.float64)).sum()) * D.lr
    assert abs(head['t'] - t0) <= 1e-6 * t0
    assert abs(head['gtd'] + (g[live].astype(np.float64) ** 2).sum()) <= 1e-12 * abs(head['gtd'])
    assert head['gmax'] == np.abs(g[live]).max()
    want = p0[live] + np.float32(head['t']) * d[live]
    assert rel_l2(D.params.cpu().numpy()[live], want) < 1e-7
    worst = 0.0
    for k in range(1, updates + 1):
        s = (np.float32(D.t) * D.d.cpu().numpy()).astype(np.float32)
        scale = rng.uniform(0.5, 1.5, p).astype(np.float32)
        drop = k == 3                                   # one pair against the curvature: y . s < 0
        g = (D.prev.cpu().numpy() + (-scale if drop else scale) * s / np.float32(D.t) + 1e-3 * rng.randn(p).astype(np.float32)).astype(np.float32)
        g[~live] = rng.randn(int((~live).sum())).astype(np.float32)         # (masked entries of g: anything)
        before = dict(count=head['count'], head=head['head'], H=head['H_diag'], S=D.S.clone(), Y=D.Y.clone(), gram=[a.copy() for a in D.gram()])
        p_before = D.params.cpu().numpy().copy()
        head = D.call(g, D.engine.LBFGS_LOOP)
        assert head['stop'] == 0.0 and head['n_iter'] == k + 1
        if drop:
            assert head['pushed'] == 0.0 and head['ys'] <= 1e-10
            assert head['count'] == before['count'] and head['head'] == before['head'] and head['H_diag'] == before['H']
            bits = lambda t: t.view(torch.int32)
            assert torch.equal(bits(D.S), bits(before['S'])) and torch.equal(bits(D.Y), bits(before['Y']))
            assert all(np.array_equal(a, b) for a, b in zip(D.gram(), before['gram']))
        else:
            assert head['pushed'] == 1.0 and head['ys'] > 1e-10
            assert head['count'] == min(before['count'] + 1, m)
        if k % check_every and k != updates:
            continue
        S, Y, order = D.pairs(head)
        for s_, y_ in zip(S, Y):
            assert np.isnan(s_[~live]).all() and np.isnan(y_[~live]).all()          # masked entries of the ring: never written
        S, Y = [np.where(live, s_, np.float32(0)) for s_ in S], [np.where(live, y_, np.float32(0)) for y_ in Y]
        # the newest pair is s = t d, y = g - prev as torch forms them, the kept matrices are the pairs' products in fp64
        if not drop:
            assert np.array_equal(S[-1][live], s[live]) and abs(head['H_diag'] - head['ys'] / head['yy']) <= 1e-15 * head['H_diag']
        SY, YY = D.gram()
        S64, Y64 = np.array(S, dtype=np.float64), np.array(Y, dtype=np.float64)
        sub = np.ix_(order, order)
        np.testing.assert_allclose(SY[sub], S64 @ Y64.T, rtol=1e-11, atol=1e-13 * np.abs(S64 @ Y64.T).max())
        np.testing.assert_allclose(YY[sub], Y64 @ Y64.T, rtol=1e-11, atol=1e-13 * np.abs(Y64 @ Y64.T).max())
        gl = np.where(live, g, 0.0).astype(np.float32)
        ref = _two_loop(gl, S, Y, head['H_diag'], torch.float64)
        low = _two_loop(gl, S, Y, head['H_diag'], torch.float32)
        got = D.d.cpu().numpy()
        err, err32 = rel_l2(got[live], ref[live]), rel_l2(low[live], ref[live])
        worst = max(worst, err / max(err32, 1e-6))
        print(f'p={p} m={m} update {k} ({len(S)} pairs): kernel {err:.2e}, torch fp32 recursion {err32:.2e} against fp64')
        assert err <= max(err32, 1e-6), (k, err, err32)
        assert abs(head['gtd'] - gl.astype(np.float64) @ ref) <= 1e-9 * np.linalg.norm(gl) * np.linalg.norm(ref)
        assert head['t'] == D.lr
        want = p_before[live] + np.float32(D.lr) * got[live]
        assert rel_l2(D.params.cpu().numpy()[live], want) < 1e-7
    record_margin('test_lbfgs', f'direction p={p} m={m}', 'kernel error / max(torch fp32 recursion, 1e-6)', worst, 1.0)
    # masked entries of the direction, the previous gradient and the parameters: bit-identical
    for key, buf in (('params', D.params), ('d', D.d), ('prev', D.prev)):
        assert np.array_equal(buf.cpu().numpy()[~live], keep[key][~live]), key
    return D, head


# (p: smaller than one sweep of 1024 entries; not a multiple of the vector width; some of a workgroup's four sweeps; several workgroups of the dots
#  pass (slices of 4096) and no multiple of the slice)
@pytest.mark.parametrize('p,m,updates', [(700, 3, 7), (701, 3, 4), (2500, 3, 5), (4500, 3, 4), (700, 1, 3), (700, 100, 4)])
def test_direction_kernels_against_the_fp64_recursion(pa, emu_lib, p, m, updates):
    _direction_case(pa, emu_lib, 'cpu', p, m, updates)


@pytest.mark.gpu
@pytest.mark.parametrize('p,m,updates,every', [(5000, 3, 7, 1), (5001, 3, 4, 1), (9000, 3, 4, 1), (700, 1, 3, 1), (5000, 100, 104, 13), (1023, 128, 5, 1)])
def test_direction_kernels_against_the_fp64_recursion_on_the_gpu(pa, p, m, updates, every):
    _direction_case(pa, pa.engine.load_library(), 'cuda', p, m, updates, every)


def _direction_stop_case(pa, lib, device):
    """ the stopping rules inside the direction call leave every buffer as it was; a directional derivative above -tolerance_change stores the
    direction and takes no step """
    D, head = _direction_case(pa, lib, device, 700, 3, 2)
    rng = D.rng
    bits = lambda t: t.clone().view(torch.int32 if t.dtype == torch.float32 else torch.int64)        # (the rings hold NaN where nothing takes part)
    state = lambda: [bits(t) for t in (D.params, D.d, D.prev, D.S, D.Y, D.ctrl[:6], D.ctrl[9:12], D.ctrl[16:])]
    g = rng.randn(700).astype(np.float32)
    for mode, kw, code in ((0, dict(tol_grad=1e9), 1.0), (1, dict(tol_grad=1e9), 1.0), (1, dict(tol_change=1e9), 2.0)):
        before = state()
        assert D.call(g, mode, **kw)['stop'] == code
        assert all(torch.equal(a, b) for a, b in zip(before, state())), (mode, kw)
    D2, _ = _direction_case(pa, lib, device, 700, 3, 1)
    params = D2.params.clone()
    out = D2.call(rng.randn(700).astype(np.float32), 0, tol_change=1e30)
    assert out['stop'] == 4.0 and out['n_iter'] == 3.0 and torch.equal(D2.params, params)
    assert np.array_equal(D2.prev.cpu().numpy()[D2.live], D2.g.cpu().numpy()[D2.live])
    # refusals of the entry point: non-zero, a message, nothing launched
    with pytest.raises(RuntimeError, match='history_size'):
        D.net.lbfgs_direction(D.params, D.g, D.prev, D.d, torch.zeros((129, 700), device=device), torch.zeros((129, 700), device=device), D.mask,
                              129, 0, True, 0.0, 1.0, 1e-7, 1e-9, D.ctrl, D.rows, off_loss=0)
    with pytest.raises(RuntimeError, match='workspace too small'):
        D.net.lbfgs_direction(D.params, D.g, D.prev, D.d, D.S, D.Y, D.mask, 3, 0, True, 0.0, 1.0, 1e-7, 1e-9, D.ctrl, D.rows[:4], off_loss=0)
    with pytest.raises(RuntimeError, match='control block'):
        D.net.lbfgs_direction(D.params, D.g, D.prev, D.d, D.S, D.Y, D.mask, 3, 0, True, 0.0, 1.0, 1e-7, 1e-9, D.ctrl[:16], D.rows, off_loss=0)


def test_direction_stopping_rules_and_refusals(pa, emu_lib):
    _direction_stop_case(pa, emu_lib, 'cpu')


@pytest.mark.gpu
def test_direction_stopping_rules_and_refusals_on_the_gpu(pa):
    _direction_stop_case(pa, pa.engine.load_library(), 'cuda')


# ---- 3. the fused optimizer path against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_fused', STEP_PATHS, ids=['fused_step', 'generic_step'])
@pytest.mark.parametrize('name', ['cfg1', 'cfg2'])
def test_flat_lbfgs_follows_the_oracle(pa, emu_lib, name, use_fused):
    _wolfe_case(pa, emu_kwargs(emu_lib), name, 'fused', use_fused)


@pytest.mark.gpu
@pytest.mark.parametrize('use_fused', STEP_PATHS, ids=['fused_step', 'generic_step'])
@pytest.mark.parametrize('name', ['cfg1', 'cfg2'])
def test_flat_lbfgs_follows_the_oracle_on_the_gpu(pa, name, use_fused):
    _wolfe_case(pa, {}, name, 'fused', use_fused)


def _continue_case(pa, extra):
    """ `_fit_lbfgs` continues with fit(optimizer=None): the same object, history intact, torch's counters """
    from pydens_amd.solver import FlatLBFGS
    solver, evals = _fit_lbfgs(pa, extra, 'cfg1', WOLFE, 'fused')
    opt = solver.optimizer
    assert type(opt) is FlatLBFGS and opt.func_evals == sum(evals)
    state = opt.state
    assert state['history'] == WOLFE['history_size'] and state['n_iter'] == opt.n_iter >= NITERS and state['H_diag'] > 0
    assert opt.S.abs().sum() > 0 and opt.d.abs().sum() > 0


def test_flat_lbfgs_carries_its_state_across_fit_calls(pa, emu_lib):
    _continue_case(pa, emu_kwargs(emu_lib))


@pytest.mark.gpu
def test_flat_lbfgs_carries_its_state_across_fit_calls_on_the_gpu(pa):
    _continue_case(pa, {})


def _variable_problem(D, V):
    def odevar(f, x):
        return D(f, x) - 2 * np.pi * torch.cos(2 * np.pi * x) + V('new_var', data=torch.Tensor([1.0]))
    return odevar


def _variable_oracle(dtype, start, pts):
    from oracle import pinn_oracle as po
    kw = dict(ndims=1, initial_condition=1, layout='fafaf', features=[12, 10, 1], activation='Tanh')
    torch.manual_seed(11)
    oracle = po.OracleSolver(_variable_problem(po.D, po.V), dtype=dtype, **kw)
    if start is not None:
        oracle.import_params(start)
    start = oracle.export_params()
    first = oracle.model.linears()[0]
    first.weight.requires_grad = False
    first.bias.requires_grad = False
    opt = torch.optim.LBFGS([p for p in oracle.model.parameters() if p.requires_grad], **WOLFE)
    losses = [float(opt.step(lambda p=p: torch.tensor(oracle.evaluate(p)['loss'], dtype=dtype))) for p in pts]
    return dict(start=start, kw=kw, losses=losses, params=oracle.export_params(), var=float(oracle.model.new_var.detach()))


def _frozen_and_variable_case(pa, extra):
    """ a frozen layer is neither moved nor counted in any product (its entries of ring and direction stay zero); a trainable V(...) scalar
    is stepped, as in the oracle (fp32, fp64 as arbiter: on this problem the fp32 reference is the noisy side) """
    pts = np.random.RandomState(5).rand(2, 40, 1).astype(np.float32)
    want = _variable_oracle(torch.float32, None, pts)
    want64 = _variable_oracle(torch.float64, want['start'], pts)
    solver = pa.Solver(_variable_problem(pa.D, pa.V), **want['kw'], **extra)
    load_params(solver, want['start'])
    frozen = solver.model.conv_block[0]                 # (what freeze_trainable does, for ONE layer of the block)
    frozen.weight.requires_grad = False
    frozen.bias.requires_grad = False
    keep = [frozen.weight.detach().clone(), frozen.bias.detach().clone()]
    solver.set_optimizer_path('fused')
    solver.fit(niters=2, batch_size=40, sampler=FixedBatches(pts), optimizer='LBFGS', **WOLFE)
    assert solver.last_fit_optimizer == 'LBFGS/fused'
    assert torch.equal(frozen.weight.detach(), keep[0]) and torch.equal(frozen.bias.detach(), keep[1])
    view = lambda buf, p: buf.as_strided(tuple(p.shape), tuple(p.stride()), p.storage_offset())
    o = solver.optimizer
    for j in range(o.S.shape[0]):
        assert not view(o.S[j], frozen.weight).any() and not view(o.Y[j], frozen.weight).any()
    assert not view(o.d, frozen.weight).any() and o.S.abs().sum() > 0
    for i, v in enumerate(solver.losses):
        ok, err, arb = close_or_arbitrated(float(v), want['losses'][i], lambda i=i: want64['losses'][i], LOSS_RTOL, atol=0.0)
        print(f'frozen + variable: loss {i} rel err {err:.2e}{" (fp64 arbiter)" if arb else ""}')
        assert ok, (i, float(v), want['losses'][i], want64['losses'][i])
    var = float(solver.model.new_var.detach())
    assert var != 1.0
    assert abs(var - want['var']) < 2e-5 or abs(var - want64['var']) <= max(2.0 * abs(want['var'] - want64['var']), 2e-5)
    for i, (p, w) in enumerate(zip(export_params(solver), want['params'])):
        ok, err, arb = close_or_arbitrated(p, w, lambda i=i: want64['params'][i], PARAM_RTOL, atol=3e-7)
        print(f'frozen + variable: tensor {i} rel err {err:.2e}{" (fp64 arbiter)" if arb else ""}')
        assert ok, (i, err, arb)


def test_flat_lbfgs_with_a_frozen_layer_and_a_trainable_variable(pa, emu_lib):
    _frozen_and_variable_case(pa, emu_kwargs(emu_lib))


@pytest.mark.gpu
def test_flat_lbfgs_with_a_frozen_layer_and_a_trainable_variable_on_the_gpu(pa):
    _frozen_and_variable_case(pa, {})


# ---- 4. stopping rules ------------------------------------------------------------------------------------------------------------------------------
def _stopping_case(pa, extra):
    for setting in (dict(lr=1, max_iter=4, max_eval=3, history_size=4, line_search_fn='strong_wolfe'), dict(lr=0.1, max_iter=3, history_size=4),
                    dict(lr=0.1, max_iter=6, max_eval=4, history_size=2)):
        want = _oracle_run('cfg1', setting, torch.float32, 2)['evals']
        for path in ('torch', 'fused'):
            solver, evals = _fit_lbfgs(pa, extra, 'cfg1', setting, path, niters=2)
            assert evals == want, (setting, path, evals, want)
            if path == 'fused':
                assert solver.optimizer.func_evals == sum(want)
    # a start gradient below tolerance_grad: exactly one evaluation, nothing moves
    for path in ('torch', 'fused'):
        _, solver = make_solver('cfg1', pa, **extra)
        load_params(solver, Golden('cfg1').params)
        solver.set_optimizer_path(path)
        before = solver.model.flat.clone()
        solver.fit(niters=1, batch_size=BATCH, sampler=FixedBatches(_points('cfg1', 1)), optimizer='LBFGS', tolerance_grad=1e30, **WOLFE)
        assert solver.optimizer.closure_calls == 1 and torch.equal(solver.model.flat, before) and np.isfinite(float(solver.losses[-1]))


def test_stopping_rules_count_evaluations_as_torch_does(pa, emu_lib):
    _stopping_case(pa, emu_kwargs(emu_lib))


@pytest.mark.gpu
def test_stopping_rules_count_evaluations_as_torch_does_on_the_gpu(pa):
    _stopping_case(pa, {})


# ---- 5. refusals and fall-backs ------------------------------------------------------------------------------------------------------------------
def test_what_keeps_the_torch_path(pa, emu_lib):
    from pydens_amd.solver import FlatLBFGS, TorchOptimizerAdapter
    _, solver = make_solver('cfg1', pa, **emu_kwargs(emu_lib))
    solver.set_optimizer_path('fused')
    pts = _points('cfg1', 1)
    fit = lambda **kw: solver.fit(niters=1, batch_size=BATCH, sampler=FixedBatches(pts), optimizer='LBFGS', **kw)
    fit(**WOLFE)
    assert solver.last_fit_optimizer == 'LBFGS/fused' and solver.optimizer_refusal is None
    p_total = solver.model.flat.numel()
    history = FlatLBFGS.HISTORY_BUDGET // (8 * p_total) + 1
    with pytest.warns(RuntimeWarning, match=f'{2 * history * p_total * 4} bytes'):
        fit(lr=1, max_iter=2, history_size=history)
    assert solver.last_fit_optimizer == 'LBFGS/torch' and isinstance(solver.optimizer, TorchOptimizerAdapter)
    assert str(FlatLBFGS.HISTORY_BUDGET) in solver.optimizer_refusal
    with pytest.warns(RuntimeWarning, match='history_size=129'):
        fit(lr=1, max_iter=2, history_size=129)
    assert solver.last_fit_optimizer == 'LBFGS/torch'
    before = solver.model.flat.clone()
    for kw in (dict(lr=torch.tensor(1.0), max_iter=2), dict(lr=1, max_iter=2, tolerance_grad=torch.tensor(1e-7))):
        fit(**kw)
        assert solver.last_fit_optimizer == 'LBFGS/torch' and solver.optimizer_refusal is None
    assert not torch.equal(solver.model.flat, before)                     # ... and still trains
    assert FlatLBFGS.hyper('LBFGS', 1, dict(foreach=True)) is None and FlatLBFGS.hyper('LBFGS', 1, dict(line_search_fn='armijo')) is None
    with pytest.raises(TypeError):
        fit(lr=1, foreach=True)                         # (torch.optim.LBFGS takes no such keyword: torch raises, as on the default path)
    with pytest.raises(ValueError):
        fit(lr=-1.0)
    # data parallel keeps torch.optim (decided in front of any kernel)
    solver._world = lambda: (0, 2)
    assert not solver._lbfgs_on_the_kernels('LBFGS', 1, {k: v for k, v in WOLFE.items() if k != 'lr'}) and solver.optimizer_refusal is None
    del solver._world


def test_strong_wolfe_of_the_installed_torch_has_the_signature_the_fused_path_calls():
    from torch.optim.lbfgs import _strong_wolfe
    names = list(inspect.signature(_strong_wolfe).parameters)
    assert names[:7] == ['obj_func', 'x', 't', 'd', 'f', 'g', 'gtd'] and 'max_ls' in names and 'tolerance_change' in names
    # f(x) = |x|^2 / 2 from x = (2, 0) along -g: returns (f_new, g_new, t, evaluations), the objective is called as (x, t, d)
    x, d = torch.tensor([2.0, 0.0]), torch.tensor([-2.0, 0.0])
    out = _strong_wolfe(lambda x, t, d: (float(((x + t * d) ** 2).sum() / 2), x + t * d), x, 1.0, d, 2.0, torch.tensor([2.0, 0.0]), -4.0, max_ls=10)
    assert len(out) == 4 and out[0] < 2.0 and out[3] >= 1


# ---- 6. bit-repeatability -------------------------------------------------------------------------------------------------------------------------
def _repeat_case(pa, extra):
    runs = [_fit_lbfgs(pa, extra, 'cfg1', WOLFE, 'fused')[0] for _ in range(2)]
    assert torch.equal(runs[0].model.flat, runs[1].model.flat)
    assert torch.equal(runs[0].optimizer.S, runs[1].optimizer.S) and torch.equal(runs[0].optimizer.ctrl, runs[1].optimizer.ctrl)
    return runs[0]


@pytest.mark.parametrize('seed', [0, 5])
def test_flat_lbfgs_is_bit_repeatable(pa, emu_lib, monkeypatch, seed):
    """ ... also with the waves of a workgroup advancing in a random order (the emulator's shuffle mode: a missing barrier turns into bits) """
    monkeypatch.delenv('PINN_EMU_SHUFFLE', raising=False)
    plain = _repeat_case(pa, emu_kwargs(emu_lib)).model.flat.clone()
    if seed:
        monkeypatch.setenv('PINN_EMU_SHUFFLE', str(seed))
        assert torch.equal(_repeat_case(pa, emu_kwargs(emu_lib)).model.flat, plain)
        D, head = _direction_case(pa, emu_lib, 'cpu', 2500, 3, 5)
        monkeypatch.delenv('PINN_EMU_SHUFFLE')
        E, _ = _direction_case(pa, emu_lib, 'cpu', 2500, 3, 5)
        assert torch.equal(D.d, E.d) and torch.equal(D.ctrl, E.ctrl) and torch.equal(D.params, E.params)


@pytest.mark.gpu
def test_flat_lbfgs_is_bit_repeatable_on_the_gpu(pa):
    _repeat_case(pa, {})


# ---- 7. data parallel ------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


DP_BATCH = 33


def _dp_points():
    return np.random.RandomState(3).rand(2, DP_BATCH, 2).astype(np.float32)


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
    _, solver = make_solver('cfg1', pa, _lib=lib, device='cpu')
    solver.set_optimizer_path('fused')                  # (world 2: torch.optim.LBFGS all the same)
    if rank == 0:
        load_params(solver, Golden('cfg1').params)
    calls = []
    for pts in _dp_points():
        solver.fit(niters=1, batch_size=DP_BATCH, sampler=FixedBatches(pts[None, rank::world]), optimizer='LBFGS' if not calls else None, **WOLFE)
        calls.append(solver.optimizer.closure_calls)
    assert solver.last_fit_optimizer == 'LBFGS/torch'
    np.savez(os.path.join(out_dir, f'rank{rank}.npz'), losses=np.array([float(v) for v in solver.losses]), calls=np.array(calls),
             **{f'p{i}': p for i, p in enumerate(export_params(solver))})
    dist.destroy_process_group()


def test_two_ranks_follow_the_single_process(pa, emu_lib):
    """ gloo, world 2, uneven shares (33 points): the torch path gives the parameters of world 1 on the same global batches within the 1e-5 of
    tests/test_data_parallel.py, and both ranks make the same number of closure calls """
    _, single = make_solver('cfg1', pa, **emu_kwargs(emu_lib))
    load_params(single, Golden('cfg1').params)
    calls = []
    for pts in _dp_points():
        single.fit(niters=1, batch_size=DP_BATCH, sampler=FixedBatches(pts[None]), optimizer='LBFGS' if not calls else None, **WOLFE)
        calls.append(single.optimizer.closure_calls)
    want_losses, want = np.array([float(v) for v in single.losses]), export_params(single)
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_dp_worker, args=(2, _free_port(), tmp), nprocs=2, join=True)
        z = [np.load(os.path.join(tmp, f'rank{rank}.npz')) for rank in range(2)]
        assert list(z[0]['calls']) == list(z[1]['calls']) == calls
        for rank in range(2):
            np.testing.assert_allclose(z[rank]['losses'], want_losses, rtol=1e-5)
            for i, w in enumerate(want):
                assert rel_l2(z[rank][f'p{i}'], w) < 1e-5, (rank, i)
