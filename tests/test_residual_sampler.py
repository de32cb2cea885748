""" Residual-adaptive sampling: `Solver.residual` (the pointwise equation residual, forward only), the device resampler (include/pinn.h
pinn_resample_points: weights, fp64 prefix sums, inverse-CDF draw with Philox uniforms) and `ResidualSampler` on top of both.
Every case runs on the emulator in the CPU tier and, marked `gpu`, on the device (the `tier` fixture).
  a. the residual field against the fp32 oracle, the fp64 oracle as arbiter, at the project's field bar; no side effects on a fit
  b. the resampler against the numpy fp64 statement of this file (`statement`), uniforms from oracle/philox.py
  c. fits with a ResidualSampler against the oracle on the very batches the sampler drew; accounting; data parallelism (gloo) """
import ctypes
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import pinn_configs as pc
from conftest import Golden
from helpers import (FixedBatches, close_or_arbitrated, export_params, fit_close, load_params, make_solver, record_margin)
from oracle import philox
from oracle import pinn_oracle as po

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'emu'))

FIELD_RTOL = 1e-5           # the project's field bar: of max|r| over the batch


class Tier:
    def __init__(self, name):
        from pydens_amd import engine
        self.name = name
        if name == 'emu':
            import build_emu
            self.lib = engine.bind(ctypes.CDLL(build_emu.build()))
            assert self.lib.pinn_backend() == b'emu-host'
            self.device, self.solver_kwargs = 'cpu', dict(_lib=self.lib, device='cpu')
        else:
            assert torch.cuda.is_available(), 'the gpu tier needs a HIP device'
            self.lib = engine.load_library()
            self.device, self.solver_kwargs = 'cuda', {}
        self.net = engine.Net([2, 16, 1], 'tanh', 2, lib=self.lib)


@pytest.fixture(scope='module', params=['emu', pytest.param('gpu', marks=pytest.mark.gpu)])
def tier(request):
    return Tier(request.param)


@pytest.fixture(scope='module')
def pa():
    import pydens_amd
    return pydens_amd


# ---- a. the residual field ------------------------------------------------------------------------------------------------------------
_FIELD_REFERENCE = {}


def _field_reference(name):
    """ (points [1000, d], fp32 oracle residual, fp64 oracle residual as a function), computed once per fixture and shared by the tiers """
    if name not in _FIELD_REFERENCE:
        g = Golden(name)
        ocfg = pc.make_config(name, po.D, torch)
        pts = pc.sample_points(ocfg, 1000, seed=11)
        oracle = po.OracleSolver(ocfg['equation'], **ocfg['solver_kwargs'])
        oracle.import_params(g.params)
        r32 = oracle.evaluate(pts)['r'].reshape(-1)
        cache = {}

        def r64():
            if 'r' not in cache:
                o64 = po.OracleSolver(ocfg['equation'], **ocfg['solver_kwargs'], dtype=torch.float64)
                o64.import_params(g.params)
                cache['r'] = o64.evaluate(pts.astype(np.float64))['r'].reshape(-1)
            return cache['r']
        _FIELD_REFERENCE[name] = (pts, r32, r64)
    return _FIELD_REFERENCE[name]


def _field_close(got, want32, want64_fn, test, case):
    """ every entry within FIELD_RTOL * max|r| -- the max over the batch that was EVALUATED, one point included -- of the fp32 oracle; where the oracle's own fp32 arithmetic is the noisy
    side, the fp64 oracle arbitrates with k = 2 -- helpers.close_or_arbitrated on the L2 norms (the bar per entry is its absolute floor:
    rtol = 0, atol = FIELD_RTOL * max|r|), and the same rule entry by entry in the max norm, so that no single entry hides in the norm.
    No entry is set aside. """
    got, want32 = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want32, dtype=np.float64).ravel()
    scale = float(np.abs(want32).max())
    bar = FIELD_RTOL * scale
    ok, err, arb = close_or_arbitrated(got, want32, want64_fn, rtol=0.0, atol=bar, k=2.0)
    worst = float(np.abs(got - want32).max())
    if worst > bar:
        w64 = np.asarray(want64_fn(), dtype=np.float64).ravel()
        arb = True
        ok = ok and float(np.abs(got - w64).max()) <= max(2.0 * float(np.abs(want32 - w64).max()), bar)
    record_margin(test, case, 'residual', worst / max(scale, 1e-30), FIELD_RTOL, arb)
    print(f'{test} {case}: max|r - ref32| / max|r| = {worst / max(scale, 1e-30):.3e} (bar {FIELD_RTOL:.0e}), arbitrated={arb}')
    return ok


@pytest.mark.parametrize('name', ['cfg2', 'cfg3', 'mixed'])
def test_residual_field_matches_the_oracle(pa, tier, name):
    g = Golden(name)
    _, solver = make_solver(name, pa, **tier.solver_kwargs)
    load_params(solver, g.params)
    pts, r32, r64 = _field_reference(name)
    grads_before = solver.grads.clone()
    mode_before = solver.model.training
    for n in (1, 1000):
        got = solver.residual(*[pts[:n, c] for c in range(pts.shape[1])])
        assert isinstance(got, np.ndarray) and got.shape == (n, 1) and got.dtype == np.float32
        assert _field_close(got.reshape(-1), r32[:n], lambda: r64()[:n], 'residual_field', f'{name} n={n} {tier.name}')
    assert torch.equal(solver.grads, grads_before) and solver.model.training == mode_before
    assert all(p.grad is None for p in solver.model.parameters())
    # a pool larger than the slice budget goes through in slices (three, the last one ragged): the same field at the same bar, taken
    # from the max|r| of the 130 points evaluated
    solver.RESIDUAL_SLICE = 64
    sliced = solver._residual_device(torch.from_numpy(pts[:130].copy()).to(solver.device))
    assert sliced.shape == (130,) and sliced.dtype == torch.float32 and sliced.device.type == solver.device.type
    assert _field_close(sliced.cpu().numpy(), r32[:130], lambda: r64()[:130], 'residual_field', f'{name} sliced {tier.name}')


def test_residual_does_not_depend_on_the_lowering(pa, tier):
    """ the generic forward half serves every equation: with the residual program taken away the field is the same bit for bit """
    g = Golden('cfg2')
    _, solver = make_solver('cfg2', pa, **tier.solver_kwargs)
    load_params(solver, g.params)
    pts = _field_reference('cfg2')[0][:257]
    a = solver.residual(pts[:, 0], pts[:, 1])
    solver.program = None
    b = solver.residual(pts[:, 0], pts[:, 1])
    assert np.array_equal(a, b)
    # set_gemm_mode is honoured: whatever forward the mode selects (operands split into three bf16 parts are exact, the six products kept
    # are accumulated in fp32 like the fp32 form's), the field holds the same bar against the oracle (of the max|r| of these 257 points)
    solver.set_gemm_mode('bf16x3')
    c = solver.residual(pts[:, 0], pts[:, 1])
    _, r32, r64 = _field_reference('cfg2')
    assert _field_close(c.reshape(-1), r32[:257], lambda: r64()[:257], 'residual_field', f'cfg2 bf16x3 {tier.name}')


def test_residual_of_a_nested_skip_net_keeps_the_step_scratch_alone(pa, tier):
    """ nets with a skip inside a skip need forward scratch. The step's buffer (`Net._fwd_ws`) is part of what a recorded launch graph of
    the generic step carries, so `residual` -- whose pools are larger than any batch -- takes a buffer of its own. The field: the golden
    residual of the fixture's first batch (Burgers, callable IC, second kernel set), the bar of its own max|r|, fp64 oracle as arbiter. """
    g = Golden('nested_acts')
    _, solver = make_solver('nested_acts', pa, **tier.solver_kwargs)
    load_params(solver, g.params)
    net = solver.model.net
    assert net.nested
    pts = g.points[0]
    solver.predict(pts[:8, 0], pts[:8, 1])                       # the step's forward scratch, sized for 8 points
    step_ws = net._fwd_ws
    assert step_ws is not None
    got = solver.residual(pts[:, 0], pts[:, 1])
    assert net._fwd_ws is step_ws and net._residual_fwd_ws is not step_ws
    ocfg = pc.make_config('nested_acts', po.D, torch)

    def r64():
        o64 = po.OracleSolver(ocfg['equation'], **ocfg['solver_kwargs'], dtype=torch.float64)
        o64.import_params(g.params)
        return o64.evaluate(pts.astype(np.float64))['r'].reshape(-1)
    assert _field_close(got.reshape(-1), np.asarray(g.residual).reshape(-1), r64, 'residual_field', f'nested_acts {tier.name}')


@pytest.mark.parametrize('fused', [True, False])
def test_residual_between_two_fits_changes_nothing(pa, tier, fused):
    g = Golden('cfg2')
    pts = g.points[:, :40]                          # (one ragged tile: the emulator's cost is per point)

    def run(call_residual):
        torch.manual_seed(7)
        _, solver = make_solver('cfg2', pa, **tier.solver_kwargs)
        load_params(solver, g.params)
        solver.use_fused = fused
        solver.fit(niters=2, batch_size=40, sampler=FixedBatches(pts[:2]), lr=g.lr)
        if call_residual:
            grads = solver.grads.clone()
            solver.residual(pts[2][:, 0], pts[2][:, 1])
            assert torch.equal(grads, solver.grads)
        solver.fit(niters=2, batch_size=40)                     # default sampler: keyed from torch's generator, which `residual` must not advance
        return np.array([float(v) for v in solver.losses]), export_params(solver)
    la, pa_ = run(False)
    lb, pb = run(True)
    assert np.array_equal(la, lb)
    assert all(np.array_equal(x, y) for x, y in zip(pa_, pb))


# ---- b. the resampler against its numpy statement -------------------------------------------------------------------------------------
def fold_key(seed):
    """ the key fold of include/pinn.h pinn_resample_points (splitmix64 finaliser over seed ^ 'RESMPLER') """
    mask = 2 ** 64 - 1
    z = (seed ^ 0x5245534D504C4552) & mask
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
    return z ^ (z >> 31)


def uniforms(n_out, seed, call):
    """ the 53-bit uniform of output row i: one Philox block, counter (i low, i high, call low, call high) """
    i = np.arange(n_out, dtype=np.uint64)
    key = fold_key(seed)
    w = philox.philox4x32_10((i & philox.MASK).astype(np.uint32), (i >> np.uint64(32)).astype(np.uint32), np.uint32(call & 0xFFFFFFFF),
                             np.uint32((call >> 32) & 0xFFFFFFFF), key & 0xFFFFFFFF, key >> 32)
    hi, lo = (w[0] >> np.uint32(5)).astype(np.float64), (w[1] >> np.uint32(6)).astype(np.float64)
    return (hi * 2.0 ** 26 + lo) * 2.0 ** -53


def statement(r, power, floor, n_out, seed, call):
    """ numpy fp64 statement of the resampler -> dict(q, P, t, u, j): j is None where the selection is by prefix sums (checked with the
    slack of `check_draw`), the exact indices in the uniform fall-back """
    r = np.asarray(r, dtype=np.float32).astype(np.float64)
    m = r.size
    w = np.abs(r) ** power
    w[~np.isfinite(r)] = 0.0
    q = w + floor * (w.sum() / m)
    P = np.cumsum(q)
    u = uniforms(n_out, seed, call)
    if P[-1] == 0.0:
        return dict(q=q, P=P, u=u, t=None, j=np.minimum(m - 1, np.floor(u * m).astype(np.int64)))
    return dict(q=q, P=P, u=u, t=u * P[-1], j=None)


def check_draw(ref, pool, xs, idx):
    """ indices inside the slack of the fp64 sums, no zero-weight row while any weight is positive, rows copied bit for bit """
    m = ref['P'].size
    assert idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < m
    if ref['j'] is not None:
        assert np.array_equal(idx, ref['j'])
    else:
        P, t = ref['P'], ref['t']
        s = m * 2.0 ** -52 * P[-1]             # two fp64 sums of m non-negative terms, each within m 2^-53 of the exact sum
        below = np.where(idx > 0, P[np.maximum(idx - 1, 0)], 0.0)
        assert np.all(below - s <= t) and np.all(t <= P[idx] + s)
        assert np.all(ref['q'][idx] > 0.0)
    assert np.array_equal(xs.view(np.uint32), pool[idx].view(np.uint32))


def make_pool(m, d, kind='normal', seed=0):
    rng = np.random.RandomState(1000 * m + d + seed)
    pool = rng.rand(m, d).astype(np.float32)
    r = (rng.randn(m) * np.exp(2.0 * rng.randn(m))).astype(np.float32)      # residuals over several decades
    if kind == 'half_zero':
        r[rng.permutation(m)[:m // 2]] = 0.0
        r[0] = 0.0                              # (first and last rows: the borders of the search)
        if m > 1:
            r[-1] = 0.0
    elif kind == 'all_zero':
        r[:] = 0.0
    elif kind == 'nonfinite':
        r[m // 3], r[2 * m // 3] = np.inf, np.nan
    return pool, r


def device_draw(tier, pool, r, n_out, power, floor, seed, call, **kwargs):
    tp, tr = torch.from_numpy(pool).to(tier.device), torch.from_numpy(r).to(tier.device)
    xs, idx, ws = tier.net.resample_points(tp, tr, n_out, power, floor, seed, call, **kwargs)
    return xs.cpu().numpy(), idx.cpu().numpy(), ws, tp


# (M, n_out, d, power, floor): every M on a workgroup border and one past the first 256 block totals, every n_out, d, power and floor
DRAW_CASES = [(1, 1, 1, 1, 0.0), (1, 64, 3, 2, 1.0), (255, 64, 3, 1, 1.0), (255, 1000, 8, 2, 0.0), (256, 1, 8, 2, 1.0), (256, 1000, 1, 1, 0.0),
              (257, 64, 1, 2, 0.0), (257, 1000, 3, 1, 1.0), (1000, 1, 3, 2, 1.0), (1000, 64, 8, 1, 0.0), (1000, 1000, 1, 2, 1.0),
              (65537, 1, 8, 1, 1.0), (65537, 64, 1, 2, 0.0), (65537, 1000, 3, 1, 0.0), (65537, 1000, 3, 2, 1.0)]


@pytest.mark.parametrize('m, n_out, d, power, floor', DRAW_CASES)
def test_resampler_matches_the_numpy_statement(tier, m, n_out, d, power, floor):
    pool, r = make_pool(m, d)
    seed, call = 0x0123456789abcdef + m, (1 << 33) + n_out
    xs, idx, _, _ = device_draw(tier, pool, r, n_out, power, floor, seed, call)
    check_draw(statement(r, power, floor, n_out, seed, call), pool, xs, idx)


@pytest.mark.parametrize('m', [255, 257, 1000, 65537])
@pytest.mark.parametrize('kind', ['half_zero', 'all_zero', 'nonfinite'])
def test_resampler_edge_pools(tier, m, kind):
    pool, r = make_pool(m, 3, kind)
    floor = 0.0
    xs, idx, _, _ = device_draw(tier, pool, r, 1000, 1, floor, 5, 9)
    ref = statement(r, 1, floor, 1000, 5, 9)
    check_draw(ref, pool, xs, idx)
    if kind == 'half_zero':
        assert np.all(r[idx] != 0.0)
    elif kind == 'all_zero':
        assert ref['j'] is not None and np.array_equal(idx, np.minimum(m - 1, np.floor(ref['u'] * m).astype(np.int64)))
    else:
        assert np.all(np.isfinite(r[idx]))
        # the others are unaffected: the same draw from the pool with the two rows' residuals set to zero
        r0 = np.where(np.isfinite(r), r, np.float32(0.0)).astype(np.float32)
        xs0, idx0, _, _ = device_draw(tier, pool, r0, 1000, 1, floor, 5, 9)
        assert np.array_equal(idx, idx0) and np.array_equal(xs, xs0)
        # ... and with a floor the non-finite rows are candidates of weight floor * mean like every other row
        xs1, idx1, _, _ = device_draw(tier, pool, r, 1000, 2, 1.0, 5, 9)
        check_draw(statement(r, 2, 1.0, 1000, 5, 9), pool, xs1, idx1)


def test_resampler_is_repeatable_and_redraws_from_a_filled_workspace(tier, monkeypatch):
    pool, r = make_pool(1000, 3)
    a = device_draw(tier, pool, r, 1000, 2, 1.0, 77, 3)
    b = device_draw(tier, pool, r, 1000, 2, 1.0, 77, 3)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    if tier.name == 'emu':                      # the waves of a workgroup in shuffled order: same sums, same rows
        monkeypatch.setenv('PINN_EMU_SHUFFLE', '3')
        c = device_draw(tier, pool, r, 1000, 2, 1.0, 77, 3)
        monkeypatch.delenv('PINN_EMU_SHUFFLE')
        assert np.array_equal(a[0].view(np.uint32), c[0].view(np.uint32)) and np.array_equal(a[1], c[1])
        assert torch.equal(a[2], c[2])          # the workspace too: weights' scans, block ends, head
    other = device_draw(tier, pool, r, 1000, 2, 1.0, 77, 4)
    assert not np.array_equal(a[1], other[1])
    assert not np.array_equal(a[1], device_draw(tier, pool, r, 1000, 2, 1.0, 78, 3)[1])
    # the redraw entry on the filled workspace of call 3 equals the full call with call number 4
    xs, idx, _ = tier.net.resample_points(a[3], None, 1000, seed=77, call_index=4, workspace=a[2], redraw=True)
    assert np.array_equal(idx.cpu().numpy(), other[1]) and np.array_equal(xs.cpu().numpy().view(np.uint32), other[0].view(np.uint32))
    # the draw stream is not the stream of pinn_sample_points under the same (seed, call): other key
    sampled = philox.sample_points(1000, [(philox.UNIFORM, 0.0, 1.0)], 77, 3)[:, 0]
    u24 = np.floor(uniforms(1000, 77, 3) * 2.0 ** 24) * 2.0 ** -24
    assert np.mean(sampled.astype(np.float64) == u24) < 0.01


DISTRIBUTION_SEED = 1


def test_resampler_distribution(tier):
    """ M = 8, r = 1 .. 8, power 1, floor 0: p_j = j / 36; 65 536 draws, every count within 5 sigma (binomial) of n p_j. Seed 1 is the
    first seed tried: the numpy statement of this file is inside 5 sigma with it (worst count 0.97 sigma off), so no seed was skipped. """
    n = 65536
    r = np.arange(1, 9, dtype=np.float32)
    pool = np.arange(8, dtype=np.float32).reshape(8, 1)
    p = r.astype(np.float64) / r.sum()
    sigma = np.sqrt(n * p * (1 - p))
    ref = statement(r, 1, 0.0, n, DISTRIBUTION_SEED, 0)
    want = np.searchsorted(ref['P'], ref['t'], side='right')
    assert np.all(np.abs(np.bincount(want, minlength=8) - n * p) <= 5 * sigma)
    xs, idx, _, _ = device_draw(tier, pool, r, n, 1, 0.0, DISTRIBUTION_SEED, 0)
    check_draw(ref, pool, xs, idx)
    counts = np.bincount(idx, minlength=8)
    print('counts', counts, 'expected', n * p, 'sigmas', (counts - n * p) / sigma)
    assert np.all(np.abs(counts - n * p) <= 5 * sigma)


def test_resampler_refusals_launch_nothing(tier):
    lib, dev = tier.lib, tier.device
    pool = torch.rand(300, 3, device=dev)
    r = torch.rand(300, device=dev)
    xs = torch.full((10, 3), -7.0, device=dev)
    idx = torch.full((10,), -7, dtype=torch.int32, device=dev)
    need = int(lib.pinn_resample_workspace_bytes(300))
    assert need >= 8 * 300 and need % 16 == 0 and lib.pinn_resample_workspace_bytes(0) == 0
    ws = torch.full((need // 8,), -7.0, dtype=torch.float64, device=dev)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def full(m=300, d=3, power=1, floor=1.0, n_out=10, workspace=ws, nbytes=need, pool_=pool, r_=r):
        return lib.pinn_resample_points(p(pool_), p(r_), m, d, power, floor, n_out, 1, 2, p(xs), p(idx), p(workspace), nbytes, None)
    cases = dict(m0=dict(m=0), m_neg=dict(m=-3), n_neg=dict(n_out=-1), d0=dict(d=0), d9=dict(d=9), power0=dict(power=0), power3=dict(power=3),
                 floor_neg=dict(floor=-0.5), floor_nan=dict(floor=float('nan')), floor_inf=dict(floor=float('inf')), floor_huge=dict(floor=1e200),
                 ws_null=dict(workspace=None), ws_small=dict(nbytes=need - 16), pool_null=dict(pool_=None), r_null=dict(r_=None))
    for name, kw in cases.items():
        assert full(**kw) != 0, name
        assert len(lib.pinn_last_error()) > 0, name
    assert lib.pinn_resample_redraw(p(pool), 300, 3, 10, 1, 2, p(xs), p(idx), None, need, None) != 0
    assert lib.pinn_resample_redraw(p(pool), 300, 3, 10, 1, 2, p(xs), p(idx), p(ws), need - 16, None) != 0
    assert lib.pinn_resample_redraw(p(pool), 300, 9, 10, 1, 2, p(xs), p(idx), p(ws), need, None) != 0
    assert full(n_out=0) == 0                                   # succeeds and does nothing
    # the Python binding refuses buffers the kernels would run past or that live elsewhere
    tp, tr = pool, r
    for kw in (dict(out=torch.empty((9, 3), device=dev)), dict(idx=torch.empty(9, dtype=torch.int32, device=dev)),
               dict(out=torch.empty((10, 2), device=dev))):
        with pytest.raises(ValueError):
            tier.net.resample_points(tp, tr, 10, workspace=ws, **kw)
    with pytest.raises(ValueError):
        tier.net.resample_points(tp, tr[:299], 10, workspace=ws)
    if dev == 'cuda':
        with pytest.raises(ValueError):
            tier.net.resample_points(tp, tr.cpu(), 10, workspace=ws)
    if dev == 'cuda':
        torch.cuda.synchronize()
    assert bool((xs == -7.0).all()) and bool((idx == -7).all()) and bool((ws == -7.0).all())       # no kernel ran in any of them
    assert full() == 0
    if dev == 'cuda':
        torch.cuda.synchronize()
    assert bool((idx >= 0).all()) and float(ws[3]) == 300.0


# ---- c. end to end ----------------------------------------------------------------------------------------------------------------------
def _recording(pa):
    class Recording(pa.ResidualSampler):
        """ keeps the batch of every iteration as the sampler's own record tells it: last_pool[last_indices] """
        def sample_device(self, size, device=None, generator=None):
            xs = super().sample_device(size, device, generator)
            batch = self.last_pool[self.last_indices.long()]
            assert torch.equal(batch, xs)
            self.__dict__.setdefault('batches', []).append(batch.cpu().numpy().copy())
            return xs
    return Recording


class _External:
    """ an external sampler without columns(): the parent's path for supplied points """
    def __init__(self, batches):
        self.batches, self.i = batches, 0

    def sample(self, size):
        self.i += 1
        return self.batches[self.i - 1].astype(np.float64)


@pytest.mark.parametrize('fused', [True, False])
def test_fit_with_a_residual_sampler_follows_the_oracle_on_the_drawn_batches(pa, tier, fused):
    g = Golden('cfg2')
    _, solver = make_solver('cfg2', pa, **tier.solver_kwargs)
    load_params(solver, g.params)
    solver.use_fused = fused
    sampler = _recording(pa)(pool=4, period=2, seed=3)
    solver.fit(6, 64, sampler=sampler, lr=g.lr)
    assert sampler.evaluations == 3 and len(sampler.batches) == 6
    assert sampler.last_pool.shape == (256, 2) and sampler.last_residual.shape == (256,) and sampler.last_indices.dtype == torch.int32
    batches = np.stack(sampler.batches)
    assert not np.array_equal(batches[0], batches[1])           # same pool, fresh uniforms
    ocfg = pc.make_config('cfg2', po.D, torch)

    def oracle(dtype):
        o = po.OracleSolver(ocfg['equation'], **ocfg['solver_kwargs'], dtype=dtype)
        o.import_params(g.params)
        o.fit(niters=6, batch_size=64, points=batches, lr=g.lr)
        return o
    fit_close('residual_sampler_fit', f"cfg2 {'fused' if fused else 'generic'} {tier.name}", solver, oracle(torch.float32),
              lambda: oracle(torch.float64), adam_move=6 * g.lr)
    # the same step path as any external sampler's fit
    _, other = make_solver('cfg2', pa, **tier.solver_kwargs)
    load_params(other, g.params)
    other.use_fused = fused
    other.fit(6, 64, sampler=_External(batches), lr=g.lr)
    assert solver.last_fit_path == other.last_fit_path == ('fused' if fused else 'generic')
    assert np.array_equal([float(v) for v in solver.losses], [float(v) for v in other.losses])      # the drawn rows ARE the batches


def test_selection_is_tilted_toward_large_residuals(pa, tier):
    torch.manual_seed(2)
    _, solver = make_solver('cfg2', pa, **tier.solver_kwargs)              # untrained
    sampler = pa.ResidualSampler(pool=4, power=2, floor=0.0, seed=1)
    sampler.bind_solver(solver)
    xs = sampler.sample_device(1024, solver.device)
    assert xs.shape == (1024, 2) and sampler.last_pool.shape == (4096, 2)
    r = sampler.last_residual.abs().cpu().numpy().astype(np.float64)
    drawn = r[sampler.last_indices.cpu().numpy()]
    print('mean |r| of the pool', r.mean(), 'of the batch', drawn.mean())
    assert drawn.mean() >= r.mean()
    assert sampler.sample(16).shape == (16, 2) and sampler.evaluations == 2      # the numpy face; another pool size: a fresh pool


def test_sampler_refusals(pa):
    """ host-side argument checks: no kernel runs, hence no device twin """
    with pytest.raises(ValueError, match='pool'):
        pa.ResidualSampler(pool=0)
    with pytest.raises(ValueError, match='period'):
        pa.ResidualSampler(period=0)
    with pytest.raises(ValueError, match='power'):
        pa.ResidualSampler(power=3)
    with pytest.raises(ValueError, match='floor'):
        pa.ResidualSampler(floor=-1.0)
    with pytest.raises(ValueError, match='floor'):
        pa.ResidualSampler(floor=1e200)
    assert pa.ResidualSampler(pool=np.int64(3), period=np.int32(2)).pool == 3
    with pytest.raises(RuntimeError, match='Solver.fit'):
        pa.ResidualSampler().sample(10)
    assert pa.ResidualSampler().columns() is None
    import pydens
    assert pydens.ResidualSampler is pa.ResidualSampler


_NO_SAMPLER_SCRIPT = '''
import ctypes, os, sys
import numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r}); sys.path.insert(0, os.path.join({tests!r}, 'emu'))
import pydens_amd as pa
from pydens_amd import engine
from conftest import Golden
from helpers import load_params, make_solver
kw = {{}}
if {tier!r} == 'emu':
    import build_emu
    kw = dict(_lib=engine.bind(ctypes.CDLL(build_emu.build())), device='cpu')
g = Golden('cfg2')
out = []
if {bound!r}:
    # a ResidualSampler has been constructed, bound to a solver of this process and used in a fit before the plain fits
    torch.manual_seed(1)
    _, first = make_solver('cfg2', pa, **kw)
    first.fit(1, 16, sampler=pa.ResidualSampler(pool=2, seed=1))
for sampler in (None, pa.NumpySampler('uniform', seed=4) & pa.NumpySampler('uniform', low=0.2, high=0.9, seed=5)):
    torch.manual_seed(9)
    _, solver = make_solver('cfg2', pa, **kw)
    load_params(solver, g.params)
    solver.fit(2, 40, sampler=sampler, lr=g.lr)
    out.append([float(v) for v in solver.losses])
np.save({out!r}, np.array(out))
'''


def test_fits_without_a_residual_sampler_are_untouched(tier):
    """ sampler=None and a NumpySampler product: the same losses, bit for bit, from a process in which a ResidualSampler was bound and
    used beforehand and from one in which none was ever constructed (the parent commit's path: fit chunks, the Philox batches). Two
    child processes: "before ResidualSampler is ever bound" is a statement about a process. """
    with tempfile.TemporaryDirectory() as tmp:
        results = []
        for bound in (False, True):
            out = os.path.join(tmp, f'losses{int(bound)}.npy')
            script = os.path.join(tmp, f'run{int(bound)}.py')
            with open(script, 'w') as f:
                f.write(_NO_SAMPLER_SCRIPT.format(root=os.path.dirname(HERE), tests=HERE, tier=tier.name, bound=bound, out=out))
            import subprocess
            res = subprocess.run([sys.executable, script], capture_output=True, text=True)
            assert res.returncode == 0, res.stdout + res.stderr
            results.append(np.load(out))
        assert results[0].shape == (2, 2) and np.array_equal(results[0], results[1])
        assert not np.array_equal(results[0][0], results[0][1])


# ---- data parallelism: every rank draws from its own pool -------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _dp_worker(rank, world, port, out_dir):
    sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.join(HERE, 'emu'))
    import torch.distributed as dist
    import build_emu
    import pydens_amd as pa
    from pydens_amd import engine
    torch.set_num_threads(1)
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    lib = engine.bind(ctypes.CDLL(build_emu.build()))
    torch.manual_seed(100 + rank)                    # the ranks start from different nets: fit broadcasts rank 0's
    _, solver = make_solver('cfg1', pa, _lib=lib, device='cpu')
    sampler = _recording(pa)(pool=4, period=2, seed=3)
    solver.fit(4, 128, sampler=sampler, lr=0.005)
    np.savez(os.path.join(out_dir, f'rank{rank}.npz'), batches=np.stack(sampler.batches), evaluations=sampler.evaluations,
             pool=sampler.last_pool.numpy(), losses=np.array([float(v) for v in solver.losses]),
             **{f'p{i}': p for i, p in enumerate(export_params(solver))})
    dist.destroy_process_group()


def test_two_ranks_draw_their_own_batches_and_stay_in_step():
    """ gloo, two ranks on the emulator, in the style of test_data_parallel.py and on its net (cfg1: the config-2 equation on the small
    10-12-15 net -- what is checked is the sampler under data parallelism, and the emulator's cost grows with the net). No device twin:
    the device tier has one GPU per test process. """
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_dp_worker, args=(2, _free_port(), tmp), nprocs=2, join=True)
        a, b = (np.load(os.path.join(tmp, f'rank{rank}.npz')) for rank in range(2))
        assert a['batches'].shape == b['batches'].shape == (4, 64, 2)            # the local share of the global batch of 128
        assert a['pool'].shape == (256, 2) and int(a['evaluations']) == int(b['evaluations']) == 2
        assert not np.array_equal(a['batches'], b['batches']) and not np.array_equal(a['pool'], b['pool'])
        assert np.array_equal(a['losses'], b['losses'])
        for i in range(len([k for k in a.files if k[0] == 'p' and k[1:].isdigit()])):
            assert np.array_equal(a[f'p{i}'], b[f'p{i}']), i
