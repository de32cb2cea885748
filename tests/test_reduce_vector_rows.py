""" The launch behind the tile kernel (pinn_reduce_kernel: sum of the per-workgroup partial rows, optimizer update, loss slot, next batch)
with 16-byte row loads. Synthetic rows through the C-ABI (pinn_reduce_rows -> launch_reduce); the expected gradients are a numpy
restatement of the order of the sums -- chunk c = rows c, c + 32, c + 64, ... ascending in float64, the 32 chunk sums ascending in
float64, the old gradient last, ONE rounding -- compared BIT FOR BIT; the updated parameters and state bit for bit against the
standalone update kernel (pinn_optim_step_at: the same pinn_optim_apply) on those gradients. Emulator build; `-m gpu` twins. """
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

from helpers import make_solver

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))

CH = 32                                             # chunks of rows: part of the result (pinn_aux_kernels.h PINN_REDUCE_CH)
CFG2_P_TOTAL = 64 * 2 + 64 + 3 * (64 * 64 + 64) + 64 + 4 + 16        # BASELINE config 2's net (2 -> 4 x 64 -> 1): 12 756
N_ROWS = (1, 7, 32, 33, 256, 300)                   # below one chunk round, no multiple of CH, no multiple of 8 CH
ROW_LENS = (4, 36, 132, 35, CFG2_P_TOTAL)           # 35: rows that are not 16-byte pieces -> the scalar form
LR, STEP = 0.01, 3


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


def _gpu_lib(pa):
    return pa.engine.load_library()


def _adam(pa):
    from pydens_amd.solver import FlatOptimizer
    return pa.engine.Optim.build(FlatOptimizer.RULES['Adam'][0], **FlatOptimizer.hyper('Adam', LR, {}))


def expected_sum(rows, g_old=None):
    """ the order of pinn_reduce_kernel (and of pinn_fit_kernel's sweep (d)) in numpy: float64 adds, one rounding to float32 """
    r64 = rows.astype(np.float64)
    t = np.zeros(rows.shape[1], dtype=np.float64)
    for c in range(CH):
        s = np.zeros(rows.shape[1], dtype=np.float64)
        for w in range(c, rows.shape[0], CH):
            s = s + r64[w]
        t = t + s
    if g_old is not None:
        t = t + g_old.astype(np.float64)
    return t.astype(np.float32)


_ROWS = {}


def _rows(n, p):
    """ the synthetic partial rows of a case and their expected sums: made once, shared, never written to """
    if (n, p) not in _ROWS:
        rng = np.random.default_rng(1000 * n + p)
        rows = (rng.standard_normal((n, p)) * np.exp(rng.uniform(-6.0, 6.0, (n, p)))).astype(np.float32)
        g_old = rng.standard_normal(p).astype(np.float32)
        for a in (rows, g_old):
            a.setflags(write=False)
        _ROWS[(n, p)] = (rows, g_old, expected_sum(rows), expected_sum(rows, g_old))
    return _ROWS[(n, p)]


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _reduce(pa, lib, rows_t, n, p, grads, accumulate, state=None, mask=None, step=None, optim=None, loss=None, off_loss=0):
    params, m, v = state if state is not None else (None, None, None)
    rc = lib.pinn_reduce_rows(_ptr(rows_t), n, p, _ptr(grads), int(accumulate), _ptr(params), _ptr(m), _ptr(v), _ptr(mask), _ptr(step),
                              STEP, ctypes.byref(optim) if optim is not None else None, _ptr(loss), off_loss, pa.engine.stream_of(grads))
    assert rc == 0, lib.pinn_last_error().decode()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _grid_case(pa, lib, device, n, p):
    rows, g_old, want, want_acc = _rows(n, p)
    rows_t = torch.from_numpy(rows.copy()).to(device)
    optim = _adam(pa)
    rng = np.random.default_rng(7)
    start = [torch.from_numpy(rng.standard_normal(p).astype(np.float32)).to(device),
             torch.from_numpy((0.1 * rng.standard_normal(p)).astype(np.float32)).to(device),
             torch.from_numpy((0.01 * rng.random(p)).astype(np.float32)).to(device)]
    some = torch.ones(p, dtype=torch.uint8, device=device)
    some[::3] = 0
    off_loss = p - 2
    form = 'pinn_reduce_kernel' if p % 4 == 0 else 'pinn_reduce_scalar_kernel'
    for accumulate in (0, 1):
        exp = want_acc if accumulate else want
        for mode in ('sum', 'adam', 'adam+mask'):
            grads = torch.from_numpy(g_old.copy()).to(device)
            if mode == 'sum':
                _reduce(pa, lib, rows_t, n, p, grads, accumulate)
                assert lib.pinn_last_reduce_kernel_name().decode() == form
                assert np.array_equal(_bits(grads), exp.view(np.uint32)), (n, p, accumulate, mode)
                continue
            mask = some if mode == 'adam+mask' else None
            got = [t.clone() for t in start]
            step = torch.zeros(1, dtype=torch.int32, device=device)
            loss = torch.full((1,), -1.0, device=device)
            _reduce(pa, lib, rows_t, n, p, grads, accumulate, got, mask, step, optim, loss, off_loss)
            assert lib.pinn_last_reduce_kernel_name().decode() == form
            assert np.array_equal(_bits(grads), exp.view(np.uint32)), (n, p, accumulate, mode)
            assert np.array_equal(_bits(loss), exp[off_loss:off_loss + 1].view(np.uint32)), (n, p, accumulate, mode)
            assert int(step) == STEP
            # the standalone update kernel on the expected gradients: the same pinn_optim_apply with the same host-side scalars
            ref = [t.clone() for t in start]
            rstep = torch.zeros(1, dtype=torch.int32, device=device)
            exp_t = torch.from_numpy(exp.copy()).to(device)
            rc = lib.pinn_optim_step_at(_ptr(ref[0]), _ptr(exp_t), _ptr(ref[1]), _ptr(ref[2]), _ptr(mask), p, _ptr(rstep), STEP,
                                        ctypes.byref(optim), None, 0, pa.engine.stream_of(grads))
            assert rc == 0, lib.pinn_last_error().decode()
            for a, b, what in zip(got, ref, ('param', 'm', 'v')):
                assert np.array_equal(_bits(a), _bits(b)), (n, p, accumulate, mode, what)
            if mask is not None:
                dead = ~mask.bool()
                for a, b in zip(got, start):
                    assert torch.equal(a[dead], b[dead])
            else:
                assert not torch.equal(got[0], start[0])
    assert np.array_equal(_bits(rows_t), rows.view(np.uint32))          # the rows are read, never written


@pytest.mark.parametrize('p', ROW_LENS)
@pytest.mark.parametrize('n', N_ROWS)
def test_sums_and_update_bit_for_bit(pa, emu_lib, n, p):
    _grid_case(pa, emu_lib, 'cpu', n, p)


@pytest.mark.gpu
@pytest.mark.parametrize('p', ROW_LENS)
@pytest.mark.parametrize('n', N_ROWS)
def test_sums_and_update_bit_for_bit_on_the_gpu(pa, n, p):
    _grid_case(pa, _gpu_lib(pa), 'cuda', n, p)


def _misaligned_case(pa, lib, device):
    """ rows of 36 floats that start 4 bytes off a 16-byte boundary: the launcher must take the scalar form, same sums """
    n, p = 33, 36
    rows, _, want, _ = _rows(n, p)
    buf = torch.zeros(n * p + 4, dtype=torch.float32, device=device)
    shifted = buf[1:1 + n * p]
    shifted.copy_(torch.from_numpy(rows.reshape(-1).copy()))
    assert shifted.data_ptr() % 16 == 4
    grads = torch.zeros(p, device=device)
    _reduce(pa, lib, shifted, n, p, grads, 0)
    assert lib.pinn_last_reduce_kernel_name().decode() == 'pinn_reduce_scalar_kernel'
    assert np.array_equal(_bits(grads), want.view(np.uint32))


def test_rows_off_a_16_byte_boundary_take_the_scalar_form(pa, emu_lib):
    _misaligned_case(pa, emu_lib, 'cpu')


@pytest.mark.gpu
def test_rows_off_a_16_byte_boundary_take_the_scalar_form_on_the_gpu(pa):
    _misaligned_case(pa, _gpu_lib(pa), 'cuda')


def _cancelling_case(pa, lib, device):
    """ entries whose terms cancel: sum of |terms| about 1e3 x |sum| (tools/cfg4_bl_probe.py: BASELINE config 4's d loss / d b_L). With
    the sums in double the result is the correctly rounded exact sum -- the 255 double adds err by 255 x 2^-53 of the largest prefix,
    1e3 x 255 x 1.1e-16 = 3e-11 of the result, against float32's half ulp of 6e-8: bound 2^-24 (1 + 1e-3). The same order in float32
    misses that bound, which is what this row set is for. """
    n, p = 256, 132
    rng = np.random.default_rng(5)
    terms = rng.standard_normal((n, p))
    terms -= terms.mean(axis=0)
    terms += np.abs(terms).sum(axis=0) * 1e-3 / n * np.where(rng.random(p) < 0.5, -1.0, 1.0)
    rows = terms.astype(np.float32)
    exact = np.array([math.fsum(rows[:, i].astype(np.float64)) for i in range(p)])
    ratio = np.abs(rows.astype(np.float64)).sum(axis=0) / np.abs(exact)
    print(f'sum |terms| / |sum|: {ratio.min():.0f} .. {ratio.max():.0f}')
    assert ratio.min() > 300
    grads = torch.zeros(p, device=device)
    _reduce(pa, lib, torch.from_numpy(rows.copy()).to(device), n, p, grads, 0)
    got = grads.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), expected_sum(rows).view(np.uint32))
    err = np.abs(got.astype(np.float64) - exact) / np.abs(exact)
    s32 = np.zeros(p, dtype=np.float32)                     # the same order with float32 adds
    for c in range(CH):
        s = np.zeros(p, dtype=np.float32)
        for w in range(c, n, CH):
            s = s + rows[w]
        s32 = s32 + s
    err32 = np.abs(s32.astype(np.float64) - exact) / np.abs(exact)
    print(f'relative error of the sums: {err.max():.3e} (float32 adds in the same order: {err32.max():.3e})')
    bound = 2.0 ** -24 * (1 + 1e-3)
    assert err.max() <= bound
    assert err32.max() > 10 * bound


def test_cancelling_rows_keep_the_double_sums(pa, emu_lib):
    _cancelling_case(pa, emu_lib, 'cpu')


@pytest.mark.gpu
def test_cancelling_rows_keep_the_double_sums_on_the_gpu(pa):
    _cancelling_case(pa, _gpu_lib(pa), 'cuda')


BATCH, NITERS = 700, 5          # more points than one block of the reduction has threads: the tail's loop has to stride by the launch's own shape


def _next_batch_case(pa, lib, extra, monkeypatch):
    """ config 1 through the chunk entry point (pinn_fit_steps: from the second iteration on the reduction's tail draws the batch) against
    the per-iteration loop (pinn_sample_points + pinn_residual_optim_step): the same trajectory, and the batch left in the buffer is the
    one pinn_sample_kernel draws for that call """
    monkeypatch.setenv('PYDENS_AMD_FIT_GRAPH', '0')
    monkeypatch.setenv('PYDENS_AMD_FIT_PERSIST', '0')          # (the tile kernel + reduction form, not the one-launch chunk)
    runs = []
    for eager in (False, True):
        torch.manual_seed(41)
        _, solver = make_solver('cfg1', pa, **extra)
        if eager:
            solver._device_columns = lambda sampler: None
        solver.fit(niters=NITERS, batch_size=BATCH, lr=0.005)
        assert solver.last_fit_path == 'fused'
        assert lib.pinn_last_reduce_kernel_name().decode() == 'pinn_reduce_kernel'
        runs.append(dict(losses=np.array([float(v) for v in solver.losses], dtype=np.float32), params=solver.model.flat.detach().cpu().numpy().copy(),
                         m=solver.optimizer.exp_avg.cpu().numpy().copy(), v=solver.optimizer.exp_avg_sq.cpu().numpy().copy(), solver=solver))
    chunk, loop = runs
    assert np.isfinite(chunk['losses']).all()
    for key in ('losses', 'params', 'm', 'v'):
        assert np.array_equal(chunk[key].view(np.uint32), loop[key].view(np.uint32)), key
    solver = chunk['solver']
    assert solver._sample_calls == NITERS
    (xs,) = solver._fit_xs.values()
    want = torch.empty_like(xs)
    solver.model.net.sample_points(want, [(pa.engine.SAMPLE_UNIFORM, 0.0, 1.0)] * xs.shape[1], solver._sample_seed, NITERS - 1)
    assert xs.shape[0] == BATCH
    assert np.array_equal(_bits(xs), _bits(want))


def test_next_batch_of_the_reduction_tail(pa, emu_lib, monkeypatch):
    _next_batch_case(pa, emu_lib, dict(_lib=emu_lib, device='cpu'), monkeypatch)


@pytest.mark.gpu
def test_next_batch_of_the_reduction_tail_on_the_gpu(pa, monkeypatch):
    _next_batch_case(pa, _gpu_lib(pa), {}, monkeypatch)
