""" The partial gradient row of the two-team width-64 kernels (BASELINE configs 2 and 4): the teams' sums meet in LDS and leave as one
coalesced row (pinn_kernel.h, PINN_TEAM_ROW_LDS) instead of team 0 storing and team 1 adding on top through global memory. Emulator build,
no GPU: one step at fixed parameters against the fp64 oracle by the rule of bench.parity_check, bit for bit against a build with the
earlier form of the row's end, twice in a row, and under random wave scheduling. """
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import pinn_configs as pc
from helpers import export_grads, export_params, make_solver

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))

CASES = [('cfg2', 100), ('cfg4', 150)]          # (ragged: the last round of a team has an empty tile)


@pytest.fixture(scope='module')
def libs():
    import build_emu
    from pydens_amd import engine
    new = engine.bind(ctypes.CDLL(build_emu.build()))
    old = engine.bind(ctypes.CDLL(build_emu.build(extra_flags=['-DPINN_TEAM_ROW_LDS=0'], tag='rowglobal', widths=(64,))))
    assert new.pinn_backend() == b'emu-host' and old.pinn_backend() == b'emu-host'
    return new, old


@pytest.fixture(scope='module')
def pa():
    import pydens_amd
    return pydens_amd


def _step(pa, lib, name, n):
    torch.manual_seed(0)
    cfg, solver = make_solver(name, pa, _lib=lib, device='cpu')
    pts = pc.sample_points(cfg, n, seed=1)
    solver._fused_step(torch.from_numpy(pts), 1)
    kernel = lib.pinn_last_kernel_name().decode()
    assert int(kernel.rstrip('>').split(',')[-1]) & 256, kernel          # a two-team instantiation
    return solver, pts, solver.grads.clone().numpy()


@pytest.mark.parametrize('name,n', CASES)
def test_row_through_lds_equals_row_through_global_memory_bit_for_bit(pa, libs, name, n):
    new, old = libs
    _, _, g_new = _step(pa, new, name, n)
    _, _, g_old = _step(pa, old, name, n)
    assert np.array_equal(g_new, g_old)


@pytest.mark.parametrize('name,n', CASES)
def test_two_runs_are_bitwise_equal(pa, libs, name, n):
    _, _, a = _step(pa, libs[0], name, n)
    _, _, b = _step(pa, libs[0], name, n)
    assert np.array_equal(a, b)


@pytest.mark.parametrize('name,n', CASES)
def test_result_does_not_depend_on_wave_order(pa, libs, name, n, monkeypatch):
    monkeypatch.delenv('PINN_EMU_SHUFFLE', raising=False)
    _, _, want = _step(pa, libs[0], name, n)
    for seed in (1, 2):
        monkeypatch.setenv('PINN_EMU_SHUFFLE', str(seed))
        _, _, got = _step(pa, libs[0], name, n)
        assert np.array_equal(got, want), seed


@pytest.mark.parametrize('name,n', CASES)
def test_one_step_against_the_fp64_oracle(pa, libs, name, n):
    """ per tensor |ours - f64| <= max(2 |ref32 - f64|, 1e-5 |f64|) (+ the absolute floor of bench.parity_check), L2 norms; loss likewise """
    from oracle import pinn_oracle as po
    solver, pts, _ = _step(pa, libs[0], name, n)
    params = export_params(solver)
    refs = {}
    for dtype in (torch.float32, torch.float64):
        ocfg = pc.make_config(name, po.D, torch, V=po.V)
        oracle = po.OracleSolver(ocfg['equation'], dtype=dtype, **ocfg['solver_kwargs'])
        oracle.import_params(params)
        ev = oracle.evaluate(pts, chunk=2048)
        refs[dtype] = (ev['loss'], oracle.export_grads())
    (l32, g32), (l64, g64) = refs[torch.float32], refs[torch.float64]
    loss = float(solver.grads[solver.model.net.layout.off_loss])
    print(f'{name}: loss ours {loss:.9g} f32 {l32:.9g} f64 {l64:.9g}')
    assert abs(loss - l64) <= max(2 * abs(l32 - l64), 1e-5 * abs(l64))
    for i, (g, a32, a64) in enumerate(zip(export_grads(solver), g32, g64)):
        if a64 is None:
            continue
        a64 = np.asarray(a64, dtype=np.float64)
        err = float(np.linalg.norm(np.asarray(g, dtype=np.float64) - a64))
        ref = float(np.linalg.norm(np.asarray(a32, dtype=np.float64) - a64))
        scale = float(np.linalg.norm(a64))
        print(f'{name}: tensor {i}: |ours - f64| {err:.3e}  |ref32 - f64| {ref:.3e}  |f64| {scale:.3e}')
        assert err <= max(2 * ref, 1e-5 * scale + 1e-9 * np.sqrt(a64.size)), i
