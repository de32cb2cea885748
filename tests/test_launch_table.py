""" Which kernel does every shape get? (pydens_amd/csrc/pinn_inst.inc: the dispatch of the tile and weight-gradient launchers)

A wrong variant bit or a reordered branch in the launchers yields a slower kernel that still computes the right numbers, which no numerical
test notices. Here a list of small cases -- one step each, at most 48 points (one tile of the tallest tile height) -- records the
instantiation names (`pinn_last_kernel_name`, `pinn_last_wgrad_kernel_name`) and threads / LDS bytes of `pinn_last_launch_info`, and compares
them EXACTLY with launch_table_expected.json beside this file. The file's header names the commit whose launchers produced it
(`python tests/test_launch_table.py --write` on the emulator); a change that means to move a shape to another kernel regenerates it and says so.

Three kinds of cases: `net` drives pinn_jet_backward of a bare net with (nd, n2) directly (the general, breadth and second-set kernels and
their weight-gradient partners); `solver` runs one fused step of a problem (combined streams, shape specialisations, GEMM / tanh modes);
`fit` runs a one-iteration fit chunk in its one-CU or its grid form. The same list runs on the emulator and, marked gpu, on the device (grid
and workgroups per CU depend on the machine and are not compared). """
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import pinn_configs as pc

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'emu'))
EXPECTED = os.path.join(HERE, 'launch_table_expected.json')
PI = float(np.pi)
N_POINTS = 40           # three 16-point tiles, the last one ragged; one tile of the 48-point kernels


def _net_cases():
    """ id -> (hidden widths, activation, skips, nd, n2): pinn_jet_backward of the bare net """
    keys = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 2), (3, 2), (4, 0), (3, 3), (1, 9), (2, 9), (1, 73)]
    out = {}
    for nd, n2 in keys:                                          # width 32: no static-depth kernels in the way
        out[f'plain32-{nd}-{n2}'] = ([24, 24], 'tanh', (), nd, n2)
        out[f'sin32-{nd}-{n2}'] = ([24, 24], 'sin', (), nd, n2)
    for nd, n2 in [(0, 0), (1, 0), (1, 1), (2, 0), (2, 2), (1, 9), (1, 73)]:     # second set (activation codes above 7)
        out[f'elu32-{nd}-{n2}'] = ([24, 24], 'elu', (), nd, n2)
    for nd, n2 in [(1, 1), (2, 2), (2, 0)]:                      # skips over Tanh layers: the light kernels for the two commonest shapes
        out[f'skip32-{nd}-{n2}'] = ([24, 24, 24], 'tanh', ((0, 2),), nd, n2)
    out['nested32-1-1'] = ([24] * 5, 'tanh', ((0, 4), (1, 3)), 1, 1)
    out['plain16-1-0'] = ([12, 12], 'tanh', (), 1, 0)
    out['fast16-2-2'] = ([12, 12, 12], 'tanh', (), 2, 2)
    for depth, shapes in ((4, [(2, 2), (1, 0), (1, 1)]), (3, [(1, 0)]), (5, [(1, 0)])):
        for nd, n2 in shapes:
            out[f'fast64x{depth}-{nd}-{n2}'] = ([48] * depth, 'tanh', (), nd, n2)
    out['plain64-3-2'] = ([48] * 4, 'tanh', (), 3, 2)
    out['sigmoid64-2-2'] = ([48] * 4, 'sigmoid', (), 2, 2)
    for nd, n2 in [(2, 2), (1, 1), (3, 3), (1, 9)]:              # streamed widths: tile kernel + weight-gradient partner
        out[f'plain128-{nd}-{n2}'] = ([96, 96, 96], 'tanh', (), nd, n2)
    out['sin128-2-2'] = ([96, 96, 96], 'sin', (), 2, 2)
    out['sin128-1-73'] = ([96, 96, 96], 'sin', (), 1, 73)
    out['elu128-2-2'] = ([96, 96, 96], 'elu', (), 2, 2)
    out['skip128-1-1'] = ([96, 96, 96], 'tanh', ((0, 2),), 1, 1)
    out['skip128-2-2'] = ([96, 96, 96], 'tanh', ((0, 2),), 2, 2)
    out['skip128-2-0'] = ([96, 96, 96], 'tanh', ((0, 2),), 2, 0)
    out['plain256-1-1'] = ([200, 200], 'tanh', (), 1, 1)
    out['elu256-1-1'] = ([200, 200], 'elu', (), 1, 1)
    out['plain512-1-1'] = ([300, 300], 'tanh', (), 1, 1)
    out['sin512-2-0'] = ([300, 300], 'sin', (), 2, 0)
    return out


def _problem(name, D, V):
    """ problems beside those of pinn_configs: (equation, solver keywords) """
    lap2 = lambda f, x, y: D(D(f, x), x) + D(D(f, y), y) - 5 * torch.sin(PI * (x + y))
    heat = lambda f, x, y, t: D(D(f, x), x) + D(D(f, y), y) - D(f, t)
    box = dict(ndims=2, boundary_condition=1)
    evo3 = dict(ndims=3, boundary_condition=0, initial_condition=lambda x, y: 10 * x * y * (1 - x) * (1 - y))
    net = lambda widths, act, layout=None: dict(layout=layout or ('fa ' * len(widths) + 'f'), features=list(widths) + [1], activation=act)
    table = {
        'cfg3_sigmoid': (heat, dict(**evo3, **net([128] * 5, 'Sigmoid'))),
        'cfg5_sigmoid': (lambda f, x, t: D(D(f, t), t) - D(D(f, x), x),
                         dict(ndims=2, boundary_condition=0, initial_condition=lambda x: x * (1 - x), **net([256] * 6, 'Sigmoid'))),
        'sin64_program': (lambda f, x, y: D(D(f, x), x) + D(D(f, y), y) + 1.5 * f * f - 5 * torch.sin(PI * (x + y)), dict(**box, **net([64] * 4, 'Sin'))),
        'skip128_sigmoid': (lap2, dict(**box, **net([128] * 4, 'Sigmoid', 'faR fa fa+ fa f'))),
        'skip32_box': (lap2, dict(**box, **net([24] * 4, 'Tanh', 'faR fa fa+ fa f'))),
        'skip32_heat': (heat, dict(**evo3, **net([24] * 4, 'Tanh', 'faR fa fa+ fa f'))),
        'skip128_heat': (heat, dict(**evo3, **net([96] * 4, 'Tanh', 'faR fa fa+ fa f'))),
        'silu32_box': (lap2, dict(**box, **net([24] * 3, 'SiLU'))),
        'silu32_heat': (heat, dict(**evo3, **net([24] * 3, 'SiLU'))),
        'silu32_heat3d': (lambda f, x, y, z, t: D(D(f, x), x) + D(D(f, y), y) + D(D(f, z), z) - D(f, t),
                          dict(ndims=4, boundary_condition=0, initial_condition=lambda x, y, z: x * y * z, **net([24] * 3, 'SiLU'))),
        'elu32_box': (lap2, dict(**box, **net([24] * 3, 'ELU'))),
        'elu128_box': (lap2, dict(**box, **net([96] * 3, 'ELU'))),
        'gelu128_box': (lap2, dict(**box, **net([128] * 4, 'GELU'))),
        'plain32_box': (lap2, dict(**box, **net([24] * 3, 'Tanh'))),
        'plain32_heat': (heat, dict(**evo3, **net([24] * 3, 'Tanh'))),
        'plain128_box': (lap2, dict(**box, **net([128] * 4, 'Tanh'))),
        'box64x3': (lap2, dict(**box, **net([64] * 3, 'Tanh'))),
        'box64x5': (lap2, dict(**box, **net([64] * 5, 'Tanh'))),
        'heat64x4': (heat, dict(**evo3, **net([64] * 4, 'Tanh'))),
        'box64_with_parameter': (lambda f, x, y, e: D(D(f, x), x) + D(D(f, y), y) - e * torch.sin(PI * (x + y)),
                                 dict(ndims=2, nparams=1, boundary_condition=1, **net([64] * 4, 'Tanh'))),
        'box16_with_parameter': (lambda f, x, y, e: D(D(f, x), x) + D(D(f, y), y) - e * torch.sin(PI * (x + y)),
                                 dict(ndims=2, nparams=1, boundary_condition=1, **net([10, 12, 15], 'Tanh'))),
    }
    return table[name]


# id -> (problem: a name of pinn_configs or of _problem, gemm mode, tanh mode)
SOLVER_CASES = {name: (name, None, None) for name in
                ('cfg1', 'cfg2', 'cfg3', 'cfg4', 'cfg5', 'program', 'heat64', 'burgers64', 'sin64', 'sin128', 'skip128', 'skip256', 'gelu256', 'heat3d',
                 'cfg3_sigmoid', 'cfg5_sigmoid', 'sin64_program', 'skip128_sigmoid', 'skip32_box', 'skip32_heat', 'skip128_heat', 'silu32_box', 'silu32_heat',
                 'silu32_heat3d', 'elu32_box', 'elu128_box', 'gelu128_box', 'plain32_box', 'plain32_heat', 'plain128_box', 'box64x3', 'box64x5',
                 'heat64x4', 'box64_with_parameter', 'box16_with_parameter')}
SOLVER_CASES.update({f'{name}-bf16x3': (name, 'bf16x3', None) for name in ('cfg2', 'cfg3', 'cfg4', 'cfg5')})
SOLVER_CASES['cfg2-accurate_tanh'] = ('cfg2', None, 'accurate')
# id -> (hidden widths, PYDENS_AMD_FIT_PERSIST, batch): the grid form runs on ONE workgroup in the emulator, hence one tile
FIT_CASES = {'fit16-onecu': ([16, 16], 2, N_POINTS), 'fit16-grid': ([16, 16], 1, 16), 'fit32-onecu': ([32, 32], 2, N_POINTS), 'fit32-grid': ([32, 32], 1, 16)}
NET_CASES = _net_cases()
# a step of these takes more than ten seconds on the emulator (measured: see the expected file's header): device list only
GPU_ONLY = ('cfg5', 'cfg5_sigmoid', 'cfg5-bf16x3', 'skip256', 'gelu256', 'plain512-1-1', 'sin512-2-0')
ALL = [('net', k) for k in NET_CASES] + [('solver', k) for k in SOLVER_CASES] + [('fit', k) for k in FIT_CASES]


def _launch_info(lib):
    info = (ctypes.c_int32 * 4)()
    assert lib.pinn_last_launch_info(info) == 0
    return [int(info[2]), int(info[3])]             # threads, LDS bytes ([0], [1]: grid and workgroups per CU follow the machine)


def _record(lib, hp, wgrad):
    """ (the weight-gradient name is a process-wide 'last': it belongs to this case only where the step streams its weight gradients) """
    threads, lds = _launch_info(lib)
    return dict(kernel=lib.pinn_last_kernel_name().decode(), wgrad=lib.pinn_last_wgrad_kernel_name().decode() if (wgrad and hp >= 128) else '',
                threads=threads, lds_bytes=lds)


def _run_net(pa, lib, device, case):
    widths, act, skips, nd, n2 = NET_CASES[case]
    net = pa.engine.Net([4] + list(widths) + [1], act, 4, lib=lib, skips=skips)
    rng = np.random.RandomState(11)
    flat = torch.zeros(net.layout.p_total, dtype=torch.float32)
    for w, b in net.param_views(flat):
        w.copy_(torch.as_tensor(rng.randn(*w.shape).astype(np.float32) * 0.3))
        b.copy_(torch.as_tensor(rng.randn(*b.shape).astype(np.float32) * 0.3))
    xs = torch.as_tensor(rng.rand(N_POINTS, 4).astype(np.float32)).to(device)
    flat = flat.to(device)
    s = 1 + nd + (n2 & 7) + ((n2 >> 3) & 7) + (n2 >> 6)
    gin = torch.full((s, N_POINTS), 1.0 / N_POINTS, dtype=torch.float32, device=device)
    grads = torch.zeros_like(flat)
    ws = torch.zeros((net.workspace_bytes(N_POINTS, nd, n2) + 3) // 4 + 4, dtype=torch.float32, device=device)
    net.jet_backward(flat, xs, gin, grads, ws, tuple(range(nd)), n2)
    return _record(lib, net.layout.hp, net.layout.lh > 0)


def _run_solver(pa, lib, extra, case):
    name, gemm, tanh = SOLVER_CASES[case]
    try:
        cfg = pc.make_config(name, pa.D, torch, V=pa.V)
        eq, kw = cfg['equation'], cfg['solver_kwargs']
    except KeyError:
        eq, kw = _problem(name, pa.D, pa.V)
    torch.manual_seed(3)
    solver = pa.Solver(eq, **kw, **extra)
    if gemm is not None:
        solver.set_gemm_mode(gemm)
    if tanh is not None:
        solver.set_tanh_mode(tanh)
    assert solver.program is not None, solver.program_error
    total = solver.model.total
    pts = torch.as_tensor(np.random.RandomState(5).rand(N_POINTS, total).astype(np.float32)).to(solver.device)
    solver._fused_step(pts, 1)
    lay = solver.model.net.layout
    return _record(lib, lay.hp, lay.lh > 0)


def _run_fit(pa, lib, extra, case, monkeypatch):
    widths, persist, batch = FIT_CASES[case]
    monkeypatch.setenv('PYDENS_AMD_FIT_PERSIST', str(persist))
    monkeypatch.setenv('PYDENS_AMD_FIT_ROUNDS', '4')
    monkeypatch.setenv('PYDENS_AMD_FIT_GRAPH', '1')
    if extra:
        monkeypatch.setattr(pa.Solver, 'FIT_CTRL_ON_HOST', True)
    eq = lambda f, x: pa.D(f, x) - 2 * PI * torch.cos(2 * PI * x)
    torch.manual_seed(3)
    solver = pa.Solver(eq, ndims=1, initial_condition=0.5, layout='fa fa f', features=list(widths) + [1], activation='Tanh', **extra)
    solver.fit(niters=1, batch_size=batch, sampler=pa.NumpySampler('uniform', seed=5, low=0.0, high=1.0), lr=0.005)
    assert solver.last_fit_path == 'fused', solver.program_error
    return _record(lib, solver.model.net.layout.hp, False)


def run_case(pa, lib, extra, kind, case, monkeypatch):
    if kind == 'net':
        return _run_net(pa, lib, extra.get('device', 'cuda'), case)
    if kind == 'solver':
        return _run_solver(pa, lib, extra, case)
    return _run_fit(pa, lib, extra, case, monkeypatch)


@pytest.fixture(scope='module')
def expected():
    with open(EXPECTED) as f:
        return json.load(f)['cases']


@pytest.fixture(scope='module')
def pa():
    import pydens_amd
    return pydens_amd


@pytest.fixture(scope='module')
def emu_lib(pa):
    import build_emu
    lib = pa.engine.bind(ctypes.CDLL(build_emu.build()))
    assert lib.pinn_backend() == b'emu-host'
    return lib


def test_the_expected_file_covers_the_list(expected):
    assert sorted(expected) == sorted(f'{kind}/{case}' for kind, case in ALL)


@pytest.mark.parametrize('kind,case', [c for c in ALL if c[1] not in GPU_ONLY], ids=lambda v: v)
def test_every_shape_gets_its_kernel_on_the_emulator(pa, emu_lib, expected, monkeypatch, kind, case):
    got = run_case(pa, emu_lib, dict(_lib=emu_lib, device='cpu'), kind, case, monkeypatch)
    assert got == expected[f'{kind}/{case}'], (kind, case)


@pytest.mark.gpu
@pytest.mark.parametrize('kind,case', ALL, ids=lambda v: v)
def test_every_shape_gets_its_kernel_on_the_gpu(pa, expected, monkeypatch, kind, case):
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    lib = pa.engine.load_library()
    assert lib.pinn_backend() == b'hip-gfx950'
    got = run_case(pa, lib, {}, kind, case, monkeypatch)
    assert got == expected[f'{kind}/{case}'], (kind, case)


if __name__ == '__main__':
    # regenerate the expected file on the emulator: python tests/test_launch_table.py --write <commit>
    import time
    import build_emu
    import pydens_amd as pa_
    assert sys.argv[1] == '--write' and len(sys.argv) == 3
    lib_ = pa_.engine.bind(ctypes.CDLL(build_emu.build()))
    mp = pytest.MonkeyPatch()
    cases, slow = {}, {}
    for kind_, case_ in ALL:
        t0 = time.time()
        cases[f'{kind_}/{case_}'] = run_case(pa_, lib_, dict(_lib=lib_, device='cpu'), kind_, case_, mp)
        if time.time() - t0 > 5.0:
            slow[f'{kind_}/{case_}'] = round(time.time() - t0, 1)
        print(f'{kind_}/{case_}', round(time.time() - t0, 2), cases[f'{kind_}/{case_}'], flush=True)
    mp.undo()
    with open(EXPECTED, 'w') as f:
        json.dump({'header': f'kernel names, threads and LDS bytes per case as the launchers of commit {sys.argv[2]} chose them (emulator build; '
                             'tests/test_launch_table.py --write)', 'emulator_seconds_above_5': slow, 'cases': cases}, f, indent=1, sort_keys=True)
