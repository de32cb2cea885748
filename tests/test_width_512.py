""" Hidden widths 257 .. 512 (padded to 512; pinn_launch_tile_hp512 / pinn_launch_wgrad_hp512, round 6) through their own loops: every unit,
every 256 x 256 block pass of the weight-gradient kernel, eight bias-gradient rows, the tile loop, ragged tiles, every stream shape in both
kernel forms, chunked slabs, direction groups, predict / residual, and the host's refusals at this width.

Reference and rule (one for the whole file): every case builds oracle.pinn_oracle.OracleSolver twice from one fp32 start (fp32 and fp64),
loads that start into pa.Solver and runs ONE _fused_step / _generic_step. The loss (1e-5, no floor) and the gradient of every parameter
tensor (helpers.GRAD_RTOL, floor 1e-9 per entry) go through helpers.close_or_arbitrated, k = 2 against fp64 -- and so does every 256-aligned
block of every hidden->hidden matrix with a side above 256 (the four block passes of pinn_wgrad_kernel at NBLK = 2 write exactly these), so
that an error confined to one block pass cannot hide in the L2 norm of the others. A tensor or block whose fp64 norm sits below its floor
1e-9 sqrt(size) would pass vacuously: there is none (test_no_reference_gradient_sits_at_the_floor on the CPU tier, and again in every
device case). The oracles are computed once per case (_reference) and shared, unchanged, by the tests that need them.
Kernel cases are marked gpu; the emulator twins (one or two tiles) need PYDENS_AMD_SLOW_EMU=1 like test_hidden_width_512_matches_the_oracle;
the host-only tests run on the CPU tier. """
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import rel_l2
from helpers import (GRAD_RTOL, FixedBatches, close_or_arbitrated, export_grads, fit_close, load_params, ran_split_kernel, record_margin)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))

gpu = pytest.mark.gpu
slow_emu = pytest.mark.skipif(os.environ.get('PYDENS_AMD_SLOW_EMU') != '1',
                              reason='a 512-wide tile costs the emulator a minute or more: PYDENS_AMD_SLOW_EMU=1, or the -m gpu twin')
LOSS_RTOL = 1e-5
HB = 256                    # PinnWgCfg<512>::HB: side of one block pass


@pytest.fixture(scope='module')
def pa():
    import pydens_amd
    return pydens_amd


@pytest.fixture(scope='module')
def dev(pa):
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    from pydens_amd import engine
    lib = engine.load_library()
    assert lib.pinn_backend() == b'hip-gfx950'
    return lib


@pytest.fixture(scope='module')
def emu_lib():
    import build_emu
    from pydens_amd import engine
    lib = engine.bind(ctypes.CDLL(build_emu.build()))
    assert lib.pinn_backend() == b'emu-host'
    return lib


# ---- the problems ----------------------------------------------------------------------------------------------------------------------
def _eq(shape):
    """ equation of a stream shape (nd, n2) as a function of D: the four shapes pinn_launch_tile_hp512 dispatches """
    if shape == (0, 0):
        return lambda D: (lambda u, x: u - torch.sin(3.0 * x)), 1
    if shape == (1, 0):
        return lambda D: (lambda u, x: D(u, x) - u), 1
    if shape == (1, 1):
        return lambda D: (lambda f, x: D(D(f, x), x) + f - torch.sin(3.0 * x)), 1
    assert shape == (2, 0)
    return lambda D: (lambda f, x, y: D(f, x) + 0.5 * D(f, y) - f * f), 2


def _problem(shape, layout, features, activation, bc=0.2):
    eq_of, ndims = _eq(shape)
    return lambda D: (eq_of(D), dict(ndims=ndims, boundary_condition=bc, layout=layout, features=list(features), activation=activation))


def _plain(shape, width, depth, act='Tanh'):
    return _problem(shape, 'fa' * depth + 'f', [width] * depth + [1], act)


# first breadth set at width 320 (activation codes 0 .. 7, one skip), one net per stream shape: identity ('f f'), a pre-activation skip with
# ReLU on the FIRST layer (its pre-activations w x + b are spread over O(1): the 320 x 53 of them can stay clear of the kink), a
# post-activation skip, and the remaining activations
BREADTH = {
    (0, 0): dict(layout='fa f fa f', features=[320, 320, 320, 1], activation=['Sin', 'Tanh']),
    (1, 0): dict(layout='fRa fa f+a f', features=[320, 320, 320, 1], activation=['ReLU', 'SiLU', 'GELU']),
    (1, 1): dict(layout='faR fa fa+ f', features=[320, 320, 320, 1], activation=['Sigmoid', 'Sin', 'Softplus']),
    (2, 0): dict(layout='fa fa fa f', features=[320, 320, 320, 1], activation=['GELU', 'Softplus', 'SiLU']),
}
RELU_SEED = 13              # (1, 0) breadth: no ReLU pre-activation within 1e-4 of zero (asserted with the fp64 oracle)


def _cases():
    """ name -> dict(group, problem, seed, n, path, kernel facts). Case D (n from the device's grid) is built in its own tests. """
    out = {}
    for width in (257, 272, 300, 384, 496, 511, 512):
        for depth in (1, 2, 3):
            for act in ('Tanh', 'Sigmoid'):
                out[f'A/{width}x{depth}/{act}'] = dict(group='A', problem=_plain((1, 1), width, depth, act), seed=width * 10 + depth, n=53,
                                                       shape=(1, 1), breadth=False, lh=depth - 1)
    for feats in ([512, 257, 512, 1], [260, 512, 300, 1]):
        out['B/' + 'x'.join(map(str, feats[:-1]))] = dict(group='B', problem=_problem((1, 1), 'fa fa fa f', feats, 'Tanh'), seed=sum(feats), n=53,
                                                          shape=(1, 1), breadth=False, lh=2)
    for n in (1, 15, 16, 17, 33):
        out[f'C/n{n}'] = dict(group='C', problem=_plain((1, 1), 512, 3), seed=512, n=n, shape=(1, 1), breadth=False, lh=2)
    for width in (272, 512):
        out[f'E/{width}x8'] = dict(group='E', problem=_plain((1, 1), width, 8), seed=width + 8, n=37, shape=(1, 1), breadth=False, lh=7)
    # (emulator twin of E: one tile)
    out['E/272x8/n16'] = dict(group='E-emu', problem=_plain((1, 1), 272, 8), seed=280, n=16, shape=(1, 1), breadth=False, lh=7)
    for shape in ((0, 0), (1, 0), (1, 1), (2, 0)):
        out[f'F/{shape[0]}{shape[1]}/plain'] = dict(group='F', problem=_plain(shape, 320, 3), seed=320 + 10 * shape[0] + shape[1], n=53, shape=shape,
                                                    breadth=False, lh=2)
        out[f'F/{shape[0]}{shape[1]}/breadth'] = dict(group='F', problem=_problem(shape, **BREADTH[shape]),
                                                      seed=RELU_SEED if shape == (1, 0) else 330 + 10 * shape[0] + shape[1], n=53, shape=shape,
                                                      breadth=True, lh=2, relu=shape == (1, 0))
    return out


CASES = _cases()
GENERIC = {
    # three second-order directions: one kernel call each
    'G/laplace3d': (lambda D: (lambda f, x, y, z: D(D(f, x), x) + D(D(f, y), y) + D(D(f, z), z) - 5 * torch.sin(np.pi * (x + y + z)),
                               dict(ndims=3, boundary_condition=1, layout='fa fa f', features=[264, 264, 1], activation='Tanh')), 264),
    # one second-order direction in a call of its own, the first-order pair in another
    'G/heat_drift': (lambda D: (lambda f, x, y, t: D(f, t) - 0.2 * D(D(f, x), x) + D(f, y),
                                dict(ndims=3, boundary_condition=0.3, layout='fa fa f', features=[264, 264, 1], activation='Tanh')), 265),
}
for _name, (_prob, _seed) in GENERIC.items():
    CASES[_name] = dict(group='G', problem=_prob, seed=_seed, n=53, shape=None, breadth=False, lh=1, path='generic')


# ---- references: computed once per case, shared, left unchanged -----------------------------------------------------------------------------
_REF = {}


def _points(n, d, seed=21):
    return np.random.RandomState(seed).rand(n, d).astype(np.float32)


def _reference(name, problem, seed, n, chunk=None, relu=False, fp32=True):
    """ dict(start, pts, loss32, g32, loss64, g64, u64, r64, relu_gap): the fp32 and the fp64 oracle from one fp32 start, one evaluation each
    (fp32=False: the fp64 side alone, for the CPU tier's look at the floors; the fp32 side is added when a kernel case asks for it) """
    key = (name, n)
    if key not in _REF:
        from oracle import pinn_oracle as po
        torch.manual_seed(seed)
        eq, kw = problem(po.D)
        o32 = po.OracleSolver(eq, **kw)
        o64 = po.OracleSolver(eq, dtype=torch.float64, **kw)
        start = o32.export_params()
        o64.import_params(start)
        pts = _points(n, kw['ndims'] + kw.get('nparams', 0))           # (parameter columns: test_width_128_256.py)
        gap, hooks = [np.inf], []
        if relu:            # smallest |pre-activation| of any ReLU layer over the batch, in fp64
            for m in o64.model.conv_block:
                if isinstance(m, torch.nn.ReLU):
                    hooks.append(m.register_forward_pre_hook(lambda mod, inp: gap.__setitem__(0, min(gap[0], float(inp[0].detach().abs().min())))))
            assert hooks
        ev64 = o64.evaluate(pts, chunk=chunk)
        g64 = o64.export_grads()
        for h in hooks:
            h.remove()
        _REF[key] = dict(start=start, pts=pts, loss64=ev64['loss'], g64=g64, u64=ev64['u'].reshape(-1), r64=ev64['r'].reshape(-1),
                         relu_gap=gap[0], problem=problem, o32=o32, chunk=chunk)
    ref = _REF[key]
    if fp32 and 'g32' not in ref:
        ev32 = ref['o32'].evaluate(ref['pts'], chunk=ref['chunk'])
        ref['loss32'], ref['g32'] = ev32['loss'], ref['o32'].export_grads()
    return ref


def _case_reference(name, fp32=True):
    c = CASES[name]
    return _reference(name, c['problem'], c['seed'], c['n'], relu=c.get('relu', False), fp32=fp32)


def _parts(i, n_tensors, arr):
    """ (label, array) of tensor i of export_grads order [W1, b1, ..., Wl, bl, log_scale]: the tensor itself, and -- for a hidden->hidden
    matrix with a side above 256 -- its 256-aligned blocks [mb, nb], the outputs of the block passes of pinn_wgrad_kernel """
    out = [(f'{i}', arr)]
    hidden = i % 2 == 0 and 0 < i < n_tensors - 3 and arr.ndim == 2
    if hidden and max(arr.shape) > HB:
        for mb in range((arr.shape[0] + HB - 1) // HB):
            for nb in range((arr.shape[1] + HB - 1) // HB):
                out.append((f'{i}[{mb},{nb}]', arr[mb * HB:(mb + 1) * HB, nb * HB:(nb + 1) * HB]))
    return out


def _at_the_floor(ref):
    """ labels of the gradient tensors / blocks of the fp64 oracle whose norm is below the absolute floor of the rule """
    low = []
    for i, g in enumerate(ref['g64']):
        if g is None:
            continue
        for label, part in _parts(i, len(ref['g64']), g):
            if float(np.linalg.norm(part)) <= 1e-9 * np.sqrt(part.size):
                low.append(label)
    return low


def _check_step(group, case, solver, ref):
    """ the rule of this file on the loss and the gradients the last step left in solver.grads """
    assert _at_the_floor(ref) == [], case
    lay = solver.model.net.layout
    loss = float(solver.grads[lay.off_loss])
    ok, err, arb = close_or_arbitrated([loss], [ref['loss32']], lambda: [ref['loss64']], LOSS_RTOL, atol=0.0, k=2.0)
    record_margin(f'width512_{group}', case, 'loss', err, LOSS_RTOL, arb)
    print(f'{case}: loss {loss!r} ref32 {ref["loss32"]!r} f64 {ref["loss64"]!r} err {err:.2e} arb={arb}')
    failed = [] if ok else [('loss', err)]
    got = export_grads(solver)
    n_blocks = 0
    for i, (g, w32, w64) in enumerate(zip(got, ref['g32'], ref['g64'])):
        if w64 is None:
            assert float(np.abs(g).max()) == 0.0, (case, i)
            continue
        for (label, gp), (_, p32), (_, p64) in zip(_parts(i, len(got), g), _parts(i, len(got), w32), _parts(i, len(got), w64)):
            ok, err, arb = close_or_arbitrated(gp, p32, lambda p64=p64: p64, GRAD_RTOL, k=2.0)
            record_margin(f'width512_{group}', f'{case}[{label}]', 'block' if '[' in label else 'gradient', err, GRAD_RTOL, arb)
            print(f'{case}: grad {label} shape {gp.shape} err {err:.2e} arb={arb}')
            n_blocks += '[' in label
            if not ok:
                failed.append((label, err))
    assert not failed, (case, failed)
    return n_blocks


def _solver(pa, ref, solver_kwargs):
    eq, kw = ref['problem'](pa.D)
    solver = pa.Solver(eq, **kw, **solver_kwargs)
    assert solver.model.net.layout.hp == 512
    load_params(solver, ref['start'])
    return solver


def _tile_name(shape, breadth):
    return f'pinn_tile_kernel<512,{shape[0]},{shape[1]},1,-1,-1,false,{136 if breadth else 128}>'


def _wgrad_name(shape, breadth):
    flags = 'true,true' if breadth else 'false,false'           # SKIPS, HEAVY
    return f'pinn_wgrad_kernel<512,{shape[0]},{shape[1]},false,1,false,{flags}>'


def _fused_case(pa, lib, name, solver_kwargs, on_device):
    """ one fused step of a case: path, kernels, rule. Returns the solver. """
    c, ref = CASES[name], _case_reference(name)
    solver = _solver(pa, ref, solver_kwargs)
    assert solver.program is not None, solver.program_error
    xs = torch.from_numpy(ref['pts'].copy()).to(solver.device)
    if on_device:
        lib.pinn_profile_tile(1)            # (HIP events around the two launches: the only witness of a weight-gradient launch that did NOT happen)
    try:
        solver._fused_step(xs, 1)
        if on_device:
            torch.cuda.synchronize()
            assert lib.pinn_last_tile_ms() >= 0.0
            # no hidden->hidden matrix, no weight-gradient launch (run_train: `plan.wgx && lh > 0`)
            assert (lib.pinn_last_wgrad_ms() >= 0.0) == (c['lh'] > 0), (name, lib.pinn_last_wgrad_ms())
    finally:
        if on_device:
            lib.pinn_profile_tile(0)
    assert lib.pinn_last_kernel_name().decode() == _tile_name(c['shape'], c['breadth']), lib.pinn_last_kernel_name()
    if c['lh'] > 0:
        assert lib.pinn_last_wgrad_kernel_name().decode() == _wgrad_name(c['shape'], c['breadth']), lib.pinn_last_wgrad_kernel_name()
    if c.get('relu'):
        assert ref['relu_gap'] > 1e-4, ref['relu_gap']
    _check_step(c['group'], name, solver, ref)
    return solver


def _names(group):
    return [k for k, c in CASES.items() if c['group'] == group]


# ---- CPU tier: no vacuous comparison, StreamSpec grouping, refusals ------------------------------------------------------------------------
@pytest.mark.parametrize('group', ['A', 'B', 'C', 'E', 'E-emu', 'F', 'G'])
def test_no_reference_gradient_sits_at_the_floor(group):
    """ with the two oracles alone: no case leaves a gradient tensor, or a 256-aligned block of a hidden matrix, whose fp64 norm is at the
    absolute floor 1e-9 sqrt(size) of the rule (it would pass whatever the kernel wrote); ReLU stays clear of its kink. Case D's batch size
    comes from the device's grid: its cases assert the same on the device. """
    for name in _names(group):
        ref = _case_reference(name, fp32=False)
        assert _at_the_floor(ref) == [], name
        assert all(np.isfinite(g).all() for g in ref['g64'] if g is not None)
        if CASES[name].get('relu'):
            assert ref['relu_gap'] > 1e-4, (name, ref['relu_gap'])
        if (group in ('C', 'E', 'E-emu') and '272' not in name) or name.startswith('A/512'):           # 512 on both sides: all four blocks of every hidden matrix are in the rule
            n_hidden = CASES[name]['lh']
            blocks = [label for i, g in enumerate(ref['g64']) if g is not None for label, _ in _parts(i, len(ref['g64']), g) if '[' in label]
            assert len(blocks) == 4 * n_hidden, (name, blocks)


def test_direction_groups_of_width_512_are_what_the_tracer_states():
    """ trace.StreamSpec at hp = 512: second-order directions one per call, the first-order rest in pairs; single calls for S <= 3 """
    from pydens_amd import trace
    lap = trace.StreamSpec({(0, 0), (1, 1), (2, 2)}, hp=512)
    assert not lap.single_call and not lap.combinable
    assert lap.groups == [([lap.dir_cols[k]], 1, [0, 1 + k, 4 + k]) for k in range(3)]
    heat = trace.StreamSpec({(0, 0), (1,), (2,)}, hp=512)
    assert (heat.nd, heat.n2) == (3, 1) and not heat.single_call and not heat.combinable
    assert heat.groups == [([heat.dir_cols[0]], 1, [0, 1, 4]), ([heat.dir_cols[1], heat.dir_cols[2]], 0, [0, 2, 3])]
    five = trace.StreamSpec({(0,), (1,), (2,), (3,), (4,)}, hp=512)
    assert [g[1] for g in five.groups] == [0, 0, 0] and [len(g[0]) for g in five.groups] == [2, 2, 1]
    for req, nd, n2 in (({()}, 0, 0), ({(0,)}, 1, 0), ({(0, 0)}, 1, 1), ({(0,), (1,)}, 2, 0)):
        spec = trace.StreamSpec(req, hp=512)
        assert spec.single_call and (spec.nd, spec.n2) == (nd, n2) and len(spec.groups) == 1
    assert not trace.StreamSpec({(0, 0), (1,)}, hp=512).single_call            # S = 4
    assert trace.StreamSpec({(0, 0), (1,)}, hp=256).single_call


def test_host_refusals_at_width_512(pa, emu_lib):
    """ what is not built at this width says so when the Solver is made (trace.StreamSpec, pinn_create_ex): third / fourth order, the second
    breadth set (activation codes above 7, nested skips), more than eight hidden layers, more than 512 units """
    kw = dict(_lib=emu_lib, device='cpu')
    net = dict(ndims=1, boundary_condition=0.2, layout='fa fa f', features=[300, 300, 1], activation='Tanh')
    third = lambda f, x: pa.D(pa.D(pa.D(f, x), x), x) - f
    fourth = lambda f, x: pa.D(pa.D(pa.D(pa.D(f, x), x), x), x) - f
    second = lambda f, x: pa.D(pa.D(f, x), x) + f
    for eq in (third, fourth):
        with pytest.raises(NotImplementedError, match='third- and fourth-order derivatives at hidden width 512 are not built'):
            pa.Solver(eq, **net, **kw)
    with pytest.raises(NotImplementedError, match='hidden width 512: the second set of full breadth kernels'):
        pa.Solver(second, **dict(net, activation=['Tanh', 'Mish']), **kw)
    with pytest.raises(NotImplementedError, match='hidden width 512: the second set of full breadth kernels'):
        pa.Solver(second, **dict(net, layout='fa R fa R fa fa + fa + f', features=[300] * 5 + [1]), **kw)
    with pytest.raises(Exception, match='at most 8 hidden layers'):
        pa.Solver(second, **dict(net, layout='fa' * 9 + 'f', features=[272] * 9 + [1]), **kw)
    with pytest.raises(Exception, match='> 512'):
        pa.Solver(second, **dict(net, features=[513, 300, 1]), **kw)
    ok = pa.Solver(second, **dict(net, layout='fa' * 8 + 'f', features=[272] * 8 + [1]), **kw)           # eight are built
    assert ok.model.net.layout.hp == 512 and ok.program is not None


# ---- A, B, C, F: fused steps -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('name', _names('A'))
def test_every_unit_of_widths_257_to_512_on_the_gpu(pa, dev, name):
    """ A: hidden layers exactly `width` wide, one to three of them, Tanh and Sigmoid, 53 points (three full tiles and a ragged one) on the
    fused (1, 1) plain kernel. At depth 1 there is no hidden->hidden matrix and no weight-gradient launch. """
    _fused_case(pa, dev, name, {}, True)


@gpu
@pytest.mark.parametrize('name', _names('B'))
def test_mixed_widths_inside_the_block_passes_on_the_gpu(pa, dev, name):
    """ B: rectangular real regions inside the 2 x 2 blocks (512 x 257, 257 x 512; 512 x 260, 300 x 512) """
    _fused_case(pa, dev, name, {}, True)


@gpu
@pytest.mark.parametrize('name', _names('C'))
def test_ragged_and_tiny_batches_on_the_gpu(pa, dev, name):
    """ C: 512 x 512 x 512 Tanh at 1, 15, 16, 17 and 33 points """
    _fused_case(pa, dev, name, {}, True)


@slow_emu
@pytest.mark.parametrize('name', ['C/n1', 'C/n17'])
def test_ragged_and_tiny_batches_on_the_emulator(pa, emu_lib, name):
    """ emulator twin of C where it fits one or two tiles """
    _fused_case(pa, emu_lib, name, dict(_lib=emu_lib, device='cpu'), False)


@gpu
@pytest.mark.parametrize('name', _names('F'))
def test_every_instantiation_in_backward_mode_on_the_gpu(pa, dev, name):
    """ F: the four stream shapes, each on a plain Tanh net (VAR 128) and on a net of the first breadth set (VAR 136; wgrad SKIPS, HEAVY):
    Sigmoid, Sin, Softplus, SiLU, GELU, ReLU, identity, a post-activation and a pre-activation skip, width 320 """
    solver = _fused_case(pa, dev, name, {}, True)
    if name == 'F/11/plain':
        # gemm='bf16x3' has no split kernels at this width: the fp32 kernels stay, with the same result
        want = solver.grads.clone()
        solver.set_gemm_mode('bf16x3')
        solver._fused_step(torch.from_numpy(_case_reference(name)['pts'].copy()).to(solver.device), 1)
        assert not ran_split_kernel(solver)
        assert dev.pinn_last_kernel_name().decode() == _tile_name((1, 1), False)
        assert torch.equal(solver.grads, want)


# ---- E: depth eight --------------------------------------------------------------------------------------------------------------------------
def _depth_eight(pa, lib, name, solver_kwargs, on_device):
    solver = _fused_case(pa, lib, name, solver_kwargs, on_device)
    ref = _case_reference(name)
    assert len([g for g in ref['g64'] if g is not None]) == 18 and solver.model.net.layout.lh == 7      # 9 matrices, 9 biases; 7 hidden->hidden
    return solver, ref


@gpu
@pytest.mark.parametrize('name', _names('E'))
def test_eight_hidden_layers_on_the_gpu(pa, dev, name):
    """ E: the limit of eight hidden layers, working: all eight bias-gradient rows (ACCB_ROWS) and all seven hidden matrices through the
    rule, then two Adam steps against the oracle """
    from oracle import pinn_oracle as po
    solver, ref = _depth_eight(pa, dev, name, {}, True)
    n, lr = CASES[name]['n'], 0.002
    pts = np.stack([_points(n, 1, seed=31), _points(n, 1, seed=32)])

    def oracle(dtype):
        eq, kw = ref['problem'](po.D)
        o = po.OracleSolver(eq, dtype=dtype, **kw)
        o.import_params(ref['start'])
        o.fit(niters=2, batch_size=n, points=pts, lr=lr)
        return o
    solver.fit(niters=2, batch_size=n, sampler=FixedBatches(pts), lr=lr)
    assert solver.last_fit_path == 'fused'
    fit_close('width512_E_fit', name, solver, oracle(torch.float32), lambda: oracle(torch.float64), adam_move=2 * lr)


@slow_emu
def test_eight_hidden_layers_on_the_emulator(pa, emu_lib):
    """ emulator twin of E at 272 units on one tile (37 points would be three) """
    _depth_eight(pa, emu_lib, 'E/272x8/n16', dict(_lib=emu_lib, device='cpu'), False)


# ---- D: the tile loop, the chunked slabs -------------------------------------------------------------------------------------------------------
D_NETS = {
    'tanh_11': ((1, 1), False, _plain((1, 1), 512, 3), 5120),
    'skip_20': ((2, 0), True, _problem((2, 0), 'faR fa fa+ f', [512, 512, 512, 1], ['Sin', 'GELU', 'Tanh'], bc=0.3), 5121),
}


def _launch_info(lib):
    info = (ctypes.c_int32 * 4)()
    assert lib.pinn_last_launch_info(info) == 0
    return dict(grid=info[0], per_cu=info[1], threads=info[2], smem=info[3])


_D_GRID = {}


def _tile_loop_reference(pa, lib, which):
    """ (solver, reference, grid) of case D: n = 16 (2 grid) + 3 points -- every workgroup of the persistent grid runs two tiles, workgroup 0
    a third, ragged one -- with `grid` read from the launch info of a probe launch large enough to fill the device """
    shape, breadth, problem, seed = D_NETS[which]
    if which not in _D_GRID:
        probe_eq, probe_kw = problem(pa.D)
        probe = pa.Solver(probe_eq, **probe_kw)
        n_probe = 16 * 8 * torch.cuda.get_device_properties(0).multi_processor_count          # more tiles than any grid (at most 4 workgroups per CU)
        probe._fused_step(torch.from_numpy(_points(n_probe, probe_kw['ndims'])).cuda(), 1)
        torch.cuda.synchronize()
        _D_GRID[which] = _launch_info(lib)['grid']
    grid = _D_GRID[which]
    n = 16 * (2 * grid) + 3
    ref = _reference('D/' + which, problem, seed, n, chunk=1024)
    return ref, grid, n


@gpu
@pytest.mark.parametrize('which', list(D_NETS))
def test_every_workgroup_runs_a_second_tile_on_the_gpu(pa, dev, which):
    """ D: the tile loop of pinn_tile_body at HP 512 (bias rows accumulated over tiles) and of pinn_wgrad_kernel (the register accumulator of
    each of the four block passes carried across tiles, its double-buffered stage pipeline across a tile boundary): 512 x 512 x 512 Tanh on
    the fused (1, 1) kernel, and a Sin / GELU / Tanh net with a skip on the (2, 0) breadth kernel. Then the same batch with the slab budget
    of one byte -- one sweep of the grid per chunk -- against the one-pass gradients. """
    shape, breadth, _, _ = D_NETS[which]
    ref, grid, n = _tile_loop_reference(pa, dev, which)
    solver = _solver(pa, ref, {})
    assert solver.program is not None, solver.program_error
    xs = torch.from_numpy(ref['pts'].copy()).cuda()
    solver._fused_step(xs, 1)
    torch.cuda.synchronize()
    info = _launch_info(dev)
    tiles = (n + 15) // 16
    print(f'D/{which}: n {n}, tiles {tiles}, launch info {info}')
    assert info['grid'] == grid and tiles > 2 * info['grid'] and n % 16 == 3
    assert dev.pinn_last_kernel_name().decode() == _tile_name(shape, breadth)
    assert dev.pinn_last_wgrad_kernel_name().decode() == _wgrad_name(shape, breadth)
    assert _check_step('D', f'D/{which}/n{n}', solver, ref) == 8
    one_pass = solver.grads.clone()
    lay = solver.model.net.layout
    try:
        dev.pinn_debug_wgx_chunk_bytes(solver.model.net.handle, 1)
        solver.model._workspaces.clear()
        solver._fused_step(xs, 1)
        torch.cuda.synchronize()
    finally:
        dev.pinn_debug_wgx_chunk_bytes(solver.model.net.handle, 0)
        solver.model._workspaces.clear()
    # no counter exposes the number of chunks: from make_plan, a budget below one tile's slabs gives chunk_tiles = one sweep =
    # max(grid, grid2) tiles, and grid2 <= CUs x WGS_PER_CU with WGS_PER_CU = 1 at width 512 (80 KB of LDS per workgroup)
    sweep = max(info['grid'], torch.cuda.get_device_properties(0).multi_processor_count)
    assert -(-tiles // sweep) > 1, (tiles, sweep)
    err = rel_l2(solver.grads[:lay.p_core].cpu().numpy(), one_pass[:lay.p_core].cpu().numpy())
    record_margin('width512_D_chunked', f'D/{which}/n{n}', 'gradient', err, 2e-6)
    print(f'D/{which}: chunked against one pass {err:.2e}')
    assert err < 2e-6
    _check_step('D', f'D/{which}/n{n}/chunked', solver, ref)


# ---- G: direction groups on the generic path -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('name', _names('G'))
def test_direction_groups_on_the_generic_path_on_the_gpu(pa, dev, name):
    """ G: stream shapes beyond S = 3 go through several calls of the (1, 1) and (2, 0) kernels and one backward call per group """
    ref = _case_reference(name)
    solver = _solver(pa, ref, {})
    assert solver.program is None and 'several kernel calls' in solver.program_error
    spec = solver.spec
    if name == 'G/laplace3d':
        assert spec.groups == [([spec.dir_cols[k]], 1, [0, 1 + k, 4 + k]) for k in range(3)]
    else:
        assert spec.groups == [([spec.dir_cols[0]], 1, [0, 1, 4]), ([spec.dir_cols[1], spec.dir_cols[2]], 0, [0, 2, 3])]
    xs = torch.from_numpy(ref['pts'].copy()).cuda()
    net, ran = solver.model.net, []
    backward = net.jet_backward

    def spy(*args, **kwargs):           # (the names are set on the host when a kernel is launched)
        out = backward(*args, **kwargs)
        ran.append((dev.pinn_last_kernel_name().decode(), dev.pinn_last_wgrad_kernel_name().decode()))
        return out
    net.jet_backward = spy
    try:
        solver._generic_step(xs, ('equation',), [], torch.nn.MSELoss(), 1)
    finally:
        del net.jet_backward
    torch.cuda.synchronize()
    shapes = [(1, 1), (2, 0)] if name == 'G/heat_drift' else [(1, 1)] * 3          # one backward call per group
    assert ran == [(_tile_name(s, False), _wgrad_name(s, False)) for s in shapes], ran
    _check_step('G', name, solver, ref)
    solver.fit(niters=1, batch_size=53, sampler=FixedBatches(ref['pts'][None]), lr=1e-3)
    assert solver.last_fit_path == 'generic'


# ---- H: predict and residual ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('batch', ['n53', 'tile_loop'])
def test_predict_and_residual_at_width_512_on_the_gpu(pa, dev, batch):
    """ H: forward mode on 512 x 512 x 512 Tanh, 53 points and case D's batch, against the fp64 oracle: the field within 2e-6 (the bar of
    test_every_width_and_depth_uses_all_its_units), the residual -- a second derivative -- within 2e-5 of max|r| (the bar of the forward
    checks of _wide512_case and test_streams_match_fp64_jets) """
    if batch == 'n53':
        ref = _reference('H/n53', _plain((1, 1), 512, 3), 5120, 53)
    else:
        ref, grid, n = _tile_loop_reference(pa, dev, 'tanh_11')
    solver = _solver(pa, ref, {})
    x = ref['pts'][:, 0]
    u = solver.predict(x).reshape(-1)
    info = _launch_info(dev)
    assert dev.pinn_last_kernel_name().decode() == 'pinn_tile_kernel<512,0,0,1,-1,-1,false,128>', dev.pinn_last_kernel_name()
    err_u = float(np.abs(u - ref['u64']).max())
    r = solver.residual(x).reshape(-1)
    assert dev.pinn_last_kernel_name().decode() == _tile_name((1, 1), False), dev.pinn_last_kernel_name()
    if batch == 'tile_loop':
        assert (len(x) + 15) // 16 > 2 * info['grid']
    scale = float(np.abs(ref['r64']).max())
    err_r = float(np.abs(r - ref['r64']).max())
    record_margin('width512_H', f'{batch}/n{len(x)}', 'predict', err_u, 2e-6)
    record_margin('width512_H', f'{batch}/n{len(x)}', 'residual', err_r / scale, 2e-5)
    print(f'H/{batch}: n {len(x)}, max|u - u64| {err_u:.2e}, max|r - r64| / max|r| {err_r / scale:.2e}')
    assert err_u < 2e-6 and err_r < 2e-5 * scale
