""" Hidden widths 65 .. 256 (padded to 128 and 256: pinn_launch_tile_hp128 / _hp256 with pinn_launch_wgrad_hp128 / _hp256, the widths of
BASELINE configs 3 and 5) through their own loops: every unit, every WAVE BLOCK of the weight-gradient kernel, unequal layers, ragged
batches, the tile loop with a weight-gradient grid larger than the tile kernel's, every stream shape in every kernel family, and the
first-layer reconstruction with parameter columns, shifted columns and diagonal directions.

Reference and rule (one for the whole file, that of test_width_512.py): every case builds oracle.pinn_oracle.OracleSolver twice from one
fp32 start (fp32 and fp64), loads that start into pa.Solver and runs ONE _fused_step / _generic_step. The loss (1e-5, no floor) and the
gradient of every parameter tensor (helpers.GRAD_RTOL, floor 1e-9 per entry) go through helpers.close_or_arbitrated, k = 2 against fp64 --
and so does every wave block of every hidden->hidden matrix: pinn_wgrad_kernel runs 2 x 4 waves (PinnWgCfg: WM = 2, WN = 4), wave w owns
rows (output units) [HP/2 (w / 4), ...) x columns (input units) [HP/4 (w % 4), ...) of the padded HP x HP matrix -- 64 x 32 at 128,
128 x 64 at 256. Units keep their index in the padded matrix (padding follows the real units), so a block is the same slice of the real
tensor, clipped to its shape. A block that clips to nothing lies wholly in the padding: it does not exist in the tensor and is no block of
the rule (width 96: column block 3; width 65: column block 3, and blocks [1, 2] are one row or one column). Every block that has an
entry is in the rule: LEFT_OUT, the list of blocks left out by name, is empty.
A tensor or block whose fp64 norm sits at or below its floor 1e-9 sqrt(size) would pass vacuously: there is none
(test_no_reference_gradient_sits_at_the_floor on the CPU tier, and again in every device case). No case has a ReLU layer; the kink rule of
test_width_512 (no pre-activation within 1e-4 of zero) is asserted through the same hook wherever one appears. The second breadth set
runs Mish / LogSigmoid, not ELU: the second derivative of ELU jumps at zero, which would need that rule for every layer.

Which path: everything up to third order in one call is a FUSED step (A, B, C, D, F but its fourth-order shape, E but the cases named
generic below). Fourth-order derivatives (F/173, E/uxxxy) and direction groups (E/uxy_var at width 200: (3, 3) is not built at 256) go
through _generic_step: one backward call per direction group, each asserted by kernel name.

Kernel cases are marked gpu. Emulator twins at HP 128 with at most 33 points run on the CPU tier; HP 256 on the emulator, and the five
calls of E/96/uxxxy (half a minute), need PYDENS_AMD_SLOW_EMU=1 like test_width_512.py. """
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_l2
from helpers import GRAD_RTOL, close_or_arbitrated, export_grads, load_params, record_margin
from test_width_512 import LOSS_RTOL, _launch_info, _reference, dev, emu_lib, pa  # noqa: F401  (fixtures)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))

gpu = pytest.mark.gpu
slow_emu = pytest.mark.skipif(os.environ.get('PYDENS_AMD_SLOW_EMU') != '1',
                              reason='a 256-wide tile costs the emulator more than ten seconds: PYDENS_AMD_SLOW_EMU=1, or the -m gpu twin')
PI = float(np.pi)
WM, WN = 2, 4               # PinnWgCfg: wave grid over the HP x HP output
EMU_N = 33                  # emulator twins: two full tiles and a ragged one
F_WIDTH = {128: 96, 256: 200}
# blocks left out of the rule by name: case -> {label: reason}. A block may only stand here if it is legitimately all zero, at most one in
# eight of a matrix, never a whole tensor. There is none.
LEFT_OUT = {}


# ---- the problems ----------------------------------------------------------------------------------------------------------------------
def _equations(D):
    """ key -> (equation, ndims, nparams): one equation per stream shape of the launchers, and those of group E """
    s = torch.sin
    return {
        '00': (lambda u, x: u - s(3.0 * x), 1, 0),
        '10': (lambda u, x: D(u, x) - u, 1, 0),
        '11': (lambda u, x: D(D(u, x), x) + u - s(3.0 * x), 1, 0),
        '20': (lambda u, x, y: D(u, x) + 0.5 * D(u, y) - u * u, 2, 0),
        # (the variable coefficient keeps the second derivatives apart: test_edge_shapes)
        '22': (lambda u, x, y: D(D(u, x), x) + x * D(D(u, y), y) - u * u, 2, 0),
        '32': (lambda u, x, y, z: D(D(u, x), x) + x * D(D(u, y), y) + D(u, z) - u * u, 3, 0),
        '33': (lambda u, x, y, z: D(D(u, x), x) + x * D(D(u, y), y) + y * D(D(u, z), z) - u * u, 3, 0),
        '21c': (lambda u, x, y: D(D(u, x), x) + D(D(u, y), y) - 5 * s(PI * (x + y)), 2, 0),
        '31c': (lambda u, x, y, t: D(D(u, x), x) + D(D(u, y), y) - D(u, t), 3, 0),
        '40': (lambda u, x, y, z, w: D(u, x) + 0.5 * D(u, y) - D(u, z) + 2.0 * D(u, w) - u * u, 4, 0),
        '41c': (lambda u, x, y, z, t: D(D(u, x), x) + D(D(u, y), y) + D(D(u, z), z) - D(u, t), 4, 0),
        '19': (lambda u, x: D(D(D(u, x), x), x) - u, 1, 0),
        '29': (lambda u, x, t: D(u, t) + u * D(u, x) + D(D(D(u, x), x), x), 2, 0),
        '173': (lambda u, x: D(D(D(D(u, x), x), x), x) - u, 1, 0),
        # E: parameter in the source term (d = 2 > nd = 1)
        'param1': (lambda u, x, e: D(D(u, x), x) + u - e * s(3.0 * x), 1, 1),
        # E: a derivative in the SECOND column only: direction column 1 at stream index 1, d = 3 > nd = 1
        'col2': (lambda u, x, y, e: D(D(u, y), y) + x * u - e * s(3.0 * y), 2, 1),
        # E: a mixed partial beside u_xx: the diagonal e_x + e_y as third direction. Constant coefficients: the three second derivatives are
        # ONE combined stream whose weights carry u_xy = (u_vv - u_xx - u_yy) / 2; a variable coefficient keeps them apart
        'uxy': (lambda u, x, y: D(D(u, x), x) + D(D(u, x), y) - u * u, 2, 0),
        'uxy_var': (lambda u, x, y: D(D(u, x), x) + x * D(D(u, x), y) - u * u, 2, 0),
        # E: weighted diagonals 2 e_x +- e_y, fourth order
        'uxxxy': (lambda u, x, y: D(D(D(D(u, x), x), x), y) - u, 2, 0),
    }


# stream shape (nd, packed n2, combined) of an equation key on the fused path
SHAPES = {'00': (0, 0, False), '10': (1, 0, False), '11': (1, 1, False), '20': (2, 0, False), '22': (2, 2, False), '32': (3, 2, False),
          '33': (3, 3, False), '21c': (2, 1, True), '31c': (3, 1, True), '40': (4, 0, False), '41c': (4, 1, True), '19': (1, 9, False),
          '29': (2, 9, False), '173': (1, 73, False), 'param1': (1, 1, False), 'col2': (1, 1, False), 'uxy': (3, 1, True), 'uxy_var': (3, 3, False)}
# kernel families: (layout, activation) of a three-layer net, and how the instantiation names carry them
FAMILIES = {
    'plain': ('fa fa fa f', 'Tanh'),
    'light': ('faR fa fa+ f', ['Tanh', 'Sigmoid', 'Tanh']),                 # a skip that carries activation outputs over Tanh / Sigmoid layers
    'heavy': ('fRa fa f+a f', ['Sin', 'SiLU', 'GELU']),                     # first breadth set, a skip that carries pre-activation jets
    'allact': ('fa fa fa f', ['Mish', 'LogSigmoid', 'Mish']),              # second breadth set (activation codes above 7)
}
WG_CASE = ['00', '10', '11', '20', '22', '32', '21c', '31c', '40', '41c', '19', '29', '173', '33']         # PINN_WG_CASE / PINN_WG_HEAVY ('33': 128 only)
FAMILY_SHAPES = {'plain': WG_CASE, 'heavy': WG_CASE, 'light': ['11', '22', '21c', '31c'],
                 'allact': ['00', '10', '11', '20', '22', '21c', '31c', '19', '173']}                    # PINN_ALLACT_SHAPES


def _tile_name(hp, shape, family):
    nd, n2, comb = shape
    actc, var = {'plain': (-1, 128), 'light': (-1, 8 | 1024 | 128), 'heavy': (-1, 8 | 128), 'allact': (-2, 8 | 128)}[family]
    if family == 'light' and (nd, n2, comb) == (2, 1, True):
        var |= 16           # the Dirichlet box of '21c' is a compile-time shape of the light-skip kernel (PINN_VAR_SPEC(1), pinn_spec_of)
    return f'pinn_tile_kernel<{hp},{nd},{n2},1,-1,{actc},{"true" if comb else "false"},{var}>'


def _wgrad_name(hp, shape, family):
    nd, n2, comb = shape
    flags = {'plain': 'false,false', 'light': 'true,false', 'heavy': 'true,true', 'allact': 'true,true,true'}[family]    # SKIPS, HEAVY[, ALLACT]
    return f'pinn_wgrad_kernel<{hp},{nd},{n2},{"true" if comb else "false"},1,false,{flags}>'


def _problem(key, layout, features, activation, bc=0.2):
    def make(D):
        eq, ndims, nparams = _equations(D)[key]
        kw = dict(ndims=ndims, boundary_condition=bc, layout=layout, features=list(features), activation=activation)
        if nparams:
            kw['nparams'] = nparams
        return eq, kw
    return make


def _hp(features):
    return 128 if max(features[:-1]) <= 128 else 256


def _case(out, name, group, key, layout, features, activation, seed, n=53, family='plain', calls=None, bc=0.2):
    """ calls: None = one fused step on the kernels of SHAPES[key]; else the (nd, n2, combined) of each backward call of the generic path """
    hp = _hp(features)
    assert 64 < max(features[:-1]) <= 256
    shapes = [SHAPES[key]] if calls is None else calls
    out[name] = dict(group=group, hp=hp, problem=_problem(key, layout, features, activation, bc), seed=seed, n=n, family=family,
                     path='fused' if calls is None else 'generic', lh=len(features) - 2,
                     kernels=[(_tile_name(hp, s, family), _wgrad_name(hp, s, family)) for s in shapes])


def _cases():
    out = {}
    for width in (65, 127, 128, 129, 255, 256):
        for depth in (2, 4):
            for act in ('Tanh', 'Sigmoid'):
                _case(out, f'A/{width}x{depth}/{act}', 'A', '11', 'fa' * depth + 'f', [width] * depth + [1], act, seed=width * 10 + depth)
    for feats in ([128, 65, 128, 1], [70, 128, 100, 1], [256, 129, 256, 1], [130, 256, 200, 1]):
        _case(out, 'B/' + 'x'.join(map(str, feats[:-1])), 'B', '11', 'fa fa fa f', feats, 'Tanh', seed=sum(feats))
    for width in (128, 256):
        for n in (1, 15, 16, 17, 33):
            _case(out, f'C/{width}/n{n}', 'C', '11', 'fa fa fa f', [width] * 3 + [1], 'Tanh', seed=width + 3, n=n)
    for hp, width in F_WIDTH.items():
        feats = [width] * 3 + [1]
        for family, keys in FAMILY_SHAPES.items():
            layout, act = FAMILIES[family]
            for key in keys:
                if key == '33' and hp == 256:
                    continue                                    # (3, 3) is not built at 256
                # fourth order runs on the generic path (Solver._try_compile): one backward call, the (1, 73) kernels
                calls = [SHAPES[key]] if key == '173' else None
                _case(out, f'F/{width}/{key}/{family}', 'F', key, layout, feats, act, seed=1000 + 7 * len(out), family=family, calls=calls)
        _case(out, f'E/{width}/param1', 'E', 'param1', 'fa fa fa f', feats, 'Tanh', seed=width + 41)
        _case(out, f'E/{width}/col2', 'E', 'col2', 'fa fa fa f', feats, 'Tanh', seed=width + 42)
        # u_xx + u_xy: directions x, y and the diagonal e_x + e_y, each with a second derivative: one fused (3, 1) combined call
        _case(out, f'E/{width}/uxy', 'E', 'uxy', 'fa fa fa f', feats, 'Tanh', seed=width + 43)
        # u_xx + x u_xy: the same directions as separate streams. Width 96: ONE fused (3, 3) call. Width 200: (3, 3) is not built, the
        # generic path's direction groups [x, y], [diagonal]
        _case(out, f'E/{width}/uxy_var', 'E', 'uxy_var', 'fa fa fa f', feats, 'Tanh', seed=width + 45,
              calls=None if hp == 128 else [(2, 2, False), (1, 1, False)])
    # u_xxxy on the generic path: four fourth-order directions (both diagonals, both weighted diagonals 2 e_x +- e_y), a call each, and
    # the column x to third order (D(D(D(u, x), x), x) is asked for on the way)
    _case(out, 'E/96/uxxxy', 'E', 'uxxxy', 'fa fa fa f', [96] * 3 + [1], 'Tanh', seed=96 + 44, calls=[(1, 73, False)] * 4 + [(1, 9, False)])
    return out


CASES = _cases()


def _names(group, hp=None, path=None):
    return [k for k, c in CASES.items() if c['group'] == group and hp in (None, c['hp']) and path in (None, c['path'])]


# ---- references: computed once per (case, batch size), shared, left unchanged ---------------------------------------------------------------
def _case_reference(name, n=None, fp32=True):
    c = CASES[name]
    relu = 'ReLU' in np.atleast_1d(c['problem'](None)[1]['activation']).tolist()          # (the equation is built, not called)
    return _reference('w128_256/' + name, c['problem'], c['seed'], n or c['n'], relu=relu, fp32=fp32)


def _hidden(i, n_tensors, arr):
    """ export_grads order [W1, b1, ..., Wl, bl, log_scale]: is tensor i a hidden->hidden matrix? """
    return i % 2 == 0 and 0 < i < n_tensors - 3 and arr.ndim == 2


def _parts(i, n_tensors, arr, hp):
    """ (label, array) of tensor i: the tensor itself, and -- for a hidden->hidden matrix -- the block of each of the 2 x 4 waves of
    pinn_wgrad_kernel, clipped to the real shape (a block that clips to nothing lies in the padding) """
    out = [(f'{i}', arr)]
    if _hidden(i, n_tensors, arr):
        bm, bn = hp // WM, hp // WN
        for wi in range(WM):
            for wj in range(WN):
                block = arr[bm * wi:bm * (wi + 1), bn * wj:bn * (wj + 1)]
                if block.size:
                    out.append((f'{i}[wave{wi * WN + wj}:{wi},{wj}]', block))
    return out


def _at_the_floor(ref, hp, case):
    """ labels of the gradient tensors / wave blocks of the fp64 oracle whose norm is at or below the absolute floor of the rule """
    low = []
    for i, g in enumerate(ref['g64']):
        if g is None:
            continue
        for label, part in _parts(i, len(ref['g64']), g, hp):
            if label in LEFT_OUT.get(case, {}):
                continue
            if float(np.linalg.norm(part)) <= 1e-9 * np.sqrt(part.size):
                low.append(label)
    return low


def _n_blocks(features):
    """ wave blocks with at least one entry, over the hidden->hidden matrices of a net """
    total = 0
    for fan_in, fan_out in zip(features[:-2], features[1:-1]):
        hp = _hp(features)
        total += min(WM, -(-fan_out // (hp // WM))) * min(WN, -(-fan_in // (hp // WN)))
    return total


def _check_step(group, case, name, solver, ref):
    """ the rule of this file on the loss and the gradients the last step left in solver.grads; returns the number of wave blocks checked """
    hp = solver.model.net.layout.hp
    assert _at_the_floor(ref, hp, name) == [], case
    assert ref['relu_gap'] > 1e-4, (case, ref['relu_gap'])
    test = f'width{hp}_{group}'
    lay = solver.model.net.layout
    loss = float(solver.grads[lay.off_loss])
    ok, err, arb = close_or_arbitrated([loss], [ref['loss32']], lambda: [ref['loss64']], LOSS_RTOL, atol=0.0, k=2.0)
    record_margin(test, case, 'loss', err, LOSS_RTOL, arb)
    print(f'{case}: loss {loss!r} ref32 {ref["loss32"]!r} f64 {ref["loss64"]!r} err {err:.2e} arb={arb}')
    failed = [] if ok else [('loss', err)]
    got = export_grads(solver)
    n_blocks = 0
    for i, (g, w32, w64) in enumerate(zip(got, ref['g32'], ref['g64'])):
        if w64 is None:
            assert float(np.abs(g).max()) == 0.0, (case, i)
            continue
        for (label, gp), (_, p32), (_, p64) in zip(_parts(i, len(got), g, hp), _parts(i, len(got), w32, hp), _parts(i, len(got), w64, hp)):
            if label in LEFT_OUT.get(name, {}):
                continue
            ok, err, arb = close_or_arbitrated(gp, p32, lambda p64=p64: p64, GRAD_RTOL, k=2.0)
            record_margin(test, f'{case}[{label}]', 'block' if '[' in label else 'gradient', err, GRAD_RTOL, arb)
            print(f'{case}: grad {label} shape {gp.shape} err {err:.2e} arb={arb}')
            n_blocks += '[' in label
            if not ok:
                failed.append((label, err))
    assert not failed, (case, failed)
    return n_blocks


def _solver(pa, ref, hp, solver_kwargs):
    eq, kw = ref['problem'](pa.D)
    solver = pa.Solver(eq, **kw, **solver_kwargs)
    assert solver.model.net.layout.hp == hp
    load_params(solver, ref['start'])
    return solver


def _run_case(pa, lib, name, solver_kwargs, n=None):
    """ one step of a case on its path: kernels by name, then the rule. Returns the solver. """
    c = CASES[name]
    ref = _case_reference(name, n)
    solver = _solver(pa, ref, c['hp'], solver_kwargs)
    xs = torch.from_numpy(ref['pts'].copy()).to(solver.device)
    on_device = solver.device.type == 'cuda'
    if c['path'] == 'fused':
        assert solver.program is not None, solver.program_error
        solver._fused_step(xs, 1)
        ran = [(lib.pinn_last_kernel_name().decode(), lib.pinn_last_wgrad_kernel_name().decode())]
    else:
        assert solver.program is None, name
        net, ran = solver.model.net, []
        backward = net.jet_backward

        def spy(*args, **kwargs):           # (the names are set on the host when a kernel is launched)
            result = backward(*args, **kwargs)
            ran.append((lib.pinn_last_kernel_name().decode(), lib.pinn_last_wgrad_kernel_name().decode()))
            return result
        net.jet_backward = spy
        try:
            solver._generic_step(xs, ('equation',), [], torch.nn.MSELoss(), 1)
        finally:
            del net.jet_backward
    if on_device:
        torch.cuda.synchronize()
    assert ran == c['kernels'], (name, ran)
    case = name if n is None else f'{name}/n{n}'
    blocks = _check_step(c['group'], case, name, solver, ref)
    feats = ref['problem'](pa.D)[1]['features']
    assert blocks == _n_blocks(feats), (name, blocks)
    return solver


# ---- CPU tier: no vacuous comparison; every instantiation of the launchers is in a case ---------------------------------------------------
@pytest.mark.parametrize('group', ['A', 'B', 'C', 'E', 'F'])
def test_no_reference_gradient_sits_at_the_floor(group):
    """ with the two oracles alone: no case -- at its device batch or at the emulator twin's -- leaves a gradient tensor, or a wave block
    of a hidden matrix, whose fp64 norm is at the absolute floor 1e-9 sqrt(size) of the rule (it would pass whatever the kernel wrote);
    no ReLU pre-activation within 1e-4 of zero. Group D's batch size comes from the device's grid: its cases assert the same there. """
    for name in _names(group):
        c = CASES[name]
        for n in sorted({c['n'], min(c['n'], EMU_N)} if c['hp'] == 128 else {c['n']}):
            ref = _case_reference(name, n, fp32=False)
            assert _at_the_floor(ref, c['hp'], name) == [], (name, n)
            assert all(np.isfinite(g).all() for g in ref['g64'] if g is not None)
            assert ref['relu_gap'] > 1e-4, (name, ref['relu_gap'])
            matrices = [g for i, g in enumerate(ref['g64']) if g is not None and _hidden(i, len(ref['g64']), g)]
            assert len(matrices) == c['lh'] and all(g is not None for g in ref['g64'][:-1]), name
            for label in LEFT_OUT.get(name, {}):
                assert '[' in label, (name, label)                 # never a whole tensor
            for i, g in enumerate(ref['g64']):
                left = [label for label in LEFT_OUT.get(name, {}) if label.startswith(f'{i}[')]
                assert len(left) <= 1, (name, left)                # at most one block in eight of a matrix
    if group == 'A':            # both sides full: all eight wave blocks of every hidden matrix are in the rule
        for hp in (128, 256):
            ref = _case_reference(f'A/{hp}x4/Tanh', fp32=False)
            blocks = [label for i, g in enumerate(ref['g64']) if g is not None for label, _ in _parts(i, len(ref['g64']), g, hp) if '[' in label]
            assert len(blocks) == 8 * 3 == _n_blocks([hp] * 4 + [1])


def _launcher_instantiations():
    """ hp -> the pinn_wgrad_kernel instantiations pinn_launch_wgrad_hp128 / _hp256 (and pinn_launch_wgrad2_*) can return in the fp32 GEMM
    mode, read from the macro lists of pinn_inst.inc: PINN_WG_CASE (plain), PINN_WG_HEAVY (first breadth set), the four light-skip lines,
    PINN_ALLACT_SHAPES (second set). Shapes inside `#if PINN_INST_HP <= 128` belong to 128 alone. """
    with open(os.path.join(ROOT, 'pydens_amd', 'csrc', 'pinn_inst.inc')) as f:
        text = f.read()
    text = text[text.index('pinn_breadth_kind'):]               # (past the width-512 launchers)
    only128 = ''.join(re.findall(r'#if PINN_INST_HP <= 128\n(.*?)#endif', text, flags=re.S))
    args = r'\((\d+), (\d+), (true|false)\)'
    shape = lambda m: (int(m[0]), int(m[1]), m[2] == 'true')
    found = {
        'plain': {shape(m) for m in re.findall(r'PINN_WG_CASE' + args, text)},
        'heavy': {shape(m) for m in re.findall(r'PINN_WG_HEAVY' + args, text)},
        'light': {shape(m) for m in re.findall(r'launch_wgrad<(\d+), (\d+), (true|false), 1, false, true>\(a, req\)', text)},
        'allact': {shape(m) for m in re.findall(r'X' + args, re.search(r'#define PINN_ALLACT_SHAPES\(X\)(.*)', text).group(1))},
    }
    narrow = {'plain': {shape(m) for m in re.findall(r'PINN_WG_CASE' + args, only128)},
              'heavy': {shape(m) for m in re.findall(r'PINN_WG_HEAVY' + args, only128)}}
    return {hp: {_wgrad_name(hp, s, family) for family, shapes in found.items() for s in shapes
                 if hp == 128 or s not in narrow.get(family, ())} for hp in (128, 256)}


def test_every_weight_gradient_instantiation_is_in_a_case():
    """ the instantiations the launchers hold against the names the cases assert (every device case asserts the exact pair it ran on): a
    shape added to a launcher later shows up here as untested """
    built = _launcher_instantiations()
    assert len(built[128]) == 14 + 14 + 4 + 9 and len(built[256]) == 13 + 13 + 4 + 9
    for hp in (128, 256):
        asserted = {w for c in CASES.values() if c['hp'] == hp for _, w in c['kernels']}
        assert built[hp] - asserted == set(), hp
        assert asserted - built[hp] == set(), hp


# ---- A, B, C, E, F on the device ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('name', _names('A'))
def test_every_unit_of_widths_65_to_256_on_the_gpu(pa, dev, name):
    """ A: hidden layers exactly `width` wide (one past a padding boundary included), two and four of them, Tanh and Sigmoid, 53 points
    (three full tiles and a ragged one) on the plain (1, 1) kernels """
    _run_case(pa, dev, name, {})


@gpu
@pytest.mark.parametrize('name', _names('B'))
def test_unequal_layers_inside_the_wave_blocks_on_the_gpu(pa, dev, name):
    """ B: rectangular real regions inside the padded blocks (65 x 128 and 128 x 65; 128 x 70 and 100 x 128; the same around 256) """
    _run_case(pa, dev, name, {})


@gpu
@pytest.mark.parametrize('name', _names('C'))
def test_ragged_and_tiny_batches_on_the_gpu(pa, dev, name):
    """ C: 1, 15, 16, 17 and 33 points: one ragged stage set, one full tile, a tile boundary inside the double-buffered pipeline """
    _run_case(pa, dev, name, {})


@gpu
@pytest.mark.parametrize('name', _names('E'))
def test_first_layer_reconstruction_on_the_gpu(pa, dev, name):
    """ E: layer li == 0 of pinn_wgrad_kernel rebuilds z_k from W1 and dir_cols: a parameter column (d > nd), a derivative in the second
    column alone, a diagonal direction, weighted diagonals """
    _run_case(pa, dev, name, {})


@gpu
@pytest.mark.parametrize('name', _names('F'))
def test_every_stream_shape_in_every_family_on_the_gpu(pa, dev, name):
    """ F: every (shape, family) pair of the weight-gradient launchers with its tile kernel, width 96 and width 200 """
    _run_case(pa, dev, name, {})


# ---- emulator twins (HP 128, at most 33 points; HP 256 and the five calls of u_xxxy behind PYDENS_AMD_SLOW_EMU) -------------------------------

def _emu(pa, emu_lib, name):
    c = CASES[name]
    _run_case(pa, emu_lib, name, dict(_lib=emu_lib, device='cpu'), n=None if c['n'] <= EMU_N else EMU_N)


SLOW_ON_THE_EMULATOR = ['E/96/uxxxy']             # 32 s


@pytest.mark.parametrize('name', [k for k in _names('A', 128) + _names('B', 128) + _names('C', 128) + _names('E', 128) if k not in SLOW_ON_THE_EMULATOR])
def test_units_layers_batches_and_first_layer_on_the_emulator(pa, emu_lib, name):
    _emu(pa, emu_lib, name)


@pytest.mark.parametrize('name', _names('F', 128))
def test_every_stream_shape_in_every_family_on_the_emulator(pa, emu_lib, name):
    _emu(pa, emu_lib, name)


@slow_emu
@pytest.mark.parametrize('name', SLOW_ON_THE_EMULATOR + ['A/129x2/Tanh', 'B/130x256x200', 'C/256/n17', 'E/200/uxy_var', 'F/200/31c/heavy',
                                                         'F/200/19/allact'])
def test_width_256_and_slow_cases_on_the_emulator(pa, emu_lib, name):
    _emu(pa, emu_lib, name)


# ---- D: the tile loop, a weight-gradient grid above the tile kernel's, the chunked slabs ----------------------------------------------------------
D_NETS = {
    'tanh_11': ('11', 'plain', 'fa fa fa f', 'Tanh', 0.2),
    'skip_20': ('20', 'heavy', 'faR fa fa+ f', ['Sin', 'GELU', 'Tanh'], 0.3),
}
_D = {}


def _tile_loop_reference(pa, lib, width, which):
    """ (reference, tile grid, weight-gradient grid, n) of case D. Both grids are persistent: make_plan (pinn_abi.cpp) sizes the tile
    kernel's as CUs x (occupancy answer, capped) and the weight-gradient kernel's as CUs x PinnWgCfg::WGS_PER_CU, each capped by the
    number of tiles, and caps the tile grid by the other. `grid` is read from the launch info of a probe launch large enough to fill the
    device; WGS_PER_CU is 2 at HP 128 (41 KB of LDS, 32 accumulator registers) and 1 at 256. n = 16 (2 sweep) + 3 points with sweep =
    max(grid, CUs x WGS_PER_CU): every workgroup of BOTH kernels runs two tiles, workgroup 0 a third, ragged one. """
    key, family, layout, act, bc = D_NETS[which]
    problem = _problem(key, layout, [width] * 3 + [1], act, bc)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    wgs_per_cu = 2 if width <= 128 else 1
    if (width, which) not in _D:
        probe_eq, probe_kw = problem(pa.D)
        probe = pa.Solver(probe_eq, **probe_kw)
        n_probe = 16 * 8 * cus                                      # more tiles than any grid (at most 4 workgroups per CU)
        probe._fused_step(torch.from_numpy(np.random.RandomState(21).rand(n_probe, probe_kw['ndims']).astype(np.float32)).cuda(), 1)
        torch.cuda.synchronize()
        _D[(width, which)] = _launch_info(lib)
    info = _D[(width, which)]
    grid2 = cus * wgs_per_cu
    n = 16 * (2 * max(info['grid'], grid2)) + 3
    ref = _reference(f'w128_256/D/{width}/{which}', problem, 5000 + width + len(which), n, chunk=1024)
    return ref, info['grid'], grid2, n


@gpu
@pytest.mark.parametrize('which', list(D_NETS))
@pytest.mark.parametrize('width', [128, 256])
def test_every_workgroup_runs_a_second_tile_on_the_gpu(pa, dev, width, which):
    """ D: the tile loop of the tile kernel (bias rows accumulated over tiles) and of pinn_wgrad_kernel (the register accumulator of every
    wave carried across tiles, the stage pipeline across a tile boundary), on a plain Tanh net ((1, 1)) and a Sin / GELU / Tanh net with a
    skip on the full breadth kernels ((2, 0)). At width 128 the weight-gradient grid is LARGER than the tile kernel's, so the workgroups
    with PINN_BID >= A.partial_row0 zero their own partial rows outside the hidden matrices. Then the same batch with a slab budget of one
    byte -- one sweep of the grids per chunk -- against the one-pass gradients. """
    key, family, _, _, _ = D_NETS[which]
    ref, grid, grid2, n = _tile_loop_reference(pa, dev, width, which)
    name = f'D/{width}/{which}/n{n}'
    solver = _solver(pa, ref, width, {})
    assert solver.program is not None, solver.program_error
    xs = torch.from_numpy(ref['pts'].copy()).cuda()
    solver._fused_step(xs, 1)
    torch.cuda.synchronize()
    info = _launch_info(dev)
    tiles = (n + 15) // 16
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f'{name}: tiles {tiles}, launch info {info}, CUs {cus}, weight-gradient grid {grid2}')
    assert info['grid'] == grid and tiles > 2 * max(grid, grid2) and n % 16 == 3
    if width == 128:
        # how we know the branch `PINN_BID >= A.partial_row0` ran: partial_row0 is the tile kernel's grid (run_train: a->partial_row0 =
        # plan.grid) = info['grid']; the weight-gradient grid is min(CUs x WGS_PER_CU, tiles) = 2 CUs (make_plan), and WGS_PER_CU = 2 is
        # a compile-time fact of PinnWgCfg<128, ...>. No counter exposes grid2 itself. The rows those workgroups own are summed by the
        # reduction (Plan::rows), so stale contents there would show in the bias and first / last-layer gradients below.
        assert info['per_cu'] == 1 and grid == cus and grid2 == 2 * cus > grid, (info, cus)
    assert dev.pinn_last_kernel_name().decode() == _tile_name(width, SHAPES[key], family)
    assert dev.pinn_last_wgrad_kernel_name().decode() == _wgrad_name(width, SHAPES[key], family)
    assert _check_step('D', name, name, solver, ref) == 16
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
    # make_plan: a budget below one tile's slabs gives chunk_tiles = one sweep = max(grid, grid2) tiles: three chunks here
    assert -(-tiles // max(grid, grid2)) == 3
    err = rel_l2(solver.grads[:lay.p_core].cpu().numpy(), one_pass[:lay.p_core].cpu().numpy())
    record_margin(f'width{width}_D_chunked', name, 'gradient', err, 2e-6)
    print(f'{name}: chunked against one pass {err:.2e}')
    assert err < 2e-6
    _check_step('D', name + '/chunked', name, solver, ref)
