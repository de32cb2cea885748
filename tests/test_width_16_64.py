""" Hidden widths up to 64 (padded to 16, 32 and 64: pinn_launch_tile_hp16 / _hp32 / _hp64, the widths of BASELINE configs 1, 2 and 4 and of
every two-team kernel) through their own loops: every unit either side of every padding and wave boundary, every wave's rows and every K tile
of every hidden matrix, unequal layers, batches one point either side of the 16-, 32- and 48-point tiles, the tile loop, every stream shape in
every kernel family, and every static / specialised instantiation of the launchers by name.

Reference and rule (one for the whole file, that of test_width_512.py and test_width_128_256.py): every case builds
oracle.pinn_oracle.OracleSolver twice from one fp32 start (fp32 and fp64), loads that start into pa.Solver and runs ONE _fused_step /
_generic_step. The loss (1e-5, no floor) and the gradient of every parameter tensor (helpers.GRAD_RTOL, floor 1e-9 per entry) go through
helpers.close_or_arbitrated, k = 2 against fp64 -- and so does every BAND below. At these widths the weight gradients never leave the tile
kernel: they sit in MFMA accumulators over the tile loop and leave through pinn_reduce_rows, so a wrong owner map shows only in the entries.

Owner map (pinn_kernel.h, "Lane map"): PinnCfg<HP <= 64> runs NW = NT = HP / 16 waves, wave w owns output units [16 w, 16 w + 16) of every
layer (lane: lr = lane & 15 the point, lq = lane >> 4 the unit quad, four consecutive units per lane), and the GEMMs walk K in quads grouped
by 16-unit tiles. Units keep their index in the padded matrix, so with torch's [out, in] weights:
    row band w of a hidden->hidden matrix     W[16 w : 16 w + 16, :]      the 16 output units of wave w, all inputs
    column band k of a hidden->hidden matrix  W[:, 16 k : 16 k + 16]      all outputs, the 16 input units of K tile k
    band w of W1 and of a hidden bias         the 16 units of wave w      (and the K tiles of the last layer's row, which the waves own alike)
each clipped to the real shape. A band that clips to nothing lies in the padding and is no band of the rule. LEFT_OUT, the bands left out
by name, is empty. Every case returns the number of bands it checked, asserted against _n_bands(features).
A tensor or band whose fp64 norm sits at or below its floor 1e-9 sqrt(size) would pass vacuously: there is none
(test_no_reference_gradient_sits_at_the_floor on the CPU tier, and again in every kernel case). No case has a ReLU / LeakyReLU / ELU / SELU
layer; the second breadth set runs Mish / LogSigmoid.

Kernel by name: every case asserts the exact pinn_last_kernel_name() of each call, built by _tile_name, which mirrors the launcher; no
weight-gradient launch happens at these widths (pinn_last_wgrad_kernel_name() is the same before and after the step).
test_every_tile_instantiation_is_in_a_case reads pinn_inst.inc and compares the instantiations the three launchers can return in the fp32
GEMM mode with the names asserted here, both ways: 144 instantiations (41 generic-depth per width, 9 + 3 static, 3 Sin, 4 + 1 two-team,
the accurate-tanh twin), of which ONE is unreachable under the product's switches (UNREACHABLE):
    pinn_tile_kernel<64,2,1,1,3,2,true,24>   the one-team Dirichlet-box Sin kernel: `pinn_spec_of(...) == 1 && PINN_SIN_TEAMS && PINN_SIN_MT == 1`
                                             (both 1) returns pinn_launch_cfg2_sin_hp64 on the line before it.

Groups, one step each: A units (48 cases, 810 bands), B unequal layers (6, 120), C ragged batches per tile height (100, 4 680), E first
layer and point-stage inputs (14, 315), F every stream shape in every family at widths 12 / 24 / 48 (123, 1 962), G static and specialised
kernels on the Dirichlet box and off it (30, 1 284): 321 cases and 9 171 bands, on the emulator (CPU tier) and again, marked gpu, on the
device. D, the tile loop with the accumulators carried into a second tile of every workgroup and of both teams, is gpu only: 3 cases, 120
bands, 8 195 / 24 579 / 16 387 points on a 256-CU device (grid 256, one workgroup per CU), 0.07 / 0.13 / 0.43 s with their shared references.
Fourth order (F/*/173/*, E/*/uxxxy) goes through _generic_step, every backward call asserted by name; everything else is ONE fused step.

Measured. Device (MI355X): the 324 gpu cases take 7 s together, the slowest 0.5 s. Emulator: all 321 twins pass; the CPU tier of this file
takes 147 s on one core (two threads), the slowest case 4.3 s (E/48/uxxxy); group C alone took 64 s of it, so 28 of its twins -- the largest
batch of each tile height, the second multiple of the 32-point and two-team rounds -- stand behind PYDENS_AMD_SLOW_EMU=1 (C_THINNED): 77 s
on one core remain, about a quarter of a minute of the six-worker CPU tier. No kernel case failed, on the emulator or on the device: no
band misses the k = 2 rule, and no kernel fix came out of this file.
Worst margins on the device (record_margin; relative error against the fp32 oracle, or against fp64 where arbitrated; bar 1e-5):
    whole tensors    9.5e-6  F/48/29/heavy[7] (the output bias of the third-order Sin / SiLU / GELU net); groups A .. E and G: 3.3e-6
    bands, A .. E    4.3e-6  C/static10x4/n97[0[wave1]]; a hidden matrix: 2.3e-7 B/32x17x32[2[rows1]], 2.1e-6 B/64x33x64[4[cols2]] (one column)
    bands, F         8.5e-6  F/48/173/heavy[0[wave2]] and F/24/19/allact[5[wave1]] (third / fourth order, arbitrated: 173 of 1 962)
    bands, D         9.5e-6  D/cfg2/n16387[5[wave1]] (16 bias entries summed over 16 387 points, arbitrated: 6 of 120)
    narrowest band   1.26e-5 A/33x4/Tanh[6[cols2]]: ONE input unit (index 32) x 33 outputs of the last hidden matrix, fp64 norm 6.3e-4 beside
                     1.31 of the whole matrix. Its absolute error is 8.2e-9 (the fp32 oracle's own: 1.3e-9) -- rounding of 53-point sums
                     whose terms cancel, at the scale of the terms, the same on the emulator -- and it passes the FIRST test of
                     close_or_arbitrated, 1e-5 x 6.3e-4 + the floor 1e-9 sqrt(33), without the arbiter. The same column of the two
                     matrices before it, and the one-row bands rows2 of all three, sit at 2e-7. """
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import GRAD_RTOL, close_or_arbitrated, export_grads, load_params, record_margin
from test_width_128_256 import FAMILIES, SHAPES, _equations
from test_width_512 import LOSS_RTOL, _launch_info, _reference, dev, emu_lib, pa  # noqa: F401  (fixtures)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))

gpu = pytest.mark.gpu
slow_emu = pytest.mark.skipif(os.environ.get('PYDENS_AMD_SLOW_EMU') != '1',
                              reason='more than about five seconds on the emulator: PYDENS_AMD_SLOW_EMU=1, or the -m gpu twin')
PI = float(np.pi)
BAND = 16                   # units per wave = units per K tile
# bands left out of the rule by name: case -> {label: reason}. A band may only stand here if it is legitimately all zero, at most one in
# eight of a matrix, never a whole tensor. There is none.
LEFT_OUT = {}
# instantiations the launchers hold that no call reaches under the product's switch values: name -> the line that shadows it
UNREACHABLE = {
    'pinn_tile_kernel<64,2,1,1,3,2,true,24>':
        'if (pinn_spec_of(a, nd, n2) == 1 && PINN_SIN_TEAMS && PINN_SIN_MT == 1)',       # returns pinn_launch_cfg2_sin_hp64 first
}


# ---- the problems ----------------------------------------------------------------------------------------------------------------------
def _more_equations(D):
    """ key -> (equation, ndims, nparams) beside test_width_128_256._equations: the shapes of the specialised kernels and of group E """
    s = torch.sin
    return {
        # Poisson box with a parameter column (d = 3 > nd = 2): the combined stream OFF the Dirichlet-box specialisation
        'box_e': (lambda u, x, y, e: D(D(u, x), x) + D(D(u, y), y) - e * s(PI * (x + y)), 2, 1),
        # ... and with a non-affine term: a residual program on the box
        'box_prog': (lambda u, x, y: D(D(u, x), x) + D(D(u, y), y) + 1.5 * u * u - 5 * s(PI * (x + y)), 2, 0),
        # evolution in (x, t): affine (heat with a source) and a residual program (viscous Burgers)
        'heat_xt': (lambda u, x, t: D(u, t) - 0.3 * D(D(u, x), x) - 2.0 * torch.exp(-t) * s(PI * x), 2, 0),
        'burgers': (lambda u, x, t: D(u, t) + u * D(u, x) - 0.05 * D(D(u, x), x), 2, 0),
        # the ODE family of BASELINE config 4: one first derivative, one parameter column
        'ode_e': (lambda u, x, e: D(u, x) - e * PI * torch.cos(e * PI * x), 1, 1),
        # five input columns (test_edge_shapes two_dims_three_parameters)
        'p5': (lambda u, x, t, a, b, c: D(u, t) - a * D(D(u, x), x) + b * u - c, 2, 3),
        # shifted domain (test_edge_shapes shifted_domain)
        'shifted': (lambda u, x, y: D(D(u, x), x) + D(D(u, y), y) - torch.exp(x), 2, 0),
    }


MORE_SHAPES = {'box_e': (2, 1, True), 'box_prog': (2, 1, True), 'heat_xt': (2, 1, True), 'burgers': (2, 1, True), 'ode_e': (1, 0, False),
               'p5': (2, 1, True), 'shifted': (2, 1, True), 'uxxxy': None}
IC = {'sin': lambda x: torch.sin(PI * x), 'bump': lambda x: x * (1 - x)}       # initial conditions by name (a number stands for itself)

FAMILY_SHAPES = {'plain': ['00', '10', '11', '20', '22', '32', '33', '40', '21c', '31c', '41c', '19', '29', '173'],
                 'heavy': ['00', '10', '11', '20', '22', '32', '33', '40', '21c', '31c', '41c', '19', '29', '173'],
                 'light': ['11', '22', '21c', '31c'],
                 'allact': ['00', '10', '11', '20', '22', '21c', '31c', '19', '173']}                    # PINN_ALLACT_SHAPES
F_WIDTH = {16: 12, 32: 24, 64: 48}
# static-depth instantiations: hp -> (PINN_FAST_LIST as {(nd, n2, lh): MT}, PINN_FAST_COMB_LIST as {(nd, lh): MT}), Tanh nets without skips
FAST = {64: ({(2, 2, 3): 1, (1, 0, 3): 3, (1, 0, 2): 3, (1, 0, 4): 3, (1, 1, 3): 2}, {(2, 3): 2, (2, 2): 2, (2, 4): 2, (3, 3): 1}),
        32: ({}, {}),
        16: ({(2, 2, 2): 1}, {(2, 2): 1})}
TEAMS2, BREADTH, SKIPS_LIGHT, PROGRAM, POLYBIT = 256, 8, 1024, 2048, 256       # PINN_VAR_* (pinn_kernel.h), PINN_ACT_TANH_POLYBIT
ACT_CODE = {'Tanh': 0, 'Sin': 2}


def _hp(features):
    width = max(features[:-1])
    return 16 if width <= 16 else 32 if width <= 32 else 64


def _tile_name(hp, shape, family='plain', lh=-1, act='Tanh', spec=0, program=False, accurate=False):
    """ the instantiation pinn_launch_tile_hp16 / _hp32 / _hp64 returns in the fp32 GEMM mode. shape = (nd, packed n2, combined); lh = hidden->hidden
    layers; act = the net's activation where one name carries all layers; spec = pinn_spec_of (1 Dirichlet box, 2 evolution in a box, 3 initial
    condition alone in 1-D) of the AFFINE residual, or with program=True of the residual program """
    nd, n2, comb = shape

    def name(mt, lhc, actc, var):
        return f'pinn_tile_kernel<{hp},{nd},{n2},{mt},{lhc},{actc},{"true" if comb else "false"},{var}>'
    if family == 'allact':
        return name(1, -1, -2, BREADTH)
    if family == 'light':
        return name(1, -1, -1, BREADTH | SKIPS_LIGHT)
    if family == 'heavy':
        if hp == 64 and comb and nd == 2 and lh == 3 and act == 'Sin':              # static 'Sin' nets of depth 4, no skips
            return name(1, 3, ACT_CODE['Sin'], TEAMS2 | 16) if spec == 1 and not program else name(1, 3, ACT_CODE['Sin'], BREADTH)
        return name(1, -1, -1, BREADTH)
    assert family == 'plain'
    tanh = act == 'Tanh'
    fast, fast_comb = FAST[hp]
    if comb:
        if hp == 64 and nd == 2 and lh == 3 and tanh and spec:                      # the two-team kernels (and the accurate-tanh twin: one team pair, MT 1)
            var = TEAMS2 | (spec << 4) | (PROGRAM if program else 0)
            return name(1, 3, POLYBIT if accurate and spec == 1 and not program else 0, var)
        if hp == 16 and nd == 2 and lh == 2 and tanh and spec == 1 and not program:
            return name(1, 2, 0, 16)
        if tanh and (nd, lh) in fast_comb:
            return name(fast_comb[(nd, lh)], lh, 0, 0)
        return name(1, -1, -1, 0)
    if hp == 64 and (nd, n2) == (1, 0) and lh == 3 and tanh and spec == 3 and not program:
        return name(2, 3, 0, (3 << 4) | TEAMS2)                                     # PINN_FAST_VAR_S2, PINN_CFG4_MT
    if tanh and (nd, n2, lh) in fast:
        return name(fast[(nd, n2, lh)], lh, 0, 0)
    return name(1, -1, -1, 0)


def _problem(key, layout, features, activation, bc=0.2, ic=None, domain=None):
    def make(D):
        eqs = dict(_equations(D))
        eqs.update(_more_equations(D))
        eq, ndims, nparams = eqs[key]
        kw = dict(ndims=ndims, layout=layout, features=list(features), activation=activation)
        if bc is not None:
            kw['boundary_condition'] = bc
        if ic is not None:
            kw['initial_condition'] = IC.get(ic, ic)
        if domain is not None:
            kw['domain'] = domain
        if nparams:
            kw['nparams'] = nparams
        return eq, kw
    return make


def _case(out, name, group, key, features, seed, n=53, act='Tanh', layout=None, family='plain', calls=None, bc=0.2, ic=None, domain=None,
          spec=0, program=False, accurate=False, shape=None):
    """ calls: None = one fused step on the kernel of the equation's stream shape; else the (nd, n2, combined) of each backward call of
    the generic path. act: one activation name for every layer (it enters the kernel's name), or a list """
    assert name not in out and max(features[:-1]) <= 64
    hp, lh = _hp(features), len(features) - 2
    layout = layout or 'fa ' * (lh + 1) + 'f'
    shapes = [shape or SHAPES.get(key) or MORE_SHAPES[key]] if calls is None else calls
    one_act = act if isinstance(act, str) else None
    # (a call of the generic path is a backward call: pinn_spec_of answers 0 outside PINN_MODE_STEP)
    kernels = [_tile_name(hp, s, family, lh, one_act, spec if calls is None else 0, program and calls is None, accurate) for s in shapes]
    out[name] = dict(group=group, hp=hp, problem=_problem(key, layout, features, act, bc, ic, domain), seed=seed, n=n, family=family,
                     path='fused' if calls is None else 'generic', lh=lh, features=list(features), kernels=kernels, accurate=accurate)


A_WIDTHS = (3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
C_N = {16: (1, 15, 16, 17, 33), 32: (1, 31, 32, 33, 63, 64, 65, 97), 48: (1, 47, 48, 49, 97), 'teams': (1, 15, 16, 17, 31, 32, 33, 49)}
# the two-team kernels, each through the smallest problem that reaches it: name -> _case keywords at width 64, four hidden layers
TWO_TEAM = {
    'cfg2': dict(key='21c', spec=1),
    'cfg2_prog': dict(key='box_prog', spec=1, program=True),
    'cfg2_sin': dict(key='21c', spec=1, act='Sin', family='heavy'),
    'evo2': dict(key='heat_xt', spec=2, bc=0.0, ic='sin'),
    'evo2_prog': dict(key='burgers', spec=2, program=True, bc=0.0, ic='sin'),
}
CFG4 = dict(key='ode_e', spec=3, bc=None, ic=1.0)


def _cases():
    out = {}
    w64 = lambda depth: [64] * depth + [1]
    # A: both sides of every padding and wave boundary; the Sigmoid side at depth 2 alone
    for width in A_WIDTHS:
        for depth, act in ((1, 'Tanh'), (2, 'Tanh'), (4, 'Tanh'), (2, 'Sigmoid')):
            _case(out, f'A/{width}x{depth}/{act}', 'A', '11', [width] * depth + [1], seed=width * 10 + depth, act=act)
    # B: rectangular real regions inside the bands; [16, 64, 16]: narrow real layers in a 64-wide padding
    for feats in ([64, 33, 64], [40, 64, 50], [32, 17, 32], [16, 5, 16], [10, 12, 15], [16, 64, 16]):
        _case(out, 'B/' + 'x'.join(map(str, feats)), 'B', '11', feats + [1], seed=sum(feats))
    # C: ragged batches per tile height
    for n in C_N[16]:
        _case(out, f'C/generic16/n{n}', 'C', '11', w64(2), seed=643, n=n)
    for n in C_N[32]:
        _case(out, f'C/static11/n{n}', 'C', '11', w64(4), seed=644, n=n)                              # (1, 1), MT 2
        for depth in (3, 4, 5):                                                                     # PINN_FAST_COMB_LIST, MT 2, spec 0
            _case(out, f'C/comb2x{depth}/n{n}', 'C', 'box_e', w64(depth), seed=650 + depth, n=n)
        _case(out, f'C/cfg4/n{n}', 'C', seed=645, n=n, features=w64(4), **CFG4)                        # two teams of 32-point tiles
    for n in C_N[48]:
        for depth in (3, 4, 5):                                                                     # (1, 0), MT 3: a boundary condition, no initial one
            _case(out, f'C/static10x{depth}/n{n}', 'C', '10', w64(depth), seed=660 + depth, n=n, spec=1)
    for which, kw in TWO_TEAM.items():
        for n in C_N['teams']:
            _case(out, f'C/{which}/n{n}', 'C', seed=670 + len(which), n=n, features=w64(4), **kw)
    # E: first layer and point-stage inputs
    for width in (24, 48):
        feats = [width] * 3 + [1]
        _case(out, f'E/{width}/param1', 'E', 'param1', feats, seed=width + 41)
        _case(out, f'E/{width}/col2', 'E', 'col2', feats, seed=width + 42)
        _case(out, f'E/{width}/uxy', 'E', 'uxy', feats, seed=width + 43)
        _case(out, f'E/{width}/uxy_var', 'E', 'uxy_var', feats, seed=width + 45)
        _case(out, f'E/{width}/uxxxy', 'E', 'uxxxy', feats, seed=width + 44, calls=[(1, 73, False)] * 4 + [(1, 9, False)])
        _case(out, f'E/{width}/five_columns', 'E', 'p5', feats, seed=width + 46, act='Sigmoid', bc=0.0, ic='bump', shape=P5_SHAPE)
        _case(out, f'E/{width}/shifted_domain', 'E', 'shifted', feats, seed=width + 47, bc=1.0, domain=(-1, 2), spec=1)
    # F: every stream shape in every family, at a depth for which the launcher holds no static kernel (plain: two hidden layers)
    for hp, width in F_WIDTH.items():
        for family, keys in FAMILY_SHAPES.items():
            layout, act = FAMILIES[family]
            feats = [width] * (2 if family == 'plain' else 3) + [1]
            for key in keys:
                calls = [SHAPES[key]] if key == '173' else None         # fourth order: the generic path, one backward call
                _case(out, f'F/{width}/{key}/{family}', 'F', key, feats, seed=1000 + 7 * len(out), act=act, layout=None if family == 'plain' else layout,
                      family=family, calls=calls, spec=1 if key == '21c' else 0)
    # G: static and specialised kernels, on their shape (the Dirichlet box, spec 1) and off it (spec 0)
    for depth in (3, 4, 5):
        _case(out, f'G/fast10x{depth}/box', 'G', '10', w64(depth), seed=700 + depth, spec=1)
        _case(out, f'G/fast10x{depth}/off', 'G', 'ode_e', w64(depth), seed=710 + depth)
        if depth != 4:                                                                              # depth 4 on the box is the cfg2 kernel
            _case(out, f'G/comb2x{depth}/box', 'G', '21c', w64(depth), seed=720 + depth, spec=1)
        _case(out, f'G/comb2x{depth}/off', 'G', 'box_e', w64(depth), seed=730 + depth)
    _case(out, 'G/fast22x4/box', 'G', '22', w64(4), seed=740)
    _case(out, 'G/fast22x4/off', 'G', '22', w64(4), seed=741, bc=0.0, ic='sin')
    _case(out, 'G/fast11x4/box', 'G', '11', w64(4), seed=742)
    _case(out, 'G/fast11x4/off', 'G', 'param1', w64(4), seed=743)
    _case(out, 'G/comb3x4/box', 'G', '31c', w64(4), seed=744)
    _case(out, 'G/comb3x4/off', 'G', '31c', w64(4), seed=745, bc=0.0, ic=lambda x, y: 10 * x * y * (1 - x) * (1 - y))
    hp16 = [16, 16, 16, 1]
    _case(out, 'G/hp16/fast22', 'G', '22', hp16, seed=750)
    _case(out, 'G/hp16/comb2/off', 'G', 'box_e', hp16, seed=751)
    _case(out, 'G/hp16/comb2/box', 'G', '21c', hp16, seed=752, spec=1)
    _case(out, 'G/hp16/cfg1', 'G', '21c', [10, 12, 15, 1], seed=753, spec=1, bc=1.0)
    for which, kw in TWO_TEAM.items():
        _case(out, f'G/{which}', 'G', seed=760 + len(which), features=w64(4), **kw)
    _case(out, 'G/sin/off', 'G', 'box_e', w64(4), seed=770, act='Sin', family='heavy')
    _case(out, 'G/sin/program', 'G', 'box_prog', w64(4), seed=771, act='Sin', family='heavy', spec=1, program=True)
    _case(out, 'G/cfg4', 'G', seed=772, features=w64(4), **CFG4)
    _case(out, 'G/accurate_tanh', 'G', '21c', w64(4), seed=773, spec=1, accurate=True)
    return out


# D(u, t) - a D(D(u, x), x) + b u - c: the coefficient of u_xx is a column, so the second derivative stays a stream of its own
P5_SHAPE = (2, 2, False)
CASES = _cases()


def _names(group):
    return [k for k, c in CASES.items() if c['group'] == group]


# ---- references: computed once per case, shared, left unchanged ------------------------------------------------------------------------------
def _case_reference(name, fp32=True):
    c = CASES[name]
    return _reference('w16_64/' + name, c['problem'], c['seed'], c['n'], fp32=fp32)


def _bands(i, n_tensors, arr):
    """ (label, array) of tensor i of export_grads order [W1, b1, ..., Wl, bl, log_scale]: the tensor itself and its bands (module docstring) """
    out = [(f'{i}', arr)]
    last = n_tensors - 3                # the output layer's matrix; n_tensors - 2 its bias, n_tensors - 1 log_scale
    if i > last:
        return out
    if arr.ndim == 1 or i == 0:         # a hidden bias, W1: the units of each wave
        for w in range(-(-arr.shape[0] // BAND)):
            out.append((f'{i}[wave{w}]', arr[BAND * w:BAND * (w + 1)]))
        return out
    if i < last:                        # hidden->hidden: the rows of each wave ...
        for w in range(-(-arr.shape[0] // BAND)):
            out.append((f'{i}[rows{w}]', arr[BAND * w:BAND * (w + 1), :]))
    for k in range(-(-arr.shape[1] // BAND)):       # ... and the inputs of each K tile
        out.append((f'{i}[cols{k}]', arr[:, BAND * k:BAND * (k + 1)]))
    return out


def _n_bands(features):
    """ bands with at least one entry, from the features alone: W1 and every hidden bias by waves, every hidden->hidden matrix by waves
    and by K tiles, the output row by K tiles """
    tiles = [-(-f // BAND) for f in features[:-1]]
    return tiles[0] + sum(tiles) + sum(a + b for a, b in zip(tiles[:-1], tiles[1:])) + tiles[-1]


def _at_the_floor(ref, case):
    """ labels of the gradient tensors / bands of the fp64 oracle whose norm is at or below the absolute floor of the rule """
    low = []
    for i, g in enumerate(ref['g64']):
        if g is None:
            continue
        for label, part in _bands(i, len(ref['g64']), g):
            if label in LEFT_OUT.get(case, {}):
                continue
            if float(np.linalg.norm(part)) <= 1e-9 * np.sqrt(part.size):
                low.append(label)
    return low


def _check_step(group, case, name, solver, ref):
    """ the rule of this file on the loss and the gradients the last step left in solver.grads; returns the number of bands checked """
    hp = solver.model.net.layout.hp
    assert _at_the_floor(ref, name) == [], case
    assert ref['relu_gap'] > 1e-4, (case, ref['relu_gap'])
    test = f'width{hp}_{group}'
    lay = solver.model.net.layout
    loss = float(solver.grads[lay.off_loss])
    ok, err, arb = close_or_arbitrated([loss], [ref['loss32']], lambda: [ref['loss64']], LOSS_RTOL, atol=0.0, k=2.0)
    record_margin(test, case, 'loss', err, LOSS_RTOL, arb)
    print(f'{case}: loss {loss!r} ref32 {ref["loss32"]!r} f64 {ref["loss64"]!r} err {err:.2e} arb={arb}')
    failed = [] if ok else [('loss', err)]
    got = export_grads(solver)
    n_bands = 0
    for i, (g, w32, w64) in enumerate(zip(got, ref['g32'], ref['g64'])):
        if w64 is None:
            assert float(np.abs(g).max()) == 0.0, (case, i)
            continue
        for (label, gp), (_, p32), (_, p64) in zip(_bands(i, len(got), g), _bands(i, len(got), w32), _bands(i, len(got), w64)):
            if label in LEFT_OUT.get(name, {}):
                continue
            ok, err, arb = close_or_arbitrated(gp, p32, lambda p64=p64: p64, GRAD_RTOL, k=2.0)
            record_margin(test, f'{case}[{label}]', 'band' if '[' in label else 'gradient', err, GRAD_RTOL, arb)
            print(f'{case}: grad {label} shape {gp.shape} err {err:.2e} arb={arb}')
            n_bands += '[' in label
            if not ok:
                failed.append((label, err))
    assert not failed, (case, failed)
    return n_bands


def _solver(pa, ref, hp, solver_kwargs, accurate=False):
    eq, kw = ref['problem'](pa.D)
    solver = pa.Solver(eq, **kw, **solver_kwargs)
    assert solver.model.net.layout.hp == hp
    load_params(solver, ref['start'])
    if accurate:
        solver.set_tanh_mode('accurate')
    return solver


def _run_case(pa, lib, name, solver_kwargs):
    """ one step of a case on its path: kernels by name, then the rule. Returns the solver. """
    c = CASES[name]
    ref = _case_reference(name)
    solver = _solver(pa, ref, c['hp'], solver_kwargs, c['accurate'])
    xs = torch.from_numpy(ref['pts'].copy()).to(solver.device)
    wgrad_before = lib.pinn_last_wgrad_kernel_name()
    if c['path'] == 'fused':
        assert solver.program is not None, solver.program_error
        solver._fused_step(xs, 1)
        ran = [lib.pinn_last_kernel_name().decode()]
    else:
        assert solver.program is None, name
        net, ran = solver.model.net, []
        backward = net.jet_backward

        def spy(*args, **kwargs):           # (the names are set on the host when a kernel is launched)
            result = backward(*args, **kwargs)
            ran.append(lib.pinn_last_kernel_name().decode())
            return result
        net.jet_backward = spy
        try:
            solver._generic_step(xs, ('equation',), [], torch.nn.MSELoss(), 1)
        finally:
            del net.jet_backward
    if solver.device.type == 'cuda':
        torch.cuda.synchronize()
    assert ran == c['kernels'], (name, ran, c['kernels'])
    # no weight-gradient partner at these widths: the process-wide 'last' name belongs to whoever streamed before, and stays
    assert lib.pinn_last_wgrad_kernel_name() == wgrad_before, name
    bands = _check_step(c['group'], name, name, solver, ref)
    assert bands == _n_bands(c['features']), (name, bands)
    return solver


# ---- CPU tier: no vacuous comparison; every instantiation of the launchers is in a case ---------------------------------------------------
@pytest.mark.parametrize('group', ['A', 'B', 'C', 'E', 'F', 'G'])
def test_no_reference_gradient_sits_at_the_floor(group):
    """ with the two oracles alone: no case leaves a gradient tensor, or a band of one, whose fp64 norm is at the absolute floor
    1e-9 sqrt(size) of the rule (it would pass whatever the kernel wrote); all references finite; no ReLU pre-activation within 1e-4 of
    zero (there is no ReLU layer: the hook of _reference answers inf). Group D's batch size comes from the device's grid: its cases assert
    the same there. """
    for name in _names(group):
        c = CASES[name]
        ref = _case_reference(name, fp32=False)
        assert _at_the_floor(ref, name) == [], name
        assert all(g is not None and np.isfinite(g).all() for g in ref['g64'][:-1]), name
        assert np.isfinite(ref['loss64']) and ref['relu_gap'] > 1e-4, (name, ref['relu_gap'])
        labels = [label for i, g in enumerate(ref['g64']) if g is not None for label, _ in _bands(i, len(ref['g64']), g) if '[' in label]
        assert len(labels) == _n_bands(c['features']), name
        for label in LEFT_OUT.get(name, {}):
            assert '[' in label, (name, label)                 # never a whole tensor
        for i, g in enumerate(ref['g64']):
            left = [label for label in LEFT_OUT.get(name, {}) if label.startswith(f'{i}[')]
            assert 8 * len(left) <= sum(label.startswith(f'{i}[') for label in labels), (name, left)       # at most one band in eight
    if group == 'A':            # full width: four waves and four K tiles of every hidden matrix
        assert _n_bands([64] * 4 + [1]) == 4 + 4 * 4 + 3 * 8 + 4 and _n_bands([3, 1]) == 3 and _n_bands([17, 17, 1]) == 2 + 4 + 4 + 2


# -- the launchers as pinn_inst.inc states them
def _preprocess(text, defined):
    """ the lines of `text` that the preprocessor keeps with the object-like macros `defined` (name -> replacement text), continuation lines
    joined, and the object-like macros the kept lines define. Conditions are integer expressions over macros; an unknown name counts as 0. """
    macros = dict(defined)

    def value(expr, depth=0):
        assert depth < 16, expr
        expr = re.sub(r'//.*|/\*.*?\*/', '', expr)
        expr = re.sub(r'defined\s*\(\s*(\w+)\s*\)|defined\s+(\w+)', lambda m: '1' if (m[1] or m[2]) in macros else '0', expr)
        expr = re.sub(r'PINN_VAR_SPEC\(([^()]*)\)', r'((\1) << 4)', expr)
        expr = re.sub(r'\b(true|false)\b', lambda m: '1' if m[1] == 'true' else '0', expr)
        expr = re.sub(r'[A-Za-z_]\w*', lambda m: str(value(macros[m[0]], depth + 1)) if macros.get(m[0], '').strip() else '0', expr)
        expr = re.sub(r'!(?!=)', ' not ', expr.replace('&&', ' and ').replace('||', ' or '))
        return int(eval(expr, {'__builtins__': {}}))            # (digits, operators and parentheses of this repository's own source file)

    kept, stack = [], []                # stack: [this branch active, a branch was taken, the enclosing region active]
    for line in re.sub(r'\\\n', ' ', text).split('\n'):
        s = line.strip()
        active = all(frame[0] for frame in stack)
        m = re.match(r'#\s*(ifdef|ifndef|if|elif|else|endif|define|undef)\b\s*(.*)', s)
        if not m:
            if active:
                kept.append(line)
            continue
        word, rest = m[1], m[2]
        if word in ('if', 'ifdef', 'ifndef'):
            cond = active and (value(rest) != 0 if word == 'if' else (rest.split()[0] in macros) == (word == 'ifdef'))
            stack.append([cond, cond, active])
        elif word == 'elif':
            frame = stack[-1]
            frame[0] = frame[2] and not frame[1] and value(rest) != 0
            frame[1] = frame[1] or frame[0]
        elif word == 'else':
            frame = stack[-1]
            frame[0] = frame[2] and not frame[1]
            frame[1] = True
        elif word == 'endif':
            stack.pop()
        elif active and word == 'define':
            d = re.match(r'(\w+)(\([^)]*\))?\s*(.*)', rest)
            macros[d[1] + (d[2] or '')] = re.sub(r'//.*', '', d[3]).strip()
            kept.append(line)
        elif active and word == 'undef':
            macros.pop(rest.split()[0], None)
    assert not stack
    return kept, macros, value


def _launcher_instantiations():
    """ hp -> the pinn_tile_kernel instantiations pinn_launch_tile_hp16 / _hp32 / _hp64 can return in the fp32 GEMM mode of the product
    build (no PINN_ONLY_BASELINE, no PINN_CHAIN), read from pinn_inst.inc: the launch_one<...> of the launcher's body, the macro lists
    PINN_FAST_LIST / PINN_FAST_COMB_LIST where the body expands them, PINN_BREADTH (first breadth set, and the second where
    PINN_ALLACT_SHAPES holds the shape), and the named pinn_launch_*_hp64 functions of the width's own translation unit. The split-bf16
    launchers (pinn_launch_split_*) belong to test_split_bf16.py. Also returns the macros of the HP 64 unit. """
    with open(os.path.join(ROOT, 'pydens_amd', 'csrc', 'pinn_inst.inc')) as f:
        text = f.read()
    with open(os.path.join(ROOT, 'pydens_amd', 'csrc', 'pinn_kernel.h')) as f:
        consts = dict(re.findall(r'\b(PINN_VAR_[A-Z0-9_]+) = (\d+)', f.read()))
    with open(os.path.join(ROOT, 'include', 'pinn.h')) as f:
        consts.update(re.findall(r'#define (PINN_ACT_\w+)\s+(\d+)', f.read()))
    consts['PINN_ACT_TANH_POLYBIT'] = str(POLYBIT)
    assert consts['PINN_VAR_TEAMS2'] == '256' and consts['PINN_ACT_SIN'] == '2'
    allact = {(int(a), int(b), c == 'true') for a, b, c in
              re.findall(r'X\((\d+), (\d+), (true|false)\)', re.search(r'#define PINN_ALLACT_SHAPES\(X\)(.*)', text).group(1))}

    def one(args, value, hp):
        """ name of launch_one<ND, N2, LHC, ACTC, MT, COMB = false, VAR = 0> """
        v = [value(a) for a in args] + [0, 0][len(args) - 5:]
        return f'pinn_tile_kernel<{hp},{v[0]},{v[1]},{v[4]},{v[2]},{v[3]},{"true" if v[5] else "false"},{v[6]}>'

    own, _, own_value = _preprocess(text, dict(consts, PINN_INST_HP='64', PINN_INST_OWN='1'))
    named = {m[0]: one(m[1].split(','), own_value, 64) for m in
             re.findall(r'int (pinn_launch_\w+_hp64)\(const PinnKArgs\* a, const PinnLaunchReq& req\) \{\s*return launch_one<([^;]*)>\(a, req\);', '\n'.join(own))}
    built, macros64 = {}, None
    for hp in (16, 32, 64):
        kept, macros, value = _preprocess(text, dict(consts, PINN_INST_HP=str(hp)))
        body = '\n'.join(line for line in kept if not line.lstrip().startswith('#'))
        body = body[body.index('int PINN_CAT(pinn_launch_tile_hp, PINN_INST_HP)'):]
        assert 'launch_chain' not in body and 'launch_wide_spec' not in body
        names = {one(args.split(','), value, hp) for args in re.findall(r'launch_one<([^;]*?)>\(a, req\)', body)}
        for nd, n2, comb in re.findall(r'PINN_BREADTH\((\d+), (\d+), (true|false)\)', body):
            shape = (int(nd), int(n2), comb == 'true')
            names.add(one([nd, n2, '-1', '-1', '1', comb, 'PINN_VAR_BREADTH'], value, hp))
            if shape in allact:
                names.add(one([nd, n2, '-1', '-2', '1', comb, 'PINN_VAR_BREADTH'], value, hp))
        if 'PINN_FAST_LIST(PINN_TRY_FAST)' in body:
            for args in re.findall(r'X\(([^()]*)\)', macros['PINN_FAST_LIST(X)']):
                nd, n2, lh, act, mt = args.split(',')
                names.add(one([nd, n2, lh, act, mt], value, hp))
        if 'PINN_FAST_COMB_LIST(PINN_TRY_FAST_COMB)' in body:
            for args in re.findall(r'X\(([^()]*)\)', macros['PINN_FAST_COMB_LIST(X)']):
                nd, lh, act, mt, var = args.split(',')
                names.add(one([nd, '1', lh, act, mt, 'true', var], value, hp))
        for fn in set(re.findall(r'return (pinn_launch_\w+)\(a, req\)', body)):
            if 'split' not in fn:
                names.add(named[fn])
        built[hp] = names
        if hp == 64:
            macros64 = (macros, value)
    return built, macros64


def test_every_tile_instantiation_is_in_a_case():
    """ the instantiations the launchers hold against the names the cases assert (every kernel case asserts the exact name of every call):
    a kernel added to a launcher later shows up here as untested, and one that nothing reaches stands in UNREACHABLE with the line that
    shadows it -- which is looked up in the file, and whose switches are evaluated """
    built, (macros, value) = _launcher_instantiations()
    generic = 14 + 4 + 14 + 9           # plain, light skips, first breadth set, second
    assert len(built[32]) == generic and len(built[16]) == generic + 3 and len(built[64]) == generic + 9 + 2 + 5 + 1 + 1, {k: len(v) for k, v in built.items()}
    for hp in (16, 32, 64):
        asserted = {k for c in CASES.values() if c['hp'] == hp for k in c['kernels']}
        unreachable = {k for k in UNREACHABLE if k.startswith(f'pinn_tile_kernel<{hp},')}
        assert built[hp] - asserted == unreachable, hp
        assert asserted - built[hp] == set(), hp
    with open(os.path.join(ROOT, 'pydens_amd', 'csrc', 'pinn_inst.inc')) as f:
        text = f.read()
    for name, line in UNREACHABLE.items():
        assert line in text, name
    assert value('PINN_SIN_TEAMS') == 1 and value('PINN_SIN_MT') == 1, 'the one-team Sin kernel is reachable again: give it a case'


# ---- A, B, C, E, F, G on the emulator (CPU tier) and on the device --------------------------------------------------------------------------
# Thinned on the emulator side only (the gpu twins run every case): of group C the largest batch of each tile height and the second multiple
# of the 32-point and two-team rounds stay behind PYDENS_AMD_SLOW_EMU=1 -- 2.5 to 5 s each, 28 cases, 70 of the file's 147 s on one core.
# One point either side of the FIRST multiple of every tile height, and one past the second, stay on the CPU tier for every kernel.
C_THINNED = {'n63', 'n64', 'n97', 'n31', 'n32'}
SLOW_ON_THE_EMULATOR = [k for k in CASES if k.startswith('C/') and k.rsplit('/', 1)[1] in C_THINNED
                        and not (k.startswith(('C/static11/', 'C/comb2', 'C/cfg4/')) and k.endswith(('/n31', '/n32')))]


def _emu(pa, emu_lib, name):
    _run_case(pa, emu_lib, name, dict(_lib=emu_lib, device='cpu'))


def _quick(group):
    return [k for k in _names(group) if k not in SLOW_ON_THE_EMULATOR]


@pytest.mark.parametrize('name', _quick('A') + _quick('B'))
def test_units_and_unequal_layers_on_the_emulator(pa, emu_lib, name):
    _emu(pa, emu_lib, name)


@pytest.mark.parametrize('name', _quick('C'))
def test_ragged_batches_per_tile_height_on_the_emulator(pa, emu_lib, name):
    _emu(pa, emu_lib, name)


@pytest.mark.parametrize('name', _quick('E'))
def test_first_layer_and_point_stage_inputs_on_the_emulator(pa, emu_lib, name):
    _emu(pa, emu_lib, name)


@pytest.mark.parametrize('name', _quick('F'))
def test_every_stream_shape_in_every_family_on_the_emulator(pa, emu_lib, name):
    _emu(pa, emu_lib, name)


@pytest.mark.parametrize('name', _quick('G'))
def test_static_and_specialised_kernels_on_the_emulator(pa, emu_lib, name):
    _emu(pa, emu_lib, name)


@slow_emu
@pytest.mark.parametrize('name', SLOW_ON_THE_EMULATOR)
def test_thinned_ragged_batches_on_the_emulator(pa, emu_lib, name):
    _emu(pa, emu_lib, name)


@gpu
@pytest.mark.parametrize('name', _names('A'))
def test_every_unit_of_widths_up_to_64_on_the_gpu(pa, dev, name):
    """ A: hidden layers exactly `width` wide, both sides of every padding (16, 32, 64) and wave (16, 32, 48) boundary; one, two and four of
    them (Tanh; Sigmoid at two), 53 points (three full 16-point tiles and a ragged one) on the (1, 1) kernels: generic depth, and at four
    Tanh layers of HP 64 the static 32-point kernel """
    _run_case(pa, dev, name, {})


@gpu
@pytest.mark.parametrize('name', _names('B'))
def test_unequal_layers_inside_the_bands_on_the_gpu(pa, dev, name):
    """ B: rectangular real regions inside the bands; 16 x 64 x 16 puts narrow real layers into a 64-wide padding """
    _run_case(pa, dev, name, {})


@gpu
@pytest.mark.parametrize('name', _names('C'))
def test_ragged_batches_per_tile_height_on_the_gpu(pa, dev, name):
    """ C: one point either side of every multiple of the tile height that fits 100 points, per kernel: 16 points (generic), 32 (static
    (1, 1), the combined kernels with MT = 2, the two-team kernel of config 4 at 64 points per workgroup round), 48 ((1, 0) at three depths),
    and the five two-team 16-point kernels: team 1 with nothing, team 1 ragged, an odd tile count """
    _run_case(pa, dev, name, {})


@gpu
@pytest.mark.parametrize('name', _names('E'))
def test_first_layer_and_point_stage_inputs_on_the_gpu(pa, dev, name):
    """ E: a parameter column (d > nd), a derivative in the second column alone, a diagonal direction, weighted diagonals, five input
    columns, a shifted domain """
    _run_case(pa, dev, name, {})


@gpu
@pytest.mark.parametrize('name', _names('F'))
def test_every_stream_shape_in_every_family_on_the_gpu(pa, dev, name):
    """ F: every (shape, family) pair of the generic-depth instantiations, widths 12, 24 and 48 """
    _run_case(pa, dev, name, {})


@gpu
@pytest.mark.parametrize('name', _names('G'))
def test_static_and_specialised_kernels_on_the_gpu(pa, dev, name):
    """ G: every static-depth and shape-specialised instantiation, on the Dirichlet box and off it, at full width """
    _run_case(pa, dev, name, {})


# ---- D: the tile loop -----------------------------------------------------------------------------------------------------------------------
# which -> (_case keywords, points per tile, teams): the generic 16-point kernel, a 48-point kernel, the two-team kernel of BASELINE config 2
D_KERNELS = {
    'generic16': (dict(key='11', features=[64, 64, 1]), 16, 1),
    'static10x4': (dict(key='10', features=[64] * 4 + [1], spec=1), 48, 1),
    'cfg2': (dict(features=[64] * 4 + [1], **TWO_TEAM['cfg2']), 16, 2),
}
_D = {}


def _tile_loop_case(pa, lib, which):
    """ (case, reference, grid, n) of group D. make_plan (pinn_abi.cpp) sizes the persistent grid as CUs x workgroups per CU, capped by the
    number of workgroup rounds; a workgroup takes `teams` tiles of `pts` points per round. `grid` is read from the launch info of a probe
    launch large enough to fill the device; n = pts (2 teams grid) + 3: every workgroup, and both teams of a two-team one, runs a second
    tile with the accumulators carried over; team 0 of workgroup 0 a third, ragged one """
    kw, pts, teams = D_KERNELS[which]
    cases = {}
    _case(cases, which, 'D', seed=5000 + len(which), **kw)
    c = cases[which]
    if which not in _D:
        probe_eq, probe_kw = c['problem'](pa.D)
        probe = pa.Solver(probe_eq, **probe_kw)
        n_probe = pts * teams * 8 * torch.cuda.get_device_properties(0).multi_processor_count        # more rounds than any grid (at most 4 workgroups per CU)
        probe._fused_step(torch.from_numpy(np.random.RandomState(21).rand(n_probe, probe.model.total).astype(np.float32)).cuda(), 1)
        torch.cuda.synchronize()
        assert lib.pinn_last_kernel_name().decode() == c['kernels'][0]
        _D[which] = _launch_info(lib)
    grid = _D[which]['grid']
    n = pts * (2 * teams * grid) + 3
    ref = _reference(f'w16_64/D/{which}', c['problem'], c['seed'], n, chunk=1024)
    return c, ref, grid, n


@gpu
@pytest.mark.parametrize('which', list(D_KERNELS))
def test_every_workgroup_runs_a_second_tile_on_the_gpu(pa, dev, which):
    """ D: the weight-gradient accumulators, bias rows and first / last-layer rows carried across the tile loop, through pinn_reduce_rows:
    the generic 16-point kernel at 64 x 64, the static 48-point (1, 0) kernel at 4 x 64, and both teams of the cfg2 kernel """
    kw, pts, teams = D_KERNELS[which]
    c, ref, grid, n = _tile_loop_case(pa, dev, which)
    solver = _solver(pa, ref, 64, {})
    assert solver.program is not None, solver.program_error
    wgrad_before = dev.pinn_last_wgrad_kernel_name()
    solver._fused_step(torch.from_numpy(ref['pts'].copy()).cuda(), 1)
    torch.cuda.synchronize()
    info = _launch_info(dev)
    rounds = -(-n // (pts * teams))
    print(f'D/{which}: n {n}, workgroup rounds {rounds}, launch info {info}')
    assert info['grid'] == grid and rounds > 2 * grid and n % pts == 3
    assert dev.pinn_last_kernel_name().decode() == c['kernels'][0]
    assert dev.pinn_last_wgrad_kernel_name() == wgrad_before
    assert _check_step('D', f'D/{which}/n{n}', which, solver, ref) == _n_bands(c['features'])
