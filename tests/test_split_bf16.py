""" The split-bf16 kernels (gemm mode 'bf16x3': pinn_launch_split_hp64_1 / _hp64_2 / _hp128 / _hp256 and pinn_launch_wgrad_split_hp128 / 256)
away from the four BASELINE shapes: padded and mixed widths, depths 1 .. 8, Sigmoid and per-layer Tanh / Sigmoid mixes (the run-time
activation form), ragged tiles, the tile loop of every workgroup and team, chunked slabs, weights whose bf16 `hi` planes cancel -- each
against the fp64 oracle, per FRAGMENT of the split data and not only per tensor.

Reference and rule (one for the whole file, taken from test_width_512.py): every case builds oracle.pinn_oracle.OracleSolver twice from one
seeded fp32 start (fp32 and fp64), loads that start into pa.Solver, sets 'bf16x3' and runs ONE _fused_step. The loss (1e-5, no floor) and
the gradient of every parameter tensor (helpers.GRAD_RTOL, floor 1e-9 per entry) go through helpers.close_or_arbitrated, k = 2 against fp64,
and so does
  (a) every 16-unit group of every bias gradient and the matching 16 rows of every weight gradient: where an error of one forward fragment
      (l, dir 0, kb, j) or one data-gradient fragment (l, dir 1, kb, j) of the split weights lands first, and
  (b) every 16 x 32 block [16 j .., 32 kb ..] of every hidden->hidden gradient, cut at the real width: the output granularity of the split
      weight-gradient GEMM.
A part whose fp64 norm sits at its floor 1e-9 sqrt(size) would pass vacuously: there is none (test_no_reference_part_sits_at_the_floor on the
CPU tier with the fp64 oracle alone, and again in every kernel case). The oracles are computed once per case (_reference) and shared, unchanged.

The rule is shown to FAIL on a subtly wrong kernel: emulator builds with PINN_SP_NPROD=5 (the lo x hi product dropped: 2^-17 of the products
of every fragment) and =3 (no i + j = 2 product) run the width-64 cases D and G (and, behind PYDENS_AMD_SLOW_EMU=1, one case A and one case G
of the width-128 kernel). Measured figures: profiles/r12_split_bf16.txt.

Kernel cases are marked gpu; the emulator twins of the width-64 cases and one single-tile width-128 case run on the CPU tier, the other
emulator twins at widths 128 / 256 need PYDENS_AMD_SLOW_EMU=1. """
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import rel_l2
from helpers import GRAD_RTOL, close_or_arbitrated, export_grads, load_params, ran_split_kernel, record_margin

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))

gpu = pytest.mark.gpu
slow_emu = pytest.mark.skipif(os.environ.get('PYDENS_AMD_SLOW_EMU') != '1',
                              reason='a 128 / 256-wide split tile costs the emulator tens of seconds: PYDENS_AMD_SLOW_EMU=1, or the -m gpu twin')
LOSS_RTOL = 1e-5
K_RULE = 2.0                # the project's arbitration factor (helpers.close_or_arbitrated)
# case G alone (ISSUE "Numbers"): k = measured worst ratio of the shipped kernels x 1.5, one digit, rounded up -- see profiles/r12_split_bf16.txt
K_G = 2.0
PI = math.pi


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


def _emu(**kwargs):
    import build_emu
    from pydens_amd import engine
    lib = engine.bind(ctypes.CDLL(build_emu.build(**kwargs)))
    assert lib.pinn_backend() == b'emu-host'
    return lib


@pytest.fixture(scope='module')
def emu_lib():
    return _emu()


_MUTANT_LIBS = {}


def _mutant(flag, tag, widths):
    """ an emulator library whose split units of `widths` are built with `flag`; built once, cached under its tag """
    key = (tag, widths)
    if key not in _MUTANT_LIBS:
        _MUTANT_LIBS[key] = _emu(extra_flags=(flag,), tag=tag, widths=widths)
    return _MUTANT_LIBS[key]


# ---- the problems: one per split kernel (and a second equation for the two wide ones) ------------------------------------------------------------
# kernel -> (HP, ND, MT, VAR) of pinn_tile_kernel<HP,ND,1,MT,LHC,ACTC,true|false,VAR>
KERNELS = {
    's64_1': dict(hp=64, head='64,2,1,1,3,0,true,784'),             # Poisson box, two teams of 16-point tiles (256 | 16 | 512)
    's64_2': dict(hp=64, head='64,1,0,2,3,0,false,816'),            # ODE family, two teams of 32-point tiles (256 | 48 | 512)
    's128': dict(hp=128, head='128,3,1,1,-1,{act},true,672'),        # heat shape in (x, y, t) (32 | 128 | 512)
    's256': dict(hp=256, head='256,2,1,1,-1,{act},true,672'),        # wave / evolution shape in (x, t)
}


def _problem(which, layout, features, activation):
    """ D -> (equation, Solver kwargs); `low` / `high` of the sampled points ride along in PROBLEM_BOX """
    net = dict(layout=layout, features=list(features), activation=activation)

    def make(D):
        if which == 'poisson':                  # BASELINE config 2's problem
            return (lambda f, x, y: D(D(f, x), x) + D(D(f, y), y) - 5 * torch.sin(PI * (x + y))), dict(ndims=2, boundary_condition=1, **net)
        if which == 'ode':                      # BASELINE config 4's problem
            return (lambda f, x, e: D(f, x) - e * PI * torch.cos(e * PI * x)), dict(ndims=1, nparams=1, initial_condition=1, **net)
        if which == 'heat3':                    # heat shape in (x, y, t), constant BC, callable IC as in BASELINE config 3
            return ((lambda f, x, y, t: D(D(f, x), x) + D(D(f, y), y) - D(f, t)),
                    dict(ndims=3, boundary_condition=0, initial_condition=lambda x, y: 10 * x * y * (1 - x) * (1 - y), **net))
        if which == 'heat3_src':                # ... with a source term in x alone
            return ((lambda f, x, y, t: D(D(f, x), x) + D(D(f, y), y) - D(f, t) - torch.sin(3.0 * x)),
                    dict(ndims=3, boundary_condition=0.1, initial_condition=lambda x, y: 10 * x * y * (1 - x) * (1 - y), **net))
        if which == 'wave':                     # wave shape in (x, t)
            return ((lambda f, x, t: D(D(f, t), t) - D(D(f, x), x)),
                    dict(ndims=2, boundary_condition=0, initial_condition=lambda x: x * (1 - x), **net))
        assert which == 'heat1'                 # 1-D heat with a source: the `heat64` equation of pinn_configs
        return ((lambda f, x, t: D(f, t) - 0.3 * D(D(f, x), x) - 2.0 * torch.exp(-t) * torch.sin(PI * x)),
                dict(ndims=2, boundary_condition=0, initial_condition=lambda x: torch.sin(PI * x), **net))
    return make


PROBLEM_BOX = {'poisson': ([0, 0], [1, 1]), 'ode': ([0, 1], [1, 5]), 'heat3': ([0, 0, 0], [1, 1, 1]), 'heat3_src': ([0, 0, 0], [1, 1, 1]),
               'wave': ([0, 0], [1, 1]), 'heat1': ([0, 0], [1, 1])}
KERNEL_OF = {'poisson': 's64_1', 'ode': 's64_2', 'heat3': 's128', 'heat3_src': 's128', 'wave': 's256', 'heat1': 's256'}


def _case(group, which, widths, acts='Tanh', n=53, seed=None, cancel=False):
    widths = list(widths)
    static = acts == 'Tanh' or (isinstance(acts, list) and all(a == 'Tanh' for a in acts))
    seed = seed if seed is not None else 7 * sum(widths) + len(widths) + (0 if static else 1000)
    return dict(group=group, which=which, kernel=KERNEL_OF[which], widths=widths, acts=acts, static=static, n=n, seed=seed, cancel=cancel,
                lh=len(widths) - 1, problem=_problem(which, 'fa' * len(widths) + 'f', widths + [1], acts))


RAGGED = (1, 15, 16, 17, 31, 33)


def _cases():
    """ name -> case. Case F (n from the device's grid) is built in its own test. """
    out = {}
    # A: widths and depths on the width-128 kernel (the depth-2 ones with the source term)
    for width in (65, 100, 127, 128):
        for depth in (1, 2, 3):
            out[f'A/{width}x{depth}'] = _case('A', 'heat3_src' if depth == 2 else 'heat3', [width] * depth)
    for width in (72, 128):
        out[f'A/{width}x8'] = _case('A', 'heat3', [width] * 8)
    for feats in ([128, 72, 128], [80, 128, 100]):
        out['A/' + 'x'.join(map(str, feats))] = _case('A', 'heat3', feats)
    out['A/100x2/n16'] = _case('A-emu', 'heat3_src', [100, 100], n=16)             # (the default tier's single-tile width-128 case)
    # B: widths and depths on the width-256 kernel (the depth-2 ones on the 1-D heat equation with its source)
    for width in (129, 200, 255, 256):
        for depth in (1, 2, 3):
            out[f'B/{width}x{depth}'] = _case('B', 'heat1' if depth == 2 else 'wave', [width] * depth)
    out['B/256x130x256'] = _case('B', 'wave', [256, 130, 256])
    out['B/200x2/n16'] = _case('B-emu', 'heat1', [200, 200], n=16)
    # C: activations on both wide kernels, one padded and one full width each
    for which, widths in (('heat3', (100, 128)), ('wave', (200, 256))):
        for width in widths:
            for tag, acts in (('tanh', 'Tanh'), ('sigmoid', 'Sigmoid'), ('tst', ['Tanh', 'Sigmoid', 'Tanh']), ('sts', ['Sigmoid', 'Tanh', 'Sigmoid'])):
                out[f'C/{KERNEL_OF[which]}/{width}/{tag}'] = _case('C', which, [width] * 3, acts)
    out['C/s128/100/sts/n16'] = _case('C-emu', 'heat3', [100] * 3, ['Sigmoid', 'Tanh', 'Sigmoid'], n=16)
    # D: the two width-64 kernels ('fa fa fa fa f', Tanh) at padded and mixed widths; the emulator twins at one or two tiles
    for which in ('poisson', 'ode'):
        for feats in ([33] * 4, [48] * 4, [63] * 4, [64] * 4, [64, 40, 64, 33]):
            tag = 'x'.join(map(str, feats)) if len(set(feats)) > 1 else f'{feats[0]}x4'
            out[f'D/{which}/{tag}'] = _case('D', which, feats)
            out[f'D/{which}/{tag}/emu'] = _case('D-emu', which, feats, n=17 if feats[0] in (33, 64) and len(set(feats)) == 1 else 16,
                                                seed=7 * sum(feats) + 4)
    # E: ragged tiles on all four kernels
    for which, feats in (('poisson', [64] * 4), ('ode', [48] * 4), ('heat3', [100] * 2), ('wave', [200] * 2)):
        for n in RAGGED:
            out[f'E/{KERNEL_OF[which]}/n{n}'] = _case('E', which, feats, n=n, seed=900 + sum(feats))
    # G: the lower planes carry the answer -- one per kernel (and an emulator twin of the wide ones on one tile)
    for which, feats in (('poisson', [64] * 4), ('ode', [64] * 4), ('heat3', [128] * 3), ('wave', [256] * 3)):
        out[f'G/{KERNEL_OF[which]}'] = _case('G', which, feats, cancel=True, seed=1200 + feats[0])
    out['G/s64_1/emu'] = _case('G-emu', 'poisson', [64] * 4, cancel=True, seed=1264, n=17)
    out['G/s64_2/emu'] = _case('G-emu', 'ode', [64] * 4, cancel=True, seed=1264, n=33)
    out['G/s128/emu'] = _case('G-emu-wide', 'heat3', [128] * 3, cancel=True, seed=1328, n=16)
    return out


CASES = _cases()
# negative dispatch: the shapes NEXT to the split width-64 kernels -- no split kernel, the fp32 mode's buffer bit for bit
NEGATIVE = {f'{which}/{tag}': _case('D-neg', which, feats, acts)
            for which in ('poisson', 'ode')
            for tag, feats, acts in (('depth3', [64] * 3, 'Tanh'), ('depth5', [64] * 5, 'Tanh'), ('sigmoid', [64] * 4, 'Sigmoid'))}


def _names(*groups):
    return [k for k, c in CASES.items() if c['group'] in groups]


# ---- case G: weights whose `hi` planes cancel ----------------------------------------------------------------------------------------------------
def _bf16_exact(x):
    """ x rounded to the nearest bf16 (an fp32 whose lower 16 bits are zero): a value that lives in the `hi` plane alone """
    b = np.asarray(x, dtype=np.float32).view(np.uint32)
    return (((b + np.uint32(0x8000)) & np.uint32(0xffff0000))).view(np.float32)


def _hadamard_row(r, n):
    """ row r of the Sylvester-Hadamard matrix, first n entries: (-1)^popcount(r & i) """
    return np.array([1.0 - 2.0 * (bin(r & i).count('1') & 1) for i in range(n)])


def _cancelling_start(start):
    """ the seeded start rebuilt so that every hidden pre-activation sum cancels in its `hi x hi` products:
      first layer   every unit = the mean unit of the start, moved by 2^-6 of the start's own deviation: near-identical units;
      hidden W[j,k] = t[j] s[k] c (1 + 2^-9 e1[j,k] + 2^-17 e2[j,k]): c = 1.5 2^e next to the mean |entry| of the start's matrix (bf16-exact, the
                    middle of its binade: the `hi` plane is +-c whatever the perturbation), t and s two rows of the Hadamard matrix, different
                    in every layer (so s is orthogonal to the t of the layer before, whose pattern the activations carry, and t to the s of the
                    layer behind, whose pattern the data gradients carry), e1 / e2 in [-1, 1] from the start's own entries: the perturbations
                    live in the `mid` and the `lo` plane;
      hidden b      the mean bias of the start, moved likewise: the next layer's input stays near-identical;
      last layer    every weight the mean |weight| of the start, moved likewise (near-identical data gradients going back).
    sum_k W[j,k] h[k] = t[j] c (sum_k s[k] h[k] + 2^-9 ...): the first sum is about 2^-6 / sqrt(K) of sum |W h|, what is left of it is decided
    by `mid`, `lo` and the products with i + j = 2. """
    out = [np.array(a, dtype=np.float32, copy=True) for a in start]
    n_lin = (len(out) - 1) // 2
    width = out[2].shape[1]
    shrink = np.float32({64: 2.0 ** -6, 128: 2.0 ** -3, 256: 2.0 ** -2}[width])          # (the sum over K units cancels like 1 / sqrt(K): the same ratio at every width)

    def near_identical(a, axis_mean, floor):
        mean = a.mean(axis=axis_mean, keepdims=True)
        mean = np.where(np.abs(mean) < floor, np.float32(floor), mean).astype(np.float32)
        return (mean + shrink * (a - a.mean(axis=axis_mean, keepdims=True))).astype(np.float32)
    out[0] = near_identical(out[0], 0, 0.3)                     # [h, d]: the same row everywhere, up to 2^-6 of the spread
    out[1] = near_identical(out[1], 0, 0.1)
    for l in range(1, n_lin - 1):
        w = out[2 * l]
        c = np.float32(1.5 * 2.0 ** math.floor(math.log2(float(np.abs(w).mean()) * 2.0)))
        e1 = w / np.abs(w).max()
        e2 = np.roll(e1, 1, axis=1)[::-1]
        sign = np.outer(_hadamard_row(3 * l + 1, w.shape[0]), _hadamard_row(3 * l + 2, w.shape[1]))
        out[2 * l] = (sign * c * (1.0 + 2.0 ** -9 * e1.astype(np.float64) + 2.0 ** -17 * e2.astype(np.float64))).astype(np.float32)
        out[2 * l + 1] = near_identical(out[2 * l + 1], 0, 0.1)
    last = 2 * (n_lin - 1)
    out[last] = near_identical(np.abs(out[last]), 1, 0.05)
    return out


def _cancellation(ref):
    """ per hidden->hidden layer: median over (point, unit) of |sum_k W[j,k] h[k]| / sum_k |W[j,k] h[k]|, in fp64 from the case's start """
    start, pts = ref['start'], np.asarray(ref['pts'], dtype=np.float64)
    n_lin = (len(start) - 1) // 2
    acts = ref['case']['acts']
    acts = [acts] * n_lin if isinstance(acts, str) else list(acts)
    h, out = pts, []
    for l in range(n_lin - 1):
        w, b = np.asarray(start[2 * l], dtype=np.float64), np.asarray(start[2 * l + 1], dtype=np.float64)
        if l > 0:
            out.append(float(np.median(np.abs(h @ w.T) / (np.abs(h) @ np.abs(w).T))))
        z = h @ w.T + b
        h = np.tanh(z) if acts[l] == 'Tanh' else 1.0 / (1.0 + np.exp(-z))
    return out


# ---- references: computed once per case, shared, left unchanged -----------------------------------------------------------------------------------
_REF = {}


def _points(n, which, seed=21):
    low, high = (np.asarray(v, dtype=np.float64) for v in PROBLEM_BOX[which])
    return (low + (high - low) * np.random.RandomState(seed).rand(n, len(low))).astype(np.float32)


def _reference(name, case, n=None, chunk=None, fp32=True):
    """ dict(start, pts, loss32, g32, loss64, g64): the fp32 and the fp64 oracle from one seeded fp32 start, one evaluation each
    (fp32=False: the fp64 side alone, for the CPU tier's look at the floors; the fp32 side is added when a kernel case asks for it) """
    n = n or case['n']
    key = (name, n)
    if key not in _REF:
        from oracle import pinn_oracle as po
        torch.manual_seed(case['seed'])
        eq, kw = case['problem'](po.D)
        o32 = po.OracleSolver(eq, **kw)
        o64 = po.OracleSolver(eq, dtype=torch.float64, **kw)
        start = o32.export_params()
        if case['cancel']:
            start = _cancelling_start(start)
            o32.import_params(start)
        o64.import_params(start)
        pts = _points(n, case['which'])
        ev64 = o64.evaluate(pts, chunk=chunk)
        _REF[key] = dict(start=start, pts=pts, loss64=ev64['loss'], g64=o64.export_grads(), o32=o32, chunk=chunk, case=case)
    ref = _REF[key]
    if fp32 and 'g32' not in ref:
        ev32 = ref['o32'].evaluate(ref['pts'], chunk=ref['chunk'])
        ref['loss32'], ref['g32'] = ev32['loss'], ref['o32'].export_grads()
    return ref


def _case_reference(name, fp32=True):
    return _reference(name, CASES[name], fp32=fp32)


# ---- the rule --------------------------------------------------------------------------------------------------------------------------------------
def _parts(i, n_tensors, arr):
    """ (label, kind, array) of tensor i of export_grads order [W1, b1, ..., Wl, bl, log_scale]: the tensor itself; (a) its 16-unit groups
    (bias entries / weight rows 16 j ..); (b) for a hidden->hidden matrix its 16 x 32 blocks [16 j .., 32 kb ..], cut at the real width """
    out = [(f'{i}', 'gradient', arr)]
    if i == n_tensors - 1 or arr.ndim == 0:
        return out
    units = arr.shape[0]
    if units > 16:
        for j in range((units + 15) // 16):
            out.append((f'{i}/u{j}', 'group', arr[16 * j:16 * j + 16]))
    if arr.ndim == 2 and 0 < i < n_tensors - 3:
        for j in range((units + 15) // 16):
            for kb in range((arr.shape[1] + 31) // 32):
                out.append((f'{i}[{j},{kb}]', 'block', arr[16 * j:16 * j + 16, 32 * kb:32 * kb + 32]))
    return out


def _at_the_floor(ref):
    """ labels of the parts of the fp64 oracle's gradients whose norm is below the absolute floor of the rule """
    low = []
    for i, g in enumerate(ref['g64']):
        if g is None:
            continue
        for label, _, part in _parts(i, len(ref['g64']), g):
            if float(np.linalg.norm(part)) <= 1e-9 * np.sqrt(part.size):
                low.append(label)
    return low


def _ratio(got, w32, w64):
    """ |ours - fp64| / |oracle32 - fp64| of one part (the quantity DESIGN quotes as 1.18x on trained models) """
    c = np.asarray(w64, dtype=np.float64).ravel()
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64).ravel() - c)) / max(float(np.linalg.norm(np.asarray(w32, dtype=np.float64).ravel() - c)), 1e-300)


def _rule(case, solver, ref, k=K_RULE, record=None):
    """ the rule of this file on what the last step left in solver.grads. Returns (failed parts, summary): nothing asserted here, so that
    the wrong builds can be shown to fail it. record: the group name for helpers.record_margin (None: nothing is recorded) """
    lay = solver.model.net.layout
    loss = float(solver.grads[lay.off_loss])
    ok, err, arb = close_or_arbitrated([loss], [ref['loss32']], lambda: [ref['loss64']], LOSS_RTOL, atol=0.0, k=k)
    if record:
        record_margin(f'split_bf16_{record}', case, 'loss', err, LOSS_RTOL, arb)
    failed = [] if ok else [('loss', err)]
    worst = {'loss': (err, arb, 'loss')}
    ratio = {}
    n_parts = {'gradient': 0, 'group': 0, 'block': 0}
    got = export_grads(solver)
    for i, (g, w32, w64) in enumerate(zip(got, ref['g32'], ref['g64'])):
        if w64 is None:
            assert float(np.abs(g).max()) == 0.0, (case, i)
            continue
        for (label, kind, gp), (_, _, p32), (_, _, p64) in zip(_parts(i, len(got), g), _parts(i, len(got), w32), _parts(i, len(got), w64)):
            ok, err, arb = close_or_arbitrated(gp, p32, lambda p64=p64: p64, GRAD_RTOL, k=k)
            if record:
                record_margin(f'split_bf16_{record}', f'{case}[{label}]', kind, err, GRAD_RTOL, arb)
            n_parts[kind] += 1
            if kind not in worst or err > worst[kind][0]:
                worst[kind] = (err, arb, label)
            r = _ratio(gp, p32, p64)
            if kind not in ratio or r > ratio[kind][0]:
                ratio[kind] = (r, label)
            if not ok:
                failed.append((label, err, r))
    summary = dict(worst=worst, ratio=ratio, n_parts=n_parts, n_failed=len(failed))
    text = ', '.join(f'{kind} {e:.2e}{"*" if a else ""} at {lab}' for kind, (e, a, lab) in worst.items())
    rtext = ', '.join(f'{kind} {r:.2f} at {lab}' for kind, (r, lab) in ratio.items())
    print(f'SPLIT {case}: k {k:g}, parts {n_parts}, failed {len(failed)}; worst error ({"*"}: arbitrated) {text}; worst ratio to the fp32 oracle {rtext}')
    return failed, summary


def _check_step(case, solver, ref, k=K_RULE, group=None):
    assert _at_the_floor(ref) == [], case
    failed, summary = _rule(case, solver, ref, k=k, record=group or ref['case']['group'])
    assert not failed, (case, failed[:8], len(failed))
    return summary


def _tile_name(case):
    return 'pinn_tile_kernel<' + KERNELS[case['kernel']]['head'].format(act=0 if case['static'] else -1) + '>'


def _solver(pa, ref, solver_kwargs):
    case = ref['case']
    eq, kw = case['problem'](pa.D)
    solver = pa.Solver(eq, **kw, **solver_kwargs)
    assert solver.model.net.layout.hp == KERNELS[case['kernel']]['hp']
    load_params(solver, ref['start'])
    solver.set_gemm_mode('bf16x3')
    return solver


def _assert_kernels(lib, solver, case):
    """ which kernel ran: a split one, the one the case meant (static Tanh: ACTC = PINN_ACT_TANH = 0 in the name, Sigmoid / mixed: -1), and for
    widths >= 128 the split form of the streamed weight-gradient kernel """
    assert ran_split_kernel(solver), lib.pinn_last_kernel_name()
    name = lib.pinn_last_kernel_name().decode()
    assert name == _tile_name(case), (name, _tile_name(case))
    assert name.rstrip('>').split(',')[5] == ('0' if case['static'] else '-1')            # <HP,ND,N2,MT,LHC,ACTC,COMB,VAR>
    if KERNELS[case['kernel']]['hp'] >= 128 and case['lh'] > 0:
        wg = lib.pinn_last_wgrad_kernel_name().decode()
        assert wg.rstrip('>').split(',')[5] == 'true', wg                                   # <HP,ND,N2,COMB,MT,SPLIT,SKIPS,HEAVY>
        assert wg.startswith(f'pinn_wgrad_kernel<{KERNELS[case["kernel"]]["hp"]},'), wg


def _step(pa, lib, name, solver_kwargs, case=None, ref=None):
    """ one fused step of a case in split mode; returns (solver, reference) with the kernels asserted and nothing else checked """
    case = case or CASES[name]
    ref = ref or _reference(name, case)
    solver = _solver(pa, ref, solver_kwargs)
    assert solver.program is not None, solver.program_error
    xs = torch.from_numpy(ref['pts'].copy()).to(solver.device)
    solver._fused_step(xs, 1)
    if solver.device.type != 'cpu':
        torch.cuda.synchronize()
    _assert_kernels(lib, solver, case)
    return solver, ref


def _fused_case(pa, lib, name, solver_kwargs, k=K_RULE):
    solver, ref = _step(pa, lib, name, solver_kwargs)
    if CASES[name]['cancel']:
        canc = _cancellation(ref)
        print(f'SPLIT {name}: cancellation |sum| / sum|.| per hidden matrix {["%.1e" % c for c in canc]}')
        assert all(3e-4 <= c <= 3e-2 for c in canc), canc
    _check_step(name, solver, ref, k=k)
    return solver


EMU = dict(device='cpu')


# ---- CPU tier: no vacuous comparison; the cancellation of case G is what it says ---------------------------------------------------------------------
@pytest.mark.parametrize('group', ['A', 'B', 'C', 'D', 'E', 'G', 'emu'])
def test_no_reference_part_sits_at_the_floor(group):
    """ with the fp64 oracle alone: no case leaves a gradient tensor, a 16-unit group or a 16 x 32 block whose fp64 norm is at the absolute
    floor 1e-9 sqrt(size) of the rule (it would pass whatever the kernel wrote). Case F's batch size comes from the device's grid: its cases
    assert the same on the device. The blocks and groups are counted at one padded width: the cut is at the REAL width. """
    names = _names('A-emu', 'B-emu', 'C-emu', 'D-emu', 'G-emu', 'G-emu-wide') if group == 'emu' else _names(group)
    assert names
    for name in names:
        ref = _case_reference(name, fp32=False)
        assert _at_the_floor(ref) == [], name
        assert all(np.isfinite(g).all() for g in ref['g64'] if g is not None)
        if CASES[name]['cancel']:
            canc = _cancellation(ref)
            assert len(canc) == CASES[name]['lh'] and all(3e-4 <= c <= 3e-2 for c in canc), (name, canc)
    if group == 'A':
        g = _case_reference('A/100x3', fp32=False)['g64']           # W2 [100, 100]: 7 groups (the last one 4 rows), 7 x 4 blocks (the last column 4 wide)
        parts = _parts(2, len(g), g[2])
        assert [p[0] for p in parts if p[1] == 'group'] == [f'2/u{j}' for j in range(7)] and parts[7][2].shape == (4, 100)
        blocks = [p for p in parts if p[1] == 'block']
        assert len(blocks) == 28 and blocks[-1][2].shape == (4, 4) and blocks[0][2].shape == (16, 32)
        assert not [p for p in _parts(0, len(g), g[0]) if p[1] == 'block'] and not [p for p in _parts(6, len(g), g[6]) if p[1] == 'block']


def test_cancelling_weights_live_in_the_lower_planes():
    """ case G's construction: the `hi` plane of every hidden weight is +-c exactly, the 2^-9 perturbation is in `mid`, the 2^-17 one in `lo` """
    ref = _case_reference('G/s64_1/emu', fp32=False)
    for l in range(1, 4):
        w = ref['start'][2 * l]
        hi = _bf16_exact(w)
        assert len(np.unique(np.abs(hi))) == 1
        mid = _bf16_exact(w - hi)
        lo = w - hi - mid
        assert 2.0 ** -12 < np.abs(mid / hi).mean() < 2.0 ** -9 and 2.0 ** -20 < np.abs(lo / hi).mean() < 2.0 ** -17
        assert abs(int(np.sign(hi).sum(axis=0).max())) == 0 and abs(int(np.sign(hi).sum(axis=1).max())) == 0       # balanced signs along both axes


# ---- D (emulator twins), H, the negative dispatch: CPU tier -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', _names('D-emu', 'G-emu'))
def test_width_64_split_kernels_on_the_emulator(pa, emu_lib, name):
    """ emulator twins of D and G on the two width-64 kernels: one or two tiles per team """
    _fused_case(pa, emu_lib, name, dict(_lib=emu_lib, **EMU), k=K_G if CASES[name]['cancel'] else K_RULE)


@pytest.mark.parametrize('name', _names('A-emu'))
def test_one_padded_tile_of_the_width_128_split_kernel_on_the_emulator(pa, emu_lib, name):
    """ the default tier's wide case: 100 x 100 (padded to 128) on one tile, heat shape with the source term, split tile and weight-gradient kernel """
    _fused_case(pa, emu_lib, name, dict(_lib=emu_lib, **EMU))


@slow_emu
@pytest.mark.parametrize('name', _names('B-emu', 'C-emu', 'G-emu-wide') + ['E/s128/n17', 'E/s256/n1', 'A/65x1'])
def test_wide_split_kernels_on_the_emulator(pa, emu_lib, name):
    """ emulator twins at widths 128 / 256: a padded width-256 tile, the run-time activation form with Sigmoid in the padded units, case G,
    a ragged second tile, one point, depth 1 (no fragment copy of hidden weights: lh == 0) """
    ref = _reference(name, CASES[name], n=16) if name == 'A/65x1' else None
    if ref is None:
        _fused_case(pa, emu_lib, name, dict(_lib=emu_lib, **EMU), k=K_G if CASES[name]['cancel'] else K_RULE)
    else:
        solver, ref = _step(pa, emu_lib, name, dict(_lib=emu_lib, **EMU), ref=ref)
        _check_step(name + '/n16', solver, ref, group='A-emu')


def _negative(pa, lib, name, solver_kwargs):
    case = NEGATIVE[name]
    torch.manual_seed(case['seed'])
    eq, kw = case['problem'](pa.D)
    solver = pa.Solver(eq, **kw, **solver_kwargs)
    xs = torch.from_numpy(_points(37, case['which'])).to(solver.device)
    solver._fused_step(xs, 1)
    assert not ran_split_kernel(solver)
    want, fp32_name = solver.grads.clone(), lib.pinn_last_kernel_name()
    solver.set_gemm_mode('bf16x3')
    assert solver.model.net.gemm_mode == 'bf16x3'
    solver._fused_step(xs, 1)
    assert not ran_split_kernel(solver), lib.pinn_last_kernel_name()
    assert lib.pinn_last_kernel_name() == fp32_name
    assert torch.equal(solver.grads, want)
    assert float(solver.grads[solver.model.net.layout.off_loss]) > 0.0


@pytest.mark.parametrize('name', list(NEGATIVE))
def test_shapes_next_to_the_split_ones_keep_the_fp32_kernels_on_the_emulator(pa, emu_lib, name):
    """ the mode is a request: depth 3, depth 5 and Sigmoid at width 64 have no split kernel -- the fp32 mode's gradient buffer, bit for bit """
    _negative(pa, emu_lib, name, dict(_lib=emu_lib, **EMU))


def test_the_environment_selects_the_split_kernels(pa, emu_lib, monkeypatch):
    """ H: PYDENS_AMD_GEMM=bf16x3 for a whole process: a new Solver reports the mode and takes the split kernel """
    case = CASES['D/poisson/48x4/emu']
    ref = _reference('D/poisson/48x4/emu', case)
    eq, kw = case['problem'](pa.D)
    plain = pa.Solver(eq, **kw, _lib=emu_lib, **EMU)
    assert plain.model.net.gemm_mode == 'fp32'
    monkeypatch.setenv('PYDENS_AMD_GEMM', 'bf16x3')
    solver = pa.Solver(eq, **kw, _lib=emu_lib, **EMU)
    assert solver.model.net.gemm_mode == 'bf16x3'
    load_params(solver, ref['start'])
    solver._fused_step(torch.from_numpy(ref['pts'].copy()), 1)
    _assert_kernels(emu_lib, solver, case)
    _check_step('H/env', solver, ref, group='H')
    load_params(plain, ref['start'])
    plain._fused_step(torch.from_numpy(ref['pts'].copy()), 1)
    assert not ran_split_kernel(plain)


# ---- the rule fails on a subtly wrong kernel (emulator) ------------------------------------------------------------------------------------------------
MUTANTS = {'spn5': '-DPINN_SP_NPROD=5', 'spn3': '-DPINN_SP_NPROD=3'}


def _mutant_run(pa, lib, names, k_of):
    """ {case: (failed parts, summary)} of the rule on `names` with the library `lib` """
    out = {}
    for name in names:
        solver, ref = _step(pa, lib, name, dict(_lib=lib, **EMU))
        assert _at_the_floor(ref) == [], name
        out[name] = _rule(f'{name}', solver, ref, k=k_of(name))
    return out


def _k_of(name):
    return K_G if CASES[name]['cancel'] else K_RULE


@pytest.mark.parametrize('tag', list(MUTANTS))
def test_the_rule_fails_on_a_wrong_width_64_split_kernel(pa, emu_lib, tag):
    """ PINN_SP_NPROD=5 drops the (weight lo) x (activation hi) product of every GEMM step -- 2^-17 of the products of every fragment --, =3 every
    product with i + j = 2. The rule, on cases D and G of both width-64 kernels: passes on the default build (asserted by the twins above and
    here on G), fails on each wrong build on BOTH kernels' case G by at least 4 x its bound, and on case D of both kernels. """
    lib = _mutant(MUTANTS[tag], tag, (64,))
    g_names, d_names = _names('G-emu'), _names('D-emu')
    res = _mutant_run(pa, lib, g_names + d_names, _k_of)
    print(f'MUTANT {tag}: ' + '; '.join(f'{n}: {len(f)} parts failed' for n, (f, s) in res.items()))
    for name in g_names:
        failed, summary = res[name]
        assert failed, (tag, name, summary)
        # the wrong build misses case G's bound by at least 4 x: its worst ratio to the fp32 oracle's own error, in a FAILED part, against k
        assert max([f[2] for f in failed if len(f) == 3], default=0.0) >= 4.0 * K_G, (tag, name, summary['ratio'])
        ok_failed, _ = _rule(name + '/default', *_step(pa, emu_lib, name, dict(_lib=emu_lib, **EMU)), k=K_G)
        assert not ok_failed, (name, ok_failed[:4])
    # case D, ordinary weights (measured, profiles/r12_split_bf16.txt): every ODE case fails on both builds (24 .. 61 parts each), of the
    # Poisson-box cases only the padded 33 x 4 does (4 / 5 parts) -- elsewhere both builds stay inside the 1e-5 bar of the first test
    assert all(res[name][0] for name in d_names if CASES[name]['kernel'] == 's64_2'), tag
    assert any(res[name][0] for name in d_names if CASES[name]['kernel'] == 's64_1'), tag


@slow_emu
@pytest.mark.parametrize('tag', list(MUTANTS))
def test_the_rule_fails_on_a_wrong_width_128_split_kernel(pa, emu_lib, tag):
    """ the same two wrong builds of the width-128 split units (tile kernel and streamed weight-gradient kernel): one case A, one case G """
    lib = _mutant(MUTANTS[tag], tag + '_128', (128,))
    res = _mutant_run(pa, lib, ['A/100x2/n16', 'G/s128/emu'], _k_of)
    print(f'MUTANT {tag} (width 128): ' + '; '.join(f'{n}: {len(f)} parts failed' for n, (f, s) in res.items()))
    assert res['G/s128/emu'][0], (tag, res['G/s128/emu'][1])


def test_an_exact_split_by_truncation_is_recorded_not_required_to_fail(pa):
    """ PINN_SP_ROUND=0 is an exact split as well (2.18x instead of 1.18x of the fp32 reference's error on trained models):
    not a bug, so nothing is required of the rule here -- its margins are printed for profiles/r12_split_bf16.txt """
    lib = _mutant('-DPINN_SP_ROUND=0', 'spround0', (64,))
    res = _mutant_run(pa, lib, _names('G-emu') + ['D/poisson/48x4/emu', 'D/ode/48x4/emu'], _k_of)
    print('MUTANT spround0: ' + '; '.join(f'{n}: {len(f)} parts failed' for n, (f, s) in res.items()))
    for name, (failed, summary) in res.items():
        assert np.isfinite(summary['worst']['gradient'][0])


@pytest.mark.parametrize('tag', list(MUTANTS))
def test_what_the_older_split_tests_make_of_the_wrong_builds(pa, emu_lib, tag):
    """ the evidence for the gap: test_split_gemm's ragged comparison (2e-6 rel-L2 of the whole buffer against our fp32 kernel, cfg2 / cfg4) and
    its golden comparison (1e-5 per tensor) on the two wrong builds. Recorded, nothing required: measured, neither comparison notices the
    dropped lo x hi product (7.5e-7 / 5.4e-8 against 2e-6, 6.7e-6 / 5.0e-6 against 1e-5); the golden comparison alone notices the build without
    i + j = 2 products, by 1.15 x and 1.6 x its bar. """
    import pinn_configs as pc
    from conftest import Golden
    from helpers import make_solver
    lib = _mutant(MUTANTS[tag], tag, (64,))
    seen = {}
    for cfg_name in ('cfg2', 'cfg4'):
        torch.manual_seed(3)
        cfg, solver = make_solver(cfg_name, pa, _lib=lib, **EMU)
        pts = torch.from_numpy(pc.sample_points(cfg, 33, seed=21))
        out = {}
        for gemm in ('fp32', 'bf16x3'):
            solver.set_gemm_mode(gemm)
            solver._fused_step(pts, 1)
            out[gemm] = solver.grads.clone().numpy()
        lay = solver.model.net.layout
        err = rel_l2(out['bf16x3'][:lay.p_core], out['fp32'][:lay.p_core])
        seen[f'ragged/{cfg_name}/n33'] = (err, 2e-6)
        g = Golden(cfg_name)
        _, solver = make_solver(cfg_name, pa, gemm='bf16x3', _lib=lib, **EMU)
        load_params(solver, g.params)
        solver._fused_step(torch.from_numpy(g.points[0].copy()), 1)
        assert ran_split_kernel(solver)
        err = max(rel_l2(got, want) for got, want in zip(export_grads(solver), g.grads) if want is not None)
        seen[f'golden/{cfg_name}'] = (err, 1e-5)
    print(f'OLD SUITE on {tag}: ' + '; '.join(f'{k}: {e:.2e} against {b:.0e} -> {"noticed" if e >= b else "NOT noticed"}' for k, (e, b) in seen.items()))
    assert all(np.isfinite(e) for e, _ in seen.values())


# ---- A, B, C, D, E, G on the device -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('name', _names('A'))
def test_widths_and_depths_of_the_width_128_split_kernel_on_the_gpu(pa, dev, name):
    """ A: 65 .. 128 units (padded to 128), one to three and eight hidden layers, mixed widths, heat shape in (x, y, t) with and without a
    source term; 53 points. At depth 1 there is no hidden->hidden matrix: no fragment copy, no weight-gradient launch -- and no bias of a
    first hidden->hidden layer to prefetch: the split kernels fetched it regardless, HP * HP floats past the end of the parameter buffer
    (an illegal memory access wherever that address was not mapped). """
    _fused_case(pa, dev, name, {})


@gpu
@pytest.mark.parametrize('name', _names('B'))
def test_widths_and_depths_of_the_width_256_split_kernel_on_the_gpu(pa, dev, name):
    """ B: 129 .. 256 units (padded to 256), one to three hidden layers, 256 x 130 x 256; the wave shape and the 1-D heat equation with a source """
    _fused_case(pa, dev, name, {})


@gpu
@pytest.mark.parametrize('name', _names('C'))
def test_activations_of_the_wide_split_kernels_on_the_gpu(pa, dev, name):
    """ C: Tanh (the static form), Sigmoid, Tanh / Sigmoid / Tanh and the reverse (the run-time form: ACTC -1) at a padded and a full width of
    both wide kernels. Sigmoid's padded units hold 0.5 where Tanh's hold 0. """
    _fused_case(pa, dev, name, {})


@gpu
@pytest.mark.parametrize('name', _names('D'))
def test_widths_of_the_width_64_split_kernels_on_the_gpu(pa, dev, name):
    """ D: 33 .. 64 units and 64 x 40 x 64 x 33 on the Poisson-box and the ODE kernel (two teams each) """
    _fused_case(pa, dev, name, {})


@gpu
@pytest.mark.parametrize('name', list(NEGATIVE))
def test_shapes_next_to_the_split_ones_keep_the_fp32_kernels_on_the_gpu(pa, dev, name):
    _negative(pa, dev, name, {})


@gpu
@pytest.mark.parametrize('name', _names('E'))
def test_ragged_tiles_of_every_split_kernel_on_the_gpu(pa, dev, name):
    """ E: 1, 15, 16, 17, 31 and 33 points: the gradients, not just the loss -- a lone team, empty lanes in the split planes, the second team's
    empty round """
    _fused_case(pa, dev, name, {})


@gpu
@pytest.mark.parametrize('name', _names('G'))
def test_lower_planes_carry_the_answer_on_the_gpu(pa, dev, name):
    """ G: every hidden pre-activation sum cancels in its hi x hi products to 1e-2 .. 1e-3 of sum |a b| """
    _fused_case(pa, dev, name, {}, k=K_G)


# ---- F: the tile loop, the chunked slabs ----------------------------------------------------------------------------------------------------------------
F_NETS = {
    's64_1': ('poisson', [64] * 4),
    's64_2': ('ode', [48] * 4),
    's128': ('heat3', [100] * 3),
    's256': ('wave', [200] * 3),
}


def _launch_info(lib):
    info = (ctypes.c_int32 * 4)()
    assert lib.pinn_last_launch_info(info) == 0
    return dict(grid=info[0], per_cu=info[1], threads=info[2], smem=info[3])


@gpu
@pytest.mark.parametrize('kernel', list(F_NETS))
def test_every_workgroup_and_team_runs_a_second_tile_on_the_gpu(pa, dev, kernel):
    """ F: n = 16 MT (2 grid teams) + 3 points, grid and threads read from the launch info of a probe launch that fills the device: every
    workgroup -- and both teams of the two-team kernels -- runs two tiles and one of them a ragged third. Widths 128 / 256 then run the same
    batch with a slab budget of one byte (one sweep of the grid per chunk): within 2e-6 of the one-pass gradients, and the rule again. """
    which, feats = F_NETS[kernel]
    case = _case('F', which, feats, seed=1500 + sum(feats))
    head = KERNELS[kernel]['head'].split(',')
    mt, teams = int(head[3]), 2 if int(head[7]) & 256 else 1
    eq, kw = case['problem'](pa.D)
    probe = pa.Solver(eq, **kw)
    probe.set_gemm_mode('bf16x3')
    n_probe = 16 * mt * teams * 8 * torch.cuda.get_device_properties(0).multi_processor_count        # more tiles than any grid (at most 4 workgroups per CU)
    probe._fused_step(torch.from_numpy(_points(n_probe, which)).cuda(), 1)
    torch.cuda.synchronize()
    info = _launch_info(dev)
    assert ran_split_kernel(probe) and info['threads'] == 512, info
    grid = info['grid']
    n = 16 * mt * 2 * grid * teams + 3
    name = f'F/{kernel}/n{n}'
    ref = _reference(name, case, n=n, chunk=2048)
    solver, ref = _step(pa, dev, name, {}, case=case, ref=ref)
    info = _launch_info(dev)
    tiles = (n + 16 * mt - 1) // (16 * mt)
    print(f'SPLIT {name}: tiles {tiles} of {16 * mt} points, teams {teams}, launch info {info}')
    assert info['grid'] == grid and tiles == 2 * grid * teams + 1
    _check_step(name, solver, ref)
    if KERNELS[kernel]['hp'] < 128:
        return
    one_pass = solver.grads.clone()
    lay = solver.model.net.layout
    try:
        dev.pinn_debug_wgx_chunk_bytes(solver.model.net.handle, 1)
        solver.model._workspaces.clear()
        solver._fused_step(torch.from_numpy(ref['pts'].copy()).cuda(), 1)
        torch.cuda.synchronize()
    finally:
        dev.pinn_debug_wgx_chunk_bytes(solver.model.net.handle, 0)
        solver.model._workspaces.clear()
    _assert_kernels(dev, solver, case)
    # (no counter exposes the number of chunks: a budget below one tile's slabs gives one sweep of max(grid, grid2) tiles per chunk, and the
    #  split weight-gradient kernel runs one workgroup per CU)
    sweep = max(grid, torch.cuda.get_device_properties(0).multi_processor_count)
    assert -(-tiles // sweep) > 1, (tiles, sweep)
    err = rel_l2(solver.grads[:lay.p_core].cpu().numpy(), one_pass[:lay.p_core].cpu().numpy())
    record_margin('split_bf16_F_chunked', name, 'gradient', err, 2e-6)
    print(f'SPLIT {name}: chunked against one pass {err:.2e}')
    assert err < 2e-6
    _check_step(name + '/chunked', solver, ref)
