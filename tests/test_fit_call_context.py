""" The context of a fit chunk belongs to the call that carries it (pinn_abi.cpp: StepCall / FitCall / StepTail handed down by reference, no
state of the calling thread): a chunk that fails leaves nothing behind for the next, unrelated step call; two nets driven alternately on one
thread follow the trajectories they follow alone; `engine.Net.fit_steps` reaches pinn_fit_steps with the header's arguments, and that one
entry point runs the same chunk with or without a control block and a rate table. CPU only, on the
emulator build of the product's own pinn_abi.cpp; every comparison is of bits. """
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))

DIMS, BATCH, ND, N2 = (2, 16, 16, 1), 64, 2, 2
COLUMNS = [(0, 0.0, 1.0), (0, 0.0, 1.0)]          # SAMPLE_UNIFORM on both columns
SEED, LR = 77, 0.01


@pytest.fixture(scope='module')
def lib():
    import build_emu
    from pydens_amd import engine
    lib = engine.bind(ctypes.CDLL(build_emu.build()))
    assert lib.pinn_backend() == b'emu-host'
    return lib


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _residual():
    """ r = u_xx + u_yy + u as a residual program: streams u, u_x, u_y, u_xx, u_yy, then the two inputs, then temporaries """
    from pydens_amd import engine
    first = 1 + ND + N2 + 2
    return engine.Residual.build(engine.RES_PROGRAM, 0, None, program=([(engine.OPS['ADD'], first, 3, 4), (engine.OPS['ADD'], first, first, 0)], []))


class Run:
    """ one net of DIMS with buffers of its own; the same seed gives the same parameters """
    def __init__(self, lib, persist):
        from pydens_amd import engine
        self.lib = lib
        self.net = engine.Net(list(DIMS), 'tanh', 2, lib=lib)
        lib.pinn_debug_fit_persistent(self.net.handle, persist)
        lay = self.net.layout
        self.params = torch.zeros(lay.p_total)
        self.params[:lay.off_log_scale] = 0.4 * torch.randn(lay.off_log_scale, generator=torch.Generator().manual_seed(5))
        self.mask = torch.zeros(lay.p_total, dtype=torch.uint8)
        self.mask[:lay.off_log_scale] = 1
        self.grads, self.m, self.v = (torch.zeros(lay.p_total) for _ in range(3))
        self.step = torch.zeros(1, dtype=torch.int32)
        self.xs = torch.zeros(BATCH, 2)
        self.ws_bytes = self.net.workspace_bytes(BATCH, ND, N2)
        self.ws = torch.zeros(self.ws_bytes // 4 + 8)
        self.ctrl = torch.zeros(int(lib.pinn_fit_ctrl_bytes()) + 64, dtype=torch.uint8)
        self.losses = torch.zeros(16)
        self.residual = _residual()
        self.optim = engine.Optim.build(engine.OPT_ADAM, LR, betas=(0.9, 0.999), eps=1e-8)
        self.at = 0

    def chunk(self, k):
        """ k iterations as ONE call with a control block (width 16, a batch of four tiles: the one-CU chunk kernel) """
        self.net.fit_steps(self.residual, self.params, self.xs, COLUMNS, SEED, self.at, self.grads, self.ws, self.m, self.v, self.mask, self.step,
                           self.at + 1, self.optim, self.losses[self.at:self.at + k], k, dir_cols=(0, 1), n2=N2, ctrl=self.ctrl)
        self.at += k

    def steps(self, k):
        """ k iterations, each a sampler call and a pinn_residual_optim_step """
        for _ in range(k):
            self.net.sample_points(self.xs, COLUMNS, SEED, self.at)
            self.net.residual_optim_step(self.residual, self.params, self.xs, self.grads, self.ws, self.m, self.v, self.mask, self.step,
                                         self.at + 1, self.optim, dir_cols=(0, 1), n2=N2, loss_out=self.losses.data_ptr() + 4 * self.at)
            self.at += 1

    def state(self):
        return {name: getattr(self, name).clone() for name in ('params', 'm', 'v', 'grads', 'xs', 'losses', 'step')}


def _same(got, want, what):
    for name in want:
        assert torch.equal(got[name], want[name]), (what, name)


def test_a_failed_chunk_leaves_nothing_behind(lib):
    dirs = (ctypes.c_int * 2)(0, 1)
    kind, lo, hi = (ctypes.c_int * 2)(0, 0), (ctypes.c_float * 2)(0.0, 0.0), (ctypes.c_float * 2)(1.0, 1.0)
    rates = (ctypes.c_float * 3)(LR, LR / 2, LR / 4)
    batch = torch.rand(BATCH, 2, generator=torch.Generator().manual_seed(9))

    def adam_step(run):
        run.xs.copy_(batch)
        rc = lib.pinn_residual_optim_step(run.net.handle, ctypes.byref(run.residual), _ptr(run.params), _ptr(run.xs), BATCH, dirs, ND, N2, None, 0.0,
                                          _ptr(run.grads), _ptr(run.m), _ptr(run.v), _ptr(run.mask), _ptr(run.step), 1, ctypes.byref(run.optim),
                                          _ptr(run.losses), _ptr(run.ws), run.ws_bytes, None)
        assert rc == 0, lib.pinn_last_error().decode()
        return run.state()

    want = adam_step(Run(lib, 2))
    assert torch.equal(want['xs'], batch) and float(want['losses'][0]) > 0.0 and int(want['step']) == 1

    run = Run(lib, 2)
    before = run.state()

    def chunk(workspace_bytes):
        """ three iterations with a control block and a schedule: the one-launch request travels with this call """
        return lib.pinn_fit_steps(run.net.handle, ctypes.byref(run.residual), _ptr(run.params), _ptr(run.xs), BATCH, kind, lo, hi, SEED, 0,
                                  dirs, ND, N2, 0.0, _ptr(run.grads), _ptr(run.m), _ptr(run.v), _ptr(run.mask), _ptr(run.step), 1,
                                  ctypes.byref(run.optim), _ptr(run.losses), 3, _ptr(run.ws), workspace_bytes, _ptr(run.ctrl),
                                  run.ctrl.numel(), None, rates)
    # pinn_workspace_bytes is an upper bound over every form a step may take (one byte less than IT still runs the chunk), so the
    # byte that matters is read from the library: a chunk one byte short of what its step needs, and one with no room at all
    assert chunk(1) != 0
    need = int(re.search(r'workspace too small: need (\d+) bytes', lib.pinn_last_error().decode()).group(1))
    assert 0 < need <= run.ws_bytes
    assert chunk(need - 1) != 0 and 'workspace too small' in lib.pinn_last_error().decode()
    _same(run.state(), before, 'the failed chunk itself')
    _same(adam_step(run), want, 'the step behind the failed chunk')      # (xs among them: no stray draw of a next batch)


def test_two_nets_interleaved_follow_their_solo_trajectories(lib):
    def drive(a, b):
        for _ in range(3):
            if a is not None:
                a.chunk(4)
            if b is not None:
                b.steps(4)
        return (a.state() if a is not None else None), (b.state() if b is not None else None)

    st0 = (ctypes.c_int32 * 4)()
    lib.pinn_debug_fit_graph_stats(st0)
    solo_a, _ = drive(Run(lib, 2), None)
    st = (ctypes.c_int32 * 4)()
    lib.pinn_debug_fit_graph_stats(st)
    assert st[0] - st0[0] == 3 and lib.pinn_last_kernel_name().decode().startswith('pinn_fit_kernel<')      # (net A's chunks ARE the one-CU form)
    _, solo_b = drive(None, Run(lib, 0))
    both_a, both_b = drive(Run(lib, 2), Run(lib, 0))
    assert int(solo_a['step']) == 12 and int(solo_b['step']) == 12 and float(solo_b['losses'][11]) > 0.0
    _same(both_a, solo_a, 'net A (one-CU chunks)')
    _same(both_b, solo_b, 'net B (per-iteration steps)')


class RecordingLib:
    """ stands in for the loaded library: every attribute is a callable that notes its name and argument count and returns 0 """
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, len(args), args))
            return 0
        return call


@pytest.mark.parametrize('with_optim', [False, True])
@pytest.mark.parametrize('with_ctrl', [False, True])
@pytest.mark.parametrize('with_rates', [False, True])
def test_fit_steps_reaches_the_symbol_its_arguments_name(with_optim, with_ctrl, with_rates):
    """ one chunk entry point whatever the arguments: pinn_fit_steps with the 29 arguments of include/pinn.h """
    from pydens_amd import engine
    rec = RecordingLib()
    net = engine.Net.__new__(engine.Net)
    net.lib, net.handle = rec, None
    n = 32
    f32 = lambda *shape: torch.zeros(*shape)
    optim = engine.Optim.build(engine.OPT_SGD, 0.5, momentum=0.9) if with_optim else engine.Optim.build(engine.OPT_ADAM, LR, betas=(0.9, 0.999), eps=1e-8)
    ctrl = torch.zeros(64, dtype=torch.uint8) if with_ctrl else None
    net.fit_steps(engine.Residual(), f32(n), f32(8, 2), COLUMNS, SEED, 0, f32(n), f32(16), f32(n), f32(n), torch.ones(n, dtype=torch.uint8),
                  torch.zeros(1, dtype=torch.int32), 1, optim, f32(3), 3, dir_cols=(0, 1), n2=N2, ctrl=ctrl,
                  lr_steps=[LR, LR / 2, LR / 4] if with_rates else None)
    (name, argc, args), = [c for c in rec.calls if c[0] != 'pinn_destroy']
    assert (name, argc) == ('pinn_fit_steps', 29)
    rule = args[20]._obj                # (what ctypes.byref wraps: the caller's struct itself, field for field)
    assert rule is optim
    if with_optim:
        assert (rule.rule, rule.lr, rule.momentum) == (engine.OPT_SGD, 0.5, ctypes.c_float(0.9).value)
    else:
        assert (rule.rule, rule.lr, rule.beta1, rule.beta2, rule.eps) == \
            (engine.OPT_ADAM, ) + tuple(ctypes.c_float(v).value for v in (LR, 0.9, 0.999, 1e-8))
    assert (args[25] is None, args[26]) == (not with_ctrl, 64 if with_ctrl else 0)         # ctrl is (None, 0) when absent
    if with_rates:                      # the rates array sits in the last position
        assert [args[28][i] for i in range(3)] == [ctypes.c_float(v).value for v in (LR, LR / 2, LR / 4)]
    else:
        assert args[28] is None


def _one_chunk(lib, optim, form):
    """ four iterations on a fresh Run (launch graphs / eager loop: pinn_debug_fit_persistent 0): 'steps' -- four sample_points +
    residual_optim_step calls; otherwise ONE pinn_fit_steps call, with a control block and / or a constant rate table as `form` names """
    run = Run(lib, 0)
    run.optim = optim
    if form == 'steps':
        run.steps(4)
    else:
        run.net.fit_steps(run.residual, run.params, run.xs, COLUMNS, SEED, 0, run.grads, run.ws, run.m, run.v, run.mask, run.step, 1, optim,
                          run.losses[:4], 4, dir_cols=(0, 1), n2=N2, ctrl=run.ctrl if 'ctrl' in form else None,
                          lr_steps=[optim.lr] * 4 if 'rates' in form else None)
    return run.state()


@pytest.mark.parametrize('rule', ['adam', 'sgd'])
def test_one_entry_point_runs_the_same_chunk_in_every_form(lib, rule):
    """ what the dispatch table used to imply: without `ctrl`, with `ctrl`, with a constant `lr_steps` and with both, the chunk is the same
    four iterations -- parameters, both state arrays, gradients, losses, step counter and the batch left in xs, bit for bit -- and those
    are four sample_points + residual_optim_step calls """
    from pydens_amd import engine
    build = {'adam': lambda: engine.Optim.build(engine.OPT_ADAM, LR, betas=(0.9, 0.999), eps=1e-8),
             'sgd': lambda: engine.Optim.build(engine.OPT_SGD, LR, momentum=0.9)}[rule]
    want = _one_chunk(lib, build(), 'steps')
    assert int(want['step']) == 4 and float(want['losses'][3]) > 0.0 and bool((want['m'] != 0).any())
    for form in ('plain', 'ctrl', 'rates', 'ctrl+rates'):
        _same(_one_chunk(lib, build(), form), want, form)


@pytest.mark.parametrize('bad', [dict(betas=(0.9, 1.0)), dict(eps=-1.0)], ids=['beta2_is_1', 'negative_eps'])
def test_adam_numbers_the_library_refuses(lib, bad):
    """ plain Adam's numbers pass through the checks of the family: beta2 = 1 and eps < 0 are refused by every entry point that updates,
    with a message, and nothing is launched -- every buffer, the batch in xs among them, stays as it was """
    from pydens_amd import engine
    optim = engine.Optim.build(engine.OPT_ADAM, LR, **dict(dict(betas=(0.9, 0.999), eps=1e-8), **bad))
    run = Run(lib, 2)
    run.xs.copy_(torch.rand(BATCH, 2, generator=torch.Generator().manual_seed(9)))
    run.grads.normal_(generator=torch.Generator().manual_seed(10))
    before = run.state()
    dirs = (ctypes.c_int * 2)(0, 1)
    kind, lo, hi = (ctypes.c_int * 2)(0, 0), (ctypes.c_float * 2)(0.0, 0.0), (ctypes.c_float * 2)(1.0, 1.0)
    n = run.params.numel()
    calls = {
        'pinn_optim_step_at': lambda: lib.pinn_optim_step_at(_ptr(run.params), _ptr(run.grads), _ptr(run.m), _ptr(run.v), _ptr(run.mask), n,
                                                             _ptr(run.step), 1, ctypes.byref(optim), _ptr(run.losses), run.net.layout.off_loss, None),
        'pinn_residual_optim_step': lambda: lib.pinn_residual_optim_step(
            run.net.handle, ctypes.byref(run.residual), _ptr(run.params), _ptr(run.xs), BATCH, dirs, ND, N2, None, 0.0, _ptr(run.grads), _ptr(run.m),
            _ptr(run.v), _ptr(run.mask), _ptr(run.step), 1, ctypes.byref(optim), _ptr(run.losses), _ptr(run.ws), run.ws_bytes, None),
        'pinn_fit_steps': lambda: lib.pinn_fit_steps(
            run.net.handle, ctypes.byref(run.residual), _ptr(run.params), _ptr(run.xs), BATCH, kind, lo, hi, SEED, 0, dirs, ND, N2, 0.0, _ptr(run.grads),
            _ptr(run.m), _ptr(run.v), _ptr(run.mask), _ptr(run.step), 1, ctypes.byref(optim), _ptr(run.losses), 2, _ptr(run.ws), run.ws_bytes,
            _ptr(run.ctrl), run.ctrl.numel(), None, None)}
    for name, call in calls.items():
        assert call() != 0, name
        assert ('beta' if 'betas' in bad else 'epsilon') in lib.pinn_last_error().decode(), name
        _same(run.state(), before, name)
    optim.beta2, optim.eps = 0.999, 1e-8            # (the same calls with torch's numbers go through: the refusals were about the numbers)
    for name, call in calls.items():
        assert call() == 0, (name, lib.pinn_last_error().decode())
