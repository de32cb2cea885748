""" Loss-term weights: the device kernels behind include/pinn.h pinn_balance_terms (statistics of every term, the weight rule in fp64, one
combination pass) and `Solver.fit(loss_weights=...)` on top of them -- constant weights and `LossBalancer`.
Every kernel-level case runs on the emulator in the CPU tier and, marked `gpu`, on the device (the `tier` fixture).
  a. the kernels against the numpy fp64 statement of this file (`statement`; math.fsum for the sums), every shape, kind and mask
  b. the keep-old rule, clipping, momentum, repeatability, refusals
  c. fits: constant weights against a rescaled constraint, adaptive weights against a restatement on the oracle, state that carries on,
     nothing else moved, refusals of `fit`, two gloo ranks (CPU tier only) """
import ctypes
import math
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import pinn_configs as pc
from helpers import FixedBatches, close_or_arbitrated, export_params, make_solver, record_margin
from oracle import pinn_oracle as po

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'emu'))

FIXED, MAX_MEAN, NORM = 0, 1, 2
KIND_NAMES = {FIXED: 'fixed', MAX_MEAN: 'max_mean', NORM: 'norm'}
SENTINEL = np.float32(-7.25e33)             # what an output entry holds before the call: no sum of these inputs comes near it
STATE_DOUBLES = 48
W, UPDATES, COUNT, GMAX, SABS, SSQ, BAD = 0, 8, 9, 16, 24, 32, 40      # include/pinn.h: the state block of pinn_balance_terms


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


@pytest.fixture(scope='module', params=['emu', pytest.param('gpu', marks=pytest.mark.gpu)])
def tier(request):
    return Tier(request.param)


@pytest.fixture(scope='module')
def pa():
    import pydens_amd
    return pydens_amd


# ---- a. the kernels against the fp64 statement ---------------------------------------------------------------------------------------
def statement(G, n, mask, off_loss, kind, ref, update, momentum, lo, hi, lam):
    """ pinn_balance_terms in numpy fp64. G [T, ld] float32, lam [T] the weights before the call.
    -> dict(live, count, gmax, sabs, ssq, bad [T], lam (after), out [n] fp64 (every entry; the caller looks at the live ones), loss) """
    T = G.shape[0]
    live = np.ones(n, dtype=bool) if mask is None else (np.asarray(mask[:n]) != 0)
    live[off_loss] = False
    count = int(live.sum())
    g = G[:, :n].astype(np.float64)
    gmax, sabs, ssq, bad = np.zeros(T), np.zeros(T), np.zeros(T), np.zeros(T, dtype=bool)
    for j in range(T):
        a = np.abs(g[j, live])
        bad[j] = not np.isfinite(a).all()
        with np.errstate(all='ignore'):
            gmax[j] = np.nanmax(a) if a.size and not np.isnan(a).all() else 0.0
            sabs[j] = math.fsum(a) if not bad[j] else np.nan
            ssq[j] = math.fsum(a * a) if not bad[j] else np.nan
    lam = np.array(lam, dtype=np.float64)
    new = lam.copy()
    if kind != FIXED and update:
        hat = np.full(T, np.nan)
        if kind == MAX_MEAN:
            if not bad[ref] and gmax[ref] > 0 and count > 0:
                for j in range(T):
                    if j == ref:
                        hat[j] = 1.0
                    elif not bad[j] and sabs[j] / count > 0:
                        hat[j] = gmax[ref] / (sabs[j] / count)
        else:
            norms = np.array([math.sqrt(ssq[j]) if not bad[j] else 0.0 for j in range(T)])
            total = math.fsum(norms)
            for j in range(T):
                if not bad[j] and norms[j] > 0:
                    hat[j] = total / norms[j]
        for j in range(T):
            if np.isfinite(hat[j]):
                new[j] = min(max(momentum * lam[j] + (1.0 - momentum) * hat[j], lo), hi)
    with np.errstate(all='ignore'):
        out = (new[:, None] * g).sum(axis=0)
        bound = np.abs(new[:, None] * g).sum(axis=0)
    return dict(live=live, count=count, gmax=gmax, sabs=sabs, ssq=ssq, bad=bad, lam=new, out=out, bound=bound,
                loss=float((new * g[:, off_loss]).sum()), loss_bound=float(np.abs(new * g[:, off_loss]).sum()))


def make_terms(T, n, ld, seed, with_mask):
    """ T term rows whose magnitudes spread over 1e-6 .. 1e3 (so that the weights differ), positive losses in the loss slot, a mask with
    about a quarter zeros (the loss slot always masked) or none; entries n .. ld hold garbage the kernels must not look at """
    rng = np.random.RandomState(seed)
    scales = 10.0 ** (np.linspace(-6, 3, T) if T > 1 else np.zeros(1))
    G = (rng.standard_normal((T, ld)) * scales[:, None]).astype(np.float32)
    G[:, n:] = np.float32(3e30)
    off_loss = n - 1 if n % 2 else n // 2
    G[:, off_loss] = (rng.rand(T) + 0.5).astype(np.float32) * scales.astype(np.float32)
    mask = None
    if with_mask:
        mask = (rng.rand(n) > 0.25).astype(np.uint8)
        mask[off_loss] = 0
    return G, mask, off_loss


class Call:
    """ the buffers of one pinn_balance_terms call on the tier's device, outputs pre-filled with sentinels """
    def __init__(self, tier, G, n, mask, lam):
        T, ld = G.shape
        dev = tier.device
        self.tier, self.T, self.n, self.ld = tier, T, n, ld
        self.G = torch.from_numpy(G.copy()).to(dev)
        self.mask = None if mask is None else torch.from_numpy(mask.copy()).to(dev)
        self.state = torch.zeros(int(tier.lib.pinn_balance_state_bytes(T)) // 8, dtype=torch.float64, device=dev)
        assert self.state.numel() == STATE_DOUBLES
        host = (ctypes.c_double * T)(*[float(v) for v in lam])
        assert tier.lib.pinn_balance_init(self._p(self.state), self.state.numel() * 8, T, host, None) == 0, self.error()
        self.ws = torch.full((int(tier.lib.pinn_balance_workspace_bytes(n, T)) // 8, ), -1.0, dtype=torch.float64, device=dev)
        self.out = torch.full((ld, ), float(SENTINEL), dtype=torch.float32, device=dev)
        self.term_loss = torch.full((T + 1, ), float(SENTINEL), dtype=torch.float32, device=dev)
        self.weight = torch.full((T + 1, ), float(SENTINEL), dtype=torch.float32, device=dev)

    @staticmethod
    def _p(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def error(self):
        return self.tier.lib.pinn_last_error().decode()

    def run(self, off_loss, kind, ref, update, momentum, lo, hi, **over):
        a = dict(G=self._p(self.G), ld=self.ld, T=self.T, n=self.n, mask=self._p(self.mask), off_loss=off_loss, kind=kind, ref=ref,
                 update=update, momentum=momentum, lo=lo, hi=hi, state=self._p(self.state), state_bytes=self.state.numel() * 8,
                 out=self._p(self.out), term_loss=self._p(self.term_loss), weight=self._p(self.weight), ws=self._p(self.ws),
                 ws_bytes=self.ws.numel() * 8)
        a.update(over)
        rc = self.tier.lib.pinn_balance_terms(a['G'], a['ld'], a['T'], a['n'], a['mask'], a['off_loss'], a['kind'], a['ref'], a['update'],
                                              a['momentum'], a['lo'], a['hi'], a['state'], a['state_bytes'], a['out'], a['term_loss'],
                                              a['weight'], a['ws'], a['ws_bytes'], None)
        if self.tier.device == 'cuda':
            torch.cuda.synchronize()
        return rc

    def host(self):
        return dict(state=self.state.cpu().numpy(), out=self.out.cpu().numpy(), term_loss=self.term_loss.cpu().numpy(),
                    weight=self.weight.cpu().numpy(), ws=self.ws.cpu().numpy())


def check_call(got, want, G, n, off_loss, T, label):
    """ the derived tolerances: max|g| and the live count exact; the fp64 sums of non-negative terms within n 2^-53 (relative) of fsum, the
    weights therefore within 1e-9; an output entry one fp32 rounding of its fp64 sum: |out - ref| <= 2^-23 sum_j |w_j g_j|; the term
    losses exact; the weights out the fp32 rounding of the state's """
    st = got['state']
    assert st[COUNT] == want['count'], label
    ok = ~want['bad']
    assert np.array_equal(st[BAD:BAD + T] != 0, want['bad']), label
    assert np.array_equal(st[GMAX:GMAX + T][ok], want['gmax'][ok]), label
    rel = max(n, 1) * 2.0 ** -53
    for first, key in ((SABS, 'sabs'), (SSQ, 'ssq')):
        a, b = st[first:first + T][ok], want[key][ok]
        assert np.all(np.abs(a - b) <= rel * np.abs(b)), (label, key, a, b)
    lam = st[W:W + T]
    assert np.all(np.isfinite(lam)), (label, lam)
    assert np.all(np.abs(lam - want['lam']) <= 1e-9 * np.abs(want['lam'])), (label, lam, want['lam'])
    out, live = got['out'], want['live']
    err = np.abs(out[:n].astype(np.float64) - want['out'])[live]
    assert np.all(err <= 2.0 ** -23 * want['bound'][live]), (label, float(err.max()) if err.size else 0.0)
    assert abs(float(out[off_loss]) - want['loss']) <= 2.0 ** -23 * want['loss_bound'], label
    untouched = np.ones(out.size, dtype=bool)
    untouched[:n] = ~live
    untouched[off_loss] = False
    assert np.array_equal(out[untouched].view(np.uint32), np.full(int(untouched.sum()), SENTINEL).view(np.uint32)), label
    assert np.array_equal(got['term_loss'][:T].view(np.uint32), G[:, off_loss].view(np.uint32)), label
    assert np.array_equal(got['weight'][:T].view(np.uint32), lam.astype(np.float32).view(np.uint32)), label
    assert got['term_loss'][T] == SENTINEL and got['weight'][T] == SENTINEL, label


@pytest.mark.parametrize('n', [1, 5, 1023, 1024, 1025, 4095, 4096, 4097, 8193])
def test_kernels_match_the_fp64_statement(tier, n):
    """ one thread, a ragged 16-byte piece, one slice of the combine and of the stats pass +- 1, two workgroups + 1 -- times the number
    of terms, the row stride, mask or none, every kind and both ends for the reference term """
    for T in (1, 2, 3, 8):
        for pad in (0, 8):
            ld = (n + 3) // 4 * 4 + pad
            for with_mask in (True, False):
                G, mask, off_loss = make_terms(T, n, ld, 1000 * T + n + pad, with_mask)
                lam0 = np.random.RandomState(T + n).rand(T) * 1.5 + 0.5
                for kind in (FIXED, MAX_MEAN, NORM):
                    for ref in sorted({0, T - 1}):
                        label = f'{tier.name} n={n} T={T} ld={ld} mask={with_mask} {KIND_NAMES[kind]} ref={ref}'
                        call = Call(tier, G, n, mask, lam0)
                        assert call.run(off_loss, kind, ref, 1, 0.25, 0.0, 1e12) == 0, (label, call.error())
                        want = statement(G, n, mask, off_loss, kind, ref, 1, 0.25, 0.0, 1e12, lam0)
                        got = call.host()
                        check_call(got, want, G, n, off_loss, T, label)
                        assert got['state'][UPDATES] == (0.0 if kind == FIXED else 1.0), label
                        if kind != FIXED and T > 1 and want['count'] > 0:
                            assert len(set(np.round(np.log10(got['state'][W:W + T]), 3))) > 1, label        # (the weights differ)


def test_output_may_be_row_zero_itself(tier):
    n, T = 4097, 3
    G, mask, off_loss = make_terms(T, n, 4100, 5, True)
    lam0 = [1.0, 2.0, 3.0]
    plain, alias = Call(tier, G, n, mask, lam0), Call(tier, G, n, mask, lam0)
    assert plain.run(off_loss, NORM, 0, 1, 0.5, 0.0, 1e12) == 0
    assert alias.run(off_loss, NORM, 0, 1, 0.5, 0.0, 1e12, out=alias._p(alias.G)) == 0, alias.error()
    a, b = plain.host(), alias.G.cpu().numpy()
    live = statement(G, n, mask, off_loss, NORM, 0, 1, 0.5, 0.0, 1e12, lam0)['live']
    live[off_loss] = True
    assert np.array_equal(a['out'][:n][live].view(np.uint32), b[0, :n][live].view(np.uint32))
    assert np.array_equal(b[0, :n][~live].view(np.uint32), G[0, :n][~live].view(np.uint32))         # masked entries of row 0: as they were
    assert np.array_equal(b[1:].view(np.uint32), G[1:].view(np.uint32))
    assert np.array_equal(a['state'], alias.state.cpu().numpy())


# ---- b. the keep-old rule, clipping, momentum, repeatability, refusals ---------------------------------------------------------------
def _keep_case(n=1500, T=3, seed=9):
    G, mask, off_loss = make_terms(T, n, (n + 3) // 4 * 4, seed, True)
    live = np.flatnonzero(mask)
    return G, mask, off_loss, live


@pytest.mark.parametrize('kind', [MAX_MEAN, NORM])
@pytest.mark.parametrize('trouble', ['zero', 'nan', 'inf'])
def test_a_term_in_trouble_keeps_its_weight_and_the_others_update(tier, kind, trouble):
    G, mask, off_loss, live = _keep_case()
    n, T = 1500, 3
    lam0 = np.array([0.7, 1.3, 2.1])
    j = 1                       # the term in trouble; the reference is term 0
    if trouble == 'zero':
        G[j, live] = 0.0
        G[j, ~mask.astype(bool)] = 5.0          # (what is not live does not count)
    else:
        G[j, live[700]] = np.float32(np.nan if trouble == 'nan' else -np.inf)
    call = Call(tier, G, n, mask, lam0)
    assert call.run(off_loss, kind, 0, 1, 0.5, 0.0, 1e12) == 0, call.error()
    st = call.host()['state']
    lam = st[W:W + T]
    want = statement(G, n, mask, off_loss, kind, 0, 1, 0.5, 0.0, 1e12, lam0)
    assert lam[j] == lam0[j] and np.all(np.isfinite(lam))
    assert lam[2] != lam0[2] and abs(lam[2] - want['lam'][2]) <= 1e-9 * want['lam'][2]
    assert abs(lam[0] - want['lam'][0]) <= 1e-9 * want['lam'][0]
    assert (st[BAD + j] != 0) == (trouble != 'zero')
    assert np.array_equal(call.host()['weight'][:T], lam.astype(np.float32))


@pytest.mark.parametrize('trouble', ['zero', 'nan', 'inf'])
def test_a_reference_in_trouble_keeps_every_weight_under_max_mean(tier, trouble):
    G, mask, off_loss, live = _keep_case()
    n, T, ref = 1500, 3, 2
    lam0 = np.array([0.7, 1.3, 2.1])
    if trouble == 'zero':
        G[ref, live] = 0.0
    else:
        G[ref, live[3]] = np.float32(np.nan if trouble == 'nan' else np.inf)
    call = Call(tier, G, n, mask, lam0)
    assert call.run(off_loss, MAX_MEAN, ref, 1, 0.5, 0.0, 1e12) == 0, call.error()
    assert np.array_equal(call.host()['state'][W:W + T], lam0)


@pytest.mark.parametrize('kind', [MAX_MEAN, NORM])
def test_update_zero_changes_no_weight_and_still_combines(tier, kind):
    G, mask, off_loss, _ = _keep_case()
    n, T = 1500, 3
    lam0 = np.array([0.7, 1.3, 2.1])
    call = Call(tier, G, n, mask, lam0)
    assert call.run(off_loss, kind, 0, 0, 0.5, 0.0, 1e12) == 0, call.error()
    got = call.host()
    assert np.array_equal(got['state'][W:W + T], lam0) and got['state'][UPDATES] == 0.0
    check_call(got, statement(G, n, mask, off_loss, kind, 0, 0, 0.5, 0.0, 1e12, lam0), G, n, off_loss, T, 'update=0')


def test_clipping_holds_at_both_ends(tier):
    G, mask, off_loss, _ = _keep_case()         # (term magnitudes 1e-6, 3e-2, 1e3: the raw weights span many decades)
    n, T = 1500, 3
    for kind, ref in ((MAX_MEAN, 1), (NORM, 0)):
        call = Call(tier, G, n, mask, [1.0, 1.0, 1.0])
        assert call.run(off_loss, kind, ref, 1, 0.0, 2.0, 50.0) == 0, call.error()
        lam = call.host()['state'][W:W + T]
        raw = statement(G, n, mask, off_loss, kind, ref, 1, 0.0, 0.0, 1e300, [1.0] * 3)['lam']
        assert raw.min() < 2.0 and raw.max() > 50.0
        assert np.array_equal(lam, np.clip(statement(G, n, mask, off_loss, kind, ref, 1, 0.0, 2.0, 50.0, [1.0] * 3)['lam'], 2.0, 50.0))
        assert lam.min() == 2.0 and lam.max() == 50.0
        call = Call(tier, G, n, mask, [1.0, 1.0, 1.0])
        assert call.run(off_loss, kind, ref, 1, 0.0, 3.0, 3.0) == 0, call.error()           # lo == hi is allowed
        assert np.array_equal(call.host()['state'][W:W + T], [3.0, 3.0, 3.0])


@pytest.mark.parametrize('kind', [MAX_MEAN, NORM])
def test_momentum(tier, kind):
    G, mask, off_loss, _ = _keep_case()
    n, T = 1500, 3
    lam0 = np.array([0.7, 1.3, 2.1])
    hat = statement(G, n, mask, off_loss, kind, 1, 1, 0.0, 0.0, 1e12, lam0)['lam']
    call = Call(tier, G, n, mask, lam0)
    assert call.run(off_loss, kind, 1, 1, 0.0, 0.0, 1e12) == 0               # momentum 0 reaches hat in one call
    assert np.all(np.abs(call.host()['state'][W:W + T] - hat) <= 1e-9 * hat)
    call = Call(tier, G, n, mask, lam0)
    for _ in range(2):                                                      # momentum 1 never moves
        assert call.run(off_loss, kind, 1, 1, 1.0, 0.0, 1e12) == 0
    assert np.array_equal(call.host()['state'][W:W + T], lam0) and call.host()['state'][UPDATES] == 2.0
    call, lam = Call(tier, G, n, mask, lam0), lam0.copy()
    for k in range(3):                                                      # three calls with momentum 0.5 follow the recurrence
        assert call.run(off_loss, kind, 1, 1, 0.5, 0.0, 1e12) == 0
        lam = 0.5 * lam + 0.5 * hat
        got = call.host()['state'][W:W + T]
        assert np.all(np.abs(got - lam) <= 1e-9 * lam), (k, got, lam)


def test_two_calls_from_equal_state_are_equal_bit_for_bit(tier, monkeypatch):
    monkeypatch.delenv('PINN_EMU_SHUFFLE', raising=False)
    n, T = 8193, 8
    G, mask, off_loss = make_terms(T, n, 8196, 21, True)
    lam0 = np.linspace(0.5, 2.0, T)

    def run():
        call = Call(tier, G, n, mask, lam0)
        for kind in (MAX_MEAN, NORM):
            assert call.run(off_loss, kind, 3, 1, 0.75, 0.0, 1e12) == 0
        return call.host()
    a, b = run(), run()
    for key in ('state', 'ws'):
        assert np.array_equal(a[key].view(np.uint64), b[key].view(np.uint64)), key
    for key in ('out', 'term_loss', 'weight'):
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key
    if tier.name == 'emu':                      # the waves of a workgroup in shuffled order: same sums, same weights
        for seed in ('3', '11'):
            monkeypatch.setenv('PINN_EMU_SHUFFLE', seed)
            c = run()
            monkeypatch.delenv('PINN_EMU_SHUFFLE')
            assert np.array_equal(a['state'].view(np.uint64), c['state'].view(np.uint64))
            assert np.array_equal(a['ws'].view(np.uint64), c['ws'].view(np.uint64))
            assert np.array_equal(a['out'].view(np.uint32), c['out'].view(np.uint32))


def test_refusals_launch_nothing(tier):
    """ every refusal: non-zero, a text, and output, state and workspace as they were (sentinels) """
    n, T = 1027, 3
    G, mask, off_loss = make_terms(T, n, 1028, 2, True)
    call = Call(tier, G, n, mask, [1.0, 2.0, 3.0])
    before = call.host()
    small = torch.zeros(4, dtype=torch.float64, device=tier.device)
    nan, inf = float('nan'), float('inf')
    cases = [dict(T=0), dict(T=9), dict(T=-1), dict(G=None), dict(state=None), dict(out=None), dict(ws=None),
             dict(ld=1030), dict(ld=1024), dict(n=0), dict(off_loss=-1), dict(off_loss=n), dict(kind=3), dict(kind=-1),
             dict(ref=-1), dict(ref=T), dict(momentum=-0.1), dict(momentum=1.5), dict(momentum=nan),
             dict(lo=-1.0), dict(lo=2.0, hi=1.0), dict(hi=inf), dict(lo=nan), dict(hi=nan),
             dict(state_bytes=STATE_DOUBLES * 8 - 8), dict(ws_bytes=call.ws.numel() * 8 - 8), dict(state=call._p(small), state_bytes=32),
             dict(out=ctypes.c_void_p(call.G.data_ptr() + 16)), dict(out=ctypes.c_void_p(call.G.data_ptr() + 4 * 1028)),
             dict(out=ctypes.c_void_p(call.out.data_ptr() + 4))]
    for over in cases:
        args = dict(off_loss=off_loss, kind=MAX_MEAN, ref=0, update=1, momentum=0.5, lo=0.0, hi=1e6)
        args.update(over)
        assert call.run(**args) != 0, over
        assert call.error(), over
        after = call.host()
        for key in before:
            assert np.array_equal(before[key].view(np.uint8), after[key].view(np.uint8)), (over, key)
        assert np.array_equal(call.G.cpu().numpy().view(np.uint32), G.view(np.uint32)), over
    # the queries and init
    lib = tier.lib
    assert lib.pinn_balance_state_bytes(0) == 0 and lib.pinn_balance_state_bytes(9) == 0 and lib.pinn_balance_state_bytes(8) == STATE_DOUBLES * 8
    assert lib.pinn_balance_workspace_bytes(0, 2) == 0 and lib.pinn_balance_workspace_bytes(10, 0) == 0
    assert lib.pinn_balance_workspace_bytes(4097, 8) >= 2 * 33 * 8
    state = torch.full((STATE_DOUBLES, ), 5.0, dtype=torch.float64, device=tier.device)
    two = (ctypes.c_double * 2)
    for args in ((call._p(state), state.numel() * 8, 0, two(1.0, 1.0)), (call._p(state), state.numel() * 8, 9, two(1.0, 1.0)),
                 (None, state.numel() * 8, 2, two(1.0, 1.0)), (call._p(state), state.numel() * 8, 2, None),
                 (call._p(state), 8, 2, two(1.0, 1.0)), (call._p(state), state.numel() * 8, 2, two(1.0, -1.0)),
                 (call._p(state), state.numel() * 8, 2, two(nan, 1.0)), (call._p(state), state.numel() * 8, 2, two(inf, 1.0))):
        assert lib.pinn_balance_init(*args, None) != 0 and lib.pinn_last_error(), args[1:3]
        assert bool((state == 5.0).all())
    assert lib.pinn_balance_init(call._p(state), state.numel() * 8, 2, two(0.0, 4.0), None) == 0
    assert state.cpu().tolist() == [0.0, 4.0] + [0.0] * (STATE_DOUBLES - 2)


# ---- c. Solver.fit(loss_weights=...) ---------------------------------------------------------------------------------------------------
RTOL = 1e-5                 # the project's bar for losses and field (README)
LR = 0.01
PX, PY = [[0.3], [0.7], [0.55]], [[0.6], [0.2], [0.85]]


def problem(D, dtype, device, kind, scale=1.0):
    """ the config-1 problem (Poisson on the unit square, hard boundary value 1, the 10-12-15 net) with one soft constraint at three fixed
    points: kind 'value' scale * (f(p) - 1), kind 'neumann' D(f(p), p_x) - 2 """
    cfg = pc.make_config('cfg1', D, torch)

    def value(f, x, y):
        px, py = torch.tensor(PX, dtype=dtype, device=device), torch.tensor(PY, dtype=dtype, device=device)
        return scale * (f(px, py) - 1)

    def neumann(f, x, y):
        px = torch.tensor(PX, dtype=dtype, device=device, requires_grad=True)
        py = torch.tensor(PY, dtype=dtype, device=device)
        return D(f(px, py), px) - 2.0
    return cfg['equation'], cfg['solver_kwargs'], value if kind == 'value' else neumann


def product_solver(pa, tier, kind, start, scale=1.0, path='fused'):
    eq, kw, con = problem(pa.D, torch.float32, tier.device, kind, scale)
    solver = pa.Solver(eq, constraints=con, **kw, **tier.solver_kwargs)
    if start is not None:
        from helpers import load_params
        load_params(solver, start)
    solver.use_fused = path == 'fused'
    return solver


def oracle_solver(kind, dtype, start=None, seed=11):
    torch.manual_seed(seed)
    eq, kw, con = problem(po.D, dtype, 'cpu', kind)
    oracle = po.OracleSolver(eq, constraints=con, dtype=dtype, **kw)
    if start is not None:
        oracle.import_params(start)
    return oracle


def batches(steps, seed=21, n=40):
    return np.random.RandomState(seed).rand(steps, n, 2).astype(np.float32)


TERMS = ['equation', 'constraint_0']


def balanced_oracle_fit(oracle, pts, kind, momentum=0.9, period=1, reference='equation', initial=1.0, clip=(0.0, 1e6), lr=LR, terms=TERMS):
    """ the independent statement: per iteration the gradient of every term by torch autograd, the weights by the numpy formulas of
    `statement` over all entries the terms reach, the weighted gradient, one torch Adam step -> (term losses, weights) per iteration;
    `oracle.losses` takes the weighted sums """
    params = [p for p in oracle.model.parameters() if p.requires_grad]
    oracle.optimizer = torch.optim.Adam(params, lr=lr)
    lam = np.full(len(terms), float(initial))
    ref = terms.index(reference)
    code = {'max_mean': MAX_MEAN, 'norm': NORM}[kind]
    term_rows, weight_rows = [], []
    zero = torch.zeros(1, dtype=oracle.dtype)
    for it, arr in enumerate(pts):
        xs = [torch.tensor(arr[:, i:i + 1], dtype=oracle.dtype).requires_grad_() for i in range(arr.shape[1])]
        u_hat = oracle.ctx.run(oracle.model, oracle.reshape_and_concat(xs))
        losses, grads = [], []
        for term in terms:
            if term == 'equation':
                loss = torch.nn.functional.mse_loss(oracle.ctx.run(oracle.equation, u_hat, *xs), torch.zeros_like(xs[0]))
            else:
                value = oracle.ctx.run(oracle.constraints[int(term[-1])], lambda *a: oracle.model(oracle.reshape_and_concat(a)), *xs)
                loss = (value ** 2).mean() + 0 * zero.sum()
            losses.append(loss.detach())
            grads.append(torch.autograd.grad(loss, params, allow_unused=True, retain_graph=True))
        reached = [k for k in range(len(params)) if any(g[k] is not None for g in grads)]
        rows = np.stack([np.concatenate([(g[k] if g[k] is not None else torch.zeros_like(params[k])).detach().numpy().ravel() for k in reached])
                         for g in grads])
        G = np.concatenate([rows, np.zeros((len(terms), 1), dtype=rows.dtype)], axis=1)          # (the last entry: the loss slot)
        want = statement(G.astype(np.float64).astype(np.float32) if oracle.dtype == torch.float32 else _Exact(G), G.shape[1], None,
                         G.shape[1] - 1, code, ref, it % period == 0, momentum, clip[0], clip[1], lam)
        lam = want['lam']
        for k, p in enumerate(params):
            p.grad = None
            if k in reached:
                total = sum(float(w) * (g[k] if g[k] is not None else torch.zeros_like(p)).double() for w, g in zip(lam, grads))
                p.grad = total.to(oracle.dtype)
        oracle.optimizer.step()
        oracle.losses.append(np.asarray(sum(float(w) * float(loss) for w, loss in zip(lam, losses))))
        term_rows.append([float(loss) for loss in losses])
        weight_rows.append(lam.copy())
    return np.array(term_rows), np.array(weight_rows)


class _Exact:
    """ fp64 term rows handed to `statement` as they are (the arbiter: no rounding to fp32 on the way) """
    def __init__(self, G):
        self.G, self.shape = G, G.shape

    def __getitem__(self, key):
        return _ExactView(self.G[key])


class _ExactView:
    def __init__(self, a):
        self.a = a

    def astype(self, dtype):
        return self.a


def judged(test, case, quantity, got, want32, want64_fn, atol=0.0, adam_move=None):
    ok, err, arb = close_or_arbitrated(got, want32, want64_fn, RTOL, atol=atol, adam_move=adam_move)
    record_margin(test, case, quantity, err, RTOL, arb)
    print(f'{test} {case} {quantity}: {err:.3e} (bar {RTOL:.0e}) arbitrated={arb}')
    assert ok, (case, quantity, err, np.asarray(got).ravel()[:8], np.asarray(want32).ravel()[:8])


@pytest.mark.parametrize('path', ['fused', 'generic'])
def test_constant_weights_are_what_they_say(pa, tier, path):
    """ weights (1, 4) against a plain fit whose constraint returns 2 * (f(x) - 1): MSE turns the 2 into 4 """
    start = oracle_solver('value', torch.float32).export_params()
    pts = batches(4)
    weighted = product_solver(pa, tier, 'value', start, path=path)
    weighted.fit(4, 40, sampler=FixedBatches(pts), lr=LR, loss_terms=TERMS, loss_weights={'equation': 1, 'constraint_0': 4.0})
    scaled = product_solver(pa, tier, 'value', start, scale=2.0, path=path)
    scaled.fit(4, 40, sampler=FixedBatches(pts), lr=LR, loss_terms=TERMS)
    assert weighted.last_fit_path == scaled.last_fit_path == path and weighted.last_fit_balance == f'fixed/{path}'
    assert scaled.last_fit_balance is None
    arbiter = {}

    def o64():
        if 'o' not in arbiter:
            torch.manual_seed(11)
            eq, kw, con = problem(po.D, torch.float64, 'cpu', 'value', 2.0)
            o = arbiter['o'] = po.OracleSolver(eq, constraints=con, dtype=torch.float64, **kw)
            o.import_params(start)
            o.fit(niters=4, batch_size=40, points=pts, lr=LR, loss_terms=TERMS)
        return arbiter['o']
    case = f'{tier.name} constant {path}'
    got, want = [float(v) for v in weighted.losses], [float(v) for v in scaled.losses]
    judged('loss_balance', case, 'losses', got, want, lambda: [float(v) for v in o64().losses])
    for i, (a, b) in enumerate(zip(export_params(weighted), export_params(scaled))):
        judged('loss_balance', case, f'parameters[{i}]', a, b, lambda i=i: o64().export_params()[i], atol=2e-6, adam_move=LR * 4)
    tl, wh = weighted.term_losses, weighted.loss_weight_history
    assert tl.shape == wh.shape == (4, 2) and tl.dtype == np.float32
    assert np.array_equal(wh, np.tile(np.float32([1.0, 4.0]), (4, 1)))
    rebuilt = tl[:, 1].astype(np.float64) * 4 + tl[:, 0]
    assert np.all(np.abs(rebuilt - got) <= 2.0 ** -23 * rebuilt)            # (the loss slot: one fp32 rounding of the fp64 sum)
    assert weighted.loss_weights == {'equation': 1.0, 'constraint_0': 4.0}
    # a sequence aligned with loss_terms is the same fit
    again = product_solver(pa, tier, 'value', start, path=path)
    again.fit(4, 40, sampler=FixedBatches(pts), lr=LR, loss_terms=TERMS, loss_weights=[1, 4.0])
    assert torch.equal(again.model.flat, weighted.model.flat)


@pytest.mark.parametrize('path', ['fused', 'generic'])
@pytest.mark.parametrize('constraint', ['value', 'neumann'])
@pytest.mark.parametrize('kind,period', [('max_mean', 1), ('max_mean', 2), ('norm', 1), ('norm', 2)])
def test_adaptive_weights_follow_the_restatement(pa, tier, path, constraint, kind, period):
    steps = 4
    pts = batches(steps)
    o32 = oracle_solver(constraint, torch.float32)
    start = o32.export_params()
    terms32, weights32 = balanced_oracle_fit(o32, pts, kind, momentum=0.5, period=period)
    arbiter = {}

    def o64():
        if 'o' not in arbiter:
            o = oracle_solver(constraint, torch.float64, start)
            arbiter['o'] = (o, ) + balanced_oracle_fit(o, pts.astype(np.float64), kind, momentum=0.5, period=period)
        return arbiter['o']
    solver = product_solver(pa, tier, constraint, start, path=path)
    balancer = pa.LossBalancer(kind, momentum=0.5, period=period)
    solver.fit(steps, 40, sampler=FixedBatches(pts), lr=LR, loss_terms=TERMS, loss_weights=balancer)
    assert solver.last_fit_path == path and solver.last_fit_balance == f'{kind}/{path}', solver.constraint_errors
    case = f'{tier.name} {kind}/{period} {constraint} {path}'
    judged('loss_balance', case, 'losses', [float(v) for v in solver.losses], [float(v) for v in o32.losses],
           lambda: [float(v) for v in o64()[0].losses])
    judged('loss_balance', case, 'term_losses', solver.term_losses, terms32, lambda: o64()[1])
    judged('loss_balance', case, 'weights', solver.loss_weight_history, weights32, lambda: o64()[2])
    for i, (a, b) in enumerate(zip(export_params(solver), o32.export_params())):
        judged('loss_balance', case, f'parameters[{i}]', a, b, lambda i=i: o64()[0].export_params()[i], atol=2e-6, adam_move=LR * steps)
    assert len(set(np.round(weights32[-1], 6))) == 2 and np.all(np.abs(np.log(weights32[-1])) < np.log(1e5))     # (no statistic near zero)
    if period == 2:
        wh = solver.loss_weight_history
        assert np.array_equal(wh[0], wh[1]) and np.array_equal(wh[2], wh[3]) and not np.array_equal(wh[1], wh[2])
    assert solver.loss_weights == pytest.approx(dict(zip(TERMS, solver.loss_weight_history[-1].astype(np.float64))), rel=1e-6)


def test_state_carries_on_and_a_fresh_balancer_restarts(pa, tier):
    start = oracle_solver('value', torch.float32).export_params()
    pts = batches(5)
    whole = product_solver(pa, tier, 'value', start)
    whole.fit(5, 40, sampler=FixedBatches(pts), lr=LR, loss_terms=TERMS, loss_weights=pa.LossBalancer('max_mean', period=2))
    parts = product_solver(pa, tier, 'value', start)
    balancer = pa.LossBalancer('max_mean', period=2)
    parts.fit(3, 40, sampler=FixedBatches(pts[:3]), lr=LR, loss_terms=TERMS, loss_weights=balancer)
    parts.fit(2, 40, sampler=FixedBatches(pts[3:]), lr=LR, loss_terms=TERMS, optimizer=None, loss_weights=balancer)
    assert np.array_equal(np.float32(whole.losses), np.float32(parts.losses))
    assert np.array_equal(whole.loss_weight_history, parts.loss_weight_history) and parts.loss_weight_history.shape == (5, 2)
    assert np.array_equal(whole.term_losses, parts.term_losses)
    assert torch.equal(whole.model.flat, parts.model.flat) and torch.equal(whole._balance.state, balancer.state)
    fresh = pa.LossBalancer('max_mean', momentum=1.0, initial=3.0)
    parts.fit(1, 40, sampler=FixedBatches(pts[:1]), lr=LR, loss_terms=TERMS, optimizer=None, loss_weights=fresh)
    assert np.array_equal(parts.loss_weight_history[-1], np.float32([3.0, 3.0])) and fresh.weights == {'equation': 3.0, 'constraint_0': 3.0}


class _Counting:
    """ the bound library with every pinn_balance_* entry point counted """
    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('pinn_balance_'):
            return fn

        def counted(*args):
            self.calls += 1
            return fn(*args)
        return counted


def test_nothing_else_moves(pa, tier):
    start = oracle_solver('value', torch.float32).export_params()
    pts = batches(3)
    used = product_solver(pa, tier, 'value', start)
    used.fit(2, 40, sampler=FixedBatches(batches(2, seed=5)), lr=LR, loss_terms=TERMS, loss_weights=pa.LossBalancer('norm'))
    from helpers import load_params
    load_params(used, start)
    fresh = product_solver(pa, tier, 'value', start)
    counting = _Counting(used.model.net.lib)
    used.model.net.lib = counting
    for solver in (used, fresh):
        solver.fit(3, 40, sampler=FixedBatches(pts), lr=LR, loss_terms=TERMS)
    assert counting.calls == 0 and used.last_fit_balance is None
    assert np.array_equal(np.float32(used.losses[-3:]), np.float32(fresh.losses)) and torch.equal(used.model.flat, fresh.model.flat)
    # the equation alone, no weights: the one-launch chunks as ever, and still no balance call
    for solver in (used, fresh):
        solver.fit(3, 40, sampler=FixedBatches(pts), lr=LR)
    assert counting.calls == 0 and torch.equal(used.model.flat, fresh.model.flat)
    used.fit(1, 40, sampler=FixedBatches(pts), lr=LR, loss_weights={'equation': 2.0})          # (a constant weight on the equation alone)
    assert counting.calls > 0 and used.last_fit_balance == 'fixed/fused' and used.term_losses.shape[1] == 1


def test_fit_refuses_with_the_reason(pa, tier):
    solver = product_solver(pa, tier, 'value', None)
    before = solver.model.flat.clone()
    fit = lambda **kw: solver.fit(1, 40, sampler=FixedBatches(batches(1)), lr=LR, **kw)
    nan = float('nan')
    for kw, exc, text in (
            (dict(loss_terms=TERMS, loss_weights={'equation': 1.0, 'constraint_0': 1.0, 'constraint_1': 2.0}), ValueError, 'constraint_1'),
            (dict(loss_terms=TERMS, loss_weights={'equation': 1.0}), ValueError, 'no weight'),
            (dict(loss_terms=TERMS, loss_weights=[1.0]), ValueError, '1 weights'),
            (dict(loss_terms=TERMS, loss_weights={'equation': 1.0, 'constraint_0': -1.0}), ValueError, 'finite number >= 0'),
            (dict(loss_terms=TERMS, loss_weights={'equation': nan, 'constraint_0': 1.0}), ValueError, 'finite number >= 0'),
            (dict(loss_terms=['equation'] + ['constraint_0'] * 8, loss_weights=[1.0] * 9), (ValueError, NotImplementedError), 'at most 8'),
            (dict(loss_terms=['equation', 'boundary'], loss_weights=[1.0, 1.0]), ValueError, "neither 'equation' nor"),
            (dict(loss_terms=['equation', 'constraint_3'], loss_weights=[1.0, 1.0]), ValueError, "neither 'equation' nor"),
            (dict(loss_terms=['equation'], loss_weights=pa.LossBalancer('norm')), ValueError, 'single term'),
            (dict(loss_terms=TERMS, loss_weights=pa.LossBalancer('max_mean', reference='constraint_1')), ValueError, 'reference'),
            (dict(loss_terms=TERMS, loss_weights=pa.LossBalancer('norm'), optimizer='LBFGS'), NotImplementedError, 'closure'),
            (dict(loss_terms=TERMS, loss_weights='equal'), ValueError, 'LossBalancer')):
        with pytest.raises(exc, match=text):
            fit(**kw)
    assert torch.equal(solver.model.flat, before) and solver.optimizer is None
    with pytest.raises(ValueError):
        pa.LossBalancer('ntk')
    with pytest.raises(ValueError):
        pa.LossBalancer(momentum=1.5)
    with pytest.raises(ValueError):
        pa.LossBalancer(clip=(2.0, 1.0))
    import pydens
    assert pydens.LossBalancer is pa.LossBalancer
    # constant weights with a closure optimizer are served: rows + combine inside the closure
    solver.fit(2, 40, sampler=FixedBatches(batches(2)), loss_terms=TERMS, loss_weights=[1.0, 4.0], optimizer='LBFGS', lr=0.5, max_iter=3)
    assert solver.last_fit_balance.startswith('fixed/') and solver.term_losses.shape == (2, 2)
    assert np.all(np.isfinite(np.float32(solver.losses)))


# ---- data parallel (CPU tier only: two gloo ranks on the emulator) --------------------------------------------------------------------
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
    eq, kw, con = problem(pa.D, torch.float32, 'cpu', 'value')
    solver = pa.Solver(eq, constraints=con, **kw, _lib=lib, device='cpu')
    pts = batches(3, seed=33, n=80)
    if rank == 0:
        np.save(os.path.join(out_dir, 'start.npy'), solver.model.flat.detach().numpy().copy())
    balancer = pa.LossBalancer('max_mean')
    solver.fit(3, 80, sampler=FixedBatches(pts[:, 40 * rank:40 * rank + 40]), lr=LR, loss_terms=TERMS, loss_weights=balancer)
    np.savez(os.path.join(out_dir, f'rank{rank}.npz'), flat=solver.model.flat.detach().numpy(), weights=solver.loss_weight_history,
             losses=np.float32(solver.losses), terms=solver.term_losses, state=balancer.state.numpy())
    dist.destroy_process_group()


def test_two_ranks_hold_the_same_weights(pa):
    """ gloo, two ranks on the emulator: identical weights and parameters on both, and those of one rank on the concatenated batch """
    tier = Tier('emu')
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_dp_worker, args=(2, _free_port(), tmp), nprocs=2, join=True)
        a, b = (np.load(os.path.join(tmp, f'rank{rank}.npz')) for rank in range(2))
        start = np.load(os.path.join(tmp, 'start.npy'))
    for key in ('flat', 'weights', 'losses', 'terms', 'state'):
        assert np.array_equal(a[key], b[key]), key
    single = product_solver(pa, tier, 'value', None)
    with torch.no_grad():
        single.model.flat.copy_(torch.from_numpy(start))
    single.fit(3, 80, sampler=FixedBatches(batches(3, seed=33, n=80)), lr=LR, loss_terms=TERMS, loss_weights=pa.LossBalancer('max_mean'))
    for key, got, want in (('weights', a['weights'], single.loss_weight_history), ('losses', a['losses'], np.float32(single.losses)),
                           ('terms', a['terms'], single.term_losses)):
        assert np.all(np.abs(got.astype(np.float64) - want) <= RTOL * np.abs(want)), (key, got, want)
    flat = single.model.flat.detach().numpy().astype(np.float64)
    assert np.linalg.norm(a['flat'] - flat) <= RTOL * np.linalg.norm(flat) + 2e-6 * np.sqrt(flat.size)
