""" Causal training weights: the device kernels behind include/pinn.h pinn_causal_weights (bin statistics, the weight rule and the tolerance
ladder in fp64 by one workgroup, one pass that hands every point its weight) and `Solver.fit(causal=CausalWeights(...))` on top of them.
Every kernel-level case runs on the emulator in the CPU tier and, marked `gpu`, on the device (the `tier` fixture).
  a. the kernels against the numpy fp64 statement of this file (`statement`; math.fsum for the sums): sizes, bins, strides, edges
  b. repeatability, bit for bit, also under the emulator's shuffled wave order
  c. the tolerance ladder against `Ladder`, the statement of its decision
  d. refusals: non-zero, a text, nothing written
  e. fits: one iteration against a restatement on the oracle, histories, the ladder carried on, eps = 0, causal=None, refusals of `fit` """
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

from helpers import FixedBatches, close_or_arbitrated, export_grads, export_params, load_params, record_margin
from oracle import pinn_oracle as po

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'emu'))

SENTINEL = np.float32(-7.25e33)             # what an output entry holds before the call: no weight comes near it
STATE_DOUBLES = 208
# include/pinn.h: the state block of pinn_causal_weights
EPS, N_EPS, INDEX, DELTA, CONVERGED, BAD, CALLS, EPS_USED, MEAN_SQ, NK, LK, WK = 0, 8, 9, 10, 11, 12, 13, 14, 15, 16, 80, 144
MAX_BINS = 64
FOLD = 256 * 256                            # points above which a workgroup of the stats pass takes more than one chunk


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


# ---- the statement (section "Definition" of include/pinn.h pinn_causal_weights, in numpy fp64) ---------------------------------------------
def bins_of(t, t_lo, t_hi, M):
    with np.errstate(all='ignore'):
        q = np.floor((np.asarray(t).astype(np.float64) - t_lo) / (t_hi - t_lo) * M)
        k = np.where(q >= M - 1, M - 1, np.where(q >= 1, q, 0))         # (NaN fails both comparisons: bin 0)
    return k.astype(np.int64)


def statistics(t, r, M, t_lo, t_hi):
    """ -> dict(k [N], n_k [M], L [M], P [M] the exclusive prefix of L, non_finite, mean_sq); r in whatever precision it comes """
    k = bins_of(t, t_lo, t_hi, M)
    r64 = np.asarray(r).astype(np.float64).reshape(-1)
    finite = np.isfinite(r64)
    with np.errstate(all='ignore'):
        sq = np.where(finite, r64 * r64, 0.0)
    n_k = np.bincount(k, minlength=M)
    L = np.array([math.fsum(sq[k == j]) / n_k[j] if n_k[j] else 0.0 for j in range(M)])
    P = np.array([math.fsum(L[:j]) for j in range(M)])
    return dict(k=k, n_k=n_k, L=L, P=P, non_finite=not bool(finite.all()), mean_sq=math.fsum(sq) / len(r64))


def weights_of(stats, eps):
    if eps == 0:
        return np.ones_like(stats['P'])
    with np.errstate(all='ignore'):
        return np.exp(-(eps * stats['P']))


class Ladder:
    """ the tolerance ladder: a call uses the tolerance at the index; then, with update and min_k w_k > delta, the index moves up for the
    next call -- at the last tolerance `converged` is set instead """
    def __init__(self, eps, delta):
        self.eps, self.delta, self.index, self.converged = [float(e) for e in eps], float(delta), 0, False

    def call(self, stats, update):
        eps = self.eps[self.index]
        w = weights_of(stats, eps)
        if update and w.min() > self.delta:
            if self.index + 1 < len(self.eps):
                self.index += 1
            else:
                self.converged = True
        return eps, w


# ---- a. the kernels against the statement ---------------------------------------------------------------------------------------------
T_LO, T_HI = -0.5, 2.25                     # a non-unit domain


def make_points(n, M, d, col, seed, one_bin=False):
    """ [n, d] points whose time column `col` covers the domain and a little beyond it; the first entries, as far as n allows: t_hi, below
    t_lo, above t_hi, every bin edge t_lo + k (t_hi - t_lo) / M, NaN and both infinities. Residuals of magnitude 1e-6 .. 1e3, both signs """
    rng = np.random.RandomState(seed)
    xs = rng.rand(n, d).astype(np.float32)
    t = (T_LO - 0.1 + (T_HI - T_LO + 0.2) * rng.rand(n)).astype(np.float32)
    if one_bin:
        t = (T_LO + (T_HI - T_LO) * (2.05 + 0.9 * rng.rand(n)) / M).astype(np.float32) if M > 3 else np.full(n, T_LO, dtype=np.float32)
    else:
        special = [T_HI, T_LO - 1.0, T_HI + 1.0] + [T_LO + k * (T_HI - T_LO) / M for k in range(M)] + [np.nan, np.inf, -np.inf, 3e38, -3e38]
        m = min(n, len(special))
        t[:m] = np.float32(special[:m])
    xs[:, col] = t
    r = (10.0 ** rng.uniform(-6, 3, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    return xs, r


class Call:
    """ the buffers of pinn_causal_weights calls on the tier's device, outputs pre-filled with sentinels """
    def __init__(self, tier, xs, col, r, M, eps=(1.0, ), delta=0.99, t_lo=T_LO, t_hi=T_HI):
        dev = tier.device
        self.tier, self.M, self.n, self.d, self.col, self.t_lo, self.t_hi = tier, M, xs.shape[0], xs.shape[1], col, t_lo, t_hi
        self.xs = torch.from_numpy(np.ascontiguousarray(xs)).to(dev)
        self.r = torch.from_numpy(np.ascontiguousarray(r)).to(dev)
        assert int(tier.lib.pinn_causal_state_bytes()) == STATE_DOUBLES * 8
        self.state = torch.full((STATE_DOUBLES, ), -3.0, dtype=torch.float64, device=dev)
        host = (ctypes.c_double * len(eps))(*[float(e) for e in eps])
        assert tier.lib.pinn_causal_init(self._p(self.state), STATE_DOUBLES * 8, host, len(eps), float(delta), None) == 0, self.error()
        self.ws = torch.full((int(tier.lib.pinn_causal_workspace_bytes(self.n, M)) // 8, ), -1.0, dtype=torch.float64, device=dev)
        assert self.ws.numel() >= 2 * M + 1
        self.w_out = torch.full((self.n + 8, ), float(SENTINEL), dtype=torch.float32, device=dev)
        self.bin_w = torch.full((MAX_BINS + 1, ), float(SENTINEL), dtype=torch.float32, device=dev)
        self.eps_out = torch.full((2, ), float(SENTINEL), dtype=torch.float32, device=dev)
        self.mse_out = torch.full((2, ), float(SENTINEL), dtype=torch.float32, device=dev)

    @staticmethod
    def _p(t, offset=0):
        return None if t is None else ctypes.c_void_p(t.data_ptr() + offset)

    def error(self):
        return self.tier.lib.pinn_last_error().decode()

    def run(self, update=1, **over):
        a = dict(t=self._p(self.xs, 4 * self.col), stride=self.d, r=self._p(self.r), n=self.n, M=self.M, t_lo=self.t_lo, t_hi=self.t_hi,
                 update=update, state=self._p(self.state), state_bytes=STATE_DOUBLES * 8, w_out=self._p(self.w_out), bin_w=self._p(self.bin_w),
                 eps_out=self._p(self.eps_out), mse_out=self._p(self.mse_out), ws=self._p(self.ws), ws_bytes=self.ws.numel() * 8)
        a.update(over)
        rc = self.tier.lib.pinn_causal_weights(a['t'], a['stride'], a['r'], a['n'], a['M'], a['t_lo'], a['t_hi'], a['update'], a['state'],
                                               a['state_bytes'], a['w_out'], a['bin_w'], a['eps_out'], a['mse_out'], a['ws'], a['ws_bytes'], None)
        if self.tier.device == 'cuda':
            torch.cuda.synchronize()
        return rc

    def host(self):
        return dict(state=self.state.cpu().numpy(), ws=self.ws.cpu().numpy(), w_out=self.w_out.cpu().numpy(), bin_w=self.bin_w.cpu().numpy(),
                    eps_out=self.eps_out.cpu().numpy(), mse_out=self.mse_out.cpu().numpy())


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def check_call(got, stats, w, eps, n, M, label, optional=True):
    """ exact: bins through n_k and the point weights' bins, w_0 == 1, eps = 0 all ones, underflow exactly 0, the flag. Bounded: L_k within
    n_k 2^-53 (relative; a product of two fp32 values is exact in fp64), w_k within eps P_k n 2^-52 + 2^-50 (the prefix's rounding, the
    exponential's), the float outputs within one fp32 ulp of fl32 of the statement's value """
    st = got['state']
    assert np.array_equal(st[NK:NK + M], stats['n_k'].astype(np.float64)), (label, st[NK:NK + M], stats['n_k'])
    assert np.all(st[NK + M:NK + MAX_BINS] == 0) and np.all(st[LK + M:LK + MAX_BINS] == 0) and np.all(st[WK + M:WK + MAX_BINS] == 0), label
    L = st[LK:LK + M]
    assert np.all(np.abs(L - stats['L']) <= stats['n_k'] * 2.0 ** -53 * stats['L']), (label, L, stats['L'])
    ws = st[WK:WK + M]
    assert ws[0] == 1.0 and np.all(np.isfinite(ws)) and np.all(np.diff(ws) <= 0), (label, ws)
    with np.errstate(all='ignore'):
        x = eps * stats['P'] if eps else np.zeros(M)
    if eps == 0:
        assert np.all(ws == 1.0), label
    assert np.all(ws[x > 800.0] == 0.0), (label, ws)                         # (exp(-745.2) is the smallest positive double)
    assert x.max() < 700.0 or x[x >= 700.0].min() > 800.0, label             # (no case sits in the subnormal range, where 2^-50 means nothing)
    assert np.all(np.abs(ws - w) <= (x * n * 2.0 ** -52 + 2.0 ** -50) * w), (label, ws, w)
    w32 = w.astype(np.float32)
    wo = got['w_out']
    assert np.all(np.abs(wo[:n].astype(np.float64) - w32[stats['k']]) <= ulp32(w32[stats['k']])), label
    assert np.array_equal(wo[:n].view(np.uint32), ws.astype(np.float32)[stats['k']].view(np.uint32)), label       # the state's, in the point's bin
    assert np.array_equal(wo[n:].view(np.uint32), np.full(8, SENTINEL).view(np.uint32)), label
    assert st[EPS_USED] == eps and st[BAD] == (1.0 if stats['non_finite'] else 0.0), (label, st[EPS_USED], st[BAD])
    assert abs(st[MEAN_SQ] - stats['mean_sq']) <= n * 2.0 ** -52 * stats['mean_sq'], label
    if optional:
        assert np.all(np.abs(got['bin_w'][:M].astype(np.float64) - w32) <= ulp32(w32)), label
        assert np.all(got['bin_w'][M:] == SENTINEL), label
        assert got['eps_out'][0] == np.float32(eps) and got['eps_out'][1] == SENTINEL, label
        assert abs(float(got['mse_out'][0]) - float(np.float32(stats['mean_sq']))) <= ulp32(stats['mean_sq']) and got['mse_out'][1] == SENTINEL, label
    else:
        assert np.all(got['bin_w'] == SENTINEL) and np.all(got['eps_out'] == SENTINEL) and np.all(got['mse_out'] == SENTINEL), label


EPS_CASES = (0.0, 1e-6, 1e30)                # all ones; weights in between (eps P_k < 64); every bin behind the first occupied one underflows


@pytest.mark.parametrize('M', [1, 2, 7, 32, 64])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 4099, FOLD + 1, 70001])
def test_kernels_match_the_fp64_statement(tier, n, M):
    """ one point, a wave +- 1, a workgroup +- 1, several workgroups, the first size at which the grid folds and one beyond -- times the
    number of bins, t as a vector of its own and as a column of [n][3] points, three tolerances: the full product on both tiers (a case
    per size and number of bins: six calls) """
    for d, col in ((1, 0), (3, 1)):
        xs, r = make_points(n, M, d, col, 1000 * M + n + d)
        stats = statistics(xs[:, col], r, M, T_LO, T_HI)
        if n >= 8 + M:
            assert stats['n_k'].min() >= 1 and stats['n_k'][0] >= 3 and stats['n_k'][M - 1] >= 3       # edges, outside, NaN: all placed
        for eps in EPS_CASES:
            label = f'{tier.name} n={n} M={M} d={d} eps={eps}'
            call = Call(tier, xs, col, r, M, eps=(eps, ))
            assert call.run() == 0, (label, call.error())
            got = call.host()
            check_call(got, stats, weights_of(stats, eps), eps, n, M, label)
            assert got['state'][CALLS] == 1.0 and got['state'][INDEX] == 0.0, label
            assert np.array_equal(call.xs.cpu().numpy().view(np.uint32), xs.view(np.uint32)), label


def test_bin_edges_land_where_the_statement_puts_them(tier):
    """ every edge t_lo + k (t_hi - t_lo) / M as the nearest float, its two neighbours, t_hi, outside, NaN: the weight a point receives is
    that of the statement's bin, for a ramp of bin losses that makes every bin's weight differ """
    M = 32
    edges = np.float32([T_LO + k * (T_HI - T_LO) / M for k in range(M + 1)])
    t = np.concatenate([edges, np.nextafter(edges, np.float32(-9)), np.nextafter(edges, np.float32(9)),
                        np.float32([T_LO - 3, T_HI + 3, np.nan, np.inf, -np.inf])])
    k = bins_of(t, T_LO, T_HI, M)
    assert k[M] == M - 1 and k[0] == 0 and k[-3] == 0 and k[-2] == M - 1 and k[-1] == 0 and set(k) == set(range(M))
    r = np.sqrt(0.01 * (1 + k)).astype(np.float32)
    stats = statistics(t, r, M, T_LO, T_HI)
    call = Call(tier, t.reshape(-1, 1), 0, r, M, eps=(1.0, ))
    assert call.run() == 0, call.error()
    got = call.host()
    check_call(got, stats, weights_of(stats, 1.0), 1.0, len(t), M, 'edges')
    assert len(set(got['state'][WK:WK + M])) == M


@pytest.mark.parametrize('M', [1, 7, 64])
def test_every_point_in_one_bin_leaves_the_others_empty(tier, M):
    n = 300
    xs, r = make_points(n, M, 3, 2, 77 + M, one_bin=True)
    stats = statistics(xs[:, 2], r, M, T_LO, T_HI)
    home = 2 if M > 3 else 0
    assert stats['n_k'][home] == n and stats['n_k'].sum() == n
    call = Call(tier, xs, 2, r, M, eps=(1e-5, ))
    assert call.run() == 0, call.error()
    got = call.host()
    check_call(got, stats, weights_of(stats, 1e-5), 1e-5, n, M, f'one bin M={M}')
    assert np.all(got['state'][LK:LK + M][np.arange(M) != home] == 0.0)
    assert np.all(got['state'][WK:WK + M][:home + 1] == 1.0) and (M <= 3 or len(set(got['state'][WK + home + 1:WK + M])) == 1)


@pytest.mark.parametrize('trouble', ['nan', 'inf', '-inf', 'all'])
def test_non_finite_residuals_add_nothing_and_raise_the_flag(tier, trouble):
    n, M = 700, 7
    xs, r = make_points(n, M, 2, 1, 5)
    if trouble == 'all':
        r[:] = np.float32(np.nan)
    else:
        r[[3, 300, 699]] = np.float32(float(trouble))
    stats = statistics(xs[:, 1], r, M, T_LO, T_HI)
    assert stats['non_finite'] and stats['n_k'].sum() == n
    call = Call(tier, xs, 1, r, M, eps=(1e-6, ))
    assert call.run() == 0, call.error()
    check_call(call.host(), stats, weights_of(stats, 1e-6), 1e-6, n, M, trouble)
    clean = np.where(np.isfinite(r), r, np.float32(0))
    again = Call(tier, xs, 1, clean, M, eps=(1e-6, ))
    assert again.run() == 0
    assert np.array_equal(again.host()['w_out'].view(np.uint32), call.host()['w_out'].view(np.uint32)) and again.host()['state'][BAD] == 0.0
    # the flag stays up over a later clean call on the same state
    call.r.copy_(torch.from_numpy(clean))
    assert call.run() == 0 and call.host()['state'][BAD] == 1.0 and call.host()['state'][CALLS] == 2.0


def test_optional_outputs_passed_as_null_are_not_written(tier):
    n, M = 257, 7
    xs, r = make_points(n, M, 3, 1, 9)
    stats = statistics(xs[:, 1], r, M, T_LO, T_HI)
    call = Call(tier, xs, 1, r, M, eps=(1e-6, ))
    assert call.run(bin_w=None, eps_out=None, mse_out=None) == 0, call.error()
    check_call(call.host(), stats, weights_of(stats, 1e-6), 1e-6, n, M, 'null outputs', optional=False)
    # n == 0: success, nothing launched, the state as it was
    before = call.host()
    assert call.run(n=0) == 0, call.error()
    after = call.host()
    for key in before:
        assert np.array_equal(before[key].view(np.uint8), after[key].view(np.uint8)), key


# ---- b. repeatability -----------------------------------------------------------------------------------------------------------------
def test_two_calls_on_equal_inputs_are_equal_bit_for_bit(tier, monkeypatch):
    monkeypatch.delenv('PINN_EMU_SHUFFLE', raising=False)
    n, M = 4099, 32
    xs, r = make_points(n, M, 3, 1, 31)

    def run():
        call = Call(tier, xs, 1, r, M, eps=(1e-7, 1e-6), delta=0.0)
        for _ in range(2):
            assert call.run() == 0
        return call.host()
    a, b = run(), run()
    assert a['state'][INDEX] == 1.0 and a['state'][CALLS] == 2.0
    for key in ('state', 'ws'):
        assert np.array_equal(a[key].view(np.uint64), b[key].view(np.uint64)), key
    for key in ('w_out', 'bin_w', 'eps_out', 'mse_out'):
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key
    if tier.name == 'emu':                      # the waves of a workgroup in shuffled order: same sums, same weights
        for seed in ('3', '11'):
            monkeypatch.setenv('PINN_EMU_SHUFFLE', seed)
            c = run()
            monkeypatch.delenv('PINN_EMU_SHUFFLE')
            for key in ('state', 'ws'):
                assert np.array_equal(a[key].view(np.uint64), c[key].view(np.uint64)), (seed, key)
            for key in ('w_out', 'bin_w', 'eps_out', 'mse_out'):
                assert np.array_equal(a[key].view(np.uint32), c[key].view(np.uint32)), (seed, key)


# ---- c. the ladder ----------------------------------------------------------------------------------------------------------------------
def _flat_batch(n, M, c, seed=1):
    """ residual c everywhere on evenly spread times: L_k = c^2, min_k w_k = exp(-eps (M - 1) c^2) """
    t = ((np.arange(n) + 0.5) / n).astype(np.float32).reshape(-1, 1)
    return t, np.full(n, c, dtype=np.float32)


def _drive(tier, eps, delta, script, M=8, n=96):
    """ script: (c, update) per call -> per call (the tolerance used, the index behind it, converged), from the device and from `Ladder` """
    t, r = _flat_batch(n, M, 1.0)
    call = Call(tier, t, 0, r, M, eps=eps, delta=delta, t_lo=0.0, t_hi=1.0)
    want, dev, stm = Ladder(eps, delta), [], []
    for c, update in script:
        call.r.fill_(float(c))
        assert call.run(update=update) == 0, call.error()
        got = call.host()
        dev.append((float(got['eps_out'][0]), got['state'][INDEX], got['state'][CONVERGED]))
        used, _ = want.call(statistics(t[:, 0], np.full(n, c, dtype=np.float32), M, 0.0, 1.0), update)
        stm.append((float(np.float32(used)), float(want.index), 1.0 if want.converged else 0.0))
        assert got['state'][EPS_USED] == used
    return dev, stm, call


def test_the_ladder_advances_where_the_statement_does(tier):
    # M = 8: min w = exp(-7 eps c^2) > 0.9 <=> eps c^2 < 0.01505
    eps = (1e-2, 1e-1, 1.0, 10.0)
    script = [(2.0, 1),         # 1e-2 * 4 = 0.04: stays
              (1.0, 0),         # 0.01 would advance: update = 0 holds it
              (1.0, 1),         # advances to 1e-1 for the next call
              (1.0, 1),         # 0.1: stays
              (0.3, 1),         # 0.009: advances to 1.0
              (0.1, 1),         # 0.01: advances to 10
              (0.1, 1),         # 0.1: stays at the last rung, not converged
              (0.01, 0),        # would converge: update = 0
              (0.01, 1),        # converged
              (5.0, 1)]         # stays converged at the last rung
    dev, stm, call = _drive(tier, eps, 0.9, script)
    assert dev == stm, (dev, stm)
    assert [d[0] for d in dev] == [float(np.float32(e)) for e in (1e-2, 1e-2, 1e-2, 1e-1, 1e-1, 1.0, 10.0, 10.0, 10.0, 10.0)]
    assert [d[1] for d in dev] == [0, 0, 1, 1, 2, 3, 3, 3, 3, 3] and [d[2] for d in dev] == [0] * 8 + [1, 1]
    st = call.host()['state']
    assert st[CALLS] == len(script) and list(st[EPS:EPS + 4]) == list(eps) and st[N_EPS] == 4 and st[DELTA] == 0.9


@pytest.mark.parametrize('delta', [1.0, 1.5, float('inf')])
def test_delta_of_one_or_more_never_advances(tier, delta):
    dev, stm, _ = _drive(tier, (0.5, 1.0), delta, [(0.0, 1), (0.0, 1), (1e-3, 1)])       # (r = 0: every weight is exactly 1, and 1 > 1 is false)
    assert dev == stm and [d[1:] for d in dev] == [(0.0, 0.0)] * 3


def test_a_ladder_of_one_converges_in_place(tier):
    dev, stm, _ = _drive(tier, (1.0, ), 0.5, [(1.0, 1), (0.1, 0), (0.1, 1), (1.0, 1)])
    assert dev == stm and [d[1] for d in dev] == [0.0] * 4 and [d[2] for d in dev] == [0.0, 0.0, 1.0, 1.0]
    dev, stm, _ = _drive(tier, (0.0, ), -1.0, [(3.0, 1)])                                  # (a negative delta: the first call converges)
    assert dev == stm == [(0.0, 0.0, 1.0)]


# ---- d. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(tier):
    """ every refusal: non-zero, a text, and outputs, state and workspace as they were (sentinels) """
    n, M = 300, 7
    xs, r = make_points(n, M, 3, 1, 2)
    call = Call(tier, xs, 1, r, M)
    before = call.host()
    small = torch.zeros(4, dtype=torch.float64, device=tier.device)
    nan, inf = float('nan'), float('inf')
    p = call._p
    cases = [(dict(M=0), 'bins=0'), (dict(M=65), 'bins=65'), (dict(M=-1), 'bins=-1'), (dict(n=-1), 'n=-1'), (dict(t=None), 'null'), (dict(r=None), 'null'),
             (dict(state=None), 'null'), (dict(w_out=None), 'null'), (dict(ws=None), 'null'),
             (dict(state_bytes=STATE_DOUBLES * 8 - 8), 'state block too small'), (dict(ws_bytes=call.ws.numel() * 8 - 8), 'workspace too small'),
             (dict(state=p(small), state_bytes=32), 'state block too small'),
             (dict(state=p(call.state, 8)), '16-byte'), (dict(ws=p(call.ws, 8)), '16-byte'), (dict(stride=0), 't_stride=0'), (dict(stride=-3), 't_stride=-3'), (dict(stride=(1 << 20) + 1), 'outside [1, 1048576]'),
             (dict(t_lo=nan), 'time domain'), (dict(t_hi=nan), 'time domain'), (dict(t_lo=-inf), 'time domain'), (dict(t_hi=inf), 'time domain'),
             (dict(t_lo=1.0, t_hi=1.0), 'time domain'), (dict(t_lo=2.0, t_hi=1.0), 'time domain'),
             (dict(w_out=p(call.r)), 'w_out overlaps r'), (dict(w_out=p(call.r, 4 * (n - 1))), 'w_out overlaps r'),
             (dict(w_out=p(call.xs, 4)), 'w_out overlaps t'), (dict(w_out=p(call.xs, 4 * (3 * n - 2))), 'w_out overlaps t'),
             (dict(bin_w=p(call.r, 16)), 'bin_weight_out overlaps r'), (dict(eps_out=p(call.xs, 40)), 'eps_out overlaps t'),
             (dict(mse_out=p(call.r, 4 * (n - 1))), 'mean_sq_out overlaps r'), (dict(w_out=p(call.state)), 'w_out overlaps the state'),
             (dict(bin_w=p(call.ws)), 'bin_weight_out overlaps the workspace'), (dict(eps_out=p(call.w_out, 8)), 'w_out overlaps eps_out'),
             (dict(mse_out=p(call.bin_w, 4)), 'bin_weight_out overlaps mean_sq_out')]
    one = (ctypes.c_double * 1)(1.0)
    for over, reason in cases:
        # (another refusal's text first: the case has to leave its own reason, not find one lying there)
        assert tier.lib.pinn_causal_init(p(call.state), STATE_DOUBLES * 8, one, 0, 0.5, None) != 0 and 'ladder of 0' in call.error()
        assert call.run(**over) != 0, over
        assert reason in call.error() and 'ladder' not in call.error(), (over, call.error())
        after = call.host()
        for key in before:
            assert np.array_equal(before[key].view(np.uint8), after[key].view(np.uint8)), (over, key)
        assert np.array_equal(call.r.cpu().numpy().view(np.uint32), r.view(np.uint32)), over
        assert np.array_equal(call.xs.cpu().numpy().view(np.uint32), xs.view(np.uint32)), over
    # the queries and init
    lib = tier.lib
    assert lib.pinn_causal_workspace_bytes(10, 0) == 0 and lib.pinn_causal_workspace_bytes(10, 65) == 0 and lib.pinn_causal_workspace_bytes(-1, 8) == 0
    assert lib.pinn_causal_workspace_bytes(FOLD, 8) == 256 * 18 * 8 and lib.pinn_causal_workspace_bytes(FOLD + 1, 8) == 129 * 18 * 8       # (the fold)
    assert lib.pinn_causal_workspace_bytes(1, 64) % 16 == 0 and lib.pinn_causal_workspace_bytes(1, 64) >= 129 * 8
    state = torch.full((STATE_DOUBLES, ), 5.0, dtype=torch.float64, device=tier.device)
    arr = lambda *v: (ctypes.c_double * len(v))(*v)
    full = STATE_DOUBLES * 8
    for args, reason in (((None, full, arr(1.0), 1, 0.5), 'null'), ((p(state), full, None, 1, 0.5), 'null'), ((p(state), full, arr(1.0), 0, 0.5), 'ladder of 0'),
                         ((p(state), full, arr(*[1.0] * 9), 9, 0.5), 'ladder of 9'), ((p(state), full - 8, arr(1.0), 1, 0.5), 'too small'),
                         ((p(state, 8), full, arr(1.0), 1, 0.5), '16-byte'), ((p(state), full, arr(1.0, -1.0), 2, 0.5), 'tolerance 1'),
                         ((p(state), full, arr(nan), 1, 0.5), 'tolerance 0'), ((p(state), full, arr(1.0, inf), 2, 0.5), 'tolerance 1'),
                         ((p(state), full, arr(1.0), 1, nan), 'delta')):
        assert call.run(M=0) != 0 and 'bins=0' in call.error()
        assert lib.pinn_causal_init(*args, None) != 0, args[1:]
        assert reason in call.error() and 'bins=0' not in call.error(), (args[1:], call.error())
        assert bool((state == 5.0).all())
    assert lib.pinn_causal_init(p(state), full, arr(0.0, 4.0), 2, 0.25, None) == 0
    assert state.cpu().tolist() == [0.0, 4.0] + [0.0] * 6 + [2.0, 0.0, 0.25] + [0.0] * (STATE_DOUBLES - 11)


# ---- e. Solver.fit(causal=...) ---------------------------------------------------------------------------------------------------------
RTOL = 1e-5                 # the project's bar for losses and gradients (README)
LR = 0.01
NETS = {'plain': dict(layout='fa fa f', features=[16, 16, 1], activation='Tanh'),
        'skip': dict(layout='faR fa fa+ f', features=[16, 16, 16, 1], activation='Tanh')}
CASES = [('plain', 96, 3), ('skip', 257, 4)]        # (net, batch, seed)


def heat(D):
    return lambda f, x, t: D(f, t) - 0.1 * D(D(f, x), x) - torch.sin(np.pi * x)


def heat_kwargs(net):
    return dict(ndims=2, initial_condition=lambda x: torch.sin(np.pi * x), **NETS[net])


def oracle_solver(net, dtype, start=None, seed=15):
    # (seed 15: for both nets the fp32 restatement's gradient sits within 1e-6 of the fp64 one; seed 11 starts the plain net where the
    #  equation's gradient nearly cancels and fp32 alone is 2.6e-5 off -- test_the_fp32_reference_alone_holds_the_bar)
    torch.manual_seed(seed)
    oracle = po.OracleSolver(heat(po.D), dtype=dtype, **heat_kwargs(net))
    if start is not None:
        oracle.import_params(start)
    return oracle


def product_solver(pa, tier, net, start, **kwargs):
    solver = pa.Solver(heat(pa.D), **heat_kwargs(net), **kwargs, **tier.solver_kwargs)
    if start is not None:
        load_params(solver, start)
    solver.use_fused = False
    return solver


def batches(steps, n, seed):
    return np.random.RandomState(seed).rand(steps, n, 2).astype(np.float32)


def causal_oracle_fit(oracle, pts, bins, eps, delta=0.99, lr=LR):
    """ the restatement: oracle/pinn_oracle.py's step with the equation term replaced by mean_i w_i r_i^2, the weights from this file's
    statement on the detached residuals (constants of the step) -> per iteration (loss, gradients as export_grads gives them, w_k) """
    params = [p for p in oracle.model.parameters() if p.requires_grad]
    oracle.optimizer = torch.optim.Adam(params, lr=lr)
    ladder, rows = Ladder(eps, delta), []
    for arr in pts:
        oracle.optimizer.zero_grad()
        xs = [torch.tensor(arr[:, i:i + 1], dtype=oracle.dtype).requires_grad_() for i in range(arr.shape[1])]
        r = oracle.ctx.run(oracle.equation, oracle.ctx.run(oracle.model, oracle.reshape_and_concat(xs)), *xs)
        stats = statistics(arr[:, 1], r.detach().numpy(), bins, 0.0, 1.0)
        _, w = ladder.call(stats, True)
        w_pt = w[stats['k']] if oracle.dtype == torch.float64 else w.astype(np.float32)[stats['k']]
        loss = (torch.tensor(w_pt, dtype=oracle.dtype).view_as(r) * r * r).mean()
        loss.backward()
        rows.append((float(loss.detach()), oracle.export_grads(), w, stats['mean_sq']))
        oracle.optimizer.step()
        oracle.losses.append(loss.detach().numpy())
    return rows


def judged(case, quantity, got, want32, want64_fn, atol=0.0):
    # (no adam_move: no comparison of this file may take the arbiter's outlier-set-aside branch)
    ok, err, arb = close_or_arbitrated(got, want32, want64_fn, RTOL, atol=atol)
    record_margin('causal_weights', case, quantity, err, RTOL, arb)
    print(f'causal_weights {case} {quantity}: {err:.3e} (bar {RTOL:.0e}) arbitrated={arb}')
    assert ok, (case, quantity, err, np.asarray(got).ravel()[:8], np.asarray(want32).ravel()[:8])


@pytest.fixture(scope='module')
def reference():
    """ per case: the start parameters, the batches, and the fp32 / fp64 restatements of ten iterations -- computed once, shared, unchanged """
    out = {}
    for net, n, seed in CASES:
        o32 = oracle_solver(net, torch.float32)
        start = o32.export_params()
        pts = batches(10, n, seed)
        rows32 = causal_oracle_fit(o32, pts[:1], 8, (1.0, ))
        rows64 = causal_oracle_fit(oracle_solver(net, torch.float64, start), pts[:1].astype(np.float64), 8, (1.0, ))
        out[net] = dict(start=start, pts=pts, rows32=rows32, rows64=rows64)
    return out


@pytest.mark.parametrize('net,n,seed', CASES)
def test_the_fp32_reference_alone_holds_the_bar(reference, net, n, seed):
    """ the comparisons below never need the arbiter's outlier branch (no adam_move is passed to them), and for these seeds not the arbiter
    either: the fp32 restatement stays within the bar of the fp64 one """
    (loss32, grads32, w32, _), (loss64, grads64, w64, _) = reference[net]['rows32'][0], reference[net]['rows64'][0]
    assert abs(loss32 - loss64) <= RTOL * abs(loss64)
    for a, b in zip(grads32, grads64):
        assert np.linalg.norm(a.astype(np.float64) - b) <= RTOL * np.linalg.norm(b) + 1e-9 * np.sqrt(b.size)
    assert np.all(np.abs(w32 - w64) <= RTOL * w64) and 0.0 < w64[-1] < 0.999           # (the weights do something in this problem)


@pytest.mark.parametrize('net,n,seed', CASES)
def test_one_iteration_follows_the_restatement(pa, tier, reference, net, n, seed):
    ref = reference[net]
    solver = product_solver(pa, tier, net, ref['start'])
    causal = pa.CausalWeights(bins=8, eps=1.0)
    solver.fit(1, n, sampler=FixedBatches(ref['pts'][:1]), lr=LR, causal=causal)
    assert solver.last_fit_path == 'generic' and solver.last_fit_causal == 'bins8/generic'
    (loss32, grads32, w32, mse32), (loss64, grads64, w64, _) = ref['rows32'][0], ref['rows64'][0]
    case = f'{tier.name} {net}/{n}'
    judged(case, 'loss', [float(solver.losses[0])], [loss32], lambda: [loss64])
    for i, (a, b) in enumerate(zip(export_grads(solver), grads32)):
        judged(case, f'gradient[{i}]', a, b, lambda i=i: grads64[i])
    judged(case, 'weights', solver.causal_weight_history[0], w32, lambda: w64)
    judged(case, 'mean r^2', solver.residual_mse_history, [mse32], lambda: [ref['rows64'][0][3]])
    assert solver.causal_eps_history.tolist() == [1.0] and causal.eps == 1.0 and not causal.non_finite
    assert np.array_equal(solver.causal_weight_history[0], causal.read('bin_weight').astype(np.float32))


@pytest.mark.parametrize('net,n,seed', CASES)
def test_ten_iterations_fill_the_histories(pa, tier, reference, net, n, seed):
    ref = reference[net]
    solver = product_solver(pa, tier, net, ref['start'])
    causal = pa.CausalWeights(bins=8, eps=1.0)
    mse = []
    for it in range(10):                        # one iteration per call: the residual of the batch under the parameters it is stepped from
        r = solver.residual(ref['pts'][it][:, 0], ref['pts'][it][:, 1]).astype(np.float64)
        mse.append(float((r * r).mean()))
        solver.fit(1, n, sampler=FixedBatches(ref['pts'][it:it + 1]), lr=LR, optimizer='Adam' if it == 0 else None, causal=causal)
    wh = solver.causal_weight_history
    assert wh.shape == (10, 8) and wh.dtype == np.float32 and np.all(wh[:, 0] == 1.0) and np.all(np.diff(wh, axis=1) <= 0) and np.all(wh > 0)
    assert solver.causal_eps_history.shape == (10, ) and np.all(solver.causal_eps_history == 1.0)
    got = solver.residual_mse_history
    assert got.shape == (10, ) and np.all(np.abs(got - mse) <= 4e-6 * np.asarray(mse)), (got, mse)
    assert len(solver.losses) == 10 and np.all(np.float32(solver.losses) <= got * (1 + 1e-6))          # (weights <= 1: the weighted loss is the smaller one)
    assert causal.read('calls') == 10.0 and causal.calls == 10
    if net != 'plain':
        return
    # the same ten iterations in one call: the same trajectory, bit for bit
    whole = product_solver(pa, tier, net, ref['start'])
    whole.fit(10, n, sampler=FixedBatches(ref['pts']), lr=LR, causal=pa.CausalWeights(bins=8, eps=1.0))
    assert np.array_equal(np.float32(whole.losses), np.float32(solver.losses)) and torch.equal(whole.model.flat, solver.model.flat)
    assert np.array_equal(whole.causal_weight_history, wh)


def test_the_ladder_carries_on_and_a_fresh_object_restarts(pa, tier, reference):
    ref = reference['plain']
    solver = product_solver(pa, tier, 'plain', ref['start'])
    causal = pa.CausalWeights(bins=8, eps=(0.0, 1.0, 2.0), delta=0.5)          # (eps = 0: every weight 1 > 0.5, the first call advances)
    solver.fit(2, 96, sampler=FixedBatches(ref['pts'][:2]), lr=LR, causal=causal)
    assert solver.causal_eps_history.tolist() == [0.0, 1.0] and causal.eps in (1.0, 2.0)
    rung = causal.eps
    solver.fit(1, 96, sampler=FixedBatches(ref['pts'][2:3]), lr=LR, optimizer=None, causal=causal)
    assert solver.causal_eps_history.tolist() == [0.0, 1.0, rung] and causal.read('calls') == 3.0
    fresh = pa.CausalWeights(bins=8, eps=(0.0, 1.0, 2.0), delta=0.5, period=2)
    solver.fit(3, 96, sampler=FixedBatches(ref['pts'][3:6]), lr=LR, optimizer=None, causal=fresh)
    assert solver.causal_eps_history.tolist()[3:] == [0.0, 1.0, 1.0]           # (period 2: the decision of the second iteration is not taken)
    assert solver.causal_weight_history.shape == (6, 8) and np.all(solver.causal_weight_history[3] == 1.0)
    assert not fresh.converged and not fresh.non_finite


def test_eps_zero_is_the_generic_fit_without_causal(pa, tier, reference):
    ref = reference['plain']
    plain = product_solver(pa, tier, 'plain', ref['start'])
    plain.fit(3, 96, sampler=FixedBatches(ref['pts'][:3]), lr=LR)
    weighted = product_solver(pa, tier, 'plain', ref['start'])
    weighted.fit(3, 96, sampler=FixedBatches(ref['pts'][:3]), lr=LR, causal=pa.CausalWeights(bins=8, eps=0.0))
    assert plain.last_fit_path == weighted.last_fit_path == 'generic' and plain.last_fit_causal is None
    arbiter = {}

    def o64():
        if 'o' not in arbiter:
            o = arbiter['o'] = oracle_solver('plain', torch.float64, ref['start'])
            o.fit(niters=3, batch_size=96, points=ref['pts'][:3].astype(np.float64), lr=LR)
        return arbiter['o']
    case = f'{tier.name} eps=0'
    judged(case, 'losses', [float(v) for v in weighted.losses], [float(v) for v in plain.losses], lambda: [float(v) for v in o64().losses])
    for i, (a, b) in enumerate(zip(export_params(weighted), export_params(plain))):
        judged(case, f'parameters[{i}]', a, b, lambda i=i: o64().export_params()[i], atol=2e-6)
    assert np.all(weighted.causal_weight_history == 1.0)
    assert np.all(np.abs(weighted.residual_mse_history - np.float32(weighted.losses)) <= 2e-6 * np.float32(weighted.losses))


class _Counting:
    """ the bound library with every pinn_causal_* entry point counted """
    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('pinn_causal_'):
            return fn

        def counted(*args):
            self.calls += 1
            return fn(*args)
        return counted


def test_causal_none_is_the_code_as_it_was(pa, tier, reference):
    ref = reference['plain']
    solver = pa.Solver(heat(pa.D), **heat_kwargs('plain'), **tier.solver_kwargs)
    load_params(solver, ref['start'])
    counting = _Counting(solver.model.net.lib)
    solver.model.net.lib = counting
    solver.fit(2, 96, sampler=FixedBatches(ref['pts'][:2]), lr=LR, causal=None)
    assert counting.calls == 0 and solver.last_fit_causal is None and solver._causal is None and solver._causal_pending == []
    assert solver.causal_weight_history.shape == (0, 0) and solver.residual_mse_history.shape == (0, )
    solver.fit(1, 96, sampler=FixedBatches(ref['pts'][2:3]), lr=LR, optimizer=None, causal=pa.CausalWeights(bins=4, eps=1.0))
    assert counting.calls > 0 and solver.last_fit_causal == 'bins4/generic' and solver.causal_weight_history.shape == (1, 4)
    solver.fit(1, 96, sampler=FixedBatches(ref['pts'][3:4]), lr=LR, optimizer=None)
    assert solver.last_fit_causal is None and solver.causal_weight_history.shape == (1, 4)


def test_fit_refuses_with_the_reason(pa, tier):
    con = lambda f, x, t: f(torch.tensor([0.5]), torch.tensor([0.5]))
    solver = pa.Solver(heat(pa.D), constraints=con, **heat_kwargs('plain'), **tier.solver_kwargs)
    before = solver.model.flat.clone()
    pts = batches(1, 40, 1)
    fit = lambda **kw: solver.fit(1, 40, sampler=FixedBatches(pts), lr=LR, **kw)
    cw = pa.CausalWeights
    for kw, exc, text in (
            (dict(causal=cw(), criterion=nn.L1Loss()), NotImplementedError, 'nn.MSELoss'),
            (dict(causal=cw(), criterion=nn.MSELoss(reduction='sum')), NotImplementedError, 'mean'),
            (dict(causal=cw(), optimizer='LBFGS'), NotImplementedError, 'closure'),
            (dict(causal=cw(), loss_terms=['constraint_0']), ValueError, "'equation' is not among"),
            (dict(causal=cw(), loss_terms=['equation', 'constraint_0'], loss_weights=[1.0, 2.0]), NotImplementedError, 'loss_weights'),
            (dict(causal=cw(time=2)), ValueError, 'time=2'),
            (dict(causal='causal'), ValueError, 'CausalWeights')):
        with pytest.raises(exc, match=text):
            fit(**kw)
    solver._world = lambda: (0, 2)
    with pytest.raises(NotImplementedError, match='torch.distributed'):
        fit(causal=cw())
    del solver._world
    assert torch.equal(solver.model.flat, before) and solver.optimizer is None and len(solver.losses) == 0
    assert solver.causal_weight_history.shape == (0, 0) and solver.last_fit_causal is None and solver.lrs == []
    # no time column beside the only one, unless it is named
    ode = pa.Solver(lambda f, t: pa.D(f, t) + f, ndims=1, initial_condition=1.0, layout='fa f', features=[8, 1], activation='Tanh',
                    **tier.solver_kwargs)
    with pytest.raises(ValueError, match='ndims=1'):
        ode.fit(1, 40, sampler=FixedBatches(batches(1, 40, 2)[:, :, :1]), lr=LR, causal=cw())
    assert ode.optimizer is None
    ode.fit(1, 40, sampler=FixedBatches(batches(1, 40, 2)[:, :, :1]), lr=LR, causal=cw(bins=4, eps=1.0, time=0))
    assert ode.causal_weight_history.shape == (1, 4) and ode.causal_weight_history[0, 0] == 1.0

    # a forward() of the model's own that hands the network another time than the batch's
    class Warped(pa.ConvBlockModel):
        def forward(self, xs):
            return self.anzatc(self.conv_block(xs * torch.tensor([1.0, 0.5], device=xs.device)), xs)

    class Kept(pa.ConvBlockModel):
        def forward(self, xs):
            return self.anzatc(self.conv_block(xs * torch.tensor([2.0, 1.0], device=xs.device)), xs)
    warped = pa.Solver(heat(pa.D), model=Warped, **heat_kwargs('plain'), **tier.solver_kwargs)
    with pytest.raises(NotImplementedError, match='time column'):
        warped.fit(1, 40, sampler=FixedBatches(pts), lr=LR, causal=cw())
    assert warped.optimizer is None
    kept = pa.Solver(heat(pa.D), model=Kept, **heat_kwargs('plain'), **tier.solver_kwargs)
    kept.fit(1, 40, sampler=FixedBatches(pts), lr=LR, causal=cw(bins=4, eps=1.0))
    assert kept.last_fit_causal == 'bins4/generic'
    # the constructor's own checks, and the alias
    for bad in (dict(bins=0), dict(bins=65), dict(eps=()), dict(eps=[1.0] * 9), dict(eps=-1.0), dict(eps=float('nan')), dict(delta=float('nan')),
                dict(period=0), dict(time=-1)):
        with pytest.raises(ValueError):
            cw(**bad)
    import pydens
    assert pydens.CausalWeights is pa.CausalWeights
