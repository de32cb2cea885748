""" The execution primitives of pydens_amd/csrc/pinn_port.h have two independent statements: HIP builtins / inline assembly in the
product build, host code in the emulator the CPU tier runs the kernels on (tests/emu/emu_runtime.*). This file holds BOTH to a
third one: plain numpy written from the comments of pinn_port.h (the contract). Every case exists twice with the same body and the
same inputs -- on the emulator library, and as a `-m gpu` twin on the product library -- through pinn_port_probe (one primitive
per call, compiled from pinn_port_probe.h into both builds). Comparison is bitwise. Both tiers equal to one independent statement
means emulator == device.

Where the contract is not bit-exact, a claim the project makes elsewhere is asserted instead:
  * pinn_exp2 / pinn_rcp: "~1 ulp" (pinn_port.h; the tanh error analysis of DESIGN.md section 3 stands on it): maximum error in ulps
    of the fp32 result against fp64;
  * the rounding inside the two MFMAs: "at or below the error of an fp32 fmaf chain" (emu_runtime.h), as
    |result - f64| <= 2 max|chain - f64| -- the factor is the suite's arbitration rule (helpers.close_or_arbitrated).
The measured figures of a run are printed before each assertion (profiles/r09_port_contract.txt keeps the recorded ones). """
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import make_solver

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu'))

# `which` of pinn_port_probe (include/pinn.h)
(MFMA16, MFMA16_BF16, LDS_TR16, PACK_HI16, ROW_SUM16, ROW_SUM16_N3, ROW_SUM16_F64, ROWS_SUM, SHFL_XOR, ROWS_TOTAL_F64, WAVE_UNIFORM, ROWS,
 WAVE_SYNC, FLAGS, EXP2, RCP) = range(16)
T = 256                         # threads per block: four waves
LDS_WORDS = 4096                # LDS image of the transpose-read probe
F32, F64, U32, I32 = np.float32, np.float64, np.uint32, np.int32


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


def _gpu(pa):
    return pa.engine.load_library(), 'cuda'


def probe(pa, lib, device, which, data, out_words, n_blocks, out_dtype=U32):
    """ one pinn_port_probe call: `data` (any 4- or 8-byte dtype) in, out_words 4-byte words per block out, viewed as out_dtype """
    raw = np.ascontiguousarray(data).view(U32).ravel()
    src = torch.from_numpy(raw.view(I32).copy()).to(device)
    dst = torch.full((n_blocks * out_words,), -0x21524111, dtype=torch.int32, device=device)        # (a pattern no case expects)
    rc = lib.pinn_port_probe(which, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), n_blocks, pa.engine.stream_of(dst))
    assert rc == 0, lib.pinn_last_error().decode()
    if device != 'cpu':
        torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy().view(U32), raw)               # the input is read, never written
    return dst.cpu().numpy().view(out_dtype)


def same_bits(got, want):
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert a.dtype.itemsize == b.dtype.itemsize and a.size == b.size
    view = U32 if a.dtype.itemsize == 4 else np.uint64
    return np.array_equal(a.view(view).ravel(), b.view(view).ravel())


_CACHE = {}


def shared(key, make):
    """ inputs and expected values of a case: made once, shared by the two tiers, never written to """
    if key not in _CACHE:
        vals = make()
        for v in vals:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = vals
    return _CACHE[key]


LANE = np.arange(64)


# ---- pinn_mfma16: D[16x16] += A[16x4] B[4x16]; lane l supplies A[l&15][l>>4] and B[l>>4][l&15]; c[r] is D[(l>>4)*4 + r][l&15] ---------
def _mfma16_pack(A0, B0, A1, B1, C):
    """ [waves][...] matrices -> the probe's per-lane words a0 b0 a1 b1 c[4] """
    w = A0.shape[0]
    lanes = np.zeros((w, 64, 8), dtype=F32)
    i, k = LANE & 15, LANE >> 4
    lanes[:, :, 0], lanes[:, :, 1] = A0[:, i, k], B0[:, k, i]
    lanes[:, :, 2], lanes[:, :, 3] = A1[:, i, k], B1[:, k, i]
    for r in range(4):
        lanes[:, :, 4 + r] = C[:, k * 4 + r, i]
    return lanes


def _mfma_unpack(out, waves):
    """ the probe's per-lane c[4] -> [waves][16][16] """
    c = out.reshape(waves, 64, 4)
    D = np.zeros((waves, 16, 16), dtype=c.dtype)
    for r in range(4):
        D[:, (LANE >> 4) * 4 + r, LANE & 15] = c[:, :, r]
    return D


def _mfma16_lane_map_inputs():
    rng = np.random.default_rng(16)
    waves = 8
    A0, A1 = (np.stack([rng.permutation(np.arange(1, 65)).reshape(16, 4) * rng.choice([-1, 1], (16, 4)) for _ in range(waves)]) for _ in range(2))
    B0, B1 = (np.stack([rng.permutation(np.arange(65, 129)).reshape(4, 16) * rng.choice([-1, 1], (4, 16)) for _ in range(waves)]) for _ in range(2))
    C = np.stack([rng.permutation(np.arange(1000, 1256)).reshape(16, 16) for _ in range(waves)])
    D = C + A0 @ B0 + A1 @ B1                                  # integers: 8 products below 2^13 each, every partial sum exact in fp32
    assert np.abs(A0 @ B0).max() + np.abs(A1 @ B1).max() + 1256 < 2 ** 24
    return _mfma16_pack(*(m.astype(F32) for m in (A0, B0, A1, B1, C))), D.astype(F32)


def _mfma16_lane_map_case(pa, lib, device):
    lanes, want = shared('mfma16', _mfma16_lane_map_inputs)
    got = _mfma_unpack(probe(pa, lib, device, MFMA16, lanes, T * 4, 2, F32), 8)
    assert same_bits(got, want), np.argwhere(got != want)[:8]


def test_mfma16_lane_map(pa, emu_lib):
    _mfma16_lane_map_case(pa, emu_lib, 'cpu')


@pytest.mark.gpu
def test_mfma16_lane_map_on_the_gpu(pa):
    _mfma16_lane_map_case(pa, *_gpu(pa))


# ---- pinn_mfma16_bf16: D[16x16] += A[16x32] B[32x16]; lane l supplies A[l&15][8*(l>>4) + e] and B[8*(l>>4) + e][l&15], e = 0..7, element e in
# bits 16*(e&1) of register e>>1 --------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """ bf16 bit patterns of values that ARE bf16 (the upper half of their fp32 pattern) """
    b = np.ascontiguousarray(x, dtype=F32).view(U32)
    assert not (b & 0xffff).any()
    return b >> 16


def _bf16_pack(A, B, C):
    """ [waves][16][32], [waves][32][16], [waves][16][16] -> per-lane words: four registers of a, four of b, c[4] """
    w = A.shape[0]
    words = np.zeros((w, 64, 12), dtype=U32)
    i, q = LANE & 15, LANE >> 4
    ab, bb = bf16_bits(A).reshape(A.shape), bf16_bits(B).reshape(B.shape)
    for e in range(8):
        words[:, :, e >> 1] |= ab[:, i, 8 * q + e] << U32(16 * (e & 1))
        words[:, :, 4 + (e >> 1)] |= bb[:, 8 * q + e, i] << U32(16 * (e & 1))
    for r in range(4):
        words[:, :, 8 + r] = np.ascontiguousarray(C[:, q * 4 + r, i], dtype=F32).view(U32)
    return words


def _mfma16_bf16_lane_map_inputs():
    rng = np.random.default_rng(32)
    waves = 8
    vals = np.concatenate([np.arange(1, 257), -np.arange(1, 257)])        # 512 distinct integers, all exact in bf16 (8 significant bits)
    A = np.stack([rng.permutation(vals).reshape(16, 32) for _ in range(waves)])
    B = np.stack([rng.permutation(vals).reshape(32, 16) for _ in range(waves)])
    C = np.stack([rng.permutation(np.arange(-128, 128)).reshape(16, 16) * 4096 for _ in range(waves)])
    assert (np.abs(A) @ np.abs(B)).max() + np.abs(C).max() < 2 ** 24      # every partial sum, in any order, is exact in fp32
    return _bf16_pack(A.astype(F32), B.astype(F32), C.astype(F32)), (C + A @ B).astype(F32)


def _mfma16_bf16_lane_map_case(pa, lib, device):
    words, want = shared('mfma16_bf16', _mfma16_bf16_lane_map_inputs)
    got = _mfma_unpack(probe(pa, lib, device, MFMA16_BF16, words, T * 4, 2, F32), 8)
    assert same_bits(got, want), np.argwhere(got != want)[:8]


def test_mfma16_bf16_lane_and_element_map(pa, emu_lib):
    _mfma16_bf16_lane_map_case(pa, emu_lib, 'cpu')


@pytest.mark.gpu
def test_mfma16_bf16_lane_and_element_map_on_the_gpu(pa):
    _mfma16_bf16_lane_map_case(pa, *_gpu(pa))


# ---- pinn_lds_tr16: within each group of 16 lanes, lane i supplies the address of 4 consecutive 16-bit elements -- row i/4, columns
# 4*(i%4) .. +3 of a [4][16] block -- and lane n receives column n: elements (row 0..3, column n) ---------------------------------------------
def _sp_off(row, chunk, rowb):
    """ pinn_kernel.h pinn_sp_off: byte offset of 16-byte chunk `chunk` of row `row`, chunk index swizzled """
    m = 15 if rowb // 16 >= 16 else 7
    return row * rowb + ((chunk ^ (row & m)) << 4)


def _tr16_offsets(how):
    """ byte offset per lane of a block [256]. 'sp128': the addresses the width-64 split-bf16 kernels hand to the instruction (tr_frag in
    pinn_kernel.h: rows of SP_ROW_BYTES = 2 * 64 bytes with swizzled 16-byte chunks -- their only caller); 128 / 256: plain rows of
    SP_ROW_BYTES at widths 64 / 128; 32: a dense block. A different base per 16-lane group. """
    off = np.zeros(T, dtype=np.int64)
    for t in range(T):
        grp, i = t >> 4, t & 15
        if how == 'sp128':
            row0, ucol = 8 * (grp % 14) + 4 * (grp & 1), 16 * (grp & 3)         # rows below 128: the image holds 128 rows of 128 bytes
            r, u = row0 + (i >> 2), ucol + 4 * (i & 3)
            off[t] = _sp_off(r, u >> 3, 128) + ((u >> 2) & 1) * 8
        else:
            off[t] = grp * 1024 + 8 * (grp % 3) + (i >> 2) * how + (i & 3) * 8
    assert (off % 8 == 0).all() and off.min() >= 0 and off.max() + 8 <= LDS_WORDS * 4
    return off


def _tr16_inputs(how):
    blocks = []
    want = np.zeros((2, T, 4), dtype=np.uint16)
    for b in range(2):
        image = ((np.arange(2 * LDS_WORDS) * 3 + 7 * b) & 0xffff).astype(np.uint16)         # counters: distinct over the image (3 is odd)
        off = _tr16_offsets(how)
        for grp in range(16):
            block = np.zeros((4, 16), dtype=np.uint16)                                      # the [4][16] block the 16 addresses describe
            for i in range(16):
                first = off[16 * grp + i] // 2
                block[i // 4, 4 * (i % 4):4 * (i % 4) + 4] = image[first:first + 4]
            for n in range(16):
                want[b, 16 * grp + n] = block[:, n]
        blocks.append(np.concatenate([image.view(U32), off.astype(U32)]))
    return np.stack(blocks), want


@pytest.mark.parametrize('how', ['sp128', 128, 256, 32])
def test_lds_tr16(pa, emu_lib, how):
    _tr16_case(pa, emu_lib, 'cpu', how)


@pytest.mark.gpu
@pytest.mark.parametrize('how', ['sp128', 128, 256, 32])
def test_lds_tr16_on_the_gpu(pa, how):
    _tr16_case(pa, *_gpu(pa), how)


def _tr16_case(pa, lib, device, how):
    data, want = shared(('tr16', how), lambda: _tr16_inputs(how))
    got = probe(pa, lib, device, LDS_TR16, data, T * 2, 2, np.uint16).reshape(2, T, 4)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


# ---- pinn_pack_hi16: (a >> 16) | (b & 0xffff0000) -------------------------------------------------------------------------------------
def _pack_inputs():
    rng = np.random.default_rng(3)
    ab = rng.integers(0, 2 ** 32, (2 * T, 2), dtype=np.uint64).astype(U32)
    special = np.array([0x7fc00001, 0xffc12345, 0x7f800000, 0xff800000, 0x80000000, 0x00000000, 0x7f812345, 0x0000ffff, 0xffff0000, 0x00010000],
                       dtype=U32)                                       # NaN payloads, infinities, -0, ones in one half only
    ab[:10, 0], ab[5:15, 1] = special, special
    return ab, (ab[:, 0] >> U32(16)) | (ab[:, 1] & U32(0xffff0000))


def _pack_case(pa, lib, device):
    ab, want = shared('pack', _pack_inputs)
    assert np.array_equal(probe(pa, lib, device, PACK_HI16, ab, T, 2), want)


def test_pack_hi16(pa, emu_lib):
    _pack_case(pa, emu_lib, 'cpu')


@pytest.mark.gpu
def test_pack_hi16_on_the_gpu(pa):
    _pack_case(pa, *_gpu(pa))


# ---- pinn_row_sum16 and its kin: the butterfly xor 1, xor 2, half-mirror, mirror over the 16 lanes of a row -------------------------------
I16 = np.arange(16)
BUTTERFLY = (I16 ^ 1, I16 ^ 2, (I16 & 8) | (7 - (I16 & 7)), 15 - I16)        # quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror


def row_sum16(x):
    """ [..., 16] -> the documented butterfly in x's own precision: every step adds the partner's value of the step before """
    v = x.copy()
    for partner in BUTTERFLY:
        v = v + v[..., partner]
    return v


def left_to_right(x):
    s = x[..., 0].copy()
    for i in range(1, x.shape[-1]):
        s = s + x[..., i]
    return s


def mixed_rows(rng, n, dtype, spread):
    """ n rows of 16 values of mixed magnitude and sign for which the butterfly gives other bits than a left-to-right sum """
    rows = []
    while len(rows) < n:
        cand = (rng.standard_normal((4 * n, 16)) * np.exp2(rng.uniform(-spread, spread, (4 * n, 16)))).astype(dtype)
        differs = row_sum16(cand)[:, 0] != left_to_right(cand)
        rows += list(cand[differs])
    return np.stack(rows[:n])


def _row_sum_inputs(kind):
    rng = np.random.default_rng({'f32': 1, 'n3': 2, 'f64': 3}[kind])
    dtype, per_lane = (F64 if kind == 'f64' else F32), (3 if kind == 'n3' else 1)
    x = mixed_rows(rng, 2 * 16 * per_lane, dtype, 30 if kind == 'f64' else 12).reshape(2 * 16, per_lane, 16)    # [block x row][value][lane of the row]
    want = row_sum16(x)
    assert (want[..., 0] != left_to_right(x)).all()                      # association is part of the contract: these inputs tell
    assert x.dtype == dtype and want.dtype == dtype
    return x.transpose(0, 2, 1), want.transpose(0, 2, 1)                # -> [block x row][lane][value]: g-major like the probe's buffers


def _row_sum_case(pa, lib, device, kind):
    x, want = shared(('row_sum', kind), lambda: _row_sum_inputs(kind))
    which, words, dtype = {'f32': (ROW_SUM16, 1, F32), 'n3': (ROW_SUM16_N3, 3, F32), 'f64': (ROW_SUM16_F64, 2, F64)}[kind]
    got = probe(pa, lib, device, which, x, T * words, 2, dtype)
    assert same_bits(got, want), kind


@pytest.mark.parametrize('kind', ['f32', 'n3', 'f64'])
def test_row_sum16_butterfly(pa, emu_lib, kind):
    _row_sum_case(pa, emu_lib, 'cpu', kind)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['f32', 'n3', 'f64'])
def test_row_sum16_butterfly_on_the_gpu(pa, kind):
    _row_sum_case(pa, *_gpu(pa), kind)


# ---- pinn_rows_sum: x[l] + x[l^16], then + the same of lane l^32; pinn_shfl_xor ------------------------------------------------------
def _rows_sum_inputs():
    rng = np.random.default_rng(5)
    cols = []
    while len(cols) < 8 * 16:                                           # per (wave, lane & 15): the four rows' values
        cand = (rng.standard_normal((512, 4)) * np.exp2(rng.uniform(-12, 12, (512, 4)))).astype(F32)
        pairs = (cand[:, 0] + cand[:, 1]) + (cand[:, 2] + cand[:, 3])
        cols += list(cand[pairs != left_to_right(cand)])
    x = np.stack(cols[:8 * 16]).reshape(8, 16, 4).transpose(0, 2, 1).reshape(8, 64).copy()      # [wave][lane]
    y = x + x[:, LANE ^ 16]
    want = y + y[:, LANE ^ 32]
    seq = ((x[:, :16] + x[:, 16:32]) + x[:, 32:48]) + x[:, 48:]
    assert (want[:, :16] != seq).all() and want.dtype == F32
    return x, want


def _rows_sum_case(pa, lib, device):
    x, want = shared('rows_sum', _rows_sum_inputs)
    assert same_bits(probe(pa, lib, device, ROWS_SUM, x, T, 2, F32), want)


def test_rows_sum(pa, emu_lib):
    _rows_sum_case(pa, emu_lib, 'cpu')


@pytest.mark.gpu
def test_rows_sum_on_the_gpu(pa):
    _rows_sum_case(pa, *_gpu(pa))


def _shfl_case(pa, lib, device):
    x, _ = shared('rows_sum', _rows_sum_inputs)
    want = np.stack([x[:, LANE ^ (1 << m)] for m in range(6)], axis=-1)         # [wave][lane][mask]
    assert same_bits(probe(pa, lib, device, SHFL_XOR, x, T * 6, 2, F32), want)


def test_shfl_xor(pa, emu_lib):
    _shfl_case(pa, emu_lib, 'cpu')


@pytest.mark.gpu
def test_shfl_xor_on_the_gpu(pa):
    _shfl_case(pa, *_gpu(pa))


# ---- pinn_rows_total_f64: v equal within each 16-lane row -> the sum over the four rows in the DEVICE's order: the row values of lanes 0,
# 16, 32, 48 added in sequence from zero, ((r0 + r1) + r2) + r3 ------------------------------------------------------------------------
def _rows_total_inputs():
    rng = np.random.default_rng(9)
    rows = rng.standard_normal((8, 4)) * np.exp2(rng.uniform(-40, 40, (8, 4)))
    rows[0] = (2.0 ** 53, 0.0, 1.0, 1.0)            # ((2^53 + 0) + 1) + 1 = 2^53 (ties to even, twice); a butterfly gives 2^53 + 2
    rows[1] = (1.0, 2.0 ** 53, -2.0 ** 53, 1.0)     # 1: the 1 is lost in the first add; a butterfly gives 2^53 + (1 - 2^53) = 2
    want = ((0.0 + rows[:, 0]) + rows[:, 1]) + rows[:, 2]
    want = want + rows[:, 3]
    assert want[0] == 2.0 ** 53 and (rows[0, 0] + rows[0, 1]) + (rows[0, 2] + rows[0, 3]) == 2.0 ** 53 + 2
    return np.repeat(rows, 16, axis=1), np.repeat(want[:, None], 64, axis=1)        # [wave][lane]


def _rows_total_case(pa, lib, device):
    x, want = shared('rows_total', _rows_total_inputs)
    got = probe(pa, lib, device, ROWS_TOTAL_F64, x, T * 2, 2, F64).reshape(8, 64)
    print(f'rows (2^53, 0, 1, 1): got {got[0, 0]!r} (2^53 + {got[0, 0] - 2.0 ** 53:g}), the device order gives {want[0, 0]!r}')
    assert same_bits(got, want), (got[:, 0], want[:, 0])


def test_rows_total_f64_device_order(pa, emu_lib):
    _rows_total_case(pa, emu_lib, 'cpu')


@pytest.mark.gpu
def test_rows_total_f64_device_order_on_the_gpu(pa):
    _rows_total_case(pa, *_gpu(pa))


# ---- pinn_wave_uniform: a value the whole wave agrees on -----------------------------------------------------------------------------
def _wave_uniform_case(pa, lib, device):
    per_wave = np.array([7, -3, 0x7fffffff, -0x80000000, 0, 123456, -1, 42], dtype=I32)          # different between the waves of a block
    x = np.repeat(per_wave[:, None], 64, axis=1)
    assert np.array_equal(probe(pa, lib, device, WAVE_UNIFORM, x, T, 2, I32).reshape(8, 64), x)     # waves do not leak into each other


def test_wave_uniform(pa, emu_lib):
    _wave_uniform_case(pa, emu_lib, 'cpu')


@pytest.mark.gpu
def test_wave_uniform_on_the_gpu(pa):
    _wave_uniform_case(pa, *_gpu(pa))


_CHILD = """
import ctypes, sys
import numpy as np
lib = ctypes.CDLL(sys.argv[1])
lib.pinn_port_probe.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
x = np.full(256, 5, dtype=np.int32)
x[64 + 37] = 6
out = np.zeros(256, dtype=np.int32)
print('rc', lib.pinn_port_probe(10, x.ctypes.data, out.ctypes.data, 1, None), flush=True)
"""


def test_emulator_refuses_a_value_that_is_not_wave_uniform(emu_lib):
    """ the device would hand every lane the first lane's value and say nothing: the emulator aborts and names the values. (A child
    process: the check ends it. PINN_EMU_STRICT=0 switches the check off: every lane keeps its own value, as before.) """
    env = dict(os.environ)
    env.pop('PINN_EMU_STRICT', None)
    res = subprocess.run([sys.executable, '-c', _CHILD, emu_lib._name], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode != 0 and 'rc' not in res.stdout, (res.returncode, res.stdout, res.stderr)
    assert 'pinn_wave_uniform' in res.stderr and 'wave 1' in res.stderr and 'lane 37 holds 6' in res.stderr, res.stderr
    env['PINN_EMU_STRICT'] = '0'
    res = subprocess.run([sys.executable, '-c', _CHILD, emu_lib._name], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0 and 'rc 0' in res.stdout, (res.returncode, res.stdout, res.stderr)


def test_product_kernels_pass_the_wave_uniform_check(pa, emu_lib, monkeypatch):
    """ one step of BASELINE configs 2 and 4 (two-team kernels: the team index goes through pinn_wave_uniform) and one one-CU fit chunk of
    config 1 with the emulator's agreement check on: a value that is not uniform would abort the process """
    monkeypatch.setenv('PINN_EMU_STRICT', '1')
    kw = dict(_lib=emu_lib, device='cpu')
    for name in ('cfg2', 'cfg4'):
        cfg, solver = make_solver(name, pa, **kw)
        rng = np.random.default_rng(11)
        pts = torch.from_numpy(rng.random((48, solver.model.net.layout.d)).astype(F32))
        solver._fused_step(pts, 1)
        assert emu_lib.pinn_debug_last_kernel() == 2
        assert np.isfinite(float(solver.grads[solver.model.net.layout.off_loss]))
    monkeypatch.setenv('PYDENS_AMD_FIT_PERSIST', '2')
    monkeypatch.setenv('PYDENS_AMD_FIT_GRAPH', '1')
    monkeypatch.setenv('PYDENS_AMD_FIT_ROUNDS', '4')
    monkeypatch.setattr(pa.Solver, 'FIT_CTRL_ON_HOST', True)
    _, solver = make_solver('cfg1', pa, **kw)
    solver.fit(niters=3, batch_size=100, lr=0.005)
    assert solver.last_fit_path == 'fused' and emu_lib.pinn_last_kernel_name().decode().startswith('pinn_fit_kernel<')
    assert np.isfinite([float(v) for v in solver.losses]).all()


# ---- pinn_rows + pinn_rows_st4 / pinn_rows_ld4: lane-private f32x4 rows of a wave-owned block, ONE offset lane * 16 for every row, the row
# offset beside it; the block is declared with a byte bound ----------------------------------------------------------------------------
def _rows_case(pa, lib, device):
    n_blocks, n_rows = 2, 3
    rng = np.random.default_rng(21)
    x = rng.standard_normal((n_blocks * 4, 64, n_rows, 4)).astype(F32)            # [block x wave][lane][row][4]
    out = probe(pa, lib, device, ROWS, x, 2 * 4 * n_rows * 64 * 4, n_blocks, F32)
    slabs, back = out[:x.size].reshape(n_blocks * 4, n_rows, 64, 4), out[x.size:].reshape(x.shape)
    # row r of lane l sits at byte r * 1024 + l * 16 of its wave's slab; the last row ends exactly at the declared bound (3 * 1024 bytes):
    # reached, never crossed -- an off-by-one in lane_bytes / row_bytes would drop lane 63's last row on the device (the pattern stays)
    # and abort on the emulator
    assert same_bits(slabs, x.transpose(0, 2, 1, 3))
    assert same_bits(back, x)


def test_rows_written_and_read_back_up_to_the_byte_bound(pa, emu_lib):
    _rows_case(pa, emu_lib, 'cpu')


@pytest.mark.gpu
def test_rows_written_and_read_back_up_to_the_byte_bound_on_the_gpu(pa):
    _rows_case(pa, *_gpu(pa))


# ---- PINN_WAVE_SYNC: LDS exchange between the lanes of one wave --------------------------------------------------------------------------
def _wave_sync_case(pa, lib, device):
    rng = np.random.default_rng(23)
    x = rng.integers(0, 2 ** 32, (8, 64), dtype=np.uint64).astype(U32)
    v, want = x.copy(), []
    for r in range(4):                              # lane l stores word l, syncs, reads word 63 - l, syncs
        v = v[:, 63 - LANE] * U32(3) + (LANE + r).astype(U32)
        want.append(v)
    assert np.array_equal(probe(pa, lib, device, WAVE_SYNC, x, T * 4, 2).reshape(8, 64, 4), np.stack(want, axis=-1))


def test_wave_sync_orders_a_waves_own_lds_traffic(pa, emu_lib):
    _wave_sync_case(pa, emu_lib, 'cpu')


@pytest.mark.gpu
def test_wave_sync_orders_a_waves_own_lds_traffic_on_the_gpu(pa):
    _wave_sync_case(pa, *_gpu(pa))


# ---- pinn_flag_publish / pinn_flag_load / pinn_flag_arrive: data, then flag -- flag, then data; an arrival counter among four waves.
# Every poll of the probe is bounded: a flag that never shows is a -1 in the output, never a hang -------------------------------------------
def _flags_case(pa, lib, device):
    rng = np.random.default_rng(29)
    x = rng.integers(1, 2 ** 20, (2, 4, 64)).astype(I32)                   # [block][wave][lane]; positive: -1 marks a poll that ran out
    want = np.zeros((2, 4, 64, 5), dtype=I32)
    want[..., 0] = x
    want[:, 1, :, 0] = x[:, 0]                                           # wave 1 reads what wave 0 published
    for r in range(1, 5):
        want[..., r] = x[:, (np.arange(4) + 1) & 3] * 7 + r              # the next wave's word of the round
    got = probe(pa, lib, device, FLAGS, x, T * 5, 2, I32).reshape(want.shape)
    assert not (got == -1).any(), np.argwhere(got == -1)[:8]
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


def test_flags_between_waves(pa, emu_lib):
    _flags_case(pa, emu_lib, 'cpu')


@pytest.mark.gpu
def test_flags_between_waves_on_the_gpu(pa):
    _flags_case(pa, *_gpu(pa))


@pytest.mark.parametrize('order', [1, 2, 3])
def test_flags_between_waves_in_any_wave_order(pa, emu_lib, order, monkeypatch):
    """ (emulator only: its waves advance in a random order and stall for random stretches) """
    monkeypatch.setenv('PINN_EMU_SHUFFLE', str(order))
    _flags_case(pa, emu_lib, 'cpu')


def test_unknown_probe_is_refused(pa, emu_lib):
    buf = torch.zeros(T * 12, dtype=torch.int32)
    p = ctypes.c_void_p(buf.data_ptr())
    for which in (-1, 16, 1000):
        assert emu_lib.pinn_port_probe(which, p, p, 1, None) != 0
        assert b'unknown port probe' in emu_lib.pinn_last_error()
    assert emu_lib.pinn_port_probe(EXP2, None, p, 1, None) != 0 and b'null' in emu_lib.pinn_last_error()
    assert emu_lib.pinn_port_probe(EXP2, p, p, 0, None) != 0 and b'n_blocks' in emu_lib.pinn_last_error()
    assert not buf.any()


# ---- pinn_exp2 / pinn_rcp: "~1 ulp" ---------------------------------------------------------------------------------------------------
ULP_BAR = 1.0           # pinn_port.h: "2^x and 1/x at hardware precision (v_exp_f32 / v_rcp_f32, ~1 ulp)". A device that measures above it is a finding:
#                         the comment in pinn_port.h is then corrected and the bar becomes the measured maximum rounded up to a whole ulp


def ulp_error(got, exact):
    """ |got - exact| in units of the fp32 spacing at `exact` (normal range) """
    _, e = np.frexp(exact)                          # exact = m 2^e, m in [0.5, 1): the spacing of fp32 there is 2^(e - 24)
    return np.abs(got.astype(F64) - exact) / np.exp2((e - 24).astype(F64))


def _pad(x):
    return np.concatenate([x, np.ones((-x.size) % T, dtype=x.dtype)])


def _exp2_case(pa, lib, device):
    n = 2 ** 16
    rng = np.random.default_rng(41)
    for name, lo, hi in (('tanh range [-126, 0]', -126.0, 0.0), ('sigmoid range [0, 126]', 0.0, 126.0)):
        x = np.sort(np.concatenate([np.linspace(lo, hi, n // 2), rng.uniform(lo, hi, n // 2)])).astype(F32)
        got = probe(pa, lib, device, EXP2, x, T, n // T, F32)
        err = ulp_error(got, np.exp2(x.astype(F64)))
        print(f'pinn_exp2, {name}, {n} inputs: max error {err.max():.4f} ulp at x = {x[err.argmax()]!r}, mean {err.mean():.4f} ulp')
        assert err.max() <= ULP_BAR
    edges = _pad(np.array([-0.0, 0.0, np.inf, -np.inf, 128.0, 128.5, 1000.0, 3e38], dtype=F32))
    got = probe(pa, lib, device, EXP2, edges, T, 1, F32)
    assert same_bits(got[:8], np.array([1.0, 1.0, np.inf, 0.0, np.inf, np.inf, np.inf, np.inf], dtype=F32)), got[:8]
    below = _pad(np.array([-126.5, -127.0, -130.0, -140.0, -149.0, -150.0, -1000.0, -3e38], dtype=F32))
    got = probe(pa, lib, device, EXP2, below, T, 1, F32)[:8]
    print('pinn_exp2 below -126:', ', '.join(f'{x:g} -> {g!r}' for x, g in zip(below[:8], got)))
    assert ((got >= 0.0) & (got <= F32(2.0 ** -126))).all() and not np.signbit(got).any()


def _rcp_case(pa, lib, device):
    n = 2 ** 16
    rng = np.random.default_rng(43)
    x = np.sort(np.concatenate([np.linspace(1.0, 2.0, n // 2), rng.uniform(1.0, 2.0, n // 2)])).astype(F32)
    got = probe(pa, lib, device, RCP, x, T, n // T, F32)
    err = ulp_error(got, 1.0 / x.astype(F64))
    print(f'pinn_rcp, [1, 2], {n} inputs: max error {err.max():.4f} ulp at x = {x[err.argmax()]!r}, mean {err.mean():.4f} ulp')
    assert err.max() <= ULP_BAR
    x = np.minimum(np.exp2(np.linspace(-126.0, 126.0, 4 * T)), 2.0 ** 126).astype(F32)          # log-spaced, results down to 2^-126 (normal)
    x = np.concatenate([x, -x])
    got = probe(pa, lib, device, RCP, x, T, 8, F32)
    err = ulp_error(got, 1.0 / x.astype(F64))
    print(f'pinn_rcp, +-2^-126 .. 2^126 log-spaced, {x.size} inputs: max error {err.max():.4f} ulp at x = {x[err.argmax()]!r}')
    assert err.max() <= ULP_BAR
    got = probe(pa, lib, device, RCP, _pad(np.array([np.inf, -np.inf], dtype=F32)), T, 1, F32)[:2]
    assert same_bits(got, np.array([0.0, -0.0], dtype=F32)), got


def test_exp2_within_one_ulp(pa, emu_lib):
    _exp2_case(pa, emu_lib, 'cpu')


@pytest.mark.gpu
def test_exp2_within_one_ulp_on_the_gpu(pa):
    _exp2_case(pa, *_gpu(pa))


def test_rcp_within_one_ulp(pa, emu_lib):
    _rcp_case(pa, emu_lib, 'cpu')


@pytest.mark.gpu
def test_rcp_within_one_ulp_on_the_gpu(pa):
    _rcp_case(pa, *_gpu(pa))


# ---- rounding inside the MFMAs: the device's internal order is undocumented; the claim is "at or below the error of an fp32 fmaf chain" ----
def fmaf(a, b, c):
    """ fp32 fused multiply-add of fp32 arrays, correctly rounded: the product is exact in double, the sum is taken in double rounded TO
    ODD (two-sum error term), which makes the second rounding to fp32 harmless (53 >= 2 * 24 + 2) """
    p = a.astype(F64) * b.astype(F64)
    c = c.astype(F64)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)                     # exact: s + e = p + c
    odd = (s.view(np.int64) & 1).astype(bool)
    fix = (e != 0) & ~odd                           # inexact and even: step to the odd neighbour on e's side
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def _cancelling(rng, waves, k, bf16_parts):
    """ A [waves][16][k], B [waves][k][16], C = 0 whose products cancel: the second half of the k slots repeats the first with the opposite
    sign, up to a relative 2^-10. bf16_parts: the slots hold the exact three-way bf16 splits (hi, mid, lo: 8 + 8 + 8 bits) of fp32 values,
    beside bf16 values in B -- mixed magnitudes, as in the split-bf16 GEMMs """
    if not bf16_parts:
        h = k // 2
        a, b = rng.standard_normal((waves, 16, h)), rng.standard_normal((waves, h, 16))
        A = np.concatenate([a, -a * (1 + rng.uniform(-1, 1, a.shape) * 2.0 ** -10)], axis=2).astype(F32)
        B = np.concatenate([b, b * (1 + rng.uniform(-1, 1, b.shape) * 2.0 ** -10)], axis=1).astype(F32)
        return A, B
    vals = k // 6                                                          # values per half: three slots each (k = 32: 5, two slots stay zero)
    a = rng.standard_normal((waves, 16, vals))
    a = np.concatenate([a, -a * (1 + rng.uniform(-1, 1, a.shape) * 2.0 ** -10)], axis=2).astype(F32)
    b = rng.standard_normal((waves, vals, 16))
    b = np.concatenate([b, b], axis=1).astype(F32)

    def trunc(x):
        return (x.view(U32) & U32(0xffff0000)).view(F32)
    hi = trunc(a)
    mid = trunc(a - hi)
    lo = trunc(a - hi - mid)
    assert np.array_equal(hi + mid + lo, a)                                # the split is exact
    A = np.zeros((waves, 16, k), dtype=F32)
    B = np.zeros((waves, k, 16), dtype=F32)
    for part, plane in enumerate((hi, mid, lo)):
        A[:, :, part:3 * 2 * vals:3] = plane
        B[:, part:3 * 2 * vals:3, :] = trunc(b)
    return A, B


def _rounding_case(pa, lib, device, which):
    waves, k = 8, (4 if which == MFMA16 else 32)
    def make():
        A, B = _cancelling(np.random.default_rng(100 + k), waves, k, which == MFMA16_BF16)
        C = np.zeros((waves, 16, 16), dtype=F32)
        exact = np.einsum('wik,wkj->wij', A.astype(F64), B.astype(F64))    # products exact in double; k adds: 1e-16 of the largest term
        size = np.einsum('wik,wkj->wij', np.abs(A).astype(F64), np.abs(B).astype(F64))
        chain = C.copy()
        for s in range(k):                                                 # the ascending fp32 fmaf chain
            chain = fmaf(A[:, :, s:s + 1], B[:, s:s + 1, :], chain)
        once = exact.astype(F32)                                           # the emulator's bf16 statement: summed in double, rounded once
        if which == MFMA16:
            Z = np.zeros_like(A)
            data = _mfma16_pack(A, B, Z, Z.transpose(0, 2, 1), C)          # (the probe's second call multiplies zeros: K = 4)
        else:
            data = _bf16_pack(A, B, C)
        return data, exact, size, chain, once
    data, exact, size, chain, once = shared(('rounding', which), make)
    assert np.median(size / np.abs(exact)) > 100                           # the sums do cancel
    got = _mfma_unpack(probe(pa, lib, device, which, data, T * 4, 2, F32), waves)
    err, err_chain = np.abs(got.astype(F64) - exact), np.abs(chain.astype(F64) - exact)
    emu = chain if which == MFMA16 else once
    name = 'pinn_mfma16 (K = 4)' if which == MFMA16 else 'pinn_mfma16_bf16 (K = 32, three-way splits)'
    print(f'{name}: max |result - f64| {err.max():.3e}, max |fmaf chain - f64| {err_chain.max():.3e} (ratio {err.max() / err_chain.max():.3f}); '
          f'bit-identical to the fmaf chain {100 * np.mean(got.view(U32) == chain.view(U32)):.1f} %, to the emulator\'s statement '
          f'{100 * np.mean(got.view(U32) == emu.view(U32)):.1f} % of {got.size} results')
    assert err_chain.max() > 0
    assert err.max() <= 2 * err_chain.max()


def test_mfma16_rounding_at_or_below_the_fmaf_chain(pa, emu_lib):
    _rounding_case(pa, emu_lib, 'cpu', MFMA16)


@pytest.mark.gpu
def test_mfma16_rounding_at_or_below_the_fmaf_chain_on_the_gpu(pa):
    _rounding_case(pa, *_gpu(pa), MFMA16)


def test_mfma16_bf16_rounding_at_or_below_the_fmaf_chain(pa, emu_lib):
    _rounding_case(pa, emu_lib, 'cpu', MFMA16_BF16)


@pytest.mark.gpu
def test_mfma16_bf16_rounding_at_or_below_the_fmaf_chain_on_the_gpu(pa):
    _rounding_case(pa, *_gpu(pa), MFMA16_BF16)
