// pinn_port_probe.h -- one small kernel per execution primitive of pinn_port.h, for tests/test_port_contract.py.
// The primitives have two independent statements: the HIP builtins / inline assembly of pinn_port.h and the host code of the test
// build's emulator (tests/emu/emu_runtime.*). Each kernel here reads a caller's buffer, applies ONE primitive exactly as pinn_port.h
// spells it and writes every lane's result, so that both statements can be held, bit for bit, to a third one written from the
// comments of pinn_port.h. Compiled from this one source into both builds (pinn_abi.cpp: pinn_port_probe), like pinn_reduce_rows.
// Never used on the training path. This header includes pinn_port.h and nothing else of the kernels.
//
// Every probe runs workgroups of PINN_PROBE_THREADS = 256 threads (four waves); g = block * 256 + thread. Sizes per BLOCK, in
// 4-byte words (include/pinn.h repeats the table for callers):
//   which                 in                                             out
//   0  MFMA16             256 x 8: a0 b0 a1 b1 c[4]                      256 x 4: mfma16(a1, b1, mfma16(a0, b0, c))
//   1  MFMA16_BF16        256 x 12: a (4 registers) b (4) c[4]           256 x 4
//   2  LDS_TR16           4096 (LDS image) + 256 (byte offset per lane)  256 x 2: the four 16-bit elements
//   3  PACK_HI16          256 x 2: a b                                   256
//   4  ROW_SUM16          256                                            256
//   5  ROW_SUM16_N3       256 x 3                                        256 x 3
//   6  ROW_SUM16_F64      256 x 2 (a double)                             256 x 2
//   7  ROWS_SUM           256                                            256
//   8  SHFL_XOR           256                                            256 x 6: masks 1, 2, 4, 8, 16, 32
//   9  ROWS_TOTAL_F64     256 x 2 (a double)                             256 x 2
//   10 WAVE_UNIFORM       256 (int)                                      256
//   11 ROWS               256 x 12: three f32x4 rows per lane            2 x 3072: the four waves' slabs, then what was read back
//   12 WAVE_SYNC          256                                            256 x 4: one word per round
//   13 FLAGS              256                                            256 x 5: the handed-over word, then one word per round
//   14 EXP2               256                                            256
//   15 RCP                256                                            256
#pragma once
#include "pinn_port.h"

enum {
    PINN_PROBE_MFMA16 = 0, PINN_PROBE_MFMA16_BF16, PINN_PROBE_LDS_TR16, PINN_PROBE_PACK_HI16, PINN_PROBE_ROW_SUM16,
    PINN_PROBE_ROW_SUM16_N3, PINN_PROBE_ROW_SUM16_F64, PINN_PROBE_ROWS_SUM, PINN_PROBE_SHFL_XOR, PINN_PROBE_ROWS_TOTAL_F64,
    PINN_PROBE_WAVE_UNIFORM, PINN_PROBE_ROWS, PINN_PROBE_WAVE_SYNC, PINN_PROBE_FLAGS, PINN_PROBE_EXP2, PINN_PROBE_RCP,
    PINN_PROBE_COUNT
};
#define PINN_PROBE_THREADS 256
#define PINN_PROBE_LDS_WORDS 4096               // LDS image of the transpose-read probe (the only probe with more than 1 KiB of LDS)
#define PINN_PROBE_ROWS_N 3                     // rows per lane of the buffer-row probe: a wave's slab is 3 x 64 x 16 bytes
#ifndef PINN_PROBE_ROWS_BOUND                   // (the declared byte bound of that slab: its exact size)
#define PINN_PROBE_ROWS_BOUND (PINN_PROBE_ROWS_N * 64 * 16)
#endif
#define PINN_PROBE_SYNC_ROUNDS 4
#define PINN_PROBE_FLAG_ROUNDS 4
#define PINN_PROBE_SPIN_BOUND (1 << 20)         // every poll loop gives up after this many looks: a lost flag is a wrong word, never a hang

#define PINN_PROBE_G ((size_t)PINN_BID * PINN_PROBE_THREADS + (size_t)PINN_TID)

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_probe_mfma16(const float* in, float* out) {
    const size_t g = PINN_PROBE_G;
    const float* p = in + 8 * g;
    f32x4 c = {p[4], p[5], p[6], p[7]};
    c = pinn_mfma16(p[0], p[1], c);
    c = pinn_mfma16(p[2], p[3], c);             // (the first result is the second call's accumulator)
    for (int r = 0; r < 4; ++r) out[4 * g + r] = c[r];
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_probe_mfma16_bf16(const unsigned* in, float* out) {
    const size_t g = PINN_PROBE_G;
    const unsigned* p = in + 12 * g;            // (48 bytes per lane: every operand starts on a 16-byte boundary)
    const pinn_s16x8 a = *reinterpret_cast<const pinn_s16x8*>(p), b = *reinterpret_cast<const pinn_s16x8*>(p + 4);  // four registers each
    const float* pc = reinterpret_cast<const float*>(p + 8);
    f32x4 c = {pc[0], pc[1], pc[2], pc[3]};
    c = pinn_mfma16_bf16(a, b, c);
    for (int r = 0; r < 4; ++r) out[4 * g + r] = c[r];
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_probe_lds_tr16(const unsigned* in, unsigned* out) {
    PINN_SMEM(smem);
    unsigned* lds = reinterpret_cast<unsigned*>(smem);
    const unsigned* blk = in + (size_t)PINN_BID * (PINN_PROBE_LDS_WORDS + PINN_PROBE_THREADS);
    for (int i = PINN_TID; i < PINN_PROBE_LDS_WORDS; i += PINN_PROBE_THREADS) lds[i] = blk[i];
    PINN_SYNC();
    // this lane's address: 8-byte aligned, inside the image (the mask keeps a caller's mistake inside it)
    const int off = (int)(blk[PINN_PROBE_LDS_WORDS + PINN_TID] & (unsigned)(PINN_PROBE_LDS_WORDS * 4 - 8));
    const pinn_s16x4 v = pinn_lds_tr16(reinterpret_cast<const char*>(lds) + off);
    const pinn_u32x2 w = __builtin_bit_cast(pinn_u32x2, v);
    out[2 * PINN_PROBE_G] = w[0];
    out[2 * PINN_PROBE_G + 1] = w[1];
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_probe_pack_hi16(const unsigned* in, unsigned* out) {
    const size_t g = PINN_PROBE_G;
    out[g] = pinn_pack_hi16(in[2 * g], in[2 * g + 1]);
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_probe_row_sum16(const float* in, float* out) {
    const size_t g = PINN_PROBE_G;
    out[g] = pinn_row_sum16(in[g]);
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_probe_row_sum16_n3(const float* in, float* out) {
    const size_t g = PINN_PROBE_G;
    float v[3] = {in[3 * g], in[3 * g + 1], in[3 * g + 2]};
    pinn_row_sum16_n<3>(v);
    for (int i = 0; i < 3; ++i) out[3 * g + i] = v[i];
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_probe_row_sum16_f64(const double* in, double* out) {
    const size_t g = PINN_PROBE_G;
    out[g] = pinn_row_sum16_f64(in[g]);
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_probe_rows_sum(const float* in, float* out) {
    const size_t g = PINN_PROBE_G;
    out[g] = pinn_rows_sum(in[g]);
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_probe_shfl_xor(const float* in, float* out) {
    const size_t g = PINN_PROBE_G;
    const float v = in[g];
    for (int m = 0; m < 6; ++m) out[6 * g + m] = pinn_shfl_xor(v, 1 << m);
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_probe_rows_total_f64(const double* in, double* out) {
    const size_t g = PINN_PROBE_G;
    out[g] = pinn_rows_total_f64(in[g]);
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_probe_wave_uniform(const int* in, int* out) {
    const size_t g = PINN_PROBE_G;
    out[g] = pinn_wave_uniform(in[g]);
}

// wave w of block b owns slab (4 b + w) of the first half of `out`: row r of lane l at byte r * 1024 + l * 16 of the slab, the last
// row ending exactly at the declared bound. Written through pinn_rows_st4, read back through pinn_rows_ld4 into the second half
// (plain stores, [g][row][4]).
PINN_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_probe_rows(const float* in, float* out) {
    const size_t g = PINN_PROBE_G;
    const int lane = PINN_TID & 63, wave = pinn_wave_uniform(PINN_TID >> 6);
    constexpr int SLAB_WORDS = PINN_PROBE_ROWS_N * 64 * 4;
    float* slab = out + ((size_t)PINN_BID * 4 + wave) * SLAB_WORDS;
    float* back = out + (size_t)PINN_NBLK * 4 * SLAB_WORDS;
    const PinnRows rows = pinn_rows(slab, (unsigned)PINN_PROBE_ROWS_BOUND);
    for (int r = 0; r < PINN_PROBE_ROWS_N; ++r) {
        const float* p = in + (g * PINN_PROBE_ROWS_N + r) * 4;
        pinn_rows_st4(rows, lane * 16, r * 1024, f32x4{p[0], p[1], p[2], p[3]});
    }
    for (int r = 0; r < PINN_PROBE_ROWS_N; ++r) {
        const f32x4 v = pinn_rows_ld4(rows, lane * 16, r * 1024);
        for (int i = 0; i < 4; ++i) back[(g * PINN_PROBE_ROWS_N + r) * 4 + i] = v[i];
    }
}

// lane l of a wave stores to the wave's LDS word l, PINN_WAVE_SYNC, reads word 63 - l, PINN_WAVE_SYNC; the word read goes into the
// next round's store, so every round depends on the one before
PINN_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_probe_wave_sync(const unsigned* in, unsigned* out) {
    PINN_SMEM(smem);
    unsigned* lds = reinterpret_cast<unsigned*>(smem);
    const size_t g = PINN_PROBE_G;
    const int lane = PINN_TID & 63, w0 = PINN_TID & ~63;
    unsigned v = in[g];
    for (int r = 0; r < PINN_PROBE_SYNC_ROUNDS; ++r) {
        lds[w0 + lane] = v;
        PINN_WAVE_SYNC();
        const unsigned o = lds[w0 + 63 - lane];
        PINN_WAVE_SYNC();
        v = o * 3u + (unsigned)(r + lane);
        out[g * PINN_PROBE_SYNC_ROUNDS + r] = v;
    }
}

// LDS words: [0, 64) wave 0's data, [64, 576) two buffers of 256 words for the rounds, 576 the flag, 577 the arrival counter.
//  (a) wave 0 writes its 64 input words, then publishes flag = 1; wave 1 polls the flag, then reads the words: out[5 g] of wave 1
//      is wave 0's word of the same lane (every other wave: its own input).
//  (b) PINN_PROBE_FLAG_ROUNDS rounds: every wave stores a word per lane into the round's buffer, arrives, polls the counter for
//      4 * round, reads the word of the NEXT wave's same lane: out[5 g + round]. Two buffers: a wave can be at most one round ahead
//      of the slowest, whose reads of the round before are in front of its own arrival.
// A poll that runs out writes -1 (and makes every later word of the lane -1); the lane goes on to the end -- nothing waits for it.
PINN_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_probe_flags(const int* in, int* out) {
    PINN_SMEM(smem);
    int* lds = reinterpret_cast<int*>(smem);
    int* flag = lds + 576;
    int* counter = lds + 577;
    const size_t g = PINN_PROBE_G;
    const int tid = PINN_TID, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { *flag = 0; *counter = 0; }
    PINN_SYNC();
    const int mine = in[g];
    bool ok = true;
    int first = mine;
    if (wave == 0) {
        lds[lane] = mine;
        pinn_flag_publish(flag, 1, lane == 0);
    } else if (wave == 1) {
        int looks = 0;
        while (pinn_flag_load(flag) != 1 && ++looks < PINN_PROBE_SPIN_BOUND) PINN_SPIN_PAUSE();
        if (looks >= PINN_PROBE_SPIN_BOUND) ok = false;
        first = lds[lane];
    }
    out[5 * g] = ok ? first : -1;
    for (int r = 1; r <= PINN_PROBE_FLAG_ROUNDS; ++r) {
        int* buf = lds + 64 + (r & 1) * 256;
        buf[tid] = mine * 7 + r;
        pinn_flag_arrive(counter, lane == 0);
        int looks = 0;
        while (pinn_flag_load(counter) < 4 * r && ++looks < PINN_PROBE_SPIN_BOUND) PINN_SPIN_PAUSE();
        if (looks >= PINN_PROBE_SPIN_BOUND) ok = false;
        const int got = buf[((wave + 1) & 3) * 64 + lane];
        out[5 * g + r] = ok ? got : -1;
    }
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_probe_exp2(const float* in, float* out) {
    const size_t g = PINN_PROBE_G;
    out[g] = pinn_exp2(in[g]);
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_probe_rcp(const float* in, float* out) {
    const size_t g = PINN_PROBE_G;
    out[g] = pinn_rcp(in[g]);
}
