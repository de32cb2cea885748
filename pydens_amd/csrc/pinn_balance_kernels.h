// pinn_balance_kernels.h -- loss-term weights on the flat gradient buffer: the terms of a fit kept apart for one more step and combined on
// the device; included by pinn_abi.cpp only (pinn_balance_terms of include/pinn.h: three launches per call, whatever the number of terms).
//
// T <= 8 term rows term_grads[j * ld + i]: row j is the gradient buffer term j wrote on its own (its loss in entry off_loss).
//   pinn_balance_stats_kernel     grid over 4096-entry slices of n: every workgroup reads its slice of every row once and forms, over the
//                                 live entries of each term, max|g| (fp32), sum|g| and sum g^2 (fp64: the product of two fp32 values is
//                                 exact there), whether any is non-finite, and the live count; one row of partials per workgroup
//   pinn_balance_finalize_kernel  one workgroup: rows summed in ascending order, the weight rule of the call in fp64 (one thread: at
//                                 most eight terms), weights and statistics to the caller's state block
//   pinn_balance_combine_kernel   out[i] = fl32(sum_j w_j g_j[i]), the sum in fp64 in ascending j, one rounding; the owner of the loss
//                                 slot also writes the weighted loss, the unweighted term losses and the weights as floats
// No atomics, no waits between workgroups: launch boundaries order the passes, every sum has a fixed order (bit-repeatable).
// Live: i < n, i != off_loss and mask[i] != 0 (no mask: every such entry). Other entries enter no statistic and are never written --
// but for out[off_loss], which takes the weighted loss.
#pragma once
#include "pinn_port.h"

#ifndef PINN_BALANCE_MAX_TERMS
#define PINN_BALANCE_MAX_TERMS 8        // (include/pinn.h)
#endif
#ifndef PINN_BALANCE_FIXED
#define PINN_BALANCE_FIXED 0            // (include/pinn.h) `kind`: the weights stay as the state holds them
#define PINN_BALANCE_MAX_MEAN 1         // max|g_ref| / mean|g_i|
#define PINN_BALANCE_NORM 2             // sum_j |g_j|_2 / |g_i|_2
#endif
#define PINN_BALANCE_THREADS 256
#define PINN_BALANCE_SLICE 1024         // entries per sweep of a workgroup: one 16-byte piece per thread (the combine pass: one sweep)
#define PINN_BALANCE_PIECES 4           // sweeps per workgroup of the stats pass
#define PINN_BALANCE_STATS_SLICE (PINN_BALANCE_PIECES * PINN_BALANCE_SLICE)

// the state block (doubles; integers are stored as doubles, exactly): pinn_balance_state_bytes = PINN_BALANCE_STATE_DOUBLES * 8
#define PINN_BALANCE_W 0                // weights [8]
#define PINN_BALANCE_UPDATES 8          // calls so far that ran the weight rule (update != 0, an adaptive kind)
#define PINN_BALANCE_COUNT 9            // live entries of the last call
#define PINN_BALANCE_GMAX 16            // max |g_j| [8] of the last call
#define PINN_BALANCE_SABS 24            // sum |g_j| [8]
#define PINN_BALANCE_SSQ 32             // sum g_j^2 [8]
#define PINN_BALANCE_BAD 40             // 1: a live entry of term j was NaN or infinite [8]
#define PINN_BALANCE_STATE_DOUBLES 48
// a row of partials: per term j (max|g|, sum|g|, sum g^2, non-finite) at 4 j, then the live count
#define PINN_BALANCE_ROWLEN(T) (4 * (T) + 1)

struct PinnBalanceArgs {
    const float* g; float* out; const unsigned char* mask;
    long long n, ld;                    // entries; row stride of the term rows (a multiple of 4, >= n)
    int T, off_loss, kind, ref, update;
    double momentum, lo, hi;
    double* state; double* rows; int n_rows;
    float* term_loss_out; float* weight_out;
    double init[PINN_BALANCE_MAX_TERMS];        // pinn_balance_init: the weights, by value
};

PINN_DEVICE void pinn_balance_live4(const PinnBalanceArgs& A, long long i, bool (&live)[4]) {
    for (int e = 0; e < 4; ++e) live[e] = i + e < A.n && i + e != (long long)A.off_loss && (!A.mask || A.mask[i + e] != 0);
}
// sum over the wave in double, the same value in every lane (DPP within the 16-lane rows, then the four rows in order)
PINN_DEVICE double pinn_balance_wave_sum(double v) { return pinn_rows_total_f64(pinn_row_sum16_f64(v)); }
PINN_DEVICE float pinn_balance_wave_max(float v) {
    for (int mask = 1; mask < 64; mask <<= 1) v = fmaxf(v, pinn_shfl_xor(v, mask));
    return v;
}
PINN_DEVICE bool pinn_balance_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }       // (false for NaN)

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(PINN_BALANCE_THREADS) pinn_balance_init_kernel(PinnBalanceArgs A) {
    const int tid = PINN_TID;
    if (tid < PINN_BALANCE_STATE_DOUBLES) A.state[tid] = tid < A.T ? A.init[tid] : 0.0;
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(PINN_BALANCE_THREADS) pinn_balance_stats_kernel(PinnBalanceArgs A) {
    PINN_SMEM(smem);
    double* part = reinterpret_cast<double*>(smem);              // [4 waves][rowlen]
    constexpr int U = PINN_BALANCE_PIECES;
    const int tid = PINN_TID, wave = tid >> 6, lane = tid & 63;
    const int T = A.T, rowlen = PINN_BALANCE_ROWLEN(T);
    // piece u of this thread: consecutive threads on consecutive 16-byte pieces, U such sweeps of 1024 entries per workgroup
    const long long base = (long long)PINN_BID * PINN_BALANCE_STATS_SLICE + 4 * tid;
    unsigned live_bits = 0;                                       // bit 4 u + e: entry e of piece u takes part
    double count = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const long long i0 = base + (long long)u * PINN_BALANCE_SLICE;
        if (i0 < A.n) {
            bool live[4];
            pinn_balance_live4(A, i0, live);
            for (int e = 0; e < 4; ++e)
                if (live[e]) { live_bits |= 1u << (4 * u + e); count += 1.0; }
        }
    }
    double* mine = part + wave * rowlen;
    for (int j = 0; j < T; ++j) {
        float gmax = 0.0f, bad = 0.0f;
        double sabs = 0.0, ssq = 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long i0 = base + (long long)u * PINN_BALANCE_SLICE;
            if (i0 >= A.n) continue;
            // (rows are ld long, ld % 4 == 0, i0 < n <= ld: always a whole piece. Entries that take no part -- masked, the loss slot, or
            //  between n and ld -- may hold anything: zero is selected here, not multiplied in)
            const f32x4 v = *reinterpret_cast<const f32x4*>(A.g + (size_t)j * A.ld + i0);
            for (int e = 0; e < 4; ++e) {
                const bool on = (live_bits >> (4 * u + e)) & 1u;
                const float a = on ? fabsf(v[e]) : 0.0f;
                if (!(a <= 3.402823466e+38f)) bad = 1.0f;         // (NaN or infinite)
                gmax = fmaxf(gmax, a);
                sabs += (double)a;
                ssq += (double)a * (double)a;
            }
        }
        gmax = pinn_balance_wave_max(gmax);
        bad = pinn_balance_wave_max(bad);
        sabs = pinn_balance_wave_sum(sabs);
        ssq = pinn_balance_wave_sum(ssq);
        if (lane == 0) { mine[4 * j + 0] = (double)gmax; mine[4 * j + 1] = sabs; mine[4 * j + 2] = ssq; mine[4 * j + 3] = (double)bad; }
    }
    count = pinn_balance_wave_sum(count);
    if (lane == 0) mine[4 * T] = count;
    PINN_SYNC();
    double* row = A.rows + (size_t)PINN_BID * rowlen;
    for (int idx = tid; idx < rowlen; idx += PINN_BALANCE_THREADS) {
        const double w0 = part[idx], w1 = part[rowlen + idx], w2 = part[2 * rowlen + idx], w3 = part[3 * rowlen + idx];
        const bool is_max = idx < 4 * T && ((idx & 3) == 0 || (idx & 3) == 3);
        row[idx] = is_max ? fmax(fmax(w0, w1), fmax(w2, w3)) : ((w0 + w1) + w2) + w3;
    }
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(PINN_BALANCE_THREADS) pinn_balance_finalize_kernel(PinnBalanceArgs A) {
    PINN_SMEM(smem);
    double* tot = reinterpret_cast<double*>(smem);               // [rowlen]
    const int tid = PINN_TID, T = A.T, rowlen = PINN_BALANCE_ROWLEN(T);
    // the rows in ascending order (a NaN among the maxima cannot occur: fmaxf dropped it, the non-finite flag carries it)
    for (int idx = tid; idx < rowlen; idx += PINN_BALANCE_THREADS) {
        const bool is_max = idx < 4 * T && ((idx & 3) == 0 || (idx & 3) == 3);
        double acc = 0.0;
        for (int r = 0; r < A.n_rows; ++r) {
            const double x = A.rows[(size_t)r * rowlen + idx];
            acc = is_max ? fmax(acc, x) : acc + x;
        }
        tot[idx] = acc;
    }
    PINN_SYNC();
    if (tid != 0) return;
    double* S = A.state;
    const double count = tot[4 * T];
    double gmax[PINN_BALANCE_MAX_TERMS], sabs[PINN_BALANCE_MAX_TERMS], ssq[PINN_BALANCE_MAX_TERMS];
    bool ok[PINN_BALANCE_MAX_TERMS];                             // the term's statistics are finite
    for (int j = 0; j < T; ++j) {
        gmax[j] = tot[4 * j]; sabs[j] = tot[4 * j + 1]; ssq[j] = tot[4 * j + 2];
        ok[j] = tot[4 * j + 3] == 0.0 && pinn_balance_finite(gmax[j]) && pinn_balance_finite(sabs[j]) && pinn_balance_finite(ssq[j]);
        S[PINN_BALANCE_GMAX + j] = gmax[j]; S[PINN_BALANCE_SABS + j] = sabs[j]; S[PINN_BALANCE_SSQ + j] = ssq[j];
        S[PINN_BALANCE_BAD + j] = ok[j] ? 0.0 : 1.0;
    }
    S[PINN_BALANCE_COUNT] = count;
    if (A.kind == PINN_BALANCE_FIXED || !A.update) return;
    S[PINN_BALANCE_UPDATES] += 1.0;
    const double m = A.momentum;
    if (A.kind == PINN_BALANCE_MAX_MEAN) {
        const double top = gmax[A.ref];
        if (!ok[A.ref] || !(top > 0.0) || !(count > 0.0)) return;       // (a zero or non-finite reference: every weight stays)
        for (int j = 0; j < T; ++j) {
            double hat = 1.0;
            if (j != A.ref) {
                const double mean = sabs[j] / count;
                if (!ok[j] || !(mean > 0.0)) continue;
                hat = top / mean;
            }
            if (!pinn_balance_finite(hat)) continue;
            S[PINN_BALANCE_W + j] = fmin(fmax(m * S[PINN_BALANCE_W + j] + (1.0 - m) * hat, A.lo), A.hi);
        }
        return;
    }
    // PINN_BALANCE_NORM: the numerator over the terms whose statistics are finite (one bad term does not stop the others), ascending j
    double norm[PINN_BALANCE_MAX_TERMS], total = 0.0;
    for (int j = 0; j < T; ++j) {
        norm[j] = ok[j] ? sqrt(ssq[j]) : 0.0;
        total += norm[j];
    }
    for (int j = 0; j < T; ++j) {
        if (!ok[j] || !(norm[j] > 0.0)) continue;
        const double hat = total / norm[j];
        if (!pinn_balance_finite(hat)) continue;
        S[PINN_BALANCE_W + j] = fmin(fmax(m * S[PINN_BALANCE_W + j] + (1.0 - m) * hat, A.lo), A.hi);
    }
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(PINN_BALANCE_THREADS) pinn_balance_combine_kernel(PinnBalanceArgs A) {
    const long long i0 = (long long)PINN_BID * PINN_BALANCE_SLICE + 4 * PINN_TID;
    if (i0 >= A.n) return;
    const int T = A.T;
    const double* w = A.state + PINN_BALANCE_W;
    bool live[4];
    pinn_balance_live4(A, i0, live);
    const int slot = (long long)A.off_loss >= i0 && (long long)A.off_loss < i0 + 4 ? (int)((long long)A.off_loss - i0) : -1;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    float term_loss[PINN_BALANCE_MAX_TERMS];
    // (every entry is read and written by this thread alone, all reads in front of all writes: `out` may be row 0 itself)
    for (int j = 0; j < T; ++j) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(A.g + (size_t)j * A.ld + i0);
        const double wj = w[j];
        for (int e = 0; e < 4; ++e) acc[e] += wj * (double)v[e];
        if (slot >= 0) term_loss[j] = v[slot];
    }
    if (slot >= 0) {
        live[slot] = true;                                        // the weighted loss: acc[slot] is sum_j w_j L_j
        for (int j = 0; j < T; ++j) {
            if (A.term_loss_out) A.term_loss_out[j] = term_loss[j];
            if (A.weight_out) A.weight_out[j] = (float)w[j];
        }
    }
    if (live[0] && live[1] && live[2] && live[3] && i0 + 4 <= A.n) {
        f32x4 o;
        for (int e = 0; e < 4; ++e) o[e] = (float)acc[e];
        *reinterpret_cast<f32x4*>(A.out + i0) = o;
        return;
    }
    for (int e = 0; e < 4; ++e) if (live[e]) A.out[i0 + e] = (float)acc[e];
}
