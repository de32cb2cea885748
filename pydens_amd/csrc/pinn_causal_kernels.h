// pinn_causal_kernels.h -- causal training weights (Wang, Sankaran, Perdikaris 2022) over time bins of a batch; included by pinn_abi.cpp
// only (pinn_causal_weights of include/pinn.h, which states the definition: three launches per call, whatever n and the number of bins).
//
//   pinn_causal_stats_kernel     workgroup b of 256 threads owns the points [b * span, (b + 1) * span), span = chunks * 256: the grid is
//                                folded so that there are at most PINN_CAUSAL_MAX_ROWS workgroups. Per chunk of 256 points every thread
//                                leaves (bin, r^2 as a double) of its point in LDS; thread (wave w, bin k) then adds the entries of wave w
//                                that fall into bin k in LANE ORDER, thread k adds the four waves in ascending order to its running
//                                (count, sum), chunk after chunk in ascending order. One row of M (count, sum) pairs per workgroup
//   pinn_causal_rule_kernel      one workgroup: rows totalled in ascending order, L_k, the exclusive prefix and w_k by one thread in fp64
//                                (M <= 64), the ladder decision, the state block; fl32(w_k), the tolerance used and mean r^2 as floats
//                                where the caller gave the addresses
//   pinn_causal_apply_kernel     w_out[i] = fl32(w_{k(i)}), k(i) by the same helper as in the first launch
// No atomics (LDS included), no waits between workgroups: launch boundaries order the passes, every sum has a fixed order (bit-repeatable).
#pragma once
#include "pinn_port.h"

#ifndef PINN_CAUSAL_MAX_BINS
#define PINN_CAUSAL_MAX_BINS 64         // (include/pinn.h)
#define PINN_CAUSAL_MAX_EPS 8
#endif
#define PINN_CAUSAL_THREADS 256
#define PINN_CAUSAL_MAX_ROWS 256        // workgroups of the stats pass: above 65 536 points a workgroup takes several chunks
#define PINN_CAUSAL_STAGE 16            // rows of partials the rule kernel loads at a time (the order of its adds does not depend on it)

// the state block (doubles; integers are stored as doubles, exactly): pinn_causal_state_bytes = PINN_CAUSAL_STATE_DOUBLES * 8
#define PINN_CAUSAL_EPS 0               // the tolerance ladder [8]
#define PINN_CAUSAL_N_EPS 8             // its length
#define PINN_CAUSAL_INDEX 9             // the rung the NEXT call uses
#define PINN_CAUSAL_DELTA 10
#define PINN_CAUSAL_CONVERGED 11        // 1: min_k w_k > delta was seen at the last rung
#define PINN_CAUSAL_BAD 12              // 1: a call since pinn_causal_init met a residual that was NaN or infinite
#define PINN_CAUSAL_CALLS 13            // calls so far
#define PINN_CAUSAL_EPS_USED 14         // the tolerance of the last call
#define PINN_CAUSAL_MEAN_SQ 15          // its unweighted mean r^2
#define PINN_CAUSAL_NK 16               // its n_k [64]
#define PINN_CAUSAL_LK 80               // its L_k [64]
#define PINN_CAUSAL_WK 144              // its w_k [64]
#define PINN_CAUSAL_STATE_DOUBLES 208
// a row of partials, 8-byte words: bin k has its count (a 64-bit integer) in word 2 k and its sum (a double) in word 2 k + 1; word 2 M:
// 1 if a residual of the row was not finite (an integer), word 2 M + 1: padding to a 16-byte piece
#define PINN_CAUSAL_ROWLEN(M) (2 * (M) + 2)

struct PinnCausalArgs {
    const float* t; long long t_stride; const float* r; long long n;
    int M, update;
    double t_lo, t_hi;
    double* state; double* rows; int n_rows, chunks;      // chunks of 256 points per workgroup of the stats pass
    float* w_out; float* bin_weight_out; float* eps_out; float* mean_sq_out;
    double ladder[PINN_CAUSAL_MAX_EPS]; int n_eps; double delta;      // pinn_causal_init: by value
};

// the bin of a point (include/pinn.h: fp64, this association; t_hi and everything outside land in the end bins, NaN in bin 0)
PINN_DEVICE int pinn_causal_bin(float t, double t_lo, double t_hi, int M) {
    const double q = floor(((double)t - t_lo) / (t_hi - t_lo) * (double)M);
    if (q >= (double)(M - 1)) return M - 1;
    return q >= 1.0 ? (int)q : 0;                                   // (NaN fails both comparisons)
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(PINN_CAUSAL_THREADS) pinn_causal_init_kernel(PinnCausalArgs A) {
    const int tid = PINN_TID;
    if (tid >= PINN_CAUSAL_STATE_DOUBLES) return;
    double v = 0.0;
    if (tid < A.n_eps) v = A.ladder[tid];
    if (tid == PINN_CAUSAL_N_EPS) v = (double)A.n_eps;
    if (tid == PINN_CAUSAL_DELTA) v = A.delta;
    A.state[tid] = v;
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(PINN_CAUSAL_THREADS) pinn_causal_stats_kernel(PinnCausalArgs A) {
    PINN_SMEM(smem);
    double* sq = reinterpret_cast<double*>(smem);                   // [256] r^2 of the chunk's points (0: not finite, or no point)
    double* wave_sum = sq + PINN_CAUSAL_THREADS;                    // [4 waves][64 bins]
    int* bin = reinterpret_cast<int*>(wave_sum + PINN_CAUSAL_THREADS);      // [256] the point's bin | 256 if r is not finite; -1: no point
    int* wave_cnt = bin + PINN_CAUSAL_THREADS;                      // [4][64]
    int* wave_bad = wave_cnt + PINN_CAUSAL_THREADS;                 // [4][64]
    const int tid = PINN_TID, wave = tid >> 6, lane = tid & 63, M = A.M;
    const long long first = (long long)PINN_BID * A.chunks * PINN_CAUSAL_THREADS;
    long long count = 0;                                            // threads 0 .. M - 1: bin `tid` of this workgroup so far
    double sum = 0.0;
    int bad = 0;
    for (int c = 0; c < A.chunks; ++c) {
        const long long i = first + (long long)c * PINN_CAUSAL_THREADS + tid;
        int k = -1;
        double v = 0.0;
        if (i < A.n) {
            const float ri = A.r[i];
            k = pinn_causal_bin(A.t[i * A.t_stride], A.t_lo, A.t_hi, M);
            if (fabsf(ri) <= 3.402823466e+38f) v = (double)ri * (double)ri;         // (exact: a product of two fp32 values)
            else k |= 256;                                                          // NaN or infinite: counted, adds nothing
        }
        bin[tid] = k; sq[tid] = v;
        PINN_SYNC();
        {   // thread (wave, lane): bin `lane` over the 64 points of this wave, in lane order
            int n_here = 0, bad_here = 0;
            double s_here = 0.0;
            if (lane < M)
                for (int l = 0; l < 64; ++l) {
                    const int kl = bin[64 * wave + l];
                    if (kl >= 0 && (kl & 255) == lane) { n_here += 1; s_here += sq[64 * wave + l]; bad_here |= kl >> 8; }
                }
            wave_cnt[tid] = n_here; wave_sum[tid] = s_here; wave_bad[tid] = bad_here;
        }
        PINN_SYNC();
        if (tid < M) {
            count += (long long)(((wave_cnt[tid] + wave_cnt[64 + tid]) + wave_cnt[128 + tid]) + wave_cnt[192 + tid]);
            sum += ((wave_sum[tid] + wave_sum[64 + tid]) + wave_sum[128 + tid]) + wave_sum[192 + tid];
            bad |= wave_bad[tid] | wave_bad[64 + tid] | wave_bad[128 + tid] | wave_bad[192 + tid];
        }
        // (the next chunk's stores to bin / sq follow the second barrier, its stores to wave_* its own first barrier: no third one)
    }
    double* row = A.rows + (size_t)PINN_BID * PINN_CAUSAL_ROWLEN(M);
    long long* row_int = reinterpret_cast<long long*>(row);
    if (tid < M) { row_int[2 * tid] = count; row[2 * tid + 1] = sum; }
    bin[tid] = tid < M ? bad : 0;                                   // (every thread is behind the loop's last reads of bin)
    PINN_SYNC();
    if (tid == 0) {
        int any = 0;
        for (int k = 0; k < M; ++k) any |= bin[k];
        row_int[2 * M] = (long long)any;
        row_int[2 * M + 1] = 0;
    }
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(PINN_CAUSAL_THREADS) pinn_causal_rule_kernel(PinnCausalArgs A) {
    PINN_SMEM(smem);
    double* tot_sum = reinterpret_cast<double*>(smem);              // [64]
    double* tot_cnt = tot_sum + PINN_CAUSAL_MAX_BINS;               // [64] (exact: counts below 2^53)
    int* tot_bad = reinterpret_cast<int*>(tot_cnt + PINN_CAUSAL_MAX_BINS);      // [1]
    const int tid = PINN_TID, M = A.M, rowlen = PINN_CAUSAL_ROWLEN(M);
    const long long* rows_int = reinterpret_cast<const long long*>(A.rows);
    if (tid == 0) tot_bad[0] = 0;
    PINN_SYNC();
    if (tid < M) {
        // the rows in ascending order, one add after the other; the loads of PINN_CAUSAL_STAGE rows are issued together in front of their
        // adds (they do not depend on each other: one round trip to memory per stage, not per row)
        long long count = 0;
        double sum = 0.0;
        for (int row0 = 0; row0 < A.n_rows; row0 += PINN_CAUSAL_STAGE) {
            long long c[PINN_CAUSAL_STAGE];
            double v[PINN_CAUSAL_STAGE];
#pragma unroll
            for (int u = 0; u < PINN_CAUSAL_STAGE; ++u) {
                const bool in = row0 + u < A.n_rows;
                const size_t at = (size_t)(in ? row0 + u : row0) * rowlen + 2 * tid;
                c[u] = rows_int[at]; v[u] = A.rows[at + 1];
                if (!in) { c[u] = 0; v[u] = 0.0; }                  // (behind the last row: x + 0.0 is x for every sum of squares)
            }
#pragma unroll
            for (int u = 0; u < PINN_CAUSAL_STAGE; ++u) { count += c[u]; sum += v[u]; }
        }
        tot_cnt[tid] = (double)count; tot_sum[tid] = sum;
    } else if (tid >= 64) {
        // the other three waves: did any row meet a non-finite residual (an OR: no order to keep; every finder stores the same 1)
        long long any = 0;
        for (int row = tid - 64; row < A.n_rows; row += PINN_CAUSAL_THREADS - 64) any |= rows_int[(size_t)row * rowlen + 2 * M];
        if (any != 0) tot_bad[0] = 1;
    }
    PINN_SYNC();
    if (tid != 0) return;
    double* S = A.state;
    // (a block pinn_causal_init never filled may hold anything: ladder length and index are brought inside [1, 8] and the ladder as
    //  doubles, before any conversion -- NaN fails every comparison and gives the lower end)
    const double raw_n = S[PINN_CAUSAL_N_EPS], raw_index = S[PINN_CAUSAL_INDEX];
    const int n_eps = raw_n >= 1.0 ? (raw_n <= (double)PINN_CAUSAL_MAX_EPS ? (int)raw_n : PINN_CAUSAL_MAX_EPS) : 1;
    const int index = raw_index >= 1.0 ? (raw_index <= (double)(n_eps - 1) ? (int)raw_index : n_eps - 1) : 0;
    const double eps = S[PINN_CAUSAL_EPS + index];
    double prefix = 0.0, total = 0.0, w_min = 1.0;
    for (int k = 0; k < PINN_CAUSAL_MAX_BINS; ++k) {
        double n_k = 0.0, L_k = 0.0, w_k = 0.0;
        if (k < M) {
            n_k = tot_cnt[k];
            L_k = n_k > 0.0 ? tot_sum[k] / n_k : 0.0;
            // eps == 0: exactly one, also over a prefix that overflowed (0 * inf is no number); else exp(-inf) = 0, never NaN
            w_k = eps == 0.0 ? 1.0 : exp(-(eps * prefix));
            w_min = fmin(w_min, w_k);
            total += tot_sum[k];
            prefix += L_k;
            if (A.bin_weight_out) A.bin_weight_out[k] = (float)w_k;
        }
        S[PINN_CAUSAL_NK + k] = n_k; S[PINN_CAUSAL_LK + k] = L_k; S[PINN_CAUSAL_WK + k] = w_k;
    }
    const double mean_sq = total / (double)A.n;
    S[PINN_CAUSAL_EPS_USED] = eps;
    S[PINN_CAUSAL_MEAN_SQ] = mean_sq;
    S[PINN_CAUSAL_CALLS] += 1.0;
    if (tot_bad[0]) S[PINN_CAUSAL_BAD] = 1.0;
    if (A.eps_out) *A.eps_out = (float)eps;
    if (A.mean_sq_out) *A.mean_sq_out = (float)mean_sq;
    // the ladder: the NEXT call's rung (w_k <= 1, so delta >= 1 never advances)
    if (A.update && w_min > S[PINN_CAUSAL_DELTA]) {
        if (index + 1 < n_eps) S[PINN_CAUSAL_INDEX] = (double)(index + 1);
        else S[PINN_CAUSAL_CONVERGED] = 1.0;
    }
}

PINN_GLOBAL void PINN_LAUNCH_BOUNDS(PINN_CAUSAL_THREADS) pinn_causal_apply_kernel(PinnCausalArgs A) {
    const long long i = (long long)PINN_BID * PINN_CAUSAL_THREADS + PINN_TID;
    if (i >= A.n) return;
    A.w_out[i] = (float)A.state[PINN_CAUSAL_WK + pinn_causal_bin(A.t[i * A.t_stride], A.t_lo, A.t_hi, A.M)];
}
