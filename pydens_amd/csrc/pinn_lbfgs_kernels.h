// pinn_lbfgs_kernels.h -- the L-BFGS direction of torch.optim.LBFGS on the flat parameter buffer, in the Gram form; included by
// pinn_abi.cpp only (pinn_lbfgs_direction of include/pinn.h: three launches per inner iteration, whatever the history size).
//
// torch runs the two-loop recursion as 4 m dependent passes over p-vectors (a dot and an axpy per stored pair and loop). Every vector of
// that recursion is a combination of g and the stored s_j, y_j, so the recursion only ever needs the SCALARS s_i.y_j, y_i.y_j, s_i.g and
// y_i.g: the m x m Gram matrices are kept from iteration to iteration (a new pair replaces one row and one column), the products with
// the new pair and the new gradient come from ONE pass over the history, the recursion runs on the scalars, and the direction is ONE
// combination d = c_g g + sum_j a_j s_j + sum_j b_j y_j:
//   pinn_lbfgs_dots_kernel      grid over 4096-entry slices of p: every workgroup reads its slice of g, of the new pair (s = t d, y = g - g_prev: formed
//                               on the fly in fp32, as torch forms them) and of every live s_j, y_j once; products of two fp32 values are
//                               exact in fp64 and are summed in fp64; one row of partial sums per workgroup
//   pinn_lbfgs_finalize_kernel  one workgroup: rows summed in ascending order, torch's stopping rules and curvature test, ring and Gram
//                               update, both loops of the recursion in fp64 (one wave; the s.y matrix staged in LDS), coefficients and
//                               scalars to the control block
//   pinn_lbfgs_combine_kernel   stores the accepted pair into the ring, d (one fp64 sum per entry, one rounding), g_prev <- g and -- without
//                               a line search -- params += t d
// No atomics, no waits between workgroups: launch boundaries order the passes, every sum has a fixed order (bit-repeatable).
// Entries with mask == 0 (padding, frozen parameters, the loss slot, unreached scalars) enter no product and are never written.
#pragma once
#include "pinn_port.h"

#define PINN_LBFGS_GLOBAL PINN_GLOBAL
#ifndef PINN_LBFGS_MAX_HISTORY
#define PINN_LBFGS_MAX_HISTORY 128      // (include/pinn.h) the s.y matrix of the recursion must fit the LDS of one workgroup: 128 x 128 doubles = 128 KB
#endif
#define PINN_LBFGS_THREADS 256
#define PINN_LBFGS_SLICE 1024           // entries per sweep of a workgroup: one 16-byte piece per thread (the combine pass: one sweep)
#define PINN_LBFGS_PIECES 4             // sweeps per workgroup of the dots pass
#define PINN_LBFGS_DOTS_SLICE (PINN_LBFGS_PIECES * PINN_LBFGS_SLICE)

// the control block (doubles; integers are stored as doubles, exactly): pinn_lbfgs_ctrl_bytes(m) = (16 + 2 m + 2 m m) * 8
#define PINN_LBFGS_COUNT 0              // live pairs in the ring
#define PINN_LBFGS_RING_HEAD 1          // physical slot of the oldest pair
#define PINN_LBFGS_N_ITER 2             // directions computed so far (torch's state['n_iter'])
#define PINN_LBFGS_H_DIAG 3
#define PINN_LBFGS_T 4                  // step length that goes with the direction just computed
#define PINN_LBFGS_GTD 5                // g . d of the direction just computed
#define PINN_LBFGS_GMAX 6               // max |g|
#define PINN_LBFGS_SMAX 7               // max |t d| of the step that led here
#define PINN_LBFGS_LOSS 8               // the loss slot of g
#define PINN_LBFGS_PREV_LOSS 9          // the loss at the previous direction
#define PINN_LBFGS_YS 10
#define PINN_LBFGS_YY 11
#define PINN_LBFGS_STOP 12              // 0 go on, 1 max|g| <= tolerance_grad, 2 max|t d| <= tolerance_change, 3 |loss - prev| < tolerance_change
                                        // (1 - 3: nothing else was touched), 4 g . d > -tolerance_change (direction stored, no step taken)
#define PINN_LBFGS_PUSHED 13            // the last pair passed the curvature test ys > 1e-10
#define PINN_LBFGS_SLOT 14              // ... into this physical slot
#define PINN_LBFGS_CG 15                // coefficient of g in d
#define PINN_LBFGS_CTRL_HEAD 16         // then a[m] (of s_j), b[m] (of y_j) by physical slot, then s.y [m][m] and y.y [m][m]
// a row of partial sums: 5 per physical slot j (s_j.g, y_j.g, s_j.y_new, y_j.s_new, y_j.y_new), then these eight
#define PINN_LBFGS_ROW_TAIL 8           // s_new.g, y_new.g, s_new.y_new, y_new.y_new, g.g, sum |g|, max |g|, max |s_new|

struct PinnLbfgsArgs {
    float* params; const float* g; float* prev_g; float* d; float* S; float* Y; const unsigned char* mask;
    long long n, ld;                    // entries; row stride of the rings (a multiple of 4, >= n)
    int m, mode, apply, off_loss;
    float t;                            // step length of the step that led to g (s_new = t d)
    double lr, tol_grad, tol_change;
    double* ctrl; double* rows; int n_rows;
};

// entries i .. i + 3 of a 16-byte aligned array of n floats (i % 4 == 0, i < n): one 16-byte load, the ragged end entry by entry
PINN_DEVICE f32x4 pinn_lbfgs_ld4(const float* p, long long i, long long n) {
    if (i + 4 <= n) return *reinterpret_cast<const f32x4*>(p + i);
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int e = 0; e < 4; ++e) if (i + e < n) v[e] = p[i + e];
    return v;
}
PINN_DEVICE void pinn_lbfgs_live4(const unsigned char* mask, long long i, long long n, bool (&live)[4]) {
    for (int e = 0; e < 4; ++e) live[e] = i + e < n && (!mask || mask[i + e] != 0);
}
PINN_DEVICE void pinn_lbfgs_st4(float* p, long long i, f32x4 v, const bool (&live)[4]) {
    if (live[0] && live[1] && live[2] && live[3]) { *reinterpret_cast<f32x4*>(p + i) = v; return; }
    for (int e = 0; e < 4; ++e) if (live[e]) p[i + e] = v[e];
}
// sum over the wave in double, the same value in every lane (DPP within the 16-lane rows, then the four rows in order)
PINN_DEVICE double pinn_lbfgs_wave_sum(double v) { return pinn_rows_total_f64(pinn_row_sum16_f64(v)); }
PINN_DEVICE float pinn_lbfgs_wave_max(float v) {
    for (int mask = 1; mask < 64; mask <<= 1) v = fmaxf(v, pinn_shfl_xor(v, mask));
    return v;
}

PINN_LBFGS_GLOBAL void PINN_LAUNCH_BOUNDS(PINN_LBFGS_THREADS) pinn_lbfgs_dots_kernel(PinnLbfgsArgs A) {
    PINN_SMEM(smem);
    double* part = reinterpret_cast<double*>(smem);              // [4 waves][row]
    constexpr int U = PINN_LBFGS_PIECES;
    const int tid = PINN_TID, wave = tid >> 6, lane = tid & 63;
    const int m = A.m, tail = 5 * m, rowlen = tail + PINN_LBFGS_ROW_TAIL;
    const int count = (int)A.ctrl[PINN_LBFGS_COUNT];
    const bool pair = A.ctrl[PINN_LBFGS_N_ITER] > 0.0;            // a previous direction and gradient exist
    // piece u of this thread: consecutive threads on consecutive 16-byte pieces, U such sweeps of 1024 entries per workgroup -- the
    // cross-lane sums below cost the same per stored pair whatever U is, so U pieces per thread divide their share of the pass by U
    const long long base = (long long)PINN_BID * PINN_LBFGS_DOTS_SLICE + 4 * tid;
    f32x4 g[U], sn[U], yn[U];
    unsigned live_bits = 0;                                       // bit 4 u + e: entry e of piece u takes part
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const long long i0 = base + (long long)u * PINN_LBFGS_SLICE;
        g[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; sn[u] = g[u]; yn[u] = g[u];
        if (i0 < A.n) {
            bool live[4];
            pinn_lbfgs_live4(A.mask, i0, A.n, live);
            const f32x4 gv = pinn_lbfgs_ld4(A.g, i0, A.n);
            f32x4 dv = {0.0f, 0.0f, 0.0f, 0.0f}, pg = dv;
            if (pair) { dv = pinn_lbfgs_ld4(A.d, i0, A.n); pg = pinn_lbfgs_ld4(A.prev_g, i0, A.n); }
            for (int e = 0; e < 4; ++e) {
                sn[u][e] = live[e] && pair ? A.t * dv[e] : 0.0f;
                yn[u][e] = live[e] && pair ? gv[e] - pg[e] : 0.0f;
                g[u][e] = live[e] ? gv[e] : 0.0f;
                live_bits |= live[e] ? 1u << (4 * u + e) : 0u;
            }
        }
    }
    double* mine = part + wave * rowlen;
    for (int j = 0; j < count; ++j) {
        double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long i0 = base + (long long)u * PINN_LBFGS_SLICE;
            if (i0 >= A.n) continue;
            // (rows are ld long, ld % 4 == 0, i0 < n <= ld: always a whole piece. Entries that take no part -- masked, or between n and ld --
            //  are never written by the combine pass and may hold anything: zero is selected here, not multiplied in)
            const f32x4 sr = *reinterpret_cast<const f32x4*>(A.S + (size_t)j * A.ld + i0);
            const f32x4 yr = *reinterpret_cast<const f32x4*>(A.Y + (size_t)j * A.ld + i0);
            for (int e = 0; e < 4; ++e) {
                const bool on = (live_bits >> (4 * u + e)) & 1u;
                const double s = on ? (double)sr[e] : 0.0, y = on ? (double)yr[e] : 0.0;
                v[0] += s * (double)g[u][e];
                v[1] += y * (double)g[u][e];
                v[2] += s * (double)yn[u][e];
                v[3] += y * (double)sn[u][e];
                v[4] += y * (double)yn[u][e];
            }
        }
        for (int k = 0; k < 5; ++k) {
            const double w = pinn_lbfgs_wave_sum(v[k]);
            if (lane == 0) mine[5 * j + k] = w;
        }
    }
    {
        double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        float gmax = 0.0f, smax = 0.0f;
#pragma unroll
        for (int u = 0; u < U; ++u)
            for (int e = 0; e < 4; ++e) {
                v[0] += (double)sn[u][e] * (double)g[u][e];
                v[1] += (double)yn[u][e] * (double)g[u][e];
                v[2] += (double)sn[u][e] * (double)yn[u][e];
                v[3] += (double)yn[u][e] * (double)yn[u][e];
                v[4] += (double)g[u][e] * (double)g[u][e];
                v[5] += (double)fabsf(g[u][e]);
                gmax = fmaxf(gmax, fabsf(g[u][e]));
                smax = fmaxf(smax, fabsf(sn[u][e]));
            }
        for (int k = 0; k < 6; ++k) {
            const double w = pinn_lbfgs_wave_sum(v[k]);
            if (lane == 0) mine[tail + k] = w;
        }
        gmax = pinn_lbfgs_wave_max(gmax);
        smax = pinn_lbfgs_wave_max(smax);
        if (lane == 0) { mine[tail + 6] = (double)gmax; mine[tail + 7] = (double)smax; }
    }
    PINN_SYNC();
    double* row = A.rows + (size_t)PINN_BID * rowlen;
    for (int idx = tid; idx < rowlen; idx += PINN_LBFGS_THREADS) {
        double w = 0.0;
        if (idx >= tail || idx < 5 * count) {
            const double w0 = part[idx], w1 = part[rowlen + idx], w2 = part[2 * rowlen + idx], w3 = part[3 * rowlen + idx];
            w = idx >= tail + 6 ? fmax(fmax(w0, w1), fmax(w2, w3)) : ((w0 + w1) + w2) + w3;
        }
        row[idx] = w;
    }
}

PINN_LBFGS_GLOBAL void PINN_LAUNCH_BOUNDS(PINN_LBFGS_THREADS) pinn_lbfgs_finalize_kernel(PinnLbfgsArgs A) {
    PINN_SMEM(smem);
    const int tid = PINN_TID, m = A.m, tail = 5 * m, rowlen = tail + PINN_LBFGS_ROW_TAIL;
    double* tot = reinterpret_cast<double*>(smem);      // [rowlen]
    double* sg = tot + rowlen;                          // s_c . g, y_c . g; from here on by AGE c (0 the oldest pair)
    double* yg = sg + m;
    double* V = yg + m;                                 // s_c . q of the first loop
    double* W = V + m;                                  // y_c . r of the second
    double* AL = W + m;
    double* RY = AL + m;                                // coefficients of y_c and s_c in the direction
    double* RS = RY + m;
    double* SYc = RS + m;                               // s_c . y_k, [m][m]
    double* C = A.ctrl;
    double* SY = C + PINN_LBFGS_CTRL_HEAD + 2 * m;      // the kept matrices, by physical slot
    double* YY = SY + (size_t)m * m;
    // the rows in ascending order
    for (int idx = tid; idx < rowlen; idx += PINN_LBFGS_THREADS) {
        double acc = 0.0;
        for (int r = 0; r < A.n_rows; ++r) {
            const double x = A.rows[(size_t)r * rowlen + idx];
            acc = idx >= tail + 6 ? fmax(acc, x) : acc + x;
        }
        tot[idx] = acc;
    }
    int count = (int)C[PINN_LBFGS_COUNT], head = (int)C[PINN_LBFGS_RING_HEAD];
    const double n_iter = C[PINN_LBFGS_N_ITER], prev_loss = C[PINN_LBFGS_PREV_LOSS];
    double H = C[PINN_LBFGS_H_DIAG];
    const double loss = (double)A.g[A.off_loss];
    PINN_SYNC();                                        // (every thread holds what it needs of the block: thread 0 may write it now)
    const double gmax = tot[tail + 6], smax = tot[tail + 7];
    // torch.optim.LBFGS.step: the optimality test behind every evaluation; behind an evaluation inside the loop also lack of progress
    int stop = 0;
    if (gmax <= A.tol_grad) stop = 1;
    else if (A.mode == 1 && smax <= A.tol_change) stop = 2;
    else if (A.mode == 1 && fabs(loss - prev_loss) < A.tol_change) stop = 3;
    if (stop) {
        if (tid == 0) {
            C[PINN_LBFGS_GMAX] = gmax; C[PINN_LBFGS_SMAX] = smax; C[PINN_LBFGS_LOSS] = loss;
            C[PINN_LBFGS_STOP] = (double)stop; C[PINN_LBFGS_PUSHED] = 0.0;
        }
        return;
    }
    const bool fresh = n_iter == 0.0;
    const double ys = tot[tail + 2], yy = tot[tail + 3];
    const int live_before = fresh ? 0 : count;
    int pushed = 0, slot = -1;
    if (fresh) { count = 0; head = 0; H = 1.0; }
    else if (ys > 1e-10) {                              // torch's curvature test: else the pair is dropped, ring, matrices and H_diag stay
        pushed = 1;
        if (count < m) { slot = count; count += 1; }
        else { slot = head; head = (head + 1) % m; }
        H = ys / yy;
    }
    if (pushed) {
        for (int j = tid; j < live_before; j += PINN_LBFGS_THREADS) {
            if (j == slot) continue;                    // (at capacity: the evicted pair's products)
            SY[(size_t)j * m + slot] = tot[5 * j + 2];
            SY[(size_t)slot * m + j] = tot[5 * j + 3];
            YY[(size_t)j * m + slot] = tot[5 * j + 4];
            YY[(size_t)slot * m + j] = tot[5 * j + 4];
        }
        if (tid == 0) { SY[(size_t)slot * m + slot] = ys; YY[(size_t)slot * m + slot] = yy; }
    }
    const int n = count;
    for (int c = tid; c < n; c += PINN_LBFGS_THREADS) {
        const int pc = (head + c) % m;
        sg[c] = pushed && pc == slot ? tot[tail + 0] : tot[5 * pc + 0];
        yg[c] = pushed && pc == slot ? tot[tail + 1] : tot[5 * pc + 1];
    }
    PINN_SYNC();                                        // (the matrices' new row and column are in place)
    for (int idx = tid; idx < n * n; idx += PINN_LBFGS_THREADS) {
        const int c = idx / n, k = idx % n;
        SYc[c * m + k] = SY[(size_t)((head + c) % m) * m + (head + k) % m];
    }
    for (int c = tid; c < n; c += PINN_LBFGS_THREADS) V[c] = -sg[c];
    PINN_SYNC();
    // q = -g; newest to oldest: al_k = (s_k . q) / (s_k . y_k), q -= al_k y_k  --  kept as V[c] = s_c . q for the pairs still to come
    if (tid < 64) {
        for (int k = n - 1; k >= 0; --k) {
            PINN_WAVE_SYNC();
            const double al = V[k] / SYc[k * m + k];
            if (tid == 0) AL[k] = al;
            for (int c = tid; c < k; c += 64) V[c] -= al * SYc[c * m + k];
        }
    }
    PINN_SYNC();
    // r = H q = -H g - H sum_k al_k y_k;  W[c] = y_c . r
    const double cg = -H;
    for (int c = tid; c < n; c += PINN_LBFGS_THREADS) {
        const int pc = (head + c) % m;
        double w = cg * yg[c];
        for (int k = 0; k < n; ++k) w -= H * AL[k] * YY[(size_t)pc * m + (head + k) % m];
        W[c] = w;
        RY[c] = -H * AL[c];
    }
    PINN_SYNC();
    // oldest to newest: be_i = (y_i . r) / (s_i . y_i), r += (al_i - be_i) s_i
    if (tid < 64) {
        for (int i = 0; i < n; ++i) {
            PINN_WAVE_SYNC();
            const double coef = AL[i] - W[i] / SYc[i * m + i];
            if (tid == 0) RS[i] = coef;
            for (int c = tid; c < n; c += 64) if (c > i) W[c] += coef * SYc[i * m + c];
        }
    }
    PINN_SYNC();
    for (int j = tid; j < m; j += PINN_LBFGS_THREADS) {
        const int c = (j - head + m) % m;               // age of physical slot j
        const bool alive = c < n;
        C[PINN_LBFGS_CTRL_HEAD + j] = alive ? RS[c] : 0.0;
        C[PINN_LBFGS_CTRL_HEAD + m + j] = alive ? RY[c] : 0.0;
    }
    if (tid == 0) {
        double gtd = cg * tot[tail + 4];
        for (int c = 0; c < n; ++c) gtd += RS[c] * sg[c] + RY[c] * yg[c];
        // the first direction of a fresh state: t = min(1, 1 / |g|_1) lr (torch forms the quotient in fp32), lr from then on
        double t = A.lr;
        if (fresh) t = (double)fminf(1.0f, 1.0f / (float)tot[tail + 5]) * A.lr;
        C[PINN_LBFGS_COUNT] = (double)count; C[PINN_LBFGS_RING_HEAD] = (double)head; C[PINN_LBFGS_N_ITER] = n_iter + 1.0;
        C[PINN_LBFGS_H_DIAG] = H; C[PINN_LBFGS_T] = t; C[PINN_LBFGS_GTD] = gtd;
        C[PINN_LBFGS_GMAX] = gmax; C[PINN_LBFGS_SMAX] = smax; C[PINN_LBFGS_LOSS] = loss; C[PINN_LBFGS_PREV_LOSS] = loss;
        C[PINN_LBFGS_YS] = ys; C[PINN_LBFGS_YY] = yy;
        C[PINN_LBFGS_STOP] = gtd > -A.tol_change ? 4.0 : 0.0;
        C[PINN_LBFGS_PUSHED] = (double)pushed; C[PINN_LBFGS_SLOT] = (double)slot; C[PINN_LBFGS_CG] = cg;
    }
}

PINN_LBFGS_GLOBAL void PINN_LAUNCH_BOUNDS(PINN_LBFGS_THREADS) pinn_lbfgs_combine_kernel(PinnLbfgsArgs A) {
    const long long i0 = (long long)PINN_BID * PINN_LBFGS_SLICE + 4 * PINN_TID;
    if (i0 >= A.n) return;
    const double* C = A.ctrl;
    const int stop = (int)C[PINN_LBFGS_STOP];
    if (stop >= 1 && stop <= 3) return;                 // the step ended in front of this direction: nothing moves
    const int m = A.m, count = (int)C[PINN_LBFGS_COUNT], slot = (int)C[PINN_LBFGS_SLOT];
    const bool pushed = C[PINN_LBFGS_PUSHED] != 0.0;
    const double cg = C[PINN_LBFGS_CG];
    const float t_new = (float)C[PINN_LBFGS_T];
    const double* a = C + PINN_LBFGS_CTRL_HEAD;
    const double* b = a + m;
    bool live[4];
    pinn_lbfgs_live4(A.mask, i0, A.n, live);
    const f32x4 g = pinn_lbfgs_ld4(A.g, i0, A.n);
    f32x4 sn = {0.0f, 0.0f, 0.0f, 0.0f}, yn = sn;
    if (pushed) {                                       // the pair as the dots pass formed it
        const f32x4 dv = pinn_lbfgs_ld4(A.d, i0, A.n), pg = pinn_lbfgs_ld4(A.prev_g, i0, A.n);
        for (int e = 0; e < 4; ++e) { sn[e] = A.t * dv[e]; yn[e] = g[e] - pg[e]; }
    }
    double acc[4];
    for (int e = 0; e < 4; ++e) acc[e] = cg * (double)g[e];
    for (int j = 0; j < count; ++j) {
        f32x4 s = sn, y = yn;
        if (!(pushed && j == slot)) {
            s = *reinterpret_cast<const f32x4*>(A.S + (size_t)j * A.ld + i0);
            y = *reinterpret_cast<const f32x4*>(A.Y + (size_t)j * A.ld + i0);
        }
        const double aj = a[j], bj = b[j];
        for (int e = 0; e < 4; ++e) acc[e] += aj * (double)s[e] + bj * (double)y[e];
    }
    f32x4 dn;
    for (int e = 0; e < 4; ++e) dn[e] = (float)acc[e];
    if (pushed) {
        pinn_lbfgs_st4(A.S + (size_t)slot * A.ld, i0, sn, live);
        pinn_lbfgs_st4(A.Y + (size_t)slot * A.ld, i0, yn, live);
    }
    pinn_lbfgs_st4(A.d, i0, dn, live);
    pinn_lbfgs_st4(A.prev_g, i0, g, live);
    if (A.apply && stop == 0) {
        f32x4 p = pinn_lbfgs_ld4(A.params, i0, A.n);
        for (int e = 0; e < 4; ++e) p[e] = p[e] + t_new * dn[e];
        pinn_lbfgs_st4(A.params, i0, p, live);
    }
}
