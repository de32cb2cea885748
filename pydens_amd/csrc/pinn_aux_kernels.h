// pinn_aux_kernels.h -- small non-template kernels (gradient reduction, Adam); included by pinn_abi.cpp only.
#pragma once
// (the small kernels of this header are launched from pinn_abi.cpp only; the per-width units of widths <= 32 include the header for the
//  structs and device functions pinn_fit_kernel.h shares with them -- there the kernels get internal linkage and are dropped unused)
#ifdef PINN_AUX_KERNELS_STATIC
#define PINN_AUX_GLOBAL static PINN_GLOBAL
#else
#define PINN_AUX_GLOBAL PINN_GLOBAL
#endif

#include "pinn_port.h"
#include "pinn_kernel.h"

// ------------------------------------------------------------------------------------------------------------
// x-only pre-pass: evaluates the source terms / variable coefficients of the residual for every point once,
// outside the tile kernel (one thread per point, registers in private memory; N * a-few-ops, microseconds).
// ------------------------------------------------------------------------------------------------------------
PINN_AUX_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_aux_kernel(const float* xs, long long n, int d, pinn_program_t pg, PinnPreConsts c64, float* aux) {
    const long long i = (long long)PINN_BID * 256 + PINN_TID;
    if (i >= n) return;
    double regs[PINN_MAX_REGS];                 // private (scratch): the program indexes it at run time; fp64 like the in-kernel form
    pinn_prepass_point(pg, c64, xs + i * d, d, aux, n, i, regs, 1);
}

// ------------------------------------------------------------------------------------------------------------
// sum of the per-workgroup partial gradients (fixed order => deterministic; pinn_reduce_kernel further down); optionally the
// optimizer update of the block's parameters right behind it (single-rank steps: no all-reduce in between, two launches less).
// ------------------------------------------------------------------------------------------------------------
// bias corrections in double like torch's Python-side scalars (1 - beta ** step); the host computes them when it knows
// the step (two double pow per thread in the tail of every block otherwise)
PINN_HOST_DEVICE inline void pinn_adam_scalars(double t, float lr, float b1, float b2, float* step_size, float* bc2_sqrt) {
    const double bc1 = 1.0 - pow((double)b1, t);
    const double bc2 = 1.0 - pow((double)b2, t);
    *step_size = (float)((double)lr / bc1);
    *bc2_sqrt = (float)sqrt(bc2);
}

// (the arithmetic of one Adam update on operands already in registers: ONE expression tree for every caller, so that every path
//  rounds -- and contracts multiply-adds -- the same way)
PINN_DEVICE void pinn_adam_apply(float* params, float* m, float* v, long long i, float gi, float m_old, float v_old, float p_old,
                                 float step_size, float bc2_sqrt, float b1, float b2, float eps) {
    const float mi = m_old + (1.0f - b1) * (gi - m_old);     // exp_avg.lerp_(grad, 1 - beta1)
    const float vi = fmaf(1.0f - b2, gi * gi, b2 * v_old);   // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    params[i] = p_old - step_size * (mi / denom);
}

// ------------------------------------------------------------------------------------------------------------
// The optimizer family (include/pinn.h pinn_optim_t): the `_single_tensor_*` arithmetic of torch.optim.{Adam, AdamW, SGD, RMSprop},
// one expression tree per rule, shared by every caller (pinn_reduce_kernel's tail, pinn_optim_kernel, sweep (d) of pinn_fit_kernel).
// The rule is a wave-uniform code in the kernel arguments, like the criterion of the point stage. What torch computes once per
// step as a Python double (1 - lr * weight_decay, 1 - dampening, 1 - alpha) is derived on the host (pinn_abi.cpp optim_prepare).
// ------------------------------------------------------------------------------------------------------------
struct PinnOptK {
    int rule, nesterov, centered, pad;
    float lr, b1, b2, eps, wd, momentum, alpha;
    float decay;            // AdamW: 1 - lr * weight_decay
    float undamp;           // SGD: 1 - dampening
    float one_m_alpha;      // RMSprop: 1 - alpha
};

// m / v: the two state arrays (exp_avg | momentum_buffer | grad_avg, exp_avg_sq | square_avg); `first`: step 1 of the optimizer (SGD: no
// momentum buffer yet). A rule writes only the state it owns.
// lr / decay: the learning rate of THIS step (SGD, RMSprop) and AdamW's 1 - lr * weight_decay; o.lr / o.decay for a constant rate, the
// iteration's entries of the control block under a schedule (PinnFitCtrl::lr / ::decay). Adam's and AdamW's rate rides in step_size.
PINN_DEVICE void pinn_optim_apply(const PinnOptK& o, float* params, float* m, float* v, long long i, float gi, float m_old, float v_old,
                                  float p_old, float lr, float decay, float step_size, float bc2_sqrt, bool first) {
    if (o.rule == PINN_OPT_ADAM && o.wd == 0.0f) {          // (plain Adam: the arithmetic the library had before the family existed)
        pinn_adam_apply(params, m, v, i, gi, m_old, v_old, p_old, step_size, bc2_sqrt, o.b1, o.b2, o.eps);
        return;
    }
    if (o.rule == PINN_OPT_ADAMW) p_old *= decay;                         // param.mul_(1 - lr * weight_decay)
    else if (o.wd != 0.0f) gi = fmaf(o.wd, p_old, gi);                      // grad = grad.add(param, alpha=weight_decay)
    if (o.rule == PINN_OPT_ADAM || o.rule == PINN_OPT_ADAMW) {
        pinn_adam_apply(params, m, v, i, gi, m_old, v_old, p_old, step_size, bc2_sqrt, o.b1, o.b2, o.eps);
    } else if (o.rule == PINN_OPT_SGD) {
        if (o.momentum != 0.0f) {
            // buf = clone(grad) on the first step, else buf.mul_(momentum).add_(grad, alpha=1 - dampening)
            const float buf = first ? gi : fmaf(o.undamp, gi, o.momentum * m_old);
            m[i] = buf;
            gi = o.nesterov ? fmaf(o.momentum, buf, gi) : buf;              // grad.add(buf, alpha=momentum)
        }
        params[i] = p_old - lr * gi;                                        // param.add_(grad, alpha=-lr)
    } else {                                                                // PINN_OPT_RMSPROP
        const float sq = fmaf(o.one_m_alpha, gi * gi, o.alpha * v_old);     // square_avg.mul_(alpha).addcmul_(grad, grad, value=1 - alpha)
        v[i] = sq;
        float avg;
        if (o.centered) {
            const float ga = m_old + o.one_m_alpha * (gi - m_old);          // grad_avg.lerp_(grad, 1 - alpha)
            m[i] = ga;
            avg = sqrtf(fmaf(-ga, ga, sq));                                 // square_avg.addcmul(grad_avg, grad_avg, value=-1).sqrt_()
        } else {
            avg = sqrtf(sq);
        }
        avg += o.eps;
        if (o.momentum > 0.0f) {
            const float buf = fmaf(o.momentum, m_old, gi / avg);            // buf.mul_(momentum).addcdiv_(grad, avg)
            m[i] = buf;
            params[i] = p_old - lr * buf;
        } else {
            params[i] = p_old - lr * (gi / avg);                            // param.addcdiv_(grad, avg, value=-lr)
        }
    }
}

PINN_DEVICE void pinn_optim_update(const PinnOptK& o, float* params, float gi, float* m, float* v, long long i, float lr, float decay,
                                   float step_size, float bc2_sqrt, bool first) {
    pinn_optim_apply(o, params, m, v, i, gi, m[i], v[i], params[i], lr, decay, step_size, bc2_sqrt, first);
}

// ------------------------------------------------------------------------------------------------------------
// Collocation sampler on the device: replaces the host-side draws of reference model_torch.py:430-434 (`torch.rand`
// per input column, or `sampler.sample(batch_size)` of a batchflow NumpySampler product `a & b & ...`).
// Counter-based generator Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
// SC'11; constants of the Random123 library): no state in memory, one launch per batch whatever the number of columns,
// every (seed, call, point, column) addresses its own random word, so a batch does not depend on the launch geometry.
// oracle/philox.py restates it in numpy (pinned to the Random123 known-answer vectors); tests compare bit for bit.
// ------------------------------------------------------------------------------------------------------------
struct PinnSampleSpec {
    int d;
    int kind[PINN_MAX_INPUTS];      // PINN_SAMPLE_UNIFORM / _NORMAL / _CONST
    float a[PINN_MAX_INPUTS], b[PINN_MAX_INPUTS];
};

PINN_DEVICE void pinn_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                    unsigned (&out)[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// products / sums that must round like the numpy oracle: separately, never contracted into a fused multiply-add
// (hipcc's __fmul_rn / __fadd_rn are plain operators and do get contracted, hence the pragma in the function bodies)
PINN_DEVICE float pinn_mul_then_add(float a, float w, float u) {
#pragma clang fp contract(off)
    const float t = w * u;
    return a + t;
}

// the d columns of point i of batch `call` (what one thread of pinn_sample_kernel does; also the tail of pinn_reduce_kernel when a fit
// chunk lets the reduction of iteration k draw the batch of iteration k + 1: one launch less per iteration)
PINN_DEVICE void pinn_sample_point(float* xs, long long i, const PinnSampleSpec& spec, unsigned k0, unsigned k1, unsigned call_lo,
                                   unsigned call_hi) {
    const unsigned i_lo = (unsigned)((unsigned long long)i & 0xffffffffull), i_hi = (unsigned)((unsigned long long)i >> 32);
    unsigned r[4] = {0u, 0u, 0u, 0u};
    for (int c = 0; c < spec.d; ++c) {
        if ((c & 3) == 0) pinn_philox4x32_10(i_lo, i_hi, call_lo, (call_hi & 0x0fffffffu) | ((unsigned)(c >> 2) << 28), k0, k1, r);
        const float a = spec.a[c], b = spec.b[c];
        float v = a;
        if (spec.kind[c] == PINN_SAMPLE_UNIFORM) {
            const float u = (float)(r[c & 3] >> 8) * 5.9604644775390625e-8f;              // 24 bits -> [0, 1)
            v = pinn_mul_then_add(a, b - a, u);
        } else if (spec.kind[c] == PINN_SAMPLE_NORMAL) {
            unsigned q[4];
            pinn_philox4x32_10(i_lo, i_hi, call_lo, (call_hi & 0x0fffffffu) | ((unsigned)(8 + c) << 28), k0, k1, q);
            const float u1 = (float)((q[0] >> 8) + 1u) * 5.9604644775390625e-8f;          // (0, 1]
            const float u2 = (float)(q[1] >> 8) * 5.9604644775390625e-8f;
            const float z = sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
            v = pinn_mul_then_add(a, b, z);
        }
        xs[i * spec.d + c] = v;
    }
}
// what the reduction of a fit iteration needs to draw the NEXT iteration's batch (n == 0: nothing to draw)
struct PinnNextBatch {
    float* xs; long long n; PinnSampleSpec spec; unsigned k0, k1; unsigned long long call;
};

// Replayable launch graph of a chunk of fit iterations (pinn_fit_steps, batches of a few thousand points: the latency regime): what
// changes from one iteration to the next -- the Philox batch counter, the Adam step with its bias corrections, the slot of the loss
// history -- is read from this block in device memory, indexed by the iteration number k that is baked into the graph's kernel nodes;
// the block itself is rewritten (pinn_fit_ctrl_kernel, an ordinary launch in front of the graph) for every chunk.
#define PINN_FIT_CHUNK_MAX 128
struct PinnFitCtrl {
    unsigned long long call_index0;     // Philox batch counter of iteration 0 of the chunk
    float* loss_base;                   // entry 0 of the chunk in the loss history
    int step0, pad;                     // Adam step number of iteration 0
    unsigned k0, k1;                    // Philox key of the fit call's sampler (round 5: the key changes per fit call; in the control
                                        // block, not baked into the graph's nodes, a recorded chunk survives across fit calls)
    float step_size[PINN_FIT_CHUNK_MAX], bc2_sqrt[PINN_FIT_CHUNK_MAX];      // pinn_adam_scalars per iteration (computed on the host in
                                                                             // double, as for the eager loop: bit-identical updates)
    // the learning rate of every iteration (lr_steps of pinn_fit_steps; a constant rate fills both arrays with one value): lr[k] is what
    // SGD and RMSprop multiply with, decay[k] AdamW's 1 - lr_k * weight_decay formed on the host like PinnOptK::decay; Adam's and AdamW's
    // rate is in step_size[k]. A recorded chunk reads all of them here, so it replays under any rate.
    float lr[PINN_FIT_CHUNK_MAX], decay[PINN_FIT_CHUNK_MAX];
};
struct PinnFitCtrlArgs { PinnFitCtrl c; };
// (the block travels to pinn_fit_ctrl_kernel BY VALUE, next to the destination pointer: kernel arguments end at 4 KB)
static_assert(sizeof(PinnFitCtrlArgs) + sizeof(PinnFitCtrl*) <= 4096, "the control block no longer fits the kernel arguments of ONE launch");
PINN_AUX_GLOBAL void PINN_LAUNCH_BOUNDS(128) pinn_fit_ctrl_kernel(PinnFitCtrl* dst, PinnFitCtrlArgs a) {
    const int t = PINN_TID;
    if (t == 0) { dst->call_index0 = a.c.call_index0; dst->loss_base = a.c.loss_base; dst->step0 = a.c.step0; dst->pad = 0;
                  dst->k0 = a.c.k0; dst->k1 = a.c.k1; }
    if (t < PINN_FIT_CHUNK_MAX) { dst->step_size[t] = a.c.step_size[t]; dst->bc2_sqrt[t] = a.c.bc2_sqrt[t];
                                  dst->lr[t] = a.c.lr[t]; dst->decay[t] = a.c.decay[t]; }
}

// ------------------------------------------------------------------------------------------------------------
// The reduction launch. A block is CH = 32 chunks of workgroup rows x LC lanes per chunk; a lane owns VW consecutive parameters of its
// chunk's rows and loads them as ONE piece per row: VW = 4, a 16-byte piece (pinn_reduce_kernel, the form the launcher takes whenever the
// rows allow it), or VW = 1, one dword (pinn_reduce_scalar_kernel: the form this kernel had through round 7, kept for rows that are not
// 16-byte aligned). The block covers PB = LC * VW parameters. For every parameter the order of the sum is the same in both forms, and
// in pinn_fit_kernel's sweep (d): chunk c adds rows c, c + CH, c + 2 CH, ... in ascending order in double, the CH chunk sums are added in
// ascending c in double, the old gradient (accumulate) last, ONE rounding to float. Only which lane loads which element differs.
// Round 8: the scalar form took 32 parameters per block with 1024 threads -- on BASELINE config 2 (256 rows x 12 756 floats, 13 MB) 399
// blocks, 6 400 waves of eight 256-byte load instructions each: bound by wave launch and load issue, not by bandwidth. The vector form
// reads the same bytes with a quarter of the load instructions, 1 KB each, from a quarter of the waves (profiles/r08_reduce_ab.txt).
// ------------------------------------------------------------------------------------------------------------
#ifndef PINN_REDUCE_LC
#define PINN_REDUCE_LC 16       // lanes per chunk of the vector form: 64 parameters per block of 512 threads (the shape sweep of round 8)
#endif
#define PINN_REDUCE_CH 32       // chunks of workgroup rows: part of the RESULT (the order of the sums), not a tuning knob
#define PINN_REDUCE_SCALAR_LC 32

struct PinnReduceArgs {
    const float* partials; int n_wg, p_core; float* grads; int accumulate, do_adam;
    float* params; float* m; float* v; const unsigned char* mask;
    int step_value; float step_size, bc2_sqrt; PinnOptK opt; int* step_ptr; float* loss_out; int off_loss;
    const PinnFitCtrl* ctrl; int ctrl_k; PinnNextBatch next;
};

template <int LC, int VW>
PINN_DEVICE void pinn_reduce_body(const PinnReduceArgs& A) {
    PINN_SMEM(red);
    constexpr int CH = PINN_REDUCE_CH, PB = LC * VW, NT = LC * CH;      // PB parameters x CH chunks of workgroups per block of NT threads
    static_assert(VW == 1 || VW == 4, "one dword or one 16-byte piece per lane and row");
    static_assert(PB <= NT && NT <= 1024, "block shape");
    const int tid = PINN_TID;
    const int n_wg = A.n_wg, p_core = A.p_core;
    int step_value = A.step_value;
    float step_size = A.step_size, bc2_sqrt = A.bc2_sqrt;
    float lr = A.opt.lr, decay = A.opt.decay;
    float* loss_out = A.loss_out;
    if (A.ctrl) {           // (graph replay: this iteration's Adam step, learning rate and loss slot come from the control block)
        step_value = A.ctrl->step0 + A.ctrl_k;
        step_size = A.ctrl->step_size[A.ctrl_k];
        bc2_sqrt = A.ctrl->bc2_sqrt[A.ctrl_k];
        lr = A.ctrl->lr[A.ctrl_k];
        decay = A.ctrl->decay[A.ctrl_k];
        loss_out = A.ctrl->loss_base + A.ctrl_k;
    }
    const int pl = tid % LC, ch = tid / LC;
    const int p0 = PINN_BID * PB + pl * VW;     // the first of this lane's VW parameters (VW = 4: p_core % 4 == 0, so all four or none)
    const int p = PINN_BID * PB + tid;          // the final lanes (the first PB threads) own ONE parameter each
    // the operands of the final lanes' update do not depend on the sums: fetched up front, so that their round trip runs under the
    // row loads instead of behind the barrier (round 5: this kernel took 8 us on BASELINE config 2 -- 4 % of the step -- for 13 MB;
    // it was a chain of dependent round trips: row after row, then the mask, then m / v / the parameter)
    const bool fin = tid < PB && p < p_core;
    bool upd = false;
    float g_old = 0.0f, m_old = 0.0f, v_old = 0.0f, p_old = 0.0f;
    if (fin) {
        if (A.accumulate) g_old = A.grads[p];
        if (A.do_adam) {
            upd = !A.mask || A.mask[p];
            if (upd) { m_old = A.m[p]; v_old = A.v[p]; p_old = A.params[p]; }
        }
    }
    // the rows of this thread's chunk, eight loads in flight at a time, summed in ascending row order (as before) -- in DOUBLE since
    // round 6: a gradient entry that is a cancelling sum over the batch (BASELINE config 4's d loss / d b_L: sum of |terms| 850 x the
    // result) walks through prefix sums far larger than its total, and every fp32 add of this loop rounded at THEIR magnitude: 5e-6
    // relative on that entry from the 256 rows alone (tools/cfg4_bl_probe.py). One rounding to fp32 at the end instead; the adds are
    // free beside the row loads.
    double s[VW];
#pragma unroll
    for (int e = 0; e < VW; ++e) s[e] = 0.0;
    if (p0 < p_core) {
        for (int w0 = ch; w0 < n_wg; w0 += 8 * CH) {
            float r[8][VW];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int w = w0 + j * CH;
                const float* src = A.partials + (size_t)w * p_core + p0;
                if constexpr (VW == 4) {
                    const f32x4 q = (w < n_wg) ? *reinterpret_cast<const f32x4*>(src) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    r[j][0] = q[0]; r[j][1] = q[1]; r[j][2] = q[2]; r[j][3] = q[3];
                } else {
                    r[j][0] = (w < n_wg) ? src[0] : 0.0f;
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (w0 + j * CH < n_wg) {
#pragma unroll
                    for (int e = 0; e < VW; ++e) s[e] += (double)r[j][e];
                }
        }
    }
    double* red64 = reinterpret_cast<double*>(red);         // [CH][PB]: a lane's VW sums are one 8 VW-byte piece of its chunk's row
#pragma unroll
    for (int e = 0; e < VW; ++e) red64[ch * PB + pl * VW + e] = s[e];
    PINN_SYNC();
    if (fin) {
        double t64 = 0.0;
        for (int c = 0; c < CH; ++c) t64 += red64[c * PB + tid];
        if (A.accumulate) t64 += (double)g_old;
        const float t = (float)t64;
        A.grads[p] = t;
        if (loss_out && p == A.off_loss) loss_out[0] = t;
        if (upd) pinn_optim_apply(A.opt, A.params, A.m, A.v, p, t, m_old, v_old, p_old, lr, decay, step_size, bc2_sqrt, step_value == 1);
    }
    if (A.do_adam && PINN_BID == 0 && tid == 0) A.step_ptr[0] = step_value;
    // fit chunks: this iteration's tile kernel is through with the batch buffer -- the batch of the next iteration is drawn here
    // (same generator, same counters as pinn_sample_kernel: bit-identical batches), which saves the iteration a dependent launch.
    // A point's words depend on its index alone, so the loop may stride by whatever shape this launch has.
    if (A.next.n > 0) {
        unsigned long long call = A.next.call;
        unsigned nk0 = A.next.k0, nk1 = A.next.k1;
        if (A.ctrl) { call = A.ctrl->call_index0 + (unsigned long long)(A.ctrl_k + 1); nk0 = A.ctrl->k0; nk1 = A.ctrl->k1; }
        for (long long i = (long long)PINN_BID * NT + tid; i < A.next.n; i += (long long)PINN_NBLK * NT)
            pinn_sample_point(A.next.xs, i, A.next.spec, nk0, nk1, (unsigned)(call & 0xffffffffull), (unsigned)(call >> 32));
    }
}

PINN_AUX_GLOBAL void PINN_LAUNCH_BOUNDS(PINN_REDUCE_LC * PINN_REDUCE_CH) pinn_reduce_kernel(PinnReduceArgs A) {
    pinn_reduce_body<PINN_REDUCE_LC, 4>(A);
}

PINN_AUX_GLOBAL void PINN_LAUNCH_BOUNDS(PINN_REDUCE_SCALAR_LC * PINN_REDUCE_CH) pinn_reduce_scalar_kernel(PinnReduceArgs A) {
    pinn_reduce_body<PINN_REDUCE_SCALAR_LC, 1>(A);
}

// ------------------------------------------------------------------------------------------------------------
// Standalone update (torch.optim single-tensor forms, model_torch.py:461): pinn_optim_kernel below
// ------------------------------------------------------------------------------------------------------------
// wt[l][in][out] = W_l[out][in] for the lh hidden->hidden matrices (hp x hp, row stride hp, layer stride hidden_stride):
// 32 x 32 tiles through LDS, both sides coalesced. Grid: (hp/32)^2 * lh workgroups of 256 threads.
PINN_AUX_GLOBAL void PINN_LAUNCH_BOUNDS(256) pinn_transpose_kernel(const float* wh, int hidden_stride, int hp, float* wt) {
    PINN_SMEM(tile);                                     // [32][33]
    const int tiles = hp / 32;
    const int l = PINN_BID / (tiles * tiles), t = PINN_BID % (tiles * tiles), tr = t / tiles, tc = t % tiles;
    const float* src = wh + (size_t)l * hidden_stride;
    float* dst = wt + (size_t)l * hp * hp;
    const int x = PINN_TID & 31, y0 = PINN_TID >> 5;
    for (int y = y0; y < 32; y += 8) tile[y * 33 + x] = src[(size_t)(tr * 32 + y) * hp + tc * 32 + x];
    PINN_SYNC();
    for (int y = y0; y < 32; y += 8) dst[(size_t)(tc * 32 + y) * hp + tr * 32 + x] = tile[x * 33 + y];
}

// ------------------------------------------------------------------------------------------------------------
// split-bf16 kernels (pinn_tile_kernel VAR 512): the hidden->hidden weights as MFMA A-operand fragments of three bf16 planes,
// w = hi + mid + lo exactly (pinn_split4's arithmetic), in the order the waves load them -- PinnCfg::wsp_frag:
// [layer][direction][K block of 32][16-unit tile j][plane][lane] x 16 bytes. Direction 0 (forward GEMM): lane (lr, lq) holds
// W[16 j + lr][32 kb + 8 lq + e], e = 0..7; direction 1 (data gradient): W[32 kb + 8 lq + e][16 j + lr]. One thread per
// (layer, direction, K block, tile, lane); rewritten before every step (the weights change every step), 147 KB at 3 x 64 x 64.
// ------------------------------------------------------------------------------------------------------------
PINN_AUX_GLOBAL void PINN_LAUNCH_BOUNDS(256) pinn_wsplit_kernel(const float* wh, int hidden_stride, int hp, int lh, pinn_s16x8* out) {
    const int kbs = hp / 32, nt = hp / 16;
    const int idx = PINN_BID * 256 + PINN_TID;
    if (idx >= lh * 2 * kbs * nt * 64) return;
    const int lane = idx & 63, j = (idx >> 6) % nt, kb = (idx >> 6) / nt % kbs, dir = (idx >> 6) / nt / kbs % 2, l = (idx >> 6) / nt / kbs / 2;
    const int lr = lane & 15, lq = lane >> 4;
    const float* W = wh + (size_t)l * hidden_stride;
    unsigned b[3][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int unit = 16 * j + lr, k = 32 * kb + 8 * lq + e;
        const float x = dir == 0 ? W[(size_t)unit * hp + k] : W[(size_t)k * hp + unit];
        pinn_split3(x, b[0][e], b[1][e], b[2][e]);
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        pinn_s16x8 f;
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = (short)(b[p][e] >> 16);
        out[((((size_t)(l * 2 + dir) * kbs + kb) * nt + j) * 3 + p) * 64 + lane] = f;
    }
}

PINN_AUX_GLOBAL void PINN_LAUNCH_BOUNDS(64) pinn_tick_kernel(int* step_ptr) {
    if (PINN_TID == 0 && PINN_BID == 0) step_ptr[0] += 1;
}

PINN_AUX_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_optim_kernel(float* params, const float* grads, float* m, float* v, const unsigned char* mask, long long n,
                  int* step_ptr, int step_value, float step_size, float bc2_sqrt, PinnOptK opt, float* loss_out, int off_loss) {
    // step_value > 0: the host counts (step_size / bc2_sqrt come with it, the count is mirrored to step_ptr); otherwise
    // the count lives on the device and the bias corrections are computed here
    // loss_out: the loss slot of the (all-reduced) gradient buffer is copied to one more address -- entry i of the host's
    // loss history (model_torch.py:464) -- so that recording an iteration costs no launch of its own
    const long long i = (long long)PINN_BID * 256 + PINN_TID;
    if (step_value > 0 && i == 0) step_ptr[0] = step_value;
    if (loss_out && i == 0) loss_out[0] = grads[off_loss];
    if (i >= n) return;
    if (mask && !mask[i]) return;
    // (the bias corrections are Adam's and AdamW's; SGD needs "is this step 1", RMSprop nothing)
    if (step_value <= 0) {
        step_value = step_ptr[0];
        if (opt.rule == PINN_OPT_ADAM || opt.rule == PINN_OPT_ADAMW) pinn_adam_scalars((double)step_value, opt.lr, opt.b1, opt.b2, &step_size, &bc2_sqrt);
    }
    pinn_optim_update(opt, params, grads[i], m, v, i, opt.lr, opt.decay, step_size, bc2_sqrt, step_value == 1);
}

// one thread per point. Counter = (point low, point high, call low, call high | block << 28): block b < 8 supplies the
// uniform words of columns 4b .. 4b+3, block 8 + c the two extra words of a normal column c (Box-Muller).
PINN_AUX_GLOBAL void PINN_LAUNCH_BOUNDS(256)
pinn_sample_kernel(float* xs, long long n, PinnSampleSpec spec, unsigned k0, unsigned k1, unsigned call_lo, unsigned call_hi,
                   const PinnFitCtrl* ctrl, int ctrl_k) {
    const long long i = (long long)PINN_BID * 256 + PINN_TID;
    if (i >= n) return;
    if (ctrl) {             // (graph replay: the batch counter of this iteration)
        const unsigned long long call = ctrl->call_index0 + (unsigned long long)ctrl_k;
        call_lo = (unsigned)(call & 0xffffffffull); call_hi = (unsigned)(call >> 32);
        k0 = ctrl->k0; k1 = ctrl->k1;
    }
    pinn_sample_point(xs, i, spec, k0, k1, call_lo, call_hi);
}

// ------------------------------------------------------------------------------------------------------------
// Residual-adaptive resampler (include/pinn.h pinn_resample_points): draws n_out rows of a pool of M candidate points with probability
// proportional to q_i = w_i + c, w_i = |r_i|^power in double (power 1 or 2: exact from the fp32 residual; a non-finite r_i counts 0),
// c = floor * mean(w) -- RAD of Wu, Zhu, Tan, Kartha, Lu, "A comprehensive study of non-adaptive and residual-based adaptive sampling for
// physics-informed neural networks" (CMAME 2023), kept unnormalised. Selection by inverse CDF over fp64 prefix sums, three launches:
//   1. pinn_resample_weights_kernel: block b of 256 threads owns points 256 b .. 256 b + 255: w, the block-local inclusive scan L_w and
//      the block total T_w[b] = L_w[last].
//   2. pinn_resample_offsets_kernel (ONE workgroup): S = sum_b T_w[b], c = floor * (S / M), then the inclusive scan E of the block totals
//      of q, T_q[b] = T_w[b] + n_b c (n_b points in block b); head = {E[nb - 1], c, S, M}.
//   3. pinn_resample_draw_kernel: one thread per output row i. One Philox4x32-10 block, counter (i_lo, i_hi, call_lo, call_hi), key = the
//      folded seed; u = ((w0 >> 5) 2^26 + (w1 >> 6)) 2^-53, t = u E[nb - 1]; b = the smallest block with E[b] > t (binary search), then
//      inside it the smallest l with E[b - 1] + (L_w[l] + (l + 1) c) > t -- or, where rounding leaves none, the block's last point of
//      positive q; row 256 b + l of the pool is copied. E[nb - 1] == 0 (no positive weight, floor 0): j = min(M - 1, floor(u M)).
// A redraw (period > 1) is launch 3 alone on a filled workspace.
// The order of every sum is fixed by the 256-thread block shape, which is part of the RESULT like PINN_REDUCE_CH: inside a wave the
// butterfly of pinn_block_scan_f64, the four wave totals in ascending order, the block totals in passes of 256 with a running carry.
// Two properties of that order carry the selection: the scans never decrease, and a term that is exactly zero leaves its prefix
// bit-equal to its left neighbour's (at wave, block and pass borders too) -- so "the smallest index whose prefix exceeds t" is never
// a point of zero weight while any weight is positive, on either level of the search. No atomics, nothing read back.
// ------------------------------------------------------------------------------------------------------------
#define PINN_RESAMPLE_BLOCK 256
#define PINN_RESAMPLE_MAX_POOL (1ll << 22)      // 16 384 block totals: 64 passes of the one workgroup of launch 2
#define PINN_RESAMPLE_HEAD 4                    // doubles in front of the workspace: E[nb - 1], c, S, M

struct PinnResampleArgs {
    const float* pool; const float* r; long long m; int d, power; double floor_c;
    long long n_out; unsigned k0, k1, call_lo, call_hi; float* xs_out; int* idx_out;
    double* head; double* local; double* tot; double* ends; int nb;      // workspace: head[4] | L_w[m] | T_w[nb] | E[nb]
};

PINN_DEVICE double pinn_lane_xor_f64(double v, int mask) {
#ifdef PINN_EMU
    return pinn_emu_shfl_xor_f64(v, mask);
#else
    return __shfl_xor(v, mask, 64);
#endif
}

// inclusive scan of one double per thread over the 256 threads of a workgroup; every thread also gets the total. Wave level: a butterfly
// -- after step k a lane holds the total of its aligned group of 2^(k+1) lanes (lower half + upper half) and, in `pre`, its inclusive
// prefix inside that group (lanes of the upper half add the lower half's total in front). lds: 4 doubles, free again on return.
PINN_DEVICE double pinn_block_scan_f64(double v, double* lds, double* total) {
    const int lane = PINN_TID & 63, wave = PINN_TID >> 6;
    double pre = v, tot = v;
    for (int k = 0; k < 6; ++k) {
        const double t = pinn_lane_xor_f64(tot, 1 << k);
        if (lane & (1 << k)) { pre = t + pre; tot = t + tot; }
        else tot = tot + t;
    }
    if (lane == 63) lds[wave] = tot;            // (== pre of the wave's last lane)
    PINN_SYNC();
    double off = 0.0, all = 0.0;
    for (int w = 0; w < PINN_RESAMPLE_BLOCK / 64; ++w) {
        if (w == wave) off = all;
        all += lds[w];
    }
    PINN_SYNC();
    *total = all;
    return off + pre;
}

// prefix of q from the prefix of w: l + 1 points of floor term c each (two roundings, never contracted: the emulator and the device agree)
PINN_DEVICE double pinn_resample_prefix(double lw, int l, double c) {
#pragma clang fp contract(off)
    const double t = (double)(l + 1) * c;
    return lw + t;
}

PINN_AUX_GLOBAL void PINN_LAUNCH_BOUNDS(PINN_RESAMPLE_BLOCK) pinn_resample_weights_kernel(PinnResampleArgs A) {
    PINN_SMEM(sm);
    double* lds = reinterpret_cast<double*>(sm);
    const long long i = (long long)PINN_BID * PINN_RESAMPLE_BLOCK + PINN_TID;
    double w = 0.0;
    if (i < A.m) {
        const double a = fabs((double)A.r[i]);
        if (a <= 3.4028234663852886e38) w = A.power == 2 ? a * a : a;       // (false for inf and NaN: weight 0)
    }
    double total;
    const double p = pinn_block_scan_f64(w, lds, &total);
    if (i < A.m) A.local[i] = p;
    if (PINN_TID == 0) A.tot[PINN_BID] = total;
}

PINN_AUX_GLOBAL void PINN_LAUNCH_BOUNDS(PINN_RESAMPLE_BLOCK) pinn_resample_offsets_kernel(PinnResampleArgs A) {
    PINN_SMEM(sm);
    double* lds = reinterpret_cast<double*>(sm);
    const int tid = PINN_TID, nb = A.nb;
    double sum_w = 0.0;
    for (int b0 = 0; b0 < nb; b0 += PINN_RESAMPLE_BLOCK) {
        double total;
        pinn_block_scan_f64(b0 + tid < nb ? A.tot[b0 + tid] : 0.0, lds, &total);
        sum_w += total;
    }
    const double c = A.floor_c * (sum_w / (double)A.m);
    double carry = 0.0;
    for (int b0 = 0; b0 < nb; b0 += PINN_RESAMPLE_BLOCK) {
        const int b = b0 + tid;
        double q = 0.0;
        if (b < nb) {
            const long long left = A.m - (long long)b * PINN_RESAMPLE_BLOCK;
            q = pinn_resample_prefix(A.tot[b], (int)(left < PINN_RESAMPLE_BLOCK ? left : PINN_RESAMPLE_BLOCK) - 1, c);
        }
        double total;
        const double incl = pinn_block_scan_f64(q, lds, &total);
        if (b < nb) A.ends[b] = carry + incl;
        carry += total;
    }
    if (tid == 0) { A.head[0] = carry; A.head[1] = c; A.head[2] = sum_w; A.head[3] = (double)A.m; }
}

PINN_AUX_GLOBAL void PINN_LAUNCH_BOUNDS(PINN_RESAMPLE_BLOCK) pinn_resample_draw_kernel(PinnResampleArgs A) {
    const long long i = (long long)PINN_BID * PINN_RESAMPLE_BLOCK + PINN_TID;
    if (i >= A.n_out) return;
    unsigned r[4];
    pinn_philox4x32_10((unsigned)((unsigned long long)i & 0xffffffffull), (unsigned)((unsigned long long)i >> 32), A.call_lo, A.call_hi,
                       A.k0, A.k1, r);
    const double u = (double)(((unsigned long long)(r[0] >> 5) << 26) | (unsigned long long)(r[1] >> 6)) * 1.1102230246251565e-16;   // 2^-53
    const double total = A.head[0], c = A.head[1];
    long long j;
    if (!(total > 0.0)) {
        j = (long long)(u * (double)A.m);
        if (j > A.m - 1) j = A.m - 1;
    } else {
        const double t = u * total;
        const int nb = A.nb;
        const double last_e = A.ends[nb - 1];
        int lo = 0, hi = nb - 1;                // E[hi] > t or E[hi] is the first block end that reaches the total: the search cannot run off
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const double e = A.ends[mid];
            if (e > t || e >= last_e) hi = mid; else lo = mid + 1;
        }
        const int b = lo;
        const double off = b > 0 ? A.ends[b - 1] : 0.0;
        const long long base = (long long)b * PINN_RESAMPLE_BLOCK;
        const long long left = A.m - base;
        const int n_b = (int)(left < PINN_RESAMPLE_BLOCK ? left : PINN_RESAMPLE_BLOCK);
        const double* lw = A.local + base;
        const double last_q = pinn_resample_prefix(lw[n_b - 1], n_b - 1, c);
        lo = 0; hi = n_b - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const double q = pinn_resample_prefix(lw[mid], mid, c);
            if (off + q > t || q >= last_q) hi = mid; else lo = mid + 1;
        }
        j = base + lo;
    }
    const float* src = A.pool + j * A.d;
    float* dst = A.xs_out + i * A.d;
    for (int k = 0; k < A.d; ++k) dst[k] = src[k];
    if (A.idx_out) A.idx_out[i] = (int)j;
}
