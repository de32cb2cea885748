// pinn_abi.cpp -- C-ABI of libpinn_hip.so (declared in include/pinn.h): descriptor, layout, launch dispatch.
// Built with hipcc for gfx950 (product) or, with -DPINN_EMU, as tests/emu/_build/libpinn_emu.so (test only).
#include "pinn_inst.h"
#include "pinn_fit_kernel.h"
#include "pinn_aux_kernels.h"
#include "pinn_port_probe.h"
#include "pinn_lbfgs_kernels.h"
#include "pinn_balance_kernels.h"
#include "pinn_causal_kernels.h"

#include <atomic>
#include <cfloat>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

namespace {
thread_local char g_err[512] = "";

int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}

int round16(int v) { return (v + 15) / 16 * 16; }

// one launch of a small kernel of this file on either backend; a refused launch is the error "<what> launch failed"
template <typename... K, typename... A>
int launch(const char* what, void (*kernel)(K...), int grid, int threads, size_t smem, void* stream, const A&... args) {
#ifdef PINN_EMU
    (void)what; (void)stream;
    emu::launch(grid, threads, smem, [&] { kernel(args...); });
#else
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), smem, (hipStream_t)stream, args...);
    if (hipGetLastError() != hipSuccess) return fail("%s launch failed", what);
#endif
    return 0;
}

int g_profile = 0;
long long* g_phase_prof = nullptr;
#ifndef PINN_EMU
// measurement hook (pinn_profile_tile): one pair of events per kernel and DEVICE -- an event belongs to the device it was
// created on, and a process may drive several
struct ProfEvents {
    hipEvent_t tile0 = nullptr, tile1 = nullptr, wg0 = nullptr, wg1 = nullptr;
    bool have_tile = false, have_wgrad = false;
};
ProfEvents g_prof[64];
int g_prof_dev = 0;                 // device of the last bracket (what pinn_last_*_ms reads)
ProfEvents* prof_events() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    ProfEvents& e = g_prof[dev];
    if (!e.tile0 && (hipEventCreate(&e.tile0) != hipSuccess || hipEventCreate(&e.tile1) != hipSuccess ||
                     hipEventCreate(&e.wg0) != hipSuccess || hipEventCreate(&e.wg1) != hipSuccess)) return nullptr;
    g_prof_dev = dev;
    return &e;
}
float prof_elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = -1.0f;
    if (hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&ms, a, b) != hipSuccess) return -1.0f;
    return ms;
}
#endif
}  // namespace

// (shared with the per-width translation units, not exported)
#define PINN_HIDDEN __attribute__((visibility("hidden")))
PINN_HIDDEN int g_pinn_last_kernel = -1;
PINN_HIDDEN char g_pinn_last_kernel_name[96] = "";
PINN_HIDDEN char g_pinn_last_wgrad_name[96] = "";
PINN_HIDDEN int g_pinn_last_launch[4] = {0, 0, 0, 0};   // grid, workgroups per CU of the plan, threads, dynamic LDS bytes
namespace {
int g_pinn_debug_flags = 0;         // -DPINN_DEBUG_ABI builds: pinn_debug_set_flags
}

struct pinn_net {
    pinn_layout_t lay;
    int n_layers, act, ndims, nparams, has_bc, has_ic, nsp;      // act: uniform activation code or -1
    unsigned long long act_codes[2];                              // 4 bits per activation index (pinn_act_code)
    float act_par[PINN_MAX_LAYERS];                               // parameter of activation a (pinn_set_act_params; torch's defaults at creation)
    int n_skips, skip_src[PINN_MAX_SKIPS], skip_dst[PINN_MAX_SKIPS], skip_pre, skip_src_pre, skip_outer;
    int dims[PINN_MAX_LAYERS + 1];
    float lo[PINN_MAX_INPUTS], hi[PINN_MAX_INPUTS], bc_value;
    int n_cu;
    int gemm_mode;                  // PINN_GEMM_FP32 / PINN_GEMM_BF16X3 (pinn_set_gemm_mode)
    int tanh_mode;                  // PINN_TANH_FAST / PINN_TANH_ACCURATE (pinn_set_tanh_mode)
    // pinn_fit_steps: the instantiated launch graph of one chunk and the arguments it was captured with (host state of the
    // descriptor; no device memory: the control block is the caller's)
    void* fit_graph_exec;
    unsigned long long fit_graph_key[4];
    int fit_graph_k;
    // diagnostics of THIS descriptor (pinn_debug_*: tests run one net at 1 workgroup per CU, with a separate pre-pass launch, with a
    // tiny slab budget -- a second Solver in the same process keeps its own planning)
    int fit_persistent;             // pinn_debug_fit_persistent: small fit chunks as ONE launch. 2 (default): the one-CU form for batches of a few tiles;
                                    // 1: the grid form (measured slower than launch-graph replay on MI355X); 0: never
    int fit_onecu_rounds;           // one-CU form: at most this many sweeps of its virtual workgroups per iteration (pinn_debug_fit_onecu_rounds)
    int max_per_cu;                 // pinn_debug_max_wgs_per_cu (default 4)
    int prepass_in_kernel;          // pinn_debug_prepass_in_kernel (default 1)
    size_t wgx_chunk_bytes;         // pinn_debug_wgx_chunk_bytes (default PINN_WGX_CHUNK_DEFAULT)
};

namespace {
typedef int (*launch_fn)(int, int, const PinnKArgs*, const PinnLaunchReq&);
typedef int (*wgrad_fn)(int, int, int, int, const PinnKArgs*, const PinnLaunchReq&);

wgrad_fn wgrad_launcher_for(int hp) {
    switch (hp) {
        case 128: return pinn_launch_wgrad_hp128;
        case 256: return pinn_launch_wgrad_hp256;
        case 512: return pinn_launch_wgrad_hp512;
        default: return nullptr;
    }
}

// WGX kernels keep the saved jets and gz of EVERY tile of a launch in HBM (44 B per point, layer and unit at S = 4): a
// batch larger than this many bytes of slab goes through the kernels chunk by chunk (gradients accumulate in the reduction)
constexpr size_t PINN_WGX_CHUNK_DEFAULT = (size_t)6656 << 20;

launch_fn launcher_for(int hp) {
    switch (hp) {
        case 16: return pinn_launch_tile_hp16;
        case 32: return pinn_launch_tile_hp32;
        case 64: return pinn_launch_tile_hp64;
        case 128: return pinn_launch_tile_hp128;
        case 256: return pinn_launch_tile_hp256;
        case 512: return pinn_launch_tile_hp512;
        default: return nullptr;
    }
}

// smallest compiled (nd, n2k) with n2k >= n2 (extra second-derivative streams get zero upstream gradient)
int pick_n2(int nd, int n2) {
    // (nd = 4: first derivatives only; its second-order form exists as ONE combined stream, `comb`)
    static const int avail[5][5] = {{1, 0, 0, 0, 0}, {1, 1, 0, 0, 0}, {1, 0, 1, 0, 0}, {0, 0, 1, 1, 0}, {1, 0, 0, 0, 0}};
    if (pinn_n3(n2) > 0 || pinn_n4(n2) > 0)     // packed count with third- / fourth-order streams: exact instantiations only
        return (((nd == 1 || nd == 2) && n2 == 9) || (nd == 1 && n2 == 73)) ? n2 : -1;       // 73 = 1 | 1 << 3 | 1 << 6: u, u', u'', u''', u''''
    if (n2 > 7) return -1;
    if (nd < 0 || nd > 4 || n2 < 0 || n2 > nd) return -1;
    for (int k = n2; k <= nd; ++k)
        if (avail[nd][k]) return k;
    return -1;
}

// compute units of the device the CALL runs on (the current device of the calling thread; cached per device): a net
// created while another device was current still gets the right grid
int device_cus(const pinn_net* net) {
#ifndef PINN_EMU
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return net->n_cu;
    if (cus[dev] == 0) {
        hipDeviceProp_t prop;
        cus[dev] = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : -1;
    }
    return cus[dev] > 0 ? cus[dev] : net->n_cu;
#else
    return net->n_cu;
#endif
}

struct Plan {
    launch_fn fn;
    int n2k, grid, threads, per_cu;
    size_t smem, slab_vec4_per_wg;  // saved-jet slab per workgroup (per TILE for WGX kernels)
    size_t wt_floats_per_wg;        // slab-in-LDS kernels: W^T scratch of every workgroup (PinnKArgs::wt)
    int64_t ntiles;                 // tiles of T = 16 * mt points in the batch
    int mt, comb;
    // WGX (widths >= 128): hidden->hidden weight gradients by pinn_wgrad_kernel from per-tile slabs in HBM
    int wgx, grid2;                 // grid2: workgroups of the weight-gradient kernel
    int wt_global;                  // the kernel reads the transposed global copy of the hidden weights (pinn_transpose_kernel)
    int split;                      // split-bf16 kernel: reads the bf16 fragment copy of the hidden weights (pinn_wsplit_kernel)
    int prepass_floats_per_lane;    // LDS floats per point of a tile the in-kernel pre-pass may use for its (double) registers; 0: no in-kernel pre-pass
    wgrad_fn wfn;
    size_t gz_vec4_per_tile;
    int64_t chunk_tiles;            // tiles per pass through the two kernels
    int rows() const { return wgx && grid2 > grid ? grid2 : grid; }       // partial-gradient rows the reduction sums
    size_t slab_bytes() const { return (size_t)(wgx ? chunk_tiles : grid) * slab_vec4_per_wg * 16; }
    size_t gz_bytes() const { return wgx ? (size_t)chunk_tiles * gz_vec4_per_tile * 16 : 0; }
};

// `hint`: the arguments of the call being planned. The launcher picks shape-specialised instantiations from them
// (pinn_spec_of), and those may differ from the general kernel in everything a plan holds -- workgroups per CU, tile
// height, slab size, whether the transposed weight copy is needed -- so a call is planned with its own arguments;
// sizing queries (no call yet) plan with the general probe AND with the arguments a typical training step of this net
// would carry (typical_step_args) and take the larger answer.
int make_plan(const pinn_net* net, int64_t n_points, int nd, int n2, Plan* plan, int mode = PINN_MODE_FORWARD,
              int res_kind = PINN_RES_PROGRAM, int comb = 0, const PinnKArgs* hint = nullptr) {
    plan->fn = launcher_for(net->lay.hp);
    if (!plan->fn) return fail("no kernel for padded hidden width %d (supported: 16, 32, 64, 128, 256, 512)", net->lay.hp);
    plan->n2k = comb ? 1 : pick_n2(nd, n2);
    if (comb && (n2 != 1 || nd < 2 || nd > 4)) return fail("combined second-order stream needs n2 == 1 and nd in {2, 3, 4}");
    if (plan->n2k < 0) return fail("unsupported derivative spec nd=%d n2=%d n3=%d n4=%d (nd <= 3 with n2 <= nd, nd = 4 with n2 = 0 / one combined second-order stream, one third-order direction with nd <= 2, or one fourth-order direction alone)", nd, pinn_n2(n2), pinn_n3(n2), pinn_n4(n2));
    PinnKArgs probe;
    if (hint) {
        probe = *hint;
    } else {
        memset(&probe, 0, sizeof(probe));
        probe.lh = net->lay.lh;
        probe.act = net->act;
        probe.act_codes[0] = net->act_codes[0]; probe.act_codes[1] = net->act_codes[1];
        for (int i = 0; i < PINN_MAX_LAYERS; ++i) probe.act_par[i] = net->act_par[i];
        probe.n_skips = net->n_skips;
        probe.skip_pre = net->skip_pre;
        probe.skip_src_pre = net->skip_src_pre;
        probe.skip_outer = net->skip_outer;
    }
    probe.gemm_mode = net->gemm_mode;
    probe.tanh_mode = net->tanh_mode;
    probe.mode = mode;
    probe.res_kind = res_kind;
    probe.comb = comb;
    PinnLaunchInfo info, winfo;
    if (plan->fn(nd, plan->n2k, &probe, {PinnLaunchOp::Plan, 0, nullptr, &info}))
        return fail("no kernel instantiation for width %d with nd=%d n2=%d%s", net->lay.hp, nd, plan->n2k, comb ? " (combined)" : "");
    plan->smem = (size_t)info.smem_bytes;
    plan->threads = info.threads;
    plan->slab_vec4_per_wg = (size_t)info.slab_vec4_per_wg;
    plan->wt_floats_per_wg = (size_t)info.wt_floats_per_wg;
    const int64_t ntiles = (n_points + 15) / 16;
    const int64_t wg_tiles = (ntiles + info.mt - 1) / info.mt;
    plan->per_cu = info.per_cu > net->max_per_cu ? net->max_per_cu : info.per_cu;
    int64_t grid = (int64_t)device_cus(net) * plan->per_cu;
    const int64_t teams = info.teams > 0 ? info.teams : 1;          // a two-team workgroup streams two tiles at a time
    if (grid > (wg_tiles + teams - 1) / teams) grid = (wg_tiles + teams - 1) / teams;
    if (grid < 1) grid = 1;
    plan->grid = (int)grid;
    plan->ntiles = wg_tiles;
    plan->mt = info.mt;
    plan->comb = comb;
    plan->wgx = (mode != PINN_MODE_FORWARD && info.wgx) ? 1 : 0;
    plan->wt_global = info.wt_global;
    plan->split = info.split;
    plan->prepass_floats_per_lane = info.prepass_floats_per_lane;
    plan->grid2 = 0; plan->wfn = nullptr; plan->gz_vec4_per_tile = 0; plan->chunk_tiles = wg_tiles;
    if (plan->wgx) {
        plan->wfn = wgrad_launcher_for(net->lay.hp);
        if (!plan->wfn || plan->wfn(nd, plan->n2k, comb, plan->mt, &probe, {PinnLaunchOp::Plan, 0, nullptr, &winfo}))
            return fail("no weight-gradient kernel for width %d with nd=%d n2=%d%s", net->lay.hp, nd, plan->n2k, comb ? " (combined)" : "");
        int64_t grid2 = (int64_t)device_cus(net) * winfo.per_cu;
        if (grid2 > wg_tiles) grid2 = wg_tiles;
        plan->grid2 = (int)(grid2 < 1 ? 1 : grid2);
        // the hidden->hidden blocks of a partial row are written by pinn_wgrad_kernel alone (rows < grid2; the tile kernel leaves
        // them untouched in WGX mode), and the reduction sums max(grid, grid2) rows: a tile-kernel grid beyond grid2 would add
        // rows whose blocks nobody wrote -- the occupancy query may answer more workgroups per CU for the tile
        // kernel than WGS_PER_CU of the weight-gradient kernel, so the tile grid is capped here
        if (plan->grid > plan->grid2) plan->grid = plan->grid2;
        plan->gz_vec4_per_tile = (size_t)info.gz_vec4_per_tile;
        // whole sweeps of the persistent workgroups per chunk
        const size_t per_tile = (plan->slab_vec4_per_wg + plan->gz_vec4_per_tile) * 16;
        const int64_t sweep = plan->grid2 > plan->grid ? plan->grid2 : plan->grid;
        int64_t chunk = (int64_t)(net->wgx_chunk_bytes / (per_tile ? per_tile : 1)) / sweep * sweep;
        if (chunk < sweep) chunk = sweep;
        plan->chunk_tiles = chunk < wg_tiles ? chunk : wg_tiles;
    }
    return 0;
}

void note_launch(const Plan& plan) {
    g_pinn_last_launch[0] = plan.grid; g_pinn_last_launch[1] = plan.per_cu;
    g_pinn_last_launch[2] = plan.threads; g_pinn_last_launch[3] = (int)plan.smem;
}

void fill_args(const pinn_net* net, PinnKArgs* a, const float* params, const float* xs, int64_t n, const int* dir_cols,
               int nd, int n2, const float* ic_streams, float ic_const) {
    memset(a, 0, sizeof(*a));
    const pinn_layout_t& L = net->lay;
    a->params = params; a->xs = xs; a->ic_streams = ic_streams; a->n_points = n;
    a->lh = L.lh; a->d = L.d; a->act = net->act; a->act_codes[0] = net->act_codes[0]; a->act_codes[1] = net->act_codes[1];
    for (int i = 0; i < PINN_MAX_LAYERS; ++i) a->act_par[i] = net->act_par[i];
    a->n_skips = net->n_skips;
    a->skip_pre = net->skip_pre;
    a->skip_src_pre = net->skip_src_pre;
    a->skip_outer = net->skip_outer;
    for (int k = 0; k < PINN_MAX_SKIPS; ++k) { a->skip_src[k] = net->skip_src[k]; a->skip_dst[k] = net->skip_dst[k]; }
    a->off_b1 = L.off_b1; a->off_wh = L.off_wh; a->hidden_stride = L.hidden_stride; a->off_wl = L.off_wl;
    a->off_bl = L.off_bl; a->off_ls = L.off_log_scale; a->off_loss = L.off_loss;
    a->p_core = L.p_total;          // partial rows / gradient buffer span the user slots too (V gradients of residual programs)
    a->off_extra = L.off_extra;
    a->ndims = net->ndims; a->nsp = net->nsp; a->has_bc = net->has_bc; a->has_ic = net->has_ic;
    a->bc_value = net->bc_value; a->t0 = net->lo[net->ndims - 1]; a->ic_const = ic_const;
    for (int i = 0; i < PINN_MAX_INPUTS; ++i) {
        a->lo[i] = net->lo[i]; a->hi[i] = net->hi[i];
        a->inv_w[i] = 1.0f / (net->hi[i] - net->lo[i]);
    }
    for (int k = 0; k < PINN_MAX_DIRS; ++k) a->dir_cols[k] = (k < nd) ? dir_cols[k] : 0;
    a->s_user = pinn_ns(nd, n2);
    a->gemm_mode = net->gemm_mode;
    a->tanh_mode = net->tanh_mode;
    a->tile_begin = 0;
    a->tile_end = 0;                // set from the plan (set_tile_range) before every launch
}

void set_tile_range(PinnKArgs* a, const Plan& plan, int64_t begin, int64_t end) {
    a->tile_begin = begin;
    a->tile_end = end < plan.ntiles ? end : plan.ntiles;
}

// what a fused training step of this net most likely passes: direction k = column k, constant affine coefficients
void typical_step_args(const pinn_net* net, PinnKArgs* a, int64_t n, int nd, int n2) {
    int dirs[PINN_MAX_DIRS];
    for (int k = 0; k < PINN_MAX_DIRS; ++k) dirs[k] = k;
    fill_args(net, a, nullptr, nullptr, n, dirs, nd, n2, nullptr, 0.0f);
    for (int s = 0; s < PINN_MAX_STREAMS; ++s) a->coef_row[s] = -1;
    a->src_row = -1;
}

int check_dirs(const pinn_net* net, const int* dir_cols, int nd, int n2p) {
    const int n2 = pinn_n2(n2p), n3 = pinn_n3(n2p), n4 = pinn_n4(n2p);       // packed count: seconds | thirds << 3 | fourths << 6 (include/pinn.h)
    if (nd < 0 || nd > PINN_MAX_DIRS || n2 > nd || n3 > n2 || n4 > n3 || n2p < 0) return fail("bad derivative spec nd=%d n2=%d n3=%d n4=%d", nd, n2, n3, n4);
    for (int k = 0; k < nd; ++k) {
        // direction code: column a, or the diagonal e_a +- e_b as a | (b + 1) << 4 | PINN_DIR_MINUS, | PINN_DIR_DOUBLE: 2 e_a +- e_b (include/pinn.h)
        if (!dir_cols || dir_cols[k] < 0 || dir_cols[k] > 0x7fff) return fail("dir_cols[%d] out of range", k);
        const int a = dir_cols[k] & 15, b = ((dir_cols[k] >> 4) & 15) - 1, c = ((dir_cols[k] >> 10) & 15) - 1;
        if (a >= net->lay.d || b >= net->lay.d || c >= net->lay.d || a == b || (c >= 0 && (c == a || c == b)))
            return fail("dir_cols[%d] names a column outside the %d inputs (or one column twice)", k, net->lay.d);
        if ((dir_cols[k] & (PINN_DIR_MINUS | PINN_DIR_DOUBLE)) && b < 0) return fail("dir_cols[%d]: PINN_DIR_MINUS / PINN_DIR_DOUBLE need a second column", k);
        if (c >= 0 && (b < 0 || (dir_cols[k] & PINN_DIR_DOUBLE))) return fail("dir_cols[%d]: a third column needs a plain second one", k);
        if ((dir_cols[k] & PINN_DIR_MINUS_C) && c < 0) return fail("dir_cols[%d]: PINN_DIR_MINUS_C needs a third column", k);
        if (c >= 0 && k < n4) return fail("dir_cols[%d]: three-column directions carry derivatives up to third order", k);
        // (the kernels decode these extensions only in the stream shapes that can carry them: pinn_dir_x, pinn_kernel.h)
        if (c >= 0 && n3 == 0) return fail("dir_cols[%d]: a three-column direction needs a third-order stream in the call (n3 > 0)", k);
        if ((dir_cols[k] & PINN_DIR_DOUBLE) && n4 == 0) return fail("dir_cols[%d]: PINN_DIR_DOUBLE needs a fourth-order stream in the call (n4 > 0)", k);
        // (round 5: third derivatives along diagonals too -- what mixed third-order partials are assembled from)
    }
    return 0;
}

// a request for the one-launch fit chunk (pinn_fit_kernel.h) in place of tile kernel + reduction. The caller fills ctrl, k_steps, xs, n and
// spec of `p`; run_train fills the rest and says in `launched` whether the chunk went out (false: the plan does not qualify, NOTHING was
// launched)
struct OneLaunch { PinnFitP p; bool launched; };

// what rides behind the tile pass of a step, handed down from residual_optim_step through residual_step_impl and run_train to
// launch_reduce: the update in the last reduction launch (buffers, step, rule) and the context of a fit chunk around it
struct StepTail {
    float* params; float* m; float* v; const unsigned char* mask; int* step_ptr;
    int step_value; PinnOptK opt;
    float* loss_out; int off_loss;
    PinnNextBatch next;             // the batch of the NEXT iteration, drawn by the same launch (n == 0: none)
    const PinnFitCtrl* capture;     // a chunk is being captured: the launches read their per-iteration values from this control block at
    int capture_k;                  // index capture_k (nullptr: they take them by value)
    OneLaunch* persist;             // nullptr: no such request
};

// the arguments of one step call and of one fit chunk, filled once by the exported entry point and handed on by reference
struct StepCall {
    pinn_t* net; const pinn_residual_t* residual; const float* params; const float* xs; int64_t n_points; const int* dir_cols; int nd, n2;
    const float* ic_streams; float ic_const; float* grads; void* workspace; size_t workspace_bytes; void* stream;
};
struct OptimState { float* params; float* exp_avg; float* exp_avg_sq; const uint8_t* mask; int32_t* step_ptr; };
struct FitCall {
    StepCall step;                  // (step.xs is `xs` below, the batch buffer every iteration overwrites; no ic_streams in a fit chunk)
    float* xs; const int* kind; const float* a; const float* b; uint64_t seed, call_index0;
    OptimState state; int32_t step0; PinnOptK opt;
    float* loss_history; int32_t k_steps; void* ctrl; size_t ctrl_bytes; const float* lr_steps;
};

// the tail of a step that only updates: no next batch, no capture, no one-launch request (off_loss: the caller's)
StepTail update_tail(const OptimState& s, int32_t step, const PinnOptK& opt, float* loss_out, int off_loss = -1) {
    return {s.params, s.exp_avg, s.exp_avg_sq, s.mask, s.step_ptr, step, opt, loss_out, off_loss, {nullptr, 0, {}, 0u, 0u, 0ull}, nullptr, 0, nullptr};
}

// the decimal a float was most likely written as, as a double: the shortest one that rounds back to it. torch derives 1 - alpha,
// 1 - dampening and 1 - lr * weight_decay from the caller's Python DOUBLES; pinn_optim_t carries floats, and 1 - (double)0.99f is 1e-6
// (relative) off 1 - 0.99
static double widen(float x) {
    char buf[40];
    for (int digits = 1; digits <= 9; ++digits) {
        snprintf(buf, sizeof(buf), "%.*g", digits, (double)x);
        const double d = strtod(buf, nullptr);
        if ((float)d == x) return d;
    }
    return (double)x;
}

static PinnOptK plain_adam(float lr, float b1, float b2, float eps) {
    PinnOptK k;
    memset(&k, 0, sizeof(k));
    k.rule = PINN_OPT_ADAM; k.lr = lr; k.b1 = b1; k.b2 = b2; k.eps = eps;
    k.decay = 1.0f; k.undamp = 1.0f; k.one_m_alpha = 1.0f;
    return k;
}

// pinn_optim_t (include/pinn.h) -> what the kernels take; non-zero (pinn_last_error set) for what the library refuses
static int optim_prepare(const pinn_optim_t* o, PinnOptK* k) {
    if (!o) return fail("null optimizer description");
    if (o->rule < 0 || o->rule > PINN_OPT_LAST) return fail("unknown optimizer rule %d", o->rule);
    if (!(o->lr >= 0.0f)) return fail("optimizer: invalid learning rate %g", (double)o->lr);
    if (!(o->weight_decay >= 0.0f)) return fail("optimizer: invalid weight_decay value %g", (double)o->weight_decay);
    *k = plain_adam(o->lr, 0.0f, 0.0f, 0.0f);
    k->rule = o->rule;
    k->wd = o->weight_decay;
    if (o->rule == PINN_OPT_ADAM || o->rule == PINN_OPT_ADAMW) {
        if (!(o->eps >= 0.0f)) return fail("optimizer: invalid epsilon value %g", (double)o->eps);
        if (!(o->beta1 >= 0.0f && o->beta1 < 1.0f) || !(o->beta2 >= 0.0f && o->beta2 < 1.0f))
            return fail("optimizer: invalid beta parameters (%g, %g)", (double)o->beta1, (double)o->beta2);
        k->b1 = o->beta1; k->b2 = o->beta2; k->eps = o->eps;
        if (o->rule == PINN_OPT_ADAMW) k->decay = (float)(1.0 - widen(o->lr) * widen(o->weight_decay));
    } else if (o->rule == PINN_OPT_SGD) {
        if (!(o->momentum >= 0.0f)) return fail("optimizer: invalid momentum value %g", (double)o->momentum);
        if (o->nesterov && (o->momentum <= 0.0f || o->dampening != 0.0f))
            return fail("optimizer: Nesterov momentum requires a momentum and zero dampening");
        k->momentum = o->momentum; k->nesterov = o->nesterov ? 1 : 0;
        k->undamp = (float)(1.0 - widen(o->dampening));
    } else {
        if (!(o->eps >= 0.0f)) return fail("optimizer: invalid epsilon value %g", (double)o->eps);
        if (!(o->momentum >= 0.0f)) return fail("optimizer: invalid momentum value %g", (double)o->momentum);
        if (!(o->alpha >= 0.0f)) return fail("optimizer: invalid alpha value %g", (double)o->alpha);
        if (o->momentum > 0.0f && o->centered)
            return fail("optimizer: RMSprop with momentum AND centered needs three state arrays; the kernels carry two");
        k->eps = o->eps; k->momentum = o->momentum; k->alpha = o->alpha; k->centered = o->centered ? 1 : 0;
        k->one_m_alpha = (float)(1.0 - widen(o->alpha));
    }
    return 0;
}

// step_size / bc2_sqrt of a step: Adam's and AdamW's bias corrections (the other rules take none)
static void optim_scalars(const PinnOptK& k, double step, float* step_size, float* bc2_sqrt) {
    *step_size = 0.0f; *bc2_sqrt = 1.0f;
    if (k.rule == PINN_OPT_ADAM || k.rule == PINN_OPT_ADAMW) pinn_adam_scalars(step, k.lr, k.b1, k.b2, step_size, bc2_sqrt);
}

// the rule `k` at the learning rate of ONE iteration of a schedule: what optim_prepare makes of the same pinn_optim_t with `lr` in place
// of its own (the rate itself and AdamW's 1 - lr * weight_decay from the widened doubles; nothing else derives from the rate)
static PinnOptK optim_at_rate(const PinnOptK& k, float lr) {
    PinnOptK r = k;
    r.lr = lr;
    if (k.rule == PINN_OPT_ADAMW) r.decay = (float)(1.0 - widen(lr) * widen(k.wd));
    return r;
}

// lr_steps of pinn_fit_steps: k_steps finite, non-negative rates in host memory (NULL: the constant rate of the struct)
static int check_lr_steps(const float* lr_steps, int32_t k_steps) {
    for (int32_t k = 0; lr_steps && k < k_steps; ++k)
        if (!(lr_steps[k] >= 0.0f) || !(lr_steps[k] <= FLT_MAX)) return fail("lr_steps[%d]: invalid learning rate %g", (int)k, (double)lr_steps[k]);
    return 0;
}

// the control block of a chunk as pinn_fit_ctrl_kernel takes it: per iteration the bias corrections, the learning rate and what
// derives from it -- the very numbers the eager loop hands its launches by value
static void fit_ctrl_fill(PinnFitCtrlArgs* ca, const FitCall& f) {
    ca->c.call_index0 = f.call_index0; ca->c.loss_base = f.loss_history; ca->c.step0 = f.step0; ca->c.pad = 0;
    ca->c.k0 = (unsigned)(f.seed & 0xffffffffull); ca->c.k1 = (unsigned)(f.seed >> 32);
    for (int k = 0; k < PINN_FIT_CHUNK_MAX; ++k) {
        const PinnOptK ok = (f.lr_steps && k < f.k_steps) ? optim_at_rate(f.opt, f.lr_steps[k]) : f.opt;
        ca->c.step_size[k] = 0.0f; ca->c.bc2_sqrt[k] = 1.0f;
        if (k < f.k_steps) optim_scalars(ok, (double)(f.step0 + k), &ca->c.step_size[k], &ca->c.bc2_sqrt[k]);
        ca->c.lr[k] = ok.lr; ca->c.decay[k] = ok.decay;
    }
}

// which form of the reduction the last launch_reduce took (pinn_last_reduce_kernel_name)
const char* g_last_reduce_name = "";

// The 16-byte row loads of pinn_reduce_kernel need every row to start on a 16-byte boundary: a base aligned to 16 bytes and a row stride
// that is a multiple of 4 floats. pinn_create_ex's layout guarantees the stride for the library's own launches (p_total = hp (d + 2) +
// lh (hp hp + hp) + 4 + PINN_EXTRA_SLOTS with hp a multiple of 16 and 16 user slots: a multiple of 4 for every net), and fill_args puts
// the partial rows at the very start of the caller's workspace, which run_train refuses unless it is 16-byte aligned: every fused step
// takes the vector form. pinn_reduce_rows takes any base and any row length: rows that do not qualify take the scalar form (same sums,
// pinn_aux_kernels.h). -DPINN_REDUCE_SCALAR=1 rebuilds the library
// with the scalar form everywhere, for the A/B.
#ifndef PINN_REDUCE_SCALAR
#define PINN_REDUCE_SCALAR 0
#endif
int launch_reduce(const float* partials, int n_wg, int p_core, float* grads, int accumulate, void* stream,
                  const StepTail* tail = nullptr) {
    const bool vec = !PINN_REDUCE_SCALAR && p_core % 4 == 0 && (reinterpret_cast<uintptr_t>(partials) & 15) == 0;
    const int lc = vec ? PINN_REDUCE_LC : PINN_REDUCE_SCALAR_LC, pb = vec ? 4 * lc : lc, threads = lc * PINN_REDUCE_CH;
    const int blocks = (p_core + pb - 1) / pb;
    const size_t smem = (size_t)PINN_REDUCE_CH * pb * sizeof(double);      // (the chunk sums cross the LDS in double: [CH][PB])
    const StepTail z = {nullptr, nullptr, nullptr, nullptr, nullptr, 0, plain_adam(0.f, 0.f, 0.f, 0.f), nullptr, -1,
                        {nullptr, 0, {}, 0u, 0u, 0ull}, nullptr, 0, nullptr};
    const StepTail& a = tail ? *tail : z;
    const int do_adam = tail ? 1 : 0;
    float step_size = 0.0f, bc2_sqrt = 1.0f;
    if (tail) optim_scalars(a.opt, (double)a.step_value, &step_size, &bc2_sqrt);
    // (a.capture is set by the HIP build's capture_chunk alone: the emulator's reductions always take their values by value)
    const PinnReduceArgs ra = {partials, n_wg, p_core, grads, accumulate, do_adam, a.params, a.m, a.v, a.mask, a.step_value, step_size, bc2_sqrt,
                               a.opt, a.step_ptr, a.loss_out, a.off_loss, a.capture, a.capture_k, a.next};
    g_last_reduce_name = vec ? "pinn_reduce_kernel" : "pinn_reduce_scalar_kernel";
    return launch("reduce kernel", vec ? pinn_reduce_kernel : pinn_reduce_scalar_kernel, blocks, threads, smem, stream, ra);
}

// pinn_sample_points; `capture` / `capture_k` as in StepTail (the exported call: nullptr)
int sample_points(float* xs, int64_t n_points, int d, const int* kind, const float* a, const float* b, uint64_t seed, uint64_t call_index,
                  void* stream, const PinnFitCtrl* capture, int capture_k) {
    if (!xs || !kind || !a || !b) return fail("null argument");
    if (d < 1 || d > PINN_MAX_INPUTS) return fail("d=%d outside [1, %d]", d, PINN_MAX_INPUTS);
    if (n_points <= 0) return 0;
    PinnSampleSpec spec;
    memset(&spec, 0, sizeof(spec));
    spec.d = d;
    for (int c = 0; c < d; ++c) {
        if (kind[c] < PINN_SAMPLE_UNIFORM || kind[c] > PINN_SAMPLE_CONST) return fail("column %d: unknown sampler kind %d", c, kind[c]);
        spec.kind[c] = kind[c]; spec.a[c] = a[c]; spec.b[c] = b[c];
    }
    const unsigned k0 = (unsigned)(seed & 0xffffffffull), k1 = (unsigned)(seed >> 32);
    const unsigned c_lo = (unsigned)(call_index & 0xffffffffull), c_hi = (unsigned)(call_index >> 32);
    return launch("sampler kernel", pinn_sample_kernel, (int)((n_points + 255) / 256), 256, 0, stream, xs, (long long)n_points, spec,
                  k0, k1, c_lo, c_hi, capture, capture_k);
}

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// widths >= 128 (PinnCfg::WTG): room for the transposed copy of the lh hidden->hidden matrices
size_t wt_workspace_bytes(const pinn_net* net) {
    return net->lay.lh > 0 ? align256((size_t)net->lay.lh * net->lay.hp * net->lay.hp * sizeof(float)) : 0;
}

// split-bf16 kernels: the bf16 fragment copy of the hidden weights (PinnCfg::wsp_bytes: 2 directions x 3 planes x 2 bytes)
size_t wsp_workspace_bytes(const pinn_net* net) {
    return net->lay.lh > 0 ? align256((size_t)net->lay.lh * 2 * 3 * net->lay.hp * net->lay.hp * 2) : 0;
}
}  // namespace

extern "C" {

const char* pinn_last_error(void) { return g_err; }

int pinn_sample_points(float* xs, int64_t n_points, int d, const int* kind, const float* a, const float* b,
                       uint64_t seed, uint64_t call_index, void* stream) {
    return sample_points(xs, n_points, d, kind, a, b, seed, call_index, stream, nullptr, 0);
}

#ifdef PINN_DEBUG_ABI
int pinn_debug_set_flags(int flags) { g_pinn_debug_flags = flags; return 0; }
#endif

int pinn_debug_last_kernel(void) { return g_pinn_last_kernel; }

// torch's default of the one parameter an activation module may carry
static float pinn_act_default_param(int code) {
    return code == PINN_ACT_LEAKYRELU ? 0.01f : (code == PINN_ACT_ELU || code == PINN_ACT_SOFTPLUS) ? 1.0f : 0.0f;
}

int pinn_set_act_params(pinn_t* net, const float* par, int n) {
    if (!net || !par) return fail("null argument");
    if (n != net->n_layers - 1) return fail("pinn_set_act_params: %d values for %d activations", n, net->n_layers - 1);
    for (int a = 0; a < n; ++a) {
        const int code = pinn_act_code(net->act_codes, a);
        const bool takes = code == PINN_ACT_LEAKYRELU || code == PINN_ACT_ELU || code == PINN_ACT_SOFTPLUS;
        if (!takes && par[a] != 0.0f) return fail("pinn_set_act_params: activation %d (code %d) takes no parameter", a, code);
        if (code == PINN_ACT_SOFTPLUS && !(par[a] > 0.0f)) return fail("pinn_set_act_params: Softplus beta must be positive (activation %d: %g)", a, par[a]);
        if (!(par[a] == par[a]) || par[a] > 1e30f || par[a] < -1e30f) return fail("pinn_set_act_params: activation %d: parameter is not finite", a);
    }
    for (int a = 0; a < n; ++a) {
        const int code = pinn_act_code(net->act_codes, a);
        if (code == PINN_ACT_LEAKYRELU || code == PINN_ACT_ELU || code == PINN_ACT_SOFTPLUS) net->act_par[a] = par[a];
    }
    return 0;
}

int pinn_set_tanh_mode(pinn_t* net, int mode) {
    if (!net) return fail("null argument");
    if (mode != PINN_TANH_FAST && mode != PINN_TANH_ACCURATE) return fail("unknown tanh mode %d", mode);
    net->tanh_mode = mode;
    return 0;
}

int pinn_set_gemm_mode(pinn_t* net, int mode) {
    if (!net) return fail("null argument");
    if (mode != PINN_GEMM_FP32 && mode != PINN_GEMM_BF16X3) return fail("unknown GEMM mode %d", mode);
    net->gemm_mode = mode;
    return 0;
}

const char* pinn_last_kernel_name(void) { return g_pinn_last_kernel_name; }

const char* pinn_last_wgrad_kernel_name(void) { return g_pinn_last_wgrad_name; }

const char* pinn_last_reduce_kernel_name(void) { return g_last_reduce_name; }

int pinn_debug_prepass_in_kernel(pinn_t* net, int enable) {
    if (!net) return fail("null argument");
    net->prepass_in_kernel = enable ? 1 : 0;
    return 0;
}

int pinn_debug_wgx_chunk_bytes(pinn_t* net, long long bytes) {
    if (!net) return fail("null argument");
    net->wgx_chunk_bytes = bytes > 0 ? (size_t)bytes : PINN_WGX_CHUNK_DEFAULT;
    return 0;
}

int pinn_debug_fit_onecu_rounds(pinn_t* net, int rounds) {
    if (!net) return -1;
    const int before = net->fit_onecu_rounds;
    if (rounds >= 1) net->fit_onecu_rounds = rounds;
    return before;
}

// the GRID form of the one-launch fit chunk (pinn_debug_fit_persistent 1) waits device-wide once per iteration with a bounded spin; a
// workgroup that gives up raises a flag and the whole grid returns WITHOUT writing parameters / losses back (pinn_fit_kernel.h). The host
// cannot see that from the launch: this call synchronises with the device and reads the flag of the last such chunk.
// (pinn_fit_chunk_status takes no handle, so this one piece of state stays with the thread; a call's context travels in StepTail)
static thread_local unsigned* g_fit_last_sync = nullptr;
int pinn_fit_chunk_status(void) {
    if (!g_fit_last_sync) return 0;
#ifdef PINN_EMU
    return (int)g_fit_last_sync[1];
#else
    unsigned host[2] = {0u, 0u};
    if (hipMemcpy(host, g_fit_last_sync, sizeof(host), hipMemcpyDeviceToHost) != hipSuccess) { fail("pinn_fit_chunk_status: hipMemcpy failed"); return -1; }
    if (host[1] != 0u) { fail("one-launch fit chunk (grid form) timed out at its device-wide wait: the chunk's iterations were NOT applied"); return 1; }
    return 0;
#endif
}

int pinn_debug_fit_persistent(pinn_t* net, int enable) {
    if (!net) return -1;
    const int before = net->fit_persistent;
    net->fit_persistent = (enable == 1 || enable == 2) ? enable : 0;
    return before;
}

int pinn_debug_max_wgs_per_cu(pinn_t* net, int cap) {
    if (!net) return -1;
    const int before = net->max_per_cu;
    net->max_per_cu = (cap <= 0 || cap > 4) ? 4 : cap;
    return before;
}

int pinn_last_launch_info(int32_t out[4]) {
    if (!out) return fail("null argument");
    for (int i = 0; i < 4; ++i) out[i] = g_pinn_last_launch[i];
    return g_pinn_last_launch[0] > 0 ? 0 : 1;
}

#ifdef PINN_DEBUG_ABI
int pinn_debug_phase_buffer(void* buf) {
    g_phase_prof = reinterpret_cast<long long*>(buf);
    return 0;
}
#endif

int pinn_profile_tile(int enable) {
    g_profile = enable ? 1 : 0;
#ifndef PINN_EMU
    for (ProfEvents& e : g_prof) e.have_tile = e.have_wgrad = false;
#endif
    return 0;
}

float pinn_last_tile_ms(void) {
#ifndef PINN_EMU
    const ProfEvents& e = g_prof[g_prof_dev];
    return e.have_tile ? prof_elapsed(e.tile0, e.tile1) : -1.0f;
#else
    return -1.0f;
#endif
}

float pinn_last_wgrad_ms(void) {
#ifndef PINN_EMU
    const ProfEvents& e = g_prof[g_prof_dev];
    return e.have_wgrad ? prof_elapsed(e.wg0, e.wg1) : -1.0f;
#else
    return -1.0f;
#endif
}

const char* pinn_backend(void) {
#ifdef PINN_EMU
    return "emu-host";
#else
    return "hip-gfx950";
#endif
}

int pinn_create(const int* layer_dims, int n_layers, int act, int ndims, int nparams, int has_bc, int has_ic,
                const float* dom_lo, const float* dom_hi, float bc_value, pinn_t** out) {
    if (n_layers < 2 || n_layers > PINN_MAX_LAYERS) return fail("n_layers=%d outside [2, %d]", n_layers, PINN_MAX_LAYERS);
    int acts[PINN_MAX_LAYERS];
    for (int a = 0; a < PINN_MAX_LAYERS; ++a) acts[a] = act;
    return pinn_create_ex(layer_dims, n_layers, acts, 0, nullptr, nullptr, ndims, nparams, has_bc, has_ic, dom_lo, dom_hi,
                          bc_value, out);
}

int pinn_create_ex(const int* layer_dims, int n_layers, const int* acts, int n_skips, const int* skip_src,
                   const int* skip_dst, int ndims, int nparams, int has_bc, int has_ic, const float* dom_lo,
                   const float* dom_hi, float bc_value, pinn_t** out) {
    if (!layer_dims || !out || !acts) return fail("null argument");
    if (n_layers < 2 || n_layers > PINN_MAX_LAYERS) return fail("n_layers=%d outside [2, %d]", n_layers, PINN_MAX_LAYERS);
    for (int a = 0; a + 1 < n_layers; ++a)
        if (acts[a] < PINN_ACT_TANH || acts[a] > PINN_ACT_LAST) return fail("unknown activation code %d (activation %d)", acts[a], a);
    if (n_skips < 0 || n_skips > PINN_MAX_SKIPS || (n_skips > 0 && (!skip_src || !skip_dst)))
        return fail("n_skips=%d outside [0, %d]", n_skips, PINN_MAX_SKIPS);
    int dst_of[PINN_MAX_SKIPS] = {0}, src_of[PINN_MAX_SKIPS] = {0}, pre_mask = 0, src_pre_mask = 0;
    for (int k = 0; k < n_skips; ++k) {
        dst_of[k] = skip_dst[k] & ~PINN_SKIP_PRE;
        src_of[k] = skip_src[k] & ~PINN_SKIP_PRE;
        if (skip_dst[k] & PINN_SKIP_PRE) pre_mask |= 1 << k;
        if (skip_src[k] & PINN_SKIP_PRE) src_pre_mask |= 1 << k;
        if (src_of[k] < 0 || src_of[k] >= dst_of[k] || dst_of[k] > n_layers - 2)
            return fail("skip %d: activations %d -> %d outside 0 <= src < dst <= %d", k, src_of[k], dst_of[k], n_layers - 2);
        if (layer_dims[src_of[k] + 1] != layer_dims[dst_of[k] + 1])
            return fail("skip %d joins widths %d and %d", k, layer_dims[src_of[k] + 1], layer_dims[dst_of[k] + 1]);
    }
    // Nesting (round 5): skips may lie inside one another ('fa R fa R fa fa + fa + f': the reference's layout letters pair like brackets)
    // or cross; at most one may START and at most one may END at an activation. A skip during whose life another one opens is "outer":
    // its jets wait in the skip's slab slot, the inner one rides in the registers.
    int outer_mask = 0;
    for (int k = 0; k < n_skips; ++k)
        for (int j = 0; j < n_skips; ++j) {
            if (j == k) continue;
            if (src_of[j] == src_of[k]) return fail("skips %d and %d both start at activation %d", k, j, src_of[k]);
            if (dst_of[j] == dst_of[k]) return fail("skips %d and %d both end at activation %d", k, j, dst_of[k]);
            if (src_of[j] > src_of[k] && src_of[j] < dst_of[k]) outer_mask |= 1 << k;
            // (a skip may start where another one ends only if it does not leave IN FRONT of the activation the other one joins behind)
            if (dst_of[j] == src_of[k] && (src_pre_mask >> k & 1) && !(pre_mask >> j & 1))
                return fail("skip %d starts in front of activation %d, skip %d ends behind it: overlap", k, src_of[k], j);
        }
    const int act = acts[0];
    const int d = ndims + nparams;
    if (ndims < 1 || nparams < 0 || d > PINN_MAX_INPUTS) return fail("ndims+nparams=%d outside [1, %d]", d, PINN_MAX_INPUTS);
    if (layer_dims[0] != d) return fail("layer_dims[0]=%d must equal ndims+nparams=%d", layer_dims[0], d);
    if (layer_dims[n_layers] != 1) return fail("the last layer must have one unit (got %d)", layer_dims[n_layers]);
    int hmax = 0;
    for (int l = 1; l < n_layers; ++l) {
        if (layer_dims[l] < 1) return fail("layer %d has width %d", l, layer_dims[l]);
        if (layer_dims[l] > hmax) hmax = layer_dims[l];
    }
    int hp = round16(hmax);
    if (hp == 48) hp = 64;
    if (hp > 64 && hp < 128) hp = 128;
    if (hp > 128 && hp <= 256) hp = 256;
    if (hp > 256 && hp <= 512) hp = 512;
    if (hp > 512) return fail("hidden width %d > 512 is not supported by this build", hmax);
    const int lh = n_layers - 2;
    // (width 512, round 6: eight bias-gradient rows in the LDS carve -- PinnCfg::ACCB_ROWS -- i.e. up to eight hidden layers)
    if (hp == 512 && lh + 1 > 8) return fail("hidden width %d (padded to 512): at most 8 hidden layers at this width, got %d", hmax, lh + 1);
    pinn_net* net = new (std::nothrow) pinn_net();
    if (!net) return fail("out of memory");
    memset(net, 0, sizeof(*net));
    net->fit_persistent = 2; net->fit_onecu_rounds = 1; net->max_per_cu = 4; net->prepass_in_kernel = 1; net->wgx_chunk_bytes = PINN_WGX_CHUNK_DEFAULT;
    net->n_layers = n_layers; net->act = act; net->ndims = ndims; net->nparams = nparams;
    for (int a = 0; a + 1 < n_layers; ++a) {
        net->act_codes[a >> 4] |= (unsigned long long)acts[a] << (4 * (a & 15));
        if (acts[a] != act) net->act = -1;
        net->act_par[a] = pinn_act_default_param(acts[a]);
    }
    net->n_skips = n_skips;
    for (int k = 0; k < n_skips; ++k) { net->skip_src[k] = src_of[k]; net->skip_dst[k] = dst_of[k]; }
    net->skip_pre = pre_mask; net->skip_src_pre = src_pre_mask; net->skip_outer = outer_mask;
    net->has_bc = has_bc ? 1 : 0; net->has_ic = has_ic ? 1 : 0; net->bc_value = bc_value;
    net->nsp = has_ic ? ndims - 1 : ndims;
    for (int l = 0; l <= n_layers; ++l) net->dims[l] = layer_dims[l];
    for (int i = 0; i < PINN_MAX_INPUTS; ++i) {
        net->lo[i] = (dom_lo && i < ndims) ? dom_lo[i] : 0.0f;
        net->hi[i] = (dom_hi && i < ndims) ? dom_hi[i] : 1.0f;
    }
    pinn_layout_t& L = net->lay;
    L.hp = hp; L.lh = lh; L.d = d;
    L.off_w1 = 0;
    L.off_b1 = hp * d;
    L.off_wh = L.off_b1 + hp;
    L.hidden_stride = hp * hp + hp;
    L.off_wl = L.off_wh + lh * L.hidden_stride;
    L.off_bl = L.off_wl + hp;
    L.off_log_scale = L.off_bl + 1;
    L.off_loss = L.off_bl + 2;
    L.p_core = L.off_bl + 4;
    L.off_extra = L.p_core;
    L.p_total = L.p_core + PINN_EXTRA_SLOTS;
    net->n_cu = 256;
#ifndef PINN_EMU
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        net->n_cu = prop.multiProcessorCount;
#else
    net->n_cu = 2;
#endif
    *out = net;
    return 0;
}

int pinn_destroy(pinn_t* net) {
#ifndef PINN_EMU
    if (net && net->fit_graph_exec) (void)hipGraphExecDestroy((hipGraphExec_t)net->fit_graph_exec);
#endif
    g_fit_last_sync = nullptr;          // (the flag lived in a workspace of this net's calls)
    delete net;
    return 0;
}

int pinn_layout(const pinn_t* net, pinn_layout_t* out) {
    if (!net || !out) return fail("null argument");
    *out = net->lay;
    return 0;
}

size_t pinn_workspace_bytes(const pinn_t* net, int64_t n_points, int nd, int n2) {
    if (!net) return 0;
    size_t need = 0;
    bool any = false;
    size_t slab_per_wg_max = 0;
    // every form a step of this derivative spec may take: separate second-order streams (affine residual, residual program, the
    // generic path's backward call) and ONE combined second-order stream (affine or program: trace.py lowers to it from a single
    // second derivative on -- `u_t + u_y + u_z = nu u_xx` in four variables exists in that form only), each planned
    // with the general probe and with the arguments of a typical training step (shape-specialised kernels); the largest answer
    const int forms[5][3] = {{PINN_MODE_STEP, PINN_RES_AFFINE, 0}, {PINN_MODE_STEP, PINN_RES_PROGRAM, 0}, {PINN_MODE_BACKWARD, 0, 0},
                             {PINN_MODE_STEP, PINN_RES_AFFINE, 1}, {PINN_MODE_STEP, PINN_RES_PROGRAM, 1}};
    for (int i = 0; i < 10; ++i) {
        Plan plan;
        const int* f = forms[i % 5];
        const bool comb = f[2] != 0;
        if (comb && (pinn_n2(n2) < 1 || nd < 2 || nd > 4 || pinn_n3(n2) > 0)) continue;
        const int n2q = comb ? 1 : n2;
        PinnKArgs typical;
        const bool with_hint = i >= 5 && nd <= net->lay.d;
        if (i >= 5 && !with_hint) continue;
        if (with_hint) typical_step_args(net, &typical, n_points, nd, n2q);
        // (a shape may exist in one form only: nd = 4 with second derivatives runs as the combined stream alone)
        if (make_plan(net, n_points, nd, n2q, &plan, f[0], f[1], comb ? 1 : 0, with_hint ? &typical : nullptr)) continue;
        any = true;
        const size_t v = align256((size_t)plan.rows() * net->lay.p_total * sizeof(float)) +
                         align256(plan.slab_bytes()) + align256(plan.gz_bytes()) +
                         align256((size_t)plan.grid * plan.wt_floats_per_wg * sizeof(float));
        if (v > need) need = v;
        if (plan.slab_vec4_per_wg > slab_per_wg_max) slab_per_wg_max = plan.slab_vec4_per_wg;
    }
    if (!any) return 0;
    // (narrow nets: partial rows of both parities and the private (parameters, exp_avg, exp_avg_sq) of every workgroup of a one-launch fit
    //  chunk, pinn_fit_kernel.h -- 5 x 16 x p_total floats at most)
    //  (+ the saved-jet slabs of the one-CU form's virtual workgroups: at most eight)
    const size_t persist = net->lay.hp <= 32 ? align256(2 * (size_t)PINN_FIT_MAX_WGS * net->lay.p_total * sizeof(float)) +
                                               align256(3 * (size_t)PINN_FIT_MAX_WGS * net->lay.p_total * sizeof(float)) + 512 +
                                               align256(8 * slab_per_wg_max * sizeof(f32x4)) : 0;
    return need + align256((size_t)PINN_MAX_AUX * (size_t)n_points * sizeof(float)) + wt_workspace_bytes(net) +
           wsp_workspace_bytes(net) + 256 + persist;
}

static int jet_forward_impl(pinn_t* net, const float* params, const float* xs, int64_t n_points, const int* dir_cols, int nd,
                            int n2, const float* ic_streams, float ic_const, float* streams_out, void* workspace, size_t workspace_bytes,
                            void* stream) {
    if (!net || !params || !xs || !streams_out) return fail("null argument");
    if (n_points <= 0) return 0;
    if (check_dirs(net, dir_cols, nd, n2)) return 1;
    Plan plan;
    if (make_plan(net, n_points, nd, n2, &plan)) return 1;
    PinnKArgs a;
    fill_args(net, &a, params, xs, n_points, dir_cols, nd, n2, ic_streams, ic_const);
    a.mode = PINN_MODE_FORWARD;
    a.out_streams = streams_out;
    if (net->skip_outer) {
        // nested skips: the outer skip's jets wait in a slab slot between 'R' and '+' -- also in a value-only forward pass
        const size_t need = align256((size_t)plan.grid * plan.slab_vec4_per_wg * sizeof(f32x4));
        if (!workspace || workspace_bytes < need)
            return fail("a net with nested skip connections needs scratch for its forward pass too: call pinn_jet_forward_ws with %zu bytes "
                        "(pinn_workspace_bytes covers it), got %zu", need, workspace ? workspace_bytes : (size_t)0);
        if (((uintptr_t)workspace & 15) != 0) return fail("workspace must be 16-byte aligned");
        a.slab = reinterpret_cast<f32x4*>(workspace);
    }
    set_tile_range(&a, plan, 0, plan.ntiles);
    const int rc = plan.fn(nd, plan.n2k, &a, {PinnLaunchOp::Launch, plan.grid, stream});
    note_launch(plan);
    return rc ? fail("tile kernel launch failed (%d)", rc) : 0;
}

int pinn_jet_forward(pinn_t* net, const float* params, const float* xs, int64_t n_points, const int* dir_cols, int nd,
                     int n2, const float* ic_streams, float ic_const, float* streams_out, void* stream) {
    return jet_forward_impl(net, params, xs, n_points, dir_cols, nd, n2, ic_streams, ic_const, streams_out, nullptr, 0, stream);
}

int pinn_jet_forward_ws(pinn_t* net, const float* params, const float* xs, int64_t n_points, const int* dir_cols, int nd,
                        int n2, const float* ic_streams, float ic_const, float* streams_out, void* workspace, size_t workspace_bytes,
                        void* stream) {
    return jet_forward_impl(net, params, xs, n_points, dir_cols, nd, n2, ic_streams, ic_const, streams_out, workspace, workspace_bytes, stream);
}

static int run_train(pinn_t* net, PinnKArgs* a, const Plan& plan, int nd, float* grads, int accumulate, void* workspace,
                     size_t workspace_bytes, void* stream, const pinn_program_t* pre = nullptr,
                     const StepTail* tail = nullptr, const double* pre_consts64 = nullptr) {
    const size_t part_bytes = align256((size_t)plan.rows() * net->lay.p_total * sizeof(float));
    const size_t slab_bytes = align256(plan.slab_bytes());
    const size_t aux_bytes = (pre && a->n_aux > 0) ? align256((size_t)a->n_aux * (size_t)a->n_points * sizeof(float)) : 0;
    // transposed hidden weights: one copy written by pinn_transpose_kernel (widths >= 128) or one scratch per workgroup
    // filled by the tile kernel itself (slab-in-LDS kernels)
    const size_t wt_bytes = plan.wt_floats_per_wg ? align256((size_t)plan.grid * plan.wt_floats_per_wg * sizeof(float))
                                                  : (plan.wt_global ? wt_workspace_bytes(net) : 0);
    const size_t gz_bytes = align256(plan.gz_bytes());
    const size_t wsp_bytes = plan.split ? wsp_workspace_bytes(net) : 0;
    const size_t need = part_bytes + slab_bytes + aux_bytes + wt_bytes + gz_bytes + wsp_bytes;
    if (!workspace || workspace_bytes < need)
        return fail("workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    if (((uintptr_t)workspace & 15) != 0) return fail("workspace must be 16-byte aligned");
    char* ws = reinterpret_cast<char*>(workspace);
    a->prof = g_phase_prof;
    a->debug_flags = g_pinn_debug_flags;
    a->partials = reinterpret_cast<float*>(ws);
    a->slab = reinterpret_cast<f32x4*>(ws + part_bytes);
    a->gzslab = gz_bytes ? reinterpret_cast<f32x4*>(ws + part_bytes + slab_bytes + aux_bytes + wt_bytes) : nullptr;
    a->partial_row0 = plan.grid;
    if (aux_bytes) {
        float* aux = reinterpret_cast<float*>(ws + part_bytes + slab_bytes);
        a->aux = aux;
        // the pre-pass runs in fp64 (include/pinn.h, pinn_residual_t::pre_consts64): its constants unrounded
        PinnPreConsts pc64;
        for (int k = 0; k < PINN_MAX_CONSTS; ++k) pc64.v[k] = pre_consts64 ? pre_consts64[k] : (double)pre->consts[k];
        int nregs = a->d;
        for (int i = 0; i < pre->n_ops; ++i) {
            const uint32_t w = pre->code[i];
            const int op = w & 255, dst = (w >> 8) & 255;
            if (op != PINN_OP_STORE && dst + 1 > nregs) nregs = dst + 1;
        }
        // in the kernel its registers are doubles in the (not yet used) LDS activation buffers: one tile's worth of points must fit --
        // always, except for a long program in front of the narrowest one-stream kernels, which takes the separate launch
        if (net->prepass_in_kernel && 2 * nregs <= plan.prepass_floats_per_lane) {
            a->pre = *pre;          // evaluated in the prologue of the tile kernel: one launch (and one dependent-launch gap) less
            a->pre_consts64 = pc64;
            a->pre_nregs = nregs;
        } else if (launch("pre-pass kernel", pinn_aux_kernel, (int)((a->n_points + 255) / 256), 256, 0, stream, a->xs, a->n_points, a->d, *pre, pc64, aux)) {
            return 1;
        }
    }
    if (plan.wt_floats_per_wg)
        a->wt = reinterpret_cast<float*>(ws + part_bytes + slab_bytes + aux_bytes);
    else if (wt_bytes) {
        // widths >= 128: transposed copy of the hidden weights for the data-gradient GEMM (the weights change every step)
        float* wt = reinterpret_cast<float*>(ws + part_bytes + slab_bytes + aux_bytes);
        a->wt = wt;
        const int hp = net->lay.hp, blocks = (hp / 32) * (hp / 32) * net->lay.lh;
        const float* wh = a->params + net->lay.off_wh;
        const int stride = net->lay.hidden_stride;
        if (launch("transpose kernel", pinn_transpose_kernel, blocks, 256, 32 * 33 * sizeof(float), stream, wh, stride, hp, wt)) return 1;
    }
    if (wsp_bytes && net->lay.lh > 0) {
        // split-bf16 kernels: hidden weights -> hi / mid / lo bf16 MFMA fragments (the weights change every step)
        pinn_s16x8* wsp = reinterpret_cast<pinn_s16x8*>(ws + part_bytes + slab_bytes + aux_bytes + wt_bytes + gz_bytes);
        a->wsp = wsp;
        const int hp = net->lay.hp, lh = net->lay.lh;
        const int blocks = (lh * 2 * (hp / 32) * (hp / 16) * 64 + 255) / 256;
        const float* wh = a->params + net->lay.off_wh;
        const int stride = net->lay.hidden_stride;
        if (launch("weight-split kernel", pinn_wsplit_kernel, blocks, 256, 0, stream, wh, stride, hp, lh, wsp)) return 1;
    }
#ifndef PINN_EMU
    ProfEvents* pe = g_profile ? prof_events() : nullptr;
    if (g_profile && !pe) return fail("hipEventCreate failed");
    if (pe) pe->have_wgrad = false;
#endif
    if (tail && tail->persist) {
        // a whole chunk of fit iterations in ONE launch (pinn_fit_kernel.h): the step must be one pass of a non-streamed kernel, the
        // instantiation must carry the kernel, the scratch for rows / private states must fit behind `need`. Mode 2: the one-CU form
        // (virtual workgroups, no device-scope wait) for batches of at most fit_onecu_rounds sweeps of its virtual workgroups; mode 1:
        // the grid form (every workgroup resident).
        tail->persist->launched = false;
        PinnFitProbe has;
        const size_t pc = (size_t)net->lay.p_total;
        bool ok = !plan.wgx && !plan.wt_global && !plan.split && plan.chunk_tiles >= plan.ntiles && !g_profile &&
                  (!aux_bytes || a->pre.n_ops > 0) && plan.fn(nd, plan.n2k, a, {PinnLaunchOp::FitProbe, plan.grid, stream, nullptr, &has}) == 0 && has.carries;
        // (pre-pass rows: only where the pre-pass went INTO the kernel above, which then evaluates it for every batch it draws. One that
        //  took the separate pinn_aux_kernel launch -- switched off, or more double registers than prepass_floats_per_lane holds -- wrote
        //  the rows of the batch in `xs` once: the chunk keeps the launch graphs or the eager loop, which run it every iteration)
        const int vw = has.onecu_vw;
        const bool onecu = ok && net->fit_persistent == 2 && vw >= 2 && vw <= 8 && plan.ntiles <= (int64_t)vw * net->fit_onecu_rounds;
        const bool gridform = ok && net->fit_persistent == 1 && plan.grid <= PINN_FIT_MAX_WGS;
        const int rows = onecu ? vw : plan.grid, states = onecu ? 1 : plan.grid;
        const size_t rows_b = align256(2 * (size_t)rows * pc * sizeof(float)), state_b = align256(3 * (size_t)states * pc * sizeof(float));
        const size_t slab1_b = onecu ? align256((size_t)vw * plan.slab_vec4_per_wg * sizeof(f32x4)) : 0;      // the virtual workgroups' own slabs
        if ((onecu || gridform) && workspace_bytes >= need + rows_b + state_b + 256 + slab1_b) {
            PinnFitP& P = tail->persist->p;
            P.rows = reinterpret_cast<float*>(ws + need);
            P.state = reinterpret_cast<float*>(ws + need + rows_b);
            P.sync = reinterpret_cast<unsigned*>(ws + need + rows_b + state_b);
            if (onecu && a->slab) a->slab = reinterpret_cast<f32x4*>(ws + need + rows_b + state_b + 256);
            P.params = tail->params; P.m = tail->m; P.v = tail->v; P.mask = tail->mask; P.step_ptr = tail->step_ptr; P.grads = grads;
            P.opt = tail->opt; P.off_loss = net->lay.off_loss;
#ifdef PINN_EMU
            memset(P.sync, 0, 256);
#else
            if (!onecu && hipMemsetAsync(P.sync, 0, 256, (hipStream_t)stream) != hipSuccess) return fail("hipMemsetAsync failed");
#endif
            set_tile_range(a, plan, 0, plan.ntiles);
            const int rc = plan.fn(nd, plan.n2k, a, {onecu ? PinnLaunchOp::FitOneCu : PinnLaunchOp::FitGrid, onecu ? 1 : plan.grid, stream, nullptr, nullptr, &P});
            note_launch(plan);
            if (rc == 1) return 0;               // (this instantiation has no such form after all: the caller falls back)
            if (rc) return fail("fit kernel launch failed (%d)", rc);
            tail->persist->launched = true;
            if (onecu) {
                // pinn_last_launch_info: ONE workgroup of vw virtual ones, and the LDS it asked for (PinnFitVw: the blocks and W^T of
                // the probe, then state, rows, batch and pre-pass rows as in resident_floats)
                const long long pcp = ((long long)pc + 3) / 4 * 4, n = a->n_points;
                const long long resident = (3 + vw) * pcp + (n * a->d + 3) / 4 * 4 + (n * a->n_aux + 3) / 4 * 4;
                g_pinn_last_launch[0] = 1; g_pinn_last_launch[1] = 1;
                g_pinn_last_launch[2] = plan.threads * vw; g_pinn_last_launch[3] = (int)(has.onecu_base_bytes + 4 * resident);
            }
            if (!onecu) g_fit_last_sync = P.sync;               // (grid form: its timeout flag, read back by pinn_fit_chunk_status)
        }
        return 0;
    }
    // one pass (any non-WGX kernel; a WGX batch whose slabs fit the net's wgx_chunk_bytes) or chunk by chunk: tile kernel ->
    // weight-gradient kernel -> reduction of the partial rows, later chunks ADD into `grads`, Adam rides in the last reduction
    for (int64_t t0 = 0; t0 < plan.ntiles || t0 == 0; t0 += plan.chunk_tiles) {
        const bool last = t0 + plan.chunk_tiles >= plan.ntiles;
        set_tile_range(a, plan, t0, t0 + plan.chunk_tiles);
#ifndef PINN_EMU
        if (pe) hipEventRecord(pe->tile0, (hipStream_t)stream);
#endif
        const int rc = plan.fn(nd, plan.n2k, a, {PinnLaunchOp::Launch, plan.grid, stream});
        note_launch(plan);
        if (rc) return fail("tile kernel launch failed (%d)", rc);
#ifndef PINN_EMU
        if (pe) { hipEventRecord(pe->tile1, (hipStream_t)stream); pe->have_tile = true; }
#endif
        if (plan.wgx && net->lay.lh > 0) {
#ifndef PINN_EMU
            if (pe) hipEventRecord(pe->wg0, (hipStream_t)stream);
#endif
            const int rw = plan.wfn(nd, plan.n2k, plan.comb, plan.mt, a, {PinnLaunchOp::Launch, plan.grid2, stream});
            if (rw) return fail("weight-gradient kernel launch failed (%d)", rw);
#ifndef PINN_EMU
            if (pe) { hipEventRecord(pe->wg1, (hipStream_t)stream); pe->have_wgrad = true; }
#endif
        }
        const int rows = (plan.wgx && net->lay.lh > 0) ? plan.rows() : plan.grid;
        if (launch_reduce(a->partials, rows, net->lay.p_total, grads, (accumulate || t0 > 0) ? 1 : 0, stream, last ? tail : nullptr))
            return 1;
        if (last) break;
    }
    return 0;
}

int pinn_jet_backward(pinn_t* net, const float* params, const float* xs, int64_t n_points, const int* dir_cols, int nd,
                      int n2, const float* ic_streams, float ic_const, const float* grad_streams, float* grads,
                      int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    if (!net || !params || !xs || !grad_streams || !grads) return fail("null argument");
    if (n_points <= 0) return 0;
    if (check_dirs(net, dir_cols, nd, n2)) return 1;
    Plan plan;
    if (make_plan(net, n_points, nd, n2, &plan, PINN_MODE_BACKWARD, 0)) return 1;
    PinnKArgs a;
    fill_args(net, &a, params, xs, n_points, dir_cols, nd, n2, ic_streams, ic_const);
    a.mode = PINN_MODE_BACKWARD;
    a.gin = grad_streams;
    return run_train(net, &a, plan, nd, grads, accumulate, workspace, workspace_bytes, stream);
}

static int check_program(const pinn_program_t& pg, int first_temp, int n_consts_max, bool pre, int n_aux, const char* what) {
    if (pg.n_ops < 0 || pg.n_ops > PINN_MAX_OPS || pg.n_consts < 0 || pg.n_consts > n_consts_max)
        return fail("%s program size out of range (ops=%d consts=%d)", what, pg.n_ops, pg.n_consts);
    for (int i = 0; i < pg.n_ops; ++i) {
        const uint32_t w = pg.code[i];
        const int op = w & 255, dst = (w >> 8) & 255, ra = (w >> 16) & 255, rb = (w >> 24) & 255;
        if (op > PINN_OP_STORE) return fail("%s program instruction %d: unknown opcode %d", what, i, op);
        if (op == PINN_OP_STORE) {
            if (!pre) return fail("%s program instruction %d: STORE is a pre-pass instruction", what, i);
            if (rb >= n_aux || ra >= PINN_MAX_REGS) return fail("%s program instruction %d: bad STORE", what, i);
            continue;
        }
        const bool b_is_reg = op == PINN_OP_ADD || op == PINN_OP_SUB || op == PINN_OP_MUL || op == PINN_OP_DIV;
        if (dst < first_temp) return fail("%s program instruction %d overwrites an input register", what, i);
        if (dst >= PINN_MAX_REGS || (op != PINN_OP_CONST && ra >= PINN_MAX_REGS) || (b_is_reg && rb >= PINN_MAX_REGS))
            return fail("%s program instruction %d uses a register >= %d", what, i, PINN_MAX_REGS);
        if (op == PINN_OP_CONST && ra >= pg.n_consts) return fail("%s program instruction %d: bad constant", what, i);
        if (op == PINN_OP_POW && rb >= pg.n_consts) return fail("%s program instruction %d: bad exponent", what, i);
    }
    return 0;
}

static int residual_step_impl(const StepCall& c, float inv_n_global, const StepTail* tail, int accumulate = 0) {
    pinn_t* net = c.net;
    const pinn_residual_t* residual = c.residual;
    const float* ic_streams = c.ic_streams;
    const int64_t n_points = c.n_points;
    const int nd = c.nd, n2 = c.n2;
    if (!net || !residual || !c.params || !c.xs || !c.grads) return fail("null argument");
    if (n_points <= 0) return fail("n_points must be positive");
    if (check_dirs(net, c.dir_cols, nd, n2)) return 1;
    if (residual->n_aux < 0 || residual->n_aux > PINN_MAX_AUX) return fail("n_aux=%d outside [0, %d]", residual->n_aux, PINN_MAX_AUX);
    if (residual->kind != PINN_RES_AFFINE && residual->kind != PINN_RES_PROGRAM) return fail("unknown residual kind %d", residual->kind);
    Plan plan;
    const int comb = residual->combined ? 1 : 0;
    // (the plan itself is made below, with the call's own arguments; here only the stream count of the instantiation)
    const int n2k = comb ? 1 : pick_n2(nd, n2);
    if (comb && (n2 != 1 || nd < 2 || nd > 4)) return fail("combined second-order stream needs n2 == 1 and nd in {2, 3, 4}");
    if (n2k < 0) return fail("unsupported derivative spec nd=%d n2=%d n3=%d", nd, pinn_n2(n2), pinn_n3(n2));
    const int d = net->lay.d;
    const int s_user = pinn_ns(nd, n2), s_kernel = pinn_ns(nd, n2k), shift = s_kernel - s_user;
    PinnKArgs a;
    fill_args(net, &a, c.params, c.xs, n_points, c.dir_cols, nd, n2, ic_streams, c.ic_const);
    a.res_kind = residual->kind;
    a.n_aux = residual->n_aux;
    a.n_vars = residual->n_vars;
    if (a.n_vars < 0 || a.n_vars > PINN_MAX_VARS || a.n_vars > PINN_EXTRA_SLOTS)
        return fail("n_vars=%d outside [0, %d]", a.n_vars, PINN_MAX_VARS);
    if (a.n_vars > 0 && residual->kind != PINN_RES_PROGRAM) return fail("trainable variables need a residual program (kind PINN_RES_PROGRAM)");
    a.ic_var1 = residual->ic_var1;
    if (a.ic_var1 < 0 || a.ic_var1 > PINN_EXTRA_SLOTS) return fail("ic_var1=%d outside [0, %d]", a.ic_var1, PINN_EXTRA_SLOTS);
    if (a.ic_var1 > 0 && (!net->has_ic || ic_streams)) return fail("ic_var1 needs a problem with an initial condition and no ic_streams");
    a.comb = comb;
    for (int k = 0; k < PINN_MAX_DIRS; ++k) a.comb_w[k] = (comb && k < nd) ? residual->comb_w[k] : 0.0f;
    a.ic_rows = residual->ic_rows ? 1 : 0;
    if (a.ic_rows) {
        if (!net->has_ic || ic_streams || residual->ic_var1 > 0) return fail("ic_rows needs a problem with an initial condition, no ic_streams and no ic_var1");
        for (int s = 0; s < PINN_MAX_STREAMS; ++s) {
            a.ic_row[s] = (s < s_user) ? residual->ic_row[s] : -1;
            a.ic_cst[s] = (s < s_user) ? residual->ic_cst[s] : 0.0f;
            if (a.ic_row[s] >= residual->n_aux) return fail("ic_row[%d] refers to a missing pre-pass row", s);
        }
    }
    if (residual->n_aux > 0 && check_program(residual->pre, d, PINN_MAX_CONSTS, true, residual->n_aux, "pre-pass")) return 1;
    if (residual->kind == PINN_RES_AFFINE) {
        for (int s = 0; s < PINN_MAX_STREAMS; ++s) {
            a.coef[s] = (s < s_user) ? residual->coef[s] : 0.0f;
            a.coef_row[s] = (s < s_user) ? residual->coef_row[s] : -1;
            if (a.coef_row[s] >= residual->n_aux) return fail("coef_row[%d] refers to a missing pre-pass row", s);
        }
        a.src_const = residual->src_const;
        a.src_row = residual->src_row;
        if (a.src_row >= residual->n_aux) return fail("src_row refers to a missing pre-pass row");
    } else {
        const pinn_program_t* program = &residual->program;
        if (program->n_ops < 1) return fail("empty residual program");
        if (check_program(*program, s_user + d + residual->n_aux + residual->n_vars, PINN_MAX_CONSTS, false, 0, "residual")) return 1;
        // the program addresses registers with the caller's stream count; re-base everything behind the streams
        // onto the instantiation's stream count (extra second-derivative streams sit in between)
        a.prog = *program;
        for (int i = 0; i < program->n_ops; ++i) {
            const uint32_t w = program->code[i];
            int op = w & 255, dst = (w >> 8) & 255, ra = (w >> 16) & 255, rb = (w >> 24) & 255;
            auto fix = [&](int r) { return r >= s_user ? r + shift : r; };
            const bool b_is_reg = op == PINN_OP_ADD || op == PINN_OP_SUB || op == PINN_OP_MUL || op == PINN_OP_DIV;
            dst = fix(dst);
            if (op != PINN_OP_CONST) ra = fix(ra);
            if (b_is_reg) rb = fix(rb);
            if (dst >= PINN_MAX_REGS || ra >= PINN_MAX_REGS || (b_is_reg && rb >= PINN_MAX_REGS))
                return fail("program instruction %d uses a register >= %d after re-basing", i, PINN_MAX_REGS);
            a.prog.code[i] = (uint32_t)op | ((uint32_t)dst << 8) | ((uint32_t)ra << 16) | ((uint32_t)rb << 24);
        }
    }
    a.mode = PINN_MODE_STEP;
    a.inv_n = inv_n_global;
    // criterion of the step (include/pinn.h PINN_CRIT_*; all zero: mean-square)
    if (residual->criterion < PINN_CRIT_MSE || residual->criterion > PINN_CRIT_LAST) return fail("unknown criterion code %d", residual->criterion);
    if (residual->criterion == PINN_CRIT_HUBER && !(residual->crit_param > 0.0f)) return fail("HuberLoss needs delta > 0 (crit_param=%g)", (double)residual->crit_param);
    if (residual->criterion == PINN_CRIT_SMOOTH_L1 && !(residual->crit_param >= 0.0f)) return fail("SmoothL1Loss needs beta >= 0 (crit_param=%g)", (double)residual->crit_param);
    a.crit = residual->criterion;
    a.crit_param = residual->crit_param;
    if (a.crit == PINN_CRIT_SMOOTH_L1 && a.crit_param == 0.0f) a.crit = PINN_CRIT_L1;      // (as torch: smooth_l1_loss with beta 0 is l1_loss)
    if (a.crit == PINN_CRIT_MSE || a.crit == PINN_CRIT_L1) a.crit_param = 0.0f;
    if (make_plan(net, n_points, nd, n2, &plan, PINN_MODE_STEP, residual->kind, comb, &a)) return 1;      // with the call's own arguments
    return run_train(net, &a, plan, nd, c.grads, accumulate, c.workspace, c.workspace_bytes, c.stream, &residual->pre, tail, residual->pre_consts64);
}

int pinn_residual_step(pinn_t* net, const pinn_residual_t* residual, const float* params, const float* xs,
                       int64_t n_points, const int* dir_cols, int nd, int n2, const float* ic_streams, float ic_const,
                       float inv_n_global, float* grads, void* workspace, size_t workspace_bytes, void* stream) {
    const StepCall c = {net, residual, params, xs, n_points, dir_cols, nd, n2, ic_streams, ic_const, grads, workspace, workspace_bytes, stream};
    return residual_step_impl(c, inv_n_global, nullptr);
}

int pinn_residual_step_add(pinn_t* net, const pinn_residual_t* residual, const float* params, const float* xs,
                           int64_t n_points, const int* dir_cols, int nd, int n2, const float* ic_streams, float ic_const,
                           float inv_n_global, float* grads, void* workspace, size_t workspace_bytes, void* stream) {
    const StepCall c = {net, residual, params, xs, n_points, dir_cols, nd, n2, ic_streams, ic_const, grads, workspace, workspace_bytes, stream};
    return residual_step_impl(c, inv_n_global, nullptr, 1);
}

// one whole iteration with the update of `tail` in the last reduction launch (the rule has been through optim_prepare)
static int residual_optim_step(const StepCall& c, StepTail* tail) {
    if (!c.net || !tail->m || !tail->v || !tail->step_ptr) return fail("null argument");
    if (tail->step_value < 1) return fail("step must be >= 1");
    tail->off_loss = c.net->lay.off_loss;
    // (reduction='sum', pinn_residual_t::crit_sum: no division by the number of points)
    return residual_step_impl(c, (c.residual && c.residual->crit_sum) ? 1.0f : 1.0f / (float)c.n_points, tail);
}

int pinn_residual_optim_step(pinn_t* net, const pinn_residual_t* residual, float* params, const float* xs,
                             int64_t n_points, const int* dir_cols, int nd, int n2, const float* ic_streams,
                             float ic_const, float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* mask,
                             int32_t* step_ptr, int32_t step, const pinn_optim_t* opt, float* loss_out, void* workspace,
                             size_t workspace_bytes, void* stream) {
    PinnOptK k;
    if (optim_prepare(opt, &k)) return 1;
    const StepCall c = {net, residual, params, xs, n_points, dir_cols, nd, n2, ic_streams, ic_const, grads, workspace, workspace_bytes, stream};
    StepTail tail = update_tail({params, exp_avg, exp_avg_sq, mask, step_ptr}, step, k, loss_out);
    return residual_optim_step(c, &tail);
}

// the sampler description of a fit chunk in the form the reduction's tail takes (non-zero: columns it cannot draw)
static int fit_next_spec(const FitCall& f, PinnNextBatch* out) {
    const pinn_net* net = f.step.net;
    if (!net || !f.xs || !f.kind || !f.a || !f.b || f.step.n_points <= 0 || net->lay.d < 1 || net->lay.d > PINN_MAX_INPUTS) return 1;
    memset(out, 0, sizeof(*out));
    out->xs = f.xs; out->n = (long long)f.step.n_points; out->spec.d = net->lay.d;
    for (int c = 0; c < net->lay.d; ++c) {
        if (f.kind[c] < PINN_SAMPLE_UNIFORM || f.kind[c] > PINN_SAMPLE_CONST) return 1;
        out->spec.kind[c] = f.kind[c]; out->spec.a[c] = f.a[c]; out->spec.b[c] = f.b[c];
    }
    out->k0 = (unsigned)(f.seed & 0xffffffffull); out->k1 = (unsigned)(f.seed >> 32);
    return 0;
}

// does a fused step of this batch run as ONE tile pass + ONE reduction (not chunk by chunk)?
static bool single_pass_step(const StepCall& c) {
    if (!c.residual) return false;
    Plan plan;
    if (make_plan(c.net, c.n_points, c.nd, c.n2, &plan, PINN_MODE_STEP, c.residual->kind, c.residual->combined ? 1 : 0, nullptr)) return false;
    return plan.chunk_tiles >= plan.ntiles;
}

// K iterations of the reference's fit loop (model_torch.py:426-464): sample, fused step, update. Nothing here waits for the device.
// `capture` nullptr, the eager loop on `stream`: what changes from one iteration to the next (Philox batch counter, step, slot of the loss
// history) travels by value. `capture` a control block, the same loop recorded on a capturing `stream`: those values are placeholders
// (0, 1, loss_history) and the launches read the real ones from the block at index k.
// From the second iteration on the batch is drawn by the reduction launch of the iteration before (pinn_reduce_kernel's tail: the tile
// kernel of that iteration is through with the buffer), which saves every iteration one dependent launch -- where the step is one pass
// (a chunked WGX step reduces several times per iteration: those keep the sampler launch). The LAST reduction draws nothing.
static int enqueue_chunk(const FitCall& f, void* stream, const PinnFitCtrl* capture) {
    StepCall c = f.step;
    c.stream = stream;
    PinnNextBatch next = {nullptr, 0, {}, 0u, 0u, 0ull};
    const bool hand_over = fit_next_spec(f, &next) == 0 && single_pass_step(c);
    int rc = 0;
    for (int32_t k = 0; k < f.k_steps && !rc; ++k) {
        const uint64_t call = capture ? 0 : f.call_index0 + (uint64_t)k;
        const int capture_k = capture ? k : 0;
        if (k == 0 || !hand_over) rc = sample_points(f.xs, c.n_points, c.net->lay.d, f.kind, f.a, f.b, f.seed, call, stream, capture, capture_k);
        if (rc) break;
        // (a schedule: iteration k is the step of pinn_residual_optim_step with opt->lr = lr_steps[k])
        StepTail tail = capture ? update_tail(f.state, 1, f.opt, f.loss_history)
                                : update_tail(f.state, f.step0 + k, f.lr_steps ? optim_at_rate(f.opt, f.lr_steps[k]) : f.opt, f.loss_history + k);
        if (hand_over && k + 1 < f.k_steps) { tail.next = next; tail.next.call = capture ? 0 : call + 1; }
        tail.capture = capture; tail.capture_k = capture_k;
        rc = residual_optim_step(c, &tail);
    }
    return rc;
}

// the eager loop: the chunk without a control block, and the fallback of the other forms (pinn_fit_steps has checked the arguments)
static int fit_steps_eager(const FitCall& f) { return enqueue_chunk(f, f.step.stream, nullptr); }

size_t pinn_fit_ctrl_bytes(void) { return sizeof(PinnFitCtrl); }

static int g_fit_graph_stats[4] = {0, 0, 0, 0};      // chunks replayed, graphs captured, captures refused, last HIP error of a refusal
int pinn_debug_fit_graph_stats(int32_t out[4]) {
    if (!out) return fail("null argument");
    for (int i = 0; i < 4; ++i) out[i] = g_fit_graph_stats[i];
    return 0;
}

static int launch_fit_ctrl(const FitCall& f) {
    PinnFitCtrlArgs ca;
    fit_ctrl_fill(&ca, f);
    return launch("control-block", pinn_fit_ctrl_kernel, 1, 128, 0, f.step.stream, reinterpret_cast<PinnFitCtrl*>(f.ctrl), ca);
}

// narrow nets, batches of a few tiles: the whole chunk -- any length up to PINN_FIT_CHUNK_MAX -- as ONE launch (pinn_fit_kernel.h); the
// eager loop's trajectory to fp32 round-off. `launched` false with 0 returned: the chunk does not qualify and is still to be run
static int try_one_launch_chunk(const FitCall& f, bool* launched) {
    const pinn_net* net = f.step.net;
    *launched = false;
    g_fit_last_sync = nullptr;          // (a chunk that declines, or takes the one-CU form, leaves no flag of an earlier call behind)
    OneLaunch one;
    memset(&one, 0, sizeof(one));
    PinnNextBatch spec_probe = {nullptr, 0, {}, 0u, 0u, 0ull};
    if (net->fit_persistent && net->lay.hp <= 32 && f.ctrl && f.ctrl_bytes >= sizeof(PinnFitCtrl) && f.k_steps >= 1 && f.k_steps <= PINN_FIT_CHUNK_MAX &&
        !g_profile && !g_phase_prof && f.step.residual && f.state.params && f.step.grads && f.state.exp_avg && f.state.exp_avg_sq && f.state.step_ptr &&
        fit_next_spec(f, &spec_probe) == 0) {
        PinnFitP& P = one.p;
        P.ctrl = reinterpret_cast<PinnFitCtrl*>(f.ctrl); P.k_steps = f.k_steps; P.xs = f.xs; P.n = (long long)f.step.n_points; P.spec = spec_probe.spec;
        if (launch_fit_ctrl(f)) return 1;
        StepTail tail = update_tail(f.state, f.step0, f.opt, f.loss_history);
        tail.persist = &one;
        if (const int rc = residual_optim_step(f.step, &tail)) return rc;
        if (one.launched) { ++g_fit_graph_stats[0]; *launched = true; }         // (counted with the replayed chunks: one launch for the chunk)
    }
    return 0;
}

#ifndef PINN_EMU
// FNV-1a over the bytes of everything a captured chunk depends on
static void key_mix(unsigned long long (&key)[4], const void* p, size_t n) {
    const unsigned char* b = reinterpret_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) {
        unsigned long long& h = key[i & 3];
        h = (h ^ b[i]) * 1099511628211ull;
    }
}

// everything the captured launches carry BY VALUE or by address (the per-iteration values travel through the control block)
static void chunk_replay_key(const FitCall& f, int dev, unsigned long long (&key)[4]) {
    const StepCall& c = f.step;
    const pinn_net* net = c.net;
    const unsigned long long seed[4] = {14695981039346656037ull, 14695981039346656037ull ^ 1, 14695981039346656037ull ^ 2, 14695981039346656037ull ^ 3};
    memcpy(key, seed, sizeof(seed));
    key_mix(key, c.residual, sizeof(*c.residual));
    const void* ptrs[] = {f.state.params, f.xs, c.grads, f.state.exp_avg, f.state.exp_avg_sq, f.state.mask, f.state.step_ptr, c.workspace, f.ctrl, c.stream};
    key_mix(key, ptrs, sizeof(ptrs));
    // (not the sampler's key `seed`: it travels through the control block, so the chunk recorded by one fit call is replayed by the next)
    const long long ints[] = {(long long)c.n_points, c.nd, c.n2, (long long)c.workspace_bytes, net->gemm_mode, net->tanh_mode, net->max_per_cu,
                              net->prepass_in_kernel, (long long)net->wgx_chunk_bytes};
    key_mix(key, ints, sizeof(ints));
    const float flts[] = {c.ic_const, c.residual->crit_param};
    // (the update rule with its hyper-parameters: the reductions of the recorded chunk carry it by value. Under a control block they
    //  read the learning rate and what derives from it -- step_size, decay -- from the block, never from that copy: a call with a
    //  schedule keys on the rule WITHOUT them, so chunks that differ only in their rates replay one recording)
    PinnOptK key_opt = f.opt;
    if (f.lr_steps) { key_opt.lr = 0.0f; key_opt.decay = 0.0f; key_opt.pad = 1; }
    key_mix(key, &key_opt, sizeof(key_opt));
    // (the criterion is part of `residual`, hashed above; named here once more so that the key does not depend on where the fields sit)
    const int crit_key[] = {c.residual->criterion, c.residual->crit_sum};
    key_mix(key, crit_key, sizeof(crit_key));
    key_mix(key, flts, sizeof(flts));
    key_mix(key, f.kind, sizeof(int) * net->lay.d); key_mix(key, f.a, sizeof(float) * net->lay.d); key_mix(key, f.b, sizeof(float) * net->lay.d);
    key_mix(key, c.dir_cols, sizeof(int) * (c.nd > 0 ? c.nd : 0));
    key_mix(key, &dev, sizeof(dev));
}

// record the chunk as a launch graph for the next chunks to replay. 0 also where the runtime refuses the capture (counted in
// g_fit_graph_stats): the chunk at hand has already run eagerly
static int capture_chunk(const FitCall& f, int dev, const unsigned long long (&key)[4]) {
    pinn_net* net = f.step.net;
    hipGraph_t graph = nullptr;
    // capture happens on a stream of the library's own (torch's current stream is usually the legacy default stream, which cannot
    // capture); nothing EXECUTES on it -- the nodes are kernel launches without a stream of their own, the graph is launched on the caller's
    static thread_local hipStream_t cap_streams[64] = {nullptr};
    hipStream_t& cs = cap_streams[dev & 63];
    if (!cs && hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); ++g_fit_graph_stats[2]; return 0; }
    const hipError_t be = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
    if (be != hipSuccess) { (void)hipGetLastError(); ++g_fit_graph_stats[2]; g_fit_graph_stats[3] = (int)be; return 0; }
    const int crc = enqueue_chunk(f, cs, reinterpret_cast<PinnFitCtrl*>(f.ctrl));
    const hipError_t ce = hipStreamEndCapture(cs, &graph);
    if (crc || ce != hipSuccess || !graph) {
        (void)hipGetLastError(); ++g_fit_graph_stats[2]; g_fit_graph_stats[3] = crc ? -crc : (int)ce;
        if (graph) (void)hipGraphDestroy(graph);
        return crc ? crc : 0;
    }
    hipGraphExec_t exec = nullptr;
    const hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (ie != hipSuccess) { (void)hipGetLastError(); ++g_fit_graph_stats[2]; g_fit_graph_stats[3] = (int)ie; (void)hipGraphDestroy(graph); return 0; }
    (void)hipGraphDestroy(graph);
    net->fit_graph_exec = exec;
    ++g_fit_graph_stats[1];
    net->fit_graph_k = f.k_steps;
    memcpy(net->fit_graph_key, key, sizeof(key));
    return 0;
}

// the graph pays where launch gaps are a visible share of an iteration; chunks that do not qualify run the eager loop
// (only whole chunks: the tail of a fit would capture a graph of its own that nothing replays)
static int replay_chunk(const FitCall& f) {
    pinn_net* net = f.step.net;
    if (f.k_steps != PINN_FIT_CHUNK_MAX || !f.ctrl || f.ctrl_bytes < sizeof(PinnFitCtrl) || g_profile || g_phase_prof) return fit_steps_eager(f);
    int dev = 0;
    (void)hipGetDevice(&dev);
    unsigned long long key[4];
    chunk_replay_key(f, dev, key);
    const bool hit = net->fit_graph_exec && net->fit_graph_k == f.k_steps && memcmp(key, net->fit_graph_key, sizeof(key)) == 0;
    if (!hit) {
        if (net->fit_graph_exec) { (void)hipGraphExecDestroy((hipGraphExec_t)net->fit_graph_exec); net->fit_graph_exec = nullptr; }
        // one eager iteration's worth of planning has to have happened (function attributes, occupancy queries are not capturable):
        // the first chunk of a configuration runs eagerly AND is followed by the capture of the graph the next chunks replay
        if (const int rc = fit_steps_eager(f)) return rc;
        return capture_chunk(f, dev, key);
    }
    if (launch_fit_ctrl(f)) return 1;
    if (hipGraphLaunch((hipGraphExec_t)net->fit_graph_exec, (hipStream_t)f.step.stream) != hipSuccess) return fail("hipGraphLaunch failed");
    ++g_fit_graph_stats[0];
    return 0;
}
#endif

int pinn_fit_steps(pinn_t* net, const pinn_residual_t* residual, float* params, float* xs, int64_t n_points,
                   const int* kind, const float* a, const float* b, uint64_t seed, uint64_t call_index0,
                   const int* dir_cols, int nd, int n2, float ic_const, float* grads, float* exp_avg, float* exp_avg_sq,
                   const uint8_t* mask, int32_t* step_ptr, int32_t step0, const pinn_optim_t* opt,
                   float* loss_history, int32_t k_steps, void* workspace, size_t workspace_bytes, void* ctrl,
                   size_t ctrl_bytes, void* stream, const float* lr_steps) {
    PinnOptK k;
    if (optim_prepare(opt, &k)) return 1;
    const FitCall f = {{net, residual, params, xs, n_points, dir_cols, nd, n2, nullptr, ic_const, grads, workspace, workspace_bytes, stream},
                       xs, kind, a, b, seed, call_index0, {params, exp_avg, exp_avg_sq, mask, step_ptr}, step0, k, loss_history, k_steps,
                       ctrl, ctrl_bytes, lr_steps};
    if (!net || !xs || !loss_history) return fail("null argument");
    // (without a control block the chunk is the eager loop alone, which reads dir_cols only for nd > 0 and, at k_steps == 0, nothing but
    //  the three above: such calls are accepted as they always were)
    if ((ctrl || k_steps != 0) && (!residual || !kind || !a || !b || (!dir_cols && (ctrl || nd > 0)))) return fail("null argument");
    if (k_steps < 0 || step0 < 1) return fail("k_steps must be >= 0 and step0 >= 1");
    if (check_lr_steps(lr_steps, k_steps)) return 1;
    bool launched = false;
    if (const int rc = try_one_launch_chunk(f, &launched)) return rc;
    if (launched) return 0;
#ifdef PINN_EMU
    return fit_steps_eager(f);      // (no launch graphs in the emulator)
#else
    return replay_chunk(f);
#endif
}

static int optim_launch(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* mask, int64_t n,
                        int32_t* step_ptr, int32_t step, const PinnOptK& opt, void* stream,
                        float* loss_out = nullptr, int off_loss = -1) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !step_ptr) return fail("null argument");
    if (n <= 0) return 0;
    const int blocks = (int)((n + 255) / 256);
    float step_size = 0.0f, bc2_sqrt = 1.0f;
    if (step > 0) optim_scalars(opt, (double)step, &step_size, &bc2_sqrt);
    if (step <= 0 && launch("optimizer kernel", pinn_tick_kernel, 1, 64, 0, stream, (int*)step_ptr)) return 1;
    return launch("optimizer kernel", pinn_optim_kernel, blocks, 256, 0, stream, params, grads, exp_avg, exp_avg_sq, mask, (long long)n,
                  (int*)step_ptr, (int)step, step_size, bc2_sqrt, opt, loss_out, off_loss);
}

int pinn_optim_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* mask, int64_t n,
                    int32_t* step_ptr, const pinn_optim_t* opt, void* stream) {
    PinnOptK k;
    if (optim_prepare(opt, &k)) return 1;
    return optim_launch(params, grads, exp_avg, exp_avg_sq, mask, n, step_ptr, 0, k, stream);
}

int pinn_optim_step_at(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* mask, int64_t n,
                       int32_t* step_ptr, int32_t step, const pinn_optim_t* opt, float* loss_out, int32_t off_loss, void* stream) {
    PinnOptK k;
    if (optim_prepare(opt, &k)) return 1;
    if (step < 1) return fail("step must be >= 1");
    if (loss_out && (off_loss < 0 || off_loss >= n)) return fail("off_loss=%d outside the gradient buffer", off_loss);
    return optim_launch(params, grads, exp_avg, exp_avg_sq, mask, n, step_ptr, step, k, stream, loss_out, off_loss);
}

int pinn_reduce_rows(const float* partials, int32_t n_rows, int32_t row_len, float* grads, int accumulate, float* params, float* exp_avg,
                     float* exp_avg_sq, const uint8_t* mask, int32_t* step_ptr, int32_t step, const pinn_optim_t* opt, float* loss_out,
                     int32_t off_loss, void* stream) {
    if (!partials || !grads) return fail("null argument");
    if (n_rows < 1 || row_len < 1) return fail("n_rows=%d, row_len=%d: both must be >= 1", n_rows, row_len);
    if (loss_out && (off_loss < 0 || off_loss >= row_len)) return fail("off_loss=%d outside the gradient buffer", off_loss);
    if (!opt) {
        if (loss_out) return fail("loss_out rides in the update's launch: it needs an optimizer description");
        return launch_reduce(partials, n_rows, row_len, grads, accumulate ? 1 : 0, stream);
    }
    PinnOptK k;
    if (optim_prepare(opt, &k)) return 1;
    if (!params || !exp_avg || !exp_avg_sq || !step_ptr) return fail("null argument");
    if (step < 1) return fail("step must be >= 1");
    const StepTail tail = update_tail({params, exp_avg, exp_avg_sq, mask, step_ptr}, step, k, loss_out, loss_out ? off_loss : -1);
    return launch_reduce(partials, n_rows, row_len, grads, accumulate ? 1 : 0, stream, &tail);
}

// ---- L-BFGS direction (pinn_lbfgs_kernels.h): three launches per inner iteration, whatever the history size --------------------------
static size_t lbfgs_ctrl_doubles(int m) { return (size_t)PINN_LBFGS_CTRL_HEAD + 2 * (size_t)m + 2 * (size_t)m * m; }

size_t pinn_lbfgs_ctrl_bytes(int32_t history) {
    if (history < 1 || history > PINN_LBFGS_MAX_HISTORY) return 0;
    return lbfgs_ctrl_doubles(history) * sizeof(double);
}

size_t pinn_lbfgs_workspace_bytes(int64_t n, int32_t history) {
    if (n < 1 || history < 1 || history > PINN_LBFGS_MAX_HISTORY) return 0;
    const size_t rows = (size_t)((n + PINN_LBFGS_DOTS_SLICE - 1) / PINN_LBFGS_DOTS_SLICE);
    return rows * (5 * (size_t)history + PINN_LBFGS_ROW_TAIL) * sizeof(double);
}

int pinn_lbfgs_direction(float* params, const float* grads, float* prev_grad, float* d, float* s_ring, float* y_ring, const uint8_t* mask,
                         int64_t n, int64_t ld, int32_t history, int32_t mode, int32_t apply_step, int32_t off_loss, float t, double lr,
                         double tolerance_grad, double tolerance_change, void* ctrl, size_t ctrl_bytes, void* workspace,
                         size_t workspace_bytes, void* stream) {
    if (!params || !grads || !prev_grad || !d || !s_ring || !y_ring || !ctrl || !workspace) return fail("null argument");
    if (history < 1 || history > PINN_LBFGS_MAX_HISTORY)
        return fail("L-BFGS history_size=%d outside [1, %d]", history, PINN_LBFGS_MAX_HISTORY);
    if (n < 1 || n > (int64_t)1 << 40) return fail("L-BFGS: n=%lld entries", (long long)n);
    if (ld < n || ld % 4 != 0) return fail("L-BFGS: row stride %lld of the rings must be a multiple of 4 and at least n=%lld", (long long)ld, (long long)n);
    if (off_loss < 0 || off_loss >= n) return fail("off_loss=%d outside the gradient buffer", off_loss);
    if (mode != 0 && mode != 1) return fail("L-BFGS: mode=%d (0: first evaluation of a step, 1: inside its loop)", mode);
    if (!(lr >= 0.0)) return fail("L-BFGS: invalid learning rate %g", lr);
    const void* aligned[] = {params, grads, prev_grad, d, s_ring, y_ring, ctrl, workspace};
    for (const void* p : aligned)
        if (reinterpret_cast<uintptr_t>(p) & 15) return fail("L-BFGS: buffers must be 16-byte aligned");
    if (ctrl_bytes < pinn_lbfgs_ctrl_bytes(history)) return fail("L-BFGS: control block too small (%zu < %zu bytes)", ctrl_bytes, pinn_lbfgs_ctrl_bytes(history));
    if (workspace_bytes < pinn_lbfgs_workspace_bytes(n, history))
        return fail("workspace too small (%zu < %zu bytes)", workspace_bytes, pinn_lbfgs_workspace_bytes(n, history));
    const int m = history, rowlen = 5 * m + PINN_LBFGS_ROW_TAIL;
    const int blocks = (int)((n + PINN_LBFGS_SLICE - 1) / PINN_LBFGS_SLICE);                   // the combine pass
    const int rows = (int)((n + PINN_LBFGS_DOTS_SLICE - 1) / PINN_LBFGS_DOTS_SLICE);           // the dots pass: one row of partial sums each
    PinnLbfgsArgs A = {params, grads, prev_grad, d, s_ring, y_ring, mask, (long long)n, (long long)ld, m, mode, apply_step ? 1 : 0, off_loss, t,
                       lr, tolerance_grad, tolerance_change, static_cast<double*>(ctrl), static_cast<double*>(workspace), rows};
    const size_t smem_dots = 4 * (size_t)rowlen * sizeof(double);
    const size_t smem_fin = ((size_t)rowlen + 7 * (size_t)m + (size_t)m * m) * sizeof(double);
#ifndef PINN_EMU
    // (the finalize pass stages the s.y matrix in LDS: above 64 KB from history_size 85; the attribute is raised once per device and size)
    static std::atomic<size_t> fin_attr[64];                  // (host threads may race to their first call: the worst case is the attribute set twice)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return fail("L-BFGS: no current device");
    if (smem_fin > 48 * 1024 && smem_fin > fin_attr[dev].load(std::memory_order_relaxed)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(pinn_lbfgs_finalize_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)smem_fin) != hipSuccess)
            return fail("L-BFGS: %zu bytes of LDS for history_size=%d refused", smem_fin, m);
        fin_attr[dev].store(smem_fin, std::memory_order_relaxed);
    }
#endif
    if (launch("L-BFGS kernel", pinn_lbfgs_dots_kernel, rows, PINN_LBFGS_THREADS, smem_dots, stream, A) ||
        launch("L-BFGS kernel", pinn_lbfgs_finalize_kernel, 1, PINN_LBFGS_THREADS, smem_fin, stream, A))
        return 1;
    return launch("L-BFGS kernel", pinn_lbfgs_combine_kernel, blocks, PINN_LBFGS_THREADS, 0, stream, A);
}

// ---- loss-term weights (pinn_balance_kernels.h): three launches per call, whatever the number of terms ---------------------------------
static_assert(PINN_BALANCE_STATE_DOUBLES % 2 == 0, "the state block is a whole number of 16-byte pieces");

size_t pinn_balance_state_bytes(int32_t n_terms) {
    if (n_terms < 1 || n_terms > PINN_BALANCE_MAX_TERMS) return 0;
    return (size_t)PINN_BALANCE_STATE_DOUBLES * sizeof(double);
}

size_t pinn_balance_workspace_bytes(int64_t n, int32_t n_terms) {
    if (n < 1 || n > (int64_t)1 << 40 || n_terms < 1 || n_terms > PINN_BALANCE_MAX_TERMS) return 0;
    const size_t rows = (size_t)((n + PINN_BALANCE_STATS_SLICE - 1) / PINN_BALANCE_STATS_SLICE);
    return (rows * (size_t)PINN_BALANCE_ROWLEN(n_terms) * sizeof(double) + 15) / 16 * 16;
}

int pinn_balance_init(void* state, size_t state_bytes, int32_t n_terms, const double* weights, void* stream) {
    if (n_terms < 1 || n_terms > PINN_BALANCE_MAX_TERMS)
        return fail("loss weights: n_terms=%d outside [1, %d]", n_terms, PINN_BALANCE_MAX_TERMS);
    if (!state || !weights) return fail("loss weights: null argument");
    if (reinterpret_cast<uintptr_t>(state) & 15) return fail("loss weights: the state block must be 16-byte aligned");
    if (state_bytes < pinn_balance_state_bytes(n_terms))
        return fail("loss weights: state block too small (%zu < %zu bytes)", state_bytes, pinn_balance_state_bytes(n_terms));
    PinnBalanceArgs A = {};
    A.T = n_terms;
    A.state = static_cast<double*>(state);
    for (int j = 0; j < n_terms; ++j) {
        if (!(weights[j] >= 0.0 && weights[j] <= DBL_MAX)) return fail("loss weights: weight %d is %g; a weight is finite and not negative", j, weights[j]);
        A.init[j] = weights[j];
    }
    return launch("loss-weight kernel", pinn_balance_init_kernel, 1, PINN_BALANCE_THREADS, 0, stream, A);
}

int pinn_balance_terms(const float* term_grads, int64_t ld, int32_t n_terms, int64_t n, const uint8_t* mask, int32_t off_loss, int32_t kind,
                       int32_t ref_term, int32_t update, double momentum, double lo, double hi, void* state, size_t state_bytes,
                       float* grads_out, float* term_loss_out, float* weight_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_terms < 1 || n_terms > PINN_BALANCE_MAX_TERMS)
        return fail("loss weights: n_terms=%d outside [1, %d]", n_terms, PINN_BALANCE_MAX_TERMS);
    if (!term_grads || !state || !grads_out || !workspace) return fail("loss weights: null argument");
    if (n < 1 || n > (int64_t)1 << 40) return fail("loss weights: n=%lld entries", (long long)n);
    if (ld < n || ld % 4 != 0)
        return fail("loss weights: row stride %lld of the term rows must be a multiple of 4 and at least n=%lld", (long long)ld, (long long)n);
    if (off_loss < 0 || off_loss >= n) return fail("off_loss=%d outside the gradient buffer", off_loss);
    if (kind != PINN_BALANCE_FIXED && kind != PINN_BALANCE_MAX_MEAN && kind != PINN_BALANCE_NORM)
        return fail("loss weights: unknown kind %d (0 fixed, 1 max / mean, 2 norm)", kind);
    if (ref_term < 0 || ref_term >= n_terms) return fail("loss weights: ref_term=%d outside [0, %d)", ref_term, n_terms);
    if (!(momentum >= 0.0 && momentum <= 1.0)) return fail("loss weights: momentum=%g outside [0, 1]", momentum);
    if (!(lo >= 0.0 && lo <= hi && hi <= DBL_MAX)) return fail("loss weights: clip [%g, %g] must be finite with 0 <= lo <= hi", lo, hi);
    const void* aligned[] = {term_grads, state, grads_out, workspace};
    for (const void* p : aligned)
        if (reinterpret_cast<uintptr_t>(p) & 15) return fail("loss weights: buffers must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(term_loss_out) | reinterpret_cast<uintptr_t>(weight_out)) & 3)
        return fail("loss weights: term_loss_out and weight_out must be 4-byte aligned");
    // the combine pass reads entry i of every row and writes entry i of the output in ONE thread, reads first: the output may be row 0
    // itself. Any other overlap with the term rows would have one workgroup write what another still reads: refused.
    const float* rows_end = term_grads + (size_t)(n_terms - 1) * (size_t)ld + (size_t)n;
    if (grads_out != term_grads && grads_out < rows_end && grads_out + n > term_grads)
        return fail("loss weights: grads_out overlaps the term rows (it may be row 0 itself, nothing else of them)");
    if (state_bytes < pinn_balance_state_bytes(n_terms))
        return fail("loss weights: state block too small (%zu < %zu bytes)", state_bytes, pinn_balance_state_bytes(n_terms));
    if (workspace_bytes < pinn_balance_workspace_bytes(n, n_terms))
        return fail("workspace too small (%zu < %zu bytes)", workspace_bytes, pinn_balance_workspace_bytes(n, n_terms));
    const int blocks = (int)((n + PINN_BALANCE_SLICE - 1) / PINN_BALANCE_SLICE);                       // the combine pass
    const int rows = (int)((n + PINN_BALANCE_STATS_SLICE - 1) / PINN_BALANCE_STATS_SLICE);             // the stats pass: one row of partials each
    PinnBalanceArgs A = {};
    A.g = term_grads; A.out = grads_out; A.mask = mask; A.n = (long long)n; A.ld = (long long)ld;
    A.T = n_terms; A.off_loss = off_loss; A.kind = kind; A.ref = ref_term; A.update = update ? 1 : 0;
    A.momentum = momentum; A.lo = lo; A.hi = hi;
    A.state = static_cast<double*>(state); A.rows = static_cast<double*>(workspace); A.n_rows = rows;
    A.term_loss_out = term_loss_out; A.weight_out = weight_out;
    const size_t rowlen = (size_t)PINN_BALANCE_ROWLEN(n_terms);
    if (launch("loss-weight kernel", pinn_balance_stats_kernel, rows, PINN_BALANCE_THREADS, 4 * rowlen * sizeof(double), stream, A) ||
        launch("loss-weight kernel", pinn_balance_finalize_kernel, 1, PINN_BALANCE_THREADS, rowlen * sizeof(double), stream, A))
        return 1;
    return launch("loss-weight kernel", pinn_balance_combine_kernel, blocks, PINN_BALANCE_THREADS, 0, stream, A);
}

// ---- causal training weights (pinn_causal_kernels.h): three launches per call, whatever n and the number of bins -----------------------
static_assert(PINN_CAUSAL_STATE_DOUBLES % 2 == 0, "the state block is a whole number of 16-byte pieces");
#define PINN_CAUSAL_MAX_POINTS ((int64_t)1 << 30)

// chunks of 256 points per workgroup of the stats pass, and the workgroups (= rows of partials) that gives
static void causal_fold(int64_t n, int* chunks, int* rows) {
    const int64_t all = (n + PINN_CAUSAL_THREADS - 1) / PINN_CAUSAL_THREADS;
    *chunks = (int)((all + PINN_CAUSAL_MAX_ROWS - 1) / PINN_CAUSAL_MAX_ROWS);
    *rows = (int)((all + *chunks - 1) / *chunks);
}

static bool causal_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a && b && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

size_t pinn_causal_state_bytes(void) { return (size_t)PINN_CAUSAL_STATE_DOUBLES * sizeof(double); }

size_t pinn_causal_workspace_bytes(int64_t n, int32_t bins) {
    if (n < 0 || n > PINN_CAUSAL_MAX_POINTS || bins < 1 || bins > PINN_CAUSAL_MAX_BINS) return 0;
    int chunks = 1, rows = 1;
    if (n > 0) causal_fold(n, &chunks, &rows);
    return (size_t)rows * (size_t)PINN_CAUSAL_ROWLEN(bins) * sizeof(double);
}

int pinn_causal_init(void* state, size_t state_bytes, const double* eps_ladder, int32_t n_eps, double delta, void* stream) {
    if (!state || !eps_ladder) return fail("causal weights: null argument");
    if (n_eps < 1 || n_eps > PINN_CAUSAL_MAX_EPS) return fail("causal weights: a ladder of %d tolerances; 1 to %d", n_eps, PINN_CAUSAL_MAX_EPS);
    if (reinterpret_cast<uintptr_t>(state) & 15) return fail("causal weights: the state block must be 16-byte aligned");
    if (state_bytes < pinn_causal_state_bytes())
        return fail("causal weights: state block too small (%zu < %zu bytes)", state_bytes, pinn_causal_state_bytes());
    if (delta != delta) return fail("causal weights: delta is not a number");
    PinnCausalArgs A = {};
    A.state = static_cast<double*>(state); A.n_eps = n_eps; A.delta = delta;
    for (int j = 0; j < n_eps; ++j) {
        if (!(eps_ladder[j] >= 0.0 && eps_ladder[j] <= DBL_MAX))
            return fail("causal weights: tolerance %d is %g; a tolerance is finite and not negative", j, eps_ladder[j]);
        A.ladder[j] = eps_ladder[j];
    }
    return launch("causal-weight kernel", pinn_causal_init_kernel, 1, PINN_CAUSAL_THREADS, 0, stream, A);
}

int pinn_causal_weights(const float* t, int64_t t_stride, const float* r, int64_t n, int32_t bins, double t_lo, double t_hi, int32_t update,
                        void* state, size_t state_bytes, float* w_out, float* bin_weight_out, float* eps_out, float* mean_sq_out,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (bins < 1 || bins > PINN_CAUSAL_MAX_BINS) return fail("causal weights: bins=%d outside [1, %d]", bins, PINN_CAUSAL_MAX_BINS);
    if (n < 0 || n > PINN_CAUSAL_MAX_POINTS) return fail("causal weights: n=%lld points outside [0, %lld]", (long long)n, (long long)PINN_CAUSAL_MAX_POINTS);
    if (!t || !r || !state || !w_out || !workspace) return fail("causal weights: null argument");
    if (t_stride < 1 || t_stride > PINN_CAUSAL_MAX_STRIDE)
        return fail("causal weights: t_stride=%lld (floats between two times) outside [1, %lld]", (long long)t_stride, (long long)PINN_CAUSAL_MAX_STRIDE);
    if (!(t_lo < t_hi && t_lo >= -DBL_MAX && t_hi <= DBL_MAX))
        return fail("causal weights: the time domain [%g, %g] must be finite with t_lo < t_hi", t_lo, t_hi);
    if ((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(workspace)) & 15)
        return fail("causal weights: state and workspace must be 16-byte aligned");
    const void* floats[] = {t, r, w_out, bin_weight_out, eps_out, mean_sq_out};
    for (const void* p : floats)
        if (reinterpret_cast<uintptr_t>(p) & 3) return fail("causal weights: float buffers must be 4-byte aligned");
    if (state_bytes < pinn_causal_state_bytes())
        return fail("causal weights: state block too small (%zu < %zu bytes)", state_bytes, pinn_causal_state_bytes());
    if (workspace_bytes < pinn_causal_workspace_bytes(n, bins))
        return fail("causal weights: workspace too small (%zu < %zu bytes)", workspace_bytes, pinn_causal_workspace_bytes(n, bins));
    // what the launches read, and what they write: no output may lie over an input, the state, the workspace or another output
    const size_t n_ = (size_t)n, t_bytes = n ? ((n_ - 1) * (size_t)t_stride + 1) * sizeof(float) : 0;
    const struct { const void* p; size_t bytes; const char* name; } outs[] = {
        {w_out, n_ * sizeof(float), "w_out"}, {bin_weight_out, (size_t)bins * sizeof(float), "bin_weight_out"},
        {eps_out, sizeof(float), "eps_out"}, {mean_sq_out, sizeof(float), "mean_sq_out"}};
    const struct { const void* p; size_t bytes; const char* name; } ins[] = {
        {t, t_bytes, "t"}, {r, n_ * sizeof(float), "r"}, {state, pinn_causal_state_bytes(), "the state"},
        {workspace, pinn_causal_workspace_bytes(n, bins), "the workspace"}};
    for (int a = 0; a < 4; ++a) {
        for (const auto& in : ins)
            if (causal_overlap(outs[a].p, outs[a].bytes, in.p, in.bytes)) return fail("causal weights: %s overlaps %s", outs[a].name, in.name);
        for (int b = a + 1; b < 4; ++b)
            if (causal_overlap(outs[a].p, outs[a].bytes, outs[b].p, outs[b].bytes))
                return fail("causal weights: %s overlaps %s", outs[a].name, outs[b].name);
    }
    if (n == 0) return 0;                       // (nothing at all: the state stays as it is)
    PinnCausalArgs A = {};
    A.t = t; A.t_stride = (long long)t_stride; A.r = r; A.n = (long long)n; A.M = bins; A.update = update ? 1 : 0;
    A.t_lo = t_lo; A.t_hi = t_hi;
    A.state = static_cast<double*>(state); A.rows = static_cast<double*>(workspace);
    causal_fold(n, &A.chunks, &A.n_rows);
    A.w_out = w_out; A.bin_weight_out = bin_weight_out; A.eps_out = eps_out; A.mean_sq_out = mean_sq_out;
    const size_t smem_stats = PINN_CAUSAL_THREADS * (2 * sizeof(double) + 3 * sizeof(int));
    const size_t smem_rule = 2 * PINN_CAUSAL_MAX_BINS * sizeof(double) + 16;
    const int blocks = (int)((n + PINN_CAUSAL_THREADS - 1) / PINN_CAUSAL_THREADS);
    if (launch("causal-weight kernel", pinn_causal_stats_kernel, A.n_rows, PINN_CAUSAL_THREADS, smem_stats, stream, A) ||
        launch("causal-weight kernel", pinn_causal_rule_kernel, 1, PINN_CAUSAL_THREADS, smem_rule, stream, A))
        return 1;
    return launch("causal-weight kernel", pinn_causal_apply_kernel, blocks, PINN_CAUSAL_THREADS, 0, stream, A);
}

// ---- residual-adaptive resampler (pinn_aux_kernels.h: three launches; the redraw is the third alone) -----------------------------------
static int resample_nb(int64_t m) { return (int)((m + PINN_RESAMPLE_BLOCK - 1) / PINN_RESAMPLE_BLOCK); }

size_t pinn_resample_workspace_bytes(int64_t m) {
    if (m < 1 || m > PINN_RESAMPLE_MAX_POOL) return 0;
    const size_t doubles = (size_t)PINN_RESAMPLE_HEAD + (size_t)m + 2 * (size_t)resample_nb(m);
    return (doubles * sizeof(double) + 15) / 16 * 16;
}

static int resample_launch(const float* pool, const float* r, int64_t m, int d, int power, double floor_c, int64_t n_out, uint64_t seed,
                           uint64_t call_index, float* xs_out, int32_t* idx_out, void* workspace, size_t workspace_bytes, void* stream,
                           bool fill) {
    if (!pool || (fill && !r) || (n_out > 0 && !xs_out)) return fail("resample: null argument");
    if (m < 1 || m > PINN_RESAMPLE_MAX_POOL) return fail("resample: pool of m=%lld points outside [1, %lld]", (long long)m, (long long)PINN_RESAMPLE_MAX_POOL);
    if (n_out < 0) return fail("resample: n_out=%lld", (long long)n_out);
    if (d < 1 || d > PINN_MAX_INPUTS) return fail("resample: d=%d outside [1, %d]", d, PINN_MAX_INPUTS);
    if (fill && power != 1 && power != 2) return fail("resample: power=%d (1 or 2)", power);
    if (fill && !(floor_c >= 0.0 && floor_c <= PINN_RESAMPLE_MAX_FLOOR))
        return fail("resample: floor=%g must lie in [0, %g] (finite, not negative; larger values could overflow the prefix sums)", floor_c, PINN_RESAMPLE_MAX_FLOOR);
    if (!workspace) return fail("resample: null workspace");
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail("resample: the workspace must be 16-byte aligned");
    if (workspace_bytes < pinn_resample_workspace_bytes(m))
        return fail("resample: workspace too small (%zu < %zu bytes)", workspace_bytes, pinn_resample_workspace_bytes(m));
    if (n_out == 0) return 0;                   // (nothing at all: the workspace is not filled either, include/pinn.h)
    unsigned long long z = seed ^ 0x5245534D504C4552ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const int nb = resample_nb(m);
    double* ws = static_cast<double*>(workspace);
    PinnResampleArgs A = {pool, r, (long long)m, d, power, floor_c, (long long)n_out, (unsigned)(z & 0xffffffffull), (unsigned)(z >> 32),
                          (unsigned)(call_index & 0xffffffffull), (unsigned)(call_index >> 32), xs_out, idx_out,
                          ws, ws + PINN_RESAMPLE_HEAD, ws + PINN_RESAMPLE_HEAD + m, ws + PINN_RESAMPLE_HEAD + m + nb, nb};
    const int draw_blocks = (int)((n_out + PINN_RESAMPLE_BLOCK - 1) / PINN_RESAMPLE_BLOCK);
    const size_t smem = (PINN_RESAMPLE_BLOCK / 64) * sizeof(double);
    if (fill && (launch("resample kernel", pinn_resample_weights_kernel, nb, PINN_RESAMPLE_BLOCK, smem, stream, A) ||
                 launch("resample kernel", pinn_resample_offsets_kernel, 1, PINN_RESAMPLE_BLOCK, smem, stream, A)))
        return 1;
    return launch("resample kernel", pinn_resample_draw_kernel, draw_blocks, PINN_RESAMPLE_BLOCK, 0, stream, A);       // (n_out > 0 here)
}

int pinn_resample_points(const float* pool, const float* r, int64_t m, int d, int power, double floor_c, int64_t n_out,
                         uint64_t seed, uint64_t call_index, float* xs_out, int32_t* idx_out, void* workspace, size_t workspace_bytes,
                         void* stream) {
    return resample_launch(pool, r, m, d, power, floor_c, n_out, seed, call_index, xs_out, idx_out, workspace, workspace_bytes, stream, true);
}

int pinn_resample_redraw(const float* pool, int64_t m, int d, int64_t n_out, uint64_t seed, uint64_t call_index, float* xs_out,
                         int32_t* idx_out, const void* workspace, size_t workspace_bytes, void* stream) {
    return resample_launch(pool, nullptr, m, d, 1, 0.0, n_out, seed, call_index, xs_out, idx_out, const_cast<void*>(workspace),
                           workspace_bytes, stream, false);
}

// one primitive of pinn_port.h per call, on the caller's buffers (pinn_port_probe.h: the layouts; tests/test_port_contract.py)
int pinn_port_probe(int which, const void* in, void* out, int n_blocks, void* stream) {
    if (which < 0 || which >= PINN_PROBE_COUNT) return fail("unknown port probe %d (0 .. %d)", which, PINN_PROBE_COUNT - 1);
    if (!in || !out) return fail("null argument");
    if (n_blocks < 1 || n_blocks > 1024) return fail("n_blocks=%d outside [1, 1024]", n_blocks);
    const size_t smem = which == PINN_PROBE_LDS_TR16 ? (size_t)PINN_PROBE_LDS_WORDS * 4
                        : (which == PINN_PROBE_WAVE_SYNC || which == PINN_PROBE_FLAGS) ? 4096 : 0;
    int rc = 0;
#define PINN_PROBE_LAUNCH(kernel, TI, TO) \
    rc = launch("port probe", kernel, n_blocks, PINN_PROBE_THREADS, smem, stream, static_cast<const TI*>(in), static_cast<TO*>(out))
    switch (which) {
        case PINN_PROBE_MFMA16:         PINN_PROBE_LAUNCH(pinn_probe_mfma16, float, float); break;
        case PINN_PROBE_MFMA16_BF16:    PINN_PROBE_LAUNCH(pinn_probe_mfma16_bf16, unsigned, float); break;
        case PINN_PROBE_LDS_TR16:       PINN_PROBE_LAUNCH(pinn_probe_lds_tr16, unsigned, unsigned); break;
        case PINN_PROBE_PACK_HI16:      PINN_PROBE_LAUNCH(pinn_probe_pack_hi16, unsigned, unsigned); break;
        case PINN_PROBE_ROW_SUM16:      PINN_PROBE_LAUNCH(pinn_probe_row_sum16, float, float); break;
        case PINN_PROBE_ROW_SUM16_N3:   PINN_PROBE_LAUNCH(pinn_probe_row_sum16_n3, float, float); break;
        case PINN_PROBE_ROW_SUM16_F64:  PINN_PROBE_LAUNCH(pinn_probe_row_sum16_f64, double, double); break;
        case PINN_PROBE_ROWS_SUM:       PINN_PROBE_LAUNCH(pinn_probe_rows_sum, float, float); break;
        case PINN_PROBE_SHFL_XOR:       PINN_PROBE_LAUNCH(pinn_probe_shfl_xor, float, float); break;
        case PINN_PROBE_ROWS_TOTAL_F64: PINN_PROBE_LAUNCH(pinn_probe_rows_total_f64, double, double); break;
        case PINN_PROBE_WAVE_UNIFORM:   PINN_PROBE_LAUNCH(pinn_probe_wave_uniform, int, int); break;
        case PINN_PROBE_ROWS:           PINN_PROBE_LAUNCH(pinn_probe_rows, float, float); break;
        case PINN_PROBE_WAVE_SYNC:      PINN_PROBE_LAUNCH(pinn_probe_wave_sync, unsigned, unsigned); break;
        case PINN_PROBE_FLAGS:          PINN_PROBE_LAUNCH(pinn_probe_flags, int, int); break;
        case PINN_PROBE_EXP2:           PINN_PROBE_LAUNCH(pinn_probe_exp2, float, float); break;
        default:                        PINN_PROBE_LAUNCH(pinn_probe_rcp, float, float); break;
    }
#undef PINN_PROBE_LAUNCH
    return rc ? fail("port probe %d: kernel launch failed", which) : 0;
}

}  // extern "C"
