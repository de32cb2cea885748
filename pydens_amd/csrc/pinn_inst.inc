// pinn_inst.inc -- compiled once per width with -DPINN_INST_HP=<16|32|64|128|256|512> (see build.py).
#include "pinn_inst.h"
#ifndef PINN_WGX_MIN_HP
#define PINN_WGX_MIN_HP 128     // from this width on the hidden->hidden weight gradients come from pinn_wgrad_kernel (VAR 128)
#endif
#if PINN_INST_HP >= 128
#include "pinn_wgrad_kernel.h"
#endif
#ifndef PINN_WIDE_TANH_STATIC
// round 6: the WGX tile kernels of BASELINE configs 3 / 5 (evolution shape, widths 128 / 256) with tanh fixed at compile time where every layer carries it, instead
// of the one-bit run-time code (tanh / sigmoid) of the plain kernels -- same-box A/B, profiles/r06_breadth_two_team_ab.txt: cfg3 tile kernel 3.50 -> 3.35 ms, cfg5
// 5.69 -> 5.57 ms, identical sums; Sigmoid nets keep the run-time form
#define PINN_WIDE_TANH_STATIC 1
#endif
#if PINN_INST_HP <= 32
#define PINN_AUX_KERNELS_STATIC
#include "pinn_fit_kernel.h"
#endif
#ifndef PINN_CHAIN
#define PINN_CHAIN 0            // 1: the BASELINE config 2 / 4 shapes at width 64 run on pinn_chain_kernel (wave-private points; experiment)
#endif
#if PINN_INST_HP == 64 && PINN_CHAIN
#include "../../tools/experiments/pinn_chain_kernel.h"
#endif

#include <cstdio>

#define PINN_HIDDEN __attribute__((visibility("hidden")))
extern PINN_HIDDEN int g_pinn_last_kernel;          // 0 = general tile kernel, 2 = shape-specialised tile kernel (telemetry, pinn_abi.cpp)
extern PINN_HIDDEN char g_pinn_last_kernel_name[96];
extern PINN_HIDDEN char g_pinn_last_wgrad_name[96];    // ... of the last streamed weight-gradient launch (pinn_last_wgrad_kernel_name)   // instantiation of the last tile-kernel launch (pinn_last_kernel_name)

// does the net need the second set of full breadth kernels (ACTC -2 / ALLACT: activation codes above 7, nested skips)?
static inline bool pinn_needs_allact(const PinnKArgs* a) {
    if (a->skip_outer) return true;
    for (int i = 0; i <= a->lh; ++i)
        if (pinn_act_code(a->act_codes, i) > 7) return true;
    return false;
}

#ifndef PINN_WIDE_MT_128
#define PINN_WIDE_MT_128 1  // 16-point row tiles per pass of the width-128 shape-specialised kernels
#endif
#ifndef PINN_WIDE_MT_256
#define PINN_WIDE_MT_256 1  // ... of the width-256 ones
#endif
#if PINN_INST_HP == 128
#define PINN_WIDE_MT PINN_WIDE_MT_128
#else
#define PINN_WIDE_MT PINN_WIDE_MT_256
#endif
#ifndef PINN_INST_HP
#error "PINN_INST_HP must be defined"
#endif
#define PINN_CAT2(a, b) a##b
#define PINN_CAT(a, b) PINN_CAT2(a, b)
// (second set of full breadth kernels, defined in the -DPINN_INST_ALLACT=1 unit of this width: below)
int PINN_CAT(pinn_launch_breadth2_hp, PINN_INST_HP)(int nd, int n2, int comb, const PinnKArgs* a, const PinnLaunchReq& req);
int PINN_CAT(pinn_launch_wgrad2_hp, PINN_INST_HP)(int nd, int n2, int comb, const PinnKArgs* a, const PinnLaunchReq& req);

// plain activations: every layer Tanh or Sigmoid (the one-bit run-time code of the kernels without the breadth bit)
static inline bool pinn_plain_acts(const PinnKArgs* a) {
    for (int i = 0; i <= a->lh; ++i)
        if (pinn_act_code(a->act_codes, i) >= 2) return false;
    return true;
}

namespace {
// one kernel launch: the dynamic-LDS attribute (`smem_attr` bytes) set once per (kernel, device) -- a process may drive several
// devices --, the launch, the error check; the emulator runs the kernel in place
template <auto K, class... Args>
int pinn_launch_kernel(int grid, int threads, size_t smem, size_t smem_attr, void* stream, const Args&... args) {
#ifdef PINN_EMU
    (void)smem_attr; (void)stream;
    emu::launch(grid, threads, smem, [&] { K(args...); });
    return 0;
#else
    static unsigned long long done_mask = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 2;
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(done_mask & bit)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_attr) != hipSuccess) return 2;
        done_mask |= bit;
    }
    hipLaunchKernelGGL(K, dim3(grid), dim3(threads), smem, (hipStream_t)stream, args...);
    return hipGetLastError() == hipSuccess ? 0 : 2;
#endif
}

template <int ND, int N2, int LHC = -1, int ACTC = -1, int MT = 1, bool COMB = false, int VAR = 0>
int launch_one(const PinnKArgs* a, const PinnLaunchReq& req) {
    using C = PinnCfg<PINN_INST_HP, ND, N2, MT, (VAR & PINN_VAR_SPLIT) != 0>;
    constexpr int TEAMS = (VAR & PINN_VAR_TEAMS2) ? 2 : 1;                 // two tile streams in one 8-wave workgroup
    constexpr int THREADS = C::NTHREADS * TEAMS;
    constexpr size_t smem = (size_t)((VAR & PINN_VAR_TEAMS2) ? C::smem_floats_teams(LHC)
                                     : (VAR & PINN_VAR_SLAB_LDS) ? C::slabl_smem_floats(LHC > 0 ? LHC : 1)
                                     : ((VAR & PINN_VAR_2WG) ? C::SMEM_FLOATS : C::smem_floats(LHC))) * sizeof(float);
    static_assert(smem <= 160 * 1024, "LDS carve of this tile-kernel instantiation exceeds the 160 KB of a CU");
    if (req.op == PinnLaunchOp::Plan) {
        PinnLaunchInfo& info = *req.info;
        info.smem_bytes = (long long)smem;
        info.threads = THREADS;
        info.slab_vec4_per_wg = (long long)C::slab_vec4_per_wg(a->lh, (VAR & PINN_VAR_BREADTH) ? a->n_skips * ((VAR & PINN_VAR_WGX) ? 2 : 1) : 0) * TEAMS;
        info.teams = TEAMS;
        info.wt_floats_per_wg = (VAR & PINN_VAR_SLAB_LDS) ? (long long)a->lh * PINN_INST_HP * PINN_INST_HP : 0;
        int per_cu = 1;
#ifndef PINN_EMU
        // (asked once per instantiation: every step plans its launch, and the occupancy API is not free)
        static int per_cu_cached = 0;
        if (per_cu_cached == 0) {
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pinn_tile_kernel<PINN_INST_HP, ND, N2, MT, LHC, ACTC, COMB, VAR>,
                                                             THREADS, smem) != hipSuccess || per_cu < 1) per_cu = 1;
            if (per_cu > 4) per_cu = 4;
            per_cu_cached = per_cu;
        }
        per_cu = per_cu_cached;
#endif
        info.per_cu = per_cu;
        info.mt = MT;
        info.wgx = (VAR & PINN_VAR_WGX) ? 1 : 0;
        info.gz_vec4_per_tile = (VAR & PINN_VAR_WGX) ? (long long)C::gz_vec4_per_tile(a->lh) : 0;
        info.wt_global = ((C::WTG || (VAR & PINN_VAR_2WG)) && !(VAR & PINN_VAR_SPLIT)) ? 1 : 0;
        info.split = (VAR & PINN_VAR_SPLIT) ? 1 : 0;
        info.prepass_floats_per_lane = C::PREPASS_FLOATS_PER_LANE;
        return 0;
    }
    if (req.op != PinnLaunchOp::Launch) {
#if PINN_INST_HP <= 32
        // the one-launch fit chunk (pinn_fit_kernel.h): the grid form (`grid` resident workgroups, device-scope wait) and the one-CU
        // form (one hardware workgroup of FIT_VW virtual ones)
        constexpr bool FITK = (VAR & (PINN_VAR_2WG | PINN_VAR_SLAB_LDS | PINN_VAR_WGX | PINN_VAR_TEAMS2 | PINN_VAR_SPLIT)) == 0;
        using FV = PinnFitVw<PINN_INST_HP, ND, N2, MT, LHC, VAR>;
        // (not the second set of breadth kernels at width 32: with the state in LDS, hipcc 7.2 dies on one of them with "Illegal instruction
        //  detected: V_CMP_NE_U32_e32 0, $src_shared_base" -- pinn_fit_kernel.h; those nets keep the launch graphs)
        constexpr int FIT_VW = (FITK && FV::VW >= 2 && !(PINN_INST_HP == 32 && ACTC == -2)) ? FV::VW : 0;
        if (req.op == PinnLaunchOp::FitProbe) {
            *req.probe = {FITK ? 1 : 0, FIT_VW, FIT_VW ? (long long)FV::BASE_FLOATS * 4 : 0};
            return 0;
        }
        if constexpr (FITK) {
            if (req.op == PinnLaunchOp::FitGrid) {
#ifdef PINN_EMU
                if (req.grid != 1) return 1;                    // (no device-scope wait in the emulator)
#else
                // the device-scope arrive / wait of this form needs EVERY workgroup of the grid resident at once (ADVICE r5): asked, not
                // assumed -- a grid beyond what the device holds declines (the caller keeps the launch graphs)
                static int fit_per_cu = 0;
                if (fit_per_cu == 0) {
                    int n = 0;
                    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, pinn_fit_kernel<PINN_INST_HP, ND, N2, MT, LHC, ACTC, COMB, VAR, 1>,
                                                                     THREADS, smem) != hipSuccess || n < 1) n = -1;
                    fit_per_cu = n;
                }
                int dev = 0, cus = 0;
                if (fit_per_cu < 1 || hipGetDevice(&dev) != hipSuccess ||
                    hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || req.grid > fit_per_cu * cus) return 1;
#endif
                snprintf(g_pinn_last_kernel_name, sizeof(g_pinn_last_kernel_name), "pinn_fit_kernel<%d,%d,%d,%d,%d,%d,%s,%d,1>",
                         PINN_INST_HP, ND, N2, MT, LHC, ACTC, COMB ? "true" : "false", VAR);
                return pinn_launch_kernel<pinn_fit_kernel<PINN_INST_HP, ND, N2, MT, LHC, ACTC, COMB, VAR, 1>>(req.grid, THREADS, smem, smem, req.stream,
                                                                                                           *a, *req.fit);
            }
            if constexpr (FIT_VW >= 2) {
                // LDS: the virtual workgroups' blocks + W^T, then what stays resident (state, rows, batch, pre-pass rows)
                const long long res_bytes = 4 * (FV::BASE_FLOATS + FV::resident_floats(a->p_core, req.fit->n, a->d, a->n_aux));
                if (res_bytes > 160 * 1024 - 128) return 1;       // (the rest: pinn_fit_kernel's static LDS -- bail flag, update rule)
                snprintf(g_pinn_last_kernel_name, sizeof(g_pinn_last_kernel_name), "pinn_fit_kernel<%d,%d,%d,%d,%d,%d,%s,%d,%d>",
                         PINN_INST_HP, ND, N2, MT, LHC, ACTC, COMB ? "true" : "false", VAR, FIT_VW);
                return pinn_launch_kernel<pinn_fit_kernel<PINN_INST_HP, ND, N2, MT, LHC, ACTC, COMB, VAR, FIT_VW>>(
                    1, C::NTHREADS * FIT_VW, (size_t)res_bytes, 160 * 1024 - 128, req.stream, *a, *req.fit);
            }
        }
        return 1;
#else
        if (req.op == PinnLaunchOp::FitProbe) { *req.probe = PinnFitProbe(); return 0; }
        return 1;
#endif
    }
    g_pinn_last_kernel = pinn_var_spec(VAR) ? 2 : 0;
    snprintf(g_pinn_last_kernel_name, sizeof(g_pinn_last_kernel_name), "pinn_tile_kernel<%d,%d,%d,%d,%d,%d,%s,%d>",
             PINN_INST_HP, ND, N2, MT, LHC, ACTC, COMB ? "true" : "false", VAR);
    return pinn_launch_kernel<pinn_tile_kernel<PINN_INST_HP, ND, N2, MT, LHC, ACTC, COMB, VAR>>(req.grid, THREADS, smem, smem, req.stream, *a);
}
}  // namespace

#if PINN_INST_HP >= 128
namespace {
template <int ND, int N2, bool COMB, int MT, bool SPLIT = false, bool SKIPS = false, bool HEAVY = false, bool ALLACT = false>
int launch_wgrad(const PinnKArgs* a, const PinnLaunchReq& req) {
    using W = PinnWgCfg<PINN_INST_HP, ND, N2, MT, SPLIT>;
    constexpr size_t smem = (size_t)W::SMEM_FLOATS * sizeof(float);
    if (req.op == PinnLaunchOp::Plan) {
        req.info->smem_bytes = (long long)smem;
        req.info->threads = W::NTHREADS;
        req.info->per_cu = W::WGS_PER_CU;
        return 0;
    }
    if (req.op != PinnLaunchOp::Launch) return 1;
    snprintf(g_pinn_last_wgrad_name, sizeof(g_pinn_last_wgrad_name), "pinn_wgrad_kernel<%d,%d,%d,%s,%d,%s,%s,%s%s>", PINN_INST_HP, ND, N2,
             COMB ? "true" : "false", MT, SPLIT ? "true" : "false", SKIPS ? "true" : "false", HEAVY ? "true" : "false", ALLACT ? ",true" : "");
    return pinn_launch_kernel<pinn_wgrad_kernel<PINN_INST_HP, ND, N2, COMB, MT, SPLIT, SKIPS, HEAVY, ALLACT>>(req.grid, W::NTHREADS, smem, smem,
                                                                                                             req.stream, *a);
}

// the wide shape-specialised kernel (BASELINE configs 3 / 5 and their split-bf16 twins): tanh fixed at compile time where every layer
// carries it, the one-bit run-time code (Sigmoid nets) otherwise -- PINN_WIDE_TANH_STATIC above
template <int ND, int VAR>
int launch_wide_spec(const PinnKArgs* a, const PinnLaunchReq& req) {
    if (PINN_WIDE_TANH_STATIC && a->act == PINN_ACT_TANH) return launch_one<ND, 1, -1, PINN_ACT_TANH, PINN_WIDE_MT, true, VAR>(a, req);
    return launch_one<ND, 1, -1, -1, PINN_WIDE_MT, true, VAR>(a, req);
}
}  // namespace
#endif

#if PINN_INST_HP == 512
// ---- width 512 (round 6; the reference takes any `features`, model_torch.py:158-168) ----------------------------------------------
// One 16-point tile of S streams is S x 16 x 520 floats of LDS activations (33 KB per stream, ONE buffer): with the first / last-layer
// staging and eight bias-gradient rows S <= 3 fits the 160 KB -- value + one direction with its second derivative, or value + two
// first-order directions. The host (trace.StreamSpec, hp = 512) sends everything else through direction groups on the generic path;
// third / fourth order and the combined second-order stream (S >= 4) do not exist at this width. Generic depth (up to eight hidden
// layers), streamed weight gradients (pinn_wgrad_kernel in four 256 x 256 block passes); plain Tanh / Sigmoid nets on the plain kernels,
// activation codes 0 .. 7 and skips on the first set of full breadth kernels; no split-bf16 twins, no second breadth set.
int pinn_launch_tile_hp512(int nd, int n2, const PinnKArgs* a, const PinnLaunchReq& req) {
    if (a->comb || pinn_n3(n2) || pinn_needs_allact(a)) return 1;
    const bool plain = a->n_skips == 0 && pinn_plain_acts(a);
#define PINN_T512(ND, N2)                                                                                       \
    if (nd == ND && n2 == N2) return plain ? launch_one<ND, N2, -1, -1, 1, false, PINN_VAR_WGX>(a, req)           \
                                           : launch_one<ND, N2, -1, -1, 1, false, PINN_VAR_BREADTH | PINN_VAR_WGX>(a, req);
    PINN_T512(0, 0) PINN_T512(1, 0) PINN_T512(1, 1) PINN_T512(2, 0)
#undef PINN_T512
    return 1;
}
int pinn_launch_wgrad_hp512(int nd, int n2, int comb, int mt, const PinnKArgs* a, const PinnLaunchReq& req) {
    if (comb || mt != 1 || pinn_n3(n2) || pinn_needs_allact(a)) return 1;
    const bool plain = a->n_skips == 0 && pinn_plain_acts(a);
#define PINN_W512(ND, N2)                                                                                       \
    if (nd == ND && n2 == N2) return plain ? launch_wgrad<ND, N2, false, 1>(a, req)            \
                                           : launch_wgrad<ND, N2, false, 1, false, true, true>(a, req);
    PINN_W512(0, 0) PINN_W512(1, 0) PINN_W512(1, 1) PINN_W512(2, 0)
#undef PINN_W512
    return 1;
}
#else       // every other width: the rest of this file
// ---- split-bf16 twins (VAR 512) of the two BASELINE width-64 kernels: translation units of their own (-DPINN_INST_SPLIT=1 / 2,
// build.py), because the two want different code generation: the S = 4 kernel is fastest with the SLP vectoriser's packed fp32
// ops (fewer instructions: a wave issues one instruction per ~5 cycles, which is what bounds these kernels), the S = 2 kernel
// without them (v_pk_* beside bf16 MFMAs costs the matrix pipe; DESIGN.md section 6b)
#ifndef PINN_SPLIT_MT_CFG2
#define PINN_SPLIT_MT_CFG2 1
#endif
#ifndef PINN_SPLIT_MT_CFG4
#define PINN_SPLIT_MT_CFG4 2
#endif
#ifndef PINN_SPLIT_VAR
#define PINN_SPLIT_VAR PINN_VAR_TEAMS2      // second wave per SIMD of the split kernels: two teams in one workgroup (2 = two workgroups per CU: refused, pinn_kernel.h)
#endif
#ifndef PINN_CFG2_VAR
// the Poisson-box kernel of BASELINE configs 1 / 2 at width 64: two teams of 16-point tiles (VAR 256) instead of one wave
// per SIMD on 32-point tiles
#define PINN_CFG2_VAR PINN_VAR_TEAMS2
#endif
#ifndef PINN_CFG2_MT
#define PINN_CFG2_MT 1
#endif
#ifndef PINN_CFG2_SLABL
// 64: the BASELINE cfg2 kernel keeps its saved jets in LDS (VAR 64) instead of the global slab. Measured (DESIGN.md
// section 6): fabric writes 141 -> 28 MB per launch, but the kernel runs 7.7 % SLOWER (the jets then compete with the
// GEMM operands for LDS bandwidth, while the global stores were fire-and-forget) -- so the product keeps the slab (0).
#define PINN_CFG2_SLABL 0
#endif
// ---- the fp32 kernel of BASELINE config 2: a translation unit of its own (-DPINN_INST_OWN=1) because it wants another instruction
// scheduler than the rest of the width (build.py OWN_FLAGS; same-box A/B late in round 5, profiles/r05_headline_ab2.txt: the default
// strategy 0.1957 ms against 0.1983 - 0.1997 under iterative-ilp, which BASELINE config 4's kernel in turn needs: 0.2034 against 0.2067)
#if defined(PINN_INST_OWN)
#if PINN_INST_HP == 64 && PINN_INST_OWN == 1
int pinn_launch_cfg2_hp64(const PinnKArgs* a, const PinnLaunchReq& req) {
    return launch_one<2, 1, 3, PINN_ACT_TANH, PINN_CFG2_MT, true, PINN_CFG2_VAR | PINN_VAR_SPEC(1) | PINN_CFG2_SLABL>(a, req);
}
// ... and its twin with a residual PROGRAM (round 6, VAR 2048: non-affine equations / trainable V(...) scalars on the Poisson-box shape --
// bench.py --workload program; they ran on the general 32-point, one-wave-per-SIMD kernel: 46 % MFMA-busy, profiles/r06_breadth_program_summary.txt)
int pinn_launch_cfg2_prog_hp64(const PinnKArgs* a, const PinnLaunchReq& req) {
    return launch_one<2, 1, 3, PINN_ACT_TANH, 1, true, PINN_VAR_TEAMS2 | PINN_VAR_SPEC(1) | PINN_VAR_PROGRAM>(a, req);
}
// ... and with the 'Sin' activation (static, no skips: the two-way activation switch of the plain kernels is not in play, so the breadth bit
// VAR 8 is not needed; bench.py --workload sin64 ran on the one-team kernel <..., 8 | 16>: one wave per SIMD, 47 % MFMA-busy)
int pinn_launch_cfg2_sin_hp64(const PinnKArgs* a, const PinnLaunchReq& req) {
    return launch_one<2, 1, 3, PINN_ACT_SIN, 1, true, PINN_VAR_TEAMS2 | PINN_VAR_SPEC(1)>(a, req);
}
// ... and the evolution-in-a-box shape in (x, t) (PinnShape 2: boundary binding in x, initial condition in t -- heat / wave / Burgers in one space
// dimension, the tutorial's time-dependent problems on a 4 x 64 Tanh net), affine residual or residual program: S = 4 like the Poisson box, so the
// two-team form fits; these ran on the general 32-point kernel
int pinn_launch_evo2_hp64(const PinnKArgs* a, const PinnLaunchReq& req) {
    return launch_one<2, 1, 3, PINN_ACT_TANH, 1, true, PINN_VAR_TEAMS2 | PINN_VAR_SPEC(2)>(a, req);
}
int pinn_launch_evo2_prog_hp64(const PinnKArgs* a, const PinnLaunchReq& req) {
    return launch_one<2, 1, 3, PINN_ACT_TANH, 1, true, PINN_VAR_TEAMS2 | PINN_VAR_SPEC(2) | PINN_VAR_PROGRAM>(a, req);
}
#endif
#elif defined(PINN_INST_SPLIT)
#if PINN_INST_HP == 64 && PINN_INST_SPLIT == 1
int pinn_launch_split_hp64_1(const PinnKArgs* a, const PinnLaunchReq& req) {
    return launch_one<2, 1, 3, PINN_ACT_TANH, PINN_SPLIT_MT_CFG2, true, PINN_SPLIT_VAR | PINN_VAR_SPEC(1) | PINN_VAR_SPLIT>(a, req);
}
#elif PINN_INST_HP == 64
int pinn_launch_split_hp64_2(const PinnKArgs* a, const PinnLaunchReq& req) {
    return launch_one<1, 0, 3, PINN_ACT_TANH, PINN_SPLIT_MT_CFG4, false, PINN_SPLIT_VAR | PINN_VAR_SPEC(3) | PINN_VAR_SPLIT>(a, req);
}
#elif PINN_INST_HP == 128
// the WGX kernels of BASELINE configs 3 (heat, width 128) and 5 (wave, width 256) with split-bf16 forward / data-gradient GEMMs
int pinn_launch_split_hp128(const PinnKArgs* a, const PinnLaunchReq& req) {
    return launch_wide_spec<3, PINN_VAR_SPEC(2) | PINN_VAR_WGX | PINN_VAR_SPLIT>(a, req);
}
// (the split-bf16 weight-gradient kernel lives here as well: every kernel with bf16 MFMAs in the units build.py takes through asm_guard.py)
int pinn_launch_wgrad_split_hp128(const PinnKArgs* a, const PinnLaunchReq& req) {
    return launch_wgrad<3, 1, true, PINN_WIDE_MT, true>(a, req);
}
#else
int pinn_launch_split_hp256(const PinnKArgs* a, const PinnLaunchReq& req) {
    return launch_wide_spec<2, PINN_VAR_SPEC(2) | PINN_VAR_WGX | PINN_VAR_SPLIT>(a, req);
}
int pinn_launch_wgrad_split_hp256(const PinnKArgs* a, const PinnLaunchReq& req) {
    return launch_wgrad<2, 1, true, PINN_WIDE_MT, true>(a, req);
}
#endif
#else      // everything below: the regular per-width translation unit
int pinn_launch_cfg2_hp64(const PinnKArgs* a, const PinnLaunchReq& req);
int pinn_launch_cfg2_prog_hp64(const PinnKArgs* a, const PinnLaunchReq& req);
int pinn_launch_cfg2_sin_hp64(const PinnKArgs* a, const PinnLaunchReq& req);
int pinn_launch_evo2_hp64(const PinnKArgs* a, const PinnLaunchReq& req);
int pinn_launch_evo2_prog_hp64(const PinnKArgs* a, const PinnLaunchReq& req);
int pinn_launch_split_hp64_1(const PinnKArgs* a, const PinnLaunchReq& req);
int pinn_launch_split_hp64_2(const PinnKArgs* a, const PinnLaunchReq& req);
int pinn_launch_split_hp128(const PinnKArgs* a, const PinnLaunchReq& req);
int pinn_launch_split_hp256(const PinnKArgs* a, const PinnLaunchReq& req);
int pinn_launch_wgrad_split_hp128(const PinnKArgs* a, const PinnLaunchReq& req);
int pinn_launch_wgrad_split_hp256(const PinnKArgs* a, const PinnLaunchReq& req);

#if PINN_INST_HP == 64 && PINN_CHAIN
namespace {
// pinn_chain_kernel: to the host a workgroup of four "teams" (PinnLaunchInfo::teams: the chain / wgrad wave pairs) on tiles of 16 * MT points
template <int ND, int N2, int LHC, int MT, bool COMB, int SPEC>
int launch_chain(const PinnKArgs* a, const PinnLaunchReq& req) {
    using C = PinnChainCfg<ND, N2, MT, LHC>;
    constexpr size_t smem = (size_t)C::SMEM_FLOATS * sizeof(float);
    static_assert(smem <= 160 * 1024, "LDS carve of the chain kernel");
    if (req.op == PinnLaunchOp::Plan) {
        req.info->smem_bytes = (long long)smem;
        req.info->threads = C::NTHREADS;
        req.info->slab_vec4_per_wg = (long long)C::SLAB_VEC4 * C::NP;
        req.info->mt = MT;
        req.info->teams = C::NP;
        return 0;
    }
    if (req.op != PinnLaunchOp::Launch) return 1;
    g_pinn_last_kernel = 2;
    snprintf(g_pinn_last_kernel_name, sizeof(g_pinn_last_kernel_name), "pinn_chain_kernel<%d,%d,%d,%d,%s,%d>",
             ND, N2, MT, LHC, COMB ? "true" : "false", SPEC);
    return pinn_launch_kernel<pinn_chain_kernel<ND, N2, MT, LHC, COMB, SPEC>>(req.grid, C::NTHREADS, smem, smem, req.stream, *a);
}
}  // namespace
#ifndef PINN_CHAIN_MT_CFG2
#define PINN_CHAIN_MT_CFG2 1
#endif
#ifndef PINN_CHAIN_MT_CFG4
#define PINN_CHAIN_MT_CFG4 1
#endif
#endif

#if PINN_INST_HP >= 128
// which kernel family a net takes: 0 = plain (Tanh / Sigmoid layers, no skips), 1 = light skips (VAR 8 | 1024: Tanh / Sigmoid layers, the
// skips carry activation outputs; the four commonest stream shapes), 2 = full breadth (VAR 8). Shared by the tile and the
// weight-gradient launcher of the widths whose kernels come in pairs.
static int pinn_breadth_kind(const PinnKArgs* a, int nd, int n2) {
    const bool plain_acts = pinn_plain_acts(a);
    if (a->n_skips == 0 && plain_acts) return 0;
    if (plain_acts && !a->skip_src_pre && !a->skip_outer) {        // (nested skips: the full breadth kernels park the outer skip's jets)
        if (a->comb) { if (n2 == 1 && (nd == 2 || nd == 3)) return 1; }
        else if (pinn_n3(n2) == 0 && ((nd == 1 && n2 == 1) || (nd == 2 && n2 == 2))) return 1;
    }
    return 2;
}

#ifndef PINN_INST_ALLACT
// streamed weight-gradient kernel matching the WGX tile kernel of (nd, n2, comb, mt): same jet structure, same lane-private layout
int PINN_CAT(pinn_launch_wgrad_hp, PINN_INST_HP)(int nd, int n2, int comb, int mt, const PinnKArgs* a, const PinnLaunchReq& req) {
    if (mt != PINN_WIDE_MT && mt != 1) return 1;
    const int kind = pinn_breadth_kind(a, nd, n2);
    if (kind == 1) {
        // partners of the VAR 8 | 1024 | 128 tile kernels below (skips over Tanh / Sigmoid layers)
        if (mt != 1) return 1;
        if (comb && n2 == 1 && nd == 2) return launch_wgrad<2, 1, true, 1, false, true>(a, req);
        if (comb && n2 == 1 && nd == 3) return launch_wgrad<3, 1, true, 1, false, true>(a, req);
        if (!comb && nd == 1 && n2 == 1) return launch_wgrad<1, 1, false, 1, false, true>(a, req);
        if (!comb && nd == 2 && n2 == 2) return launch_wgrad<2, 2, false, 1, false, true>(a, req);
        return 1;
    }
    if (kind == 2) {
        // ... of the full breadth kernels (VAR 8 | 128): any activation, any skip form
        if (mt != 1) return 1;
#define PINN_WG_HEAVY(ND, N2, COMB) \
        if (nd == ND && n2 == N2 && (comb != 0) == COMB) return pinn_needs_allact(a) ? PINN_CAT(pinn_launch_wgrad2_hp, PINN_INST_HP)(nd, n2, comb, a, req) \
                                                                                     : launch_wgrad<ND, N2, COMB, 1, false, true, true>(a, req);
#ifndef PINN_ONLY_BASELINE
        PINN_WG_HEAVY(0, 0, false) PINN_WG_HEAVY(1, 0, false) PINN_WG_HEAVY(1, 1, false) PINN_WG_HEAVY(2, 0, false)
        PINN_WG_HEAVY(2, 2, false) PINN_WG_HEAVY(3, 2, false) PINN_WG_HEAVY(2, 1, true) PINN_WG_HEAVY(3, 1, true)
        PINN_WG_HEAVY(4, 0, false) PINN_WG_HEAVY(4, 1, true) PINN_WG_HEAVY(1, 9, false) PINN_WG_HEAVY(2, 9, false) PINN_WG_HEAVY(1, 73, false)
#if PINN_INST_HP <= 128
        PINN_WG_HEAVY(3, 3, false)
#endif
#endif
#undef PINN_WG_HEAVY
        return 1;
    }
    // split-bf16 form (pinn_set_gemm_mode) for the shapes of BASELINE configs 3 / 5: the kernel only consumes the slabs, so it
    // pairs with the exact-fp32 tile kernel as well
#if PINN_INST_HP == 128
    if (a->gemm_mode == PINN_GEMM_BF16X3 && nd == 3 && n2 == 1 && comb && mt == PINN_WIDE_MT)
        return pinn_launch_wgrad_split_hp128(a, req);
#else
    if (a->gemm_mode == PINN_GEMM_BF16X3 && nd == 2 && n2 == 1 && comb && mt == PINN_WIDE_MT)
        return pinn_launch_wgrad_split_hp256(a, req);
#endif
#define PINN_WG_CASE(ND, N2, COMB)                                                                                  \
    if (nd == ND && n2 == N2 && (comb != 0) == COMB) {                                                              \
        if (mt == 1) return launch_wgrad<ND, N2, COMB, 1>(a, req);                            \
        return launch_wgrad<ND, N2, COMB, PINN_WIDE_MT>(a, req);                             \
    }
#ifdef PINN_ONLY_BASELINE
    // experiment builds: only the BASELINE kernels; sizing queries of any other shape get their answer
#if PINN_INST_HP == 128
    PINN_WG_CASE(3, 1, true)
    if (req.op == PinnLaunchOp::Plan) return launch_wgrad<3, 1, true, PINN_WIDE_MT>(a, req);
#else
    PINN_WG_CASE(2, 1, true)
    if (req.op == PinnLaunchOp::Plan) return launch_wgrad<2, 1, true, PINN_WIDE_MT>(a, req);
#endif
#else
    PINN_WG_CASE(0, 0, false) PINN_WG_CASE(1, 0, false) PINN_WG_CASE(1, 1, false) PINN_WG_CASE(2, 0, false)
    PINN_WG_CASE(2, 2, false) PINN_WG_CASE(3, 2, false) PINN_WG_CASE(2, 1, true) PINN_WG_CASE(3, 1, true)
    PINN_WG_CASE(4, 0, false) PINN_WG_CASE(4, 1, true) PINN_WG_CASE(1, 9, false) PINN_WG_CASE(2, 9, false) PINN_WG_CASE(1, 73, false)
#if PINN_INST_HP <= 128
    PINN_WG_CASE(3, 3, false)
#endif
#endif
#undef PINN_WG_CASE
    return 1;
}
#endif  // !PINN_INST_ALLACT
#endif

// fast instantiations: layer count and activation fixed at compile time for the BASELINE shapes
#if PINN_INST_HP == 64
// points per tile = 16 * MT: more row tiles per pass amortise barriers / weight fetches and give the latency-bound
// vector phases independent work, as long as the jets of MT*S streams still fit the register file
#ifndef PINN_FAST_MT_S5
#define PINN_FAST_MT_S5 1
#endif
#ifndef PINN_FAST_MT_S2
#define PINN_FAST_MT_S2 3
#endif
#define PINN_FAST_LIST(X)                                                                     \
    X(2, 2, 3, PINN_ACT_TANH, PINN_FAST_MT_S5) X(1, 0, 3, PINN_ACT_TANH, PINN_FAST_MT_S2)        \
    X(1, 0, 2, PINN_ACT_TANH, PINN_FAST_MT_S2) X(1, 0, 4, PINN_ACT_TANH, PINN_FAST_MT_S2)        \
    X(1, 1, 3, PINN_ACT_TANH, 2)
#ifndef PINN_FAST_VAR_S2
// VAR of the ODE-family kernel of BASELINE config 4: PinnShape 3 (48) | two workgroups per CU (2). With S = 2 streams and
// 32-point tiles the kernel fits 256 registers, and a second wave per SIMD fills the latency of the vector phases (30 % of
// this kernel): 0.226 -> 0.203 ms per 131 072 points in a same-box A/B (one wave at 48-point tiles before)
#define PINN_FAST_VAR_S2 (PINN_VAR_SPEC(3) | PINN_VAR_TEAMS2)
#endif
#ifndef PINN_CFG4_MT
#define PINN_CFG4_MT 2
#endif

#ifndef PINN_FAST_MT_COMB
#define PINN_FAST_MT_COMB 2
#endif
#ifndef PINN_SIN_MT
#define PINN_SIN_MT 1           // (32-point tiles spill 59 registers on the Sin kernel)
#endif
#ifndef PINN_FAST_VAR_COMB
#define PINN_FAST_VAR_COMB 0
#endif
#define PINN_FAST_COMB_LIST(X)                                                                \
    X(2, 3, PINN_ACT_TANH, PINN_FAST_MT_COMB, PINN_FAST_VAR_COMB)                               \
    X(2, 2, PINN_ACT_TANH, PINN_FAST_MT_COMB, 0) X(2, 4, PINN_ACT_TANH, PINN_FAST_MT_COMB, 0)  \
    X(3, 3, PINN_ACT_TANH, 1, 0)
// (width 128: the generic instantiations win -- keeping 4 x 8 weight-gradient tiles per wave in registers makes the
//  8-wave kernel spill 600+ VGPRs; accumulating them in the workgroup's partial buffer runs cfg3 1.7x faster)
#elif PINN_INST_HP == 16
#define PINN_FAST_LIST(X) X(2, 2, 2, PINN_ACT_TANH, 1)
#define PINN_FAST_COMB_LIST(X) X(2, 2, PINN_ACT_TANH, 1, 0)
#else
#define PINN_FAST_LIST(X)
#define PINN_FAST_COMB_LIST(X)
#endif

// VAR bit of the widths whose hidden->hidden weight gradients come from pinn_wgrad_kernel
constexpr int WGXV = (PINN_INST_HP >= PINN_WGX_MIN_HP && PINN_INST_HP >= 128) ? PINN_VAR_WGX : 0;
#ifndef PINN_HEAVY_WGX
#define PINN_HEAVY_WGX 1        // ... of the full breadth kernels (VAR 8) too (round 4; 0: read-modify-write rows of the partial buffer, the A/B partner)
#endif
constexpr int WGXH = PINN_HEAVY_WGX ? WGXV : 0;

// which of the shapes PinnShape fixes at compile time does the call describe (0: none)?
// (program = true, round 6: the same shapes with a residual PROGRAM -- PinnShape SPEC | 4; the coefficient rows belong to the affine form)
static int pinn_spec_of(const PinnKArgs* a, int nd, int n2, bool program = false) {
    if (a->mode != PINN_MODE_STEP || a->res_kind != (program ? PINN_RES_PROGRAM : PINN_RES_AFFINE) || a->s_user != 1 + nd + n2 || a->ic_var1 > 0) return 0;
    // (the shape-specialised AFFINE kernels are compiled for the mean-square criterion alone -- PinnShape::crit; their residual-program twins
    //  read the criterion from the arguments)
    if (!program && a->crit != PINN_CRIT_MSE) return 0;
    for (int k = 0; k < nd; ++k)
        if (a->dir_cols[k] != k) return 0;
    for (int s = 0; s < a->s_user && !program; ++s)
        if (a->coef_row[s] >= 0) return 0;
    if (a->has_bc && !a->has_ic && !a->ic_streams && a->d == nd && a->nsp == nd && a->ndims == nd) return 1;
    if (a->has_bc && a->has_ic && a->d == nd && a->nsp == nd - 1 && a->ndims == nd) return 2;
    if (!a->has_bc && a->has_ic && nd == 1 && a->nsp == 0 && a->ndims == 1) return 3;
    return 0;
}


// ---- second set of full breadth kernels (round 5; ACTC -2 / ALLACT: all sixteen activation codes, nested skips) and, for the streamed
// widths, their weight-gradient partners: a translation unit of their own per width (-DPINN_INST_ALLACT=1)
#ifdef PINN_INST_ALLACT
// the stream shapes of the second set: what the generic path's direction groups (one or two directions per call, one third-order
// direction) and the commonest fused steps (Laplacian-type operators as ONE combined stream) ask for. Shapes beyond these exist in
// the first set only; for the second set the host splits them into direction groups (trace.StreamSpec, `allact`). The tile kernels
// (PINN_INST_ALLACT=1) and their weight-gradient partners (=2, widths >= 128) compile as separate units.
#define PINN_ALLACT_SHAPES(X) X(0, 0, false) X(1, 0, false) X(1, 1, false) X(2, 0, false) X(2, 2, false) X(2, 1, true) X(3, 1, true) X(1, 9, false) X(1, 73, false)
#if PINN_INST_ALLACT == 1
int PINN_CAT(pinn_launch_breadth2_hp, PINN_INST_HP)(int nd, int n2, int comb, const PinnKArgs* a, const PinnLaunchReq& req) {
#ifndef PINN_ONLY_BASELINE
#define PINN_B2(ND, N2, COMB) if (nd == ND && n2 == N2 && (comb != 0) == COMB) return launch_one<ND, N2, -1, -2, 1, COMB, PINN_VAR_BREADTH | WGXH>(a, req);
    PINN_ALLACT_SHAPES(PINN_B2)
#undef PINN_B2
#endif
    return 1;
}
#endif
#if PINN_INST_ALLACT == 2 || (PINN_INST_ALLACT == 1 && PINN_INST_HP < 128)
int PINN_CAT(pinn_launch_wgrad2_hp, PINN_INST_HP)(int nd, int n2, int comb, const PinnKArgs* a, const PinnLaunchReq& req) {
#if PINN_INST_HP >= 128 && !defined(PINN_ONLY_BASELINE)
#define PINN_W2(ND, N2, COMB) if (nd == ND && n2 == N2 && (comb != 0) == COMB) return launch_wgrad<ND, N2, COMB, 1, false, true, true, true>(a, req);
    PINN_ALLACT_SHAPES(PINN_W2)
#undef PINN_W2
#endif
    return 1;
}
#endif
#endif  // PINN_INST_ALLACT
#ifndef PINN_INST_ALLACT
// the full breadth tile kernel of a stream shape: first set (ACTC -1: activation codes 0 .. 7, no nested skips) or second (ACTC -2: all)
// (the second set lives in a translation unit of its own, -DPINN_INST_ALLACT=1: build.py compiles the units in parallel)
#define PINN_BREADTH(ND, N2, COMB) (pinn_needs_allact(a) ? PINN_CAT(pinn_launch_breadth2_hp, PINN_INST_HP)(nd, n2, COMB ? 1 : 0, a, req) \
                                                         : launch_one<ND, N2, -1, -1, 1, COMB, PINN_VAR_BREADTH | WGXH>(a, req))
int PINN_CAT(pinn_launch_tile_hp, PINN_INST_HP)(int nd, int n2, const PinnKArgs* a, const PinnLaunchReq& req) {
    [[maybe_unused]] const bool sizing = req.op == PinnLaunchOp::Plan;
#define PINN_TRY_FAST(ND, N2, LH, ACT, MT)                                                                             \
    if (nd == ND && n2 == N2 && a->lh == LH && a->act == ACT && !skips)                                                \
        return launch_one<ND, N2, LH, ACT, MT>(a, req);
    // nets with skip connections ('R ... +') or activations other than tanh / sigmoid take the generic-depth kernels
    // compiled with the breadth bit (VAR 8)
#ifdef PINN_ONLY_BASELINE
    // experiment builds (tools/variant.sh): nothing but the kernels of the BASELINE configs, so that a variant compiles in
    // seconds (queries -- workspace sizing -- are answered with the same kernels)
#if PINN_INST_HP == 64
#if PINN_CHAIN
    if (a->comb && nd == 2 && n2 == 1 && a->lh == 3 && a->act == PINN_ACT_TANH && pinn_spec_of(a, nd, n2) == 1)
        return launch_chain<2, 1, 3, PINN_CHAIN_MT_CFG2, true, 1>(a, req);
    if (!a->comb && nd == 1 && n2 == 0 && a->lh == 3 && a->act == PINN_ACT_TANH && pinn_spec_of(a, nd, n2) == 3)
        return launch_chain<1, 0, 3, PINN_CHAIN_MT_CFG4, false, 3>(a, req);
#endif
    if (a->gemm_mode == PINN_GEMM_BF16X3) {
        if (a->comb && nd == 2 && n2 == 1 && a->lh == 3 && a->act == PINN_ACT_TANH && pinn_spec_of(a, nd, n2) == 1)
            return pinn_launch_split_hp64_1(a, req);
        if (!a->comb && nd == 1 && n2 == 0 && a->lh == 3 && a->act == PINN_ACT_TANH && pinn_spec_of(a, nd, n2) == 3)
            return pinn_launch_split_hp64_2(a, req);
    }
    if (a->comb && nd == 2 && n2 == 1 && (sizing || (a->lh == 3 && a->act == PINN_ACT_TANH && pinn_spec_of(a, nd, n2) == 1)))
        return launch_one<2, 1, 3, PINN_ACT_TANH, PINN_CFG2_MT, true, PINN_CFG2_VAR | PINN_VAR_SPEC(1) | PINN_CFG2_SLABL>(a, req);
    if (!a->comb && nd == 1 && n2 == 0 && (sizing || (a->lh == 3 && a->act == PINN_ACT_TANH && pinn_spec_of(a, nd, n2) == 3)))
        return launch_one<1, 0, 3, PINN_ACT_TANH, PINN_CFG4_MT, false, PINN_FAST_VAR_S2>(a, req);
    if (sizing) return launch_one<2, 1, 3, PINN_ACT_TANH, PINN_CFG2_MT, true, PINN_CFG2_VAR | PINN_VAR_SPEC(1) | PINN_CFG2_SLABL>(a, req);
#elif PINN_INST_HP == 128
    if (a->gemm_mode == PINN_GEMM_BF16X3 && WGXV && a->comb && nd == 3 && n2 == 1 && pinn_spec_of(a, nd, n2) == 2)
        return pinn_launch_split_hp128(a, req);
    if (sizing || (a->comb && nd == 3 && n2 == 1 && pinn_spec_of(a, nd, n2) == 2))
        return launch_wide_spec<3, PINN_VAR_SPEC(2) | WGXV>(a, req);
#elif PINN_INST_HP == 256
    if (a->gemm_mode == PINN_GEMM_BF16X3 && WGXV && a->comb && nd == 2 && n2 == 1 && pinn_spec_of(a, nd, n2) == 2)
        return pinn_launch_split_hp256(a, req);
    if (sizing || (a->comb && nd == 2 && n2 == 1 && pinn_spec_of(a, nd, n2) == 2))
        return launch_wide_spec<2, PINN_VAR_SPEC(2) | WGXV>(a, req);
#endif
    return 1;
#else
    bool skips = a->n_skips > 0, plain_acts = pinn_plain_acts(a);
    skips = skips || !plain_acts;
    if (a->skip_src_pre || a->skip_outer) plain_acts = false;   // (the lighter skip kernels, VAR 8 | 1024, carry activation outputs only, one skip at a time)
    const int spec = skips ? 0 : pinn_spec_of(a, nd, n2);
    if (a->comb) {
        // combined second-order stream (n2 == 1): sum_k c_k d2/dx_k2 over nd = 2 or 3 directions
        if (n2 != 1) return 1;
        if (skips) {
#if PINN_INST_HP == 64
            // 'Sin' nets of depth 4 (round 3, the worst breadth workload of bench.py): static depth and activation, so that the
            // weight gradients stay in registers instead of read-modify-write rows of the partial buffer (generic-depth kernels)
            if (nd == 2 && a->lh == 3 && a->act == PINN_ACT_SIN && a->n_skips == 0) {
#ifndef PINN_SIN_TEAMS
#define PINN_SIN_TEAMS 1        // 1: the Dirichlet-box 'Sin' kernel as two teams of 16-point tiles (round 6), 0: one team (round 3's form)
#endif
                if (pinn_spec_of(a, nd, n2) == 1 && PINN_SIN_TEAMS && PINN_SIN_MT == 1)
                    return pinn_launch_cfg2_sin_hp64(a, req);
                if (pinn_spec_of(a, nd, n2) == 1)       // Dirichlet box, affine residual: the shape facts fixed as for BASELINE config 2
                    return launch_one<2, 1, 3, PINN_ACT_SIN, PINN_SIN_MT, true, PINN_VAR_BREADTH | PINN_VAR_SPEC(1)>(a, req);
                return launch_one<2, 1, 3, PINN_ACT_SIN, PINN_SIN_MT, true, PINN_VAR_BREADTH>(a, req);
            }
#endif
            // (skips over Tanh / Sigmoid layers only: the breadth kernel without the heavy activation paths, VAR 8 | 1024)
            // (widths >= 128: hidden->hidden weight gradients from pinn_wgrad_kernel<..., SKIPS>, round 4)
#if PINN_INST_HP >= 128
#ifndef PINN_WIDE_SIN_STATIC
#define PINN_WIDE_SIN_STATIC 1  // 'Sin' nets without skips on the Dirichlet-box shape: activation fixed at compile time instead of the full breadth kernel's run-time code
#endif
            // (round 6: bench.py `sin128` sat at 0.49 of the peak executed with 3.8 non-MFMA vector instructions per MFMA -- the run-time activation
            //  switch of the full breadth kernel around `sincos`; its weight-gradient partner stays the HEAVY one, which reads the same slab)
            if (PINN_WIDE_SIN_STATIC && nd == 2 && a->act == PINN_ACT_SIN && a->n_skips == 0 && pinn_spec_of(a, nd, n2) == 1)
                return launch_one<2, 1, -1, PINN_ACT_SIN, 1, true, PINN_VAR_SPEC(1) | WGXV>(a, req);
            // (Dirichlet box, affine residual: the shape facts fixed as for BASELINE config 2 -- the residual nets one meets first)
            // (round 6: Tanh throughout -- the usual residual PINN, bench.py skip128 / skip256: the activation as a compile-time fact here as well)
            if (PINN_WIDE_TANH_STATIC && nd == 2 && a->act == PINN_ACT_TANH && a->n_skips > 0 && !a->skip_src_pre && !a->skip_outer && pinn_spec_of(a, nd, n2) == 1)
                return launch_one<2, 1, -1, PINN_ACT_TANH, 1, true, PINN_VAR_BREADTH | PINN_VAR_SPEC(1) | PINN_VAR_SKIPS_LIGHT | WGXV>(a, req);
            if (nd == 2 && plain_acts && a->n_skips > 0 && pinn_spec_of(a, nd, n2) == 1)
                return launch_one<2, 1, -1, -1, 1, true, PINN_VAR_BREADTH | PINN_VAR_SPEC(1) | PINN_VAR_SKIPS_LIGHT | WGXV>(a, req);
#endif
            if (nd == 2 && plain_acts) return launch_one<2, 1, -1, -1, 1, true, PINN_VAR_BREADTH | PINN_VAR_SKIPS_LIGHT | WGXV>(a, req);
            if (nd == 3 && plain_acts) return launch_one<3, 1, -1, -1, 1, true, PINN_VAR_BREADTH | PINN_VAR_SKIPS_LIGHT | WGXV>(a, req);
#if PINN_INST_HP >= 128
#ifndef PINN_WIDE_GELU_STATIC
#define PINN_WIDE_GELU_STATIC 1 // GELU nets (any skip form of the first breadth set) of the streamed widths: the full breadth kernel with the activation fixed at compile time
#endif
            // (round 6: bench.py `gelu256` -- Burgers on a GELU pre-activation ResNet -- ran the full breadth kernel with 299 spilled registers at width 256: every
            //  activation's derivative code competes for them; the skip machinery stays, VAR 8, only the activation is a compile-time fact)
            if (PINN_WIDE_GELU_STATIC && nd == 2 && a->act == PINN_ACT_GELU && WGXH && !pinn_needs_allact(a))
                return launch_one<2, 1, -1, PINN_ACT_GELU, 1, true, PINN_VAR_BREADTH | WGXH>(a, req);
#endif
            if (nd == 2) return PINN_BREADTH(2, 1, true);
            if (nd == 3) return PINN_BREADTH(3, 1, true);
            if (nd == 4) return PINN_BREADTH(4, 1, true);
            return 1;
        }
#if PINN_INST_HP == 64
        // the Poisson-type shape of BASELINE configs 1/2 with everything the point stage branches on fixed (VAR 16)
        if (sizing && nd == 2 && a->lh == 3 && a->act == PINN_ACT_TANH && PINN_CFG2_SLABL) {
            // sizing queries do not know the shape yet: the general kernel's answer (it needs the global slab) plus the
            // W^T scratch the slab-in-LDS kernel would need
            const int rc = launch_one<2, 1, 3, PINN_ACT_TANH, PINN_FAST_MT_COMB, true, PINN_FAST_VAR_COMB>(a, req);
            req.info->wt_floats_per_wg = 3LL * PINN_INST_HP * PINN_INST_HP;
            return rc;
        }
#if PINN_CHAIN
        if (nd == 2 && a->lh == 3 && a->act == PINN_ACT_TANH && spec == 1)
            return launch_chain<2, 1, 3, PINN_CHAIN_MT_CFG2, true, 1>(a, req);
#endif
        // a residual program on the Poisson-box shape: the two-team kernel's twin (exact-fp32 GEMMs in either GEMM mode)
        if (!skips && nd == 2 && a->lh == 3 && a->act == PINN_ACT_TANH && pinn_spec_of(a, nd, n2, true) == 1)
            return pinn_launch_cfg2_prog_hp64(a, req);
#ifndef PINN_EVO2_TEAMS
#define PINN_EVO2_TEAMS 1       // 1: the (x, t) evolution shape on two-team kernels (round 6), 0: the general 32-point kernel (before)
#endif
        if (PINN_EVO2_TEAMS && !skips && nd == 2 && a->lh == 3 && a->act == PINN_ACT_TANH && spec == 2)
            return pinn_launch_evo2_hp64(a, req);
        if (PINN_EVO2_TEAMS && !skips && nd == 2 && a->lh == 3 && a->act == PINN_ACT_TANH && pinn_spec_of(a, nd, n2, true) == 2)
            return pinn_launch_evo2_prog_hp64(a, req);
        if (nd == 2 && a->lh == 3 && a->act == PINN_ACT_TANH && spec == 1 && a->gemm_mode == PINN_GEMM_BF16X3)
            return pinn_launch_split_hp64_1(a, req);
        // (pinn_set_tanh_mode(PINN_TANH_ACCURATE): the same kernel with the polynomial tanh below 0.45 -- ACTC carries PINN_ACT_TANH_POLYBIT)
        if (nd == 2 && a->lh == 3 && a->act == PINN_ACT_TANH && spec == 1 && a->tanh_mode == PINN_TANH_ACCURATE)
            return launch_one<2, 1, 3, PINN_ACT_TANH | PINN_ACT_TANH_POLYBIT, PINN_CFG2_MT, true, PINN_CFG2_VAR | PINN_VAR_SPEC(1) | PINN_CFG2_SLABL>(a, req);
        if (nd == 2 && a->lh == 3 && a->act == PINN_ACT_TANH && spec == 1)
            return pinn_launch_cfg2_hp64(a, req);        // (its own translation unit: above)
#elif PINN_INST_HP == 16
        if (nd == 2 && a->lh == 2 && a->act == PINN_ACT_TANH && spec == 1)
            return launch_one<2, 1, 2, PINN_ACT_TANH, 1, true, PINN_VAR_SPEC(1)>(a, req);
#elif PINN_INST_HP == 128
        // heat-type shape of BASELINE config 3 on the generic-depth kernel
        if (nd == 3 && spec == 2 && a->gemm_mode == PINN_GEMM_BF16X3 && WGXV) return pinn_launch_split_hp128(a, req);
        if (nd == 3 && spec == 2) return launch_wide_spec<3, PINN_VAR_SPEC(2) | WGXV>(a, req);
#elif PINN_INST_HP == 256
        // wave-type shape of BASELINE config 5
        if (nd == 2 && spec == 2 && a->gemm_mode == PINN_GEMM_BF16X3 && WGXV) return pinn_launch_split_hp256(a, req);
        if (nd == 2 && spec == 2) return launch_wide_spec<2, PINN_VAR_SPEC(2) | WGXV>(a, req);
#endif
#define PINN_TRY_FAST_COMB(ND, LH, ACT, MT, VAR) \
        if (nd == ND && a->lh == LH && a->act == ACT) return launch_one<ND, 1, LH, ACT, MT, true, VAR>(a, req);
        PINN_FAST_COMB_LIST(PINN_TRY_FAST_COMB)
#undef PINN_TRY_FAST_COMB
        if (nd == 2) return launch_one<2, 1, -1, -1, 1, true, WGXV>(a, req);
        if (nd == 3) return launch_one<3, 1, -1, -1, 1, true, WGXV>(a, req);
        if (nd == 4) return launch_one<4, 1, -1, -1, 1, true, WGXV>(a, req);       // 3-D space + time
        return 1;
    }
#if PINN_INST_HP == 64
    // ODE-family shape of BASELINE config 4
#if PINN_CHAIN
    if (nd == 1 && n2 == 0 && a->lh == 3 && a->act == PINN_ACT_TANH && spec == 3)
        return launch_chain<1, 0, 3, PINN_CHAIN_MT_CFG4, false, 3>(a, req);
#endif
    if (nd == 1 && n2 == 0 && a->lh == 3 && a->act == PINN_ACT_TANH && spec == 3 && a->gemm_mode == PINN_GEMM_BF16X3)
        return pinn_launch_split_hp64_2(a, req);
    if (nd == 1 && n2 == 0 && a->lh == 3 && a->act == PINN_ACT_TANH && spec == 3)
        return launch_one<1, 0, 3, PINN_ACT_TANH, PINN_CFG4_MT, false, PINN_FAST_VAR_S2>(a, req);
#endif
    // (the S = 5 kernel of the 4 x 64 net -- residual programs, the generic path of config 2 -- measured with 32-point tiles: 0.349 ->
    //  0.445 ms, and as two workgroups per CU with W^T from the global copy: 0.381 ms; 16-point tiles, one workgroup per CU stay)
    PINN_FAST_LIST(PINN_TRY_FAST)
#undef PINN_TRY_FAST
    if (pinn_n3(n2) > 0 || pinn_n4(n2) > 0) {
        // third-order streams (n2 is the packed count: 9 = one second-order direction that also carries a third derivative):
        // generic-depth kernels, u_xxx-type equations in one or two variables (KdV: x to third order, t to first)
        // fourth order (round 5; packed 73 = one direction with second, third and fourth derivative: beam / Kuramoto-Sivashinsky / biharmonic
        // operators, one such direction per call)
        if (skips && nd == 1 && n2 == 73) return PINN_BREADTH(1, 73, false);
        if (nd == 1 && n2 == 73) return launch_one<1, 73, -1, -1, 1, false, WGXV>(a, req);
        if (skips && nd == 1 && n2 == 9) return PINN_BREADTH(1, 9, false);
        if (skips && nd == 2 && n2 == 9) return PINN_BREADTH(2, 9, false);
        if (nd == 1 && n2 == 9) return launch_one<1, 9, -1, -1, 1, false, WGXV>(a, req);
        if (nd == 2 && n2 == 9) return launch_one<2, 9, -1, -1, 1, false, WGXV>(a, req);
        return 1;
    }
    const int key = nd * 4 + n2;          // (nd = 4 comes with n2 = 0 only: key 16)
    if (skips && plain_acts) {
        switch (key) {         // the commonest residual-program shapes of residual nets (others: the full breadth kernels below)
            case 1 * 4 + 1: return launch_one<1, 1, -1, -1, 1, false, PINN_VAR_BREADTH | PINN_VAR_SKIPS_LIGHT | WGXV>(a, req);
            case 2 * 4 + 2: return launch_one<2, 2, -1, -1, 1, false, PINN_VAR_BREADTH | PINN_VAR_SKIPS_LIGHT | WGXV>(a, req);
            default: break;
        }
    }
    if (skips) {
        switch (key) {
            case 0 * 4 + 0: return PINN_BREADTH(0, 0, false);
            case 1 * 4 + 0: return PINN_BREADTH(1, 0, false);
            case 1 * 4 + 1: return PINN_BREADTH(1, 1, false);
            case 2 * 4 + 0: return PINN_BREADTH(2, 0, false);
            case 2 * 4 + 2: return PINN_BREADTH(2, 2, false);
            case 3 * 4 + 2: return PINN_BREADTH(3, 2, false);
            case 4 * 4 + 0: return PINN_BREADTH(4, 0, false);
#if PINN_INST_HP <= 128
            case 3 * 4 + 3: return PINN_BREADTH(3, 3, false);
#endif
            default: return 1;
        }
    }
    switch (key) {
        case 0 * 4 + 0: return launch_one<0, 0, -1, -1, 1, false, WGXV>(a, req);
        case 1 * 4 + 0: return launch_one<1, 0, -1, -1, 1, false, WGXV>(a, req);
        case 1 * 4 + 1: return launch_one<1, 1, -1, -1, 1, false, WGXV>(a, req);
        case 2 * 4 + 0: return launch_one<2, 0, -1, -1, 1, false, WGXV>(a, req);
        case 2 * 4 + 2: return launch_one<2, 2, -1, -1, 1, false, WGXV>(a, req);
        case 3 * 4 + 2: return launch_one<3, 2, -1, -1, 1, false, WGXV>(a, req);
        case 4 * 4 + 0: return launch_one<4, 0, -1, -1, 1, false, WGXV>(a, req);
#if PINN_INST_HP <= 128
        case 3 * 4 + 3: return launch_one<3, 3, -1, -1, 1, false, WGXV>(a, req);
#endif
        default: return 1;
    }
#endif  // PINN_ONLY_BASELINE
}
#endif  // !PINN_INST_ALLACT
#endif  // PINN_INST_SPLIT
#endif  // PINN_INST_HP == 512
