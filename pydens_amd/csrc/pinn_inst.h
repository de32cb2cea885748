// pinn_inst.h -- per-width launch entry points (one translation unit per padded hidden width HP).
#pragma once
#include "pinn_kernel.h"

struct PinnFitP;        // pinn_fit_kernel.h

// what the launcher tells the planner (make_plan, pinn_abi.cpp) about the instantiation it picked
struct PinnLaunchInfo {
    long long smem_bytes = 0;           // dynamic LDS of the launch
    int threads = 0;
    long long slab_vec4_per_wg = 0;     // saved-jet slab per workgroup (per TILE for WGX kernels)
    int per_cu = 1;                     // suggested workgroups per CU
    int mt = 1;                         // 16-point row tiles per tile
    long long wt_floats_per_wg = 0;     // slab-in-LDS kernels: per-workgroup W^T scratch
    int wgx = 0;                        // slab per TILE + gz slab + pinn_wgrad_kernel
    long long gz_vec4_per_tile = 0;
    int wt_global = 0;                  // data-gradient GEMM reads the transposed GLOBAL copy of the hidden weights
    int teams = 1;                      // tile streams of one workgroup
    int split = 0;                      // split-bf16 kernel: needs the fragment copy of the hidden weights (pinn_wsplit_kernel)
    int prepass_floats_per_lane = 0;    // LDS floats per point of a tile for the in-kernel pre-pass's double registers
};

// the one-launch fit chunk (pinn_fit_kernel.h) of an instantiation
struct PinnFitProbe {
    int carries = 0;                    // 1: the instantiation has the kernel
    int onecu_vw = 0;                   // virtual workgroups of its one-CU form (0: none)
    long long onecu_base_bytes = 0;     // LDS bytes of that form in front of what stays resident
};

enum class PinnLaunchOp {
    Launch,         // run the tile (or weight-gradient) kernel on `grid` workgroups
    Plan,           // launch nothing: fill *info
    FitProbe,       // launch nothing: fill *probe
    FitGrid,        // the fit chunk on `grid` resident workgroups (device-scope wait), arguments *fit
    FitOneCu,       // the fit chunk on ONE hardware workgroup of virtual ones, arguments *fit
};

struct PinnLaunchReq {
    PinnLaunchOp op = PinnLaunchOp::Launch;
    int grid = 0;
    void* stream = nullptr;
    PinnLaunchInfo* info = nullptr;     // Plan
    PinnFitProbe* probe = nullptr;      // FitProbe
    const PinnFitP* fit = nullptr;      // FitGrid, FitOneCu
};

// Every launcher picks the instantiation for (nd, n2[, comb, mt]) and the net / step in `a`, then does what req.op says.
// Returns 0 on success, 1 if there is no instantiation for the arguments or the instantiation does not know the op (the
// weight-gradient launchers know Launch and Plan; a fit form an instantiation lacks, or whose grid is not resident, is 1 too),
// 2 on launch failure. Plan and FitProbe write only the fields they know: the caller's defaults stand for the rest.
int pinn_launch_tile_hp16(int nd, int n2, const PinnKArgs* a, const PinnLaunchReq& req);
int pinn_launch_tile_hp32(int nd, int n2, const PinnKArgs* a, const PinnLaunchReq& req);
int pinn_launch_tile_hp64(int nd, int n2, const PinnKArgs* a, const PinnLaunchReq& req);
int pinn_launch_tile_hp128(int nd, int n2, const PinnKArgs* a, const PinnLaunchReq& req);
int pinn_launch_tile_hp256(int nd, int n2, const PinnKArgs* a, const PinnLaunchReq& req);
int pinn_launch_tile_hp512(int nd, int n2, const PinnKArgs* a, const PinnLaunchReq& req);

// streamed weight-gradient kernel of the WGX tile kernels (widths >= 128): Plan fills smem_bytes, threads and per_cu
int pinn_launch_wgrad_hp128(int nd, int n2, int comb, int mt, const PinnKArgs* a, const PinnLaunchReq& req);
int pinn_launch_wgrad_hp256(int nd, int n2, int comb, int mt, const PinnKArgs* a, const PinnLaunchReq& req);
int pinn_launch_wgrad_hp512(int nd, int n2, int comb, int mt, const PinnKArgs* a, const PinnLaunchReq& req);
