""" The reduction launch alone (pinn_reduce_kernel: sum of the partial rows + Adam + loss slot), back to back on one stream, by HIP events,
for one or more builds of the library, interleaved. Synthetic rows through pinn_reduce_rows, at BASELINE config 2's sizes (256 rows of
12 756 floats) and at a tiny grid (4 rows of config 1's 628 floats).
    python tools/reduce_bench.py [--sizes 256x12756,4x628] [--reps 2000] [--rounds 3] lib1.so [lib2.so ...]
A launch behind a launch of the same stream starts when its predecessor has drained: the figure is kernel time plus the gap between
two dependent launches, per launch. The 13 MB of rows stay in the Infinity Cache between launches, as they do behind the tile kernel
that has just written them. """
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402
from pydens_amd import engine   # noqa: E402
from pydens_amd.solver import FlatOptimizer     # noqa: E402


def load(path):
    lib = ctypes.CDLL(path)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.pinn_reduce_rows.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, i32, ctypes.POINTER(engine.Optim), vp, i32, vp]
    lib.pinn_reduce_rows.restype = i32
    lib.pinn_last_reduce_kernel_name.restype = ctypes.c_char_p
    lib.pinn_last_error.restype = ctypes.c_char_p
    return lib


class Case:
    def __init__(self, n, p):
        g = torch.Generator(device='cuda').manual_seed(n * 100003 + p)
        self.n, self.p = n, p
        self.rows = torch.randn((n, p), device='cuda', generator=g)
        self.start = [torch.randn(p, device='cuda', generator=g), torch.zeros(p, device='cuda'), torch.zeros(p, device='cuda')]
        self.grads = torch.zeros(p, device='cuda')
        self.step = torch.zeros(1, dtype=torch.int32, device='cuda')
        self.loss = torch.zeros(1, device='cuda')
        self.optim = engine.Optim.build(FlatOptimizer.RULES['Adam'][0], **FlatOptimizer.hyper('Adam', 0.001, {}))
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(self, lib, reps):
        """ `reps` launches from the same start (Adam steps 1 .. reps); returns microseconds per launch """
        state = [t.clone() for t in self.start]
        ptr = [ctypes.c_void_p(t.data_ptr()) for t in (self.rows, self.grads, *state, self.step, self.loss)]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for k in range(reps):
            rc = lib.pinn_reduce_rows(ptr[0], self.n, self.p, ptr[1], 0, ptr[2], ptr[3], ptr[4], None, ptr[5], k + 1, ctypes.byref(self.optim),
                                      ptr[6], self.p - 18, self.stream)
            if rc:
                raise RuntimeError(lib.pinn_last_error().decode())
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 / reps, state[0]


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='256x12756,4x628')
    ap.add_argument('--reps', type=int, default=2000)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('libs', nargs='*', default=[engine.library_path()])
    args = ap.parse_args()
    libs = [(os.path.basename(path), load(path)) for path in args.libs]
    for size in args.sizes.split(','):
        n, p = (int(v) for v in size.split('x'))
        case = Case(n, p)
        times = {name: [] for name, _ in libs}
        sums = {}
        for name, lib in libs:
            case.run(lib, 300)          # (code object, clocks)
        for _ in range(args.rounds):
            for name, lib in libs:
                us, params = case.run(lib, args.reps)
                times[name].append(us)
                sums[name] = (lib.pinn_last_reduce_kernel_name().decode(), float(case.grads.double().abs().sum()), float(params.double().abs().sum()))
        for name, _ in libs:
            t = times[name]
            print(f'{n:4d} x {p:6d}  {name:28s} {sums[name][0]:26s} us per launch: ' + ' '.join(f'{v:6.2f}' for v in t) +
                  f'  median {np.median(t):6.2f}   |g|1 {sums[name][1]:.9g} |params|1 {sums[name][2]:.9g}', flush=True)
