""" What residual-adaptive sampling costs on the device.

  1. Iterations per second of a BASELINE-config-2-shaped fit (4 x 64 Poisson) at batch 65 536 and 4 096 with `ResidualSampler(pool=4)` at
     period 1 and 10, against the same fit fed uniform batches by an external sampler without `columns()` (the per-iteration path for
     supplied points) -- same process, same start parameters, the cells of a batch size alternating, `--repeats` timed windows each,
     the median window reported with the spread.
  2. The three resampler launches (pinn_resample_points) and the one-launch redraw against the torch composition a user would write
     (abs / pow, cumsum in fp64, rand, searchsorted, index_select) at M = 262 144, n_out = 65 536, d = 2: microseconds per call by the
     host clock over `--calls` calls between two device synchronisations (launch overhead included).

The defaults are short windows for a quick look; profiles/resample_rate.txt was recorded with `--niters 2000 --calls 1000` (the header
of the output names the values used).

Needs the device: there is no CPU form of this measurement.

    python tools/resample_rate.py [--out profiles/resample_rate.txt] [--niters 200] [--repeats 3] [--calls 200] """
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pinn_configs as pc                # noqa: E402
import pydens_amd as pa                  # noqa: E402


class UniformExternal:
    """ U[0, 1) batches drawn on the device by a sampler the solver knows nothing about: no `columns()`, so no one-launch fit chunks """
    dim = 2

    def sample_device(self, size, device, generator=None):
        return torch.rand((size, self.dim), dtype=torch.float32, device=device, generator=generator)


def window(solver, start, sampler, batch, niters):
    solver.model.flat.copy_(start)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    solver.fit(niters=niters, batch_size=batch, sampler=sampler)
    torch.cuda.synchronize()
    return niters / (time.perf_counter() - t0)


def timed(fn, calls):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'resample_rate.txt'))
    ap.add_argument('--niters', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/resample_rate.py measures on the device: no HIP device here')
    lines = [f'# tools/resample_rate.py --niters {args.niters} --repeats {args.repeats} --calls {args.calls}; {torch.cuda.get_device_name(0)}',
             '# 1. fit of BASELINE config 2 (4 x 64 Poisson, Adam): iterations per second, MEDIAN window (slowest - fastest) of the repeats; the cells of a',
             '#    batch size alternate inside every repeat. external: uniform batches from a sampler without columns() (the path for supplied points);',
             '#    ratio: that cell over the external one',
             f'# {"batch":>7s} | {"external it/s":>26s} | {"pool=4 period=1 it/s":>26s} {"ratio":>6s} | {"pool=4 period=10 it/s":>26s} {"ratio":>6s}']
    print('\n'.join(lines), flush=True)
    cfg = pc.make_config('cfg2', pa.D, torch)
    torch.manual_seed(0)
    solver = pa.Solver(cfg['equation'], **cfg['solver_kwargs'])
    start = solver.model.flat.clone()
    for batch in (65536, 4096):
        cells = {'external': UniformExternal, 'period1': lambda: pa.ResidualSampler(pool=4, period=1),
                 'period10': lambda: pa.ResidualSampler(pool=4, period=10)}
        runs = {key: [] for key in cells}
        for key, make in cells.items():                  # warm-up of every cell, not timed
            window(solver, start, make(), batch, 12)
        for _ in range(args.repeats):
            for key, make in cells.items():
                torch.manual_seed(1)
                runs[key].append(window(solver, start, make(), batch, args.niters))
        med = {key: sorted(v)[len(v) // 2] for key, v in runs.items()}
        cell = lambda key: f'{med[key]:9.1f} ({min(runs[key]):7.1f} - {max(runs[key]):7.1f})'
        line = (f'  {batch:7d} | {cell("external"):>26s} | {cell("period1"):>26s} {med["period1"] / med["external"]:6.2f} | '
                f'{cell("period10"):>26s} {med["period10"] / med["external"]:6.2f}')
        print(line, flush=True)
        lines.append(line)

    m, n_out, d = 262144, 65536, 2
    gen = torch.Generator(device='cuda')
    gen.manual_seed(3)
    pool = torch.rand((m, d), device='cuda', generator=gen)
    r = torch.randn(m, device='cuda', generator=gen)
    net = solver.model.net
    ws = net.resample_workspace(m, pool.device)
    out = torch.empty((n_out, d), device='cuda')
    idx = torch.empty(n_out, dtype=torch.int32, device='cuda')
    state = {'call': 0}

    def kernels(redraw=False):
        state['call'] += 1
        net.resample_points(pool, r, n_out, 1, 1.0, 7, state['call'], workspace=ws, out=out, idx=idx, redraw=redraw)

    def composition():
        w = r.double().abs()
        q = w + 1.0 * w.mean()
        cdf = torch.cumsum(q, 0)
        t = torch.rand(n_out, dtype=torch.float64, device='cuda', generator=gen) * cdf[-1]
        j = torch.searchsorted(cdf, t, right=True).clamp_(max=m - 1)
        return pool.index_select(0, j)
    rows = []
    for _ in range(args.repeats):                        # alternating
        rows.append((timed(kernels, args.calls), timed(lambda: kernels(True), args.calls), timed(composition, args.calls)))
    med = [sorted(col)[len(col) // 2] for col in zip(*rows)]
    spread = [f'{min(col):.1f} - {max(col):.1f}' for col in zip(*rows)]
    tail = [f'# 2. one selection at M = {m}, n_out = {n_out}, d = {d}: microseconds per call (host clock over {args.calls} calls between two device',
            '#    synchronisations: launch overhead included), median of the repeats (fastest - slowest)',
            f'  pinn_resample_points (3 launches)      {med[0]:8.1f} us  ({spread[0]})',
            f'  pinn_resample_redraw (1 launch)        {med[1]:8.1f} us  ({spread[1]})',
            f'  torch abs/mean/add, cumsum, rand, searchsorted, index_select  {med[2]:8.1f} us  ({spread[2]})',
            f'  composition over three launches: {med[2] / med[0]:.2f}']
    print('\n'.join(tail), flush=True)
    lines += tail
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
