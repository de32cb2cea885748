""" What causal weights cost `Solver.fit` per iteration: iterations per second on the heat-in-(x, t) problem of the `heat64` workload (4 x 64
Tanh, initial and boundary condition) at batch 4 096 and 65 536 of
  * `generic`  -- causal=None on the generic step (`solver.use_fused = False`): the step the causal fit is built on,
  * `causal`   -- causal=CausalWeights(bins=32): the same step with pinn_causal_weights between its two halves,
same process, same start parameters, the settings alternating, `--repeats` timed windows each, the median reported; and the time of the
three launches of pinn_causal_weights alone at n = 65 536, 32 bins (device events around `--calls` back-to-back calls).

A window is one fit call of `--niters` iterations; the host clock runs from a device synchronise to a device synchronise. Every setting
is warmed up by a fit call of its own first; the collector is frozen and off while the windows run. No target is set in advance. The
fused tile kernels do not serve a causal fit; the fit with causal=None against the commit before this feature is `tools/fit_rate.py`, run
on both trees on the same box. Needs the device: there is no CPU form of this measurement.

    python tools/causal_rate.py [--out profiles/causal_rate.txt] [--niters 256] [--repeats 3] [--calls 200] """
import argparse
import gc
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pinn_configs as pc                # noqa: E402
import pydens_amd as pa                  # noqa: E402

BATCHES = (4096, 65536)
SETTINGS = {'generic': lambda: None, 'causal': lambda: pa.CausalWeights(bins=32)}


def window(solver, batch, niters, key, start):
    """ one timed fit call from the same start -> iterations per second """
    solver.model.flat.copy_(start)
    causal = SETTINGS[key]()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    solver.fit(niters=niters, batch_size=batch, lr=0.005, causal=causal)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    assert solver.last_fit_path == 'generic' and solver.last_fit_causal == {'generic': None, 'causal': 'bins32/generic'}[key]
    return niters / seconds


def launches_alone(net, n, bins, calls):
    """ microseconds per pinn_causal_weights call (three launches), back to back on one stream """
    xs = torch.rand((n, 2), device='cuda')
    r = torch.randn(n, device='cuda')
    state = net.causal_state([1.0], 0.99, 'cuda')
    ws, w = net.causal_workspace(n, bins, 'cuda'), torch.empty(n, device='cuda')
    for _ in range(20):
        net.causal_weights(xs, 1, r, bins, 0.0, 1.0, True, state, w, ws)
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    begin.record()
    for _ in range(calls):
        net.causal_weights(xs, 1, r, bins, 0.0, 1.0, True, state, w, ws)
    end.record()
    torch.cuda.synchronize()
    return 1e3 * begin.elapsed_time(end) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'causal_rate.txt'))
    ap.add_argument('--niters', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/causal_rate.py measures on the device: no HIP device here')
    keys = list(SETTINGS)
    lines = [f'# tools/causal_rate.py --niters {args.niters} --repeats {args.repeats}: fit(optimizer="Adam", lr=0.005) on the heat64 shape, generic step '
             f'(use_fused = False); per setting the MEDIAN window of {args.repeats} in it/s (slowest - fastest); {torch.cuda.get_device_name(0)}',
             f'# {"batch":>7s} | ' + ' | '.join(f'{key + " it/s":>14s} {"min - max":>19s}' for key in keys) + ' | causal / generic']
    print('\n'.join(lines), flush=True)
    cfg = pc.make_config('heat64', pa.D, torch)
    torch.manual_seed(0)
    solver = pa.Solver(cfg['equation'], **cfg['solver_kwargs'])
    solver.use_fused = False
    start = solver.model.flat.clone()
    gc.collect()
    gc.freeze()
    gc.disable()
    for batch in BATCHES:
        runs = {key: [] for key in keys}
        for key in keys:                                    # warm-up of the setting, not timed
            window(solver, batch, 48, key, start)
        for _ in range(args.repeats):                       # alternating
            for key in keys:
                runs[key].append(window(solver, batch, args.niters, key, start))
        med = {key: sorted(rows)[len(rows) // 2] for key, rows in runs.items()}
        line = f'  {batch:7d} | ' + ' | '.join(f'{med[key]:14.1f} {min(runs[key]):9.1f} -{max(runs[key]):9.1f}' for key in keys)
        line += f' | {med["causal"] / med["generic"]:5.3f}'
        print(line, flush=True)
        lines.append(line)
    gc.enable()
    us = launches_alone(solver.model.net, 65536, 32, args.calls)
    line = f'# pinn_causal_weights alone, n = 65536, 32 bins: {us:.1f} us per call (three launches; mean of {args.calls} back-to-back calls)'
    print(line, flush=True)
    lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
