""" What a learning-rate schedule costs `Solver.fit`: iterations per second of the default fit (plain Adam, on-device sampler) at a constant
rate against the same fit with `lr_scheduler='ExponentialLR'`, on the three chunk forms -- BASELINE config 1 (the one-CU chunk kernel),
config 2 at batch 4 096 (chunks replayed as launch graphs) and config 2 at batch 65 536 (eager chunks) -- same process, same start
parameters, the two settings alternating, `--repeats` timed windows each.

A window is one fit call of `--niters` iterations; the host clock runs from a device synchronise to a device synchronise. Every cell is
warmed up by a fit call of its own first (code objects, workspaces, the recording of the launch graph). The expectation to confirm or refute:
equal rates -- the extra work is one host loop over the chunk's rates per chunk and two uniform loads per block of the reduction.
The comparison of a constant-rate fit with the commit before this feature is `tools/fit_rate.py`'s, run on both commits on the same box.
Needs the device: there is no CPU form of this measurement.

    python tools/lr_schedule_rate.py [--out profiles/lr_schedule_rate.txt] [--niters 2048] [--repeats 3] """
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pinn_configs as pc                # noqa: E402
import pydens_amd as pa                  # noqa: E402

CELLS = (('cfg1', None, 'one-CU chunk'), ('cfg2', 4096, 'launch-graph chunk'), ('cfg2', 65536, 'eager chunk'))
SETTINGS = {'constant': {}, 'ExponentialLR': dict(lr_scheduler='ExponentialLR', lr_scheduler_kwargs=dict(gamma=0.9999))}


def window(solver, batch, niters, setting, start):
    """ one timed fit call from the same start -> iterations per second """
    solver.model.flat.copy_(start)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    solver.fit(niters=niters, batch_size=batch, lr=0.005, **setting)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    assert solver.last_fit_path == 'fused' and solver.last_fit_optimizer == 'Adam/fused', (solver.last_fit_path, solver.last_fit_optimizer)
    assert (solver.lr_scheduler is not None) == bool(setting)
    return niters / seconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'lr_schedule_rate.txt'))
    ap.add_argument('--niters', type=int, default=2048)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/lr_schedule_rate.py measures on the device: no HIP device here')
    lines = [f'# tools/lr_schedule_rate.py --niters {args.niters} --repeats {args.repeats}: fit(optimizer="Adam", lr=0.005) at a constant rate and with '
             f'lr_scheduler="ExponentialLR" (gamma 0.9999), per cell the MEDIAN window of {args.repeats} and the slowest - fastest window; '
             f'{torch.cuda.get_device_name(0)}',
             f'# {"config":6s} {"batch":>7s} {"form":>18s} | {"constant it/s":>13s} {"min - max":>19s} | {"scheduled it/s":>14s} {"min - max":>19s} | ratio']
    print('\n'.join(lines), flush=True)
    for name, batch, form in CELLS:
        cfg = pc.make_config(name, pa.D, torch)
        torch.manual_seed(0)
        solver = pa.Solver(cfg['equation'], **cfg['solver_kwargs'])
        start = solver.model.flat.clone()
        batch = cfg['n_points'] if batch is None else batch
        runs = {key: [] for key in SETTINGS}
        for key, setting in SETTINGS.items():               # warm-up of the cell, not timed
            window(solver, batch, 256, setting, start)
        for _ in range(args.repeats):                       # alternating
            for key, setting in SETTINGS.items():
                runs[key].append(window(solver, batch, args.niters, setting, start))
        med = {key: sorted(rows)[len(rows) // 2] for key, rows in runs.items()}
        span = {key: f'{min(rows):9.1f} -{max(rows):9.1f}' for key, rows in runs.items()}
        line = (f'  {name:6s} {batch:7d} {form:>18s} | {med["constant"]:13.1f} {span["constant"]:>19s} | {med["ExponentialLR"]:14.1f} '
                f'{span["ExponentialLR"]:>19s} | {med["ExponentialLR"] / med["constant"]:5.3f}')
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
