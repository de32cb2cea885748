""" What loss-term weights cost `Solver.fit` per iteration: iterations per second on the BASELINE config 2 shape (4 x 64 Tanh, Poisson in
2-D) with one VALUE constraint on 64 fixed points, loss_terms ['equation', 'constraint_0'], at batch 4 096 and 65 536 of
  * `none`      -- loss_weights=None: the plain sum, the terms accumulated into one gradient buffer (the code before loss weights),
  * `constant`  -- loss_weights={'equation': 1.0, 'constraint_0': 25.0}: every term into a row of its own, then pinn_balance_terms,
  * `max_mean`  -- loss_weights=LossBalancer('max_mean'): the same rows, the weights updated on the device every iteration,
same process, same start parameters, the settings alternating, `--repeats` timed windows each, the median reported.

A window is one fit call of `--niters` iterations; the host clock runs from a device synchronise to a device synchronise. Every setting
is warmed up by a fit call of its own first; the collector is frozen and off while the windows run. No target is set in advance: the
weighted fits add three small launches per iteration (statistics, finalize, combine over the flat buffer) and one Python call.
The `none` fit against the commit before this feature is `tools/constraint_rate.py --cells equation value`, run on both trees on the
same box. Needs the device: there is no CPU form of this measurement.

    python tools/loss_balance_rate.py [--out profiles/loss_balance_rate.txt] [--niters 512] [--repeats 3] """
import argparse
import gc
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pinn_configs as pc                # noqa: E402
import pydens_amd as pa                  # noqa: E402

BATCHES = (4096, 65536)
TERMS = ['equation', 'constraint_0']
YG = np.linspace(0.0, 1.0, 64, dtype=np.float32).reshape(-1, 1)
SETTINGS = {'none': lambda: None, 'constant': lambda: {'equation': 1.0, 'constraint_0': 25.0}, 'max_mean': lambda: pa.LossBalancer('max_mean')}


def value_at_the_face(f, x, y):
    return f(np.ones_like(YG), YG) - 1.0


def window(solver, batch, niters, key, start):
    """ one timed fit call from the same start -> iterations per second """
    solver.model.flat.copy_(start)
    weights = SETTINGS[key]()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    solver.fit(niters=niters, batch_size=batch, lr=0.005, loss_terms=TERMS, loss_weights=weights)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    assert solver.last_fit_path == 'fused', (solver.last_fit_path, solver.constraint_errors)
    assert solver.last_fit_balance == {'none': None, 'constant': 'fixed/fused', 'max_mean': 'max_mean/fused'}[key], solver.last_fit_balance
    return niters / seconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'loss_balance_rate.txt'))
    ap.add_argument('--niters', type=int, default=512)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/loss_balance_rate.py measures on the device: no HIP device here')
    keys = list(SETTINGS)
    lines = [f'# tools/loss_balance_rate.py --niters {args.niters} --repeats {args.repeats}: fit(optimizer="Adam", lr=0.005, loss_terms={TERMS}) on the '
             f'config 2 shape, one value constraint on 64 fixed points; per setting the MEDIAN window of {args.repeats} in it/s (slowest - fastest); '
             f'{torch.cuda.get_device_name(0)}',
             f'# {"batch":>7s} | ' + ' | '.join(f'{key + " it/s":>14s} {"min - max":>19s}' for key in keys) + ' | ratios to none']
    print('\n'.join(lines), flush=True)
    cfg = pc.make_config('cfg2', pa.D, torch)
    torch.manual_seed(0)
    solver = pa.Solver(cfg['equation'], **cfg['solver_kwargs'], constraints=value_at_the_face)
    assert solver.constraint_plans[0] is not None, solver.constraint_errors
    start = solver.model.flat.clone()
    gc.collect()
    gc.freeze()
    gc.disable()
    for batch in BATCHES:
        runs = {key: [] for key in keys}
        for key in keys:                                    # warm-up of the setting, not timed
            window(solver, batch, 64, key, start)
        for _ in range(args.repeats):                       # alternating
            for key in keys:
                runs[key].append(window(solver, batch, args.niters, key, start))
        med = {key: sorted(rows)[len(rows) // 2] for key, rows in runs.items()}
        line = f'  {batch:7d} | ' + ' | '.join(f'{med[key]:14.1f} {min(runs[key]):9.1f} -{max(runs[key]):9.1f}' for key in keys)
        line += ' | ' + ' '.join(f'{key} {med[key] / med["none"]:5.3f}' for key in keys if key != 'none')
        print(line, flush=True)
        lines.append(line)
    gc.enable()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
