""" What a lowered constraint term costs `Solver.fit` per iteration: iterations per second on the BASELINE config 2 shape (4 x 64 Tanh,
Poisson in 2-D) at batch 4 096 and 65 536 of
  * `equation`            -- the equation-only fit (one-launch fit chunks),
  * `value`               -- loss_terms ['equation', 'constraint_0'], the constraint being the model's VALUE at 64 fixed points
                             (the commit before derivative constraints runs this cell too: `--cells equation value` there),
  * `neumann`             -- the same with the Neumann term D(f(x1, yg), x1) - 2 on the same 64 points of the face x = 1,
same process, same start parameters, the cells alternating, `--repeats` timed windows each, the median reported.

A window is one fit call of `--niters` iterations; the host clock runs from a device synchronise to a device synchronise. Every cell is
warmed up by a fit call of its own first; the collector is frozen and off while the windows run (tools/fit_one.py). The expectation to
confirm or refute: the derivative term costs what the value term costs plus the difference between the nd = 0 and the nd = 1
instantiation on 64 points -- one small launch either way. Needs the device: there is no CPU form of this measurement.

    python tools/constraint_rate.py [--out profiles/constraint_rate.txt] [--niters 512] [--repeats 3] [--cells equation value neumann]
                                    [--label TEXT] [--append] """
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
YG = np.linspace(0.0, 1.0, 64, dtype=np.float32).reshape(-1, 1)


def value_at_the_face(f, x, y):
    return f(np.ones_like(YG), YG) - 1.0


def neumann_at_the_face(f, x, y):
    x1 = torch.ones((64, 1), requires_grad=True)
    return pa.D(f(x1, torch.from_numpy(YG)), x1) - 2.0


CELLS = {'equation': (None, 'equation'), 'value': (value_at_the_face, ['equation', 'constraint_0']),
         'neumann': (neumann_at_the_face, ['equation', 'constraint_0'])}


def window(solver, batch, niters, terms, start):
    """ one timed fit call from the same start -> iterations per second """
    solver.model.flat.copy_(start)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    solver.fit(niters=niters, batch_size=batch, lr=0.005, loss_terms=terms)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    assert solver.last_fit_path == 'fused', (solver.last_fit_path, solver.constraint_errors)
    return niters / seconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'constraint_rate.txt'))
    ap.add_argument('--niters', type=int, default=512)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--cells', nargs='*', default=list(CELLS), choices=list(CELLS))
    ap.add_argument('--label', default='this commit', help='which tree is measured; goes into the header line')
    ap.add_argument('--append', action='store_true', help='add to --out instead of replacing it (the second of two trees)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/constraint_rate.py measures on the device: no HIP device here')
    lines = [f'# [{args.label}] tools/constraint_rate.py --niters {args.niters} --repeats {args.repeats} --cells {" ".join(args.cells)}: fit(optimizer="Adam", lr=0.005) on '
             f'the config 2 shape; per cell the MEDIAN window of {args.repeats} in it/s (slowest - fastest); {torch.cuda.get_device_name(0)}',
             f'# {"batch":>7s} | ' + ' | '.join(f'{key + " it/s":>14s} {"min - max":>19s}' for key in args.cells) + ' | ratios to equation']
    print('\n'.join(lines), flush=True)
    cfg = pc.make_config('cfg2', pa.D, torch)
    solvers = {}
    for key in args.cells:
        torch.manual_seed(0)
        constraint = CELLS[key][0]
        solvers[key] = pa.Solver(cfg['equation'], **cfg['solver_kwargs'], **({} if constraint is None else dict(constraints=constraint)))
        if constraint is not None:
            assert solvers[key].constraint_plans[0] is not None, solvers[key].constraint_errors
    starts = {key: solver.model.flat.clone() for key, solver in solvers.items()}
    gc.collect()
    gc.freeze()
    gc.disable()
    for batch in BATCHES:
        runs = {key: [] for key in args.cells}
        for key in args.cells:                              # warm-up of the cell, not timed
            window(solvers[key], batch, 64, CELLS[key][1], starts[key])
        for _ in range(args.repeats):                       # alternating
            for key in args.cells:
                runs[key].append(window(solvers[key], batch, args.niters, CELLS[key][1], starts[key]))
        med = {key: sorted(rows)[len(rows) // 2] for key, rows in runs.items()}
        line = f'  {batch:7d} | ' + ' | '.join(f'{med[key]:14.1f} {min(runs[key]):9.1f} -{max(runs[key]):9.1f}' for key in args.cells)
        if 'equation' in med:
            line += ' | ' + ' '.join(f'{key} {med[key] / med["equation"]:5.3f}' for key in args.cells if key != 'equation')
        print(line, flush=True)
        lines.append(line)
    gc.enable()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a' if args.append else 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
