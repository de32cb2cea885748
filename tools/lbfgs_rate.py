""" Closure evaluations per second and inner iterations per second of `Solver.fit(optimizer='LBFGS')`: BASELINE config 2 and config 3 shapes
(network, equation, batch), history_size 10 and 100, with and without 'strong_wolfe', torch.optim.LBFGS stepped through the closure (the
'torch' optimizer path) against FlatLBFGS with the direction kernels (the 'fused' path) -- same process, same start parameters, the two
paths alternating, `--repeats` timed windows each.

A window is one fit call of `--niters` iterations at max_iter inner iterations each, on the on-device sampler; the host clock runs from a
device synchronise to a device synchronise. Every cell is warmed up by a fit call of its own first (code objects, workspaces, the history
buffers). The history fills as the window runs: `--niters` x max_iter is chosen above history_size 100 so that the larger history is live
for most of the window. Needs the device: there is no CPU form of this measurement.

    python tools/lbfgs_rate.py [--out profiles/lbfgs_rate.txt] [--niters 8] [--max-iter 20] [--repeats 3] """
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pinn_configs as pc                # noqa: E402
import pydens_amd as pa                  # noqa: E402


def window(solver, path, batch, niters, setting, start):
    """ one timed fit call from the same start -> (seconds, closure evaluations, inner iterations) """
    solver.model.flat.copy_(start)
    solver.set_optimizer_path(path)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    solver.fit(niters=niters, batch_size=batch, optimizer='LBFGS', **setting)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    opt = solver.optimizer
    if path == 'fused':
        evals, inner, pairs = opt.func_evals, opt.n_iter, opt.state['history']
    else:
        state = opt.opt.state[opt.opt._params[0]]
        evals, inner, pairs = state['func_evals'], state['n_iter'], len(state.get('old_dirs') or [])
    assert solver.last_fit_optimizer == f'LBFGS/{path}', solver.last_fit_optimizer
    return seconds, evals, inner, pairs, float(solver.losses[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'lbfgs_rate.txt'))
    ap.add_argument('--niters', type=int, default=8)
    ap.add_argument('--max-iter', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--configs', default='cfg2,cfg3')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/lbfgs_rate.py measures on the device: no HIP device here')
    lines = [f'# tools/lbfgs_rate.py --niters {args.niters} --max-iter {args.max_iter} --repeats {args.repeats}: fit(optimizer="LBFGS"), lr 1 with the line search and 0.1 without, '
             f'max_iter {args.max_iter} (max_eval torch\'s default), per cell the MEDIAN window of {args.repeats}; {torch.cuda.get_device_name(0)}',
             '# evals/s: closure evaluations per second; it/s: inner iterations per second; ratio: fused evals/s over torch evals/s (medians); spread: slowest fused window over fastest torch window - fastest fused over slowest torch',
             f'# {"config":6s} {"batch":>7s} {"history":>7s} {"line search":>12s} | {"torch evals/s":>13s} {"it/s":>8s} {"evals":>6s} | '
             f'{"fused evals/s":>13s} {"it/s":>8s} {"evals":>6s} | {"ratio":>6s} {"spread":>13s} | pairs held and last loss at the end of the window, torch/fused']
    print('\n'.join(lines), flush=True)
    for name in args.configs.split(','):
        cfg = pc.make_config(name, pa.D, torch)
        torch.manual_seed(0)
        solver = pa.Solver(cfg['equation'], **cfg['solver_kwargs'])
        start = solver.model.flat.clone()
        batch = cfg['n_points']
        for history in (10, 100):
            for search in (None, 'strong_wolfe'):
                # (the fixed-step rule at lr 1 leaves the basin on these problems and stops accepting pairs: lr 0.1 keeps the history filling)
                setting = dict(lr=1 if search else 0.1, max_iter=args.max_iter, history_size=history, line_search_fn=search)
                runs = {'torch': [], 'fused': []}
                for path in ('torch', 'fused'):                     # warm-up of the cell, not timed
                    window(solver, path, batch, 2, setting, start)
                for _ in range(args.repeats):                       # alternating
                    for path in ('torch', 'fused'):
                        torch.manual_seed(1)                        # the same batches for both paths
                        runs[path].append(window(solver, path, batch, args.niters, setting, start))
                med = {}
                for path, rows in runs.items():
                    rows = sorted(rows, key=lambda r: r[1] / r[0])
                    s, e, i, pairs, loss = rows[len(rows) // 2]
                    med[path] = (e / s, i / s, e, rows[0][1] / rows[0][0], rows[-1][1] / rows[-1][0], pairs, loss)
                ratio = med['fused'][0] / med['torch'][0]
                spread = f"{med['fused'][3] / med['torch'][4]:.2f}-{med['fused'][4] / med['torch'][3]:.2f}"
                line = (f'  {name:6s} {batch:7d} {history:7d} {str(search):>12s} | {med["torch"][0]:13.1f} {med["torch"][1]:8.1f} {med["torch"][2]:6d} | '
                        f'{med["fused"][0]:13.1f} {med["fused"][1]:8.1f} {med["fused"][2]:6d} | {ratio:6.2f} {spread:>13s} | '
                        f'{med["torch"][5]:3d}/{med["fused"][5]:3d} {med["torch"][6]:.3e}/{med["fused"][6]:.3e}')
                print(line, flush=True)
                lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
