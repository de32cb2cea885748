""" User-facing Solver.fit rate (iterations/s, points/s) for the BASELINE configs, default on-device sampler (cfg4: the
README's two-column NumpySampler product). One fresh process per config (tools/fit_one.py): inside one process the
later configs inherit recycled allocator blocks and a warm chip from the earlier ones and cfg3 measured 5 % slower.
--criterion NAME (a torch.nn loss module with its defaults, e.g. L1Loss) and --criterion-path generic|fused
(Solver.set_criterion_path) time a fit with another criterion; --optimizer NAME, --optimizer-kwargs JSON and --optimizer-path torch|fused
(Solver.set_optimizer_path) one with another torch.optim update rule; --configs picks the configs (default: all five). """
import argparse, os, subprocess, sys
HERE = os.path.dirname(os.path.abspath(__file__))
ITERS = {'cfg1': 12800, 'cfg2': 300, 'cfg4': 300, 'cfg3': 40, 'cfg5': 20}
ap = argparse.ArgumentParser()
ap.add_argument('--criterion', default='MSELoss')
ap.add_argument('--criterion-path', choices=('generic', 'fused'), default='generic')
ap.add_argument('--optimizer', default='Adam')
ap.add_argument('--optimizer-kwargs', default='{}')
ap.add_argument('--optimizer-path', choices=('torch', 'fused'), default='torch')
ap.add_argument('--configs', nargs='*', default=list(ITERS), choices=list(ITERS))
args = ap.parse_args()
for name in args.configs:
    out = subprocess.run([sys.executable, os.path.join(HERE, 'fit_one.py'), name, str(ITERS[name]), args.criterion, args.criterion_path,
                          '--optimizer', args.optimizer, '--optimizer-kwargs', args.optimizer_kwargs, '--optimizer-path', args.optimizer_path],
                         capture_output=True, text=True)
    lines = [l for l in out.stdout.splitlines() if l.startswith(name)]
    print('\n'.join(lines) if lines else f'{name}: FAILED\n{out.stdout[-400:]}\n{out.stderr[-400:]}', flush=True)
