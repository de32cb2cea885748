""" Registers, spills and scratch of the small kernels around the update rule -- every pinn_fit_kernel instantiation, pinn_reduce_kernel,
pinn_optim_kernel -- read from the code-object metadata of a BUILT library (tools/kernel_resources.sh covers the tile and weight-gradient
kernels of widths >= 64 from assembly; the fit kernels live in the narrow units). No GPU needed.
Usage: python tools/fit_kernel_resources.py [libpinn_hip.so [other.so]]      (two libraries: the second one's figures beside the first's) """
import os, re, struct, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
WANTED = ('pinn_fit_kernel', 'pinn_reduce_kernel', 'pinn_optim_kernel', 'pinn_adam_kernel')


def kernels(path):
    """ {demangled name: (vgprs, spilled vgprs, spilled sgprs, scratch bytes)} of the gfx950 code objects bundled into a shared library """
    data, out, tmp = open(path, 'rb').read(), {}, tempfile.mkdtemp()
    magic = b'__CLANG_OFFLOAD_BUNDLE__'
    pos, count = data.find(magic), 0
    while pos != -1:
        entries, off = struct.unpack_from('<Q', data, pos + 24)[0], pos + 32
        for _ in range(entries):
            start, size, tlen = struct.unpack_from('<QQQ', data, off)
            triple = data[off + 24:off + 24 + tlen].decode()
            off += 24 + tlen
            if 'gfx950' not in triple or size == 0:
                continue
            elf = os.path.join(tmp, f'co{count}.elf')
            count += 1
            open(elf, 'wb').write(data[pos + start:pos + start + size])
            notes = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', elf], capture_output=True, text=True).stdout
            for block in notes.split('  - .agpr_count')[1:]:
                name = re.search(r'\.name:\s+(\S+)', block)
                if name and any(w in name.group(1) for w in WANTED):
                    field = lambda key: int(re.search(r'\.' + key + r':\s+(\d+)', block).group(1))
                    out[name.group(1)] = (field('vgpr_count'), field('vgpr_spill_count'), field('sgpr_spill_count'), field('private_segment_fixed_size'))
        pos = data.find(magic, pos + 1)
    names = subprocess.run(['c++filt'], input='\n'.join(out), capture_output=True, text=True).stdout.split('\n')
    return {n.split('(')[0].replace('void ', '').replace('pinn_adam_kernel', 'pinn_optim_kernel'): v for n, v in zip(names, out.values())}


def main():
    libs = sys.argv[1:] or [os.path.join(ROOT, 'pydens_amd', 'libpinn_hip.so')]
    tables = [kernels(p) for p in libs]
    print('# kernel | vgprs | spilled vgprs | spilled sgprs | scratch bytes' + (' || the same of the second library' if len(tables) > 1 else ''))
    for name in sorted(tables[0]):
        row = '  '.join(f'{v:5d}' for v in tables[0][name])
        if len(tables) > 1 and name in tables[1]:
            row += '  ||  ' + '  '.join(f'{v:5d}' for v in tables[1][name])
        print(f'{name:62s} {row}')
    if len(tables) > 1:
        both = [n for n in tables[0] if n in tables[1] and 'pinn_fit_kernel' in n]
        delta = sorted(tables[0][n][3] - tables[1][n][3] for n in both)
        print(f'# scratch bytes of {len(both)} pinn_fit_kernel instantiations, first minus second: min {delta[0]}, median {delta[len(delta) // 2]}, max {delta[-1]}; '
              f'{sum(d > 0 for d in delta)} more, {sum(d < 0 for d in delta)} less')


if __name__ == '__main__':
    main()
