"""Developer aid (round 5): rewrites `__global__ void NAME(params) { body }` in a .hip file into
`__device__ NAME_body(const dim3 blockIdx, const dim3 gridDim, params) { body }` (lockstep.h generates the kernels that run it) for
the kernels named on the command line, and prints each kernel's launch bounds: they go to its rdm::launch<NAME_body, THREADS[, MIN_WAVES]>
(tools/to_launch.py takes THREADS from the launch).   python tools/to_body.py FILE NAME [NAME ...]"""
import re, sys


def convert(src, name):
    m = re.search(r'((?:template\s*<[^>]*>\s*\n)?)(static\s+)?__global__\s*((?:__launch_bounds__\([^)]*(?:\([^)]*\)[^)]*)*\)\s*)?)void\s+' + re.escape(name) + r'\s*\(', src)
    assert m, name
    tmpl, bounds = m.group(1), m.group(3)
    i = m.end()
    depth, j = 1, i
    while depth:
        depth += {'(': 1, ')': -1}.get(src[j], 0)
        j += 1
    params = src[i:j - 1]
    k = src.index('{', j)
    end = src.index('\n}\n', k) + 2  # kernels close at column 0
    body = src[k + 1:end - 1]
    sep = ', ' if params.strip() else ''
    print(f'{name}: {bounds.strip() or "no launch bounds"}', file=sys.stderr)
    new = (f'{tmpl}__device__ __forceinline__ void {name}_body(const dim3 blockIdx, const dim3 gridDim{sep}{params}) {{\n'
           f'  (void)blockIdx; (void)gridDim;{body}}}\n')
    return src[:m.start()] + new + src[end:]


if __name__ == '__main__':
    path = sys.argv[1]
    s = open(path).read()
    for n in sys.argv[2:]:
        s = convert(s, n)
    open(path, 'w').write(s)  # (only after every conversion succeeded)
