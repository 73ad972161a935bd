#!/usr/bin/env python3
"""Times the two Mahalanobis kernels (cmhar.ood.class_moments / class_min_dist) against their torch composites.

Shapes: N = 100 000 feature rows, C = 32 classes, d in {128, 256, 768}, fp32 and bf16 features.  The composites do
the same fp32 math with torch ops (16-bit features are widened with `.float()` first, as the kernels widen on load):
  class_moments   counts by bincount, means by `index_add_`, then the centred rows R = x − μ[y] and `R.T @ R`
                  (this stores the N x d centred rows and computes the full d x d product);
  class_min_dist  `z = x @ W.T`, `torch.cdist(z, m) ** 2`, `.min(1)`, chunked over rows so that one chunk's z and
                  distances stay under `--composite-bytes` (the chunk size is reported).
All variants of one shape are run alternately, round after round, each timed with device events after warm-up
rounds; the JSON carries every round's time, the median and min, the achieved TF/s of the kernels and the error of
both results against fp64 on the same features.  No speed-up is asserted: the file states what was measured, on which
build.

    python tools/mahalanobis_bench.py --out profiles/mahalanobis_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'crossmodal-imu-video-ood-har_amd'))

from cmhar import _lib  # noqa: E402
from cmhar.ood import class_min_dist, class_moments  # noqa: E402


def composite_moments(x, y, C):
    x = x.float()
    counts = torch.bincount(y, minlength=C)
    means = torch.zeros(C, x.shape[1], device=x.device).index_add_(0, y, x) / counts.clamp(min=1)[:, None]
    R = x - means[y]
    return counts, means, R.T @ R


def composite_min_dist(x, W, m, chunk):
    d2, cls = [], []
    for i in range(0, x.shape[0], chunk):
        v, c = (torch.cdist(x[i:i + chunk].float() @ W.T, m) ** 2).min(1)
        d2.append(v)
        cls.append(c)
    return torch.cat(d2), torch.cat(cls)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def build_id():
    try:
        return subprocess.run(['git', '-C', REPO, 'describe', '--always', '--dirty'], capture_output=True, text=True,
                              check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return 'unknown'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--classes', type=int, default=32)
    ap.add_argument('--d', type=int, nargs='+', default=[128, 256, 768])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--composite-bytes', type=int, default=1 << 30, help='z + distance bytes of one composite chunk')
    ap.add_argument('--build', default=None, help='what to record as the measured build (default: git describe)')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mahalanobis_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('mahalanobis_bench needs the GPU (there is no CPU path to time)')
    dev = 'cuda'
    N, C = a.n, a.classes
    res = {'shape': {'N': N, 'C': C, 'd': a.d}, 'device': torch.cuda.get_device_name(0),
           'build': a.build or build_id(), 'library_version': int(_lib.lib().cmhar_version()), 'rounds': a.rounds,
           'warmup_rounds': a.warmup, 'timing': 'device events, variants alternated per round', 'cases': {}}
    for d in a.d:
        g = torch.Generator(device=dev).manual_seed(d)
        y = torch.arange(N, device=dev) % C
        mu = 2 * torch.randn(C, d, device=dev, generator=g)
        x32 = mu[y] + torch.randn(N, d, device=dev, generator=g)
        W = torch.randn(d, d, device=dev, generator=g) / d ** 0.5
        m = mu @ W.T
        chunk = max(1, min(N, a.composite_bytes // (4 * (d + C))))
        variants = {}
        for n, x in (('fp32', x32), ('bf16', x32.bfloat16())):
            variants[f'moments_kernel_{n}'] = (lambda x=x: class_moments(x, y, C))
            variants[f'moments_composite_{n}'] = (lambda x=x: composite_moments(x, y, C))
            variants[f'min_dist_kernel_{n}'] = (lambda x=x: class_min_dist(x, W, m))
            variants[f'min_dist_composite_{n}'] = (lambda x=x: composite_min_dist(x, W, m, chunk))
        times = {n: [] for n in variants}
        outs = {}
        for r in range(a.warmup + a.rounds):
            for n, fn in variants.items():              # alternated: one call of each per round
                ms, out = timed(fn)
                if r >= a.warmup:
                    times[n].append(ms)
                outs[n] = out
        # useful work: class sums + upper-triangle scatter; whitening GEMM + the class loop (3 flops per term)
        flop = {'moments': 2.0 * N * d + N * d * (d + 1.0), 'min_dist': 2.0 * N * d * d + 3.0 * N * C * d}
        case = {'moments_workspace_bytes': int(_lib.lib().cmhar_class_moments_ws(N, d, C)),
                'min_dist_composite_chunk_rows': chunk, 'min_dist_composite_chunk_bytes': chunk * 4 * (d + C),
                'variants': {}}
        for n, ts in times.items():
            med = statistics.median(ts)
            case['variants'][n] = {'ms_median': round(med, 4), 'ms_min': round(min(ts), 4),
                                   'ms_max': round(max(ts), 4), 'ms_all': [round(t, 4) for t in ts]}
            if '_kernel_' in n:
                case['variants'][n]['tflops_at_median'] = round(flop[n.split('_kernel_')[0]] / med / 1e9, 2)
        for n in ('fp32', 'bf16'):
            for op in ('moments', 'min_dist'):
                k, c = (case['variants'][f'{op}_{v}_{n}']['ms_median'] for v in ('kernel', 'composite'))
                case[f'composite_over_kernel_{op}_{n}'] = round(c / k, 3)
            kc, km, ks = outs[f'moments_kernel_{n}']
            cc, cm, cs = outs[f'moments_composite_{n}']
            kd, kcls = outs[f'min_dist_kernel_{n}']
            cd, ccls = outs[f'min_dist_composite_{n}']
            # both against fp64 on the same (already rounded) features
            xd = (x32 if n == 'fp32' else x32.bfloat16()).double()
            m64 = torch.zeros(C, d, device=dev, dtype=torch.float64).index_add_(0, y, xd) / cc[:, None]
            R = xd - m64[y]
            s64 = R.T @ R
            z = xd @ W.double().T
            d64 = torch.stack([((z - m[c].double()) ** 2).sum(1) for c in range(C)], 1).min(1).values
            del xd, R, z
            case[f'agreement_{n}'] = {
                'counts_equal': bool(torch.equal(kc, cc)),
                'class_match_fraction': float((kcls == ccls).float().mean()),
                'means_max_abs_err_vs_fp64': {'kernel': float((km - m64).abs().max()),
                                              'composite': float((cm - m64).abs().max())},
                'scatter_rel_frobenius_err_vs_fp64': {'kernel': float((ks - s64).norm() / s64.norm()),
                                                      'composite': float((cs - s64).norm() / s64.norm())},
                'dist2_max_rel_err_vs_fp64': {'kernel': float(((kd - d64).abs() / d64).max()),
                                              'composite': float(((cd - d64).abs() / d64).max())}}
        res['cases'][f'd{d}'] = case
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
