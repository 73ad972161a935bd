#!/usr/bin/env python3
"""Times the fused similarity top-k (cmhar.retrieval.sim_topk) against the torch composite on one shape.

Default shape: the config-5 stream (N = 10 000 clips) against a 100 000-window bank, d = 256, k = 10, in fp32 and
bf16.  The composite is `(q @ bank.T).topk(k)`, chunked over queries so that one chunk's N_c x M scores stay under
`--composite-bytes` (its chunk size is reported; it is not tuned down in any other way).  The four variants are run
alternately, round after round, each timed with device events after warm-up rounds; the JSON carries every round's
time, the median, the achieved TF/s (2·N·M·d over the median) and how far the two results agree.

    python tools/sim_topk_bench.py --out profiles/sim_topk_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'crossmodal-imu-video-ood-har_amd'))

from cmhar import _lib  # noqa: E402
from cmhar.retrieval import sim_topk  # noqa: E402


def composite(q, bank, k, chunk):
    vals, idx = [], []
    for i in range(0, q.shape[0], chunk):
        v, ix = (q[i:i + chunk] @ bank.T).topk(k, dim=1)
        vals.append(v)
        idx.append(ix)
    return torch.cat(vals), torch.cat(idx)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nq', type=int, default=10000)
    ap.add_argument('--nb', type=int, default=100000)
    ap.add_argument('--d', type=int, default=256)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--composite-bytes', type=int, default=1 << 30, help='score bytes of one composite chunk')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'sim_topk_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('sim_topk_bench needs the GPU (there is no CPU path to time)')
    dev = 'cuda'
    g = torch.Generator(device=dev).manual_seed(0)
    q32 = torch.nn.functional.normalize(torch.randn(a.nq, a.d, device=dev, generator=g), dim=1)
    b32 = torch.nn.functional.normalize(torch.randn(a.nb, a.d, device=dev, generator=g), dim=1)
    data = {'fp32': (q32, b32), 'bf16': (q32.bfloat16(), b32.bfloat16())}
    chunk = {n: max(1, min(a.nq, a.composite_bytes // (a.nb * t[0].element_size()))) for n, t in data.items()}
    variants = {}
    for n, (q, b) in data.items():
        variants[f'fused_{n}'] = (lambda q=q, b=b: sim_topk(q, b, a.k))
        variants[f'composite_{n}'] = (lambda q=q, b=b, c=chunk[n]: composite(q, b, a.k, c))
    times = {n: [] for n in variants}
    outs = {}
    for r in range(a.warmup + a.rounds):
        for n, fn in variants.items():                  # alternated: one call of each per round
            ms, out = timed(fn)
            if r >= a.warmup:
                times[n].append(ms)
            outs[n] = out
    flop = 2.0 * a.nq * a.nb * a.d
    res = {'shape': {'nq': a.nq, 'nb': a.nb, 'd': a.d, 'k': a.k}, 'device': torch.cuda.get_device_name(0),
           'rounds': a.rounds, 'warmup_rounds': a.warmup, 'timing': 'device events, variants alternated per round',
           'splits': int(_lib.lib().cmhar_sim_topk_splits(a.nq, a.nb, a.k)),
           'fused_workspace_bytes': int(_lib.lib().cmhar_sim_topk_ws(a.nq, a.nb, a.k)), 'variants': {}}
    for n, ts in times.items():
        med = statistics.median(ts)
        res['variants'][n] = {'ms_median': round(med, 4), 'ms_min': round(min(ts), 4), 'ms_max': round(max(ts), 4),
                              'ms_all': [round(t, 4) for t in ts], 'tflops_at_median': round(flop / med / 1e9, 2)}
    for n in data:
        res['variants'][f'composite_{n}']['chunk_queries'] = chunk[n]
        res['variants'][f'composite_{n}']['chunk_score_bytes'] = chunk[n] * a.nb * data[n][0].element_size()
        fv, fi = outs[f'fused_{n}']
        cv, ci = outs[f'composite_{n}']
        res[f'agreement_{n}'] = {'index_match_fraction': float((fi == ci).float().mean()),
                                 'max_abs_value_diff': float((fv - cv.float()).abs().max())}
        f, c = res['variants'][f'fused_{n}']['ms_median'], res['variants'][f'composite_{n}']['ms_median']
        res[f'speedup_{n}'] = round(c / f, 3)
    res['gate_fused_no_slower'] = all(res[f'speedup_{n}'] >= 1.0 for n in data)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
