#!/usr/bin/env python3
"""Times forward + backward of `cmhar.losses.SoftmaxContrastiveLoss` through the module, D = 256, B in {32, 256, 1024,
4096, 16384}, against two other arms on the same inputs:

* `InfoNCELoss(0.07)`, the composite of GEMM and cross-entropy launches that stores S and dS (unchanged code);
* a torch composite of the same formula under autograd (it stores the B x B matrices too).

One call = loss(a, b) and loss.backward() with the embeddings requiring gradients; the new loss runs with
`learnable=False` (a fixed logit scale of 1/0.07, like the other two arms).  The arms are run alternately, round after
round, each call timed with device events after warm-up rounds; the JSON carries the median, minimum and maximum per
arm and shape, and for every shape the ratio of the new loss's median to each other arm's.  `gate_b256` is the one
performance condition: at B = 256 the new loss takes no longer than `InfoNCELoss` within a 10 % margin, by median of
>= 200 alternated calls.  The larger shapes are recorded, not gated.

    python tools/softmax_contrast_bench.py --out profiles/softmax_contrast_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'crossmodal-imu-video-ood-har_amd'))

from cmhar.losses import InfoNCELoss, SoftmaxContrastiveLoss  # noqa: E402


class Composite(torch.nn.Module):
    """(CE(S, arange) + CE(Sᵀ, arange)) / 2 with S = a·bᵀ/0.07, in torch ops."""

    def forward(self, a, b):
        S = a @ b.T * (1 / 0.07)
        y = torch.arange(a.shape[0], device=a.device)
        return (F.cross_entropy(S, y) + F.cross_entropy(S.T, y)) / 2


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def rounds_for(B, rounds):
    return rounds if B <= 1024 else max(5, rounds // (10 if B <= 4096 else 40))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--d', type=int, default=256)
    ap.add_argument('--batches', type=int, nargs='+', default=[32, 256, 1024, 4096, 16384])
    ap.add_argument('--rounds', type=int, default=200, help='timed calls per arm at B <= 1024 (fewer above)')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'softmax_contrast_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('softmax_contrast_bench needs the GPU (there is no CPU path to time)')
    dev = 'cuda'
    res = {'d': a.d, 'device': torch.cuda.get_device_name(0), 'warmup_rounds': a.warmup,
           'timing': 'device events around loss(a, b) + backward(), arms alternated per round', 'shapes': {}}
    for B in a.batches:
        g = torch.Generator(device=dev).manual_seed(B)
        x = F.normalize(torch.randn(B, a.d, device=dev, generator=g), dim=1).requires_grad_(True)
        y = F.normalize(torch.randn(B, a.d, device=dev, generator=g), dim=1).requires_grad_(True)
        arms = {'softmax_contrastive': SoftmaxContrastiveLoss(learnable=False, group=False).to(dev),
                'infonce': InfoNCELoss(0.07), 'torch_composite': Composite()}

        def call(lf):
            x.grad = y.grad = None
            loss = lf(x, y)
            loss.backward()
            return loss

        n = rounds_for(B, a.rounds)
        warm = a.warmup if B <= 1024 else 2
        times = {k: [] for k in arms}
        last = {}
        for r in range(warm + n):
            for k, lf in arms.items():                      # alternated: one call of each per round
                ms, out = timed(lambda lf=lf: call(lf))
                if r >= warm:
                    times[k].append(ms)
                last[k] = out
        sh = {'rounds': n, 'arms': {}}
        for k, ts in times.items():
            sh['arms'][k] = {'ms_median': round(statistics.median(ts), 4), 'ms_min': round(min(ts), 4),
                             'ms_max': round(max(ts), 4)}
        new = sh['arms']['softmax_contrastive']['ms_median']
        for k in arms:
            if k != 'softmax_contrastive':
                sh[f'new_over_{k}'] = round(new / sh['arms'][k]['ms_median'], 3)
        sh['loss_abs_diff_vs_composite'] = abs(last['softmax_contrastive'].item() - last['torch_composite'].item())
        res['shapes'][str(B)] = sh
        del arms, last
        torch.cuda.empty_cache()
    if '256' in res['shapes']:
        s = res['shapes']['256']
        res['gate_b256'] = {'new_over_infonce': s['new_over_infonce'], 'margin': 1.10, 'rounds': s['rounds'],
                            'pass': s['rounds'] >= 200 and s['new_over_infonce'] <= 1.10}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
