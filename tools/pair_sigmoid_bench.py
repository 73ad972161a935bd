#!/usr/bin/env python3
"""Times forward + backward of `cmhar.losses.PairwiseSigmoidLoss` through the module, D = 256, B in {32, 256, 1024,
4096, 16384}, against two other arms:

* `SigmoidContrastiveLoss` (the reference-parity loss on `cmhar_siglip_loss`), where it accepts the shape (B <= 1024);
* a torch composite of the same pairwise-sigmoid formula under autograd (it stores the B x B matrices).

One call = loss(a, b) and loss.backward() with the embeddings and the loss's temperature / bias requiring gradients.
The arms are run alternately, round after round, each call timed with device events after warm-up rounds; the JSON
carries the median, minimum and maximum per arm and shape, and for every shape the ratio of the new loss's median to
each other arm's.  `gate_b256` is the one performance condition: at B = 256 the new loss takes no longer than
`SigmoidContrastiveLoss` within a 10 % margin, by median of >= 200 alternated calls.

    python tools/pair_sigmoid_bench.py --out profiles/pair_sigmoid_bench.json
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

from cmhar.losses import PairwiseSigmoidLoss, SigmoidContrastiveLoss  # noqa: E402


class Composite(torch.nn.Module):
    """Σ_ij softplus(−z_ij·S_ij) / B in torch ops (z = 2I − 1)."""

    def __init__(self):
        super().__init__()
        self.temperature = torch.nn.Parameter(torch.tensor(10.0).log())
        self.bias = torch.nn.Parameter(torch.tensor(-10.0))

    def forward(self, a, b):
        S = a @ b.T * self.temperature.exp() + self.bias
        z = 2 * torch.eye(a.shape[0], device=a.device) - 1
        return F.softplus(-z * S).sum() / a.shape[0]


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
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'pair_sigmoid_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('pair_sigmoid_bench needs the GPU (there is no CPU path to time)')
    dev = 'cuda'
    res = {'d': a.d, 'device': torch.cuda.get_device_name(0), 'warmup_rounds': a.warmup,
           'timing': 'device events around loss(a, b) + backward(), arms alternated per round', 'shapes': {}}
    for B in a.batches:
        g = torch.Generator(device=dev).manual_seed(B)
        x = F.normalize(torch.randn(B, a.d, device=dev, generator=g), dim=1).requires_grad_(True)
        y = F.normalize(torch.randn(B, a.d, device=dev, generator=g), dim=1).requires_grad_(True)
        arms = {'pairwise_sigmoid': PairwiseSigmoidLoss(group=False).to(dev), 'torch_composite': Composite().to(dev)}
        if B <= 1024:
            arms['sigmoid_contrastive'] = SigmoidContrastiveLoss(group=False).to(dev)

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
        new = sh['arms']['pairwise_sigmoid']['ms_median']
        for k in arms:
            if k != 'pairwise_sigmoid':
                sh[f'new_over_{k}'] = round(new / sh['arms'][k]['ms_median'], 3)
        sh['loss_abs_diff_vs_composite'] = abs(last['pairwise_sigmoid'].item() - last['torch_composite'].item())
        res['shapes'][str(B)] = sh
        del arms, last
        torch.cuda.empty_cache()
    if '256' in res['shapes'] and 'new_over_sigmoid_contrastive' in res['shapes']['256']:
        s = res['shapes']['256']
        res['gate_b256'] = {'new_over_sigmoid_contrastive': s['new_over_sigmoid_contrastive'], 'margin': 1.10,
                            'rounds': s['rounds'], 'pass': s['new_over_sigmoid_contrastive'] <= 1.10}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
