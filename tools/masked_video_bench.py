#!/usr/bin/env python3
"""Times `CrossModalTrainer.train_step` with masked-token video encoding (`model.video_mask_ratio`): bf16, B = 32,
VideoMAE-B over 16x224^2 clips + IMU 6x200, `video_mask_ratio` in {0, 0.5, 0.75, 0.9} (tube masks, token 0 kept).

ONE model and trainer serve every ratio (the encoder reads its ratio at each call), so the arms differ in nothing but
the number of tokens encoded.  The ratios are run alternately, round after round, each step timed with device events
after warm-up rounds; ratio 0 is the same-run baseline.  The JSON carries the median / minimum / maximum per ratio,
the ratio of each median to ratio 0's, and beside it the backbone FLOP ratio the geometry gives (per layer and clip
2·L·7.08M GEMM FLOPs + 4·L²·768 attention FLOPs at L kept tokens) — the time ratio a step made of nothing but backbone
FLOPs at a constant rate would show.  No speed-up is asserted.

After the timing, one further step per ratio runs with every GEMM / attention launch bracketed by events (the library's
launch tracer, weight gradients on the main stream): `kernels_ms` lists the traced time per kernel family and
`vs_ratio0` its ratio to the unmasked step's, which names the kernels that shrink less than their FLOPs.

    python tools/masked_video_bench.py --out profiles/masked_video_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'crossmodal-imu-video-ood-har_amd'))

from cmhar import kernels as K  # noqa: E402
from cmhar.config import Config  # noqa: E402
from cmhar.losses import SigmoidContrastiveLoss  # noqa: E402
from cmhar.models import CrossModalModel  # noqa: E402
from cmhar.trainer import CrossModalTrainer  # noqa: E402
from cmhar.videomae import tube_keep_indices  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def backbone_flop_ratio(L, L0, hidden=768, inter=3072):
    """Backbone FLOPs at L kept tokens over those at L0 (per layer: the four GEMMs are linear in L, attention
    quadratic)."""
    def f(n):
        return 2 * n * (3 * hidden * hidden + hidden * hidden + 2 * hidden * inter) + 4 * n * n * hidden
    return f(L) / f(L0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--image', type=int, default=224)
    ap.add_argument('--imu-len', type=int, default=200)
    ap.add_argument('--ratios', type=float, nargs='+', default=[0.0, 0.5, 0.75, 0.9])
    ap.add_argument('--rounds', type=int, default=20, help='timed steps per ratio')
    ap.add_argument('--warmup', type=int, default=5, help='untimed rounds (every ratio once per round)')
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'masked_video_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('masked_video_bench needs the GPU (there is no CPU path to time)')
    if a.ratios[0] != 0.0:
        sys.exit('the first ratio must be 0 (the same-run baseline)')
    dev = 'cuda'
    cfg = Config()
    cfg.data.imu_window_size = a.imu_len
    cfg.data.video_frames_per_window = a.frames
    cfg.data.video_resize = (a.image, a.image)
    cfg.model.compute_dtype = 'bf16'
    cfg.model.allow_random_init = True
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = CrossModalModel(cfg)
    tr = CrossModalTrainer(model, SigmoidContrastiveLoss().to(dev), cfg, device=dev)
    model.train()
    enc = model.video_encoder
    bcfg = enc.backbone.config
    Tp, Hp = a.frames // bcfg.tubelet_size, a.image // bcfg.patch_size
    L0 = Tp * Hp * Hp
    g = torch.Generator(device=dev).manual_seed(1)
    video = torch.randn(a.batch, a.frames, 3, a.image, a.image, device=dev, generator=g)
    imu = torch.randn(a.batch, 6, a.imu_len, device=dev, generator=g)

    def step(ratio):
        enc.video_mask_ratio = ratio
        return tr.train_step(imu, video)

    times = {r: [] for r in a.ratios}
    for i in range(a.warmup + a.rounds):
        for r in a.ratios:                                  # alternated: one step of each ratio per round
            ms, loss = timed(lambda r=r: step(r))
            if i >= a.warmup:
                times[r].append(ms)
    res = {'device': torch.cuda.get_device_name(0), 'batch': a.batch, 'clip': [a.frames, 3, a.image, a.image],
           'imu': [6, a.imu_len], 'dtype': 'bf16', 'tokens_unmasked': L0, 'warmup_rounds': a.warmup, 'rounds': a.rounds,
           'timing': 'device events around CrossModalTrainer.train_step, ratios alternated per round, one model',
           'ratios': {}}
    base = statistics.median(times[0.0])
    for r in a.ratios:
        L = L0 if r == 0.0 else tube_keep_indices(1, Tp, Hp, Hp, r, device='cpu', multiple=8).shape[1]
        ts = times[r]
        res['ratios'][str(r)] = {'tokens_kept': L, 'ms_median': round(statistics.median(ts), 3),
                                 'ms_min': round(min(ts), 3), 'ms_max': round(max(ts), 3),
                                 'clips_per_s': round(1000 * a.batch / statistics.median(ts), 1),
                                 'time_over_ratio0': round(statistics.median(ts) / base, 3),
                                 'backbone_flops_over_ratio0': round(backbone_flop_ratio(L, L0), 3)}
    if not a.no_trace:
        enc.backbone.overlap_wgrad = False                  # each traced kernel alone on the chip
        traced = {}
        for r in a.ratios:
            K.TRACE.records, K.TRACE.only, K.TRACE.active = [], None, True
            step(r)
            torch.cuda.synchronize()
            K.TRACE.active = False
            traced[r] = {k: (v[0], v[1]) for k, v in K.TRACE.summary().items()}
        del enc.backbone.overlap_wgrad
        K.TRACE.records = []
        def family(label):
            return 'attention_fwd' if label.startswith('attn_fwd') else \
                'attention_bwd' if label.startswith('attn_bwd') else 'gemm'

        for r in a.ratios:
            fam = {}
            for k, (n, ms) in traced[r].items():
                fam[family(k)] = fam.get(family(k), 0.0) + ms
            fam0 = {}
            for k, (n, ms) in traced[0.0].items():
                fam0[family(k)] = fam0.get(family(k), 0.0) + ms
            res['ratios'][str(r)]['families_ms'] = {
                k: {'ms': round(v, 3), 'vs_ratio0': round(v / fam0[k], 3)} for k, v in fam.items() if k in fam0}
            rows = {}
            for k, (n, ms) in sorted(traced[r].items(), key=lambda kv: -kv[1][1]):
                rows[k] = {'launches': n, 'ms': round(ms, 3)}
                if r != 0.0 and k in traced[0.0]:
                    rows[k]['vs_ratio0'] = round(ms / traced[0.0][k][1], 3)
            res['ratios'][str(r)]['kernels_ms'] = rows
            res['ratios'][str(r)]['traced_ms_total'] = round(sum(ms for _, ms in traced[r].values()), 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
