"""Generate tests/golden/g10_videomae_masked.npz from the installed third-party `transformers.VideoMAEModel`
(run by hand, from any directory; needs transformers, not a GPU):

    python tests/golden/make_golden_masked.py

`VideoMAEModel.forward(pixel_values, bool_masked_pos)` at geometry A of tests/masked_ref.py (hidden 128, 2 layers,
2 heads, intermediate 256, image 32, patch 8, 8 frames: Lt = 64), B = 3, kept counts 24 and 40, both
`use_mean_pooling` values.  Weights and inputs are regenerated from seeds (tests/golden/seeded.py), so the fixture
stores only: the geometry, the key list and shapes, the seeds, the kept indices, `last_hidden_state`, and the gradients
of sum(last_hidden_state · seeded_input(5, shape)).  Four gradient sets of the whole backbone in full would be 4.9 MB,
so only the parameters of at most FULL_LIMIT elements (biases, LayerNorms) are stored in full; the weight matrices are
stored as norm, sum and every SAMPLE_STRIDE-th element.
"""
from __future__ import annotations

import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(REPO, 'tests'), REPO, os.path.join(REPO, 'crossmodal-imu-video-ood-har_amd')):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from transformers import VideoMAEConfig, VideoMAEModel  # noqa: E402

import masked_ref as R  # noqa: E402
from seeded import seeded_input, seeded_state_dict  # noqa: E402

FULL_LIMIT, SAMPLE_STRIDE = 2048, 11
B, KEPT = 3, (24, 40)
KEEP_SEED = 1000          # the kept lists of count n come from masked_ref.keep_indices(B, Lt, n, KEEP_SEED + n)


def hf_model(geom, use_mean_pooling, seed=R.WEIGHT_SEED):
    m = VideoMAEModel(VideoMAEConfig(use_mean_pooling=use_mean_pooling, **geom))
    sd = seeded_state_dict({k: v for k, v in m.state_dict().items()}, seed)
    m.load_state_dict(sd, strict=True)
    return m.train(), sd


def hf_run(geom, use_mean_pooling, video, keep):
    """(last_hidden_state, {key: gradient}) of the third-party model on the seeded weights."""
    m, sd = hf_model(geom, use_mean_pooling)
    hs = m(video, bool_masked_pos=R.mask_of(keep, R.num_tokens(geom))).last_hidden_state
    (hs * seeded_input(R.COTANGENT_SEED, tuple(hs.shape))).sum().backward()
    return hs.detach(), {n: p.grad for n, p in m.named_parameters() if p.grad is not None}, sd


def main():
    torch.set_num_threads(8)
    geom = R.GEOM_A
    Lt = R.num_tokens(geom)
    video = R.video_for(geom, B)
    arrays = {}
    for pool in (True, False):
        for n in KEPT:
            keep = R.keep_indices(B, Lt, n, KEEP_SEED + n)
            hs, grads, sd = hf_run(geom, pool, video, keep)
            tag = f'pool{int(pool)}.keep{n}.'
            arrays[tag + 'keep_idx'] = keep.numpy().astype(np.int32)
            arrays[tag + 'last_hidden_state'] = hs.numpy().copy()
            keys = list(sd.keys())
            arrays[f'pool{int(pool)}.keys'] = json.dumps(keys)
            arrays[f'pool{int(pool)}.shapes'] = json.dumps([list(sd[k].shape) for k in keys])
            for k, g in grads.items():
                if g.numel() <= FULL_LIMIT:
                    arrays[tag + 'grad.' + k] = g.numpy().copy()
                else:
                    arrays[tag + 'gnorm.' + k] = np.array(g.double().norm().item())
                    arrays[tag + 'gsum.' + k] = np.array(g.double().sum().item())
                    arrays[tag + 'gsample.' + k] = g.reshape(-1)[::SAMPLE_STRIDE].numpy().copy()
    path = os.path.join(HERE, 'g10_videomae_masked.npz')
    np.savez_compressed(path, config=json.dumps(geom), B=B, kept=np.array(KEPT), seed=R.WEIGHT_SEED,
                        video_seed=R.VIDEO_SEED, cotangent_seed=R.COTANGENT_SEED, keep_seed=KEEP_SEED,
                        sample_stride=SAMPLE_STRIDE, **arrays)
    print(f'wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)')


if __name__ == '__main__':
    main()
