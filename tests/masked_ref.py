"""Plain-torch fp32 restatement of `transformers.VideoMAEModel.forward(pixel_values, bool_masked_pos)`
(modeling_videomae.py:109-122, 398-466): Conv3d patch embedding + sin-cos position table → the kept tokens gathered in
ascending order → pre-LN encoder layers → optional final LayerNorm.  Pinned to the third-party implementation by
tests/golden/g10_videomae_masked.npz (tests/test_video_mask_cpu.py); the GPU tests use it where no fixture exists.

Also the shared geometry / weight / input helpers of the masked-token tests.
"""
from __future__ import annotations

import json
import types

import torch
import torch.nn.functional as F

from oracle.cpu_model import sinusoid_table
from seeded import seeded_input, seeded_state_dict

# geometry A of g10 (Lt = 4 · 4 · 4 = 64) and geometry B of the attention launch-arm cases (Lt = 8 · 6 · 6 = 288):
# hidden 128, 2 layers, 2 heads of 64, intermediate 256, patch 8, tubelet 2
GEOM_A = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, image_size=32,
              patch_size=8, num_frames=8, tubelet_size=2)
GEOM_B = dict(GEOM_A, image_size=48, num_frames=16)
WEIGHT_SEED, VIDEO_SEED, COTANGENT_SEED = 10, 101, 5


def num_tokens(geom):
    return (geom['num_frames'] // geom['tubelet_size']) * (geom['image_size'] // geom['patch_size']) ** 2


def video_for(geom, B, seed=VIDEO_SEED):
    return seeded_input(seed, (B, geom['num_frames'], 3, geom['image_size'], geom['image_size']))


def keep_indices(B, Lt, Lkeep, seed):
    """Seeded kept-token lists, int64 [B, Lkeep], ascending; clip 0 keeps token 0 and token Lt - 1 when Lkeep >= 2
    (Lkeep = 1: token 0 for clip 0, token Lt - 1 for the last clip)."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for b in range(B):
        perm = torch.randperm(Lt, generator=g)
        if b == 0:
            ends = [0, Lt - 1][:Lkeep]
            perm = torch.cat([torch.tensor(ends), perm[~torch.isin(perm, torch.tensor(ends))]])
        elif b == B - 1 and Lkeep == 1:
            perm = torch.tensor([Lt - 1])
        rows.append(perm[:Lkeep].sort().values)
    return torch.stack(rows)


def mask_of(keep, Lt):
    """bool_masked_pos [B, Lt] (True = dropped) of kept-token lists."""
    m = torch.ones(keep.shape[0], Lt, dtype=torch.bool)
    m.scatter_(1, keep.long(), False)
    return m


def backbone_state_dict(geom, use_mean_pooling, seed=WEIGHT_SEED):
    """Seeded state dict of the VideoMAE backbone at `geom` (keys and shapes from the package's own module tree, which
    tests/test_api_cpu.py pins to the third-party one)."""
    from cmhar.videomae import VideoMAEBackbone, default_videomae_config
    cfg = default_videomae_config(use_mean_pooling=use_mean_pooling, **geom)
    tmpl = VideoMAEBackbone(cfg, 'fp32').state_dict()
    return seeded_state_dict(tmpl, seed)


def masked_videomae(sd, video, keep, *, num_heads, patch_size, tubelet, eps=1e-12, use_mean_pooling=True,
                    prefix=''):
    """last_hidden_state [B, Lkeep, Hd] over the kept tokens `keep` (integer [B, Lkeep], ascending), fp32."""
    w = sd[prefix + 'embeddings.patch_embeddings.projection.weight']
    hd = w.shape[0]
    x = video.permute(0, 2, 1, 3, 4)                                        # (B, C, T, H, W)
    emb = F.conv3d(x, w, sd[prefix + 'embeddings.patch_embeddings.projection.bias'],
                   stride=(tubelet, patch_size, patch_size))
    emb = emb.flatten(2).transpose(1, 2)                                    # (B, Lt, Hd)
    h = emb + sinusoid_table(emb.shape[1], hd)[None]
    h = torch.gather(h, 1, keep.long()[:, :, None].expand(-1, -1, hd))     # embeddings[~mask].reshape(B, -1, C)
    B, L, _ = h.shape
    dh = hd // num_heads
    i = 0
    while f'{prefix}encoder.layer.{i}.layernorm_before.weight' in sd:
        p = f'{prefix}encoder.layer.{i}.'
        n = F.layer_norm(h, (hd,), sd[p + 'layernorm_before.weight'], sd[p + 'layernorm_before.bias'], eps)

        def proj(name):
            return F.linear(n, sd[p + f'attention.attention.{name}.weight'],
                            sd.get(p + f'attention.attention.{name}.bias')).reshape(B, L, num_heads, dh).transpose(1, 2)
        q, k, v = proj('query'), proj('key'), proj('value')
        att = torch.softmax((q @ k.transpose(-1, -2)) * dh ** -0.5, dim=-1)
        o = (att @ v).transpose(1, 2).reshape(B, L, hd)
        h = h + F.linear(o, sd[p + 'attention.output.dense.weight'], sd[p + 'attention.output.dense.bias'])
        n2 = F.layer_norm(h, (hd,), sd[p + 'layernorm_after.weight'], sd[p + 'layernorm_after.bias'], eps)
        a = F.gelu(F.linear(n2, sd[p + 'intermediate.dense.weight'], sd[p + 'intermediate.dense.bias']))
        h = h + F.linear(a, sd[p + 'output.dense.weight'], sd[p + 'output.dense.bias'])
        i += 1
    if not use_mean_pooling:
        h = F.layer_norm(h, (hd,), sd[prefix + 'layernorm.weight'], sd[prefix + 'layernorm.bias'], eps)
    return h


def run_ref(geom, use_mean_pooling, video, keep, *, sd=None, grads=True, readout=None):
    """masked_videomae at `geom` on the seeded weights.  Returns types.SimpleNamespace(out, grads, sd): `out` the
    detached last_hidden_state, or with readout=(weight, bias) the projected first kept token; `grads` {key: gradient
    of sum(out · seeded_input(COTANGENT_SEED, out.shape))} for every parameter the output depends on."""
    sd = backbone_state_dict(geom, use_mean_pooling) if sd is None else sd
    leaf = {k: v.clone().requires_grad_(grads) for k, v in sd.items() if v.is_floating_point()}
    h = masked_videomae(leaf, video, keep, num_heads=geom['num_attention_heads'], patch_size=geom['patch_size'],
                        tubelet=geom['tubelet_size'], use_mean_pooling=use_mean_pooling)
    extra = {}
    if readout is not None:
        extra = {'projection.weight': readout[0].clone().requires_grad_(grads),
                 'projection.bias': readout[1].clone().requires_grad_(grads)}
        h = F.linear(h[:, 0], extra['projection.weight'], extra['projection.bias'])
    g = {}
    if grads:
        (h * seeded_input(COTANGENT_SEED, tuple(h.shape))).sum().backward()
        g = {k: v.grad for k, v in {**leaf, **extra}.items() if v.grad is not None}
    return types.SimpleNamespace(out=h.detach(), grads=g, sd=sd)


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


G10_CASES = [(pool, n) for pool in (True, False) for n in (24, 40)]


def g10_case(fx, pool, n):
    """One case of g10_videomae_masked.npz: (keep int64 [B, n], last_hidden_state, {key: ('full', grad) |
    ('sample', norm, sum, every sample_stride-th element)})."""
    tag = f'pool{int(pool)}.keep{n}.'
    grads = {}
    for k in json.loads(str(fx[f'pool{int(pool)}.keys'])):
        if tag + 'grad.' + k in fx:
            grads[k] = ('full', torch.from_numpy(fx[tag + 'grad.' + k]).clone())
        elif tag + 'gnorm.' + k in fx:
            grads[k] = ('sample', float(fx[tag + 'gnorm.' + k]), float(fx[tag + 'gsum.' + k]),
                        torch.from_numpy(fx[tag + 'gsample.' + k]).clone())
    return (torch.from_numpy(fx[tag + 'keep_idx']).long(), torch.from_numpy(fx[tag + 'last_hidden_state']).clone(),
            grads)


def g10_grad_errors(fx, got, grads):
    """Norm-relative error of every gradient in `got` {key: tensor} against a g10 record, skipping the
    mathematically-zero ones (reference magnitude below 1e-5 of the largest: the key biases), as
    tests/test_geometries_gpu.py does.  Weight matrices are recorded as norm + sum + a strided sample: the larger of
    the sample's norm-relative error and the norm's relative error counts."""
    stride = int(fx['sample_stride'])
    gscale = max(float((g[1] if g[0] == 'full' else g[3]).abs().max()) for g in grads.values())
    errs = {}
    for k, rec in grads.items():
        ref = rec[1] if rec[0] == 'full' else rec[3]
        if float(ref.abs().max()) < 1e-5 * gscale:
            continue
        assert got.get(k) is not None, f'no gradient for {k}'
        g = got[k].detach().float().cpu()
        if rec[0] == 'full':
            errs[k] = rel(g, ref)
        else:
            errs[k] = max(rel(g.reshape(-1)[::stride], ref), abs(g.double().norm().item() - rec[1]) / rec[1])
    assert len(errs) >= 20
    return errs


def worst_grad_error(got, ref):
    """Largest norm-relative gradient error over the parameters of `ref`, skipping those whose reference magnitude is
    below 1e-5 of the largest (mathematically zero, e.g. the key biases: noise only), as tests/test_geometries_gpu.py
    does.  got: {key: gradient or None}."""
    gscale = max(float(g.abs().max()) for g in ref.values())
    worst = {}
    for k, g in ref.items():
        if float(g.abs().max()) < 1e-5 * gscale:
            continue
        assert got.get(k) is not None, f'no gradient for {k}'
        worst[k] = rel(got[k], g)
    assert worst
    return max(worst.values()), sorted(worst.items(), key=lambda kv: -kv[1])[:4]
