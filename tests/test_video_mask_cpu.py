"""Masked-token VideoMAE encoding, the parts that need no GPU: the mask generator, the plain-torch restatement
(tests/masked_ref.py) against the third-party numbers of g10_videomae_masked.npz (and live against transformers where
it is installed), the argument errors raised before any device work, and the config surface."""
import json

import pytest
import torch

import masked_ref as R
from fixtures import load


# ------------------------------------------------------------------------------------------------------------
# tube_keep_indices
# ------------------------------------------------------------------------------------------------------------
def _expected_count(ratio, n, rep, multiple):
    k = max(1, round((1.0 - ratio) * n))
    while (k * rep) % multiple:
        k += 1
    return k


@pytest.mark.parametrize('mode', ['tube', 'random'])
@pytest.mark.parametrize('ratio', [0.0, 0.3, 0.5, 0.75, 0.9, 0.999])
@pytest.mark.parametrize('multiple', [1, 8])
@pytest.mark.parametrize('keep_first', [True, False])
def test_tube_keep_indices_properties(mode, ratio, multiple, keep_first):
    from cmhar.videomae import tube_keep_indices
    B, Tp, Hp, Wp = 5, 4, 4, 6                                        # 96 tokens: ratio 0 is a multiple of 8 too
    g = torch.Generator().manual_seed(3)
    idx = tube_keep_indices(B, Tp, Hp, Wp, ratio, device='cpu', mode=mode, keep_first=keep_first, multiple=multiple,
                            generator=g)
    n, rep = (Hp * Wp, Tp) if mode == 'tube' else (Tp * Hp * Wp, 1)
    assert idx.dtype == torch.int32 and idx.is_contiguous()
    assert tuple(idx.shape) == (B, _expected_count(ratio, n, rep, multiple) * rep)
    assert idx.shape[1] % multiple == 0
    assert int(idx.min()) >= 0 and int(idx.max()) < Tp * Hp * Wp
    assert bool((idx[:, 1:] > idx[:, :-1]).all())                     # ascending, hence unique
    if keep_first:
        assert bool((idx[:, 0] == 0).all())
    if mode == 'tube':
        per_t = idx.view(B, Tp, -1)
        assert torch.equal(per_t // (Hp * Wp), torch.arange(Tp, dtype=torch.int32).view(1, Tp, 1).expand_as(per_t))
        assert torch.equal(per_t % (Hp * Wp), (per_t[:, :1] % (Hp * Wp)).expand_as(per_t))   # same set at every t'
    if ratio == 0.0:
        assert torch.equal(idx, torch.arange(Tp * Hp * Wp, dtype=torch.int32).expand(B, -1))


def test_tube_keep_indices_rounding_examples():
    from cmhar.videomae import tube_keep_indices
    # VideoMAE-B: 8 x 14 x 14 tokens; the kept counts the issue's FLOP ratios assume
    assert tube_keep_indices(2, 8, 14, 14, 0.5, device='cpu').shape[1] == 784
    assert tube_keep_indices(2, 8, 14, 14, 0.75, device='cpu').shape[1] == 392
    assert tube_keep_indices(2, 8, 14, 14, 0.9, device='cpu', multiple=8).shape[1] == 160
    # 3 x 3 spatial, 1 time step: round(0.45 * 9) = 4 → rounded up to the next multiple of 8 = 8
    assert tube_keep_indices(2, 1, 3, 3, 0.55, device='cpu', multiple=8).shape[1] == 8
    assert tube_keep_indices(2, 1, 3, 3, 0.999, device='cpu').shape[1] == 1              # max(1, round(0.009))


def test_tube_keep_indices_reproducible_and_varied():
    from cmhar.videomae import tube_keep_indices
    a = tube_keep_indices(4, 4, 6, 6, 0.5, device='cpu', generator=torch.Generator().manual_seed(11))
    b = tube_keep_indices(4, 4, 6, 6, 0.5, device='cpu', generator=torch.Generator().manual_seed(11))
    c = tube_keep_indices(4, 4, 6, 6, 0.5, device='cpu', generator=torch.Generator().manual_seed(12))
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert not torch.equal(a[0], a[1])                                 # clips draw their own sets
    torch.manual_seed(5)
    d = tube_keep_indices(4, 4, 6, 6, 0.5, device='cpu')
    torch.manual_seed(5)
    assert torch.equal(d, tube_keep_indices(4, 4, 6, 6, 0.5, device='cpu'))      # the global RNG


@pytest.mark.parametrize('kw', [dict(mask_ratio=1.0), dict(mask_ratio=-0.1), dict(mask_ratio=1.5),
                                dict(mask_ratio=0.5, mode='block'), dict(mask_ratio=0.5, multiple=0),
                                dict(mask_ratio=0.5, multiple=8, Tp=1, Hp=1, Wp=7),      # no multiple of 8 <= 7
                                dict(mask_ratio=0.5, Tp=0)])
def test_tube_keep_indices_value_errors(kw):
    from cmhar.videomae import tube_keep_indices
    args = dict(B=2, Tp=4, Hp=3, Wp=3, mask_ratio=0.5, device='cpu')
    args.update(kw)
    with pytest.raises(ValueError):
        tube_keep_indices(**args)


# ------------------------------------------------------------------------------------------------------------
# masked_ref against the third-party implementation
# ------------------------------------------------------------------------------------------------------------
G10_CASES = R.G10_CASES
g10_case, g10_grad_errors = R.g10_case, R.g10_grad_errors


def test_g10_fixture_records_what_the_tests_regenerate():
    fx = load('g10_videomae_masked')
    assert json.loads(str(fx['config'])) == R.GEOM_A
    assert (int(fx['seed']), int(fx['video_seed']), int(fx['cotangent_seed'])) == \
        (R.WEIGHT_SEED, R.VIDEO_SEED, R.COTANGENT_SEED)
    for pool, n in G10_CASES:
        keep, hs, grads = g10_case(fx, pool, n)
        assert torch.equal(keep, R.keep_indices(int(fx['B']), R.num_tokens(R.GEOM_A), n, int(fx['keep_seed']) + n))
        assert tuple(hs.shape) == (3, n, 128)
        assert int(keep.min()) == 0 and int(keep.max()) == 63          # token 0 and token Lt - 1 are in the sets
        sd = R.backbone_state_dict(R.GEOM_A, pool)
        assert list(sd.keys()) == json.loads(str(fx[f'pool{int(pool)}.keys']))
        assert [list(v.shape) for v in sd.values()] == json.loads(str(fx[f'pool{int(pool)}.shapes']))


@pytest.mark.parametrize('pool,n', G10_CASES)
def test_masked_ref_matches_g10(pool, n):
    fx = load('g10_videomae_masked')
    keep, hs, grads = g10_case(fx, pool, n)
    r = R.run_ref(R.GEOM_A, pool, R.video_for(R.GEOM_A, int(fx['B'])), keep)
    e = R.rel(r.out, hs)
    errs = g10_grad_errors(fx, r.grads, grads)
    print(f'masked_ref vs g10 pool={pool} keep={n}: out {e:.2e}  worst grad {max(errs.values()):.2e}')
    assert e <= 1e-5
    assert max(errs.values()) <= 1e-4, sorted(errs.items(), key=lambda kv: -kv[1])[:4]


@pytest.mark.parametrize('pool,n', G10_CASES)
def test_masked_ref_matches_transformers_live(pool, n):
    pytest.importorskip('transformers')
    import make_golden_masked as G
    geom = R.GEOM_A
    video = R.video_for(geom, 3)
    keep = R.keep_indices(3, R.num_tokens(geom), n, 2000 + n)
    hs, hf_grads, sd = G.hf_run(geom, pool, video, keep)
    r = R.run_ref(geom, pool, video, keep, sd=sd)
    e = R.rel(r.out, hs)
    worst, top = R.worst_grad_error(r.grads, hf_grads)
    print(f'masked_ref vs transformers pool={pool} keep={n}: out {e:.2e}  worst grad {worst:.2e}')
    assert e <= 1e-5
    assert worst <= 1e-4, top


# ------------------------------------------------------------------------------------------------------------
# argument errors before any device work; config surface
# ------------------------------------------------------------------------------------------------------------
def _backbone_a():
    from cmhar.videomae import VideoMAEBackbone, default_videomae_config
    return VideoMAEBackbone(default_videomae_config(**R.GEOM_A), 'fp32')


def test_backbone_mask_errors_are_value_errors_on_cpu():
    m = _backbone_a()
    video = R.video_for(R.GEOM_A, 3)
    Lt = R.num_tokens(R.GEOM_A)
    good = R.mask_of(R.keep_indices(3, Lt, 24, 1), Lt)
    with pytest.raises(ValueError, match='shape'):
        m(video, bool_masked_pos=good[:, :-1])
    with pytest.raises(ValueError, match='shape'):
        m(video, bool_masked_pos=good[:2])
    with pytest.raises(ValueError, match='bool'):
        m(video, bool_masked_pos=good.to(torch.uint8))
    uneven = good.clone()
    uneven[1, int(torch.nonzero(~good[1])[0])] = True                  # clip 1 keeps one token fewer
    with pytest.raises(ValueError, match='same number'):
        m(video, bool_masked_pos=uneven)
    with pytest.raises(ValueError, match='every token'):
        m(video, bool_masked_pos=torch.ones(3, Lt, dtype=torch.bool))
    none_kept_in_one = good.clone()
    none_kept_in_one[2] = True
    with pytest.raises(ValueError):
        m(video, bool_masked_pos=none_kept_in_one)


def test_mask_to_keep_indices_is_ascending_kept_tokens():
    from cmhar.videomae import mask_to_keep_indices
    keep = R.keep_indices(4, 64, 24, 9)
    out = mask_to_keep_indices(R.mask_of(keep, 64), 4, 64)
    assert out.dtype == torch.int32 and torch.equal(out.long(), keep)
    assert torch.equal(mask_to_keep_indices(torch.zeros(2, 64, dtype=torch.bool), 2, 64),
                       torch.arange(64, dtype=torch.int32).expand(2, -1))


def test_model_config_mask_defaults():
    from cmhar.config import Config, ModelConfig
    assert ModelConfig().video_mask_ratio == 0.0 and ModelConfig().video_mask_mode == 'tube'
    c = Config()
    assert c.model.video_mask_ratio == 0.0 and c.model.video_mask_mode == 'tube'


def _tiny_cfg(backbone, ratio, mode='tube'):
    from cmhar.config import Config
    cfg = Config()
    cfg.data.video_frames_per_window = 8
    cfg.data.video_resize = (32, 32)
    m = cfg.model
    m.video_backbone, m.video_pretrained = backbone, False
    m.videomae_hidden_size, m.videomae_num_layers, m.videomae_num_heads = 128, 2, 2
    m.videomae_intermediate_size, m.videomae_patch_size = 256, 8
    m.video_d_model = 64
    m.video_mask_ratio, m.video_mask_mode = ratio, mode
    return cfg


def test_video_encoder_mask_config_checks():
    from cmhar.models import VideoEncoder
    with pytest.raises(ValueError, match='video_mask_ratio'):
        VideoEncoder(_tiny_cfg('r3d_18', 0.5))
    with pytest.raises(ValueError, match='video_mask_ratio'):
        VideoEncoder(_tiny_cfg('/nonexistent/videomae-mask', 1.0))
    with pytest.raises(ValueError, match='video_mask_mode'):
        VideoEncoder(_tiny_cfg('/nonexistent/videomae-mask', 0.5, mode='block'))
    enc = VideoEncoder(_tiny_cfg('/nonexistent/videomae-mask', 0.5))
    ref = VideoEncoder(_tiny_cfg('/nonexistent/videomae-mask', 0.0))
    assert list(enc.state_dict().keys()) == list(ref.state_dict().keys())
    VideoEncoder(_tiny_cfg('r3d_18', 0.0))                              # ratio 0 on another backbone stays valid


def test_video_encoder_draws_the_documented_indices():
    """The indices a training-mode call encodes are those tube_keep_indices draws from the global RNG with
    keep_first=True and multiple 8 for bf16 / 1 for fp32; eval and ratio 0 draw none."""
    from cmhar.models import VideoEncoder
    from cmhar.videomae import tube_keep_indices
    x = torch.zeros(3, 8, 3, 32, 32)
    for dtype, multiple in (('fp32', 1), ('bf16', 8)):
        cfg = _tiny_cfg('/nonexistent/videomae-mask', 0.6)
        cfg.model.compute_dtype = dtype
        enc = VideoEncoder(cfg).train()
        torch.manual_seed(21)
        got = enc._keep_indices(x, None)
        torch.manual_seed(21)
        want = tube_keep_indices(3, 4, 4, 4, 0.6, device='cpu', mode='tube', keep_first=True, multiple=multiple)
        assert torch.equal(got, want) and got.shape[1] % multiple == 0
        assert enc.eval()._keep_indices(x, None) is None
        explicit = R.mask_of(R.keep_indices(3, 64, 5, 4), 64)
        assert torch.equal(enc._keep_indices(x, explicit).long(), R.keep_indices(3, 64, 5, 4))
    assert VideoEncoder(_tiny_cfg('/nonexistent/videomae-mask', 0.0)).train()._keep_indices(x, None) is None
