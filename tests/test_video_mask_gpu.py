"""Masked-token VideoMAE encoding on the GPU: the kept-token gather kernels bit for bit, the identity mask bit for bit
against the unmasked path, the masked backbone against the third-party numbers of g10_videomae_masked.npz and the
plain-torch restatement tests/masked_ref.py (pinned to the third-party model by tests/test_video_mask_cpu.py), the
attention launch arms that only masked lengths reach, the VideoEncoder readout, one masked trainer step.

Bounds: fp32 outputs ≤ 1e-4 and gradients ≤ 1e-3 norm-relative, bf16 outputs ≤ 3e-2 (the project's existing bounds,
tests/test_geometries_gpu.py); gradients whose reference magnitude is below 1e-5 of the largest are skipped (the key
biases: mathematically zero)."""
import functools
import warnings

import pytest
import torch

import masked_ref as R
from fixtures import load
from seeded import seeded_input, seeded_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}


def K():
    from cmhar import kernels
    return kernels


# ------------------------------------------------------------------------------------------------------------
# gather kernels: bit-exact
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('Lkeep', [1, 5, 24, 64])
def test_tubelet_im2col_gather_equals_rows_of_im2col(dtype, Lkeep):
    geom, B = R.GEOM_A, 3
    Lt = R.num_tokens(geom)
    video = R.video_for(geom, B).to(DEV)
    keep = R.keep_indices(B, Lt, Lkeep, 300 + Lkeep)
    assert int(keep.min()) == 0 and int(keep.max()) == Lt - 1
    full = K().tubelet_im2col(video, geom['tubelet_size'], geom['patch_size'], DTYPES[dtype])
    got = K().tubelet_im2col_gather(video, geom['tubelet_size'], geom['patch_size'], DTYPES[dtype],
                                    keep.to(DEV, torch.int32))
    rows = (torch.arange(B)[:, None] * Lt + keep).reshape(-1).to(DEV)
    assert got.shape == (B * Lkeep, full.shape[1]) and got.dtype == full.dtype
    assert torch.equal(got, full[rows])


@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
def test_tubelet_im2col_gather_two_groups_per_row(dtype):
    """C = 3, tubelet 2, patch 16 (two 8-wide dx groups per patch row), a non-square frame: Lt = 2 · 2 · 3 = 12."""
    B, T, C, H, W, tub, P = 2, 4, 3, 32, 48, 2, 16
    video = seeded_input(311, (B, T, C, H, W)).to(DEV)
    keep = torch.tensor([[0, 3, 4, 7, 11], [1, 2, 5, 10, 11]])
    full = K().tubelet_im2col(video, tub, P, DTYPES[dtype])
    got = K().tubelet_im2col_gather(video, tub, P, DTYPES[dtype], keep.to(DEV, torch.int32))
    rows = (torch.arange(B)[:, None] * 12 + keep).reshape(-1).to(DEV)
    assert got.shape == (10, C * tub * P * P)
    assert torch.equal(got, full[rows])


@pytest.mark.parametrize('rows,N,view', [(64, 128, False), (64, 128, True), (9, 7, False), (1, 4, False)])
def test_gather_rows_equals_indexing(rows, N, view):
    """16-B rows (the float4 arm), a table that is a column slice of a wider one (its own leading dimension), and an
    odd width (the scalar arm); repeated indices, first and last row."""
    table = seeded_input(320, (rows, N + (8 if view else 0))).to(DEV)
    if view:
        table = table[:, 4:4 + N]
    g = torch.Generator().manual_seed(321)
    idx = torch.cat([torch.tensor([0, rows - 1, rows - 1]), torch.randint(0, rows, (70,), generator=g)])
    idx = idx.reshape(1, -1).to(DEV, torch.int32)
    got = K().gather_rows(table, idx)
    assert got.shape == (73, N) and got.is_contiguous()
    assert torch.equal(got, table[idx.reshape(-1).long()])


def test_gather_wrappers_refuse_what_the_kernel_would():
    video = R.video_for(R.GEOM_A, 2).to(DEV)
    keep = torch.zeros(2, 4, dtype=torch.int32, device=DEV)
    for bad_video, tub, P, bad_keep in [(video.cpu(), 2, 8, keep), (video, 2, 8, keep.cpu()), (video, 2, 8, keep.long()),
                                        (video, 2, 8, keep[:1]), (video, 2, 8, keep[:, :0]), (video, 2, 8, keep.t()),
                                        (video, 3, 8, keep), (video, 2, 12, keep), (video, 2, 4, keep),
                                        (video.double(), 2, 8, keep)]:
        with pytest.raises(ValueError):
            K().tubelet_im2col_gather(bad_video, tub, P, torch.float32, bad_keep)
    table = torch.zeros(8, 16, device=DEV)
    for bad_table, bad_idx in [(table.cpu(), keep), (table, keep.cpu()), (table, keep.long()), (table.half(), keep),
                               (table, keep[:, :0]), (table.t(), keep)]:
        with pytest.raises(ValueError):
            K().gather_rows(bad_table, bad_idx)


# ------------------------------------------------------------------------------------------------------------
# backbone
# ------------------------------------------------------------------------------------------------------------
def _backbone(geom, pool, dtype):
    from cmhar.videomae import VideoMAEBackbone, default_videomae_config
    m = VideoMAEBackbone(default_videomae_config(use_mean_pooling=pool, **geom), dtype)
    m.load_state_dict(R.backbone_state_dict(geom, pool), strict=True)
    return m.to(DEV).train()


def _run(m, video, mask, backward=True):
    """last_hidden_state and {key: gradient of sum(hs · seeded_input(5, hs.shape))} of the GPU backbone."""
    for p in m.parameters():
        p.grad = None
    hs = m(video.to(DEV), bool_masked_pos=None if mask is None else mask.to(DEV)).last_hidden_state
    if not backward:
        return hs.detach(), {}
    (hs * seeded_input(R.COTANGENT_SEED, tuple(hs.shape)).to(DEV)).sum().backward()
    return hs.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_identity_mask_is_the_unmasked_path_bit_for_bit(dtype):
    geom, B = R.GEOM_A, 4
    m = _backbone(geom, True, dtype)
    video = R.video_for(geom, B)
    hs0, g0 = _run(m, video, None)
    hs1, g1 = _run(m, video, torch.zeros(B, R.num_tokens(geom), dtype=torch.bool))
    assert hs1.shape == hs0.shape and torch.equal(hs1, hs0)
    assert g0.keys() == g1.keys() and len(g0) == len(list(m.parameters()))
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k


@pytest.mark.parametrize('pool,n', R.G10_CASES)
def test_masked_backbone_fp32_vs_g10(pool, n):
    fx = load('g10_videomae_masked')
    keep, ref_hs, ref_grads = R.g10_case(fx, pool, n)
    m = _backbone(R.GEOM_A, pool, 'fp32')
    hs, grads = _run(m, R.video_for(R.GEOM_A, int(fx['B'])), R.mask_of(keep, R.num_tokens(R.GEOM_A)))
    e = R.rel(hs, ref_hs)
    errs = R.g10_grad_errors(fx, grads, ref_grads)
    print(f'masked backbone fp32 vs g10 pool={pool} keep={n}: out {e:.2e}  worst grad {max(errs.values()):.2e}')
    assert tuple(hs.shape) == (3, n, 128)
    assert e <= 1e-4
    assert max(errs.values()) <= 1e-3, sorted(errs.items(), key=lambda kv: -kv[1])[:4]


def test_masked_backbone_fp32_one_kept_token():
    """Lkeep = 1 (clip 0 keeps token 0, clip 2 the last token): forward against masked_ref."""
    geom, B = R.GEOM_A, 3
    keep = R.keep_indices(B, R.num_tokens(geom), 1, 301)
    video = R.video_for(geom, B)
    ref = R.run_ref(geom, True, video, keep, grads=False)
    with torch.no_grad():
        hs, _ = _run(_backbone(geom, True, 'fp32'), video, R.mask_of(keep, R.num_tokens(geom)), backward=False)
    e = R.rel(hs, ref.out)
    print(f'masked backbone fp32, one kept token: out {e:.2e}')
    assert tuple(hs.shape) == (B, 1, 128) and e <= 1e-4


@functools.lru_cache(maxsize=None)
def _arm_reference(n):
    geom, B = R.GEOM_B, 2
    keep = R.keep_indices(B, R.num_tokens(geom), n, 400 + n)
    return keep, R.run_ref(geom, True, R.video_for(geom, B), keep)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('n', [136, 200, 264])
def test_masked_lengths_reach_other_attention_arms(dtype, n):
    """Kept counts around the 128- / 256-query blocks and the 64-row tail limit of csrc/attention.hip (production:
    392 = 256 + a 136-row remainder no tail kernel takes; 784 = 3 · 256 + a 16-row tail): 136 = 128 + 8 (tail),
    200 = 128 + 72 (remainder past the tail limit), 264 = 256 + 8 (bulk block + tail)."""
    geom, B = R.GEOM_B, 2
    keep, ref = _arm_reference(n)
    hs, grads = _run(_backbone(geom, True, dtype), R.video_for(geom, B), R.mask_of(keep, R.num_tokens(geom)))
    e = R.rel(hs, ref.out)
    worst, top = R.worst_grad_error(grads, ref.grads)
    print(f'masked backbone {dtype} Lkeep={n}: out {e:.2e}  worst grad {worst:.2e}')
    assert tuple(hs.shape) == (B, n, 128)
    if dtype == 'fp32':
        assert e <= 1e-4
        assert worst <= 1e-3, top
    else:
        assert e <= 3e-2
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())


def test_bf16_training_needs_kept_rows_in_multiples_of_8():
    geom, B = R.GEOM_A, 3
    m = _backbone(geom, True, 'bf16')
    mask = R.mask_of(R.keep_indices(B, R.num_tokens(geom), 5, 305), R.num_tokens(geom)).to(DEV)
    with pytest.raises(ValueError, match='multiple of 8'):
        m(R.video_for(geom, B).to(DEV), bool_masked_pos=mask)
    with torch.no_grad():                                   # forward-only takes any count
        assert m(R.video_for(geom, B).to(DEV), bool_masked_pos=mask).last_hidden_state.shape == (B, 5, 128)


# ------------------------------------------------------------------------------------------------------------
# VideoEncoder / CrossModalModel
# ------------------------------------------------------------------------------------------------------------
def _model_cfg(dtype, ratio):
    from cmhar.config import Config
    cfg = Config()
    cfg.data.imu_window_size = 64
    cfg.data.video_frames_per_window = R.GEOM_A['num_frames']
    cfg.data.video_resize = (R.GEOM_A['image_size'],) * 2
    m = cfg.model
    m.video_backbone, m.video_pretrained = '/nonexistent/videomae-mask', False
    m.imu_d_model, m.imu_nhead, m.imu_num_layers, m.imu_dropout = 32, 4, 2, 0.0
    m.videomae_hidden_size, m.videomae_num_layers = R.GEOM_A['hidden_size'], R.GEOM_A['num_hidden_layers']
    m.videomae_num_heads, m.videomae_intermediate_size = R.GEOM_A['num_attention_heads'], R.GEOM_A['intermediate_size']
    m.videomae_patch_size = R.GEOM_A['patch_size']
    m.video_d_model, m.projection_hidden_dim, m.projection_dim = 64, 64, 32
    m.compute_dtype, m.video_mask_ratio = dtype, ratio
    return cfg


def _encoder(dtype, ratio):
    from cmhar.models import VideoEncoder
    enc = VideoEncoder(_model_cfg(dtype, ratio))
    sd = seeded_state_dict(enc.state_dict(), seed=R.WEIGHT_SEED)
    enc.load_state_dict(sd, strict=True)
    return enc.to(DEV), sd


# bf16 gradient bound: the unit round-off of bf16 is 2^-9 = 2e-3; a gradient of the two-layer backbone passes about 40
# bf16-stored tensors (13 forward and 8 backward per layer), so between 40^0.5 · 2e-3 = 1.2e-2 (independent roundings)
# and 40 · 2e-3 = 8e-2 (all aligned); 6e-2 is the blanket bound the project used for bf16 gradients before the
# storage-emulating oracle (tests/test_models_gpu.py), which has no masked variant.
@pytest.mark.parametrize('dtype,B,out_tol,grad_tol', [('fp32', 3, 1e-4, 1e-3), ('bf16', 8, 3e-2, 6e-2)])
def test_video_encoder_masked_readout(dtype, B, out_tol, grad_tol):
    """Training mode at ratio 0.5: the encoder draws tube_keep_indices from the global RNG (keep_first, multiple 8
    for bf16) and projects the first kept token — token 0.  bf16 at B = 8 takes the token-0 last-layer path."""
    from cmhar.videomae import tube_keep_indices
    enc, sd = _encoder(dtype, 0.5)
    enc.train()
    video = R.video_for(R.GEOM_A, B)
    torch.manual_seed(77)
    keep = tube_keep_indices(B, 4, 4, 4, 0.5, device=DEV, mode='tube', keep_first=True,
                             multiple=8 if dtype == 'bf16' else 1)
    assert tuple(keep.shape) == (B, 32) and bool((keep[:, 0] == 0).all())
    torch.manual_seed(77)
    feat = enc(video.to(DEV))
    (feat * seeded_input(R.COTANGENT_SEED, tuple(feat.shape)).to(DEV)).sum().backward()
    grads = {n: p.grad for n, p in enc.named_parameters()}
    bsd = {k[len('backbone.'):]: v for k, v in sd.items() if k.startswith('backbone.')}
    ref = R.run_ref(R.GEOM_A, True, video, keep.cpu(), sd=bsd, readout=(sd['projection.weight'], sd['projection.bias']))
    ref_grads = {(k if k.startswith('projection.') else 'backbone.' + k): g for k, g in ref.grads.items()}
    e = R.rel(feat, ref.out)
    worst, top = R.worst_grad_error(grads, ref_grads)
    print(f'VideoEncoder masked readout {dtype}: feature {e:.2e}  worst grad {worst:.2e}')
    assert e <= out_tol
    assert worst <= grad_tol, top


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_video_encoder_eval_is_unmasked(dtype):
    enc, _ = _encoder(dtype, 0.5)
    plain, _ = _encoder(dtype, 0.0)
    video = R.video_for(R.GEOM_A, 4).to(DEV)
    with torch.no_grad():
        assert torch.equal(enc.eval()(video), plain.eval()(video))
        assert not torch.equal(enc.train()(video), plain.train()(video))      # training mode does mask
        # an explicit mask is honoured in eval mode too
        mask = R.mask_of(R.keep_indices(4, 64, 24, 306), 64).to(DEV)
        a, b = enc.eval()(video, bool_masked_pos=mask), plain.eval()(video, bool_masked_pos=mask)
        assert torch.equal(a, b) and not torch.equal(a, plain(video))


def test_masked_crossmodal_train_step():
    from cmhar.losses import SigmoidContrastiveLoss
    from cmhar.models import CrossModalModel
    from cmhar.trainer import CrossModalTrainer
    B = 8
    imu, video = seeded_input(330, (B, 6, 64)).to(DEV), R.video_for(R.GEOM_A, B).to(DEV)
    seen = {}
    for ratio in (0.0, 0.5):
        cfg = _model_cfg('bf16', ratio)
        torch.manual_seed(0)                                         # the same initialisation for both ratios
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            m = CrossModalModel(cfg)
        tr =CrossModalTrainer(m, SigmoidContrastiveLoss().to(DEV), cfg, device=DEV)
        tr.model.train()
        torch.manual_seed(78)
        loss = tr.train_step(imu, video)
        seen[ratio] = (float(loss.detach()), {n: p.grad for n, p in m.named_parameters() if p.requires_grad},
                       all(bool(torch.isfinite(p).all()) for p in m.parameters()))
    loss0, g0, _ = seen[0.0]
    loss1, g1, finite_params = seen[0.5]
    assert loss1 == loss1 and abs(loss1) < float('inf') and finite_params
    assert loss1 != loss0                                            # the masked step encoded other tokens
    with_grad = [n for n, g in g0.items() if g is not None]
    assert len(with_grad) > 40
    for n in with_grad:
        assert g1[n] is not None and bool(torch.isfinite(g1[n]).all()), n
