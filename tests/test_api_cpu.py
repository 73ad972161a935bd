"""CPU-side checks: the C-ABI library loads and exports every symbol include/cmhar.h declares; the drop-in modules
have the reference's constructor signatures, attributes and EXACT state_dict keys/shapes (checked against the
key lists recorded from the reference in the golden fixtures); config field parity."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from fixtures import fixture_config, load

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(REPO, 'include', 'cmhar.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(cmhar_[a-z0-9_]+)\s*\(', src)))


def test_library_exports_every_declared_symbol():
    from cmhar import _lib
    lib = _lib.lib()
    syms = header_symbols()
    assert len(syms) >= 20
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    # and the python binding covers exactly the header
    assert sorted(_lib.EXPORTED) == syms
    assert lib.cmhar_version() == 1


@pytest.mark.parametrize('cname,pyname', [('CmharEpilogue', 'Epilogue'), ('CmharIMULayer', 'IMULayer')])
def test_struct_layout_matches_header(tmp_path, cname, pyname):
    """ctypes mirrors vs the C compiler's view of the ABI structs (offsetof every field, sizeof)."""
    import ctypes
    import shutil
    import subprocess
    from cmhar import _lib
    cc = shutil.which('gcc')
    if cc is None:
        pytest.skip('gcc not available')
    cls = getattr(_lib, pyname)
    fields = [f for f, _ in cls._fields_]
    src = tmp_path / 'probe.c'      # plain C: the header must be consumable by a C / cgo / FFI binding
    src.write_text(f'#include "cmhar.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){{printf("%zu", sizeof({cname}));'
                   + ''.join(f'printf(" %zu", offsetof({cname}, {f}));' for f in fields) + 'return 0;}\n')
    exe = tmp_path / 'probe'
    subprocess.run([cc, '-D__HIP_PLATFORM_AMD__', '-I/opt/rocm/include', f'-I{REPO}/include', str(src), '-o',
                    str(exe)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    assert got == want


def test_product_path_has_no_fallback(monkeypatch):
    from cmhar import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', '/nonexistent/libcmhar.so')
    with pytest.raises(RuntimeError, match='not found'):
        _lib.lib()


def _keys_shapes(fx):
    import json
    return list(zip(json.loads(str(fx['keys'])), [tuple(s) for s in json.loads(str(fx['shapes']))]))


def test_state_dict_keys_crossmodal_tiny():
    from cmhar.models import CrossModalModel
    fx = load('g2_crossmodal_tiny')
    cfg = fixture_config(fx)
    with pytest.warns(UserWarning):
        m = CrossModalModel(cfg)
    ours = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert ours == _keys_shapes(fx)


def test_state_dict_keys_imu_encoder_and_classifier():
    from cmhar.models import IMUClassifier, IMUEncoder
    fx = load('g1_imu_encoder')
    m = IMUEncoder(fixture_config(fx))
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == _keys_shapes(fx)
    fx4 = load('g4_classifier')
    cfg = fixture_config(fx4)
    c = IMUClassifier(IMUEncoder(cfg), cfg)
    assert [(k, tuple(v.shape)) for k, v in c.state_dict().items()] == _keys_shapes(fx4)
    assert not c.freeze_encoder
    c2 = IMUClassifier(IMUEncoder(cfg), cfg, freeze_encoder=True)
    assert c2.freeze_encoder
    c2.unfreeze_encoder()
    assert not c2.freeze_encoder


def test_state_dict_keys_videomae_base():
    """280-entry key set of the full model at the default (VideoMAE-B) geometry."""
    from cmhar.config import Config
    from cmhar.models import VideoEncoder
    fx = load('g5_videomae_base_16x224')
    cfg = Config()
    cfg.model.video_backbone = '/nonexistent/videomae'
    with pytest.warns(UserWarning):
        v = VideoEncoder(cfg)
    assert [(k, tuple(t.shape)) for k, t in v.state_dict().items()] == _keys_shapes(fx)
    assert v.is_videomae and v.feature_dim == 768
    assert sum(p.numel() for p in v.parameters()) == 86_825_472          # SURVEY §6 (backbone + projection)


def test_same_initialisation_as_reference_construction_order():
    """IMUEncoder / ProjectionHead are built in the reference's order from the reference's torch modules, so a
    given torch seed yields the same initial weights (checked for the deterministic parts of the structure)."""
    from cmhar.models import IMUEncoder
    from cmhar.config import Config
    cfg = Config()
    torch.manual_seed(123)
    a = IMUEncoder(cfg)
    torch.manual_seed(123)
    b = IMUEncoder(cfg)
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    assert a.pos_encoding.shape == (1, (250 - 16) // 16 + 1 + 1, 128)


def test_config_fields_mirror_reference():
    from cmhar.config import Config
    c = Config()
    for sect, fields in {
        'data': ['imu_window_size', 'imu_stride', 'imu_sampling_rate', 'imu_channels', 'video_fps',
                 'video_frames_per_window', 'video_resize', 'normalize_imu', 'median_filter_kernel'],
        'model': ['imu_patch_size', 'imu_stride', 'imu_d_model', 'imu_nhead', 'imu_num_layers', 'imu_dropout',
                  'video_backbone', 'video_pretrained', 'video_d_model', 'projection_dim', 'projection_hidden_dim',
                  'num_classes', 'classifier_hidden_dims', 'classifier_dropout'],
        'training': ['seed', 'device', 'pretrain_epochs', 'pretrain_batch_size', 'pretrain_lr',
                     'pretrain_weight_decay', 'pretrain_warmup_epochs', 'train_lr_encoder', 'train_lr_head'],
    }.items():
        for f in fields:
            assert hasattr(getattr(c, sect), f), (sect, f)
    assert c.model.video_backbone == 'MCG-NJU/videomae-base-ssv2'
    assert c.training.pretrain_lr == 1e-4 and c.model.imu_dropout == 0.1


def test_loss_module_surface():
    from cmhar.losses import SigmoidContrastiveLoss
    lf = SigmoidContrastiveLoss()
    assert abs(lf.temperature.item() - np.log(10.0)) < 1e-7 and lf.bias.item() == -10.0
    assert sorted(k for k, _ in lf.named_parameters()) == ['bias', 'temperature']
    lf2 = SigmoidContrastiveLoss(learnable=False)
    assert sorted(lf2.state_dict()) == ['bias', 'temperature'] and not list(lf2.parameters())


def test_r3d18_state_dict_matches_torchvision_layout():
    """torchvision `r3d_18(num_classes=400)` has 33 371 472 parameters and 122 state_dict entries; the drop-in keeps
    its key names so torchvision checkpoints load strict (the build constructs on CPU; compute needs the GPU)."""
    from cmhar.r3d import R3D18
    m = R3D18(400)
    sd = m.state_dict()
    assert sum(p.numel() for p in m.parameters()) == 33371472
    assert len(sd) == 122
    for k in ('stem.0.weight', 'stem.1.running_var', 'layer1.0.conv1.0.weight', 'layer1.1.conv2.1.bias',
              'layer2.0.downsample.0.weight', 'layer4.1.conv2.0.weight', 'fc.weight'):
        assert k in sd, k
    assert tuple(sd['stem.0.weight'].shape) == (64, 3, 3, 7, 7)
    assert tuple(sd['layer3.0.downsample.0.weight'].shape) == (256, 128, 1, 1, 1)


def test_unloadable_pretrained_backbone_raises(monkeypatch):
    """video_pretrained=True with a hub name that cannot be loaded must fail like
    VideoMAEModel.from_pretrained (reference models.py:157), unless random init is explicitly allowed."""
    from cmhar.config import Config
    from cmhar.models import VideoEncoder
    monkeypatch.delenv('CMHAR_ALLOW_RANDOM_INIT', raising=False)
    cfg = Config()
    cfg.model.videomae_num_layers, cfg.model.videomae_hidden_size = 1, 64
    cfg.model.videomae_num_heads, cfg.model.videomae_intermediate_size = 2, 128
    with pytest.raises(OSError):
        VideoEncoder(cfg)
    cfg.model.allow_random_init = True
    with pytest.warns(UserWarning):
        VideoEncoder(cfg)
    cfg.model.allow_random_init = False
    cfg.model.video_pretrained = False
    VideoEncoder(cfg)


def test_cnn2d_backbones_torchvision_layout():
    """resnet18 children()[:-2] / mobilenet_v2 .features (models.py:163-173): torchvision parameter counts and key
    names; hub / ImageNet weights are not fetchable offline, so video_pretrained=True raises unless opted in."""
    import pytest
    import torch
    from cmhar.cnn2d import MobileNetV2Features, ResNet18Features
    from cmhar.config import Config
    from cmhar.models import VideoEncoder
    from oracle import cnn2d_cpu as O
    r, m = ResNet18Features(), MobileNetV2Features()
    assert sum(p.numel() for p in r.parameters()) == 11_176_512     # resnet18 (11 689 512) minus fc (513 000)
    assert sum(p.numel() for p in m.parameters()) == 2_223_872      # mobilenet_v2 (3 504 872) minus classifier
    rk, mk = list(r.state_dict()), list(m.state_dict())
    assert rk[:2] == ['0.weight', '1.weight'] and '5.0.downsample.0.weight' in rk and '7.1.bn2.running_var' in rk
    assert mk[0] == '0.0.weight' and '1.conv.0.0.weight' in mk and '2.conv.3.running_mean' in mk
    assert mk[-1] == '18.1.num_batches_tracked' and len(m) == 19
    with torch.no_grad():
        fr = O.resnet18_features({k: v for k, v in r.state_dict().items()}, torch.randn(2, 3, 64, 64), False)
        fm = O.mobilenet_v2_features({k: v for k, v in m.state_dict().items()}, torch.randn(2, 3, 64, 64), False)
    assert fr.shape == (2, 512, 2, 2) and fm.shape == (2, 1280, 2, 2)
    cfg = Config()
    cfg.model.video_backbone = 'resnet18'
    cfg.model.video_pretrained = True
    cfg.model.allow_random_init = False
    import os
    old = os.environ.pop('CMHAR_ALLOW_RANDOM_INIT', None)
    try:
        with pytest.raises(OSError):
            VideoEncoder(cfg)
    finally:
        if old is not None:
            os.environ['CMHAR_ALLOW_RANDOM_INIT'] = old
    cfg.model.video_pretrained = False
    venc = VideoEncoder(cfg)
    assert venc.feature_dim == 512 and hasattr(venc, 'temporal_pool')
    assert all(k.startswith(('backbone.', 'projection.')) for k in venc.state_dict())


def test_imu_fused_gating():
    """The one-launch IMU encoder takes the reference geometry (d 128, 8 heads, FF 512, T <= 32, <= 8 layers) and
    leaves every other geometry to the per-op launches (CPU check of the dispatch only; the kernels are
    tests/test_imu_fused_gpu.py)."""
    from cmhar import imu
    from cmhar.config import Config
    from cmhar.imu import IMUEncoder
    ok = []
    for W, d, nh, nl in ((200, 128, 8, 4), (250, 128, 8, 4), (400, 128, 8, 4), (600, 128, 8, 4), (200, 64, 8, 4),
                         (200, 128, 4, 4), (200, 128, 8, 9)):
        cfg = Config()
        cfg.data.imu_window_size = W
        cfg.model.imu_d_model, cfg.model.imu_nhead, cfg.model.imu_num_layers = d, nh, nl
        m = IMUEncoder(cfg)
        T = min(1 + 6 * ((W - 16) // 16 + 1), m.pos_encoding.shape[1])
        ok.append(imu._fused_ok(m, T))
    assert ok == [True, True, True, False, False, False, False]


@pytest.mark.parametrize('backbone', ['videomae', 'r3d_18', 'resnet18'])
def test_multi_device_dataparallel_refused_with_pointer(backbone):
    """VERDICT r02 item 8 (SURVEY §8b threading contract): `nn.DataParallel(model)` over several GPUs replicates
    each submodule with `_replicate_for_data_parallel` (torch replicate.py); the cmhar HIP modules refuse it and
    name cmhar.dist, the supported DataParallel-equivalent path."""
    from cmhar.config import Config
    from cmhar.models import CrossModalModel
    cfg = Config()
    cfg.data.video_frames_per_window, cfg.data.video_resize = 2, (16, 16)
    m = cfg.model
    m.video_pretrained = False
    m.video_backbone = '/nonexistent/videomae' if backbone == 'videomae' else backbone
    m.videomae_hidden_size, m.videomae_num_layers, m.videomae_num_heads, m.videomae_intermediate_size = 64, 1, 1, 128
    model = CrossModalModel(cfg)
    refused = []
    for name, mod in model.named_modules():
        try:
            mod._replicate_for_data_parallel()
        except RuntimeError as e:
            assert 'cmhar.dist' in str(e) and 'GradReducer' in str(e)
            refused.append(name)
    assert {'imu_encoder', 'video_encoder.backbone', 'imu_proj', 'video_proj'} <= set(refused), refused


def test_bench_imu_flops_count():
    """bench.imu_flops_per_window (the config-1 workload's roofline numerator) at the reference geometry: 200-sample
    windows → 12 patches + CLS = 13 tokens of d 128, FF 512, 4 layers, 128-256-128-32 head."""
    import bench
    n, d, ff = 13, 128, 512
    want = 2 * 12 * 16 * d + 4 * (2 * n * (4 * d * d + 2 * d * ff) + 4 * n * n * d) + \
        2 * (128 * 256 + 256 * 128 + 128 * 32)
    assert bench.imu_flops_per_window(200) == want


def test_bench_arguments(monkeypatch):
    """bench.parse: `--steps` sets the number of timed steps in either spelling, for every workload (defaults: 50,
    and the 313-batch stream of ood_fp16); `--full` is off unless given; `--dump-outputs` takes the directory."""
    import bench

    def parse(*argv):
        monkeypatch.setattr(sys, 'argv', ['bench.py', *argv])
        return bench.parse()
    a = parse('--gpus', '1', '--steps', '7', '--warmup', '2')
    assert (a.steps, a.warmup, a.full, a.dump_outputs, a.workload) == (7, 2, False, None, 'videomae')
    assert parse().steps == 50 and parse('--workload', 'ood_fp16').steps == 313
    assert parse('--workload', 'ood_fp16', '--steps=5').steps == 5
    assert parse('--workload', 'ood_fp16', '--steps', '5').steps == 5
    a = parse('--full', '--dump-outputs', 'some/dir')
    assert a.full and a.dump_outputs == 'some/dir' and not a.no_trace and not a.no_cpu_baseline
