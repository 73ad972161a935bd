"""SoftmaxContrastiveLoss (the softmax contrastive loss on the tiled kernel, next to the composite `InfoNCELoss`): the
parts that need no GPU — the two ABI symbols, the workspace bound, the factory names, parameter versus buffer and
every argument check (raised on CPU tensors before anything is launched)."""
import math

import pytest
import torch


def test_library_exports_softmax_contrast_symbols():
    from cmhar import _lib
    lib = _lib.lib()
    for name in ('cmhar_softmax_contrast_ws', 'cmhar_softmax_contrast_loss'):
        assert name in _lib._SIGS
        assert hasattr(lib, name), name


def test_workspace_never_quadratic():
    """Stated, not measured: positive and below 64 MiB at the largest batch, where the matrix alone would be 4 GiB;
    nothing for a shape the kernel rejects."""
    from cmhar import _lib
    ws = _lib.lib().cmhar_softmax_contrast_ws
    assert 0 < ws(32768, 256) < 64 << 20
    assert 0 < ws(32768, 1024) < 64 << 20
    assert ws(32769, 256) == 0 and ws(4, 1056) == 0


@pytest.mark.parametrize('name,default', [('softmax_contrastive', 'negative'), ('clip', 'negative'),
                                          ('supcon', 'positive')])
def test_factory_names(name, default):
    from cmhar.losses import InfoNCELoss, SoftmaxContrastiveLoss, get_loss_function
    lf = get_loss_function(name)
    assert type(lf) is SoftmaxContrastiveLoss and lf.same_group == default
    assert get_loss_function(name, same_group='ignore', learnable=False).same_group == 'ignore'
    assert SoftmaxContrastiveLoss.wants_labels is True
    nce = get_loss_function('infonce', temperature=0.1)                                     # unchanged
    assert type(nce) is InfoNCELoss and nce.temperature == 0.1
    assert not getattr(InfoNCELoss, 'wants_labels', False)


def test_parameter_follows_learnable():
    from cmhar.losses import SoftmaxContrastiveLoss
    lf = SoftmaxContrastiveLoss()
    assert [n for n, _ in lf.named_parameters()] == ['temperature'] and list(lf.buffers()) == []
    assert lf.temperature.item() == pytest.approx(math.log(1 / 0.07))
    fz = SoftmaxContrastiveLoss(init_temperature=7.0, learnable=False)
    assert list(fz.parameters()) == []
    assert [n for n, _ in fz.named_buffers()] == ['temperature']
    assert fz.temperature.item() == pytest.approx(math.log(7.0))
    assert not hasattr(lf, 'bias')                                    # a softmax does not see one


def test_unknown_same_group_raises():
    from cmhar.losses import SoftmaxContrastiveLoss
    with pytest.raises(ValueError):
        SoftmaxContrastiveLoss(same_group='push')
    lf = SoftmaxContrastiveLoss()
    lf.same_group = 'push'
    with pytest.raises(ValueError):
        lf(torch.zeros(4, 8), torch.zeros(4, 8))


@pytest.mark.parametrize('a,b,labels,same_group', [
    (torch.zeros(4, 8), torch.zeros(5, 8), None, 'negative'),                     # shapes that do not match
    (torch.zeros(4, 8), torch.zeros(4, 9), None, 'negative'),
    (torch.zeros(4, 8, 1), torch.zeros(4, 8, 1), None, 'negative'),
    (torch.zeros(2, 1056), torch.zeros(2, 1056), None, 'negative'),               # D > 1024
    (torch.zeros(32769, 1), torch.zeros(32769, 1), None, 'negative'),             # B > 32768
    (torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4), 'ignore'),             # floating-point labels
    (torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4), 'negative'),
    (torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(5, dtype=torch.int64), 'positive'),   # wrong length
    (torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4, 1, dtype=torch.int64), 'ignore'),
    (torch.zeros(4, 8), torch.zeros(4, 8), None, 'ignore'),                       # needs labels
    (torch.zeros(4, 8), torch.zeros(4, 8), None, 'positive'),
], ids=['rows', 'cols', 'rank3', 'D1056', 'B32769', 'float-labels', 'float-labels-negative', 'long-labels',
        'labels-2d', 'ignore-no-labels', 'positive-no-labels'])
def test_argument_checks_raise_before_any_launch(a, b, labels, same_group, monkeypatch):
    from cmhar import _lib
    from cmhar.losses import SoftmaxContrastiveLoss

    def no_launch(*args, **kw):
        raise AssertionError('a kernel call was attempted')
    monkeypatch.setattr(_lib, 'call', no_launch)
    with pytest.raises(ValueError):
        SoftmaxContrastiveLoss(same_group=same_group)(a, b, labels)
