"""PairwiseSigmoidLoss (the real SigLIP loss next to the reference-parity `SigmoidContrastiveLoss`): the parts that
need no GPU — the two ABI symbols, the factory names, parameters versus buffers, every argument check (raised on CPU
tensors before anything is launched) and the trainer's new keyword."""
import inspect
import math

import pytest
import torch


def test_library_exports_pair_sigmoid_symbols():
    from cmhar import _lib
    lib = _lib.lib()
    for name in ('cmhar_pair_sigmoid_ws', 'cmhar_pair_sigmoid_loss'):
        assert name in _lib._SIGS
        assert hasattr(lib, name), name


def test_workspace_never_quadratic():
    """Stated, not measured: the issue allows (Ba + Bb)·D·4 B = 64 MiB plus small terms at the largest shape."""
    from cmhar import _lib
    ws = _lib.lib().cmhar_pair_sigmoid_ws(32768, 32768, 256)
    assert 0 < ws < 128 << 20


@pytest.mark.parametrize('name', ['siglip', 'pairwise_sigmoid'])
def test_factory_returns_pairwise_sigmoid(name):
    from cmhar.losses import PairwiseSigmoidLoss, SigmoidContrastiveLoss, get_loss_function
    lf = get_loss_function(name, same_group='ignore')
    assert isinstance(lf, PairwiseSigmoidLoss) and lf.same_group == 'ignore'
    assert PairwiseSigmoidLoss.wants_labels is True
    assert isinstance(get_loss_function('sigmoid_contrastive'), SigmoidContrastiveLoss)     # unchanged
    assert not getattr(SigmoidContrastiveLoss, 'wants_labels', False)


def test_parameters_follow_learnable():
    from cmhar.losses import PairwiseSigmoidLoss
    lf = PairwiseSigmoidLoss(init_temperature=7.0, init_bias=-3.0)
    assert sorted(n for n, _ in lf.named_parameters()) == ['bias', 'temperature']
    assert lf.temperature.item() == pytest.approx(math.log(7.0)) and lf.bias.item() == -3.0
    fz = PairwiseSigmoidLoss(learnable=False)
    assert list(fz.parameters()) == []
    assert sorted(n for n, _ in fz.named_buffers()) == ['bias', 'temperature']
    assert fz.temperature.item() == pytest.approx(math.log(10.0)) and fz.bias.item() == -10.0


def test_unknown_same_group_raises():
    from cmhar.losses import PairwiseSigmoidLoss
    with pytest.raises(ValueError):
        PairwiseSigmoidLoss(same_group='push')
    lf = PairwiseSigmoidLoss()
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
    from cmhar.losses import PairwiseSigmoidLoss

    def no_launch(*args, **kw):
        raise AssertionError('a kernel call was attempted')
    monkeypatch.setattr(_lib, 'call', no_launch)
    with pytest.raises(ValueError):
        PairwiseSigmoidLoss(same_group=same_group)(a, b, labels)


def test_trainer_accepts_train_loss_params():
    from cmhar.trainer import CrossModalTrainer
    sig = inspect.signature(CrossModalTrainer.__init__)
    p = sig.parameters['train_loss_params']
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(CrossModalTrainer.train_step).parameters['labels'].default is None
