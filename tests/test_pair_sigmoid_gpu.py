"""`cmhar_pair_sigmoid_loss` (csrc/pair_sigmoid.hip), `cmhar.losses.PairwiseSigmoidLoss` and the trainer's use of it.

The reference is fp64 torch, written here: the formula of include/cmhar.h under `torch.autograd.grad`.  Error measures
and bound are those of tests/test_loss_kernels_gpu.py's SigLIP test: `rel(x, ref) = ‖x − ref‖/‖ref‖ ≤ 1e-5` for the
loss, da, db and gbias; the temperature gradient, a cancelling sum, against the fp64 sum of its terms' magnitudes,
`≤ 1e-5`.  Shard-against-full, repeated-run and NULL-output comparisons are exact (`torch.equal`).  Outputs are
prefilled with NaN."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

DEV = 'cuda'
pytestmark = pytest.mark.gpu
NAN = float('nan')
TOL = 1e-5
SHAPES = [(1, 32), (5, 100), (17, 36), (63, 64), (64, 64), (65, 128), (130, 1024), (257, 256)]
TB = [(math.log(10.0), -10.0), (math.log(100.0), -5.0), (0.0, 0.0)]
TB_IDS = ['t10-b10', 't100-b5-saturated', 't1-b0']


def K():
    from cmhar import kernels
    return kernels


def L():
    from cmhar import _lib
    return _lib


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def nans(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def _raw(a, b, t, bias, ga=None, gb=None, sg=0, a_rows=None, b_rows=None, want=('da', 'db', 'gt', 'gbias'), rc=False):
    """cmhar_pair_sigmoid_loss over NaN-filled outputs -> dict(loss, da, db, gt, gbias); outputs not in `want` are
    passed as NULL and come back as None.  a / b may be strided row views (unit inner stride)."""
    Ba, D = a.shape
    Bb = b.shape[0]
    a_off, a_cnt = a_rows if a_rows is not None else (0, Ba)
    b_off, b_cnt = b_rows if b_rows is not None else (0, Bb)
    o = dict(loss=nans(1), da=nans(a_cnt, D) if 'da' in want else None, db=nans(b_cnt, D) if 'db' in want else None,
             gt=nans(1) if 'gt' in want else None, gbias=nans(1) if 'gbias' in want else None)
    ws = K().workspace(max(L().lib().cmhar_pair_sigmoid_ws(Ba, Bb, D), 4) // 4 + 1, a.device)
    p = L().ptr
    args = (Ba, Bb, D, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), p(ga), p(gb), sg, t.data_ptr(),
            bias.data_ptr(), o['loss'].data_ptr(), p(o['da']), a_off, a_cnt, p(o['db']), b_off, b_cnt, p(o['gt']),
            p(o['gbias']), ws.data_ptr(), L().stream(a.device))
    if rc:
        code = L().lib().cmhar_pair_sigmoid_loss(*args)
        torch.cuda.synchronize()
        return code, o
    L().call('cmhar_pair_sigmoid_loss', *args)
    return o


def _ref64(a, b, t, bias, ga=None, gb=None, sg=0):
    """fp64 autograd of loss = (1/Ba)·Σ w·softplus(−z·S): dict of the five outputs plus mag_t = Σ|dS·dot·e^t|."""
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    t64, c64 = t.double().requires_grad_(True), bias.double().requires_grad_(True)
    Ba, Bb = a.shape[0], b.shape[0]
    dots = a64 @ b64.T
    S = dots * t64.exp() + c64
    eye = torch.eye(Ba, Bb, dtype=torch.bool, device=a.device)
    z = torch.where(eye, 1.0, -1.0).double()
    w = torch.ones(Ba, Bb, dtype=torch.float64, device=a.device)
    if ga is not None:
        same = (ga[:, None] == gb[None, :]) & ~eye
        if sg == 1:
            w = torch.where(same, 0.0, 1.0).double()
        elif sg == 2:
            z = torch.where(same | eye, 1.0, -1.0).double()
    x = -z * S
    loss = (w * (x.clamp_min(0) + torch.log1p(torch.exp(-x.abs())))).sum() / Ba
    da, db, gt, gc, gS = torch.autograd.grad(loss, (a64, b64, t64, c64, S))
    mag_t = (gS * dots.detach() * t64.detach().exp()).abs().sum()
    return dict(loss=loss.detach(), da=da, db=db, gt=gt, gbias=gc, mag_t=mag_t)


def _errors(o, r):
    e = {k: rel(o[k], r[k]) for k in ('loss', 'da', 'db', 'gbias') if o[k] is not None}
    if o['gt'] is not None:
        e['gt'] = abs(o['gt'].item() - r['gt'].item()) / max(r['mag_t'].item(), 1e-300)
    return e


@functools.lru_cache(maxsize=None)
def _inputs(Ba, Bb, D):
    """Unit rows a [Ba, D], b [Bb, D] and group ids in [0, 4) for both sides (shared by the tests; never modified)."""
    g = torch.Generator().manual_seed(1000 * Ba + 10 * Bb + D)
    a = F.normalize(torch.randn(Ba, D, generator=g).double(), dim=1).float().to(DEV)
    b = F.normalize(torch.randn(Bb, D, generator=g).double(), dim=1).float().to(DEV)
    n = max(Ba, Bb)
    ids = torch.randint(0, 4, (n,), generator=g).to(DEV)
    return a, b, ids[:Ba].contiguous(), ids[:Bb].contiguous()


def _scalars(t, bias):
    return torch.tensor([t], device=DEV), torch.tensor([bias], device=DEV)


@pytest.mark.parametrize('sg', [0, 1, 2], ids=['negative', 'ignore', 'positive'])
@pytest.mark.parametrize('t,bias', TB, ids=TB_IDS)
@pytest.mark.parametrize('B,D', SHAPES)
def test_values_and_gradients(B, D, t, bias, sg):
    a, b, ga, gb = _inputs(B, B, D)
    tt, bb = _scalars(t, bias)
    o = _raw(a, b, tt, bb, ga, gb, sg)
    r = _ref64(a, b, tt, bb, ga, gb, sg)
    e = _errors(o, r)
    print(f'pair_sigmoid B={B} D={D} t={t:.3f} bias={bias} same_group={sg}: '
          + ' '.join(f'{k} {v:.2e}' for k, v in e.items()))
    assert all(v <= TOL for v in e.values()), e


def test_no_ids_is_plain_siglip():
    """Without ids every off-diagonal pair is negative, whatever same_group says; with ids, same_group 0 is the same."""
    a, b, ga, gb = _inputs(65, 65, 128)
    tt, bb = _scalars(*TB[0])
    plain = _raw(a, b, tt, bb)
    for other in (_raw(a, b, tt, bb, None, None, 2), _raw(a, b, tt, bb, ga, gb, 0)):
        assert all(torch.equal(plain[k], other[k]) for k in plain)
    e = _errors(plain, _ref64(a, b, tt, bb))
    assert all(v <= TOL for v in e.values()), e


@pytest.mark.parametrize('B,D', SHAPES)
def test_shard_invariance_and_determinism(B, D):
    """The two data-parallel shards (rows [0, ⌈B/2⌉) and the rest; B = 1: the second has no rows) give the full run's
    gradient rows, loss, gt and gbias to the bit; so does a second full run."""
    a, b, ga, gb = _inputs(B, B, D)
    tt, bb = _scalars(*TB[0])
    h = (B + 1) // 2
    for sg in (0, 1, 2):
        full = _raw(a, b, tt, bb, ga, gb, sg)
        again = _raw(a, b, tt, bb, ga, gb, sg)
        assert all(torch.equal(full[k], again[k]) for k in full), sg
        assert not any(bool(torch.isnan(v).any()) for v in full.values())
        for off, cnt in ((0, h), (h, B - h)):
            s = _raw(a, b, tt, bb, ga, gb, sg, (off, cnt), (off, cnt))
            assert torch.equal(s['da'], full['da'][off:off + cnt]) and torch.equal(s['db'], full['db'][off:off + cnt])
            assert all(torch.equal(s[k], full[k]) for k in ('loss', 'gt', 'gbias'))


@pytest.mark.parametrize('B,D', [(17, 36), (130, 1024), (257, 256)])
def test_null_outputs(B, D):
    a, b, ga, gb = _inputs(B, B, D)
    tt, bb = _scalars(*TB[0])
    full = _raw(a, b, tt, bb, ga, gb, 1)
    none = _raw(a, b, tt, bb, ga, gb, 1, want=())
    assert torch.equal(none['loss'], full['loss'])
    nodb = _raw(a, b, tt, bb, ga, gb, 1, want=('da', 'gt', 'gbias'))
    assert all(torch.equal(nodb[k], full[k]) for k in ('loss', 'da', 'gt', 'gbias'))


@pytest.mark.parametrize('sg', [0, 1, 2])
@pytest.mark.parametrize('Ba,Bb,D', [(3, 70, 64), (70, 3, 64)])
def test_rectangular(Ba, Bb, D, sg):
    """Ba != Bb through the raw ABI: the rows past the square part have no positive of their own."""
    a, b, ga, gb = _inputs(Ba, Bb, D)
    tt, bb = _scalars(*TB[0])
    o = _raw(a, b, tt, bb, ga, gb, sg)
    e = _errors(o, _ref64(a, b, tt, bb, ga, gb, sg))
    print(f'pair_sigmoid Ba={Ba} Bb={Bb} D={D} same_group={sg}: ' + ' '.join(f'{k} {v:.2e}' for k, v in e.items()))
    assert all(v <= TOL for v in e.values()), e


@pytest.mark.parametrize('B,D,width,first', [(70, 256, 320, 32), (33, 100, 103, 1), (33, 30, 30, 0)],
                         ids=['lda320-aligned', 'D100-misaligned', 'D30-odd-stride'])
def test_strided_rows(B, D, width, first):
    """a is a column slice of a wider tensor; rows that are not 16-byte aligned take the scalar staging path.  The
    values must be those of the contiguous copy, to the bit, and right against fp64."""
    g = torch.Generator().manual_seed(B + D)
    wide = torch.randn(B, width, generator=g).to(DEV)
    wide[:, first:first + D] = F.normalize(wide[:, first:first + D], dim=1)
    a = wide[:, first:first + D]
    assert a.stride(0) == width and a.data_ptr() == wide.data_ptr() + 4 * first
    _, b, ga, gb = _inputs(B, B, D)
    tt, bb = _scalars(*TB[0])
    o = _raw(a, b, tt, bb, ga, gb, 1)
    e = _errors(o, _ref64(a, b, tt, bb, ga, gb, 1))
    assert all(v <= TOL for v in e.values()), e
    c = _raw(a.contiguous(), b, tt, bb, ga, gb, 1)
    assert all(torch.equal(o[k], c[k]) for k in o)
    o2 = _raw(b, a, tt, bb, gb, ga, 1)                     # the strided operand on the column side
    e2 = _errors(o2, _ref64(b, a, tt, bb, gb, ga, 1))
    assert all(v <= TOL for v in e2.values()), e2


def test_beyond_the_old_kernels_limit():
    """B = 1500 > 1024: cmhar_siglip_loss refuses it, the tiled kernel does not store the matrix and takes it."""
    B, D = 1500, 32
    a, b, ga, gb = _inputs(B, B, D)
    tt, bb = _scalars(*TB[0])
    old = L().lib().cmhar_siglip_loss(B, B, D, a.data_ptr(), b.data_ptr(), tt.data_ptr(), bb.data_ptr(),
                                      nans(1).data_ptr(), None, 0, 0, None, 0, 0, None, None,
                                      K().workspace(1, DEV).data_ptr(), L().stream(DEV))
    assert old == -1
    o = _raw(a, b, tt, bb, ga, gb, 1)
    e = _errors(o, _ref64(a, b, tt, bb, ga, gb, 1))
    print('pair_sigmoid B=1500 D=32: ' + ' '.join(f'{k} {v:.2e}' for k, v in e.items()))
    assert all(v <= TOL for v in e.values()), e
    # stated, not measured: (Ba + Bb)·D·4 B = 64 MiB plus small terms is the allowance at the largest shape
    assert 0 < L().lib().cmhar_pair_sigmoid_ws(32768, 32768, 256) < 128 << 20


@pytest.mark.parametrize('Ba,Bb', [(8160, 8160), (8180, 8200), (12000, 4500)],
                         ids=['last-16-row-strips', 'first-32-row-strips', '32-row-strips-rectangular'])
def test_wide_strips(Ba, Bb):
    """From 512 strips of 32 rows on (both sides together, D <= 256) a workgroup owns 32 rows instead of 16: values
    against fp64 on both sides of that threshold, and shards cut at a row that is no multiple of 32."""
    D = 40
    a, b, ga, gb = _inputs(Ba, Bb, D)
    tt, bb = _scalars(*TB[0])
    full = _raw(a, b, tt, bb, ga, gb, 1)
    e = _errors(full, _ref64(a, b, tt, bb, ga, gb, 1))
    print(f'pair_sigmoid Ba={Ba} Bb={Bb} D={D}: ' + ' '.join(f'{k} {v:.2e}' for k, v in e.items()))
    assert all(v <= TOL for v in e.values()), e
    s = _raw(a, b, tt, bb, ga, gb, 1, (1001, 77), (2037, 150))
    assert torch.equal(s['da'], full['da'][1001:1078]) and torch.equal(s['db'], full['db'][2037:2187])
    assert all(torch.equal(s[k], full[k]) for k in ('loss', 'gt', 'gbias'))


@pytest.mark.parametrize('Ba,Bb,D,sg', [(2, 2, 1056, 0), (32769, 2, 1, 0), (4, 4, 32, 3)],
                         ids=['D1056', 'Ba32769', 'same_group3'])
def test_rejections_write_nothing(Ba, Bb, D, sg):
    a, b = torch.zeros(Ba, D, device=DEV), torch.zeros(Bb, D, device=DEV)
    ga, gb = torch.zeros(Ba, dtype=torch.int64, device=DEV), torch.zeros(Bb, dtype=torch.int64, device=DEV)
    tt, bb = _scalars(0.0, 0.0)
    code, o = _raw(a, b, tt, bb, ga, gb, sg, rc=True)
    assert code == -1
    assert all(bool(torch.isnan(v).all()) for v in o.values())


# ---------------------------------------------------------------------------------------------------------------
# module
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('same_group', ['negative', 'ignore', 'positive'])
def test_module_matches_raw_call(same_group):
    from cmhar.losses import PairwiseSigmoidLoss
    B, D = 65, 128
    a, b, ga, _ = _inputs(B, B, D)
    sg = {'negative': 0, 'ignore': 1, 'positive': 2}[same_group]
    lf = PairwiseSigmoidLoss(same_group=same_group, group=False)            # parameters stay on the CPU (main.py:97)
    tt, bb = _scalars(lf.temperature.item(), lf.bias.item())
    raw = _raw(a, b, tt, bb, ga, ga, sg)
    for scale in (1.0, 3.0):
        ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        lf.zero_grad(set_to_none=True)
        loss = lf(ar, br, labels=ga.cpu() if scale == 1.0 else ga)          # host or device ids
        assert loss.shape == () and loss.device.type == 'cuda'
        assert torch.equal(loss.reshape(1), raw['loss'])
        (loss * scale).backward()
        assert torch.equal(ar.grad, raw['da'] * scale) and torch.equal(br.grad, raw['db'] * scale)
        assert lf.temperature.grad.device.type == 'cpu' and lf.bias.grad.device.type == 'cpu'
        assert torch.equal(lf.temperature.grad.reshape(1), (raw['gt'] * scale).cpu())
        assert torch.equal(lf.bias.grad.reshape(1), (raw['gbias'] * scale).cpu())
    with torch.no_grad():
        assert torch.equal(lf(a, b, labels=ga).reshape(1), raw['loss'])
    fz = PairwiseSigmoidLoss(same_group=same_group, learnable=False, group=False).to(DEV)
    assert torch.equal(fz(a, b, labels=ga).reshape(1), raw['loss'])         # nothing requires grad: the NULL path


def test_no_grad_path_passes_null_gradients(monkeypatch):
    """Under no_grad (and when nothing requires grad) the four gradient pointers are NULL: no gradient product is paid."""
    from cmhar import losses
    a, b, _, _ = _inputs(17, 17, 36)
    seen = []
    real = losses.L.call

    def spy(name, *args):
        seen.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(losses.L, 'call', spy)
    lf = losses.PairwiseSigmoidLoss(group=False)
    with torch.no_grad():
        lf(a, b)
    lf(a, b).backward()
    (n0, a0), (n1, a1) = seen
    assert n0 == n1 == 'cmhar_pair_sigmoid_loss'
    grads = lambda args: (args[13], args[16], args[19], args[20])            # da, db, gt, gbias
    assert grads(a0) == (None, None, None, None)
    assert all(p is not None for p in grads(a1))


# ---------------------------------------------------------------------------------------------------------------
# it actually contrasts
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_toy_problem_learns_to_retrieve(seed):
    """64 pairs from a shared 16-d latent, two linear encoders (48 -> 32, 40 -> 32, 0.1·randn), torch Adam lr 1e-2,
    100 steps on the GPU kernel's loss: recall@1 >= 0.95 both ways (the fp32 CPU formula reaches 1.0 for the three
    seeds, and e^temperature ends near 13.6; `SigmoidContrastiveLoss` stays at chance, 1/64)."""
    from cmhar.losses import PairwiseSigmoidLoss
    from cmhar.retrieval import recall_at_k
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(64, 16, generator=g)
    x = (z @ torch.randn(16, 48, generator=g)).to(DEV)
    y = (z @ torch.randn(16, 40, generator=g)).to(DEV)
    Wa = (0.1 * torch.randn(48, 32, generator=g)).to(DEV).requires_grad_(True)
    Wb = (0.1 * torch.randn(40, 32, generator=g)).to(DEV).requires_grad_(True)
    lf = PairwiseSigmoidLoss(group=False).to(DEV)
    t0 = lf.temperature.item()
    opt = torch.optim.Adam([Wa, Wb, *lf.parameters()], lr=1e-2)
    for _ in range(100):
        loss = lf(F.normalize(x @ Wa, dim=1), F.normalize(y @ Wb, dim=1))
        opt.zero_grad()
        loss.backward()
        opt.step()
    with torch.no_grad():
        r = recall_at_k(F.normalize(x @ Wa, dim=1), F.normalize(y @ Wb, dim=1), ks=(1,))
    print(f'toy seed {seed}: loss {loss.item():.4f} recall@1 {r} e^t {math.exp(lf.temperature.item()):.3f}')
    assert r['imu_to_video'][1] >= 0.95 and r['video_to_imu'][1] >= 0.95, r
    assert abs(lf.temperature.item() - t0) > 1e-3


# ---------------------------------------------------------------------------------------------------------------
# trainer
# ---------------------------------------------------------------------------------------------------------------
def _tiny():
    from fixtures import fixture_config, fixture_state_dict, load
    from cmhar import models
    fx = load('g2_crossmodal_tiny')
    cfg = fixture_config(fx)
    cfg.model.compute_dtype = 'fp32'
    torch.manual_seed(0)
    m = models.CrossModalModel(cfg)
    m.load_state_dict(fixture_state_dict(fx), strict=True)
    batches = [{'imu': torch.tensor(fx['imu']), 'video': torch.tensor(fx['video'])},
               {'imu': torch.tensor(fx['step_imu2']), 'video': torch.tensor(fx['step_video2'])}]
    return m, cfg, batches


def test_trainer_trains_loss_parameters():
    from cmhar.losses import PairwiseSigmoidLoss
    from cmhar.trainer import CrossModalTrainer
    m, cfg, batches = _tiny()
    lf = PairwiseSigmoidLoss()
    t0, b0 = lf.temperature.item(), lf.bias.item()
    tr = CrossModalTrainer(m, lf, cfg, device=DEV, train_loss_params=True)
    assert lf.temperature.is_cuda and lf.bias.is_cuda
    groups = tr.optimizer.param_groups
    assert len(groups) == 2 and groups[1]['weight_decay'] == 0
    assert {id(p) for p in groups[1]['params']} == {id(lf.temperature), id(lf.bias)}
    assert groups[0]['lr'] == groups[1]['lr']
    assert {id(lf.temperature), id(lf.bias)} <= {id(p) for p in tr.optimizer.clip_params}
    for bt in batches:
        loss = tr.train_step(*tr._batch(bt))
    assert math.isfinite(loss.item())
    assert lf.temperature.item() != t0 and lf.bias.item() != b0


def test_trainer_checkpoint_keeps_loss_parameters(tmp_path):
    """With train_loss_params the checkpoint carries the loss's state and `cmhar.checkpoint.resume` restores it, so the
    restored Adam moments meet the values they belong to; without it the checkpoint has no such key."""
    from cmhar.checkpoint import resume
    from cmhar.losses import PairwiseSigmoidLoss
    from cmhar.trainer import CrossModalTrainer
    m, cfg, batches = _tiny()
    lf = PairwiseSigmoidLoss()
    tr = CrossModalTrainer(m, lf, cfg, device=DEV, train_loss_params=True)
    for bt in batches:
        tr.train_step(*tr._batch(bt))
    tr.save_checkpoint(tmp_path / 'last.pt', extra=tr._extra())
    m2, cfg2, _ = _tiny()
    lf2 = PairwiseSigmoidLoss()
    tr2 = CrossModalTrainer(m2, lf2, cfg2, device=DEV, train_loss_params=True)
    resume(tr2, tmp_path / 'last.pt')
    assert torch.equal(lf2.temperature, lf.temperature) and torch.equal(lf2.bias, lf.bias)
    assert lf2.temperature.item() != pytest.approx(math.log(10.0), abs=1e-7)
    st = tr2.optimizer.state[lf2.temperature]
    assert torch.equal(st['exp_avg'], tr.optimizer.state[lf.temperature]['exp_avg'])
    m3, cfg3, _ = _tiny()
    tr3 = CrossModalTrainer(m3, PairwiseSigmoidLoss(), cfg3, device=DEV)
    assert 'loss_state_dict' not in tr3._extra()


def test_trainer_default_is_unchanged():
    """train_loss_params=False with the reference-parity loss: the same bits as a trainer built without the keyword,
    one optimizer group, the loss's parameters left alone."""
    from cmhar.losses import SigmoidContrastiveLoss
    from cmhar.trainer import CrossModalTrainer
    after = []
    for kw in ({}, {'train_loss_params': False}):
        m, cfg, batches = _tiny()
        lf = SigmoidContrastiveLoss().to(DEV)
        tr = CrossModalTrainer(m, lf, cfg, device=DEV, **kw)
        assert len(tr.optimizer.param_groups) == 1
        for bt in batches:
            tr.train_step(*tr._batch(bt))
        assert lf.temperature.item() == pytest.approx(math.log(10.0)) and lf.bias.item() == -10.0
        after.append({k: v.detach().clone() for k, v in m.state_dict().items()})
    assert after[0].keys() == after[1].keys()
    for k in after[0]:
        assert torch.equal(after[0][k], after[1][k]), k


def test_trainer_passes_labels():
    from cmhar.losses import PairwiseSigmoidLoss
    from cmhar.trainer import CrossModalTrainer
    m, cfg, batches = _tiny()
    seen = []

    class Spy(PairwiseSigmoidLoss):
        def forward(self, a, b, labels=None):
            seen.append(labels)
            return super().forward(a, b, labels)
    for i, bt in enumerate(batches):
        n = bt['imu'].shape[0]
        bt['label'] = (torch.arange(n) + i) % 2
    tr = CrossModalTrainer(m, Spy(same_group='ignore').to(DEV), cfg, device=DEV)
    assert math.isfinite(tr.train_epoch(batches))
    assert math.isfinite(tr.validate(batches))
    assert len(seen) == 4 and all(s is not None for s in seen)
    assert all(torch.equal(s.cpu(), bt['label']) for s, bt in zip(seen, batches + batches))
