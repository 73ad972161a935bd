"""`cmhar_softmax_contrast_loss` (csrc/softmax_contrast.hip), `cmhar.losses.SoftmaxContrastiveLoss` and the trainer's
use of it.

The reference is fp64 torch, written here: the formula of include/cmhar.h under `torch.autograd.grad`.  Error measures
and bound are those of tests/test_pair_sigmoid_gpu.py: `rel(x, ref) = ‖x − ref‖/‖ref‖ ≤ 1e-5` for the loss, da and db;
the temperature gradient, a cancelling sum, against the fp64 sum of its terms' magnitudes, `≤ 1e-5`.
Shard-against-full, repeated-run and NULL-output comparisons are exact (`torch.equal`).  Outputs are prefilled with
NaN."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

DEV = 'cuda'
pytestmark = pytest.mark.gpu
NAN = float('nan')
TOL = 1e-5
SHAPES = [(5, 100), (17, 36), (63, 64), (64, 64), (65, 128), (130, 1024), (257, 256)]
SCALES = [1 / 0.07, 1.0, 100.0]
SCALE_IDS = ['s14', 's1', 's100']
MODES = ['negative', 'ignore', 'positive']


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


def _raw(a, b, t, ids=None, sg=0, a_rows=None, b_rows=None, want=('da', 'db', 'gt'), rc=False):
    """cmhar_softmax_contrast_loss over NaN-filled outputs -> dict(loss, da, db, gt); outputs not in `want` are passed
    as NULL and come back as None.  a / b may be strided row views (unit inner stride)."""
    B, D = a.shape
    a_off, a_cnt = a_rows if a_rows is not None else (0, B)
    b_off, b_cnt = b_rows if b_rows is not None else (0, B)
    o = dict(loss=nans(1), da=nans(a_cnt, D) if 'da' in want else None, db=nans(b_cnt, D) if 'db' in want else None,
             gt=nans(1) if 'gt' in want else None)
    ws = K().workspace(max(L().lib().cmhar_softmax_contrast_ws(B, D), 4) // 4 + 1, a.device)
    p = L().ptr
    args = (B, D, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), p(ids), sg, t.data_ptr(),
            o['loss'].data_ptr(), p(o['da']), a_off, a_cnt, p(o['db']), b_off, b_cnt, p(o['gt']), ws.data_ptr(),
            L().stream(a.device))
    if rc:
        code = L().lib().cmhar_softmax_contrast_loss(*args)
        torch.cuda.synchronize()
        return code, o
    L().call('cmhar_softmax_contrast_loss', *args)
    return o


def _ref64(a, b, t, ids=None, sg=0):
    """fp64 autograd of the loss of include/cmhar.h: dict of the four outputs plus mag_t = Σ|dS·S|."""
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    t64 = t.double().requires_grad_(True)
    B = a.shape[0]
    S = (a64 @ b64.T) * t64.exp()
    eye = torch.eye(B, dtype=torch.bool, device=a.device)
    same = (ids[:, None] == ids[None, :]) & ~eye if ids is not None else torch.zeros_like(eye)
    P = ((eye | same) if sg == 2 else eye).double()
    V = ~same if sg == 1 else torch.ones_like(eye)
    n = P.sum(1)
    Sm = S.masked_fill(~V, -math.inf)
    lse_r, lse_c = torch.logsumexp(Sm, 1), torch.logsumexp(Sm, 0)
    loss = (lse_r - (S * P).sum(1) / n + lse_c - (S * P).sum(0) / n).sum() / (2 * B)
    da, db, gt, gS = torch.autograd.grad(loss, (a64, b64, t64, S))
    return dict(loss=loss.detach(), da=da, db=db, gt=gt, mag_t=(gS * S.detach()).abs().sum())


def _errors(o, r):
    e = {k: rel(o[k], r[k]) for k in ('loss', 'da', 'db') if o[k] is not None}
    if o['gt'] is not None:
        e['gt'] = abs(o['gt'].item() - r['gt'].item()) / max(r['mag_t'].item(), 1e-300)
    return e


def _check(o, r, what):
    e = _errors(o, r)
    print(f'softmax_contrast {what}: ' + ' '.join(f'{k} {v:.2e}' for k, v in e.items()))
    assert not any(bool(torch.isnan(v).any()) for v in o.values() if v is not None), what
    assert all(v <= TOL for v in e.values()), (what, e)


@functools.lru_cache(maxsize=None)
def _inputs(B, D, pairs='random'):
    """Unit rows a, b [B, D] and group ids in [0, 4) (shared by the tests; never modified).  'correlated':
    b = normalize(a + 0.3·randn), so the diagonal dominates and sits in a different tile for every strip."""
    g = torch.Generator().manual_seed(1000 * B + D)
    a = F.normalize(torch.randn(B, D, generator=g).double(), dim=1).float()
    r = torch.randn(B, D, generator=g)
    b = F.normalize((a + 0.3 * r if pairs == 'correlated' else r).double(), dim=1).float()
    ids = torch.randint(0, 4, (B,), generator=g)
    return a.to(DEV), b.to(DEV), ids.to(DEV)


def _t(scale):
    return torch.tensor([math.log(scale)], device=DEV)


@pytest.mark.parametrize('sg', [0, 1, 2], ids=MODES)
@pytest.mark.parametrize('scale', SCALES, ids=SCALE_IDS)
@pytest.mark.parametrize('pairs', ['random', 'correlated'])
@pytest.mark.parametrize('B,D', SHAPES)
def test_values_and_gradients(B, D, pairs, scale, sg):
    a, b, ids = _inputs(B, D, pairs)
    t = _t(scale)
    _check(_raw(a, b, t, ids, sg), _ref64(a, b, t, ids, sg), f'B={B} D={D} {pairs} e^t={scale:.3g} {MODES[sg]}')


def test_no_ids_is_plain_clip():
    """Without ids every off-diagonal pair is a negative, whatever same_group says; with ids, same_group 0 is the same."""
    a, b, ids = _inputs(65, 128)
    t = _t(SCALES[0])
    plain = _raw(a, b, t)
    for other in (_raw(a, b, t, None, 2), _raw(a, b, t, ids, 0)):
        assert all(torch.equal(plain[k], other[k]) for k in plain)
    _check(plain, _ref64(a, b, t), 'B=65 D=128 no ids')


@pytest.mark.parametrize('case', ['B1', 'all-one-group-ignored'])
def test_degenerate_cases_are_exactly_zero(case):
    """One pair, or every off-diagonal pair ignored: each softmax has one term, the loss and every gradient are 0 in
    fp64 and must be exactly 0 here (no relative error exists)."""
    if case == 'B1':
        a, b, _ = _inputs(1, 32)
        ids, sg = None, 0
    else:
        a, b, _ = _inputs(130, 64, 'correlated')
        ids, sg = torch.zeros(130, dtype=torch.int64, device=DEV), 1
    t = _t(SCALES[0])
    r = _ref64(a, b, t, ids, sg)
    assert r['loss'].item() == 0 and not r['da'].any() and not r['db'].any() and r['gt'].item() == 0
    o = _raw(a, b, t, ids, sg)
    assert all(bool((v == 0).all()) for v in o.values()), o


@pytest.mark.parametrize('sg', [1, 2], ids=['ignore', 'positive'])
def test_fully_masked_tiles(sg):
    """ids[:80] = 0, the rest distinct: under 'ignore' rows 64..79 have their whole first tile of 64 columns masked (the
    running max is still −∞ when the second tile starts), rows 0..63 all of it but the diagonal."""
    B, D = 130, 64
    a, b, _ = _inputs(B, D, 'correlated')
    ids = torch.arange(B, device=DEV)
    ids[:80] = 0
    t = _t(SCALES[0])
    _check(_raw(a, b, t, ids, sg), _ref64(a, b, t, ids, sg), f'B=130 D=64 ids[:80]=0 {MODES[sg]}')


@pytest.mark.parametrize('B,D', [(65, 128), (257, 256)])
def test_unnormalised_rows(B, D):
    """a = 30·randn/√D against unit b at e^t = 1/0.07: max|S| is far above 88.7, where expf overflows without the
    running max."""
    g = torch.Generator().manual_seed(7 * B + D)
    a = (30 * torch.randn(B, D, generator=g) / math.sqrt(D)).to(DEV)
    _, b, ids = _inputs(B, D)
    t = _t(SCALES[0])
    smax = ((a.double() @ b.double().T) * t.double().exp()).abs().max().item()
    print(f'max|S| = {smax:.1f}')
    assert smax > 88.7
    for sg in (0, 1, 2):
        o = _raw(a, b, t, ids, sg)
        assert all(bool(torch.isfinite(v).all()) for v in o.values())
        _check(o, _ref64(a, b, t, ids, sg), f'B={B} D={D} unnormalised {MODES[sg]}')


@pytest.mark.parametrize('B,D,width,first', [(70, 256, 320, 32), (33, 100, 103, 1), (33, 30, 30, 0)],
                         ids=['lda320-aligned', 'D100-misaligned', 'D30-odd-stride'])
def test_strided_rows(B, D, width, first):
    """One operand is a column slice of a wider tensor; rows that are not 16-byte aligned take the scalar staging path.
    The values must be those of the contiguous copy, to the bit, and right against fp64; on either side."""
    g = torch.Generator().manual_seed(B + D)
    wide = torch.randn(B, width, generator=g).to(DEV)
    wide[:, first:first + D] = F.normalize(wide[:, first:first + D], dim=1)
    x = wide[:, first:first + D]
    assert x.stride(0) == width and x.data_ptr() == wide.data_ptr() + 4 * first
    _, y, ids = _inputs(B, D)
    t = _t(SCALES[0])
    for a, b in ((x, y), (y, x)):
        o = _raw(a, b, t, ids, 1)
        _check(o, _ref64(a, b, t, ids, 1), f'B={B} D={D} strided {"a" if a is x else "b"}')
        c = _raw(a.contiguous(), b.contiguous(), t, ids, 1)
        assert all(torch.equal(o[k], c[k]) for k in o)


def test_beyond_the_composites_comfort():
    """B = 1500: the matrix is never stored; the workspace is O(B) (stated, not measured: below 64 MiB at the largest
    shape, where the matrix alone would be 4 GiB)."""
    B, D = 1500, 32
    a, b, ids = _inputs(B, D)
    t = _t(SCALES[0])
    _check(_raw(a, b, t, ids, 1), _ref64(a, b, t, ids, 1), 'B=1500 D=32 ignore')
    assert 0 < L().lib().cmhar_softmax_contrast_ws(32768, 256) < 64 << 20


@pytest.mark.parametrize('B', [8160, 8200], ids=['last-16-row-strips', 'first-32-row-strips'])
def test_wide_strips(B):
    """From 512 strips of 32 rows on (both sides together) a workgroup owns 32 rows instead of 16: values against fp64
    on both sides of that threshold, and shards cut at rows that are no multiple of 32."""
    D = 40
    a, b, ids = _inputs(B, D)
    t = _t(SCALES[0])
    full = _raw(a, b, t, ids, 1)
    _check(full, _ref64(a, b, t, ids, 1), f'B={B} D={D} ignore')
    s = _raw(a, b, t, ids, 1, (1001, 77), (2037, 150))
    assert torch.equal(s['da'], full['da'][1001:1078]) and torch.equal(s['db'], full['db'][2037:2187])
    assert all(torch.equal(s[k], full[k]) for k in ('loss', 'gt'))


def test_reference_parity_on_g7():
    """The reference's InfoNCELoss(temperature=0.07) fixture, with the bounds of test_g7_losses_match_reference."""
    import numpy as np
    from fixtures import load
    from cmhar.losses import SoftmaxContrastiveLoss
    fx = load('g7_losses')
    a = torch.tensor(fx['nce_a'], device=DEV).requires_grad_(True)
    b = torch.tensor(fx['nce_b'], device=DEV).requires_grad_(True)
    loss = SoftmaxContrastiveLoss(init_temperature=1 / 0.07, learnable=False, group=False)(a, b)
    loss.backward()
    assert loss.item() == pytest.approx(float(fx['nce_loss']), rel=1e-5)
    np.testing.assert_allclose(a.grad.cpu().numpy(), np.asarray(fx['nce_grad_a']), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(b.grad.cpu().numpy(), np.asarray(fx['nce_grad_b']), rtol=1e-4, atol=1e-6)


def test_agrees_with_infonce_loss():
    from cmhar.losses import InfoNCELoss, SoftmaxContrastiveLoss
    a, b, _ = _inputs(257, 256, 'correlated')
    out = []
    for lf in (SoftmaxContrastiveLoss(init_temperature=1 / 0.07, learnable=False, group=False).to(DEV),
               InfoNCELoss(0.07)):
        ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        loss = lf(ar, br)
        loss.backward()
        out.append((loss.detach(), ar.grad, br.grad))
    e = [rel(x, y) for x, y in zip(*out)]
    print('softmax_contrast vs InfoNCELoss: loss %.2e da %.2e db %.2e' % tuple(e))
    assert all(v <= TOL for v in e), e


# ---------------------------------------------------------------------------------------------------------------
# exact comparisons
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,D', SHAPES)
def test_shard_invariance_and_determinism(B, D):
    """The two data-parallel shards (rows [0, ⌈B/2⌉) and the rest) give the full run's gradient rows, loss and gt to
    the bit; so does a second full run."""
    a, b, ids = _inputs(B, D, 'correlated')
    t = _t(SCALES[0])
    h = (B + 1) // 2
    for sg in (0, 1, 2):
        full = _raw(a, b, t, ids, sg)
        again = _raw(a, b, t, ids, sg)
        assert all(torch.equal(full[k], again[k]) for k in full), sg
        assert not any(bool(torch.isnan(v).any()) for v in full.values())
        for off, cnt in ((0, h), (h, B - h)):
            s = _raw(a, b, t, ids, sg, (off, cnt), (off, cnt))
            assert torch.equal(s['da'], full['da'][off:off + cnt]) and torch.equal(s['db'], full['db'][off:off + cnt])
            assert all(torch.equal(s[k], full[k]) for k in ('loss', 'gt'))


def test_uneven_shards():
    a, b, ids = _inputs(257, 256)
    t = _t(SCALES[0])
    for sg in (0, 1, 2):
        full = _raw(a, b, t, ids, sg)
        s = _raw(a, b, t, ids, sg, (101, 77), (37, 150))
        assert torch.equal(s['da'], full['da'][101:178]) and torch.equal(s['db'], full['db'][37:187])
        assert all(torch.equal(s[k], full[k]) for k in ('loss', 'gt'))


@pytest.mark.parametrize('B,D', [(17, 36), (130, 1024), (257, 256)])
def test_null_outputs(B, D):
    a, b, ids = _inputs(B, D)
    t = _t(SCALES[0])
    full = _raw(a, b, t, ids, 1)
    none = _raw(a, b, t, ids, 1, want=())
    assert torch.equal(none['loss'], full['loss'])
    nodb = _raw(a, b, t, ids, 1, want=('da', 'gt'))
    assert all(torch.equal(nodb[k], full[k]) for k in ('loss', 'da', 'gt'))


@pytest.mark.parametrize('B,D,sg', [(2, 1056, 0), (32769, 1, 0), (4, 32, 3)], ids=['D1056', 'B32769', 'same_group3'])
def test_rejections_write_nothing(B, D, sg):
    a, b = torch.zeros(B, D, device=DEV), torch.zeros(B, D, device=DEV)
    ids = torch.zeros(B, dtype=torch.int64, device=DEV)
    code, o = _raw(a, b, _t(1.0), ids, sg, rc=True)
    assert code == -1
    assert all(bool(torch.isnan(v).all()) for v in o.values())


# ---------------------------------------------------------------------------------------------------------------
# module
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('same_group', MODES)
def test_module_matches_raw_call(same_group):
    from cmhar.losses import SoftmaxContrastiveLoss
    B, D = 65, 128
    a, b, ids = _inputs(B, D)
    sg = MODES.index(same_group)
    lf = SoftmaxContrastiveLoss(same_group=same_group, group=False)         # the parameter stays on the CPU
    raw = _raw(a, b, torch.tensor([lf.temperature.item()], device=DEV), ids, sg)
    for scale in (1.0, 3.0):
        ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        lf.zero_grad(set_to_none=True)
        loss = lf(ar, br, labels=ids.cpu() if scale == 1.0 else ids)        # host or device ids
        assert loss.shape == () and loss.device.type == 'cuda'
        assert torch.equal(loss.reshape(1), raw['loss'])
        (loss * scale).backward()
        assert torch.equal(ar.grad, raw['da'] * scale) and torch.equal(br.grad, raw['db'] * scale)
        assert lf.temperature.grad.device.type == 'cpu'
        assert torch.equal(lf.temperature.grad.reshape(1), (raw['gt'] * scale).cpu())
    with torch.no_grad():
        assert torch.equal(lf(a, b, labels=ids).reshape(1), raw['loss'])
    fz = SoftmaxContrastiveLoss(same_group=same_group, learnable=False, group=False).to(DEV)
    assert torch.equal(fz(a, b, labels=ids).reshape(1), raw['loss'])        # nothing requires grad: the NULL path


def test_no_grad_path_passes_null_gradients(monkeypatch):
    """Under no_grad (and when nothing requires grad) the three gradient pointers are NULL: pass 2 does not run."""
    from cmhar import losses
    a, b, _ = _inputs(17, 36)
    seen = []
    real = losses.L.call

    def spy(name, *args):
        seen.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(losses.L, 'call', spy)
    lf = losses.SoftmaxContrastiveLoss(group=False)
    with torch.no_grad():
        lf(a, b)
    lf(a, b).backward()
    (n0, a0), (n1, a1) = seen
    assert n0 == n1 == 'cmhar_softmax_contrast_loss'
    grads = lambda args: (args[10], args[13], args[16])                      # da, db, gt
    assert grads(a0) == (None, None, None)
    assert all(p is not None for p in grads(a1))


def test_two_ranks_contrast_over_the_global_batch(tmp_path):
    """`group=`: two ranks (gloo, sharing the one GPU; tests/softmax_contrast_dp_worker.py) each give their shard of a
    130-pair batch with its ids; every rank's loss and temperature gradient are the single-process full-batch ones and
    its gradient rows are that run's rows, to the bit."""
    import os
    import socket
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK='0', WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), CMHAR_SMC_OUT=str(tmp_path), CMHAR_SMC_MODE='positive')
        worker = os.path.join(repo, 'tests', 'softmax_contrast_dp_worker.py')
        procs.append(subprocess.Popen([sys.executable, '-u', worker], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    for p in procs:
        try:
            out, _ = p.communicate(timeout=100)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert p.returncode == 0, out.decode(errors='replace')[-4000:]
    full = torch.load(tmp_path / 'full.pt')
    assert math.isfinite(full['loss'].item()) and full['gt'].item() != 0
    for r in range(2):
        o = torch.load(tmp_path / f'rank{r}.pt')
        assert torch.equal(o['loss'], full['loss']) and torch.equal(o['gt'], full['gt'])
        assert torch.equal(o['da'], full['da'][65 * r:65 * r + 65])
        assert torch.equal(o['db'], full['db'][65 * r:65 * r + 65])


# ---------------------------------------------------------------------------------------------------------------
# it actually contrasts
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_toy_problem_learns_to_retrieve(seed):
    """The toy problem of tests/test_pair_sigmoid_gpu.py: 64 pairs from a shared 16-d latent, two linear encoders
    (48 -> 32, 40 -> 32, 0.1·randn), torch Adam lr 1e-2, 100 steps on the GPU kernel's loss: recall@1 >= 0.95 both ways
    (the fp32 CPU formula reaches 1.0 for the three seeds; the temperature moves by about 0.1, e^t ends near 15.7)."""
    from cmhar.losses import SoftmaxContrastiveLoss
    from cmhar.retrieval import recall_at_k
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(64, 16, generator=g)
    x = (z @ torch.randn(16, 48, generator=g)).to(DEV)
    y = (z @ torch.randn(16, 40, generator=g)).to(DEV)
    Wa = (0.1 * torch.randn(48, 32, generator=g)).to(DEV).requires_grad_(True)
    Wb = (0.1 * torch.randn(40, 32, generator=g)).to(DEV).requires_grad_(True)
    lf = SoftmaxContrastiveLoss(group=False).to(DEV)
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
# trainer (its code is unchanged)
# ---------------------------------------------------------------------------------------------------------------
def test_trainer_trains_temperature_and_passes_labels():
    from fixtures import fixture_config, fixture_state_dict, load
    from cmhar import models
    from cmhar.losses import SoftmaxContrastiveLoss
    from cmhar.trainer import CrossModalTrainer
    fx = load('g2_crossmodal_tiny')
    cfg = fixture_config(fx)
    cfg.model.compute_dtype = 'fp32'
    torch.manual_seed(0)
    m = models.CrossModalModel(cfg)
    m.load_state_dict(fixture_state_dict(fx), strict=True)
    batches = [{'imu': torch.tensor(fx['imu']), 'video': torch.tensor(fx['video'])},
               {'imu': torch.tensor(fx['step_imu2']), 'video': torch.tensor(fx['step_video2'])}]
    for i, bt in enumerate(batches):
        bt['label'] = (torch.arange(bt['imu'].shape[0]) + i) % 2
    seen = []

    class Spy(SoftmaxContrastiveLoss):
        def forward(self, a, b, labels=None):
            seen.append(labels)
            return super().forward(a, b, labels)
    lf = Spy(same_group='positive')
    t0 = lf.temperature.item()
    tr = CrossModalTrainer(m, lf, cfg, device=DEV, train_loss_params=True)
    assert lf.temperature.is_cuda
    groups = tr.optimizer.param_groups
    assert len(groups) == 2 and groups[1]['weight_decay'] == 0
    assert [id(p) for p in groups[1]['params']] == [id(lf.temperature)]
    for bt in batches:
        loss = tr.train_step(*tr._batch(bt), labels=tr._labels(bt))
        assert math.isfinite(loss.item())
    assert len(seen) == 2 and all(torch.equal(s.cpu(), bt['label']) for s, bt in zip(seen, batches))
    assert lf.temperature.item() != t0
