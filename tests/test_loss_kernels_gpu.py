"""Loss kernels (csrc/loss.hip) against fp64 references: `cmhar_siglip_loss` called directly (sizes, saturated logits,
the shard arguments) and the cross-entropy family through `cmhar.kernels.cross_entropy` (plain, label-smoothed,
focal; every reduction; upstream gradients; ignored rows; accumulation; transposed views; argmax ties; masked, -inf
logits).  Companion of tests/test_rowops_gpu.py, whose conventions it shares.

References are fp64 torch: autograd of `oracle/cpu_model.py`'s restatements of the reference's losses (and of
`F.cross_entropy` where a logit is -inf, which the restatement's explicit smoothing term does not take).  Tolerances
are the project's fp32 bound, `rel(a, b) = ‖a−b‖/‖b‖ ≤ 1e-5`; the SigLIP temperature gradient, a cancelling sum, is
measured against the fp64 sum of its terms' magnitudes, `≤ 1e-5`.  Integer outputs, shard-against-full comparisons
and gradients that must be zero are compared exactly.  Outputs are prefilled with NaN / an integer sentinel."""
import math

import pytest
import torch
import torch.nn.functional as F

DEV = 'cuda'
pytestmark = pytest.mark.gpu
NAN = float('nan')
IGNORE = -100


def K():
    from cmhar import kernels
    return kernels


def L():
    from cmhar import _lib
    return _lib


def O():
    from oracle import cpu_model
    return cpu_model


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def nans(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


# ---------------------------------------------------------------------------------------------------------------
# SigLIP
# ---------------------------------------------------------------------------------------------------------------
def _siglip(a, b, t, bias, a_off, a_cnt, b_off, b_cnt):
    """cmhar_siglip_loss over NaN-filled outputs: (loss, da [a_cnt, D], db [b_cnt, D], gt, gbias)."""
    Ba, D = a.shape
    Bb = b.shape[0]
    loss, gt, gb = nans(1), nans(1), nans(1)
    da, db = nans(a_cnt, D), nans(b_cnt, D)
    ws = K().workspace(L().lib().cmhar_siglip_ws(Ba, Bb), a.device)
    L().call('cmhar_siglip_loss', Ba, Bb, D, a.data_ptr(), b.data_ptr(), t.data_ptr(), bias.data_ptr(),
             loss.data_ptr(), da.data_ptr(), a_off, a_cnt, db.data_ptr(), b_off, b_cnt, gt.data_ptr(), gb.data_ptr(),
             ws.data_ptr(), L().stream(a.device))
    return loss, da, db, gt, gb


def _unit_rows(B, D, seed):
    g = torch.Generator().manual_seed(seed)
    return (F.normalize(torch.randn(B, D, generator=g).double(), dim=1).float().to(DEV),
            F.normalize(torch.randn(B, D, generator=g).double(), dim=1).float().to(DEV))


@pytest.mark.parametrize('t,bias', [(math.log(10.0), -10.0), (math.log(100.0), -5.0), (0.0, 0.0)],
                         ids=['t10-b10', 't100-b5-saturated', 't1-b0'])
@pytest.mark.parametrize('B,D', [(1, 32), (5, 100), (67, 128), (130, 1024)])
def test_siglip(B, D, t, bias):
    """Loss and all gradients against fp64 autograd; then the two data-parallel shards (rows [0, ⌈B/2⌉) and the rest),
    whose gradient rows, loss, gt and gbias must be the full run's bits.  B = 1: the second shard has a_cnt = b_cnt =
    0.  (ln 100, −5) gives logits up to ±100 (saturated sigmoid)."""
    a, b = _unit_rows(B, D, 10 * B + D)
    tt, bb = torch.tensor([t], device=DEV), torch.tensor([bias], device=DEV)
    loss, da, db, gt, gb = _siglip(a, b, tt, bb, 0, B, 0, B)
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    t64, c64 = tt.double().requires_grad_(True), bb.double().requires_grad_(True)
    dots = a64 @ b64.T
    S = dots * t64.exp() + c64
    lab = 2 * torch.eye(B, dtype=torch.float64, device=DEV) - 1
    ref = F.binary_cross_entropy_with_logits(S * lab, (lab + 1) / 2, reduction='mean')      # oracle.siglip_loss
    ga, gbv, gtt, gc, gS = torch.autograd.grad(ref, (a64, b64, t64, c64, S))
    mag_t = (gS * dots.detach() * t64.detach().exp()).abs().sum()                           # Σ |dS_ij · dot_ij · e^t|
    e = dict(loss=rel(loss, ref.detach()), da=rel(da, ga), db=rel(db, gbv), gbias=rel(gb, gc),
             gt=(abs(gt.item() - gtt.item()) / max(mag_t.item(), 1e-300)))
    print(f'siglip B={B} D={D} t={t:.3f} bias={bias}: ' + ' '.join(f'{k} {v:.2e}' for k, v in e.items()))
    assert all(v <= 1e-5 for v in e.values()), e
    h = (B + 1) // 2
    for off, cnt in ((0, h), (h, B - h)):
        l2, da2, db2, gt2, gb2 = _siglip(a, b, tt, bb, off, cnt, off, cnt)
        assert torch.equal(da2, da[off:off + cnt]) and torch.equal(db2, db[off:off + cnt])
        assert torch.equal(l2, loss) and torch.equal(gt2, gt) and torch.equal(gb2, gb)


def test_siglip_no_b_rows():
    """b_cnt = 0 (a rank that owns no rows of b): accepted, the other outputs as in the full run."""
    a, b = _unit_rows(5, 100, 1)
    tt, bb = torch.tensor([math.log(10.0)], device=DEV), torch.tensor([-10.0], device=DEV)
    full = _siglip(a, b, tt, bb, 0, 5, 0, 5)
    part = _siglip(a, b, tt, bb, 0, 5, 0, 0)
    assert part[2].numel() == 0
    for i in (0, 1, 3, 4):
        assert torch.equal(part[i], full[i])


@pytest.mark.parametrize('Ba,Bb,D', [(2, 2, 1056), (1, 1025, 32)], ids=['D>1024', 'Bb>1024'])
def test_siglip_rejects_oversize(Ba, Bb, D):
    a, b = torch.zeros(Ba, D, device=DEV), torch.zeros(Bb, D, device=DEV)
    tt, bb = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    loss, da, db = torch.full((1,), 3.0, device=DEV), torch.full((Ba, D), 3.0, device=DEV), torch.full((Bb, D), 3.0, device=DEV)
    ws = K().workspace(L().lib().cmhar_siglip_ws(Ba, Bb), a.device)
    rc = L().lib().cmhar_siglip_loss(Ba, Bb, D, a.data_ptr(), b.data_ptr(), tt.data_ptr(), bb.data_ptr(),
                                     loss.data_ptr(), da.data_ptr(), 0, Ba, db.data_ptr(), 0, Bb, None, None,
                                     ws.data_ptr(), L().stream(a.device))
    torch.cuda.synchronize()
    assert rc == -1
    assert loss.item() == 3.0 and bool((da == 3.0).all()) and bool((db == 3.0).all())


# ---------------------------------------------------------------------------------------------------------------
# cross-entropy family
# ---------------------------------------------------------------------------------------------------------------
VARIANTS = {'plain': dict(), 'smooth0.1': dict(label_smoothing=0.1), 'focal-g2-a0.5': dict(gamma=2.0, alpha=0.5),
            'focal-g0.5-a1': dict(gamma=0.5, alpha=1.0), 'focal-g1-a0.25': dict(gamma=1.0, alpha=0.25)}


def _row_losses64(z64, y, kw):
    """Per-row fp64 losses from oracle/cpu_model.py's formulas; ignored rows contribute 0."""
    keep = y != IGNORE
    v = torch.zeros(z64.shape[0], dtype=torch.float64, device=z64.device)
    if bool(keep.any()):
        if kw.get('gamma', 0.0) != 0.0:
            vk = O().focal_loss(z64[keep], y[keep], alpha=kw['alpha'], gamma=kw['gamma'], reduction='none')
        else:
            vk = O().cross_entropy(z64[keep], y[keep], 'none', label_smoothing=kw.get('label_smoothing', 0.0))
        v = v.index_put((keep.nonzero().squeeze(1),), vk)
    return v, keep


def _reduce64(v, keep, reduction):
    return v if reduction == 'none' else v.sum() if reduction == 'sum' else v.sum() / keep.sum()


def _transposed(t):
    """The same matrix stored column-major: strides (1, rows)."""
    return t.t().contiguous().t()


def _ce_call(z, y, kw, reduction, *, g_up, dz, grad_scale=1.0, grad_beta=0.0):
    N = z.shape[0]
    out = dict(loss=nans(1), row_loss=nans(N), pred=torch.full((N,), -7, dtype=torch.int64, device=DEV),
               correct=torch.full((1,), -7, dtype=torch.int32, device=DEV),
               status=torch.full((1,), -7, dtype=torch.int32, device=DEV))
    K().cross_entropy(z, y, ignore_index=IGNORE, reduction=reduction, dlogits=dz, grad_scale=grad_scale,
                      grad_beta=grad_beta, g_up=g_up, **out, **kw)
    return out


@pytest.mark.parametrize('scale', [1.0, 10.0], ids=['scale1', 'scale10'])
@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('N,C', [(1, 2), (5, 64), (37, 65), (70, 300), (300, 11)])
def test_cross_entropy_family(N, C, variant, scale):
    """Each loss × reduction ('none' with per-row upstream gradients, 'mean' / 'sum' with a scalar one) × (overwrite,
    grad_beta = 1 accumulation with grad_scale = 0.5) × (row-major, transposed logit and gradient views); every 7th
    label is ignore_index.  C = 2, 11: lanes without a column; 64 / 65: the wave boundary; 300: five strides."""
    kw = VARIANTS[variant]
    g = torch.Generator().manual_seed(1000 * N + C)
    z = (scale * torch.randn(N, C, generator=g)).to(DEV)
    y = torch.randint(0, C, (N,), generator=g).to(DEV)
    y[6::7] = IGNORE
    old = torch.randn(N, C, generator=g).to(DEV)
    g_rows, g_one = torch.randn(N, generator=g).to(DEV), torch.tensor([0.7], device=DEV)
    want_pred = torch.argmax(z.cpu(), dim=1)
    want_correct = int((want_pred == y.cpu()).sum())
    worst = 0.0
    for reduction in ('none', 'mean', 'sum'):
        g_up = g_rows if reduction == 'none' else g_one
        z64 = z.double().requires_grad_(True)
        v, keep = _row_losses64(z64, y, kw)
        ref = _reduce64(v, keep, reduction)
        (gz,) = torch.autograd.grad((ref * g_up.double()).sum(), z64)
        for tr in (False, True):
            zz = _transposed(z) if tr else z
            for grad_beta, grad_scale in ((0.0, 1.0), (1.0, 0.5)):
                dz = old.clone() if grad_beta else nans(N, C)
                dz = _transposed(dz) if tr else dz
                out = _ce_call(zz, y, kw, reduction, g_up=g_up, dz=dz, grad_scale=grad_scale, grad_beta=grad_beta)
                el = rel(out['row_loss'], v.detach())
                if reduction != 'none':
                    el = max(el, rel(out['loss'], ref.detach()))
                eg = rel(dz, grad_beta * old.double() + grad_scale * gz)
                worst = max(worst, el, eg)
                assert el <= 1e-5 and eg <= 1e-5, (reduction, tr, grad_beta, el, eg)
                assert torch.equal(out['pred'].cpu(), want_pred)
                assert out['correct'].item() == want_correct and out['status'].item() == 0
    print(f'xent {variant} N={N} C={C} scale={scale}: worst rel {worst:.2e}')


def test_cross_entropy_argmax_ties():
    """Rows whose maximum appears twice: in different 64-column strides and lanes (5 | 70, 64 | 3, 0 | 199), in
    neighbouring lanes (130 | 131, 63 | 64) and twice in one lane (5 | 69).  pred is the first maximum, as
    torch.argmax of the same fp32 tensor; correct counts the rows whose label is that index."""
    pairs = [(5, 70), (64, 3), (130, 131), (0, 199), (63, 64), (5, 69), (127, 1), (199, 198)]
    C = 200
    g = torch.Generator().manual_seed(4)
    z = torch.randn(2 * len(pairs), C, generator=g)
    y = torch.empty(2 * len(pairs), dtype=torch.int64)
    for i, (p, q) in enumerate(pairs):
        for r, lab in ((2 * i, min(p, q)), (2 * i + 1, max(p, q))):
            z[r, p] = z[r, q] = 9.0
            y[r] = lab
    want = torch.argmax(z, dim=1)
    assert want.tolist() == [min(p) for p in pairs for _ in range(2)]
    for tr in (False, True):
        zz = _transposed(z.to(DEV)) if tr else z.to(DEV)
        out = _ce_call(zz, y.to(DEV), {}, 'mean', g_up=None, dz=None)
        assert torch.equal(out['pred'].cpu(), want)
        assert out['correct'].item() == len(pairs)


@pytest.mark.parametrize('grad_beta', [0.0, 1.0])
def test_cross_entropy_all_rows_ignored(grad_beta):
    """'mean' over no rows: the loss is NaN as documented (torch's mean of nothing); the gradient is exactly zero, or
    grad_beta · old."""
    N, C = 9, 70
    g = torch.Generator().manual_seed(8)
    z = torch.randn(N, C, generator=g).to(DEV)
    y = torch.full((N,), IGNORE, dtype=torch.int64, device=DEV)
    old = torch.randn(N, C, generator=g).to(DEV)
    dz = old.clone() if grad_beta else nans(N, C)
    out = _ce_call(z, y, {}, 'mean', g_up=None, dz=dz, grad_beta=grad_beta)
    assert math.isnan(out['loss'].item())
    assert torch.equal(dz, old if grad_beta else torch.zeros_like(dz))
    assert bool((out['row_loss'] == 0).all()) and out['correct'].item() == 0 and out['status'].item() == 0
    assert torch.equal(out['pred'].cpu(), torch.argmax(z.cpu(), dim=1))


@pytest.mark.parametrize('variant', ['plain', 'focal-g2-a0.5'])
@pytest.mark.parametrize('reduction', ['none', 'mean', 'sum'])
def test_cross_entropy_masked_class(variant, reduction):
    """One -inf column outside every target, no label smoothing: loss and gradients are finite and equal fp64
    F.cross_entropy (NaN before the smoothing term was made conditional on label_smoothing != 0)."""
    kw = VARIANTS[variant]
    N, C, dead = 37, 65, 17
    g = torch.Generator().manual_seed(6)
    z = (3 * torch.randn(N, C, generator=g)).to(DEV)
    z[:, dead] = -float('inf')
    y = torch.randint(0, C - 1, (N,), generator=g).to(DEV)
    y[y >= dead] += 1
    g_up = torch.randn(N, generator=g).to(DEV) if reduction == 'none' else torch.tensor([0.7], device=DEV)
    z64 = z.double().requires_grad_(True)
    ce = F.cross_entropy(z64, y, reduction='none')
    v = kw['alpha'] * (1 - torch.exp(-ce)) ** kw['gamma'] * ce if kw else ce
    ref = v if reduction == 'none' else v.sum() if reduction == 'sum' else v.mean()
    (gz,) = torch.autograd.grad((ref * g_up.double()).sum(), z64)
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(gz).all())
    dz = nans(N, C)
    out = _ce_call(z, y, kw, reduction, g_up=g_up, dz=dz)
    el = rel(out['row_loss'], v.detach()) if reduction == 'none' else rel(out['loss'], ref.detach())
    eg = rel(dz, gz)
    print(f'xent masked class {variant} {reduction}: loss {el:.2e} grad {eg:.2e}')
    assert bool(torch.isfinite(out['row_loss']).all()) and bool(torch.isfinite(dz).all())
    assert el <= 1e-5 and eg <= 1e-5
    assert bool((dz[:, dead] == 0).all())
    assert torch.equal(out['pred'].cpu(), torch.argmax(z.cpu(), dim=1))


def test_cross_entropy_rejects_focal_with_smoothing():
    z = torch.zeros(4, 8, device=DEV)
    y = torch.zeros(4, dtype=torch.int64, device=DEV)
    loss = torch.full((1,), 3.0, device=DEV)
    with pytest.raises(RuntimeError):
        K().cross_entropy(z, y, label_smoothing=0.1, gamma=2.0, loss=loss)
    torch.cuda.synchronize()
    assert loss.item() == 3.0
