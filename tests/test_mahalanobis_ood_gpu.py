"""`cmhar.ood.MahalanobisDetector` / `MahalanobisOODEvaluator` on the class-moment and class-distance kernels.

The data are anisotropic on purpose: 8 loud and 56 quiet directions, OOD rows shifted inside the quiet subspace, so
that the Euclidean nearest-class-mean score sees nothing (AUROC ~0.5) and only a score that whitens separates them.
The detector is checked against an fp64 restatement of the whole pipeline written here, with the same pipeline in
fp32 on the CPU as the yardstick for its error."""
import functools

import numpy as np
import pytest
import torch

DEV = 'cuda'
pytestmark = pytest.mark.gpu


def _gauss_data(C, d, n_train, n_in, n_out, seed=5):
    """C class means 2·N(0, I), shared covariance Q diag(s²) Qᵀ with s = 6 on 8 directions and 0.3 on the rest, rows
    assigned round-robin; OOD rows are in-distribution rows shifted by a vector of norm 3 inside the quiet subspace."""
    g = torch.Generator().manual_seed(seed)
    mu = 2 * torch.randn(C, d, generator=g, dtype=torch.float64)
    Q, _ = torch.linalg.qr(torch.randn(d, d, generator=g, dtype=torch.float64))
    s = torch.full((d,), 0.3, dtype=torch.float64)
    s[:8] = 6.0

    def draw(n):
        y = torch.arange(n) % C
        return mu[y] + (torch.randn(n, d, generator=g, dtype=torch.float64) * s) @ Q.T, y
    (train, ytrain), (x_in, y_in), (x_out, y_out) = draw(n_train), draw(n_in), draw(n_out)
    v = torch.randn(n_out, d - 8, generator=g, dtype=torch.float64) @ Q[:, 8:].T
    x_out = x_out + 3.0 * v / v.norm(dim=1, keepdim=True)
    return train.float(), ytrain, x_in.float(), y_in, x_out.float(), y_out


@functools.lru_cache(maxsize=None)
def _data():
    return _gauss_data(8, 64, 1600, 400, 400)


def _pipeline(train, y, xs, dtype, shrinkage=0.0, relative=False):
    """The detector restated with torch on the CPU in `dtype`: (scores, arg-min classes) for each x of xs."""
    tr = train.to(dtype)
    classes = torch.unique(y)
    n, d = tr.shape

    def gaussian(labels, cls):
        means = torch.stack([tr[labels == c].mean(0) for c in cls])
        R = tr - means[torch.searchsorted(cls, labels)]
        cov = R.T @ R / n
        if shrinkage > 0:
            cov = (1 - shrinkage) * cov + shrinkage * (torch.trace(cov) / d) * torch.eye(d, dtype=dtype)
        W = torch.linalg.solve_triangular(torch.linalg.cholesky(cov), torch.eye(d, dtype=dtype), upper=False)
        return W, means @ W.T

    W, wm = gaussian(y, classes)
    if relative:
        W0, wm0 = gaussian(torch.zeros_like(y), torch.zeros(1, dtype=y.dtype))
    out = []
    for x in xs:
        z = x.to(dtype) @ W.T
        d2, cls = torch.stack([((z - wm[c]) ** 2).sum(1) for c in range(len(classes))], 1).min(1)
        if relative:
            d2 = d2 - ((x.to(dtype) @ W0.T - wm0[0]) ** 2).sum(1)
        out.append((-d2, classes[cls]))
    return out


def _err(s, want):
    return ((s.double() - want).abs().max() / want.abs().max()).item()


def test_detector_separates_where_euclid_cannot():
    from cmhar.ood import MahalanobisDetector, auroc
    train, y, x_in, y_in, x_out, _ = _data()
    (r_in, rc_in), (r_out, _) = _pipeline(train, y, (x_in, x_out), torch.float64)
    assert auroc(r_in.numpy(), r_out.numpy()) > 0.99 and torch.equal(rc_in, y_in)     # the fp64 reference
    mu = torch.stack([train[y == c].double().mean(0) for c in range(8)])
    e_in, e_out = (-(torch.cdist(x.double(), mu) ** 2).min(1).values for x in (x_in, x_out))
    assert auroc(e_in.numpy(), e_out.numpy()) < 0.6                                   # the Euclidean score is blind

    det = MahalanobisDetector()
    assert det.fit(train.to(DEV), y) is det
    assert det.classes_.tolist() == list(range(8)) and det.counts_.tolist() == [200] * 8
    assert det.means_.shape == (8, 64) and det.covariance_.shape == (64, 64) and det.whitening_.shape == (64, 64)
    assert all(t.dtype == torch.float32 and t.is_cuda for t in (det.means_, det.covariance_, det.whitening_))
    s_in, c_in = det.predict(x_in.to(DEV))
    s_out = det.score(x_out.to(DEV))
    assert s_in.dtype == torch.float32 and s_in.shape == (400,) and c_in.dtype == torch.int64
    assert auroc(s_in.cpu().numpy(), s_out.cpu().numpy()) > 0.99
    assert torch.equal(c_in.cpu(), y_in)
    assert torch.equal(s_in, det.score(x_in.to(DEV)))
    dall = det.distances(x_in.to(DEV))
    assert dall.shape == (400, 8) and torch.equal(dall.min(1).values, -s_in)
    w, cov = det.whitening_.double().cpu(), det.covariance_.double().cpu()
    assert (w @ cov @ w.T - torch.eye(64, dtype=torch.float64)).abs().max().item() < 1e-3

    # against the fp64 restatement, with the fp32 restatement's error as the yardstick
    (f_in, _), (f_out, _) = _pipeline(train, y, (x_in, x_out), torch.float32)
    for got, want, f32 in ((s_in, r_in, f_in), (s_out, r_out, f_out)):
        print(f'score err {_err(got.cpu(), want):.3e}, fp32 restatement {_err(f32, want):.3e}')
        assert _err(got.cpu(), want) <= 32 * _err(f32, want)


def test_detector_relative():
    from cmhar.ood import MahalanobisDetector
    train, y, x_in, _, x_out, _ = _data()
    want = _pipeline(train, y, (x_in, x_out), torch.float64, relative=True)
    f32 = _pipeline(train, y, (x_in, x_out), torch.float32, relative=True)
    det = MahalanobisDetector(relative=True).fit(train.to(DEV), y.to(DEV))
    for x, (w, _), (f, _) in zip((x_in, x_out), want, f32):
        s = det.score(x.to(DEV)).cpu()
        print(f'relative score err {_err(s, w):.3e}, fp32 restatement {_err(f, w):.3e}')
        assert _err(s, w) <= 32 * _err(f, w)


def test_detector_labels():
    from cmhar.ood import MahalanobisDetector
    train, y, x_in, y_in, *_ = _data()
    orig = torch.tensor([0, 3, 7])
    keep = y < 3
    det = MahalanobisDetector().fit(train[keep].to(DEV), orig[y[keep]])
    assert det.classes_.tolist() == [0, 3, 7] and det.means_.shape == (3, 64) and det.counts_.tolist() == [200] * 3
    k_in = y_in < 3
    s, cls = det.predict(x_in[k_in].to(DEV))
    assert torch.equal(cls.cpu(), orig[y_in[k_in]])
    (want, wc), = _pipeline(train[keep], orig[y[keep]], (x_in[k_in],), torch.float64)
    assert torch.equal(cls.cpu(), wc) and _err(s.cpu(), want) < 1e-4
    assert det.distances(x_in[k_in].to(DEV)).shape == (int(k_in.sum()), 3)
    with pytest.raises(ValueError):
        MahalanobisDetector().fit(train.to(DEV), y - 1)
    with pytest.raises(ValueError):
        MahalanobisDetector().fit(train.to(DEV), y + 121)                 # max label 128: 129 classes
    with pytest.raises(RuntimeError):
        MahalanobisDetector().score(x_in.to(DEV))


def test_detector_few_shot_needs_shrinkage():
    from cmhar.ood import MahalanobisDetector
    train, y, x_in, *_ = _data()
    with pytest.raises(ValueError, match='shrinkage'):
        MahalanobisDetector().fit(train[:40].to(DEV), y[:40])
    det = MahalanobisDetector(shrinkage=0.1).fit(train[:40].to(DEV), y[:40])
    s = det.score(x_in.to(DEV))
    assert s.shape == (400,) and bool(torch.isfinite(s).all())
    (want, _), = _pipeline(train[:40], y[:40], (x_in,), torch.float64, shrinkage=0.1)
    assert _err(s.cpu(), want) < 1e-4


def test_bf16_features_are_widened_exactly():
    from cmhar.ood import MahalanobisDetector, class_moments
    train, y, x_in, *_ = _data()
    tb, xb = train.to(DEV, torch.bfloat16), x_in.to(DEV, torch.bfloat16)
    a, b = class_moments(tb, y, 8), class_moments(tb.float(), y, 8)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    d16, d32 = MahalanobisDetector().fit(tb, y), MahalanobisDetector().fit(tb.float(), y)
    assert torch.equal(d16.whitening_, d32.whitening_)
    assert torch.equal(d16.score(xb), d32.score(xb.float()))


def test_mahalanobis_ood_evaluator_contract():
    from cmhar.config import Config
    from cmhar.imu import IMUEncoder
    from cmhar.models import IMUClassifier
    from cmhar.ood import MahalanobisDetector, MahalanobisOODEvaluator
    cfg = Config()
    cfg.model.imu_dropout = 0.0
    torch.manual_seed(0)
    clf = IMUClassifier(IMUEncoder(cfg), cfg)
    ev = MahalanobisOODEvaluator(clf, cfg, DEV, shrinkage=0.1)
    g = torch.Generator().manual_seed(1)

    def loader():
        return [{'imu': torch.randn(16, 6, cfg.data.imu_window_size, generator=g), 'label': torch.arange(16) % 4}
                for _ in range(3)]
    train, test = loader(), loader()
    assert ev.fit(train) is ev
    scores, labels, classes = ev.predict(test)
    assert isinstance(scores, np.ndarray) and scores.shape == (48,) and scores.dtype == np.float32
    assert labels.shape == (48,) and np.array_equal(labels, np.tile(np.arange(16) % 4, 3))
    assert classes.shape == (48,) and classes.dtype == np.int64 and set(classes.tolist()) <= {0, 1, 2, 3}
    with torch.no_grad():
        def feats(batches):
            return torch.cat([clf.imu_encoder(b['imu'].to(DEV))[0] for b in batches])
        det = MahalanobisDetector(shrinkage=0.1).fit(feats(train), torch.arange(16).repeat(3) % 4)
        want, wcls = det.predict(feats(test))
    assert np.array_equal(scores, want.cpu().numpy()) and np.array_equal(classes, wcls.cpu().numpy())
    assert 0.0 <= ev.ood_auroc(test, train) <= 1.0
