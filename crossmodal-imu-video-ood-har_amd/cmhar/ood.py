"""Energy-score out-of-distribution scoring on the prediction path (BASELINE config 5).

The reference repository is named for OOD HAR but contains no OOD code; its inference path is
`Evaluator.predict` (`src/eval/evaluator.py:28-53`): `model.eval()`, `logits = model(imu)` per batch under
`torch.no_grad()`, `logits.max(1)` for the predictions, numpy arrays out.  `OODEvaluator` keeps that interface and
adds the energy score E(x) = −T·logsumexp(f(x)/T) (Liu et al., energy-based OOD detection), computed on the device
in the same single pass over the logits as the predictions (`cmhar_logits_energy`).  Lower energy = more
in-distribution; `auroc(in_scores, out_scores)` reports how well a score separates the two (parity unpinned
w.r.t. the reference, which has no such code: checked against torch / sklearn in the tests).

The pretrained `CrossModalModel` has no logits: its product is a pair of unit-norm embeddings.  For such features
`KNNDetector` / `KNNOODEvaluator` give the label-free deep k-NN score (Sun et al. 2022, "Out-of-distribution detection
with deep nearest neighbors"): minus the Euclidean distance from the L2-normalised feature to its k-th nearest
training feature, −sqrt(2 − 2·s_k) with s_k the k-th largest cosine, found by the fused similarity top-k kernel
(`cmhar.retrieval.sim_topk`) without storing the N×M similarities.  Higher score = more in-distribution.

With LABELLED in-distribution features and no classifier head — the few-shot HAR setting — `MahalanobisDetector` /
`MahalanobisOODEvaluator` give the class-conditional Gaussian score (Lee et al. 2018, "A simple unified framework for
detecting out-of-distribution samples and adversarial attacks"): class means and one tied covariance are fitted by
`class_moments` (`cmhar_class_moments`), and a feature is scored by minus its smallest squared Mahalanobis distance to
a class mean, found by `class_min_dist` (`cmhar_class_min_dist`: whitening GEMM, per-class squared distance and row
minimum in one kernel, exact fp32).  The arg-min class is a nearest-class-mean classifier.  `relative=True` subtracts
the distance to one background Gaussian fitted to all rows (Ren et al. 2021, "A simple fix to Mahalanobis distance for
improving near-OOD detection").  `auroc`, `fpr_at_tpr` and `aupr` are the three figures OOD results are quoted in.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from .retrieval import sim_topk


def logits_energy(logits: torch.Tensor, temperature: float = 1.0):
    """(pred int64 [N], energy fp32 [N], max logit fp32 [N]) of a device [N, C] fp32/bf16 logits matrix."""
    if logits.dim() != 2 or not logits.is_cuda:
        raise ValueError('expected a 2-D device logits matrix')
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    if temperature <= 0:
        raise ValueError('temperature must be positive')
    N, C = logits.shape
    dev = logits.device
    pred = torch.empty(N, dtype=torch.int32, device=dev)
    energy = torch.empty(N, dtype=torch.float32, device=dev)
    mx = torch.empty(N, dtype=torch.float32, device=dev)
    L.call('cmhar_logits_energy', L.dtype_code(logits.dtype), N, C, logits.data_ptr(), logits.stride(0),
           float(temperature), pred.data_ptr(), energy.data_ptr(), mx.data_ptr(), L.stream(dev))
    return pred.long(), energy, mx


def energy_score(logits: torch.Tensor, temperature: float = 1.0) -> torch.Tensor:
    """E = −T·logsumexp(logits/T) per row (fp32, on the device)."""
    return logits_energy(logits, temperature)[1]


def auroc(in_scores, out_scores) -> float:
    """Area under the ROC curve for separating in-distribution (positive, HIGHER score) from OOD samples — the
    Mann–Whitney U statistic with average ranks for ties (equals sklearn.metrics.roc_auc_score).  For energies pass
    −E (lower energy = in-distribution)."""
    a = np.asarray(in_scores, dtype=np.float64).ravel()
    b = np.asarray(out_scores, dtype=np.float64).ravel()
    if a.size == 0 or b.size == 0:
        raise ValueError('both score sets must be non-empty')
    allv = np.concatenate([a, b])
    order = np.argsort(allv, kind='mergesort')
    ranks = np.empty(allv.size, dtype=np.float64)
    sv = allv[order]
    new_run = np.r_[True, sv[1:] != sv[:-1]]    # average ranks over tied runs, vectorised (O(n log n) overall)
    starts = np.flatnonzero(new_run)
    ends = np.r_[starts[1:], sv.size] - 1
    ranks[order] = (0.5 * (starts + ends) + 1.0)[np.cumsum(new_run) - 1]
    u = ranks[:a.size].sum() - a.size * (a.size + 1) / 2.0
    return float(u / (a.size * b.size))


def _roc_counts(in_scores, out_scores):
    """(true positives, false positives, #positives, #negatives) at every distinct threshold, from the highest score
    down (in-distribution = positive, HIGHER score; a threshold takes all of its tied scores at once)."""
    a = np.asarray(in_scores, dtype=np.float64).ravel()
    b = np.asarray(out_scores, dtype=np.float64).ravel()
    if a.size == 0 or b.size == 0:
        raise ValueError('both score sets must be non-empty')
    allv = np.concatenate([a, b])
    pos = np.r_[np.ones(a.size), np.zeros(b.size)]
    order = np.argsort(-allv, kind='mergesort')
    sv = allv[order]
    last = np.r_[np.flatnonzero(sv[1:] != sv[:-1]), sv.size - 1]      # the last entry of each tied run
    tps = np.cumsum(pos[order])[last]
    return tps, last + 1.0 - tps, a.size, b.size


def fpr_at_tpr(in_scores, out_scores, tpr: float = 0.95) -> float:
    """False-positive rate (OOD samples accepted) at the first ROC point whose true-positive rate is at least `tpr`
    — FPR@95 for the default (equals `fpr[argmax(tpr >= t)]` of sklearn.metrics.roc_curve without dropped points).
    Same conventions as `auroc`."""
    tps, fps, npos, nneg = _roc_counts(in_scores, out_scores)
    tp_rate = np.r_[0.0, tps / npos]
    fp_rate = np.r_[0.0, fps / nneg]
    return float(fp_rate[np.argmax(tp_rate >= tpr)])


def aupr(in_scores, out_scores) -> float:
    """Area under the precision-recall curve with in-distribution as the positive class, as the step-wise average
    precision Σ_n (R_n − R_{n−1})·P_n (equals sklearn.metrics.average_precision_score).  Same conventions as
    `auroc`."""
    tps, fps, npos, _ = _roc_counts(in_scores, out_scores)
    recall = tps / npos
    return float(np.sum(np.diff(np.r_[0.0, recall]) * (tps / (tps + fps))))


class OODEvaluator:
    """`Evaluator` (`src/eval/evaluator.py:18-53`) with energy scores: same constructor and `predict(dataloader)`
    (batches with 'imu' and 'label'), returning (predictions, labels, logits, energies) numpy arrays.  Batches that
    also carry 'video' are scored by a two-input model — `model(imu, video)`, e.g. the cross-attention fusion
    classifier (`cmhar.fusion.CrossModalFusionClassifier`), whose class logits are the "fused logits" of config 5."""

    def __init__(self, model, config, device='cuda', temperature: float = 1.0):
        self.model = model.to(device)
        self.config = config
        self.device = device
        self.temperature = float(temperature)
        self.model.eval()

    @torch.no_grad()
    def predict(self, dataloader):
        preds, labels, logits, energies = [], [], [], []
        for batch in dataloader:
            imu = batch['imu'].to(self.device)
            if 'video' in batch:
                out = self.model(imu, batch['video'].to(self.device))
            else:
                out = self.model(imu)
            p, e, _ = logits_energy(out.float(), self.temperature)
            preds.append(p.cpu().numpy())
            labels.append(np.asarray(batch['label']))
            logits.append(out.float().cpu().numpy())
            energies.append(e.cpu().numpy())
        return (np.concatenate(preds), np.concatenate(labels), np.vstack(logits), np.concatenate(energies))

    def ood_auroc(self, in_loader, out_loader) -> float:
        """AUROC of −energy for in-distribution vs OOD loaders."""
        e_in = self.predict(in_loader)[3]
        e_out = self.predict(out_loader)[3]
        return auroc(-e_in, -e_out)


def _knn_score(s_k: torch.Tensor) -> torch.Tensor:
    return -torch.sqrt(torch.clamp(2.0 - 2.0 * s_k, min=0.0))


class KNNDetector:
    """Deep k-NN OOD score on L2-normalised features.  `fit(features)` stores the normalised bank in `bank_dtype`
    (fp32 by default: with cosines near 1 the bf16 rounding of the embeddings is visible in sqrt(2 − 2s));
    `score(features)` → fp32 [N], −(distance to the k-th nearest bank row); `score_bank()` scores the bank against
    itself leaving each row out of its own neighbours — the scores a threshold at a chosen TPR is read from."""

    def __init__(self, k: int = 10, bank_dtype=torch.float32):
        self.k = int(k)
        self.bank_dtype = bank_dtype
        self.bank = None

    def _normalise(self, features):
        from .heads import l2_normalize
        if features.dim() != 2 or not features.is_cuda:
            raise ValueError('expected a 2-D device feature matrix')
        with torch.no_grad():
            return l2_normalize(features.detach()).to(self.bank_dtype)

    def fit(self, features: torch.Tensor):
        self.bank = self._normalise(features)
        return self

    def _need_bank(self):
        if self.bank is None:
            raise RuntimeError('KNNDetector.fit has not been called')

    def score(self, features: torch.Tensor) -> torch.Tensor:
        self._need_bank()
        vals, _ = sim_topk(self._normalise(features), self.bank, self.k)
        return _knn_score(vals[:, self.k - 1])

    def score_bank(self) -> torch.Tensor:
        self._need_bank()
        vals, _ = sim_topk(self.bank, self.bank, self.k, self_offset=0)
        return _knn_score(vals[:, self.k - 1])


def _imu_cls_feature(model, imu):
    """The IMU CLS feature of an IMUEncoder, an IMUClassifier or a CrossModalModel (there through its projection)."""
    if hasattr(model, 'imu_proj'):
        return model.imu_proj(model.imu_encoder(imu)[0])
    if hasattr(model, 'imu_encoder'):
        return model.imu_encoder(imu)[0]
    return model(imu)[0]


class KNNOODEvaluator:
    """`OODEvaluator`'s loader interface with the k-NN score: `fit(train_loader)` builds the bank from the
    in-distribution training windows, `predict(loader)` → (scores, labels) numpy arrays, `ood_auroc(in, out)`.
    `feature_fn(model, imu)` → [B, d] device features; the default takes the IMU CLS feature."""

    def __init__(self, model, config, device='cuda', k: int = 10, feature_fn=None, bank_dtype=torch.float32):
        self.model = model.to(device)
        self.config = config
        self.device = device
        self.feature_fn = feature_fn or _imu_cls_feature
        self.detector = KNNDetector(k, bank_dtype)
        self.model.eval()

    @torch.no_grad()
    def _features(self, dataloader):
        feats, labels = [], []
        for batch in dataloader:
            feats.append(self.feature_fn(self.model, batch['imu'].to(self.device)).float())
            if 'label' in batch:
                labels.append(np.asarray(batch['label']))
        return torch.cat(feats), (np.concatenate(labels) if labels else np.zeros(0, dtype=np.int64))

    def fit(self, train_loader):
        self.detector.fit(self._features(train_loader)[0])
        return self

    def predict(self, dataloader):
        feats, labels = self._features(dataloader)
        return self.detector.score(feats).cpu().numpy(), labels

    def ood_auroc(self, in_loader, out_loader) -> float:
        """AUROC of the k-NN score for in-distribution vs OOD loaders."""
        return auroc(self.predict(in_loader)[0], self.predict(out_loader)[0])


_FEATURE_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
MAX_CLASSES = 128


def _feature_rows(features, what='features'):
    """Argument checks shared by the two Mahalanobis kernels' wrappers: what the kernels would refuse raises
    ValueError; a view whose rows are not 16-byte aligned is copied."""
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or not features.is_cuda:
        raise ValueError(f'{what}: expected a 2-D device tensor')
    if features.dtype not in _FEATURE_DTYPES:
        raise ValueError(f'{what}: unsupported dtype {features.dtype} (fp32, bf16 or fp16)')
    N, d = features.shape
    if N < 1:
        raise ValueError(f'{what}: no rows')
    if d < 32 or d > 1024 or d % 32 != 0:
        raise ValueError(f'd = {d} is outside the supported range (32..1024, a multiple of 32)')
    align = 16 // features.element_size()
    if (features.stride(1) != 1 or features.stride(0) % align != 0 or features.stride(0) < d
            or features.data_ptr() % 16 != 0):
        features = features.contiguous()
    return features.detach()


def _fp32_rows(t, d, what):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or not t.is_cuda:
        raise ValueError(f'{what}: expected a 2-D device tensor')
    if t.dtype != torch.float32:
        raise ValueError(f'{what} must be fp32, got {t.dtype}')
    if t.shape[1] != d:
        raise ValueError(f'{what} has width {t.shape[1]}, the features have {d}')
    if t.stride(1) != 1 or t.stride(0) % 4 != 0 or t.stride(0) < d or t.data_ptr() % 16 != 0:
        t = t.contiguous()
    return t.detach()


def class_moments(features: torch.Tensor, labels, num_classes: int):
    """(counts int64 [C], means fp32 [C, d], scatter fp32 [d, d]) of device features [N, d] (fp32 / bf16 / fp16,
    32 <= d <= 1024, d % 32 == 0) with integer labels [N]: class sizes, class means (an empty class: zeros) and the
    tied scatter Σ_i (x_i − μ_{y_i})(x_i − μ_{y_i})ᵀ, exactly symmetric, in fp32 and in two passes
    (`cmhar_class_moments`).  Rows labelled outside [0, num_classes) count for nothing."""
    x = _feature_rows(features)
    N, d = x.shape
    C = int(num_classes)
    if C < 1 or C > MAX_CLASSES:
        raise ValueError(f'num_classes = {C} is outside 1..{MAX_CLASSES}')
    dev = x.device
    labels = torch.as_tensor(labels)
    if labels.dim() != 1 or labels.shape[0] != N or labels.is_floating_point():
        raise ValueError('labels must be N integers')
    labels = labels.to(device=dev, dtype=torch.int64).contiguous()
    counts = torch.empty(C, dtype=torch.int32, device=dev)
    means = torch.empty(C, d, dtype=torch.float32, device=dev)
    scatter = torch.empty(d, d, dtype=torch.float32, device=dev)
    ws = torch.empty(L.lib().cmhar_class_moments_ws(N, d, C), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.call('cmhar_class_moments', L.dtype_code(x.dtype), N, d, C, x.data_ptr(), x.stride(0), labels.data_ptr(),
               counts.data_ptr(), means.data_ptr(), scatter.data_ptr(), ws.data_ptr(), L.stream(dev))
    return counts.long(), means, scatter


def class_min_dist(features: torch.Tensor, W: torch.Tensor, m: torch.Tensor, return_all: bool = False):
    """(dist2 fp32 [N], cls int64 [N]) and, with `return_all`, dist_all fp32 [N, C]: for each row x of the device
    features [N, d], z = W·x and D[c] = Σ_j (z_j − m[c][j])² in exact fp32, its minimum over the classes and the first
    class attaining it (`cmhar_class_min_dist`).  W [d, d] and m [C, d] are fp32, C <= 128."""
    x = _feature_rows(features)
    N, d = x.shape
    W = _fp32_rows(W, d, 'W')
    m = _fp32_rows(m, d, 'm')
    if W.shape[0] != d:
        raise ValueError(f'W must be [{d}, {d}], got {tuple(W.shape)}')
    C = m.shape[0]
    if C < 1 or C > MAX_CLASSES:
        raise ValueError(f'm has {C} rows, outside 1..{MAX_CLASSES}')
    dev = x.device
    if W.device != dev or m.device != dev:
        raise ValueError('features, W and m must be on one GPU')
    dist2 = torch.empty(N, dtype=torch.float32, device=dev)
    cls = torch.empty(N, dtype=torch.int32, device=dev)
    dist_all = torch.empty(N, C, dtype=torch.float32, device=dev) if return_all else None
    with torch.cuda.device(dev):
        L.call('cmhar_class_min_dist', L.dtype_code(x.dtype), N, d, C, x.data_ptr(), x.stride(0), W.data_ptr(),
               W.stride(0), m.data_ptr(), m.stride(0), dist2.data_ptr(), cls.data_ptr(), L.ptr(dist_all), C,
               L.stream(dev))
    return (dist2, cls.long(), dist_all) if return_all else (dist2, cls.long())


class MahalanobisDetector:
    """Class-conditional Gaussian OOD score with one tied covariance (Lee et al. 2018).  `fit(features, labels)`:
    class means and Σ = scatter / N from `class_moments`, with `shrinkage` α Σ ← (1−α)Σ + α·(tr Σ / d)·I, factored
    Σ = L Lᵀ on the host in fp64 (one d×d copy and one sync per fit); `whitening_` = L⁻¹ so that the squared
    Mahalanobis distance to class c is ‖L⁻¹x − L⁻¹μ_c‖².  `score(features)` → fp32 [N], −min_c d²_c (higher = more
    in-distribution); `predict` adds the arg-min class in the ORIGINAL labels (`classes_`: empty classes are
    dropped); `distances` → [N, C'].  `relative=True` scores −(min_c d²_c − d²_0) against one background Gaussian
    fitted to all rows (Ren et al. 2021).  When N − C < d the covariance is singular and `fit` raises ValueError:
    few-shot fits need `shrinkage` > 0."""

    def __init__(self, shrinkage: float = 0.0, relative: bool = False):
        self.shrinkage = float(shrinkage)
        if not 0.0 <= self.shrinkage <= 1.0:
            raise ValueError('shrinkage must lie in [0, 1]')
        self.relative = bool(relative)
        self.classes_ = None

    def _whiten(self, scatter, n, means):
        """(covariance fp32, L⁻¹ fp32, whitened means fp32) on the scatter's device."""
        dev = scatter.device
        d = scatter.shape[0]
        cov = scatter.double().cpu() / n
        if self.shrinkage > 0:
            cov = (1.0 - self.shrinkage) * cov + self.shrinkage * (torch.trace(cov) / d) * torch.eye(
                d, dtype=torch.float64)
        cov32 = cov.float()
        chol, info = torch.linalg.cholesky_ex(cov32.double())
        # a pivot below the fp32 rounding of the stored covariance is noise: a singular Σ must not pass by luck
        floor = d * 2.0 ** -24 * float(cov32.diagonal().max())
        if int(info) != 0 or not float(chol.diagonal().min()) ** 2 > floor:
            raise ValueError(f'the tied covariance of {n} rows at d = {d} is not positive definite with shrinkage = '
                             f'{self.shrinkage}; raise shrinkage (few-shot fits with N - C < d need it)')
        linv = torch.linalg.solve_triangular(chol, torch.eye(d, dtype=torch.float64), upper=False)
        wm = means.double().cpu() @ linv.T
        return cov32.to(dev), linv.float().to(dev), wm.float().to(dev)

    def fit(self, features: torch.Tensor, labels):
        x = _feature_rows(features)
        labels = torch.as_tensor(labels)
        if labels.dim() != 1 or labels.shape[0] != x.shape[0] or labels.is_floating_point():
            raise ValueError('labels must be N integers')
        lo, hi = int(labels.min()), int(labels.max())
        if lo < 0:
            raise ValueError('labels must be non-negative')
        C = hi + 1
        if C > MAX_CLASSES:
            raise ValueError(f'{C} classes (max label + 1) exceed the supported {MAX_CLASSES}')
        N = x.shape[0]
        counts, means, scatter = class_moments(x, labels, C)
        keep = counts > 0
        cov, w, wm = self._whiten(scatter, N, means[keep])
        if self.relative:
            _, mean0, scatter0 = class_moments(x, torch.zeros(N, dtype=torch.int64, device=x.device), 1)
            self.covariance0_, self.whitening0_, self._wmean0 = self._whiten(scatter0, N, mean0)
            self.mean0_ = mean0
        self.classes_ = torch.nonzero(keep).flatten()
        self.counts_ = counts[keep]
        self.means_ = means[keep]
        self.covariance_, self.whitening_, self._wmeans = cov, w, wm
        return self

    def _need_fit(self):
        if self.classes_ is None:
            raise RuntimeError('MahalanobisDetector.fit has not been called')

    def distances(self, features: torch.Tensor) -> torch.Tensor:
        """Squared Mahalanobis distances [N, C'] to the fitted classes (columns in `classes_` order)."""
        self._need_fit()
        return class_min_dist(features, self.whitening_, self._wmeans, return_all=True)[2]

    def predict(self, features: torch.Tensor):
        """(score fp32 [N], class int64 [N] in the original labels)."""
        self._need_fit()
        d2, cls = class_min_dist(features, self.whitening_, self._wmeans)
        if self.relative:
            d2 = d2 - class_min_dist(features, self.whitening0_, self._wmean0)[0]
        return -d2, self.classes_[cls]

    def score(self, features: torch.Tensor) -> torch.Tensor:
        return self.predict(features)[0]


class MahalanobisOODEvaluator:
    """`KNNOODEvaluator`'s loader interface with the Mahalanobis score: `fit(train_loader)` fits the detector on the
    labelled in-distribution training windows (batches with 'imu' and 'label'), `predict(loader)` → (scores, labels,
    predicted classes) numpy arrays, `ood_auroc(in, out)`.  `feature_fn(model, imu)` → [B, d] device features; the
    default takes the IMU CLS feature."""

    def __init__(self, model, config, device='cuda', feature_fn=None, shrinkage: float = 0.0, relative: bool = False):
        self.model = model.to(device)
        self.config = config
        self.device = device
        self.feature_fn = feature_fn or _imu_cls_feature
        self.detector = MahalanobisDetector(shrinkage, relative)
        self.model.eval()

    _features = KNNOODEvaluator._features

    def fit(self, train_loader):
        feats, labels = self._features(train_loader)
        self.detector.fit(feats, torch.from_numpy(np.asarray(labels, dtype=np.int64)))
        return self

    def predict(self, dataloader):
        feats, labels = self._features(dataloader)
        score, cls = self.detector.predict(feats)
        return score.cpu().numpy(), labels, cls.cpu().numpy()

    def ood_auroc(self, in_loader, out_loader) -> float:
        """AUROC of the Mahalanobis score for in-distribution vs OOD loaders."""
        return auroc(self.predict(in_loader)[0], self.predict(out_loader)[0])
