"""Retrieval recall@k (`cmhar.retrieval`) and the deep k-NN OOD detector (`cmhar.ood.KNNDetector`,
`KNNOODEvaluator`) against fp64 restatements written here (the reference has no counterpart of either)."""
import numpy as np
import pytest
import torch

DEV = 'cuda'
pytestmark = pytest.mark.gpu


def _ref_recall(a, b, ks):
    """Fraction of rows i of `a` whose positive (row i of `b`) is among the first k of (−score, index) order."""
    s = a.double() @ b.double().T
    order = torch.sort(-s, dim=1, stable=True).indices
    hit = order == torch.arange(a.shape[0]).unsqueeze(1)
    return {k: int(hit[:, :k].any(1).sum()) / a.shape[0] for k in ks}


def test_recall_at_k_vs_fp64_restatement():
    from cmhar.retrieval import recall_at_k
    g = torch.Generator().manual_seed(2)
    base = torch.randint(-1, 2, (300, 64), generator=g).float()
    a = base + torch.randint(-2, 3, (300, 64), generator=g).float()      # integer-valued, correlated pairs, many ties:
    b = base + torch.randint(-2, 3, (300, 64), generator=g).float()      # reference recall@1/5/10 ≈ 0.2 / 0.4 / 0.6
    ks = (1, 5, 10)
    got = recall_at_k(a.to(DEV), b.to(DEV), ks)
    assert got == {'imu_to_video': _ref_recall(a, b, ks), 'video_to_imu': _ref_recall(b, a, ks)}
    assert 0.0 < got['imu_to_video'][1] <= got['imu_to_video'][5] <= got['imu_to_video'][10]

    u = torch.nn.functional.normalize(torch.randn(300, 64, generator=g), dim=1).to(DEV)
    same = recall_at_k(u, u.clone(), ks)
    assert same['imu_to_video'][1] == 1.0 and same['video_to_imu'][1] == 1.0
    shifted = recall_at_k(u, torch.roll(u, 1, dims=0), (1,))
    assert shifted['imu_to_video'][1] == 0.0 and shifted['video_to_imu'][1] == 0.0


def _ref_knn_scores(feats, bank, k, leave_one_out=False):
    fn = torch.nn.functional.normalize(feats.double(), dim=1)
    bn = torch.nn.functional.normalize(bank.double(), dim=1)
    s = fn @ bn.T
    if leave_one_out:
        s.fill_diagonal_(-float('inf'))
    s_k = s.topk(k, dim=1).values[:, -1]
    return -torch.sqrt(torch.clamp(2 - 2 * s_k, min=0))


def _cluster_data():
    """8 cluster centres on the 64-d sphere; in-distribution = centre + 0.05·N(0, I) per coordinate, OOD = uniform on
    the sphere.  With seed 4 the fp64 reference scores alone give AUROC 1.0 (checked on the CPU; in-cluster cosines
    are ≈ 0.86, an OOD point's best cosine against 800 bank rows ≈ 0.45)."""
    g = torch.Generator().manual_seed(4)
    centres = torch.nn.functional.normalize(torch.randn(8, 64, generator=g), dim=1)

    def around(n):
        return centres[torch.arange(n) % 8] + 0.05 * torch.randn(n, 64, generator=g)
    return around(800), around(200), torch.randn(200, 64, generator=g)


def test_knn_detector_scores_and_separation():
    from cmhar.ood import KNNDetector, auroc
    train, x_in, x_out = _cluster_data()
    det = KNNDetector(k=10).fit(train.to(DEV))
    assert det.bank.dtype == torch.float32 and det.bank.shape == (800, 64)
    for x in (x_in, x_out):
        s = det.score(x.to(DEV))
        assert s.dtype == torch.float32 and s.shape == (200,)
        assert (s.cpu().double() - _ref_knn_scores(x, train, 10)).abs().max().item() < 1e-5
    sb = det.score_bank()
    assert (sb.cpu().double() - _ref_knn_scores(train, train, 10, leave_one_out=True)).abs().max().item() < 1e-5
    ref_in, ref_out = _ref_knn_scores(x_in, train, 10), _ref_knn_scores(x_out, train, 10)
    assert auroc(ref_in.numpy(), ref_out.numpy()) > 0.99                  # the reference separates them
    assert auroc(det.score(x_in.to(DEV)).cpu().numpy(), det.score(x_out.to(DEV)).cpu().numpy()) > 0.99
    with pytest.raises(RuntimeError):
        KNNDetector().score(x_in.to(DEV))
    # a 16-bit bank is an option; its scores stay close to the fp32 ones (bf16 rounding of unit rows: ~2^-9 per cosine)
    det16 = KNNDetector(k=10, bank_dtype=torch.bfloat16).fit(train.to(DEV))
    assert det16.bank.dtype == torch.bfloat16
    assert auroc(det16.score(x_in.to(DEV)).cpu().numpy(), det16.score(x_out.to(DEV)).cpu().numpy()) > 0.99


def test_knn_ood_evaluator_contract():
    from cmhar.config import Config
    from cmhar.imu import IMUEncoder
    from cmhar.models import IMUClassifier
    from cmhar.ood import KNNDetector, KNNOODEvaluator
    cfg = Config()
    cfg.model.imu_dropout = 0.0
    torch.manual_seed(0)
    clf = IMUClassifier(IMUEncoder(cfg), cfg)
    ev = KNNOODEvaluator(clf, cfg, DEV, k=5)
    g = torch.Generator().manual_seed(1)

    def loader():
        return [{'imu': torch.randn(16, 6, cfg.data.imu_window_size, generator=g), 'label': torch.arange(16) % 4}
                for _ in range(3)]
    train, test = loader(), loader()
    assert ev.fit(train) is ev
    scores, labels = ev.predict(test)
    assert isinstance(scores, np.ndarray) and scores.shape == (48,) and scores.dtype == np.float32
    assert labels.shape == (48,) and np.array_equal(labels, np.tile(np.arange(16) % 4, 3))
    with torch.no_grad():
        def feats(batches):
            return torch.cat([clf.imu_encoder(b['imu'].to(DEV))[0] for b in batches])
        want = KNNDetector(k=5).fit(feats(train)).score(feats(test))
    assert np.array_equal(scores, want.cpu().numpy())
    assert 0.0 <= ev.ood_auroc(test, train) <= 1.0


def test_evaluate_retrieval_tiny_crossmodal():
    from cmhar.config import Config
    from cmhar.models import CrossModalModel
    from cmhar.retrieval import evaluate_retrieval, recall_at_k
    cfg = Config()
    cfg.data.video_frames_per_window, cfg.data.video_resize = 2, (16, 16)
    m = cfg.model
    m.video_pretrained = False
    m.video_backbone = '/nonexistent/videomae'
    m.videomae_hidden_size, m.videomae_num_layers, m.videomae_num_heads, m.videomae_intermediate_size = 64, 1, 1, 128
    m.imu_dropout = 0.0
    torch.manual_seed(0)
    model = CrossModalModel(cfg)
    g = torch.Generator().manual_seed(3)
    batches = [{'imu': torch.randn(8, 6, cfg.data.imu_window_size, generator=g),
                'video': torch.randn(8, 2, 3, 16, 16, generator=g)} for _ in range(2)]
    got = evaluate_retrieval(model, batches, ks=(1, 5, 10), device=DEV)
    assert set(got) == {'imu_to_video', 'video_to_imu'}
    for d in got.values():
        assert set(d) == {1, 5, 10} and all(0.0 <= f <= 1.0 for f in d.values())
        assert d[1] <= d[5] <= d[10]
    model.eval()
    with torch.no_grad():
        outs = [model(b['imu'].to(DEV), b['video'].to(DEV)) for b in batches]
    a, b = torch.cat([o[0] for o in outs]).float(), torch.cat([o[1] for o in outs]).float()
    assert got == recall_at_k(a, b, (1, 5, 10))
