"""The two Mahalanobis kernels (`cmhar_class_moments`, `cmhar_class_min_dist`, csrc/mahalanobis.hip) through
`cmhar.ood.class_moments` / `class_min_dist` and the raw ABI.

No reference counterpart (the reference has no OOD code), so both are checked against fp64 restatements written here.
With small-integer operands every sum is exact in fp32 in any order (the tests assert that precondition on the fp64
values first), so the outputs must EQUAL the fp64 ones; with floats the bounds are multiples of the error of the fp32
torch composite of the same form, computed in the test on the CPU."""
import ctypes
import functools

import pytest
import torch

DEV = 'cuda'
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
EXACT = 2.0 ** 24
pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ class_min_dist

def _int_case(N, d, C, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-2, 3, (N, d), generator=g).float(), torch.randint(-1, 2, (d, d), generator=g).float(),
            torch.randint(-8, 9, (C, d), generator=g).float())


def _ref_dist(x, W, m):
    """fp64 z = W·x and D[c] = Σ_j (z_j − m[c][j])², class by class; also the largest sum of absolute terms of any
    sum the kernel could form (the z chains, and D in the difference or the expanded form)."""
    xd, Wd, md = x.double(), W.double(), m.double()
    z = xd @ Wd.T
    D = torch.stack([((z - md[c]) ** 2).sum(1) for c in range(m.shape[0])], 1)
    big = max((xd.abs() @ Wd.abs().T).max().item(),
              max(((z.abs() + md[c].abs()) ** 2).sum(1).max().item() for c in range(m.shape[0])))
    return D, big


def _check_dist_exact(x, W, m, xdev):
    from cmhar.ood import class_min_dist
    D, big = _ref_dist(x, W, m)
    assert big < EXACT                                                  # exact in fp32 in any summation order
    N, C = D.shape
    dist2, cls, dist_all = class_min_dist(xdev, W.to(DEV), m.to(DEV), return_all=True)
    assert dist2.dtype == torch.float32 and dist2.shape == (N,)
    assert cls.dtype == torch.int64 and cls.shape == (N,)
    assert dist_all.dtype == torch.float32 and dist_all.shape == (N, C)
    assert torch.equal(dist_all.cpu().double(), D)
    assert torch.equal(dist2.cpu().double(), D.min(1).values)
    first = (D == D.min(1, keepdim=True).values).int().argmax(1)        # first index attaining the minimum
    assert torch.equal(cls.cpu(), first)
    d2, c2 = class_min_dist(xdev, W.to(DEV), m.to(DEV))
    assert torch.equal(d2, dist2) and torch.equal(c2, cls)
    return cls.cpu()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('N,d,C', [(1, 32, 1), (17, 32, 3), (130, 256, 32), (64, 768, 10), (3, 1024, 128),
                                   (300, 64, 128), (4099, 128, 33)])
def test_min_dist_exact_integer_operands(dtype, N, d, C):
    x, W, m = _int_case(N, d, C, 1000 * N + C)
    _check_dist_exact(x, W, m, x.to(DEV, dtype))


def test_min_dist_duplicated_class_takes_the_first():
    x, W, m = _int_case(130, 64, 8, 21)
    m[5] = m[2]
    x[:20] = 0
    m[2] = 0                                    # rows 0..19 have z = 0 = m[2] = m[5]: the minimum is attained twice
    m[5] = 0
    cls = _check_dist_exact(x, W, m, x.to(DEV))
    assert bool((cls[:20] == 2).all()) and not bool((cls == 5).any())


def test_min_dist_many_workgroups():
    x, W, m = _int_case(70001, 32, 3, 13)
    _check_dist_exact(x, W, m, x.to(DEV))


@pytest.mark.parametrize('dtype', DTYPES)
def test_min_dist_strided_rows(dtype):
    """x is a column slice of a wider tensor (row stride 320 for d = 256)."""
    x, W, m = _int_case(70, 256, 10, 7)
    wide = torch.full((70, 320), 9.0)
    wide[:, :256] = x
    xv = wide.to(DEV, dtype)[:, :256]
    assert xv.stride(0) == 320
    _check_dist_exact(x, W, m, xv)


# ------------------------------------------------------------------------------------------------- class_moments

def _ref_moments(x, labels, C):
    """fp64 (counts, means, scatter, centred rows) of the rows whose label lies in [0, C)."""
    ok = (labels >= 0) & (labels < C)
    xd, y = x.double()[ok], labels[ok]
    counts = torch.bincount(y, minlength=C)
    means = torch.zeros(C, x.shape[1], dtype=torch.float64).index_add_(0, y, xd)
    means = torch.where(counts[:, None] > 0, means / counts.clamp(min=1)[:, None], torch.zeros_like(means))
    R = xd - means[y]
    return counts, means, R.T @ R, R


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C,d', [(33, 32), (128, 256), (100, 1024)])
def test_moments_exact_integer_operands(dtype, C, d):
    from cmhar.ood import class_moments
    g = torch.Generator().manual_seed(1000 * C + d)
    empty = 3
    sizes = [0 if c == empty else (1, 2, 4, 8)[c % 4] for c in range(C)]
    labels = torch.cat([torch.full((n,), c) for c, n in enumerate(sizes)] + [torch.tensor([-1, C, -1, C, C + 5])])
    labels = labels[torch.randperm(labels.numel(), generator=g)]
    x = torch.randint(-2, 3, (labels.numel(), d), generator=g).float()
    counts64, means64, scatter64, R = _ref_moments(x, labels, C)
    assert (R.abs().T @ R.abs()).max().item() * 64 < EXACT               # multiples of 1/64 below 2^24 / 64: exact
    assert torch.equal(means64 * 8, (means64 * 8).round())

    counts, means, scatter = class_moments(x.to(DEV, dtype), labels, C)
    assert counts.dtype == torch.int64 and means.dtype == torch.float32 and scatter.dtype == torch.float32
    assert counts.shape == (C,) and means.shape == (C, d) and scatter.shape == (d, d)
    assert torch.equal(counts.cpu(), counts64) and counts[empty].item() == 0
    assert torch.equal(means.cpu().double(), means64) and not bool(means[empty].any())
    assert torch.equal(scatter.cpu().double(), scatter64)
    assert torch.equal(scatter, scatter.T)
    # the rows with labels outside [0, C) are as good as absent
    ok = (labels >= 0) & (labels < C)
    c2, m2, s2 = class_moments(x[ok].to(DEV, dtype), labels[ok].to(DEV), C)
    assert torch.equal(c2, counts) and torch.equal(m2, means) and torch.equal(s2, scatter)


def _gauss_data(C, d, n_train, n_in, n_out, seed=5):
    """C class means 2·N(0, I), shared covariance Q diag(s²) Qᵀ with s = 6 on 8 directions and 0.3 on the rest, rows
    assigned round-robin; OOD rows are in-distribution rows shifted by a vector of norm 3 inside the quiet subspace.
    fp64."""
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
    return train, ytrain, x_in, y_in, x_out, y_out


def test_moments_offset_floats():
    """Features with a common offset of 100: the two-pass form keeps the scatter's digits (the one-pass XᵀX − Σ n μμᵀ
    loses four).  Measured on MI355X: scatter error 6.9e-8, 0.79x the composite's 8.8e-8; one-pass 8.4e-4."""
    from cmhar.ood import class_moments
    train, y, *_ = _gauss_data(8, 64, 1600, 1, 1)
    x = (train + 100.0).float()
    counts64, means64, scatter64, _ = _ref_moments(x, y, 8)
    # the fp32 two-pass torch composite, on the CPU
    m32 = torch.zeros(8, 64).index_add_(0, y, x) / counts64[:, None].float()
    R32 = x - m32[y]
    err_comp = ((R32.T @ R32).double() - scatter64).norm().item() / scatter64.norm().item()
    xd = x.double()
    one_pass = (x.T @ x - (m32.T * counts64.float()) @ m32).double()
    err_one = (one_pass - scatter64).norm().item() / scatter64.norm().item()

    counts, means, scatter = class_moments(x.to(DEV), y, 8)
    assert torch.equal(counts.cpu(), counts64)
    bound = counts64[:, None].double() * 2.0 ** -23 * xd.abs().max().item()
    merr = (means.cpu().double() - means64).abs()
    err = (scatter.cpu().double() - scatter64).norm().item() / scatter64.norm().item()
    print(f'means: max err / bound = {(merr / bound).max().item():.3f}; scatter rel err {err:.3e}, composite '
          f'{err_comp:.3e} (ratio {err / err_comp:.2f}), one-pass {err_one:.3e}')
    assert bool((merr <= bound).all())
    assert torch.equal(scatter, scatter.T)
    assert err <= 64 * err_comp


@functools.lru_cache(maxsize=None)
def _fitted(C, d):
    """fp32 (W, m) of the generator's data fitted in fp64, and its in-distribution and OOD rows."""
    train, y, x_in, _, x_out, _ = _gauss_data(C, d, 1600, 400, 400)
    _, means, scatter, _ = _ref_moments(train, y, C)
    chol = torch.linalg.cholesky(scatter / train.shape[0])
    W = torch.linalg.solve_triangular(chol, torch.eye(d, dtype=torch.float64), upper=False)
    return W.float(), (means @ W.T).float(), torch.cat([x_in, x_out]).float()


@pytest.mark.parametrize('C,d', [(8, 64), (10, 768)])
def test_min_dist_floats(C, d):
    """Measured on MI355X: 6.8e-7 = 1.20x the composite's error at (8, 64), 5.2e-7 = 1.84x at (10, 768)."""
    from cmhar.ood import class_min_dist
    W, m, x = _fitted(C, d)
    D64, _ = _ref_dist(x, W, m)
    want = D64.min(1).values
    z32 = x @ W.T                                                        # the fp32 difference-form torch composite
    comp = torch.stack([((z32 - m[c]) ** 2).sum(1) for c in range(C)], 1).min(1).values
    err_comp = ((comp.double() - want).abs() / want).max().item()
    dist2, cls, dist_all = class_min_dist(x.to(DEV), W.to(DEV), m.to(DEV), return_all=True)
    err = ((dist2.cpu().double() - want).abs() / want).max().item()
    print(f'dist2 max rel err {err:.3e}, composite {err_comp:.3e} (ratio {err / err_comp:.2f})')
    assert err <= 32 * err_comp
    assert torch.equal(dist_all.min(1).values, dist2)
    assert torch.equal(cls.cpu(), D64.argmin(1))                         # well separated classes: no near ties


def test_deterministic():
    from cmhar.ood import class_min_dist, class_moments
    g = torch.Generator().manual_seed(17)
    x = torch.randn(5000, 128, generator=g).to(DEV)
    y = torch.randint(0, 10, (5000,), generator=g).to(DEV)
    W = torch.randn(128, 128, generator=g).to(DEV)
    m = torch.randn(10, 128, generator=g).to(DEV)
    a, b = class_moments(x, y, 10), class_moments(x, y, 10)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    a, b = class_min_dist(x, W, m, return_all=True), class_min_dist(x, W, m, return_all=True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


# ----------------------------------------------------------------------------------------------------- refusals

def test_raw_refusals_launch_nothing():
    from cmhar import _lib
    lib = _lib.lib()
    x = torch.ones(8 * 1056 + 16, device=DEV)
    y = torch.zeros(8, dtype=torch.int64, device=DEV)
    Wm = torch.ones(1056 * 1056, device=DEV)
    ws = torch.zeros(max(int(lib.cmhar_class_moments_ws(8, 1024, 128)), 16), dtype=torch.uint8, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = {k: torch.full((n,), 77, dtype=dt, device=DEV)
            for k, n, dt in (('counts', 256, torch.int32), ('means', 129 * 1056, torch.float32),
                             ('scatter', 1056 * 1056, torch.float32), ('dist2', 8, torch.float32),
                             ('cls', 8, torch.int32), ('dist_all', 8 * 129, torch.float32))}

    def moments(N, d, C, xp):
        return lib.cmhar_class_moments(0, N, d, C, xp, d, y.data_ptr(), outs['counts'].data_ptr(),
                                       outs['means'].data_ptr(), outs['scatter'].data_ptr(), ws.data_ptr(), st)

    def dist(N, d, C, xp):
        return lib.cmhar_class_min_dist(0, N, d, C, xp, d, Wm.data_ptr(), d, Wm.data_ptr(), d,
                                        outs['dist2'].data_ptr(), outs['cls'].data_ptr(),
                                        outs['dist_all'].data_ptr(), max(C, 1), st)
    invalid = 1                                                           # hipErrorInvalidValue
    for N, d, C, off in ((8, 48, 4, 0), (8, 1056, 4, 0), (8, 64, 0, 0), (8, 64, 129, 0), (0, 64, 4, 0),
                         (8, 64, 4, 4)):
        assert moments(N, d, C, x.data_ptr() + off) == invalid, (N, d, C, off)
        assert dist(N, d, C, x.data_ptr() + off) == invalid, (N, d, C, off)
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in outs.values())
    assert moments(8, 64, 4, x.data_ptr()) == 0 and dist(8, 64, 4, x.data_ptr()) == 0      # accepted, for contrast
    torch.cuda.synchronize()
    # x = 1, W = 1, m = 1: z_j = 64 and D = 64 · 63²
    assert outs['counts'][:4].tolist() == [8, 0, 0, 0] and bool((outs['dist2'] == 64 * 63 * 63).all())


def test_python_refusals():
    from cmhar.ood import class_min_dist, class_moments
    x = torch.ones(8, 64, device=DEV)
    W = torch.eye(64, device=DEV)
    m = torch.ones(3, 64, device=DEV)
    y = torch.zeros(8, dtype=torch.int64)
    for args in ((x[0], W, m), (x.cpu(), W, m), (x, W[:32], m), (x, torch.ones(64, 96, device=DEV), m),
                 (x, W, torch.ones(3, 32, device=DEV)), (x, W.bfloat16(), m), (x, W, m.half()), (x, W.cpu(), m),
                 (torch.ones(8, 48, device=DEV), torch.eye(48, device=DEV), torch.ones(3, 48, device=DEV)),
                 (x.int(), W, m), (x, W, torch.ones(129, 64, device=DEV))):
        with pytest.raises(ValueError):
            class_min_dist(*args)
    for args in ((x[0], y, 3), (x.cpu(), y, 3), (x, y, 0), (x, y, 129), (x, y[:5], 3), (x, y.float(), 3),
                 (torch.ones(8, 48, device=DEV), y, 3)):
        with pytest.raises(ValueError):
            class_moments(*args)
