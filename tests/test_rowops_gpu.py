"""Norm, reduction and data-movement kernels (csrc/norm.hip, csrc/rowops.h, csrc/misc.hip) against fp64 references at
the shapes where their dispatch changes: LayerNorm forward / backward (vector and generic kernels, both grid-stride
rounds, the three partial-row reducers), `cmhar_colsum`, BatchNorm1d, L2-normalise, `copy2d` and the IMU patch
embedding.  The loss kernels are in tests/test_loss_kernels_gpu.py.

Every reference is plain torch in fp64, evaluated on the values the kernel read (16-bit inputs widened after their
rounding).  Tolerances are the project's (tests/test_kernels_gpu.py): `rel(a, b) = ‖a−b‖/‖b‖ ≤ 1e-5` for fp32 kernels;
16-bit outputs are fp32 math plus one output rounding, `≤ 8e-3` for bf16 and `≤ 1e-3` for fp16 (10-bit mantissa).
Cancelling column sums (dγ, dβ, colsum, BatchNorm dw / db) are measured against the fp64 sum of term magnitudes,
`‖got − ref‖ / ‖Σ|terms|‖ ≤ 1e-5` (`relmag`).  Exact arithmetic (h_out = a + b, db_out = dh, power-of-two copies, integer
outputs, gradients that must be zero) is compared with `torch.equal`.  Every output buffer is prefilled with NaN (or
an integer sentinel) so a missed write fails the comparison; strided views come from wider NaN-filled allocations
whose padding must still be NaN afterwards.  Dropout is not covered here (pdrop = 0 throughout)."""
import pytest
import torch
import torch.nn.functional as F

DEV = 'cuda'
pytestmark = pytest.mark.gpu
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
TOL = {F32: 1e-5, BF16: 8e-3, F16: 1e-3}
NAN = float('nan')


def K():
    from cmhar import kernels
    return kernels


def L():
    from cmhar import _lib
    return _lib


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def relmag(got, ref, mag):
    """‖got − ref‖ / ‖Σ|terms|‖ for sums that cancel."""
    return ((got.double() - ref).norm() / mag.norm().clamp_min(1e-30)).item()


def nans(*shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def padded(t, pad):
    """A [:, :N] view (row stride N + pad) of a NaN-filled allocation holding t; returns (view, allocation)."""
    M, N = t.shape
    w = nans(M, N + pad, dtype=t.dtype)
    v = w[:, :N]
    v.copy_(t)
    return v, w


def pad_intact(w, N):
    return bool(torch.isnan(w[:, N:]).all())


def _name(dt):
    return {F32: 'f32', BF16: 'bf16', F16: 'f16'}[dt]


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm forward.  Rows have mean 50 (fp32) / 4 (16-bit) and std 1: a one-pass E[x²] − E[x]² variance would fail.
# ---------------------------------------------------------------------------------------------------------------
def _rows(M, N, dt, seed, offset=None):
    g = torch.Generator().manual_seed(seed)
    if offset is None:
        offset = 50.0 if dt == F32 else 4.0
    return (offset + torch.randn(M, N, generator=g)).to(DEV, dt)


def _affine(N, seed):
    g = torch.Generator().manual_seed(seed)
    return (1 + 0.1 * torch.randn(N, generator=g)).to(DEV), (0.1 * torch.randn(N, generator=g)).to(DEV)


def _ln_fwd_check(dt, M, N, *, with_b=False, with_h=False, pad_in=0, pad_out=0, eps=1e-5):
    a, aw = padded(_rows(M, N, dt, 11 * M + N), pad_in)
    b = bw = None
    if with_b:
        b, bw = padded(_rows(M, N, dt, 13 * M + N, offset=0.0), pad_in)
    gamma, beta = _affine(N, N)
    y, yw = padded(nans(M, N, dtype=dt), pad_out)
    h = hw = None
    if with_h:
        h, hw = padded(nans(M, N, dtype=dt), pad_out)
    mean, rstd = nans(M), nans(M)
    K().layernorm_fwd(a, gamma, beta, eps, b=b, h_out=h, out=y, mean=mean, rstd=rstd)
    s64 = a.double() + (b.double() if with_b else 0.0)
    ref = F.layer_norm(s64, (N,), gamma.double(), beta.double(), eps)
    ey, em = rel(y, ref), rel(mean, s64.mean(1))
    er = rel(rstd, 1 / (s64.var(1, unbiased=False) + eps).sqrt())
    print(f'ln_fwd {_name(dt)} M={M} N={N}: y {ey:.2e} mean {em:.2e} rstd {er:.2e}')
    assert ey <= TOL[dt]
    assert em <= 1e-6 and er <= 1e-5
    if with_h:      # pdrop = 0: the fp32 sum, rounded once to the storage type
        assert torch.equal(h, (a.float() + b.float()).to(dt))
    for w in (aw, bw, yw, hw):
        assert w is None or pad_intact(w, N)
    return y, mean, rstd


@pytest.mark.parametrize('dt', [F32, BF16], ids=_name)
@pytest.mark.parametrize('M', [1, 9, 333])
@pytest.mark.parametrize('N', [256, 512, 768, 1024])
def test_ln_fwd_vector(dt, M, N):
    """ln_fwd_vec_kernel<T, G>, G = N/256 = 1..4 (N = 512 is G = 2), one grid-stride round."""
    _ln_fwd_check(dt, M, N, eps=1e-12 if N == 768 else 1e-5)


@pytest.mark.parametrize('M', [1, 9, 333])
def test_ln_fwd_vector_fp16(M):
    _ln_fwd_check(F16, M, 768, eps=1e-12)


@pytest.mark.parametrize('dt', [F32, BF16], ids=_name)
@pytest.mark.parametrize('M,N', [(6155, 256), (4107, 1024)])
def test_ln_fwd_vector_second_round(dt, M, N):
    """More rows than the grid's waves (768 blocks × 8 for N ≤ 768, 512 × 8 for N = 1024): the second grid-stride
    iteration with its register prefetch, ending in a ragged tail (11 rows)."""
    _ln_fwd_check(dt, M, N)


@pytest.mark.parametrize('dt', [F32, BF16], ids=_name)
@pytest.mark.parametrize('M', [1, 5, 70])
@pytest.mark.parametrize('N', [1, 63, 100, 128, 130, 1000])
def test_ln_fwd_generic(dt, M, N):
    """ln_fwd_kernel (one wave per row, lane + 64i columns): N below a wave, no multiple of 64, near the 1024 cap."""
    y, _, rstd = _ln_fwd_check(dt, M, N)
    if N == 1:      # a one-column row is its own mean: y = beta and rstd = rsqrt(eps), finite
        _, beta = _affine(1, 1)
        assert torch.equal(y, beta.to(dt).expand(M, 1))
        assert bool(torch.isfinite(rstd).all()) and rel(rstd, torch.full((M,), 1e-5 ** -0.5, device=DEV)) <= 1e-5


@pytest.mark.parametrize('N', [100, 256])
def test_ln_fwd_generic_fp16(N):
    _ln_fwd_check(F16, 70, N, with_b=True, with_h=True)


@pytest.mark.parametrize('dt', [F32, BF16], ids=_name)
@pytest.mark.parametrize('with_h', [False, True], ids=['b', 'b+h_out'])
@pytest.mark.parametrize('M,N', [(70, 256), (5, 100)])
def test_ln_fwd_residual_add(dt, with_h, M, N):
    """`b` (and `h_out`) force the generic kernel at N = 256; h_out is exact."""
    _ln_fwd_check(dt, M, N, with_b=True, with_h=with_h)


@pytest.mark.parametrize('dt', [F32, BF16], ids=_name)
def test_ln_fwd_unaligned_stride_falls_back(dt):
    """Row strides N + 2 (fp32) / N + 6 (bf16) are no multiple of 4 elements: the generic kernel takes N = 256."""
    pad = 2 if dt == F32 else 6
    _ln_fwd_check(dt, 70, 256, pad_in=pad, pad_out=pad)
    _ln_fwd_check(dt, 70, 256, with_b=True, with_h=True, pad_in=pad, pad_out=pad)


@pytest.mark.parametrize('dt', [F32, BF16, F16], ids=_name)
def test_ln_fwd_vector_strided_views(dt):
    """Row stride N + 8 keeps the vector kernel (4-element aligned rows); input and output strides differ."""
    _ln_fwd_check(dt, 70, 256, pad_in=8, pad_out=16)


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm backward: h, mean, rstd from the forward under test; the reference differentiates fp64 layer_norm of the
# same h.  Each case runs (dres, beta_acc = 0 over NaN-filled dγ / dβ) and (no dres, beta_acc = 1 over known values).
# ---------------------------------------------------------------------------------------------------------------
def _ln_bwd_check(dt, M, N, *, db_out=False, pad_dy=0, eps=1e-5):
    h = _rows(M, N, dt, 17 * M + N, offset=10.0 if dt == F32 else 4.0)      # a residual stream off zero, std 1
    gamma, beta = _affine(N, N + 1)
    _, mean, rstd = K().layernorm_fwd(h, gamma, beta, eps)
    g = torch.Generator().manual_seed(19 * M + N)
    dy, dyw = padded(torch.randn(M, N, generator=g).to(DEV, dt), pad_dy)
    dres = torch.randn(M, N, generator=g).to(DEV, dt)
    g0, b0 = torch.randn(N, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)
    h64 = h.double().requires_grad_(True)
    gam64, bet64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    gx, gg, gb = torch.autograd.grad(F.layer_norm(h64, (N,), gam64, bet64, eps), (h64, gam64, bet64), dy.double())
    hd = h.double()
    xhat = (hd - hd.mean(1, keepdim=True)) / (hd.var(1, unbiased=False, keepdim=True) + eps).sqrt()
    mag_g, mag_b = (dy.double() * xhat).abs().sum(0), dy.double().abs().sum(0)
    for use_dres, beta_acc in ((True, 0.0), (False, 1.0)):
        dgam = g0.clone() if beta_acc else nans(N)
        dbet = b0.clone() if beta_acc else nans(N)
        dh = nans(M, N, dtype=dt)
        dbo = nans(M, N, dtype=dt) if db_out else None
        K().layernorm_bwd(dy, h, gamma, mean, rstd, dgam, dbet, dres=dres if use_dres else None, dh=dh, db_out=dbo,
                          beta_acc=beta_acc)
        eh = rel(dh, gx + dres.double() if use_dres else gx)
        eg = relmag(dgam, gg + beta_acc * g0.double(), mag_g + beta_acc * g0.double().abs())
        eb = relmag(dbet, gb + beta_acc * b0.double(), mag_b + beta_acc * b0.double().abs())
        print(f'ln_bwd {_name(dt)} M={M} N={N} dres={use_dres} beta_acc={beta_acc}: dh {eh:.2e} dgamma {eg:.2e} '
              f'dbeta {eb:.2e}')
        assert eb <= 1e-5
        # N = 1: x̂ = 0 and g − mean(g) = 0, so dh is the residual gradient alone and dγ gets nothing: compared bitwise
        # (the fp64 autograd of a one-column row leaves ~1e-13 where the value is 0: nothing to measure against)
        assert (eh <= TOL[dt] and eg <= 1e-5) or N == 1
        if N == 1:
            assert torch.equal(dh, dres if use_dres else torch.zeros_like(dh))
            assert torch.equal(dgam, g0 if beta_acc else torch.zeros_like(dgam))
        if db_out:     # pdrop = 0: the dropout-branch gradient is the same value, stored again
            assert torch.equal(dbo, dh)
    assert pad_intact(dyw, N)


@pytest.mark.parametrize('dt', [F32, BF16], ids=_name)
@pytest.mark.parametrize('M', [1, 333])
@pytest.mark.parametrize('N', [256, 512, 768, 1024])
def test_ln_bwd_vector(dt, M, N):
    """ln_bwd_vec_kernel<T, G>; 1 and 42 partial rows: colsum_final2_kernel, and colsum_rows2_kernel's tail loop."""
    _ln_bwd_check(dt, M, N)


@pytest.mark.parametrize('dt', [F32, BF16], ids=_name)
@pytest.mark.parametrize('M,N', [(1100, 256), (4107, 512)])
def test_ln_bwd_vector_many_rows(dt, M, N):
    """(1100, 256): 138 partial rows, colsum_rows2_kernel's 8-way unrolled loop (needs ≥ 128).  (4107, 512): more rows
    than the 512 × 8 waves, the second grid-stride round of the vector kernel with its prefetch."""
    _ln_bwd_check(dt, M, N)


@pytest.mark.parametrize('M', [1, 13, 70])
@pytest.mark.parametrize('N', [1, 63, 128])
def test_ln_bwd_generic_mp2(M, N):
    """fp32 N ≤ 128: ln_bwd_kernel<float, 2> (two columns per lane)."""
    _ln_bwd_check(F32, M, N)


@pytest.mark.parametrize('dt,N', [(F32, 130), (F32, 1000), (BF16, 100), (BF16, 128)],
                         ids=['f32-130', 'f32-1000', 'bf16-100', 'bf16-128'])
@pytest.mark.parametrize('M', [1, 13, 70])
def test_ln_bwd_generic_mp16(dt, N, M):
    """ln_bwd_kernel<T, 16>: fp32 above 128 columns, and every bf16 width the vector kernel does not take."""
    _ln_bwd_check(dt, M, N)


@pytest.mark.parametrize('dt', [F32, BF16], ids=_name)
@pytest.mark.parametrize('how', ['db_out', 'dy_stride'])
def test_ln_bwd_forced_generic_at_256(dt, how):
    """N = 256 leaves the vector kernel when db_out is requested or when dy's row stride (N + 2) is unaligned."""
    _ln_bwd_check(dt, 70, 256, db_out=how == 'db_out', pad_dy=2 if how == 'dy_stride' else 0)


@pytest.mark.parametrize('M,N', [(8200, 96), (65600, 64)])
def test_ln_bwd_partial_row_reducers(M, N):
    """Generic kernel, one partial row per 64 rows.  (8200, 96): 129 partial rows, colsum_rows2_kernel's unrolled loop.
    (65600, 64): 1025 partial rows, past RR1_MAX: colsum_partial_kernel then colsum_final2_kernel."""
    _ln_bwd_check(F32, M, N)


def test_ln_bwd_rejects_fp16():
    """fp16 is the inference-only path: the backward returns -1 before any launch and writes nothing."""
    M, N = 9, 256
    h = _rows(M, N, F16, 3)
    gamma, _ = _affine(N, 3)
    dy = torch.ones(M, N, dtype=F16, device=DEV)
    mean, rstd = torch.zeros(M, device=DEV), torch.ones(M, device=DEV)
    dh = torch.full((M, N), 7.0, dtype=F16, device=DEV)
    dgam, dbet = torch.full((N,), 5.0, device=DEV), torch.full((N,), 6.0, device=DEV)
    with pytest.raises(RuntimeError):
        K().layernorm_bwd(dy, h, gamma, mean, rstd, dgam, dbet, dh=dh)
    torch.cuda.synchronize()
    assert bool((dh == 7.0).all()) and bool((dgam == 5.0).all()) and bool((dbet == 6.0).all())


# ---------------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------------
_AB = [(1.0, 0.0), (0.5, 1.0), (-2.0, 0.25)]


def _colsum_check(x, xw=None):
    M, N = x.shape
    g = torch.Generator().manual_seed(M + N)
    o0 = torch.randn(N, generator=g).to(DEV)
    x64 = x.double()
    for alpha, beta in _AB:
        out = o0.clone() if beta else nans(N)       # beta = 0 must overwrite a dirty (NaN) output
        K().colsum(x, out, alpha=alpha, beta=beta)
        ref = alpha * x64.sum(0) + beta * o0.double()
        mag = abs(alpha) * x64.abs().sum(0) + abs(beta) * o0.double().abs()
        e = relmag(out, ref, mag)
        print(f'colsum {_name(x.dtype)} M={M} N={N} ld={x.stride(0)} alpha={alpha} beta={beta}: {e:.2e}')
        assert e <= 1e-5
    assert xw is None or pad_intact(xw, N)


@pytest.mark.parametrize('dt', [F32, BF16], ids=_name)
@pytest.mark.parametrize('M', [1, 7, 256, 257, 5000])
@pytest.mark.parametrize('N', [1, 63, 256, 301])
def test_colsum(dt, M, N):
    """M ≤ 256: ≤ 32 chunks, reduced by colsum_final_kernel alone (the head bias gradients at M = batch rows); 257: 33
    chunks, the two-level reduce; 5000: 64 chunks.  N = 256: float4 / bf16x4 lanes; N = 1, 63, 301 contiguous: ldx is
    no multiple of 4, the scalar fallback."""
    g = torch.Generator().manual_seed(M * 1000 + N)
    _colsum_check(torch.randn(M, N, generator=g).to(DEV, dt))


@pytest.mark.parametrize('dt', [F32, BF16], ids=_name)
@pytest.mark.parametrize('N,pad', [(256, 4), (256, 2), (301, 3)], ids=['vector', 'scalar', 'mixed'])
def test_colsum_strided(dt, N, pad):
    """ldx = N + 4: vector lanes on a view; N + 2: scalar fallback; N = 301 with ldx = 304: the lane holding column
    300 takes the scalar path next to vector lanes."""
    g = torch.Generator().manual_seed(N + pad)
    x, xw = padded(torch.randn(300, N, generator=g).to(DEV, dt), pad)
    _colsum_check(x, xw)


def test_colsum_rejects_fp16():
    x = torch.ones(7, 64, dtype=F16, device=DEV)
    out = torch.full((64,), 5.0, device=DEV)
    with pytest.raises(RuntimeError):
        K().colsum(x, out)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())


# ---------------------------------------------------------------------------------------------------------------
# BatchNorm1d (+ ReLU): inputs with mean 30 and std 0.5
# ---------------------------------------------------------------------------------------------------------------
def _bn_ref(x64, w64, b64, mu, var, eps, relu):
    y = (x64 - mu) / (var + eps).sqrt() * w64 + b64
    return torch.relu(y) if relu else y


def _bn_f32(x, w, b, dy, mu, var, training, relu, eps):
    """The kernels' formulas in plain fp32 torch on the CPU: (y, dx, dw), for the fp32 floor of an input."""
    x, w, b, dy = (t.cpu() for t in (x, w, b, dy))
    B = x.shape[0]
    if training:
        mu = x.mean(0)
        var = ((x - mu) ** 2).mean(0)
    r = (var.cpu() + eps).rsqrt()
    xh = (x - mu.cpu()) * r
    y = xh * w + b
    g = dy * (y > 0) if relu else dy
    sg, sgx = g.sum(0), (g * xh).sum(0)
    dx = w * r * (g - sg / B - xh * sgx / B) if training else w * r * g
    return (torch.relu(y) if relu else y), dx, sgx


@pytest.mark.parametrize('relu', [0, 1], ids=['norelu', 'relu'])
@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('B', [2, 5, 32])
@pytest.mark.parametrize('C', [1, 127, 130, 512])
def test_batchnorm(C, B, training, relu):
    """C = 1, 127, 130: ragged 128-thread blocks.  Training: batch statistics, running statistics for momentum 0.1 and
    1.0, the counter; eval: running statistics, nothing else written.  Backward against autograd, beta_acc = 0 and 1.

    y, dx and dw carry x̂ = (x − μ)/σ, and with a batch of 2 to 5 rows of mean 30 a column's σ can be a hundredth of the
    spread while μ is only good to ulp(30)/2 ≈ 1e-6: fp32 itself cannot reach 1e-5 there.  Plain fp32 torch on the CPU
    (`_bn_f32`, the same formulas) against the fp64 reference gives, for these inputs: B = 2 training y 5.8e-6 … 2.2e-5,
    dw (over Σ|terms|) 5.5e-6 … 3.0e-5 and dx 1.0e-4 … 6.2e-2 (with two rows dx is the eps-sized remainder of terms that
    cancel), B = 5 training y and dx up to 4.7e-6, every other case ≤ 1e-6.  So each of the three bounds is 1e-5, or 4× the fp32 floor of that exact input
    where that is larger (the factor covers another summation order and the hardware rsqrt); the floor is computed from
    torch, never from the kernel's output."""
    eps = 1e-5
    g = torch.Generator().manual_seed(100 * C + B)
    x = (30 + 0.5 * torch.randn(B, C, generator=g)).to(DEV)
    w = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    b = (0.1 * torch.randn(C, generator=g)).to(DEV)
    rm0 = (30 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    rv0 = (0.25 * (1 + 0.2 * torch.rand(C, generator=g))).to(DEV)
    dy = torch.randn(B, C, generator=g).to(DEV)
    dw0, db0 = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    x64 = x.double().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    mu64 = x64.mean(0) if training else rm0.double()
    var64 = x64.var(0, unbiased=False) if training else rv0.double()
    ref = _bn_ref(x64, w64, b64, mu64, var64, eps, relu)
    gx, gw, gb = torch.autograd.grad(ref, (x64, w64, b64), dy.double())
    with torch.no_grad():
        live = (ref > 0).double() if relu else torch.ones_like(ref)
        xhat = (x64 - mu64) / (var64 + eps).sqrt()
        mag_w, mag_b = (dy.double() * live * xhat).abs().sum(0), (dy.double() * live).abs().sum(0)
    fy, fdx, fdw = _bn_f32(x, w, b, dy, rm0, rv0, training, relu, eps)
    floor_y, floor_dx = rel(fy, ref.detach().cpu()), rel(fdx, gx.cpu())
    floor_dw = relmag(fdw, gw.cpu(), mag_w.cpu())
    tol_y, tol_dx, tol_dw = (max(1e-5, 4 * f) for f in (floor_y, floor_dx, floor_dw))
    print(f'bn B={B} C={C} train={training} relu={relu}: fp32 floors y {floor_y:.2e} dx {floor_dx:.2e} dw {floor_dw:.2e}')
    for momentum in ((0.1, 1.0) if training else (0.1,)):
        rm, rv = rm0.clone(), rv0.clone()
        nbt = torch.tensor(7, dtype=torch.int64, device=DEV)
        y, sm, sr = K().batchnorm_fwd(x, w, b, rm, rv, training, momentum, eps, relu, nbt, out=nans(B, C))
        ey, em = rel(y, ref), rel(sm, mu64)
        er = rel(sr, 1 / (var64 + eps).sqrt())
        print(f'bn_fwd B={B} C={C} train={training} relu={relu} m={momentum}: y {ey:.2e} smean {em:.2e} srstd {er:.2e}')
        assert ey <= tol_y and em <= 1e-6 and er <= 1e-5
        if training:
            want_m = (1 - momentum) * rm0.double() + momentum * mu64
            want_v = (1 - momentum) * rv0.double() + momentum * var64 * B / (B - 1)
            assert rel(rm, want_m) <= 1e-6 and rel(rv, want_v) <= 1e-5
            assert nbt.item() == 8
        else:
            assert torch.equal(rm, rm0) and torch.equal(rv, rv0) and nbt.item() == 7
    for beta_acc in (0.0, 1.0):
        dw = dw0.clone() if beta_acc else nans(C)
        db = db0.clone() if beta_acc else nans(C)
        dx, dw, db = K().batchnorm_bwd(x, y, dy, w, sm, sr, training, relu, beta_acc=beta_acc, dw=dw, db=db)
        ex = rel(dx, gx)
        ew = relmag(dw, gw + beta_acc * dw0.double(), mag_w + beta_acc * dw0.double().abs())
        eb = relmag(db, gb + beta_acc * db0.double(), mag_b + beta_acc * db0.double().abs())
        print(f'bn_bwd B={B} C={C} train={training} relu={relu} beta_acc={beta_acc}: dx {ex:.2e} dw {ew:.2e} db {eb:.2e}')
        assert ex <= tol_dx and ew <= tol_dw and eb <= 1e-5


# ---------------------------------------------------------------------------------------------------------------
# L2 normalise
# ---------------------------------------------------------------------------------------------------------------
L2_EPS = 1e-12


def _l2_check(x):
    M, N = x.shape
    g = torch.Generator().manual_seed(M * 7 + N)
    dy = torch.randn(M, N, generator=g).to(DEV)
    x64 = x.double().requires_grad_(True)
    ref = F.normalize(x64, dim=1, eps=L2_EPS)
    n64 = x64.detach().norm(dim=1)
    y, nrm = K().l2normalize_fwd(x, L2_EPS)
    ey = rel(y, ref)
    en = ((nrm.double() - n64).abs() / n64.clamp_min(1e-300)).max().item()
    assert ey <= 1e-5 and en <= 1e-5, (ey, en)
    zero = n64 == 0
    assert bool((y[zero] == 0).all()) and bool((nrm[zero] == 0).all())
    (gx,) = torch.autograd.grad(ref, x64, dy.double())
    dx = K().l2normalize_bwd(y, dy, nrm, L2_EPS)
    # per row, against the size of the terms dy/n and y·(y·dy)/n that the gradient is the difference of (for N = 1 they
    # cancel to zero; the rows' scales differ by up to 10^18, a whole-matrix norm would see only the smallest row)
    scale = dy.double().norm(dim=1) / n64.clamp_min(L2_EPS)
    ex = ((dx.double() - gx).norm(dim=1) / scale).max().item()
    print(f'l2n M={M} N={N}: y {ey:.2e} norm {en:.2e} dx {ex:.2e}')
    assert ex <= 1e-5
    if bool(zero.any()):     # the n ≤ eps branch: the subgradient torch takes through clamp_min, dx = dy / eps
        assert rel(dx[zero], dy[zero].double() / L2_EPS) <= 1e-6


def _l2_rows(M, N, norms):
    g = torch.Generator().manual_seed(M * 31 + N)
    u = F.normalize(torch.randn(M, N, generator=g).double(), dim=1)
    return (u * torch.tensor(norms, dtype=torch.float64)[:, None]).float().to(DEV)


@pytest.mark.parametrize('M', [1, 5, 33])
@pytest.mark.parametrize('N', [1, 63, 128, 200])
def test_l2normalize(M, N):
    """Row norms from 1e-6 to 1e3; from M = 5 on, one all-zero row and one row of norm 2e-12, just above eps."""
    norms = torch.logspace(-6, 3, M).tolist() if M > 1 else [3.0]
    if M >= 5:
        norms[1], norms[2] = 0.0, 2e-12
    _l2_check(_l2_rows(M, N, norms))


@pytest.mark.parametrize('norm', [0.0, 2e-12, 0.5e-12], ids=['zero', 'above-eps', 'below-eps'])
@pytest.mark.parametrize('N', [1, 200])
def test_l2normalize_single_row_at_eps(N, norm):
    _l2_check(_l2_rows(1, N, [norm]))


# ---------------------------------------------------------------------------------------------------------------
# copy2d
# ---------------------------------------------------------------------------------------------------------------
PAIRS = [(F32, F32), (F32, BF16), (BF16, F32), (F16, F32), (F32, F16), (F16, F16), (BF16, BF16)]
_pair_id = lambda p: f'{_name(p[0])}-{_name(p[1])}'      # noqa: E731


@pytest.mark.parametrize('pair', PAIRS, ids=_pair_id)
@pytest.mark.parametrize('rows,cols', [(1, 1), (7, 301), (300, 64)])
def test_copy2d(pair, rows, cols):
    """Every dtype pair of the dispatcher, on source and destination views of unequal strides."""
    ti, to = pair
    g = torch.Generator().manual_seed(rows + cols)
    src, sw = padded(torch.randn(rows, cols, generator=g).to(DEV, ti), 5)
    d0 = torch.randn(rows, cols, generator=g).to(DEV, to)
    for alpha in (1.0, 0.5):            # exact: a power-of-two scale in fp32, one rounding to the output type
        dst, dw = padded(nans(rows, cols, dtype=to), 3)
        K().copy2d(src, dst, alpha=alpha)
        assert torch.equal(dst, (src.float() * alpha).to(to))
        assert pad_intact(dw, cols) and pad_intact(sw, cols)
    for alpha, beta in ((1.0, 1.0), (-2.0, 0.25), (0.3, -1.5)):     # accumulation: fp32 math, one output rounding
        dst, dw = padded(d0, 3)
        K().copy2d(src, dst, alpha=alpha, beta=beta)
        e = rel(dst, alpha * src.double() + beta * d0.double())
        print(f'copy2d {_pair_id(pair)} {rows}x{cols} alpha={alpha} beta={beta}: {e:.2e}')
        assert e <= TOL[to]
        assert pad_intact(dw, cols)


@pytest.mark.parametrize('dt', [F32, BF16, F16], ids=_name)
def test_copy2d_in_place(dt):
    """src is dst (heads.py scales a gradient in place)."""
    g = torch.Generator().manual_seed(3)
    t0 = torch.randn(37, 130, generator=g).to(DEV, dt)
    t, tw = padded(t0, 6)
    K().copy2d(t, t, alpha=0.5)
    assert torch.equal(t, (t0.float() * 0.5).to(dt)) and pad_intact(tw, 130)
    K().copy2d(t, t, alpha=1.0, beta=1.0)
    assert torch.equal(t, ((t0.float() * 0.5).to(dt).float() * 2).to(dt))


@pytest.mark.parametrize('pair', [(BF16, F16), (F16, BF16)], ids=_pair_id)
def test_copy2d_rejects_mixed_16bit(pair):
    src = torch.ones(4, 8, dtype=pair[0], device=DEV)
    dst = torch.full((4, 8), 3.0, dtype=pair[1], device=DEV)
    with pytest.raises(RuntimeError):
        K().copy2d(src, dst)
    torch.cuda.synchronize()
    assert bool((dst == 3.0).all())


# ---------------------------------------------------------------------------------------------------------------
# IMU patch embedding (cmhar_imu_embed_fwd / _bwd), called as cmhar/imu.py calls it
# ---------------------------------------------------------------------------------------------------------------
def _embed_ref(x, ws, bs, cls, pos, P, S):
    """fp64 unfold → per-channel Linear(P, D) → prepend CLS → + pos[:T] (the reference model's patch embedding)."""
    B, C, _ = x.shape
    patches = x.unfold(2, P, S)                                         # (B, C, N, P)
    emb = torch.stack([patches[:, c] @ ws[c].T + bs[c] for c in range(C)], 1)
    D = emb.shape[-1]
    tokens = torch.cat([cls.expand(B, 1, D), emb.reshape(B, -1, D)], 1)
    T = min(tokens.shape[1], pos.shape[0])
    return tokens[:, :T] + pos[:T]


def _embed_params(B, C, Lx, P, D, Tpos, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, Lx, generator=g)
    ws = [torch.randn(D, P, generator=g) / P ** 0.5 for _ in range(C)]
    bs = [0.1 * torch.randn(D, generator=g) for _ in range(C)]
    return x, ws, bs, torch.randn(1, 1, D, generator=g), torch.randn(Tpos, D, generator=g), g


def _embed_call_fwd(x, ws, bs, cls, pos, P, S, out, N, T):
    B, C, Lx = x.shape
    return L().call('cmhar_imu_embed_fwd', B, C, Lx, N, P, S, ws[0].shape[0], T, x.data_ptr(), K().ptr_array(ws),
                    K().ptr_array(bs), cls.data_ptr(), pos.data_ptr(), out.data_ptr(), L().stream(x.device))


@pytest.mark.parametrize('D', [24, 128])
@pytest.mark.parametrize('B,C,Lx,P,S,Tpos', [(3, 3, 40, 8, 4, 28), (3, 3, 40, 8, 4, 20), (3, 3, 40, 8, 4, 10),
                                             (3, 3, 40, 8, 4, 40), (2, 8, 96, 32, 32, 25), (1, 3, 40, 8, 4, 28)],
                         ids=['full', 'ch2-one-token', 'ch1-ch2-dead', 'long-table', 'C8-P32', 'B1'])
def test_imu_embed(B, C, Lx, P, S, Tpos, D):
    """(3, 3, 40, 8, 4): 9 patches per channel, 28 tokens.  Tpos = 20 cuts channel 2 to one token; 10 leaves channels
    1 and 2 without tokens (dw, db exact zeros); 40 > T: dpos[28:] written as exact zeros."""
    N = (Lx - P) // S + 1
    T = min(1 + C * N, Tpos)
    x, ws, bs, cls, pos, g = _embed_params(B, C, Lx, P, D, Tpos, 1000 * Tpos + D)
    dout = torch.randn(B, T, D, generator=g)
    leaves = [t.double().requires_grad_(True) for t in (cls, pos, *ws, *bs)]
    ref = _embed_ref(x.double(), leaves[2:2 + C], leaves[2 + C:], leaves[0], leaves[1], P, S)
    assert ref.shape == (B, T, D)
    grads = torch.autograd.grad(ref, leaves, dout.double())
    xd, clsd, posd, doutd = x.to(DEV), cls.to(DEV), pos.to(DEV), dout.to(DEV)
    wd, bd = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    out = nans(B * T, D)
    _embed_call_fwd(xd, wd, bd, clsd, posd, P, S, out, N, T)
    ef = rel(out.cpu().view(B, T, D), ref.detach())
    dcls, dpos = nans(1, 1, D), nans(Tpos, D)
    dws, dbs = [nans(D, P) for _ in range(C)], [nans(D) for _ in range(C)]
    L().call('cmhar_imu_embed_bwd', B, C, Lx, N, P, S, D, T, Tpos, xd.data_ptr(), doutd.data_ptr(), dcls.data_ptr(),
             dpos.data_ptr(), K().ptr_array(dws), K().ptr_array(dbs), L().stream(xd.device))
    got = [t.cpu() for t in (dcls, dpos, *dws, *dbs)]
    errs = [rel(a, b) for a, b in zip(got, grads)]
    print(f'imu_embed Tpos={Tpos} D={D}: fwd {ef:.2e} grads max {max(errs):.2e}')
    assert ef <= 1e-6
    assert max(errs) <= 1e-5
    assert torch.equal(got[0].view(D), got[1][0])                      # dcls == dpos[0] bitwise
    assert bool((got[1][T:] == 0).all())                               # table rows past the used length
    for c in range(C):
        if 1 + c * N >= T:                                             # channel without live tokens
            assert bool((got[2 + c] == 0).all()) and bool((got[2 + C + c] == 0).all())


def test_imu_embed_rejects_nine_channels():
    B, C, Lx, P, S, D = 2, 9, 40, 8, 8, 24
    N = (Lx - P) // S + 1
    T = 1 + C * N
    x, ws, bs, cls, pos, _ = _embed_params(B, C, Lx, P, D, T, 5)
    xd, clsd, posd = x.to(DEV), cls.to(DEV), pos.to(DEV)
    wd, bd = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    out = torch.full((B * T, D), 3.0, device=DEV)
    with pytest.raises(RuntimeError):
        _embed_call_fwd(xd, wd, bd, clsd, posd, P, S, out, N, T)
    dcls, dpos = torch.full((1, 1, D), 3.0, device=DEV), torch.full((T, D), 3.0, device=DEV)
    dws, dbs = [torch.full((D, P), 3.0, device=DEV) for _ in range(C)], [torch.full((D,), 3.0, device=DEV) for _ in range(C)]
    with pytest.raises(RuntimeError):
        L().call('cmhar_imu_embed_bwd', B, C, Lx, N, P, S, D, T, T, xd.data_ptr(), out.data_ptr(), dcls.data_ptr(),
                 dpos.data_ptr(), K().ptr_array(dws), K().ptr_array(dbs), L().stream(xd.device))
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((dpos == 3.0).all()) and all(bool((t == 3.0).all()) for t in dws + dbs)


def test_imu_embed_restatement_matches_oracle():
    """The fp64 restatement above against oracle/cpu_model.imu_encoder's embedding stage: with no transformer layers
    and an identity final norm the oracle returns layer_norm(embedding).  (Runs on the CPU; kept here with the tests
    that rely on it.)"""
    from oracle import cpu_model as O
    B, C, Lx, P, S, D, Tpos = 3, 3, 40, 8, 4, 24, 20
    x, ws, bs, cls, pos, _ = _embed_params(B, C, Lx, P, D, Tpos, 9)
    x, cls, pos = x.double(), cls.double(), pos.double()
    ws, bs = [w.double() for w in ws], [b.double() for b in bs]
    sd = {'imu_encoder.cls_token': cls, 'imu_encoder.pos_encoding': pos[None],
          'imu_encoder.norm.weight': torch.ones(D, dtype=torch.float64),
          'imu_encoder.norm.bias': torch.zeros(D, dtype=torch.float64)}
    for c in range(C):
        sd[f'imu_encoder.patch_embed.projections.{c}.weight'] = ws[c]
        sd[f'imu_encoder.patch_embed.projections.{c}.bias'] = bs[c]
    _, enc = O.imu_encoder(sd, x, patch_size=P, stride=S, nhead=4, num_layers=0)
    mine = F.layer_norm(_embed_ref(x, ws, bs, cls, pos, P, S), (D,), eps=1e-5)
    assert enc.shape == mine.shape == (B, Tpos, D)
    assert rel(mine, enc) <= 1e-14
