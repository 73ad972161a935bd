"""Fused similarity top-k kernel (`cmhar_sim_topk`, csrc/sim_topk.hip) through `cmhar.retrieval.sim_topk`.

No reference counterpart (the reference has neither retrieval nor k-NN code), so the kernel is checked against an
fp64 restatement written here: scores q·bᵀ in fp64 on the (already rounded) inputs, ordered by (−score, index).
With small-integer operands every dot product is exact in fp32 in any summation order, so values AND indices must be
equal, ties (plentiful there) included; with random floats the bound is the fp32 recursive-summation bound."""
import ctypes
import functools

import pytest
import torch

DEV = 'cuda'
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
pytestmark = pytest.mark.gpu


def _int_operands(nq, nb, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-2, 3, (nq, d), generator=g).float(), torch.randint(-2, 3, (nb, d), generator=g).float())


def _ref_topk(q, b, k, self_offset=None):
    """fp64 scores sorted by (−score, index): a stable sort of −s keeps equal scores in ascending index."""
    s = q.double() @ b.double().T
    if self_offset is not None:
        i = torch.arange(q.shape[0])
        j = i + self_offset
        ok = j < b.shape[0]
        s[i[ok], j[ok]] = -float('inf')
    v, ix = torch.sort(-s, dim=1, stable=True)
    return -v[:, :k], ix[:, :k]


def _check_exact(vals, idx, q, b, k, self_offset=None):
    wv, wi = _ref_topk(q, b, k, self_offset)
    assert vals.dtype == torch.float32 and idx.dtype == torch.int64 and vals.shape == idx.shape == (q.shape[0], k)
    assert torch.equal(idx.cpu(), wi)
    assert torch.equal(vals.cpu().double(), wv)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nq,nb,d,k', [(1, 1, 32, 1), (17, 63, 32, 5), (130, 1000, 256, 10), (64, 4099, 768, 64),
                                       (3, 64, 1024, 64)])
def test_exact_integer_operands(dtype, nq, nb, d, k):
    from cmhar.retrieval import sim_topk
    q, b = _int_operands(nq, nb, d, 1000 * nq + nb)
    vals, idx = sim_topk(q.to(DEV, dtype), b.to(DEV, dtype), k)
    _check_exact(vals, idx, q, b, k)


@pytest.mark.parametrize('dtype', DTYPES)
def test_exact_strided_rows(dtype):
    """Both operands are column slices of wider tensors (row strides 320 and 288 for d = 256)."""
    from cmhar.retrieval import sim_topk
    q, b = _int_operands(70, 300, 256, 7)
    qw = torch.full((70, 320), 9.0)
    bw = torch.full((300, 288), 9.0)
    qw[:, :256], bw[:, :256] = q, b
    qv, bv = qw.to(DEV, dtype)[:, :256], bw.to(DEV, dtype)[:, :256]
    assert qv.stride(0) == 320 and bv.stride(0) == 288
    vals, idx = sim_topk(qv, bv, 10)
    _check_exact(vals, idx, q, b, 10)


@functools.lru_cache(maxsize=None)
def _split_case():
    q, b = _int_operands(16, 50000, 32, 11)
    return q, b, _ref_topk(q, b, 64)


def test_split_merge_exact():
    """The only path where the tie rule crosses workgroups: several bank ranges, merged by the second kernel."""
    from cmhar import _lib
    from cmhar.retrieval import sim_topk
    assert _lib.lib().cmhar_sim_topk_splits(16, 50000, 64) > 1
    assert _lib.lib().cmhar_sim_topk_ws(16, 50000, 64) > 0
    q, b, (wv, wi) = _split_case()
    vals, idx = sim_topk(q.to(DEV), b.to(DEV), 64)
    assert torch.equal(idx.cpu(), wi) and torch.equal(vals.cpu().double(), wv)


def test_deterministic():
    from cmhar.retrieval import sim_topk
    q, b, _ = _split_case()
    qd, bd = q.to(DEV), b.to(DEV)
    v1, i1 = sim_topk(qd, bd, 64)
    v2, i2 = sim_topk(qd, bd, 64)
    assert torch.equal(v1, v2) and torch.equal(i1, i2)


@functools.lru_cache(maxsize=None)
def _float_case(dtype):
    g = torch.Generator().manual_seed(5)
    q = torch.randn(300, 256, generator=g).to(dtype)
    b = torch.randn(5000, 256, generator=g).to(dtype)
    qd, bd = q.double(), b.double()
    s64 = qd @ bd.T
    tol = 256 * 2.0 ** -23 * (qd.abs() @ bd.abs().T).max(1).values     # twice the fp32 recursive-summation bound
    return q, b, s64, tol


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('k', [1, 64])
def test_random_floats(dtype, k):
    from cmhar.retrieval import sim_topk
    q, b, s64, tol = _float_case(dtype)
    vals, idx = sim_topk(q.to(DEV), b.to(DEV), k)
    vals, idx = vals.cpu().double(), idx.cpu()
    assert bool((vals[:, 1:] <= vals[:, :-1]).all())                     # non-increasing
    assert bool(((idx >= 0) & (idx < 5000)).all())
    assert all(len(set(r.tolist())) == k for r in idx)                   # distinct
    got = s64.gather(1, idx)
    err = (vals - got).abs()
    print(f'max |vals - s64| / tol = {(err / tol[:, None]).max().item():.3f}')
    assert bool((err <= tol[:, None]).all())
    kth = s64.topk(k, dim=1).values[:, -1]
    assert bool((got >= (kth - 2 * tol)[:, None]).all())


def test_self_exclusion():
    from cmhar.retrieval import sim_topk
    g = torch.Generator().manual_seed(9)
    bank = torch.nn.functional.normalize(torch.randn(400, 64, generator=g), dim=1).to(DEV)
    own = torch.arange(100, 164, device=DEV)
    _, idx = sim_topk(bank[100:164], bank, 1, self_offset=100)
    assert not bool((idx[:, 0] == own).any())
    _, idx = sim_topk(bank[100:164], bank, 1)
    assert torch.equal(idx[:, 0], own)
    # leave-one-out of the whole bank: equal to the reference with the diagonal removed
    vals, idx = sim_topk(bank, bank, 3, self_offset=0)
    wv, wi = _ref_topk(bank.cpu(), bank.cpu(), 3, self_offset=0)
    assert torch.equal(idx.cpu(), wi) and torch.allclose(vals.cpu().double(), wv, atol=1e-6, rtol=0)


def _raw(dtype_code, nq, nb, d, k, q, b, self_offset=-1):
    from cmhar import _lib
    lib = _lib.lib()
    vals = torch.zeros(max(nq, 1) * 65, dtype=torch.float32, device=DEV)
    idx = torch.zeros(max(nq, 1) * 65, dtype=torch.int32, device=DEV)
    ws = torch.zeros(max(int(lib.cmhar_sim_topk_ws(nq, nb, max(1, min(k, 64)))), 16), dtype=torch.uint8, device=DEV)
    return lib.cmhar_sim_topk(dtype_code, nq, nb, d, k, q.data_ptr(), q.stride(0), b.data_ptr(), b.stride(0),
                              self_offset, vals.data_ptr(), idx.data_ptr(), ws.data_ptr(),
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_refusals_launch_nothing():
    from cmhar.retrieval import sim_topk
    q = torch.ones(8, 64, device=DEV)
    b = torch.ones(20, 64, device=DEV)
    q48, b48 = torch.ones(8, 48, device=DEV), torch.ones(20, 48, device=DEV)
    for args, kw in (((q48, b48, 1), {}), ((q, b, 0), {}), ((q, b, 65), {}), ((q, b[:5], 6), {}),
                     ((q, b[:5], 5), {'self_offset': 0}), ((q, b.bfloat16(), 1), {}),
                     ((q.int(), b.int(), 1), {})):
        with pytest.raises(ValueError):
            sim_topk(*args, **kw)
    assert _raw(0, 8, 20, 64, 1, q, b) == 0                               # the accepted call, for contrast
    assert _raw(0, 8, 20, 48, 1, q48, b48) != 0                           # d = 48
    assert _raw(0, 8, 20, 64, 0, q, b) != 0                               # k = 0
    assert _raw(0, 8, 20, 64, 65, q, b) != 0                              # k = 65
    assert _raw(0, 8, 5, 64, 6, q, b) != 0                                # k = nb + 1
    assert _raw(0, 8, 5, 64, 5, q, b, self_offset=0) != 0                 # k = nb with self-exclusion
    assert _raw(3, 8, 20, 64, 1, q, b) != 0                               # not a dtype code
    torch.cuda.synchronize()
