"""Every launch arm of the convolution stack (csrc/conv3d.hip: cmhar_conv3d_fwd / _fwd_split / _wgrad / _col2im /
_stem_*; csrc/cnn2d.hip: cmhar_dwconv2d_cl_* / cmhar_maxpool2d_cl_*) bit-exactly at the SMALLEST geometry that reaches
it and each of its tile edges (ragged last tile, frame boundary inside a tile, partly live Cout column groups, the
slab-fit and slot-fill thresholds between two plans, ragged statistics groups).

Integer operands (tests/conv_exact.py): every fp32 partial sum is exact in any order, so each output equals torch's
fp64 convolution / autograd after one round-to-nearest-even — bf16 outputs `==` the rounded reference, fp32 weight
gradients `==` the reference; a single wrong element fails, and the message names its (n, t, h, w, c).  Every case
asserts through the library's own plan queries that it runs the kernel it is named for BEFORE launching, and writes
into NaN-prefilled outputs (an unwritten element fails).  The kernels run through the entry points of the training
step (`cmhar/r3d.py` `_pack_all`, `_conv_fwd`, `_conv_wgrad`, `_conv_dgrad`) and, into the NaN-prefilled buffers and
for the unsplit / split forms of one geometry, through the library calls those make.

`test_conv_plan_table` needs no GPU (host-side plan queries).  DESIGN.md ("Convolution launch arms and the tests
that pin them") maps every arm to its case here."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_exact as X

DEV = 'cuda'
BF = torch.bfloat16
gpu = pytest.mark.gpu

# ---- forward: (id, cin, cout, taps, stride, pad, input (N, T, H, W), cmhar_conv3d_fwd_plan, split count) ----------
# plan 1 = nine-tap conv3d_fwd_rows3, 2 = conv3d_fwd_rows<128>, 3 = conv3d_fwd_rows<256>, 4 = conv3d_fwd_igemm 128x64,
# 5 = conv3d_fwd_igemm 128x128; split count > 0: the step takes cmhar_conv3d_fwd_split (rows<128> for plan 2, the
# igemm kernels over K for plans 4 / 5) — those cases run the unsplit kernel directly as well.
K133, P011 = (1, 3, 3), (0, 1, 1)
FWD = [
    # rows<256>: M = 350 = one full tile + 94 rows; tile 0 crosses the frame boundary at row 175; Wo = 25 is the first
    # width whose 128-row slab no longer fits (Wo = 24 below takes plan 2)
    ('p3-w25-rag94', 64, 64, 3, 1, 1, (1, 2, 7, 25), 3, 0),
    ('p3-two-cout-slices', 64, 128, 3, 1, 1, (1, 2, 7, 25), 3, 0),
    ('p3-kt1-eight-cin-slices', 512, 64, K133, 1, P011, (2, 1, 7, 25), 3, 0),
    ('p3-w64', 64, 64, 3, 1, 1, (1, 2, 4, 64), 3, 0),
    # rows<128>: the slab-fit boundary from below, unsplit and split 4 ways
    ('p2-w24-h7', 64, 64, 3, 1, 1, (1, 2, 7, 24), 2, 4),
    ('p2-w24-h6', 64, 64, 3, 1, 1, (1, 2, 6, 24), 2, 4),
    ('p2-7x7-frames-rag19', 64, 128, K133, 1, P011, (3, 1, 7, 7), 2, 0),
    # igemm 128x64: one ragged tile of 90 rows; Cout = 24: three of the eight column groups live
    ('p4-1x1-rag90', 128, 64, 1, 1, 0, (1, 2, 5, 9), 4, 0),
    ('p4-1x1-cout24', 256, 24, 1, 1, 0, (1, 2, 5, 9), 4, 0),
    ('p4-stride2-odd-split', 64, 64, 3, 2, 1, (1, 3, 9, 11), 4, 4),
    ('p5-stride2-split', 64, 128, 3, 2, 1, (2, 6, 11, 10), 5, 4),
    # Cout = 72: the column mask inside a 128-wide tile (the library also plans a 4-way split for it: both run)
    ('p5-cout72', 192, 72, 3, 1, 1, (1, 3, 6, 5), 5, 4),
    # nine-tap: R = 3 rows of 64 = 192 of 256 slots, exactly the 3/4-fill threshold
    ('p1-fill-threshold', 64, 64, 3, 1, 1, (1, 2, 3, 64), 1, 0),
    ('p1-tiles-8-8-8-6-three-slices', 128, 192, 3, 1, 1, (1, 2, 30, 30), 1, 0),
    # 17 and 33 statistics tiles: a ragged last group of the BN_TG = 16 merge
    ('p1-17-stat-tiles', 64, 64, 3, 1, 1, (1, 17, 3, 64), 1, 0),
    ('p1-33-stat-tiles', 64, 64, 3, 1, 1, (1, 33, 14, 14), 1, 0),
]

# ---- weight gradient: (id, cin, cout, taps, stride, pad, input, cmhar_conv3d_wgrad_plan, splits (1 = no reduce)) --
# 1 = nine-tap conv3d_wgrad_rows3, 2 = conv3d_wgrad_rows 128-wide, 3 = 64-wide, 4 = conv3d_wgrad_igemm
WGRAD = [
    ('w1', 256, 256, 3, 1, 1, (1, 3, 14, 14), 1, 1),
    ('w1+r', 128, 128, 3, 1, 1, (2, 4, 28, 28), 1, 8),
    ('w2', 64, 128, 3, 2, 1, (2, 6, 11, 10), 2, 1),
    ('w2+r7', 64, 128, 3, 1, 1, (4, 4, 7, 25), 2, 7),
    ('w3', 64, 64, 3, 1, 1, (3, 5, 9, 7), 3, 1),
    ('w3+r2', 64, 64, 3, 1, 1, (2, 3, 7, 25), 3, 2),
    ('w4', 128, 256, 1, 2, 0, (2, 4, 7, 9), 4, 1),
    ('w4+r3', 128, 64, 1, 1, 0, (2, 4, 12, 13), 4, 3),       # M = 1248: slices of 448 / 448 / 352 rows
    # the wr::SLOTS = 64 boundary: Wo = 64 keeps the nine-tap kernel, Wo = 65 falls to the generic one
    ('w-slots-64', 64, 64, 3, 1, 1, (1, 2, 3, 64), 1, 1),
    ('w-slots-65', 64, 64, 3, 1, 1, (1, 2, 3, 65), 4, 1),
]

# ---- flipped-weight input gradient: (id, cin, cout, input, plan of the flipped conv, its split count) ------------
DGRAD = [
    ('flip3', 64, 64, (1, 2, 7, 25), 3, 0),
    ('flip4-ig-split', 64, 64, (1, 3, 5, 4), 4, 4),
    ('flip2-rows-split', 64, 64, (3, 5, 9, 7), 2, 4),
    ('flip1', 128, 192, (1, 2, 30, 30), 1, 0),
]

# ---- dz·W + col2im input gradient (sparse dz): (id, cin, cout, taps, stride, pad, input, col2im3d_gather<MT>) ------
COL2IM = [
    # odd sizes under stride 2: the last input row and column sit in no window's stride phase
    ('mt2-stride2-odd', 64, 128, 3, 2, 1, (2, 5, 11, 9), 2),
    ('mt1-1x1-stride2', 128, 256, 1, 2, 0, (2, 4, 7, 9), 1),
    # Cin = 32 is no implicit-GEMM geometry: im2col + GEMM forward, GEMM weight gradient, GEMM + col2im input gradient
    ('mt3-cin32', 32, 64, 3, 1, 1, (1, 3, 6, 5), 3),
]

STEM = [(3, (3, 7, 7), (1, 2, 2), (1, 3, 3), (1, 4, 112, 112)), (3, (3, 7, 7), (1, 2, 2), (1, 3, 3), (2, 3, 30, 34)),
        (3, (1, 7, 7), (1, 2, 2), (0, 3, 3), (2, 2, 40, 36)), (2, (3, 5, 5), (2, 1, 2), (1, 2, 2), (1, 5, 20, 24)),
        (4, (2, 3, 8), (1, 2, 2), (0, 1, 3), (2, 3, 11, 120))]


def _ids(table):
    return [t[0] for t in table]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def test_conv_plan_table():
    """Every case above takes the plan it is named for (host-side queries of the library; no GPU needed)."""
    wrong = {}
    for name, cin, cout, k, s, p, shape, plan, splits in FWD:
        d = X.plan_detail(cin, cout, k, s, p, shape)
        if (d['fwd'], d['fwd_splits']) != (plan, splits):
            wrong[name] = ((d['fwd'], d['fwd_splits']), (plan, splits))
    for name, cin, cout, k, s, p, shape, plan, splits in WGRAD:
        d = X.plan_detail(cin, cout, k, s, p, shape)
        if (d['wgrad'], d['wgrad_splits'], d['wgrad_reduce']) != (plan, splits, splits > 1):
            wrong[name] = ((d['wgrad'], d['wgrad_splits']), (plan, splits))
    for name, cin, cout, shape, plan, splits in DGRAD:
        d = X.plan_detail(cin, cout, 3, 1, 1, shape)
        if (d['flip'], d['flip_splits']) != (plan, splits):
            wrong[name] = ((d['flip'], d['flip_splits']), (plan, splits))
    for name, cin, cout, k, s, p, shape, mt in COL2IM:
        if X.plans(cin, cout, k, s, p, shape)[1] != 'col2im' and cin % 64 == 0:
            wrong[name] = X.plans(cin, cout, k, s, p, shape)
    assert not wrong, wrong
    # the slot boundary of the nine-tap weight gradient leaves the forward on the nine-tap kernel
    assert X.plans(64, 64, 3, 1, 1, (1, 2, 3, 65)) == (1, 'flip:1', '4')
    assert X.plans(64, 64, 3, 1, 1, (1, 2, 3, 64)) == (1, 'flip:1', '1')
    # and the plan helper is the production test's
    assert X.plans(64, 128, 3, 2, 1, (32, 16, 56, 56)) == (5, 'col2im', '2+r')


# ------------------------------------------------------------------------------------------------------------------
def _device_case(c, flip=False):
    """The case's operands on the GPU and the step's weight packs (cmhar.r3d._pack_all: one launch)."""
    from cmhar import r3d
    conv = X.conv3d(c.cin, c.cout, c.k, c.s, c.p).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(c.conv.weight)
    packs = r3d._pack_all([(conv, flip)], BF, torch.device(DEV))[conv]
    wp, wf = packs if flip else (packs, None)
    x = c.x.to(DEV)
    shp = tuple(x.shape)
    dims = r3d._dims(shp, conv, wp.shape[1])
    rows = r3d._r8(c.M)
    dz = torch.zeros(rows, c.cout, dtype=BF, device=DEV)       # the step's layout: rows past M zero
    dz[:c.M] = c.dz.reshape(c.M, c.cout).to(DEV)
    return conv, x, shp, dims, wp, wf, dz


def _unit(c, conv, x, shp, wp, wf, col, igemm, stem=False):
    from cmhar import r3d
    u = r3d._Unit()
    u.conv, u.shape, u.oshape, u.Kp, u.rows, u.wp = conv, shp, c.oshape, r3d._r8(conv.weight[0].numel()), \
        r3d._r8(c.M), wp
    u.x, u.col, u.igemm, u.wf, u.stem = x, col, igemm, wf, stem
    return u


def _check_tile_stats(z, ts, nt, M, cout):
    """The epilogue's statistics tiles: their row counts sum to M, and BatchNorm from them (cmhar_bn_cl_fwd_tiles)
    agrees with the two-pass kernel on the same z to 1e-5 rel."""
    from cmhar import r3d
    ng = (nt + 15) // 16
    off = 2 * (nt + ng) * cout
    cnt = ts[off:off + nt].cpu()
    assert cnt.sum().item() == M and bool((cnt > 0).all()), ('tile counts', cnt.tolist(), M)
    bn_a, bn_b = torch.nn.BatchNorm3d(cout).to(DEV), torch.nn.BatchNorm3d(cout).to(DEV)
    ya, sma, sra = r3d._bn_fwd(z, bn_a, None, True, True)
    yb, smb, srb = r3d._bn_fwd_tiles(z, bn_b, None, True, ts, nt)
    print(f'  tile statistics: {nt} tiles, mean rel {rel(smb, sma):.2e}, rstd rel {rel(srb, sra):.2e}')
    assert rel(smb, sma) < 1e-5 and rel(srb, sra) < 1e-5, (rel(smb, sma), rel(srb, sra))
    assert rel(bn_b.running_var, bn_a.running_var) < 1e-5 and int(bn_b.num_batches_tracked) == 1


def _fwd_unsplit(dims, cout, M, x, wp, res):
    from cmhar import _lib as L
    lib = L.lib()
    z = X.nan_like((M, cout), BF, DEV)
    nt = lib.cmhar_conv3d_fwd_tiles(dims, cout)
    ts = X.nan_like(lib.cmhar_conv3d_fwd_stats_floats(dims, cout), torch.float32, DEV)
    L.call('cmhar_conv3d_fwd', dims, cout, x.data_ptr(), wp.data_ptr(), L.ptr(res), z.data_ptr(), ts.data_ptr(),
           L.stream(x.device))
    return z, ts, nt


def _fwd_split(dims, cout, M, x, wp, res):
    from cmhar import _lib as L
    z = X.nan_like((M, cout), BF, DEV)
    ws = X.nan_like(L.lib().cmhar_conv3d_fwd_split_ws(dims, cout), torch.float32, DEV)
    L.call('cmhar_conv3d_fwd_split', dims, cout, x.data_ptr(), wp.data_ptr(), L.ptr(res), z.data_ptr(),
           ws.data_ptr(), L.stream(x.device))
    return z


@gpu
@pytest.mark.parametrize('name,cin,cout,k,s,p,shape,plan,splits', FWD, ids=_ids(FWD))
def test_conv_forward_exact(name, cin, cout, k, s, p, shape, plan, splits):
    """z (and z + residual, rounded once) of the unsplit kernel, of the split form where the library plans one, and
    of the step's `_conv_fwd`, element for element; the unsplit kernel's BatchNorm tile statistics."""
    from cmhar import _lib as L
    from cmhar import r3d
    c = X.case(cin, cout, k, s, p, shape, seed=1, backward=False)
    conv, x, shp, dims, wp, _, _ = _device_case(c)
    lib = L.lib()
    assert r3d._igemm_ok(x, shp, conv, wp.shape[1])
    assert lib.cmhar_conv3d_fwd_plan(dims, cout) == plan, (name, lib.cmhar_conv3d_fwd_plan(dims, cout))
    assert lib.cmhar_conv3d_fwd_split_ws(dims, cout) == splits * c.M * cout, name
    res = c.res.to(DEV)
    osh = c.oshape
    with torch.no_grad():
        z, ts, nt = _fwd_unsplit(dims, cout, c.M, x, wp, None)
        X.assert_exact(f'{name} z plan {plan}', z, c.z, osh)
        _check_tile_stats(z, ts, nt, c.M, cout)
        zr, _, _ = _fwd_unsplit(dims, cout, c.M, x, wp, res)
        X.assert_exact(f'{name} z + res plan {plan}', zr, c.z + c.res.double(), osh)
        if splits:
            X.assert_exact(f'{name} z plan {plan} split', _fwd_split(dims, cout, c.M, x, wp, None), c.z, osh)
            X.assert_exact(f'{name} z + res plan {plan} split', _fwd_split(dims, cout, c.M, x, wp, res),
                           c.z + c.res.double(), osh)
        # the step's own launch (split where planned, statistics tiles otherwise)
        zs, col, _, stem, igemm, tstats, ntile = r3d._conv_fwd(x, shp, conv, wp, stats=True)
        assert igemm and not stem and col is None and (tstats is None) == bool(splits)
        X.assert_exact(f'{name} z step', zs, c.z, osh)
        torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize('name,cin,cout,k,s,p,shape,plan,splits', WGRAD, ids=_ids(WGRAD))
def test_conv_wgrad_exact(name, cin, cout, k, s, p, shape, plan, splits):
    """dW (fp32) == the fp64 reference, from `cmhar_conv3d_wgrad` into NaN-prefilled dW and split workspace and from
    the step's `_conv_wgrad`."""
    from cmhar import _lib as L
    from cmhar import r3d
    c = X.case(cin, cout, k, s, p, shape, seed=2)
    conv, x, shp, dims, wp, _, dz = _device_case(c)
    lib = L.lib()
    assert lib.cmhar_conv3d_wgrad_plan(dims, cout) == plan, (name, lib.cmhar_conv3d_wgrad_plan(dims, cout))
    n = lib.cmhar_conv3d_wgrad_ws(dims, cout)
    assert n == (splits * cout * conv.weight[0].numel() if splits > 1 else 0), (name, n)
    names = ('co', 'ci', 'kt', 'kh', 'kw')
    with torch.no_grad():
        dwp = X.nan_like((cout, wp.shape[1]), torch.float32, DEV)
        ws = X.nan_like(n, torch.float32, DEV) if n > 0 else None
        L.call('cmhar_conv3d_wgrad', dims, cout, x.data_ptr(), dz.data_ptr(), dwp.data_ptr(), L.ptr(ws),
               L.stream(x.device))
        X.assert_exact(f'{name} dW plan {plan}', c.dw_packed(dwp), c.dw, c.dw.shape, names)
        u = _unit(c, conv, x, shp, wp, None, None, True)
        X.assert_exact(f'{name} dW step', c.dw_packed(r3d._conv_wgrad(u, dz)), c.dw, c.dw.shape, names)
        torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize('acc', [False, True], ids=['noacc', 'acc'])
@pytest.mark.parametrize('name,cin,cout,shape,plan,splits', DGRAD, ids=_ids(DGRAD))
def test_conv_dgrad_flip_exact(name, cin, cout, shape, plan, splits, acc):
    """dx (+ the accumulated residual-branch gradient, rounded once) of the stride-1 input gradient as the conv of dz
    with the tap-flipped weight: the kernel the flipped geometry plans, its split form, and the step's `_conv_dgrad`."""
    from cmhar import _lib as L
    from cmhar import r3d
    c = X.case(cin, cout, 3, 1, 1, shape, seed=3)
    conv, x, shp, dims, wp, wf, dz = _device_case(c, flip=True)
    lib = L.lib()
    assert r3d._dgrad_igemm_ok(conv)
    N, To, Ho, Wo, _ = c.oshape
    fd = X.int_dims(N, To, Ho, Wo, cout, 3, 3, 3, 1, 1, 1, 1, 1, 1, wf.shape[1])
    Mx = math.prod(shape)
    assert lib.cmhar_conv3d_fwd_plan(fd, cin) == plan, (name, lib.cmhar_conv3d_fwd_plan(fd, cin))
    assert lib.cmhar_conv3d_fwd_split_ws(fd, cin) == splits * Mx * cin, name
    assert X.plans(cin, cout, 3, 1, 1, shape)[1] == 'flip:' + ('split' if splits else str(plan))
    dacc = c.acc.to(DEV) if acc else None
    want = c.dx + (c.acc.double() if acc else 0)
    with torch.no_grad():
        dx, _, _ = _fwd_unsplit(fd, cin, Mx, dz, wf, None if dacc is None else dacc.reshape(Mx, cin))
        X.assert_exact(f'{name} dx flip:{plan}', dx, want, shp)
        if splits:
            dx = _fwd_split(fd, cin, Mx, dz, wf, None if dacc is None else dacc.reshape(Mx, cin))
            X.assert_exact(f'{name} dx flip:{plan} split', dx, want, shp)
        u = _unit(c, conv, x, shp, wp, wf, None, True)
        dxs = r3d._conv_dgrad(u, dz, None if dacc is None else dacc.clone())
        X.assert_exact(f'{name} dx step', dxs, want, shp)
        torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize('acc', [False, True], ids=['noacc', 'acc'])
@pytest.mark.parametrize('name,cin,cout,k,s,p,shape,mt', COL2IM, ids=_ids(COL2IM))
def test_conv_dgrad_col2im_exact(name, cin, cout, k, s, p, shape, mt, acc):
    """dx = col2im(dz·W) (+ the accumulated gradient) with sparse dz (dcol stays an exact bf16 integer), one case per
    col2im3d_gather<MT> instance; also the forward and weight gradient of the same geometry on the step's route."""
    from cmhar import _lib as L
    from cmhar import kernels as K
    from cmhar import r3d
    c = X.case(cin, cout, k, s, p, shape, seed=4, dz_kind='sparse')
    conv, x, shp, dims, wp, _, dz = _device_case(c)
    assert max(-(-kk // ss) for kk, ss in zip(c.k, c.s)) == mt          # the gather instance (⌈k / s⌉ windows per axis)
    igemm = r3d._igemm_ok(x, shp, conv, wp.shape[1])
    assert igemm == (cin % 64 == 0) and not (igemm and r3d._dgrad_igemm_ok(conv))
    assert (L.lib().cmhar_conv3d_fwd_plan(dims, cout) > 0) == igemm
    assert not r3d._pointwise(conv, shp, wp.shape[1], c.M, r3d._r8(c.M))
    want = c.dx + (c.acc.double() if acc else 0)
    with torch.no_grad():
        dcol = X.nan_like((c.M, wp.shape[1]), BF, DEV)
        K.gemm(1, dz[:c.M], wp, dcol)
        kk = conv.weight[0].numel()
        dcol_want = c.dz.reshape(c.M, cout).double() @ wp[:, :kk].double().cpu()
        X.assert_exact(f'{name} dcol', dcol[:, :kk], dcol_want, dcol_want.shape, ('row', 'k'))
        dx = c.acc.to(DEV).clone() if acc else X.nan_like(shp, BF, DEV)
        L.call('cmhar_conv3d_col2im', L.BF16, dims, dcol.data_ptr(), dx.data_ptr(), int(acc), L.stream(x.device))
        X.assert_exact(f'{name} dx col2im<{mt}>', dx, want, shp)
        if mt == 1 and not acc:
            # 1x1 at stride 2: only even (t, h, w) lie in a window — more than three quarters of dx are exact zeros
            live = torch.zeros(shp, dtype=torch.bool)
            live[:, ::2, ::2, ::2] = True
            assert live.float().mean().item() < 0.25 and bool((dx.cpu()[~live] == 0).all())
        # the step's route: forward (implicit GEMM, or im2col + GEMM), weight gradient, input gradient
        z, col, _, stem, ig, _, _ = r3d._conv_fwd(x, shp, conv, wp, stats=False)
        assert ig == igemm and not stem
        X.assert_exact(f'{name} z step', z, c.z, c.oshape)
        u = _unit(c, conv, x, shp, wp, None, col, igemm)
        X.assert_exact(f'{name} dW step', c.dw_packed(r3d._conv_wgrad(u, dz)), c.dw, c.dw.shape,
                       ('co', 'ci', 'kt', 'kh', 'kw'))
        dxs = r3d._conv_dgrad(u, dz, c.acc.to(DEV).clone() if acc else None)
        X.assert_exact(f'{name} dx step', dxs, want, shp)
        torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize('cin,k,s,p,shape', STEM)
def test_conv_stem_exact(cin, k, s, p, shape):
    """The implicit stem (cmhar_conv3d_stem_fwd / _wgrad) at the geometries of test_conv3d_implicit_stem_fwd_wgrad
    with integer operands: z == the reference after RNE, dW4 == the reference, statistics tiles as above."""
    from cmhar import _lib as L
    from cmhar import r3d
    c = X.case(cin, 64, k, s, p, shape, seed=5)
    conv = X.conv3d(cin, 64, k, s, p).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(c.conv.weight)
    x = c.x.to(DEV)
    shp = tuple(x.shape)
    lib = L.lib()
    assert r3d._stem_ok(x, shp, conv)
    dims = r3d._dims(shp, conv, r3d._stem_kp(conv))
    ntile = lib.cmhar_conv3d_stem_tiles(dims, 64)
    assert ntile > 0
    kt, kh, kw = k
    with torch.no_grad():
        w4 = r3d._pack_stem(conv)
        ts = X.nan_like(lib.cmhar_conv3d_stem_stats_floats(dims, 64), torch.float32, DEV)
        z = X.nan_like((c.M, 64), BF, DEV)
        L.call('cmhar_conv3d_stem_fwd', dims, 64, x.data_ptr(), w4.data_ptr(), z.data_ptr(), ts.data_ptr(),
               L.stream(x.device))
        X.assert_exact('stem z', z, c.z, c.oshape)
        _check_tile_stats(z, ts, ntile, c.M, 64)
        dz = torch.zeros(r3d._r8(c.M), 64, dtype=BF, device=DEV)
        dz[:c.M] = c.dz.reshape(c.M, 64).to(DEV)
        dw4 = X.nan_like((64, r3d._stem_kp(conv)), torch.float32, DEV)
        ws = X.nan_like(lib.cmhar_conv3d_stem_wgrad_ws(dims, 64), torch.float32, DEV)
        L.call('cmhar_conv3d_stem_wgrad', dims, 64, x.data_ptr(), dz.data_ptr(), dw4.data_ptr(), ws.data_ptr(),
               L.stream(x.device))
        dw = dw4.view(64, kt, kh, 8, 4)[:, :, :, :kw, :cin].permute(0, 4, 1, 2, 3)
        X.assert_exact('stem dW4', dw, c.dw, c.dw.shape, ('co', 'ci', 'kt', 'kh', 'kw'))
        # the step's route
        zs, col, w4s, stem, igemm, tstats, nt = r3d._conv_fwd(x, shp, conv, None, stats=True)
        assert stem and not igemm and nt == ntile and torch.equal(w4s, w4)
        X.assert_exact('stem z step', zs, c.z, c.oshape)
        u = _unit(c, conv, x, shp, w4s, None, None, False, stem=True)
        dws = r3d._conv_wgrad(u, dz).view(64, kt, kh, 8, 4)[:, :, :, :kw, :cin].permute(0, 4, 1, 2, 3)
        X.assert_exact('stem dW4 step', dws, c.dw, c.dw.shape, ('co', 'ci', 'kt', 'kh', 'kw'))
        torch.cuda.synchronize()
    # the zero padding of the packed layout (iw >= kw, c >= C) carries no gradient into the parameter view
    assert torch.equal(w4.view(64, kt, kh, 8, 4)[:, :, :, kw:, :].float().cpu(), torch.zeros(64, kt, kh, 8 - kw, 4))
    assert torch.equal(w4.view(64, kt, kh, 8, 4)[:, :, :, :, cin:].float().cpu(), torch.zeros(64, kt, kh, 8, 4 - cin))


# ------------------------------------------------------------------------------------------------------------------
# csrc/cnn2d.hip: depthwise conv and max-pool, direct ABI calls
# ------------------------------------------------------------------------------------------------------------------
DW_KSP = [(1, 1, 0), (1, 2, 0), (2, 1, 0), (2, 2, 0), (2, 2, 1), (3, 1, 1), (3, 2, 1), (3, 1, 0)]
POOL_KSP = [(2, 2, 0), (2, 1, 1), (3, 1, 1), (3, 3, 0), (1, 2, 0), (3, 2, 1)]


def _dw_case(N, H, W, C, k, s, p, seed):
    """Integer depthwise-conv operands and the fp64 reference (F.conv2d(groups=C) + autograd), channels-last."""
    g = torch.Generator().manual_seed(seed)
    x = X.int_tensor(g, (N, C, H, W)).double().requires_grad_(True)
    w = X.int_tensor(g, (C, 1, k, k)).double().requires_grad_(True)
    z = F.conv2d(x, w, stride=s, padding=p, groups=C)
    dz = X.int_tensor(g, z.shape, -1, 1).double()
    dx, dw = torch.autograd.grad(z, (x, w), dz)
    # premise: Σ|x·w| <= 4 k², Σ|dz·w| <= 2 k², Σ|dz·x| <= 2 M — exact in bf16 (<= 256) resp. fp32 (< 2^24)
    assert z.abs().max() <= 256 and dx.abs().max() <= 256 and 2 * z.numel() // C < X.EXACT
    cl = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()      # noqa: E731
    return cl(x), w.detach().float(), cl(z), cl(dz), cl(dx), dw


def _dw_run(dt, N, H, W, C, k, s, p, seed, only_wgrad=False):
    from cmhar import _lib as L
    x, w, z_want, dz, dx_want, dw_want = _dw_case(N, H, W, C, k, s, p, seed)
    Ho, Wo = z_want.shape[1:3]
    xc, wc, dzc = x.to(DEV, dt), w.to(DEV), dz.to(DEV, dt)
    st = L.stream(xc.device)
    dc = L.dtype_code(dt)
    tag = f'dw k{k} s{s} p{p} C{C} {dt}'
    if not only_wgrad:
        z = X.nan_like((N, Ho, Wo, C), dt, DEV)
        L.call('cmhar_dwconv2d_cl_fwd', dc, N, H, W, C, k, s, p, xc.data_ptr(), wc.data_ptr(), z.data_ptr(), st)
        X.assert_exact(tag + ' z', z, z_want, z_want.shape, 'nhwc')
        dx = X.nan_like((N, H, W, C), dt, DEV)
        L.call('cmhar_dwconv2d_cl_dgrad', dc, N, H, W, C, k, s, p, dzc.data_ptr(), wc.data_ptr(), dx.data_ptr(), st)
        X.assert_exact(tag + ' dx', dx, dx_want, dx_want.shape, 'nhwc')
    dw = X.nan_like((C, 1, k, k), torch.float32, DEV)
    ws = X.nan_like(L.lib().cmhar_dwconv2d_cl_wgrad_ws(N, H, W, C, k, s, p), torch.float32, DEV)
    L.call('cmhar_dwconv2d_cl_wgrad', dc, N, H, W, C, k, s, p, xc.data_ptr(), dzc.data_ptr(), dw.data_ptr(),
           ws.data_ptr(), st)
    X.assert_exact(tag + ' dw', dw, dw_want, dw_want.shape, ('c', 'one', 'kh', 'kw'))
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize('dt', [torch.float32, BF], ids=['f32', 'bf16'])
@pytest.mark.parametrize('k,s,p', DW_KSP)
def test_depthwise_conv_exact(k, s, p, dt):
    """cmhar_dwconv2d_cl_{fwd,dgrad,wgrad}: the K = 1, 2, 3 instances at every (stride, pad) the entry accepts, on a
    9 x 7 frame (odd sizes: windows cut by both borders, a last row / column outside every stride-2 window), 8
    channels (one vector, 256 weight-gradient row slots) and 96 (12 vectors: 21 row slots, 4 idle threads)."""
    for C in (8, 96):
        _dw_run(dt, 2, 9, 7, C, k, s, p, seed=10 * k + s + p + C)


@gpu
@pytest.mark.parametrize('dt', [torch.float32, BF], ids=['f32', 'bf16'])
@pytest.mark.parametrize('C', [2048, 8])
@pytest.mark.parametrize('k,s,p', [(3, 1, 1), (2, 1, 1)])
def test_depthwise_wgrad_row_slots_exact(k, s, p, C, dt):
    """Depthwise weight gradient at C = 2048 (one row slot per block: every chunk walks its rows two at a time, an
    even-length chunk and an odd-length last one) and C = 8 (256 row slots, some idle), with M = 19 x 21 = 399 output
    rows: two chunks of 200 and 199, M no multiple of the chunk length."""
    from cmhar import _lib as L
    N, H, W = 1, 18 + k - 2 * p, 20 + k - 2 * p
    M = ((H + 2 * p - k) // s + 1) * ((W + 2 * p - k) // s + 1)
    nch = (M + 255) // 256
    assert M == 399 and nch == 2 and M % ((M + nch - 1) // nch) != 0
    assert L.lib().cmhar_dwconv2d_cl_wgrad_ws(N, H, W, C, k, s, p) == nch * k * k * C
    _dw_run(dt, N, H, W, C, k, s, p, seed=C + k, only_wgrad=True)


@gpu
@pytest.mark.parametrize('dt', [torch.float32, BF], ids=['f32', 'bf16'])
@pytest.mark.parametrize('k,s,p', POOL_KSP)
def test_maxpool_geometries_exact(k, s, p, dt):
    """cmhar_maxpool2d_cl_{fwd,bwd} at every kind of geometry the entry accepts (overlapping, abutting and gapped
    windows, k = 1, padded k = 2) on tied integer data: y and the arg-max routing of the gradient equal torch's CPU
    max_pool2d (first maximum in scan order)."""
    from cmhar import _lib as L
    N, C, H, W = 2, 16, 13, 11
    g = torch.Generator().manual_seed(100 + 10 * k + 3 * s + p)
    x = X.int_tensor(g, (N, C, H, W), -3, 3).requires_grad_(True)          # many tied maxima
    ref = F.max_pool2d(x, k, s, p)
    dy = X.int_tensor(g, ref.shape, -4, 4)
    ref.backward(dy)
    Ho, Wo = ref.shape[2:]
    xc = x.detach().permute(0, 2, 3, 1).contiguous().to(DEV, dt)
    y = X.nan_like((N, Ho, Wo, C), dt, DEV)
    arg = torch.full((N * Ho * Wo, C), 255, dtype=torch.uint8, device=DEV)
    dc = L.dtype_code(dt)
    L.call('cmhar_maxpool2d_cl_fwd', dc, N, H, W, C, k, s, p, xc.data_ptr(), y.data_ptr(), arg.data_ptr(),
           L.stream(xc.device))
    X.assert_exact(f'maxpool k{k} s{s} p{p} y', y, ref.detach().permute(0, 2, 3, 1).double(), (N, Ho, Wo, C), 'nhwc')
    assert int(arg.max()) < k * k
    dyc = dy.permute(0, 2, 3, 1).contiguous().to(DEV, dt)
    dx = X.nan_like((N, H, W, C), dt, DEV)
    L.call('cmhar_maxpool2d_cl_bwd', dc, N, H, W, C, k, s, p, dyc.data_ptr(), arg.data_ptr(), dx.data_ptr(),
           L.stream(xc.device))
    X.assert_exact(f'maxpool k{k} s{s} p{p} dx', dx, x.grad.permute(0, 2, 3, 1).double(), (N, H, W, C), 'nhwc')
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize('why,C,k,s,p', [('k=4', 16, 4, 1, 1), ('2p>k', 16, 2, 1, 2), ('2p>k', 16, 3, 1, 2),
                                         ('C=12', 12, 3, 1, 1)])
def test_dwconv_maxpool_refusals(why, C, k, s, p):
    """A geometry the templated kernels do not cover is refused (non-zero return) and nothing is written."""
    from cmhar import _lib as L
    lib = L.lib()
    N, H, W = 2, 9, 7
    st = L.stream(torch.device(DEV))
    for dt in (torch.float32, BF):
        dc = L.dtype_code(dt)
        a = torch.ones(N * (H + 4) * (W + 4) * C, dtype=dt, device=DEV)      # any operand: larger than every tensor
        w = torch.ones(C * k * k, device=DEV)
        arg = torch.zeros(a.numel(), dtype=torch.uint8, device=DEV)
        out = X.nan_like(a.numel(), dt, DEV)
        dw = X.nan_like(C * k * k, torch.float32, DEV)
        ws = X.nan_like(4096 * k * k, torch.float32, DEV)
        g = (dc, N, H, W, C, k, s, p)
        assert lib.cmhar_dwconv2d_cl_wgrad_ws(N, H, W, C, k, s, p) < 0
        assert lib.cmhar_dwconv2d_cl_fwd(*g, a.data_ptr(), w.data_ptr(), out.data_ptr(), st) != 0
        assert lib.cmhar_dwconv2d_cl_dgrad(*g, a.data_ptr(), w.data_ptr(), out.data_ptr(), st) != 0
        assert lib.cmhar_dwconv2d_cl_wgrad(*g, a.data_ptr(), a.data_ptr(), dw.data_ptr(), ws.data_ptr(), st) != 0
        assert lib.cmhar_maxpool2d_cl_fwd(*g, a.data_ptr(), out.data_ptr(), arg.data_ptr(), st) != 0
        assert lib.cmhar_maxpool2d_cl_bwd(*g, a.data_ptr(), arg.data_ptr(), out.data_ptr(), st) != 0
        torch.cuda.synchronize()
        assert bool(out.isnan().all()) and bool(dw.isnan().all()) and bool(ws.isnan().all()) and int(arg.max()) == 0


@gpu
def test_depthwise_wgrad_refuses_past_2048_channels():
    """The depthwise weight gradient keeps C / 8 threads per row within one 256-thread block: C = 2056 is refused,
    dw and the workspace stay untouched (the forward and input gradient have no such limit)."""
    from cmhar import _lib as L
    lib = L.lib()
    N, H, W, C, k, s, p = 1, 5, 4, 2056, 3, 1, 1
    x = torch.ones(N * H * W * C, dtype=BF, device=DEV)
    n = lib.cmhar_dwconv2d_cl_wgrad_ws(N, H, W, C, k, s, p)
    assert n > 0
    dw = X.nan_like(C * k * k, torch.float32, DEV)
    ws = X.nan_like(n, torch.float32, DEV)
    rc = lib.cmhar_dwconv2d_cl_wgrad(L.BF16, N, H, W, C, k, s, p, x.data_ptr(), x.data_ptr(), dw.data_ptr(),
                                     ws.data_ptr(), L.stream(x.device))
    torch.cuda.synchronize()
    assert rc != 0 and bool(dw.isnan().all()) and bool(ws.isnan().all())
    _dw_run(BF, N, H, W, 2048, k, s, p, seed=7, only_wgrad=True)          # the last width it takes
