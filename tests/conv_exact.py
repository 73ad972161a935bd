"""Bit-exact convolution checks with integer operands (helper of tests/test_conv_plans_gpu.py and
tests/test_r3d_production_gpu.py; not a conftest).

Method: x and W are integers in [-2, 2] (x stored bf16), dz is in {-1, 0, 1}.  Every product and every fp32 partial
sum of the kernels is then an integer below 2^24, exact in ANY summation order, so a kernel's output equals torch's
fp64 convolution (and its autograd) after ONE round-to-nearest-even to the output dtype: bf16 outputs are compared
with `==` against `.to(torch.bfloat16)` of the fp64 value, fp32 weight gradients with `==` against the fp64 value.  A
single wrong element (a halo row, a dropped tap on a ragged tile, a mis-masked column group) fails the comparison.

* `dense` dz (every element in {-1, 0, 1}) serves the forward, the weight gradient and the flipped-weight input
  gradient; `sparse` dz (density 1/32) only the GEMM + col2im input gradient, whose dz·W passes through a bf16 `dcol`
  that must stay an exactly representable integer (|dcol| <= 256).
* The premise guard (`Case.guard`) is computed from the reference alone: Σ|x·w| per output, Σ|dz·x| per weight and
  Σ|dz·w| per input below 2^24, and |dcol| <= 256 on the col2im route.  A shape that breaks it is the wrong shape;
  the comparison never changes.
* `plans` / `plan_detail` ask the library which kernel a geometry takes (host-side queries, no GPU).
"""
import ctypes
import functools
import math

import torch
import torch.nn.functional as F

EXACT = 1 << 24          # integers below this are exact in fp32
DCOL_MAX = 256           # integers up to this are exact in bf16


def _t3(v):
    return (v, v, v) if isinstance(v, int) else tuple(v)


def conv3d(cin, cout, k, s, p):
    return torch.nn.Conv3d(cin, cout, k, s, p, bias=False)


def plan_detail(cin, cout, k, s, p, shape):
    """Host-side plan queries of one conv at input (N, T, H, W): the forward plan (cmhar_conv3d_fwd_plan) and its
    split count (cmhar_conv3d_fwd_split_ws / (M·Cout)), the same two of the flipped-weight conv the stride-1 input
    gradient runs (None when the input gradient is dz·W + col2im), the weight-gradient plan and whether it ends in
    the split reduce."""
    from cmhar import _lib as L
    from cmhar import r3d
    lib = L.lib()
    conv = conv3d(cin, cout, k, s, p)
    shp = tuple(shape) + (cin,)
    Kp = r3d._r8(conv.weight[0].numel())
    dims = r3d._dims(shp, conv, Kp)
    N, To, Ho, Wo, _ = r3d._out_shape(shp, conv)
    M = N * To * Ho * Wo
    d = {'fwd': lib.cmhar_conv3d_fwd_plan(dims, cout),
         'fwd_splits': lib.cmhar_conv3d_fwd_split_ws(dims, cout) // (M * cout),
         'flip': None, 'flip_splits': 0,
         'wgrad': lib.cmhar_conv3d_wgrad_plan(dims, cout),
         'wgrad_reduce': lib.cmhar_conv3d_wgrad_ws(dims, cout) > 0,
         'wgrad_splits': max(1, lib.cmhar_conv3d_wgrad_ws(dims, cout) // (cout * conv.weight[0].numel()))}
    if r3d._dgrad_igemm_ok(conv):
        kt, kh, kw = conv.kernel_size
        fd = r3d._dims((N, To, Ho, Wo, cout), conv3d(cout, cin, k, 1, p), kt * kh * kw * cout)
        d['flip'] = lib.cmhar_conv3d_fwd_plan(fd, cin)
        d['flip_splits'] = lib.cmhar_conv3d_fwd_split_ws(fd, cin) // (math.prod(shape) * cin)
    return d


def plans(cin, cout, k, s, p, shape):
    """(forward, input gradient, weight gradient) as the training step takes them: forward 'split' or the
    cmhar_conv3d_fwd_plan number; input gradient 'flip:<plan of the flipped conv or split>' or 'col2im'; weight
    gradient the cmhar_conv3d_wgrad_plan number, '+r' with the split reduce."""
    d = plan_detail(cin, cout, k, s, p, shape)
    fwd = 'split' if d['fwd_splits'] > 0 else d['fwd']
    dg = 'col2im' if d['flip'] is None else 'flip:' + str('split' if d['flip_splits'] > 0 else d['flip'])
    return fwd, dg, str(d['wgrad']) + ('+r' if d['wgrad_reduce'] else '')


def int_tensor(g, shape, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


class Case:
    """Integer operands of one conv geometry and its fp64 reference (all on the CPU).

    x (N, T, H, W, Cin) bf16, conv.weight integers, dz (N, To, Ho, Wo, Cout) bf16 ('dense' or 'sparse'), acc
    (N, T, H, W, Cin) bf16 (a residual-branch gradient the input gradient accumulates into), res (M, Cout) bf16 (a
    forward residual); z [M, Cout], dx (N, T, H, W, Cin) and dw (the parameter's shape) in fp64."""

    def __init__(self, cin, cout, k, s, p, shape, seed, dz_kind='dense', backward=True):
        g = torch.Generator().manual_seed(seed)
        self.cin, self.cout, self.k, self.s, self.p, self.shape = cin, cout, _t3(k), _t3(s), _t3(p), tuple(shape)
        N, T, H, W = shape
        self.conv = conv3d(cin, cout, k, s, p)
        with torch.no_grad():
            self.conv.weight.copy_(int_tensor(g, self.conv.weight.shape))
        self.x = int_tensor(g, (N, T, H, W, cin)).bfloat16()
        self.oshape = (N,) + tuple((d + 2 * pp - kk) // ss + 1
                                   for d, pp, kk, ss in zip((T, H, W), self.p, self.k, self.s)) + (cout,)
        self.M = math.prod(self.oshape[:4])
        dz = int_tensor(g, self.oshape, -1, 1)
        if dz_kind == 'sparse':
            dz = dz * (torch.rand(self.oshape, generator=g) < 1.0 / 32).float()
        self.dz_kind = dz_kind
        self.dz = dz.bfloat16()
        self.acc = int_tensor(g, (N, T, H, W, cin)).bfloat16()
        self.res = int_tensor(g, (self.M, cout)).bfloat16()
        # reference: torch's fp64 convolution and its autograd (integers: exact)
        xr = self.x.permute(0, 4, 1, 2, 3).double().requires_grad_(backward)
        wr = self.conv.weight.detach().double().requires_grad_(backward)
        zr = F.conv3d(xr, wr, stride=self.s, padding=self.p)
        self.z = zr.detach().permute(0, 2, 3, 4, 1).reshape(self.M, cout).contiguous()
        self.dx = self.dw = None
        if backward:
            gx, gw = torch.autograd.grad(zr, (xr, wr), self.dz.permute(0, 4, 1, 2, 3).double())
            self.dx = gx.permute(0, 2, 3, 4, 1).contiguous()
            self.dw = gw
        self.guard(backward)

    def guard(self, backward=True):
        """The premise, from the reference alone: with every operand replaced by its magnitude the convolution and
        its gradients give Σ|x·w|, Σ|dz·x| and Σ|dz·w| — all below 2^24 (sums of integers below 2^24 are exact in the
        fp32 this runs in, and a sum at or past it fails the guard all the same); on the col2im route every element
        of dcol = dz·W is an integer of magnitude <= 256."""
        xa = self.x.permute(0, 4, 1, 2, 3).float().abs().requires_grad_(backward)
        wa = self.conv.weight.detach().abs().requires_grad_(backward)
        za = F.conv3d(xa, wa, stride=self.s, padding=self.p)
        assert za.max().item() < EXACT, ('Σ|x·w|', za.max().item())
        if backward:
            gx, gw = torch.autograd.grad(za, (xa, wa), self.dz.permute(0, 4, 1, 2, 3).float().abs())
            assert gw.max().item() < EXACT, ('Σ|dz·x|', gw.max().item())
            assert gx.max().item() < EXACT, ('Σ|dz·w|', gx.max().item())
        if self.dz_kind == 'sparse':
            dcol = self.dz.reshape(self.M, self.cout).double() @ self.conv.weight.detach().double().reshape(self.cout, -1)
            assert dcol.abs().max().item() <= DCOL_MAX, ('|dcol|', dcol.abs().max().item())

    def dw_packed(self, dwp):
        """[Cout, Kp] fp32 in the im2col k order (kt, kh, kw, Cin) → the parameter's shape."""
        kk = self.conv.weight[0].numel()
        return dwp[:, :kk].reshape(self.cout, *self.k, self.cin).permute(0, 4, 1, 2, 3)


@functools.lru_cache(maxsize=6)
def case(cin, cout, k, s, p, shape, seed=0, dz_kind='dense', backward=True):
    """One `Case` per (geometry, seed, dz kind), shared by the tests that need it and never modified."""
    return Case(cin, cout, k, s, p, shape, seed, dz_kind, backward)


def mismatches(got, want, names, limit=6):
    """Number of elements of `got` that differ from `want` (a NaN differs from everything) and the coordinates of
    the first few, labelled with `names` (one per dimension)."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    bad = got != want
    n = int(bad.sum())
    if n == 0:
        return 0, ''
    idx = bad.nonzero()[:limit]
    where = ['(' + ', '.join(f'{nm}={int(i)}' for nm, i in zip(names, row)) + f'): got {got[tuple(row)].item()}, '
             f'want {want[tuple(row)].item()}' for row in idx]
    return n, '; '.join(where)


def assert_exact(what, got, want64, shape, names='nthwc'):
    """`got` (any shape with `shape`'s element count, bf16 or fp32) == `want64` after one round-to-nearest-even to
    got's dtype, element for element; the failure names how many differ and where the first few are."""
    want = want64.reshape(shape).to(got.dtype)
    n, where = mismatches(got.reshape(shape), want, names)
    assert n == 0, f'{what}: {n} of {want.numel()} elements wrong; first at {where}'


def nan_like(shape, dtype, device):
    return torch.full(tuple(shape) if not isinstance(shape, int) else (shape,), float('nan'), dtype=dtype,
                      device=device)


def int_dims(*v):
    return (ctypes.c_int * len(v))(*v)
