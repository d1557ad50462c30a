"""Direct tests of the LayerNorm epilogues fused into the GEMM and FFN kernels -- gemm_kernel and
splitk_finalize_kernel (csrc/gemm.hip), gemm_rw_kernel (csrc/gemm_rw.hip), ffn_fused_kernel and
ffn_fused_rt2_kernel with its attention-out pre-phase (csrc/ffn.hip) -- against an f64 LayerNorm of
the f64 pre-activation (direct_refs.ln_epilogue_ref).

The matrix operands are small dyadic numbers, exact in every compute dtype and with exact f32
partial sums in any order, so the pre-activation the kernel normalises is known exactly up to the
additions of the f32 bias and the residual: what is measured is the epilogue.  The offset enters
through the f32 bias, 100 + randn (rows of 100 + O(1)); every site also runs with zero offset.
Bounds, per element: f32 4x the maximum error of torch's CPU f32 layer_norm of the same
pre-activation; 16-bit one output rounding of the f64 result plus that 4x term.  A one-pass variance
(sums of v and v^2) misses both at offset 100 (test_direct_refs_cpu.py)."""
import time

import pytest
import torch

import direct_refs as R

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
EPS = 1e-5
OFFSETS = [100.0, 0.0]
_T0 = time.time()


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    yield kernels
    torch.cuda.synchronize()
    print(f'\ntest_ln_epilogue_direct_gpu wall time {time.time() - _T0:.1f} s')


@pytest.fixture
def gemm_flags():
    """Select the GEMM kernel family for one test and restore the default afterwards."""
    from kinet_amd import _native
    lib = _native.lib()
    yield lib.kinet_gemm_set_flags
    lib.kinet_gemm_set_flags(0)


def _id(v):
    return str(v).replace('torch.', '').replace(' ', '')


def _dyadic(shape, g, step, lim):
    """Multiples of `step` in [-lim * step, lim * step], f64."""
    return torch.randint(-lim, lim + 1, shape, generator=g).double() * step


def _ln_params(d, g):
    return torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)


def _check(y, pre64, gam, bet, dtype, what, extra=None):
    """|y - LN64(pre64)| <= one rounding of a 16-bit output + 4x torch's CPU f32 error (+ extra)."""
    assert y.dtype == dtype and tuple(y.shape) == tuple(pre64.shape), (what, y.dtype, y.shape)
    ref, t = R.ln_epilogue_yardstick(pre64, gam, bet, EPS)
    got = y.double().cpu()
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    tol = R.OUT_ROUND[dtype] * ref.abs() + 4 * t
    if extra is not None:
        tol = tol + extra
    worst = (err / tol).max().item()
    print(f'{what}: torch CPU f32 max err {t:.3e}, bound 4x = {4 * t:.3e} (+ output rounding '
          f'{R.OUT_ROUND[dtype]:.1e} |y|), kernel max err {err.max().item():.3e}, worst err / bound {worst:.3f}')
    bad = err > tol
    assert not bad.any(), (what, int(bad.sum()), err.max().item(), worst)


# ------------------------------------------------------------------------------ GEMM sites
def _gemm_case(M, N, Kd, dtype, offset):
    """x in {-1, -1/2, 0, 1/2, 1}, W in multiples of 1/8 up to 1/4: products multiples of 1/16, every
    partial sum below 2^9 -- exact in f32 whatever the order and the split.  bias f32, residual
    rounded to the compute dtype."""
    g = torch.Generator().manual_seed(M * 7 + N * 3 + Kd + int(offset))
    x, w = _dyadic((M, Kd), g, 0.5, 2), _dyadic((N, Kd), g, 0.125, 2)
    b = offset + torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g).to(dtype)
    gam, bet = _ln_params(N, g)
    pre = x @ w.t() + b.double() + r.double()
    return x.to(dtype), w.to(dtype), b, r, gam, bet, pre


def _gemm_run(K, case):
    x, w, b, r, gam, bet, _ = case
    return K.linear(x.cuda(), w.cuda(), b.cuda(), residual=r.cuda(), ln=(gam.cuda(), bet.cuda(), EPS))


@pytest.mark.parametrize('offset', OFFSETS)
@pytest.mark.parametrize('dtype', [F32, F16], ids=_id)
@pytest.mark.parametrize('M,N,Kd', [(37, 256, 64), (33, 200, 72), (40, 288, 64)])   # ragged N; the 320-wide tile
def test_gemm_kernel_ln_epilogue(K, M, N, Kd, dtype, offset):
    case = _gemm_case(M, N, Kd, dtype, offset)
    assert K.ksplit_for(M, N, Kd, True) == 1
    _check(_gemm_run(K, case), case[-1], case[4], case[5], dtype, f'gemm_kernel LN ({M}, {N}, {Kd}) {_id(dtype)} +{offset}')


@pytest.mark.parametrize('offset', OFFSETS)
def test_gemm_kernel_ln_epilogue_64_row_tile(K, gemm_flags, offset):
    """M > 8192 takes the 64-row LayerNorm tile of gemm_kernel; K = 64 in a 16-bit type would go to the
    resident-weight kernel, so the tiled family is selected (flag 4)."""
    M, N, Kd = 8200, 256, 64
    case = _gemm_case(M, N, Kd, BF16, offset)
    gemm_flags(4)
    _check(_gemm_run(K, case), case[-1], case[4], case[5], BF16, f'gemm_kernel LN 64-row tile ({M}, {N}, {Kd}) bf16 +{offset}')


@pytest.mark.parametrize('offset', OFFSETS)
@pytest.mark.parametrize('dtype', [F32, F16], ids=_id)
@pytest.mark.parametrize('M,N,Kd', [(64, 256, 1024), (50, 288, 1024)])
def test_splitk_finalize_ln_epilogue(K, M, N, Kd, dtype, offset):
    assert K.ksplit_for(M, N, Kd, True) > 1
    case = _gemm_case(M, N, Kd, dtype, offset)
    _check(_gemm_run(K, case), case[-1], case[4], case[5], dtype, f'splitk_finalize LN ({M}, {N}, {Kd}) {_id(dtype)} +{offset}')


@pytest.mark.parametrize('dtype', [F16, BF16], ids=_id)
@pytest.mark.parametrize('M,N,Kd', [(4100, 256, 64), (4100, 200, 128)])
def test_gemm_rw_ln_epilogue(K, gemm_flags, M, N, Kd, dtype):
    # the resident-weight kernel takes this shape class: with generic operands (sums that depend on
    # their order) the default route and the tiled family (flag 4) differ in bits
    g = torch.Generator().manual_seed(M + N + Kd)
    x = torch.randn(M, Kd, generator=g).to(dtype).cuda()
    w = (torch.randn(N, Kd, generator=g) / Kd ** 0.5).to(dtype).cuda()
    b, r = torch.randn(N, generator=g).cuda(), torch.randn(M, N, generator=g).to(dtype).cuda()
    gam, bet = (t.cuda() for t in _ln_params(N, g))
    y_default = K.linear(x, w, b, residual=r, ln=(gam, bet, EPS))
    gemm_flags(4)
    y_tiled = K.linear(x, w, b, residual=r, ln=(gam, bet, EPS))
    gemm_flags(0)
    assert not torch.equal(y_default, y_tiled)
    for offset in OFFSETS:
        case = _gemm_case(M, N, Kd, dtype, offset)
        _check(_gemm_run(K, case), case[-1], case[4], case[5], dtype, f'gemm_rw LN ({M}, {N}, {Kd}) {_id(dtype)} +{offset}')


# ------------------------------------------------------------------------------- FFN sites
def _ffn_modules(D, Fh, dtype, offset, g):
    """linear1: W1 multiples of 1/4 up to 1/2, b1 multiples of 1/4 up to 1; linear2: W2 multiples of 1/64
    up to 1/16, b2 = offset + randn (f32); norm with random gamma / beta.  With x in {-1, 0, 1} the hidden
    h = relu(W1 x + b1) is a multiple of 1/4 below 64: exact in bf16 and f16, so its rounding inside the
    kernel changes nothing; W2 h is a multiple of 1/256 below 2^8: exact f32 sums."""
    lin1, lin2, norm = torch.nn.Linear(D, Fh), torch.nn.Linear(Fh, D), torch.nn.LayerNorm(D, eps=EPS)
    gam, bet = _ln_params(D, g)
    with torch.no_grad():
        lin1.weight.copy_(_dyadic((Fh, D), g, 0.25, 2))
        lin1.bias.copy_(_dyadic((Fh,), g, 0.25, 4))
        lin2.weight.copy_(_dyadic((D, Fh), g, 1.0 / 64, 4))
        lin2.bias.copy_(offset + torch.randn(D, generator=g))
        norm.weight.copy_(gam)
        norm.bias.copy_(bet)
    return lin1, lin2, norm


def _ffn_pre(x64, lin1, lin2, dtype):
    h = torch.relu(x64 @ lin1.weight.detach().double().t() + lin1.bias.detach().double())
    assert torch.equal(h.to(dtype).double(), h) and h.max().item() < 64       # the kernel's rounding of h is exact
    return x64 + h @ lin2.weight.detach().double().t() + lin2.bias.detach().double()


def _ffn_check(K, M, D, Fh, dtype, offset, what):
    g = torch.Generator().manual_seed(M + D + Fh + int(offset))
    lin1, lin2, norm = _ffn_modules(D, Fh, dtype, offset, g)
    x = _dyadic((M, D), g, 1.0, 1)
    pre = _ffn_pre(x, lin1, lin2, dtype)
    y = K.ffn_fused(x.to(dtype).cuda(), lin1.cuda(), lin2.cuda(), norm.cuda())
    _check(y, pre, norm.weight.detach().cpu(), norm.bias.detach().cpu(), dtype, f'{what} M={M} D={D} F={Fh} {_id(dtype)} +{offset}')


@pytest.mark.parametrize('offset', OFFSETS)
@pytest.mark.parametrize('dtype', [F16, BF16], ids=_id)
@pytest.mark.parametrize('D', [256, 288])
def test_ffn_fused_norm_epilogue(K, D, dtype, offset):
    _ffn_check(K, 37, D, 64, dtype, offset, 'ffn_fused_kernel norm')


@pytest.mark.parametrize('offset', OFFSETS)
def test_ffn_fused_rt2_norm_epilogue(K, offset):
    """M >= 16384 at D = 256: the 8-wave x 32-row tile (launch_ffn)."""
    assert 16385 >= K.ATTN_OUT_FFN_MIN_ROWS
    _ffn_check(K, 16385, 256, 32, F16, offset, 'ffn_fused_rt2_kernel norm')


# ------------------------------------------- attention-out pre-phase (norm1) + FFN + norm2
def _ln_perturbation(d, pre64, gam, eps=EPS):
    """Majorant of |LN(z + delta) - LN(z)| for |delta_i| <= d_i, rigorous (not first order): with
    sigma = sqrt(var + eps), rho = rms(d) + mean(d) >= |sigma' - sigma|,
      |dy_i| <= |gamma_i| (d_i + mean d + |xh_i| rho) / (sigma - rho)."""
    z = pre64.double()
    mean = z.mean(-1, keepdim=True)
    sigma = (((z - mean) ** 2).mean(-1, keepdim=True) + R.eps32(eps)).sqrt()
    rho = (d * d).mean(-1, keepdim=True).sqrt() + d.mean(-1, keepdim=True)
    assert (rho < 0.5 * sigma).all()
    return gam.double().abs() * (d + d.mean(-1, keepdim=True) + ((z - mean) / sigma).abs() * rho) / (sigma - rho)


@pytest.mark.parametrize('variant', ['generic-ffn', 'ffn-off'])
def test_attn_out_ffn_norm_epilogues(K, variant):
    """y = LN2(x + W2 relu(W1 x + b1) + b2), x = LN1(R + A Wo^T + bo) rounded to f16 once: offsets of
    100 on out_proj.bias (norm1) and linear2.bias (norm2).  A, Wo dyadic: norm1's pre-activation is
    exact.  The kernel's x and the reference's are two f16 roundings of values 4x torch's f32 error
    apart at most, so they differ by up to dx = 4 t1 + one f16 ulp wherever a rounding flips; y is
    bounded by its own output rounding + 4x torch's error on norm2 + the majorant of dx propagated
    through |W1|, the hidden rounding, |W2| (relu is 1-Lipschitz: sign flips included) and norm2
    (_ln_perturbation), nothing added.
      generic-ffn: random W1, W2 -- the whole chain, the bound dominated by the propagated ulp;
      ffn-off: W1 = 0, b1 = 0 (h = 0: x + b2 reaches norm2 as it is) and norm1's gamma, beta scaled by
               1/64, so dx ~ 3e-5 and norm2's conditioning at offset 100 is pinned to ~1e-4, a
               twentieth of what a one-pass variance loses there."""
    M, D, Fh, dtype = 70, 256, 64, F16
    u16 = R.OUT_ROUND[dtype]
    g = torch.Generator().manual_seed(70)
    a, wo = _dyadic((M, D), g, 0.5, 2), _dyadic((D, D), g, 0.125, 2)
    bo = 100.0 + torch.randn(D, generator=g)
    r = torch.randn(M, D, generator=g).to(dtype)
    s1 = 1.0 if variant == 'generic-ffn' else 1.0 / 64
    gam1, bet1 = (t * s1 for t in _ln_params(D, g))
    gam2, bet2 = _ln_params(D, g)
    w1 = (torch.randn(Fh, D, generator=g) / D ** 0.5).to(dtype)
    b1 = torch.randn(Fh, generator=g) * 0.5
    w2 = (torch.randn(D, Fh, generator=g) / Fh ** 0.5).to(dtype)
    b2 = 100.0 + torch.randn(D, generator=g)
    if variant == 'ffn-off':
        w1, b1 = torch.zeros_like(w1), torch.zeros_like(b1)
    out_proj, lin1, lin2 = torch.nn.Linear(D, D), torch.nn.Linear(D, Fh), torch.nn.Linear(Fh, D)
    n1, n2 = torch.nn.LayerNorm(D, eps=EPS), torch.nn.LayerNorm(D, eps=EPS)
    with torch.no_grad():
        for p, v in ((out_proj.weight, wo), (out_proj.bias, bo), (lin1.weight, w1), (lin1.bias, b1), (lin2.weight, w2),
                     (lin2.bias, b2), (n1.weight, gam1), (n1.bias, bet1), (n2.weight, gam2), (n2.bias, bet2)):
            p.copy_(v)
    W1, W2 = lin1.weight.detach().double(), lin2.weight.detach().double()
    B1, B2 = lin1.bias.detach().double(), lin2.bias.detach().double()
    pre1 = a @ wo.t() + out_proj.bias.detach().double() + r.double()
    x64, t1 = R.ln_epilogue_yardstick(pre1, n1.weight.detach(), n1.bias.detach(), EPS)
    xr = x64.to(dtype).double()
    dx = 4 * t1 + u16 * (x64.abs() + 4 * t1)
    hr = torch.relu(xr @ W1.t() + B1).to(dtype).double()
    pre2 = xr + hr @ W2.t() + B2
    lin_dx = dx @ W1.abs().t()
    dh = lin_dx * (1 + u16) + u16 * hr.abs() + (D + 2) * R.U32 * (xr.abs() @ W1.abs().t() + B1.abs())
    dpre = dx + dh @ W2.abs().t() + Fh * R.U32 * (hr.abs() @ W2.abs().t())
    extra = _ln_perturbation(dpre, pre2, n2.weight.detach())
    print(f'attn_out_ffn {variant}: norm1 torch CPU f32 max err {t1:.3e}; max dx {dx.max().item():.3e}, max propagated '
          f'pre-activation majorant {dpre.max().item():.3e}, max of its image under norm2 {extra.max().item():.3e}')
    mods = [m.cuda() for m in (out_proj, n1, lin1, lin2, n2)]
    y = K.attn_out_ffn_fused(a.to(dtype).cuda(), mods[0], r.cuda(), mods[1], mods[2], mods[3], mods[4], force=True)
    _check(y, pre2, gam2, bet2, dtype, f'attn_out_ffn_fused {variant} M={M} D={D} F={Fh} f16 +100', extra=extra)
