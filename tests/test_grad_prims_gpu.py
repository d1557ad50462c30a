"""Direct tests of the backward-pass primitives of csrc/grad.hip -- transpose, im2col / col2im,
gemm_tn -- against plain references (tests/direct_refs.py): bit-exact where the kernel only moves
data, f64 with a worst-case summation bound where it adds.  Seeded inputs; shapes at tile, K-step
and split-K edges, strided operands with misaligned bases, accumulate and strided outputs."""
import pytest
import torch

import direct_refs as R
from test_gemm_gpu import _x3_bound

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


@pytest.fixture
def gemm_flags():
    """Select the GEMM kernel family for one test and restore the default afterwards."""
    from kinet_amd import _native
    lib = _native.lib()
    yield lib.kinet_gemm_set_flags
    lib.kinet_gemm_set_flags(0)


@pytest.fixture(params=['highest', 'high'])
def precision(request):
    """'highest': the exact-f32 MFMA kernel; 'high': f32 operands as three bf16 passes (X3)."""
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision(request.param)
    yield request.param
    torch.set_float32_matmul_precision(prev)


@pytest.fixture
def x3_precision():
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision('high')
    yield
    torch.set_float32_matmul_precision(prev)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------ transpose
@pytest.mark.parametrize('R_,C', [(1, 1), (1, 40), (31, 33), (32, 32), (65, 7), (300, 1000)])
@pytest.mark.parametrize('dtype', DTYPES)
def test_transpose2d_bit_exact(K, dtype, R_, C):
    x = torch.randn(R_, C, generator=_gen(R_ * C)).to(dtype)
    y = K.transpose2d(x.cuda())
    assert y.shape == (C, R_) and y.is_contiguous()
    assert torch.equal(y.cpu(), x.t().contiguous())
    # row-strided source: ld_src > cols, base 3 elements into the row (not 16-byte aligned)
    big = torch.randn(R_, C + 9, generator=_gen(R_ + C)).to(dtype)
    src = big.cuda()[:, 3:3 + C]
    assert src.stride(0) == C + 9
    y2 = K.transpose2d(src)
    assert torch.equal(y2.cpu(), big[:, 3:3 + C].t().contiguous())


# ----------------------------------------------------------------------- im2col / col2im
# (KH, KW, stride, pad, H, W) on B = 2
CONV_GEOMS = [
    (3, 3, 1, 1, 13, 18), (3, 3, 2, 1, 13, 18), (1, 1, 2, 0, 13, 18), (7, 7, 2, 3, 13, 18),
    (3, 3, 2, 0, 14, 18),                       # the last input row is in no window
    (1, 3, (2, 1), (0, 1), 13, 18), (3, 1, (1, 2), (1, 0), 13, 18),
    (5, 3, 1, (2, 1), 2, 18),                   # kernel taller than the unpadded image
]
CONV_IDS = ['3x3s1', '3x3s2', '1x1s2', '7x7s2', '3x3s2p0_h14', '1x3', '3x1', '5x3_h2']


def _conv_x(H, W, C, dtype, seed=0):
    return torch.randn(2, H, W, C, generator=_gen(seed + H * W + C)).to(dtype)


@pytest.mark.parametrize('C', [4, 8, 36, 64])
@pytest.mark.parametrize('geom', CONV_GEOMS, ids=CONV_IDS)
def test_im2col_bit_exact(K, geom, C):
    KH, KW, stride, pad, H, W = geom
    for dtype in DTYPES:
        x = _conv_x(H, W, C, dtype)
        # pure data movement: unfold the (exactly representable) values in f32, cast back
        ref = R.unfold_nhwc(x.float(), KH, KW, stride, pad).to(dtype)
        cols = K.im2col_nhwc(x.cuda(), KH, KW, stride, pad)
        assert cols.dtype == dtype and cols.shape == ref.shape
        assert torch.equal(cols.cpu(), ref)


@pytest.mark.parametrize('C', [4, 8, 36, 64])
@pytest.mark.parametrize('geom', CONV_GEOMS, ids=CONV_IDS)
def test_col2im_vs_f64_fold(K, geom, C):
    KH, KW, stride, pad, H, W = geom
    Ho, Wo = R.out_size(H, W, KH, KW, stride, pad)
    shape = (2, H, W, C)
    base = torch.randn(2 * Ho * Wo, KH * KW * C, generator=_gen(KH * 100 + KW * 10 + C))
    for dtype in DTYPES:
        cols = base.to(dtype)
        ref = R.fold_nhwc(cols.double(), shape, KH, KW, stride, pad)
        # every pixel sums <= KH*KW taps in f32: worst case of any order, KH*KW u fold(|cols|);
        # 16-bit: plus one output rounding
        bound = KH * KW * R.U32 * R.fold_nhwc(cols.double().abs(), shape, KH, KW, stride, pad)
        tol = bound + R.OUT_ROUND[dtype] * ref.abs()
        dx = K.col2im_nhwc(cols.cuda(), shape, KH, KW, stride, pad)
        assert dx.dtype == dtype and dx.shape == shape
        err = (dx.double().cpu() - ref).abs()
        assert (err <= tol).all(), (dtype, err.max().item())
        if dtype == torch.float32:
            # adjoint identity <im2col(x), c> = <x, col2im(c)> in f64: im2col is exact, so the two
            # sides differ by at most <|x|, bound>
            x = _conv_x(H, W, C, dtype, seed=1)
            xc = K.im2col_nhwc(x.cuda(), KH, KW, stride, pad).double().cpu()
            lhs = (xc * cols.double()).sum().item()
            rhs = (x.double() * dx.double().cpu()).sum().item()
            assert abs(lhs - rhs) <= (x.double().abs() * bound).sum().item(), (lhs, rhs)


def test_col2im_uncovered_row_is_exact_zero(K):
    """3x3 / stride 2 / pad 0 on H = 14: input row 13 is in no window -- no taps, exact zeros."""
    KH, KW, stride, pad, H, W = CONV_GEOMS[4]
    Ho, Wo = R.out_size(H, W, KH, KW, stride, pad)
    cols = torch.randn(2 * Ho * Wo, 9 * 8, generator=_gen(2))
    dx = K.col2im_nhwc(cols.cuda(), (2, H, W, 8), KH, KW, stride, pad).cpu()
    assert (dx[:, 13] == 0).all() and (dx[:, :13] != 0).any()


def test_im2col_col2im_channels_not_multiple_of_4_raise(K):
    x = torch.zeros(2, 13, 18, 6, device='cuda')
    with pytest.raises(RuntimeError, match='multiple of 4'):
        K.im2col_nhwc(x, 3, 3, 1, 1)
    with pytest.raises(RuntimeError, match='multiple of 4'):
        K.col2im_nhwc(torch.zeros(2 * 13 * 18, 54, device='cuda'), (2, 13, 18, 6), 3, 3, 1, 1)


# --------------------------------------------------------------------------------- gemm_tn
TN_SHAPES = [(1, 1, 1), (15, 3, 5), (16, 64, 64), (17, 65, 63), (63, 70, 33), (64, 64, 1), (129, 1, 64),
             (1000, 130, 67),
             (8200, 64, 64),      # split-K, one tile
             (8192, 64, 64),      # split-K with 64 slices: a multiple of 8, XCD slice placement live
             (8200, 200, 130)]    # split-K with a slice count that is no multiple of 8
TN_STRIDED = [(17, 65, 63), (1000, 130, 67), (8200, 64, 64), (8192, 64, 64)]


def _tn_check(y, ref, bound, extra=None):
    err = (y.double().cpu() - ref).abs()
    tol = bound if extra is None else bound + extra
    assert (err <= tol).all(), (err.max().item(), (err / tol).max().item())


def _bound(precision, a, b):
    a64, b64 = a.double(), b.double()
    return R.tn_exact_bound(a64, b64) if precision == 'highest' else _x3_bound(a64.T, b64)


def _round_of(total, bound):
    # one f32 rounding of a sum whose computed value is within `bound` of `total`
    return R.U32 * (total.abs() + bound)


@pytest.mark.parametrize('Kd,M,N', TN_SHAPES)
def test_gemm_tn_f32_vs_f64(K, precision, Kd, M, N):
    """f32 operands: the exact-f32 kernel ('highest') within the summation worst case, the default
    X3 kernel ('high') within the three-pass bound."""
    a, b, ref = R.tn_operands(Kd, M, N, torch.float32)
    y = K.gemm_tn(a.cuda(), b.cuda())
    assert y.shape == (M, N) and y.dtype == torch.float32
    _tn_check(y, ref, _bound(precision, a, b))


@pytest.mark.parametrize('Kd,M,N', TN_SHAPES)
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_gemm_tn_16bit_vs_f64(K, dtype, Kd, M, N):
    """16-bit operands widened to f32: products exact, f32 accumulation; f32 result."""
    a, b, ref = R.tn_operands(Kd, M, N, dtype)
    y = K.gemm_tn(a.cuda(), b.cuda())
    assert y.dtype == torch.float32
    _tn_check(y, ref, R.tn_exact_bound(a.double(), b.double()))


@pytest.mark.parametrize('Kd,M,N', TN_SHAPES)
@pytest.mark.parametrize('flag', [128, 256])
def test_gemm_tn_x3_flag_variants(K, gemm_flags, x3_precision, flag, Kd, M, N):
    """'high' precision on the fallback X3 kernel (flag 128: the 16-deep kernel splitting at
    fragment-read time) and with the XCD slice placement off (flag 256)."""
    a, b, ref = R.tn_operands(Kd, M, N, torch.float32)
    gemm_flags(flag)
    y = K.gemm_tn(a.cuda(), b.cuda())
    gemm_flags(0)
    _tn_check(y, ref, _x3_bound(a.double().T, b.double()))


@pytest.mark.parametrize('Kd,M,N', [(17, 65, 63), (1000, 130, 67), (8200, 64, 64), (8200, 200, 130)])
def test_gemm_tn_accumulate(K, precision, Kd, M, N):
    """accumulate=True onto a non-zero out (a single-slice and split-K cases): out0 + a^T b within
    the product's bound plus one f32 rounding of the sum."""
    a, b, ref = R.tn_operands(Kd, M, N, torch.float32)
    out0 = torch.randn(M, N, generator=_gen(Kd + M)) * 10
    out = out0.cuda()
    ret = K.gemm_tn(a.cuda(), b.cuda(), out=out, accumulate=True)
    assert ret.data_ptr() == out.data_ptr()
    bound = _bound(precision, a, b)
    total = out0.double() + ref
    _tn_check(out, total, bound, _round_of(total, bound))
    assert not torch.equal(out.cpu(), out0)


@pytest.mark.parametrize('Kd,M,N', [(17, 65, 63), (8200, 64, 64)])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_gemm_tn_accumulate_16bit(K, dtype, Kd, M, N):
    a, b, ref = R.tn_operands(Kd, M, N, dtype)
    out0 = torch.randn(M, N, generator=_gen(Kd + N)) * 10
    out = out0.cuda()
    K.gemm_tn(a.cuda(), b.cuda(), out=out, accumulate=True)
    bound = R.tn_exact_bound(a.double(), b.double())
    total = out0.double() + ref
    _tn_check(out, total, bound, _round_of(total, bound))


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('Kd,M,N', [(17, 65, 63), (63, 70, 33), (8200, 64, 64)])
def test_gemm_tn_column_slice_out(K, precision, Kd, M, N, accumulate):
    """out= a column slice of a wider buffer (ldc > N): the columns outside stay unchanged."""
    a, b, ref = R.tn_operands(Kd, M, N, torch.float32)
    wide0 = torch.randn(M, N + 11, generator=_gen(Kd + N + 1))
    wide = wide0.cuda()
    out = wide[:, 5:5 + N]
    assert out.stride(0) == N + 11
    K.gemm_tn(a.cuda(), b.cuda(), out=out, accumulate=accumulate)
    torch.cuda.synchronize()
    got = wide.cpu()
    assert torch.equal(got[:, :5], wide0[:, :5]) and torch.equal(got[:, 5 + N:], wide0[:, 5 + N:])
    bound = _bound(precision, a, b)
    total = (wide0[:, 5:5 + N].double() + ref) if accumulate else ref
    _tn_check(got[:, 5:5 + N], total, bound, _round_of(total, bound) if accumulate else None)


@pytest.mark.parametrize('Kd,M,N', TN_STRIDED)
def test_gemm_tn_strided_misaligned_operands(K, precision, Kd, M, N):
    """a = A_big[:, 1:1+M], b = B_big[:, 3:3+N]: lda > M, ldb > N, bases 4-byte but not 16-byte
    aligned (the scalar branch of the exact kernel's loader); stride(0) is passed through, so no
    copy is made."""
    g = _gen(Kd + M + N)
    A_big = torch.randn(Kd, M + 6, generator=g)
    B_big = torch.randn(Kd, N + 9, generator=g)
    Ag, Bg = A_big.cuda(), B_big.cuda()
    a, b = Ag[:, 1:1 + M], Bg[:, 3:3 + N]
    assert a.data_ptr() % 16 == 4 and b.data_ptr() % 16 == 12 and a.stride(0) == M + 6
    ac, bc = A_big[:, 1:1 + M], B_big[:, 3:3 + N]
    ref = ac.double().T @ bc.double()
    y = K.gemm_tn(a, b)
    _tn_check(y, ref, _bound(precision, ac, bc))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_gemm_tn_strided_16bit(K, dtype):
    Kd, M, N = 1000, 130, 67
    g = _gen(3)
    A_big = torch.randn(Kd, M + 5, generator=g).to(dtype)
    B_big = torch.randn(Kd, N + 3, generator=g).to(dtype)
    ac, bc = A_big[:, 1:1 + M], B_big[:, 3:3 + N]
    y = K.gemm_tn(A_big.cuda()[:, 1:1 + M], B_big.cuda()[:, 3:3 + N])
    _tn_check(y, ac.double().T @ bc.double(), R.tn_exact_bound(ac.double(), bc.double()))


@pytest.mark.parametrize('dtype', DTYPES)
def test_gemm_tn_empty_k(K, precision, dtype):
    """K = 0: out becomes zeros (a strided out: only its own columns), or stays unchanged under
    accumulate."""
    M, N = 65, 63
    a = torch.zeros(0, M, dtype=dtype, device='cuda')
    b = torch.zeros(0, N, dtype=dtype, device='cuda')
    wide = torch.full((M, N + 4), 2.5, device='cuda')
    K.gemm_tn(a, b, out=wide[:, 2:2 + N])
    torch.cuda.synchronize()
    assert (wide[:, 2:2 + N] == 0).all() and (wide[:, :2] == 2.5).all() and (wide[:, 2 + N:] == 2.5).all()
    keep = torch.full((M, N), 1.25, device='cuda')
    K.gemm_tn(a, b, out=keep, accumulate=True)
    torch.cuda.synchronize()
    assert (keep == 1.25).all()
    y = K.gemm_tn(a, b)
    assert y.shape == (M, N) and (y == 0).all()
