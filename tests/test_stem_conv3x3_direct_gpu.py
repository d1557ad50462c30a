"""Direct tests of the front of the backbone -- stem_conv_kernel, stem_img_kernel, stem_pool_kernel
(csrc/stem.hip) and conv3x3_c64_kernel (csrc/conv3x3.hip) -- path by path, against f64 references
(tests/direct_refs.py, checked on the CPU by test_direct_refs_cpu.py).

Two operand classes, the tiled GEMM module's: EXACT (dyadic image / activation, weights, scale and bias:
every f32 partial sum is exact in any order, the kernel must equal the f64 result rounded once to the
output type on every element) and GENERIC (randn rounded to nearest even by torch, every element under
gemm_generic_bound; a pooled element under the 3x3 / 2 maximum of the conv map's bounds, because
|max a - max b| <= the maximum over the window of |a - b|).  Every conv2d_nhwc call asserts through
gemm_last_kernel that the family under test served it; the two image entry points have no such
report and are called directly.  KINET_STEM_CONV3X3_LOG names a file that receives the module's figures (profiles/stem_conv3x3_direct.log).

On the figures: the bound's leading term, OUT_ROUND |ref|, is 2^-8 for bf16 -- exactly half an ulp at the
bottom of a binade -- so ONE correct output rounding reaches err / bound ~ 0.98 there (torch's own f32
convolution rounded once gives the same 0.983 on the CPU, test_direct_refs_cpu.py); for f16 it is 2^-10,
twice the half ulp, and the worst ratio is ~ 0.49.  A ratio near 1 in bf16 is the output rounding, not the kernel."""
import os
import time

import pytest
import torch

import direct_refs as R

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
DTYPES = [BF16, F16]
SENTINEL = 77.0

_LOG = {'t0': time.time(), 'generic': {}, 'exact': {}}


def _name(dt):
    return str(dt).replace('torch.', '')


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


@pytest.fixture(scope='module')
def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    lines = [f'module wall time: {time.time() - _LOG["t0"]:.1f} s', 'exact class, elements not equal to the expected value:']
    lines += [f'  {k}: {bad} of {n}' for k, (bad, n) in sorted(_LOG['exact'].items())]
    lines += ['generic class, worst err / bound:']
    lines += [f'  {k}: {v:.3f}' for k, v in sorted(_LOG['generic'].items())]
    print('\n'.join(lines))
    path = os.environ.get('KINET_STEM_CONV3X3_LOG')
    if path:
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


def _check(tag, what, y, cls, pre, bound_of, odt, scale=None):
    """Compare a kernel's output rows with the f64 value `pre` (the same rows): equality with pre rounded once
    (exact), or |err| <= bound_of() per element (generic)."""
    torch.cuda.synchronize()
    got = y.detach().cpu().reshape(pre.shape)
    assert got.dtype == odt
    assert not torch.isnan(got.float()).any(), f'{what}: NaN in the output'
    if cls == 'exact':
        assert R.exact_headroom(pre, scale, odt).all(), f'{what}: the case cannot resolve one dropped product'
        bad = int((got != pre.to(odt)).sum())
        b0, n0 = _LOG['exact'].get(tag, (0, 0))
        _LOG['exact'][tag] = (b0 + bad, n0 + pre.numel())
        print(f'{tag} {what} exact: {bad} of {pre.numel()} differ')
        assert bad == 0, f'{what}: {bad} of {pre.numel()} elements differ from the f64 result rounded once'
        assert torch.equal(got, pre.to(odt))
    else:
        ratio = float(((got.double() - pre).abs() / bound_of()).max())
        _LOG['generic'][tag] = max(_LOG['generic'].get(tag, 0.0), ratio)
        print(f'{tag} {what} generic: worst err / bound {ratio:.3f}')
        assert ratio <= 1.0, f'{what}: err / bound = {ratio}'


def _case(kind, shape, cls, dtype, variant=None, dev='cpu'):
    return R.front_case(kind, shape, cls, None if cls == 'exact' else dtype, variant, dev)


# ------------------------------------------------------------------------ conv3x3_c64_kernel
def _c3(K, tag, shape, cls, dtype, epilogues=R.C3_EPILOGUES, ldc=None, dev='cpu'):
    c = _case('c3', shape, cls, dtype, dev=dev)
    B, H, W = shape
    x, wp = c['x'].to(dtype).cuda(), K.pack_conv_weight(c['w'].cuda(), dtype)
    for name in epilogues:
        sb, relu = R.C3_EPILOGUES[name]
        kw = dict(scale=c['scale'].cuda(), bias=c['bias'].cuda()) if sb else {}
        wide = None
        if ldc:
            wide = torch.full((B, H, W, ldc), SENTINEL, dtype=dtype).cuda()
            kw['out'] = wide[..., :64]
            assert kw['out'].stride(2) == ldc
        y = K.conv2d_nhwc(x, wp, 1, 1, relu=relu, ksplit=1, **kw)
        got = K.gemm_last_kernel()
        assert got == ('conv3x3', 0, 0), f'{got} served the call, not the direct 3x3 kernel'
        pre, maj, s = R.front_expected(c, sb, relu)
        if wide is not None:
            y = y.contiguous()
        _check(tag, f'{shape} {name}', y, cls, pre,
               lambda: R.gemm_generic_bound(c['absprod'], c['K'], maj, pre, dtype, s), dtype, s)
        if not relu:
            assert (y < 0).any(), f'{shape} {name}: no negative output passed through'
        if wide is not None:
            assert (wide[..., 64:] == SENTINEL).all(), f'{shape} {name}: the 32 channels beside the output were written'


@pytest.mark.parametrize('cls', ['exact', 'generic'])
@pytest.mark.parametrize('shape', R.C3_SHAPES, ids=str)
@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
def test_conv3x3_shapes(K, dtype, shape, cls):
    _c3(K, f'conv3x3 shapes {_name(dtype)}', shape, cls, dtype)


@pytest.mark.parametrize('cls', ['exact', 'generic'])
@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
def test_conv3x3_persistent(K, cus, dtype, cls):
    """More than 2 tiles per workgroup (one workgroup per CU): some walk three tiles, reusing both halo
    buffers behind the vmcnt(4) wait."""
    shape = R.c3_persistent_shape(cus)
    assert shape[0] * 9 > 2 * cus
    _c3(K, f'conv3x3 persistent {_name(dtype)}', shape, cls, dtype, epilogues=('full', 'plain'), dev='cuda')


@pytest.mark.parametrize('cls', ['exact', 'generic'])
@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
def test_conv3x3_ldc96(K, dtype, cls):
    """out = the first 64 channels of a (B, H, W, 96) buffer: the other 32 of every pixel stay as they were."""
    _c3(K, f'conv3x3 ldc96 {_name(dtype)}', R.C3_LDC_SHAPE, cls, dtype, epilogues=('full', 'plain'), ldc=96)


# ---------------------------------------------------------- stem_conv_kernel, stem_img_kernel
def _stem_args(K, c, dtype):
    return c['x'].cuda(), K.pack_stem_weight(c['w'].cuda(), dtype, 24), c['scale'].cuda(), c['bias'].cuda()


def _stem(K, group, shape, cls, dtype, dev='cpu'):
    c = _case('stem', shape, cls, dtype, dev=dev)
    img, wp, scale, bias = _stem_args(K, c, dtype)
    pre, maj, s = R.front_expected(c)
    bound = [None]

    def bound_of():
        if bound[0] is None:
            bound[0] = R.gemm_generic_bound(c['absprod'], c['K'], maj, pre, dtype, s)
        return bound[0]
    xp = K.pack_image_kwfold(img, dtype, 7, 2, 3, 24)
    y0 = K.conv2d_nhwc(xp, wp, (2, 1), (3, 0), scale=scale, bias=bias, relu=True)
    got = K.gemm_last_kernel()
    assert got == ('stem', 0, 0), f'{got} served the call, not the folded stem kernel'
    assert y0.shape == (c['B'], c['Ho'], c['Wo'], 64)
    _check(f'stem_conv {group} {_name(dtype)}', f'{shape}', y0, cls, pre, bound_of, dtype, s)
    y1 = K.stem_conv_image(img, wp, scale, bias, dtype)
    assert y1.shape == y0.shape
    _check(f'stem_img {group} {_name(dtype)}', f'{shape}', y1, cls, pre, bound_of, dtype, s)


@pytest.mark.parametrize('cls', ['exact', 'generic'])
@pytest.mark.parametrize('shape', R.STEM_SHAPES, ids=str)
@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
def test_stem_conv_and_image_shapes(K, dtype, shape, cls):
    """Both kernels are held to the f64 reference independently of each other."""
    _stem(K, 'shapes', shape, cls, dtype)


@pytest.mark.parametrize('cls', ['exact', 'generic'])
@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
def test_stem_conv_and_image_persistent(K, dtype, cls):
    """1026 tiles on the 512-wide grid: workgroups 0 and 1 walk three tiles (the one-tile-ahead loads twice)."""
    _stem(K, 'persistent', R.STEM_PERSISTENT, cls, dtype, dev='cuda')


def test_stem_conv_without_scale_bias_relu(K):
    """stem_conv_kernel's optional epilogue (the image entry points always scale, shift and clamp): negative
    outputs pass through."""
    shape = R.STEM_MULTI_TILE
    for dtype in DTYPES:
        for cls in ('exact', 'generic'):
            c = _case('stem', shape, cls, dtype)
            img, wp, _, _ = _stem_args(K, c, dtype)
            y = K.conv2d_nhwc(K.pack_image_kwfold(img, dtype, 7, 2, 3, 24), wp, (2, 1), (3, 0))
            assert K.gemm_last_kernel() == ('stem', 0, 0)
            pre, maj, s = R.front_expected(c, False, False)
            _check(f'stem_conv plain {_name(dtype)}', f'{shape}', y, cls, pre,
                   lambda: R.gemm_generic_bound(c['absprod'], c['K'], maj, pre, dtype, s), dtype, s)
            assert (y < 0).any()


# ------------------------------------------------------------------------- stem_pool_kernel
def _pool(K, group, shape, cls, dtype, segs, variant=None, dev='cpu'):
    c = _case('stem', shape, cls, dtype, variant, dev)
    args = _stem_args(K, c, dtype)
    pre, maj, s = R.front_expected(c)
    geo = (c['B'], c['Ho'], c['Wo'])
    Hp, Wp = (c['Ho'] - 1) // 2 + 1, (c['Wo'] - 1) // 2 + 1
    tag = f'stem_pool {group} {_name(dtype)}'
    if cls == 'exact':
        assert R.exact_headroom(pre, s, dtype).all(), f'{shape}: the conv map cannot resolve one dropped product'
        want = R.pool_rows(pre.to(dtype), *geo)                # the pool of the once-rounded conv map
    else:
        want = R.pool_rows(pre, *geo)
        pbound = R.pool_rows(R.gemm_generic_bound(c['absprod'], c['K'], maj, pre, dtype, s), *geo)
    out = None
    for seg in segs:
        y = K.stem_pool_image(*args, dtype, seg_tiles=seg)
        torch.cuda.synchronize()
        assert y.shape == (c['B'], Hp, Wp, 64) and y.dtype == dtype
        got = y.cpu().reshape(want.shape)
        assert not torch.isnan(got.float()).any(), f'{shape} seg_tiles={seg}: NaN in the output'
        if cls == 'exact':
            bad = int((got != want).sum())
            b0, n0 = _LOG['exact'].get(tag, (0, 0))
            _LOG['exact'][tag] = (b0 + bad, n0 + want.numel())
            print(f'{tag} {shape} seg_tiles={seg} exact: {bad} of {want.numel()} differ')
            assert bad == 0, f'{shape} seg_tiles={seg}: {bad} of {want.numel()} pooled elements differ'
            assert torch.equal(got, want)
        else:
            ratio = float(((got.double() - want).abs() / pbound).max())
            _LOG['generic'][tag] = max(_LOG['generic'].get(tag, 0.0), ratio)
            print(f'{tag} {shape} seg_tiles={seg} generic: worst err / bound {ratio:.3f}')
            assert ratio <= 1.0, f'{shape} seg_tiles={seg}: err / bound = {ratio}'
        out = got
    return out


@pytest.mark.parametrize('shape', R.POOL_SHAPES, ids=str)
@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
def test_stem_pool_geometries(K, dtype, shape):
    for cls in ('exact', 'generic'):
        _pool(K, 'geometries', shape, cls, dtype, R.POOL_SEG_TILES)


@pytest.mark.parametrize('cls', ['exact', 'generic'])
@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
def test_stem_pool_many_units(K, dtype, cls):
    """1026 work units of one tile (two of three start with a pre step) on the 512-wide grid."""
    _pool(K, 'units>1024', R.STEM_PERSISTENT, cls, dtype, (1,), dev='cuda')


@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
def test_stem_pool_bias_one_borders(K, dtype):
    """bias = 1 on every channel: the conv rows and columns past the map's edge (relu(bias) = 1 of a zero input)
    would win the last pooled row's and column's maxima if they were not parked as -0.0."""
    _pool(K, 'bias1', R.POOL_BIAS1_SHAPE, 'exact', dtype, R.POOL_SEG_TILES, variant='bias1')


@pytest.mark.parametrize('dtype', DTYPES, ids=_name)
def test_stem_pool_zero_weights(K, dtype):
    """All weights and biases zero: the output is zero everywhere, and no element carries any of its low 15
    bits (a -0.0 of the parked padding would still compare equal; anything else would not)."""
    for seg in R.POOL_SEG_TILES:
        got = _pool(K, 'zero', R.POOL_ZERO_SHAPE, 'exact', dtype, (seg,), variant='zero')
        assert (got == 0).all()
        assert (got.view(torch.int16) & 0x7FFF == 0).all()
