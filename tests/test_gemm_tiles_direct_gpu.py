"""Direct tests of the tiled GEMM / implicit-convolution kernel (csrc/gemm.hip gemm_kernel, its
LDS-DMA staged twin of flag 16, splitk_finalize_kernel), tile by tile, against f64 references
(tests/direct_refs.py, checked on the CPU by test_direct_refs_cpu.py).

Every case forces the tile (kinet_gemm_force_tile) and asserts through kinet_gemm_last_kernel that the
intended kernel family and tile served it.  Two operand classes: EXACT (small dyadic values: every
f32 partial sum is exact in any order, the expected output is the f64 result rounded once, compared
for equality) and GENERIC (randn under a per-element running-error bound).  KINET_GEMM_TILES_LOG names
a file that receives the module's figures (profiles/gemm_tiles_direct.log)."""
import os
import time

import pytest
import torch

import direct_refs as R

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
TYPES = [(BF16, BF16), (BF16, F32), (BF16, F16), (F16, F16), (F16, F32), (F32, F32)]
SENTINEL = 77.0
NO_SPECIAL = 4 | 32 | 1024      # never the resident-weight, stem or direct 3x3 kernels (test_gemm_rw_direct_gpu.py,
#                                 test_stem_conv3x3_direct_gpu.py hold those to their own f64 references)
DMA4 = 16                       # LDS-DMA staging of the 4-wave tiles

_LOG = {'t0': time.time(), 'generic': {}, 'exact_bad': 0, 'exact_n': 0, 'kernels': set()}


def _name(dt):
    return str(dt).replace('torch.', '')


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    lines = [f'module wall time: {time.time() - _LOG["t0"]:.1f} s',
             f'exact class: {_LOG["exact_bad"]} of {_LOG["exact_n"]} elements not equal to the expected value',
             'kernels reached: ' + ', '.join(f'{f} {bm}x{bn}' for f, bm, bn in sorted(_LOG['kernels'])),
             'generic class, worst err / bound per test:']
    lines += [f'  {k}: {v:.3f}' for k, v in sorted(_LOG['generic'].items())]
    print('\n'.join(lines))
    path = os.environ.get('KINET_GEMM_TILES_LOG')
    if path:
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


@pytest.fixture
def knobs():
    """force_tile / set_flags for one test, restored afterwards."""
    from kinet_amd import _native

    class Knobs:
        @staticmethod
        def tile(bm, bn):
            _native.call('kinet_gemm_force_tile', bm, bn)

        @staticmethod
        def flags(v):
            _native.lib().kinet_gemm_set_flags(v)
    yield Knobs
    _native.lib().kinet_gemm_force_tile(0, 0)
    _native.lib().kinet_gemm_set_flags(0)


@pytest.fixture
def x3_precision():
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision('high')
    yield
    torch.set_float32_matmul_precision(prev)


def _ran(K, family, bm, bn):
    got = K.gemm_last_kernel()
    assert got == (family, bm, bn), f'{got} served the call, not {(family, bm, bn)}'
    _LOG['kernels'].add(got)


def _check(tag, what, y, cls, acc64, absprod, Kd, odt, scale=None, bias=None, res=None, relu=False, row_mask=None,
           x3=False):
    """Compare the kernel's (M, N) output with the f64 epilogue of acc64."""
    torch.cuda.synchronize()
    pre, maj = R.epilogue64(acc64, scale, bias, res, relu, row_mask)
    got = y.detach().cpu().reshape(pre.shape)
    assert got.dtype == odt
    if cls == 'exact':
        assert R.exact_headroom(pre, scale, odt).all(), f'{what}: the case cannot resolve one dropped product'
        bad = int((got != pre.to(odt)).sum())
        _LOG['exact_bad'] += bad
        _LOG['exact_n'] += pre.numel()
        print(f'{tag} {what} exact: {bad} of {pre.numel()} differ')
        assert bad == 0, f'{what}: {bad} of {pre.numel()} elements differ from the f64 result rounded once'
    else:
        err = (got.double() - pre).abs()
        bound = R.gemm_generic_bound(absprod, Kd, maj, pre, odt, scale, x3=x3)
        ratio = float((err / bound).max())
        _LOG['generic'][tag] = max(_LOG['generic'].get(tag, 0.0), ratio)
        print(f'{tag} {what} generic: worst err / bound {ratio:.3f}')
        assert ratio <= 1.0, f'{what}: err / bound = {ratio}'


# ----------------------------------------------------------------------------- the GEMM table
def _gemm_table(K, knobs, tag, bm, bn, cdt, odt, flags, family, classes=('exact', 'generic'), x3=False, table=None):
    knobs.flags(flags)
    knobs.tile(bm, bn)
    for M, N, Kd in table or R.gemm_table(bm, bn, cdt == F32):
        for cls in classes:
            x, w, acc, ap = R.gemm_case(M, N, Kd, cdt, cls)
            y = K.linear(x.to(cdt).cuda(), w.to(cdt).cuda(), out_dtype=odt)
            _ran(K, family, bm, bn)
            if x3 and cls == 'generic':
                ap = R.x3_bound(x.double(), w.double().T)
            _check(tag, f'({M}, {N}, {Kd})', y, cls, acc, ap, Kd, odt, x3=x3)


@pytest.mark.parametrize('cdt,odt', TYPES, ids=lambda d: _name(d))
@pytest.mark.parametrize('bm,bn', R.GEMM_TILES)
def test_gemm_table(K, knobs, bm, bn, cdt, odt):
    _gemm_table(K, knobs, f'gemm {bm}x{bn} {_name(cdt)}->{_name(odt)}', bm, bn, cdt, odt, 4, 'tiled')


@pytest.mark.parametrize('bm,bn', R.GEMM_TILES)
def test_gemm_table_x3(K, knobs, x3_precision, bm, bn):
    """KINET_F32_X3 (three bf16 MFMA passes): the exact class is exact there too (the operands have
    no low part), one generic case under x3_bound."""
    tag = f'gemm x3 {bm}x{bn}'
    _gemm_table(K, knobs, tag, bm, bn, F32, F32, 4, 'tiled', classes=('exact',), x3=True)
    _gemm_table(K, knobs, tag, bm, bn, F32, F32, 4, 'tiled', classes=('generic',), x3=True,
                table=[(2 * bm + 3, 2 * bn + 8, 104)])


def test_dma4_smallest(K, knobs):
    """Flag 16's smallest case on its own (run before the rest of the flag-16 tests)."""
    _gemm_table(K, knobs, 'dma4 smallest', 32, 64, BF16, BF16, 4 | DMA4, 'tiled-dma', table=[(1, 4, 8)])


@pytest.mark.parametrize('cdt,odt', TYPES[:5], ids=lambda d: _name(d))
@pytest.mark.parametrize('bm,bn', R.GEMM_TILES)
def test_gemm_table_dma4(K, knobs, bm, bn, cdt, odt):
    _gemm_table(K, knobs, f'gemm dma4 {bm}x{bn} {_name(cdt)}->{_name(odt)}', bm, bn, cdt, odt, 4 | DMA4, 'tiled-dma')


# ------------------------------------------------------------- epilogue and stride variants
VARIANTS = ['none', 'bias', 'scale_bias', 'relu', 'mask', 'res', 'res_ld4', 'res_ld3', 'out_ld4', 'out_ld1',
            'res_out_vec', 'lda8', 'x_add']


def _variant(K, tag, var, M, N, Kd, cdt, cls, family, bm, bn):
    g = torch.Generator().manual_seed(M * 31 + N + len(var))
    x, w, acc, ap = R.gemm_case(M, N, Kd, cdt, cls)
    kw, ep = {}, {}
    xa = x.to(cdt).cuda()
    if var in ('bias', 'scale_bias', 'relu', 'mask', 'res_out_vec'):
        scale, bias = R.exact_epilogue(N, g) if cls == 'exact' else R.generic_epilogue(N, g)
        ep['bias'] = bias
        kw['bias'] = bias.cuda()
        if var != 'bias':
            ep['scale'] = scale
            kw['scale'] = scale.cuda()
    if var == 'relu':
        ep['relu'] = kw['relu'] = True
    if var == 'mask':
        ep['row_mask'] = torch.rand(M, generator=g) < 0.3
        kw['row_mask'] = ep['row_mask'].cuda()
    pad_r = {'res': 0, 'res_ld4': 4, 'res_ld3': 3, 'res_out_vec': (-N) % 4 + 4}.get(var)
    if pad_r is not None:
        # a residual of `cdt` values (the output type), contiguous or a view of a wider buffer
        res = R.exact_res((M, N), g) if cls == 'exact' else torch.randn(M, N, generator=g).to(cdt).float()
        ep['res'] = res
        rbuf = torch.full((M, N + pad_r), SENTINEL, dtype=cdt).cuda()
        rbuf[:, :N] = res.to(cdt).cuda()
        kw['residual'] = rbuf[:, :N]
        assert kw['residual'].stride(0) == N + pad_r
    pad_c = {'out_ld4': 4, 'out_ld1': 1, 'res_out_vec': (-N) % 4 + 4}.get(var)
    cbuf = None
    if pad_c is not None:
        cbuf = torch.full((M, N + pad_c), SENTINEL, dtype=cdt).cuda()
        kw['out'] = cbuf[:, :N]
    if var == 'lda8':
        abuf = torch.full((M, Kd + 8), 3.0, dtype=cdt).cuda()
        abuf[:, :Kd] = xa
        xa = abuf[:, :Kd]
    odt = cdt
    if var == 'x_add':
        # the A operand is (x + x_add) rounded ONCE, to nearest even, to the compute type.  Exact
        # class: x_add in multiples of 2^-9 up to 7/512, so that 1/2 + x_add and 1 + x_add need
        # rounding in bf16 (ties included); the rounded sums are multiples of 2^-9, their products
        # with W multiples of 2^-12 below 2^9 -- still exact in f32 -- and the output is taken in
        # f32, where a truncated sum (off by 2^-7 or 2^-8) cannot hide
        if cls == 'exact':
            x2 = torch.randint(-7, 8, (M, Kd), generator=g).float() / 512
            odt = kw['out_dtype'] = F32
        else:
            x2 = torch.randn(M, Kd, generator=g).to(cdt).float()
        kw['x_add'] = x2.to(cdt).cuda()
        a = (x + x2).to(cdt).double()
        acc, ap = a @ w.double().T, a.abs() @ w.double().abs().T
    y = K.linear(xa, w.to(cdt).cuda(), **kw)
    _ran(K, family, bm, bn)
    _check(tag, f'{var} ({M}, {N}, {Kd}) {cls}', y, cls, acc, ap, Kd, odt, **ep)
    if cbuf is not None:
        assert (cbuf[:, N:] == SENTINEL).all(), f'{var}: the gap columns were written'


@pytest.mark.parametrize('cdt', [BF16, F32], ids=_name)
@pytest.mark.parametrize('bm,bn', R.GEMM_TILES)
def test_epilogue_variants(K, knobs, bm, bn, cdt):
    knobs.flags(4)
    knobs.tile(bm, bn)
    tag = f'variants {bm}x{bn} {_name(cdt)}'
    for M, N in ((bm + 1, bn + 4), (5, bn + 1)):
        for var in VARIANTS:
            for cls in ('exact', 'generic'):
                _variant(K, tag, var, M, N, 72, cdt, cls, 'tiled', bm, bn)


# ------------------------------------------------------------ head-major stores at small M
@pytest.mark.parametrize('cdt,odt', [(BF16, BF16), (BF16, F16), (F16, F16), (F32, F32)], ids=lambda d: _name(d))
@pytest.mark.parametrize('bm,bn', [(32, 64), (64, 128)])
def test_headmajor_small(K, knobs, bm, bn, cdt, odt):
    knobs.flags(4)
    knobs.tile(bm, bn)
    B, S = 2, 37
    tag = f'headmajor {bm}x{bn} {_name(cdt)}->{_name(odt)}'
    for d, hd in ((256, 32), (288, 36), (288, 48), (288, 'split')):
        g = torch.Generator().manual_seed(d + bm)
        x, w, acc, ap = R.gemm_case(B * S, d, d, cdt, 'exact')
        bias = R.exact_epilogue(d, g)[1]
        mask = torch.rand(B * S, generator=g) < 0.3
        xc, wc = x.to(cdt).cuda().view(B, S, d), w.to(cdt).cuda()
        if hd == 'split':
            ws, bs = K.split_value_weights(wc, bias.cuda(), 8)
            y = K.value_proj_headmajor_split(xc, ws, bs, 8, row_mask=mask.cuda().view(B, S), out_dtype=odt).merged()
            hd = 36
        else:
            y = K.value_proj_headmajor(xc, wc, bias.cuda(), hd, row_mask=mask.cuda().view(B, S), out_dtype=odt)
        _ran(K, 'tiled', bm, bn)
        assert y.shape == (d // hd, B, S, hd)
        rows = y.permute(1, 2, 0, 3).reshape(B * S, d)        # back to (row, column) order
        _check(tag, f'd={d} hd={hd}', rows, 'exact', acc, ap, d, odt, bias=bias, row_mask=mask)


# -------------------------------------------------------------------------- implicit conv
def _conv(K, tag, name, cdt, cls, full, family, bm, bn, ksplit=None):
    (KH, KW), stride, pad, B, H, W, Cin, Cout = R.CONV_CASES[name]
    x, w, acc, ap = R.conv_case(name, cdt, cls)
    Ho, Wo = R.out_size(H, W, KH, KW, stride, pad)
    st, pd = (stride[0], pad[0]) if stride[0] == stride[1] and pad[0] == pad[1] else (stride, pad)
    if ksplit is None and isinstance(st, int):
        ksplit = 1          # (C2's K = 1152 would split by itself)
    kw, ep, buf = {}, {}, None
    if full:
        g = torch.Generator().manual_seed(len(name) + Cout)
        scale, bias = R.exact_epilogue(Cout, g) if cls == 'exact' else R.generic_epilogue(Cout, g)
        res = R.exact_res((B * Ho * Wo, Cout), g) if cls == 'exact' else \
            torch.randn(B * Ho * Wo, Cout, generator=g).to(cdt).float()
        ep = dict(scale=scale, bias=bias, res=res, relu=True)
        buf = torch.full((B, Ho, Wo, Cout + 8), SENTINEL, dtype=cdt).cuda()
        kw = dict(scale=scale.cuda(), bias=bias.cuda(), relu=True, out=buf[..., 4:4 + Cout],
                  residual=res.to(cdt).cuda().view(B, Ho, Wo, Cout))
    y = K.conv2d_nhwc(x.to(cdt).cuda(), w.to(cdt).cuda(), st, pd, ksplit=ksplit, **kw)
    _ran(K, family, bm, bn)
    _check(tag, f'{name}{" full" if full else ""} {cls}', y, cls, acc, ap, KH * KW * Cin, cdt, **ep)
    if buf is not None:
        assert (buf[..., :4] == SENTINEL).all() and (buf[..., 4 + Cout:] == SENTINEL).all(), f'{name}: gap written'
    return y


@pytest.mark.parametrize('cdt', [BF16, F16, F32], ids=_name)
@pytest.mark.parametrize('bm,bn', [(32, 64), (64, 128), (128, 128)])
def test_conv_cases(K, knobs, bm, bn, cdt):
    knobs.flags(NO_SPECIAL)
    knobs.tile(bm, bn)
    tag = f'conv {bm}x{bn} {_name(cdt)}'
    for name in R.CONV_CASES:
        for cls in ('exact', 'generic') if name in ('C1', 'C3') else ('exact',):
            for full in (False, True):
                y = _conv(K, tag, name, cdt, cls, full, 'tiled', bm, bn)
                if name == 'C7b' and not full and cls == 'exact':
                    # pad 3 around a 3x3 filter: the outermost ring of windows is all padding
                    ring = torch.ones(y.shape[1:3], dtype=torch.bool)
                    ring[1:-1, 1:-1] = False
                    assert (y[0].cpu()[ring] == 0).all()


@pytest.mark.parametrize('cdt', [BF16, F16], ids=_name)
@pytest.mark.parametrize('bm,bn', [(32, 64), (64, 128), (128, 128)])
def test_conv_cases_dma4(K, knobs, bm, bn, cdt):
    knobs.flags(NO_SPECIAL | DMA4)
    knobs.tile(bm, bn)
    for name in ('C1', 'C2', 'C3'):
        for cls in ('exact', 'generic') if name in ('C1', 'C3') else ('exact',):
            for full in (False, True):
                _conv(K, f'conv dma4 {bm}x{bn} {_name(cdt)}', name, cdt, cls, full, 'tiled-dma', bm, bn)


# -------------------------------------------------------------------------------- split-K
@pytest.mark.parametrize('cdt', [BF16, F32], ids=_name)
def test_splitk_conv(K, knobs, cdt):
    knobs.flags(NO_SPECIAL)
    for name in ('C2', 'C3'):
        for ks in (2, 3):
            _conv(K, f'splitk conv {_name(cdt)}', f'{name}', cdt, 'exact', True, 'splitk', 64, 64, ksplit=ks)


@pytest.mark.parametrize('cdt', [BF16, F32], ids=_name)
def test_splitk_linear_natural(K, knobs, cdt):
    knobs.flags(4)
    for M, N, Kd in ((8, 1100, 1024), (5, 91, 2048)):      # the finalize's columns past 1024; odd N
        assert K.ksplit_for(M, N, Kd) > 1
        g = torch.Generator().manual_seed(N)
        x, w, acc, ap = R.gemm_case(M, N, Kd, cdt, 'exact')
        scale, bias = R.exact_epilogue(N, g)
        res = R.exact_res((M, N), g)
        mask = torch.rand(M, generator=g) < 0.3
        y = K.linear(x.to(cdt).cuda(), w.to(cdt).cuda(), bias=bias.cuda(), scale=scale.cuda(), relu=True,
                     residual=res.to(cdt).cuda(), row_mask=mask.cuda())
        _ran(K, 'splitk', 64, 64)
        _check(f'splitk linear {_name(cdt)}', f'({M}, {N}, {Kd})', y, 'exact', acc, ap, Kd, cdt, scale=scale, bias=bias,
               res=res, relu=True, row_mask=mask)


# ------------------------------------------------ the planner's answer against the launch itself
def test_plan_matches_launch(K, knobs):
    """kinet_gemm_plan of a call names the kernel that kinet_gemm_last_kernel reports after it (the
    plan's last launch), on the tile the heuristic is meant to pick for the shape."""
    knobs.flags(4)
    dev = 'cuda'

    def ones(M, N, Kd):
        y = K.linear(torch.ones(M, Kd, dtype=BF16, device=dev), torch.ones(N, Kd, dtype=BF16, device=dev))
        torch.cuda.synchronize()
        assert (y == Kd).all()

    for M, N, Kd, bm, bn in ((4096, 1024, 8, 32, 64), (4097, 1024, 8, 64, 128), (4096, 1028, 8, 64, 128),
                             (5000, 64, 8, 128, 64), (5000, 68, 8, 64, 128), (65536, 512, 8, 128, 128),
                             (65536, 508, 8, 64, 128)):
        ones(M, N, Kd)
        assert K.gemm_plan(M, N, Kd) == [(('tiled', bm, bn), 0, -(-M // bm))]
        _ran(K, 'tiled', bm, bn)
    # a fused-LayerNorm launch and a split-K one
    g = torch.Generator().manual_seed(1)
    y = K.linear(torch.randn(100, 64, generator=g).bfloat16().cuda(), torch.randn(256, 64, generator=g).bfloat16().cuda(),
                 ln=(torch.ones(256).cuda(), torch.zeros(256).cuda(), 1e-5))
    assert K.gemm_plan(100, 256, 64, ln=True) == [(('tiled', 32, 256), 0, 4)]
    _ran(K, 'tiled', 32, 256)
    ks = K.ksplit_for(8, 1100, 1024)
    assert ks > 1
    y = K.linear(torch.ones(8, 1024, dtype=BF16, device=dev), torch.ones(1100, 1024, dtype=BF16, device=dev))
    torch.cuda.synchronize()
    assert (y == 1024).all()
    assert K.gemm_plan(8, 1100, 1024, kchunk=1024 // ks) == [(('tiled', 64, 64), 0, 1)]    # the grid of the K slices
    _ran(K, 'splitk', 64, 64)
    # a multi-tap convolution planned as two launches: a round of 8-wave tiles, then the 64x128 tail
    # (2x2 taps of 16 channels: K = 64; 140 x 256 output pixels, N = 512: 140 m-tiles of 2 column tiles)
    knobs.flags(NO_SPECIAL)
    y = K.conv2d_nhwc(torch.ones(1, 141, 257, 16, dtype=BF16, device=dev), torch.ones(512, 2, 2, 16, dtype=BF16, device=dev), 1, 0)
    torch.cuda.synchronize()
    assert y.shape == (1, 140, 256, 512) and (y == 64).all()
    plan = K.gemm_plan(140 * 256, 512, 64, conv=True, Cin=16)
    assert plan == [(('dma8', 256, 256), 0, 128), (('tiled', 64, 128), 128 * 256, 48)]
    _ran(K, *plan[-1][0])
    # an 8-wave tile under flag 2
    knobs.flags(4 | 2)
    ones(4096, 128, 64)
    assert K.gemm_plan(4096, 128, 64) == [(('dma8', 256, 128), 0, 16)]
    _ran(K, 'dma8', 256, 128)


# -------------------------------------------------- refusals (no kernel starts) and alignment
def test_forced_tile_without_instantiation_is_refused(K, knobs):
    knobs.flags(4)
    x, w = torch.ones(300, 64, device='cuda'), torch.ones(128, 64, device='cuda')
    y = torch.full((300, 128), SENTINEL, device='cuda')
    for bm, bn in ((256, 128), (128, 256), (256, 256)):
        knobs.tile(bm, bn)
        with pytest.raises(RuntimeError, match='forced tile'):
            K.linear(x, w, out=y)                                       # f32 operands
        with pytest.raises(RuntimeError, match='forced tile'):
            K.linear(x.bfloat16(), w, x_add=x.bfloat16())                 # the load-time add
    knobs.tile(0, 0)
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision('high')
    try:
        knobs.tile(256, 128)
        with pytest.raises(RuntimeError, match='forced tile'):
            K.linear(x, w, out=y)                                       # KINET_F32_X3
    finally:
        torch.set_float32_matmul_precision(prev)
    torch.cuda.synchronize()
    assert (y == SENTINEL).all()
    with pytest.raises(RuntimeError, match='unsupported tile'):
        knobs.tile(48, 64)


@pytest.mark.parametrize('dt', [BF16, F32], ids=_name)
def test_misaligned_c_and_r_are_refused(K, knobs, dt):
    """Through the C ABI: a C or R that starts off a 4-element boundary while its row stride is a
    multiple of 4 (the epilogue's 4-element accesses) is an argument error; nothing is launched."""
    from kinet_amd import _native as nat
    M, N, Kd = 8, 16, 8
    x, w = torch.ones(M, Kd, dtype=dt, device='cuda'), torch.ones(N, Kd, dtype=dt, device='cuda')
    flat = torch.full((M * 20 + 8,), SENTINEL, dtype=dt, device='cuda')
    good = torch.full((M, N), SENTINEL, dtype=dt, device='cuda')
    code = nat.dtype_code(dt)

    def gemm(c, ldc, r, ldr):
        return nat.lib().kinet_gemm_ex(x.data_ptr(), None, w.data_ptr(), c, M, N, Kd, Kd, Kd, ldc, code, None, None, r, ldr,
                                       0, None, None, 0.0, code, None, nat.stream(x.device))
    es = flat.element_size()
    for off in (1, 2, 3):
        assert gemm(flat.data_ptr() + off * es, 20, None, 0) != 0                      # C, vector stores
        assert b'aligned' in nat.lib().kinet_last_error()
        assert gemm(good.data_ptr(), N, flat.data_ptr() + off * es, 20) != 0           # R, rows loaded ahead
        assert nat.lib().kinet_conv2d(x.data_ptr(), w.data_ptr(), flat.data_ptr() + off * es, 1, 2, 4, Kd, 2, 4, N, 1, 1,
                                      1, 0, code, None, None, None, 0, 0, 20, nat.stream(x.device)) != 0
    torch.cuda.synchronize()
    assert (flat == SENTINEL).all() and (good == SENTINEL).all()
    # the element-wise path (ldc % 4 != 0) takes any element-aligned pointer
    assert gemm(flat.data_ptr() + es, 19, None, 0) == 0
    torch.cuda.synchronize()
    assert (flat[1:1 + M * 19].view(M, 19)[:, :N] == Kd).all() and (flat[1:1 + M * 19].view(M, 19)[:, N:] == SENTINEL).all()


@pytest.mark.parametrize('cdt', [BF16, F32], ids=_name)
def test_misaligned_views_through_kernels(K, knobs, cdt):
    """kernels.linear / conv2d_nhwc copy a misaligned residual view (exact class: same bits as the
    aligned call) and raise on a misaligned out= view."""
    knobs.flags(NO_SPECIAL)
    M, N, Kd = 33, 68, 72
    g = torch.Generator().manual_seed(9)
    x, w, acc, ap = R.gemm_case(M, N, Kd, cdt, 'exact')
    res = R.exact_res((M, N), g)
    flat = torch.zeros(M * N + 8, dtype=cdt).cuda()
    for off in (1, 2):
        rv = flat[off:off + M * N].view(M, N)
        rv.copy_(res.to(cdt))
        assert rv.data_ptr() % (4 * rv.element_size())
        y = K.linear(x.to(cdt).cuda(), w.to(cdt).cuda(), residual=rv)
        _check(f'misaligned {_name(cdt)}', f'linear residual + {off}', y, 'exact', acc, ap, Kd, cdt, res=res)
        with pytest.raises(RuntimeError, match='aligned'):
            K.linear(x.to(cdt).cuda(), w.to(cdt).cuda(), out=flat[off:off + M * N].view(M, N))
    (KH, KW), stride, pad, B, H, W, Cin, Cout = R.CONV_CASES['C1']
    xc, wc, cacc, cap = R.conv_case('C1', cdt, 'exact')
    cres = R.exact_res(cacc.shape, g)
    flat = torch.zeros(cacc.numel() + 8, dtype=cdt).cuda()
    rv = flat[1:1 + cacc.numel()].view(B, H, W, Cout)
    rv.copy_(cres.to(cdt).view(B, H, W, Cout))
    y = K.conv2d_nhwc(xc.to(cdt).cuda(), wc.to(cdt).cuda(), 1, 1, residual=rv)
    _check(f'misaligned {_name(cdt)}', 'conv residual + 1', y, 'exact', cacc, cap, 9 * Cin, cdt, res=cres)
    with pytest.raises(RuntimeError, match='aligned'):
        K.conv2d_nhwc(xc.to(cdt).cuda(), wc.to(cdt).cuda(), 1, 1, out=flat[1:1 + cacc.numel()].view(B, H, W, Cout))
