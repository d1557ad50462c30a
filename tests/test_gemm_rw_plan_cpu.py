"""CPU-only tests of the resident-weight GEMM's launch planner (csrc/gemm_rw_plan.h through
kinet_gemm_rw_plan): every row of the literal case tables of direct_refs.py, described as
tests/test_gemm_rw_direct_gpu.py runs it, under every grid cap used there; every rule at its boundary
against plans worked out by hand from the rule's own thresholds; and the structural properties a plan
must have whatever the rules say.  256 compute units unless a test says otherwise."""
import itertools

import pytest
import torch

import direct_refs as R

F32, BF16, F16 = 0, 1, 2        # kinet_dtype codes (include/kinet_common.h)
DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}
RW = 8                          # the resident-weight kernel from M >= 256
F_K512_OFF, F_DS_OFF, F_K288_OFF = 256, 2048, 1048576
CAPS = (0, 1, 3, 16)


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


@pytest.fixture
def knobs(K):
    """flags / grid cap of this thread for one test, restored afterwards."""
    from kinet_amd import _native
    L = _native.lib()

    class Knobs:
        flags = staticmethod(L.kinet_gemm_set_flags)
        cap = staticmethod(K.gemm_rw_grid_cap)
    yield Knobs
    L.kinet_gemm_set_flags(0)
    K.gemm_rw_grid_cap(0)


def variant(plan):
    """(KC, NT, BMR, NS, NW, OCC) of a plan, None if not eligible."""
    return None if plan is None else tuple(plan[f] for f in R.RW_CONFIG_FIELDS[:6])


def grid(plan):
    return None if plan is None else (plan['P'], plan['ng'], plan['n_mtiles'])


# --------------------------------------------------------- the literal tables of the GPU test
def _id(c):
    return c[0].replace(' ', '_')


@pytest.mark.parametrize('case', R.RW_CASES, ids=_id)
def test_table_gemm(K, knobs, case):
    name, Kd, N, flags, _, cdt, odt, cfg, ng = case
    o = R.rw_opts(case)
    knobs.flags(RW | flags)
    for cap in CAPS:
        knobs.cap(cap)
        got = K.gemm_rw_plan(R.rw_rows(cfg[2]), N, Kd, DT[cdt], DT[odt], residual='R' in o, ln='LN' in o, a2='A2' in o,
                             ldc=N + (8 if 'ld' in o else 0), ldr=N + (8 if 'Rld' in o else 0), row_mask='mask' in o)
        assert got == R.rw_expected(cfg, ng, 'R' in o, 'LN' in o, 'A2' in o, odt, cap), f'{name} cap {cap}'


@pytest.mark.parametrize('case', R.RW_HM_CASES, ids=_id)
def test_table_headmajor(K, knobs, case):
    name, d, hd, flags, cdt, odt, cfg, ng = case
    B, S = R.rw_hm_batch(cfg[2])
    hm = dict(hm_rows=S, hm_d=32, hm_split=256, hm_d2=4) if hd == 'split' else dict(hm_rows=S, hm_d=hd)   # 8 heads x (32 | 4)
    knobs.flags(RW | flags)
    for cap in CAPS:
        knobs.cap(cap)
        got = K.gemm_rw_plan(B * S, d, d, DT[cdt], DT[odt], row_mask=1, **hm)
        assert got == R.rw_expected(cfg, ng, False, False, False, odt, cap), f'{name} cap {cap}'


@pytest.mark.parametrize('Kd,cfg,ng', [(256, (8, 4, 16, 4, 4, 2), 2), (288, (9, 3, 16, 4, 8, 1), 1)])
def test_table_a2_period(K, knobs, Kd, cfg, ng):
    """test_rw_a2_period: offsets_proj_headmajor of 3 x 89 rows, 8 heads x 48 columns, bf16 -> f16."""
    knobs.flags(RW)
    for cap in CAPS:
        knobs.cap(cap)
        got = K.gemm_rw_plan(3 * 89, 384, Kd, BF16, F16, a2=1, hm_rows=89, hm_d=48)
        assert got == R.rw_expected(cfg, ng, False, False, True, torch.float16, cap)


@pytest.mark.parametrize('cdt', [BF16, F16])
@pytest.mark.parametrize('case', R.RW_CONV_CASES, ids=_id)
def test_table_conv(K, knobs, case, cdt):
    name, (KH, Cin, Cout, stride, pad_h, Hin, Win), flags, opts, cfg, ng = case
    M, Wout = R.RW_CONV_ROWS, 33
    assert Wout == (Win - 1) // stride[1] + 1
    tiles = -(-M // cfg[2])
    odt = torch.bfloat16 if cdt == BF16 else torch.float16
    knobs.flags(RW | flags)
    for cap in CAPS + (tiles - 1,):
        knobs.cap(cap)
        got = K.gemm_rw_plan(M, Cout, KH * Cin, cdt, kind='conv', ldc=Cout + 8, Cin=Cin, KW=1, stride=stride[0],
                             stride_w=stride[1], pad=pad_h, pad_w=0, Win=Win, Wout=Wout)
        assert got == R.rw_expected(cfg, ng, False, False, False, odt, cap, cr=1, tiles=tiles), f'{name} cap {cap}'


@pytest.mark.parametrize('cdt', [BF16, F16])
@pytest.mark.parametrize('case', R.PREP_CASES, ids=_id)
def test_table_records(K, knobs, case, cdt):
    name, flags, add, cfg, ng = case
    knobs.flags(flags)              # (the records launcher has no smallest M)
    for cap in CAPS:
        knobs.cap(cap)
        got = K.gemm_rw_plan(3 * 89, 8 * 48, 256, cdt, kind='records', a2=add, row_mask=1)
        assert got == R.rw_expected(cfg, ng, False, False, add, torch.float16, cap, prep=1, tiles=17), f'{name} cap {cap}'


# --------------------------------------------------------------------- the rules, one by one
PLAIN32 = {64: (2, 4, 32, 4, 4, 2), 128: (4, 4, 32, 4, 4, 2), 256: (8, 4, 32, 4, 4, 2)}
K512_4W, K512_8W = (16, 2, 16, 4, 4, 2), (16, 2, 16, 4, 8, 1)
K288_4W, K288_8W = (9, 3, 16, 4, 4, 2), (9, 3, 16, 4, 8, 1)


def test_smallest_m(K, knobs):
    assert K.gemm_rw_plan(4095, 256, 256) is None
    assert variant(K.gemm_rw_plan(4096, 256, 256)) == PLAIN32[256]
    assert variant(K.gemm_rw_plan(4097, 256, 256)) == PLAIN32[256]
    knobs.flags(RW)
    assert K.gemm_rw_plan(255, 256, 256) is None
    assert variant(K.gemm_rw_plan(256, 256, 256)) == PLAIN32[256]
    assert variant(K.gemm_rw_plan(257, 256, 256)) == PLAIN32[256]
    # the convolutions follow the same threshold, the records have none
    ds = dict(kind='conv', Cin=256, KW=1, stride=2, stride_w=2, Win=65, Wout=33)
    assert K.gemm_rw_plan(255, 256, 256, **ds) is None and K.gemm_rw_plan(256, 256, 256, **ds) is not None
    knobs.flags(0)
    assert K.gemm_rw_plan(4095, 256, 256, **ds) is None and K.gemm_rw_plan(4096, 256, 256, **ds) is not None
    assert variant(K.gemm_rw_plan(1, 192, 256, kind='records')) == (8, 3, 16, 4, 4, 2)


def test_k_values(K, knobs):
    knobs.flags(RW)
    for Kd, want in PLAIN32.items():
        assert variant(K.gemm_rw_plan(4096, 128, Kd)) == want
    assert variant(K.gemm_rw_plan(4096, 128, 512)) == K512_4W
    assert variant(K.gemm_rw_plan(4096, 128, 288)) == K288_4W
    for Kd in (32, 56, 72, 96, 120, 136, 192, 248, 264, 280, 296, 320, 384, 504, 520, 576, 1024):
        assert K.gemm_rw_plan(4096, 128, Kd) is None, Kd


def test_column_groups_and_n(K, knobs):
    """ng = ceil(N / GW) with GW = 256 (K <= 256), 128 or 256 (K = 512), 192 or 384 (K = 288)."""
    knobs.flags(RW)
    M = 4096
    for Kd in (64, 128, 256):
        assert [K.gemm_rw_plan(M, n, Kd)['ng'] for n in (8, 256, 264, 512, 520)] == [1, 1, 2, 2, 3]
    # K = 512: N <= 128 one 4-wave group; 128 < N <= 256 one 8-wave group; N > 256 refused
    assert [(variant(p), p['ng']) for p in (K.gemm_rw_plan(M, n, 512) for n in (128, 136, 256))] == \
        [(K512_4W, 1), (K512_8W, 1), (K512_8W, 1)]
    assert K.gemm_rw_plan(M, 264, 512) is None
    # K = 288 plain: 4-wave 192-column groups up to N = 384, 8-wave 384-column groups past it
    assert [(variant(p), p['ng']) for p in (K.gemm_rw_plan(M, n, 288) for n in (192, 200, 288, 296, 384, 392, 768, 776))] == \
        [(K288_4W, 1), (K288_4W, 2), (K288_4W, 2), (K288_4W, 2), (K288_4W, 2), (K288_8W, 2), (K288_8W, 2), (K288_8W, 3)]
    # K = 288 + A2: the 8-wave group for 192 < N <= 384 only (4-wave: a 3-slot ring)
    a2_4w = (9, 3, 16, 3, 4, 2)
    assert [(variant(p), p['ng']) for p in (K.gemm_rw_plan(M, n, 288, a2=1) for n in (192, 200, 384, 392))] == \
        [(a2_4w, 1), (K288_8W, 1), (K288_8W, 1), (a2_4w, 3)]
    for Kd in (64, 128, 256, 288, 512):
        for n in (0, 4, 12, 100, 130, 252):
            assert K.gemm_rw_plan(M, n, Kd) is None, (Kd, n)


def test_residual_wide_rule(K, knobs):
    """+ residual: 4-wave groups up to N = 256, 8-wave 512-column groups past it (K <= 256 only)."""
    knobs.flags(RW)
    for Kd, kc in ((64, 2), (128, 4), (256, 8)):
        r4 = (kc, 4, 32, 3, 4, 2) if kc == 2 else (kc, 4, 16, 4, 4, 2)
        assert variant(K.gemm_rw_plan(4096, 256, Kd, residual=1)) == r4
        p = K.gemm_rw_plan(4096, 264, Kd, residual=1)
        assert (variant(p), p['ng']) == ((kc, 4, 16, 4, 8, 1), 1)
        assert K.gemm_rw_plan(4096, 520, Kd, residual=1)['ng'] == 2
    p = K.gemm_rw_plan(4096, 264, 288, residual=1)
    assert (variant(p), p['ng']) == ((9, 3, 16, 3, 4, 2), 2)
    knobs.flags(RW | R.RW_W4)
    p = K.gemm_rw_plan(4096, 264, 256, residual=1)
    assert (variant(p), p['ng']) == ((8, 4, 16, 4, 4, 2), 2)


def test_epilogue_combinations(K, knobs):
    knobs.flags(RW)
    # LayerNorm: one group spans the row
    assert K.gemm_rw_plan(4096, 256, 256, ln=1)['ng'] == 1 and K.gemm_rw_plan(4096, 264, 256, ln=1) is None
    assert variant(K.gemm_rw_plan(4096, 288, 288, ln=1)) == (9, 2, 16, 4, 9, 1) and K.gemm_rw_plan(4096, 296, 288, ln=1) is None
    # K = 64: 32-row tiles whatever the epilogue; K >= 128: 16-row tiles with a second operand or LayerNorm
    assert variant(K.gemm_rw_plan(4096, 256, 64, ln=1)) == (2, 4, 32, 4, 4, 2)
    assert variant(K.gemm_rw_plan(4096, 256, 64, residual=1, ln=1)) == (2, 4, 32, 3, 4, 2)
    assert variant(K.gemm_rw_plan(4096, 256, 64, a2=1)) == (2, 4, 32, 4, 4, 2)
    for Kd, kc in ((128, 4), (256, 8)):
        for epi in (dict(ln=1), dict(residual=1, ln=1), dict(a2=1), dict(residual=1)):
            assert variant(K.gemm_rw_plan(4096, 256, Kd, **epi)) == (kc, 4, 16, 4, 4, 2)
    # A2 goes with neither residual nor LayerNorm, and needs a 16-byte aligned pointer
    for Kd in (64, 256, 288):
        assert K.gemm_rw_plan(4096, 192, Kd, a2=1, residual=1) is None
        assert K.gemm_rw_plan(4096, 192, Kd, a2=1, ln=1) is None
        assert K.gemm_rw_plan(4096, 192, Kd, a2=1, a2_aligned=0) is None
        assert K.gemm_rw_plan(4096, 192, Kd, a2=0, a2_aligned=0) is not None


def test_k512_refusals(K, knobs):
    knobs.flags(RW)
    assert variant(K.gemm_rw_plan(4096, 256, 512)) == K512_8W
    for bad in (dict(residual=1), dict(ln=1), dict(a2=1)):
        assert K.gemm_rw_plan(4096, 256, 512, **bad) is None
    assert K.gemm_rw_plan(4096, 264, 512) is None
    knobs.flags(RW | F_K512_OFF)
    assert K.gemm_rw_plan(4096, 256, 512) is None
    assert K.gemm_rw_plan(4096, 256, 256) is not None


def test_output_types_strides_alignment(K, knobs):
    knobs.flags(RW)
    pairs = {(BF16, BF16), (BF16, F16), (BF16, F32), (F16, F16), (F16, F32)}
    for i, o in itertools.product((F32, BF16, F16, 4), (F32, BF16, F16)):
        p = K.gemm_rw_plan(4096, 256, 256, i, o)
        assert (p is not None) == ((i, o) in pairs), (i, o)
        if p:
            assert p['out_bytes'] == (4 if o == F32 else 2)
    # 16-bit outputs: ldc % 8; f32 outputs: ldc % 4; C 16-byte aligned
    assert K.gemm_rw_plan(4096, 256, 256, BF16, BF16, ldc=264) is not None
    assert K.gemm_rw_plan(4096, 256, 256, BF16, BF16, ldc=260) is None
    assert K.gemm_rw_plan(4096, 256, 256, BF16, F32, ldc=260) is not None
    assert K.gemm_rw_plan(4096, 256, 256, BF16, F32, ldc=258) is None
    assert K.gemm_rw_plan(4096, 256, 256, c_aligned=0) is None
    # a residual: 16-bit output only, ldr % 8, R 16-byte aligned
    assert K.gemm_rw_plan(4096, 256, 256, BF16, F16, residual=1, ldr=264) is not None
    assert K.gemm_rw_plan(4096, 256, 256, BF16, F32, residual=1) is None
    assert K.gemm_rw_plan(4096, 256, 256, residual=1, ldr=260) is None
    assert K.gemm_rw_plan(4096, 256, 256, residual=1, r_aligned=0) is None
    assert K.gemm_rw_plan(4096, 256, 256, residual=0, r_aligned=0, ldr=3) is not None


def test_headmajor_rules(K, knobs):
    knobs.flags(RW)
    M = 4096
    # K != 288: 16-byte units (hm_d % 8), no split planes
    assert K.gemm_rw_plan(M, 256, 256, hm_rows=64, hm_d=32) is not None
    assert K.gemm_rw_plan(M, 256, 256, hm_rows=64, hm_d=8) is not None
    assert K.gemm_rw_plan(M, 256, 256, hm_rows=64, hm_d=4) is None
    assert K.gemm_rw_plan(M, 256, 256, hm_rows=64, hm_d=32, hm_split=128, hm_d2=4) is None
    # K = 288: 4-column units; split planes with a 4-column tail after whole heads
    assert K.gemm_rw_plan(M, 288, 288, hm_rows=64, hm_d=36) is not None
    assert K.gemm_rw_plan(M, 288, 288, hm_rows=64, hm_d=4) is not None
    assert K.gemm_rw_plan(M, 288, 288, hm_rows=64, hm_d=6) is None
    assert K.gemm_rw_plan(M, 288, 288, hm_rows=64, hm_d=32, hm_split=256, hm_d2=4) is not None
    assert K.gemm_rw_plan(M, 288, 288, hm_rows=64, hm_d=32, hm_split=256, hm_d2=8) is None
    assert K.gemm_rw_plan(M, 288, 288, hm_rows=64, hm_d=32, hm_split=248, hm_d2=4) is None
    # without a head-major store the fields are not looked at
    assert K.gemm_rw_plan(M, 256, 256, hm_rows=0, hm_d=3, hm_split=5) is not None


def test_output_extent_2gib(K, knobs):
    """((M - 1) * ldc + N) * element size, or M * N * element size head-major, must stay below 2^31."""
    M = 1 << 22
    assert K.gemm_rw_plan(M, 256, 256, BF16, BF16) is None                         # 2^22 * 256 * 2 = 2^31
    assert K.gemm_rw_plan(M - 1, 256, 256, BF16, BF16) is not None
    assert K.gemm_rw_plan(M, 256, 256, BF16, BF16, ldc=264) is None
    assert K.gemm_rw_plan((1 << 21) - 1, 256, 256, BF16, F32) is not None
    assert K.gemm_rw_plan(1 << 21, 256, 256, BF16, F32) is None
    # head-major: whole planes, M * N elements
    assert K.gemm_rw_plan(M, 256, 256, BF16, F16, hm_rows=1 << 10, hm_d=32) is None
    assert K.gemm_rw_plan(M - 8, 256, 256, BF16, F16, hm_rows=8, hm_d=32) is not None
    # rows of ldc elements: the last row's gap does not count
    m = (1 << 31) // (264 * 2)                                                       # 4067203.9...
    assert ((m - 1) * 264 + 256) * 2 < 1 << 31 <= (m * 264 + 256) * 2
    assert K.gemm_rw_plan(m, 256, 256, ldc=264) is not None and K.gemm_rw_plan(m + 1, 256, 256, ldc=264) is None
    # the convolutions: 2-byte outputs
    ds = dict(kind='conv', Cin=256, KW=1, stride=2, stride_w=2, Win=65, Wout=33)
    assert K.gemm_rw_plan(M, 256, 256, **ds) is None and K.gemm_rw_plan(M - 1, 256, 256, **ds) is not None


DS = dict(K=256, Cin=256, KW=1, stride=2, stride_w=2, pad=0, pad_w=0, Win=65, Wout=33, N=512)
TAPS = dict(K=168, Cin=24, KW=1, stride=2, stride_w=1, pad=3, pad_w=0, Win=33, Wout=33, N=64)


def _conv(kernels, geo, in_dtype=BF16, **change):
    g = dict(geo, **change)
    return kernels.gemm_rw_plan(g.pop('M', 4096), g.pop('N'), g.pop('K'), in_dtype, g.pop('out_dtype', None), kind='conv', **g)


def test_conv_strided_1x1(K, knobs):
    """K = Cin = 256, 1 x 1, unpadded, equal strides > 1, Wout >= 32, N % 256 == 0, nothing but scale / bias."""
    assert variant(_conv(K, DS)) == (8, 4, 32, 4, 4, 2) and _conv(K, DS)['CR'] == 1 and _conv(K, DS)['ng'] == 2
    assert variant(_conv(K, DS, F16)) == (8, 4, 32, 4, 4, 2)
    for bad in (dict(K=128, Cin=128), dict(K=512, Cin=512), dict(KW=3), dict(pad=1), dict(pad_w=1), dict(stride=3),
                dict(stride_w=1), dict(M=4095), dict(Wout=31), dict(N=384), dict(N=520), dict(residual=1), dict(ln=1),
                dict(row_mask=1), dict(ldc=516), dict(c_aligned=0)):
        assert _conv(K, DS, **bad) is None, bad
    assert _conv(K, DS, F32) is None and _conv(K, DS, BF16, out_dtype=F16) is None and _conv(K, DS, BF16, out_dtype=F32) is None
    assert _conv(K, DS, Wout=32) is not None and _conv(K, DS, N=256)['ng'] == 1
    knobs.flags(F_DS_OFF)
    assert _conv(K, DS) is None
    knobs.flags(R.RW_F16ROW)
    assert variant(_conv(K, DS)) == (8, 4, 16, 4, 4, 2)


def test_conv_tap_rows(K, knobs):
    """KH x 1 taps, K = KH * Cin <= 256, horizontally stride-1 unpadded (Win == Wout >= 32), Cin % 8 == 0,
    N <= 128, nothing but scale / bias; the vertical stride and padding are free."""
    assert variant(_conv(K, TAPS)) == (8, 2, 32, 4, 4, 2) and _conv(K, TAPS)['CR'] == 1
    assert variant(_conv(K, TAPS, N=128, K=256, Cin=64, stride=1, pad=0)) == (8, 2, 32, 4, 4, 2)
    for bad in (dict(M=4095), dict(K=264), dict(KW=3), dict(stride_w=2), dict(pad_w=1), dict(Win=34), dict(Cin=20),
                dict(Win=31, Wout=31), dict(N=136), dict(N=60), dict(residual=1), dict(ln=1), dict(ldc=68), dict(c_aligned=0),
                dict(row_mask=1)):
        assert _conv(K, TAPS, **bad) is None, bad
    assert _conv(K, TAPS, F32) is None and _conv(K, TAPS, F16, out_dtype=F32) is None
    knobs.flags(F_DS_OFF)                    # (the strided 1 x 1's flag is not this form's)
    assert _conv(K, TAPS) is not None
    knobs.flags(R.RW_F16ROW)
    assert variant(_conv(K, TAPS)) == (8, 2, 16, 4, 4, 2)


def test_flag_16_row_tiles(K, knobs):
    """Flag 131072: 16-row tiles where the default is 32 rows and K >= 128."""
    knobs.flags(RW | R.RW_F16ROW)
    assert variant(K.gemm_rw_plan(4096, 256, 64)) == PLAIN32[64]
    assert variant(K.gemm_rw_plan(4096, 256, 128)) == (4, 4, 16, 4, 4, 2)
    assert variant(K.gemm_rw_plan(4096, 256, 256)) == (8, 4, 16, 4, 4, 2)
    assert variant(K.gemm_rw_plan(4096, 256, 64, residual=1)) == (2, 4, 32, 3, 4, 2)
    assert variant(K.gemm_rw_plan(4096, 128, 512)) == K512_4W and variant(K.gemm_rw_plan(4096, 128, 288)) == K288_4W


def test_flag_4_wave_groups(K, knobs):
    """Flag 268435456: every 8-wave rule off."""
    knobs.flags(RW | R.RW_W4)
    assert variant(K.gemm_rw_plan(4096, 256, 512)) == K512_4W and K.gemm_rw_plan(4096, 256, 512)['ng'] == 2
    assert variant(K.gemm_rw_plan(4096, 1728, 288)) == K288_4W and K.gemm_rw_plan(4096, 1728, 288)['ng'] == 9
    assert variant(K.gemm_rw_plan(4096, 384, 288, a2=1)) == (9, 3, 16, 3, 4, 2)
    assert variant(K.gemm_rw_plan(4096, 512, 128, residual=1)) == (4, 4, 16, 4, 4, 2)
    assert variant(K.gemm_rw_plan(4096, 384, 256, kind='records', a2=1)) == (8, 3, 16, 2, 4, 3)
    assert variant(K.gemm_rw_plan(4096, 384, 256, kind='records')) == (8, 3, 16, 4, 4, 2)
    assert variant(K.gemm_rw_plan(4096, 288, 288, ln=1)) == (9, 2, 16, 4, 9, 1)      # (not a LayerNorm flag)
    knobs.flags(RW)
    assert variant(K.gemm_rw_plan(4096, 384, 256, kind='records', a2=1)) == (8, 3, 16, 4, 8, 1)
    assert variant(K.gemm_rw_plan(4096, 384, 256, kind='records')) == (8, 3, 16, 4, 4, 2)


def test_flag_6_wave_layernorm_and_k288_off(K, knobs):
    knobs.flags(RW | R.RW_LN6)
    assert variant(K.gemm_rw_plan(4096, 288, 288, ln=1)) == (9, 3, 16, 4, 6, 1)
    assert variant(K.gemm_rw_plan(4096, 280, 288, ln=1, residual=1)) == (9, 3, 16, 4, 6, 1)
    assert variant(K.gemm_rw_plan(4096, 288, 288)) == K288_4W and variant(K.gemm_rw_plan(4096, 256, 256, ln=1)) == (8, 4, 16, 4, 4, 2)
    knobs.flags(RW | F_K288_OFF)
    assert K.gemm_rw_plan(4096, 288, 288) is None and K.gemm_rw_plan(4096, 256, 256) is not None


def test_records_arguments(K, knobs):
    for bad in (dict(K=288), dict(Nout=100), dict(out_dtype=BF16), dict(M=0)):
        a = dict(dict(M=4096, Nout=384, K=256, kind='records'), **bad)
        with pytest.raises(RuntimeError, match='gemm_rw_plan: records'):
            K.gemm_rw_plan(**a)
    assert K.gemm_rw_plan(4096, 384, 256, F32, kind='records') is None


def test_min_a2_rows(K):
    """The smallest per-frame A2 the entry points accept is the tallest A2 row tile of the table (32:
    K = 64); the frame-shared form of the Python layer starts there."""
    from kinet_amd import _native
    assert _native.lib().kinet_gemm_rw_min_a2_rows() == 32
    assert [K.gemm_rw_plan(4096, 192, kd, a2=1)['BMR'] for kd in (64, 128, 256, 288)] == [32, 16, 16, 16]
    x = torch.zeros(2, 31, 64, dtype=torch.bfloat16)
    assert K._load_add_operand(x.view(62, 64), torch.zeros(1, 31, 64, dtype=torch.bfloat16), 2, 31, 64)[2] == 0
    x = torch.zeros(2, 32, 64, dtype=torch.bfloat16)
    assert K._load_add_operand(x.view(64, 64), torch.zeros(1, 32, 64, dtype=torch.bfloat16), 2, 32, 64)[2] == 32


# -------------------------------------------------------------------------------- the grid
def test_grid_by_hand(K, knobs):
    """P = the largest multiple of 8 within cus * OCC / ng workgroups (the quotient itself below 8),
    at most one per row tile."""
    knobs.flags(RW)
    big = 1 << 19
    assert grid(K.gemm_rw_plan(big, 256, 256)) == (512, 1, big // 32)                # 2 per CU, one group
    assert grid(K.gemm_rw_plan(big, 1024, 256)) == (128, 4, big // 32)
    assert grid(K.gemm_rw_plan(big, 768, 256)) == (168, 3, big // 32)                # 512 / 3 = 170 -> 168
    assert grid(K.gemm_rw_plan(big, 512, 256, residual=1)) == (256, 1, big // 16)    # 8 waves: 1 per CU
    assert grid(K.gemm_rw_plan(big, 1728, 288)) == (48, 5, big // 16)                # 256 / 5 = 51 -> 48
    assert grid(K.gemm_rw_plan(big, 384, 256, kind='records', a2=1)) == (256, 1, big // 16)
    knobs.flags(RW | R.RW_W4)
    assert grid(K.gemm_rw_plan(big, 384, 256, kind='records', a2=1)) == (384, 2, big // 16)   # 3 per CU: 768 / 2
    knobs.flags(RW)
    assert grid(K.gemm_rw_plan(4097, 256, 256)) == (129, 1, 129)                     # clipped to the row tiles
    assert grid(K.gemm_rw_plan(4096, 256 * 100, 256)) == (5, 100, 128)               # 512 / 100 = 5 (< 8: as it is)
    # other CU counts
    assert grid(K.gemm_rw_plan(big, 256, 256, cus=304)) == (608, 1, big // 32)
    assert grid(K.gemm_rw_plan(big, 768, 256, cus=64)) == (40, 3, big // 32)          # 128 / 3 = 42 -> 40
    assert grid(K.gemm_rw_plan(big, 512, 256, residual=1, cus=3)) == (3, 1, big // 16)
    # the cap bounds P from above only, and never below 1
    knobs.cap(100)
    assert grid(K.gemm_rw_plan(big, 256, 256))[0] == 100 and grid(K.gemm_rw_plan(256, 256, 256))[0] == 8
    assert grid(K.gemm_rw_plan(4096, 256 * 100, 256, cus=32))[0] == 1                # 64 / 100 = 0 slots -> 1 under a cap


def test_structure_over_a_grid(K, knobs):
    """For every eligible plan: 1 <= P <= n_mtiles; uncapped P * ng <= cus * OCC; P a multiple of 8 whenever
    cus * OCC / ng >= 8 and the row tiles do not clip it; only the five type pairs; LayerNorm plans have one
    column group; n_mtiles and ng cover M and N exactly once."""
    pairs = {(BF16, BF16), (BF16, F16), (BF16, F32), (F16, F16), (F16, F32)}
    n = 0
    for flags in (RW, RW | R.RW_W4, RW | R.RW_F16ROW, RW | R.RW_LN6, 0):
        knobs.flags(flags)
        for cap, cus in ((0, 256), (0, 304), (0, 20), (3, 256)):
            knobs.cap(cap)
            for M, N, Kd, epi, (i, o) in itertools.product(
                    (256, 539, 4097, 44446, 700000), (8, 136, 192, 256, 288, 392, 520, 1728, 4104), (64, 128, 256, 288, 512),
                    (dict(), dict(residual=1), dict(ln=1), dict(residual=1, ln=1), dict(a2=1)),
                    ((BF16, BF16), (BF16, F32), (F16, F16), (F16, BF16), (F32, F32))):
                p = K.gemm_rw_plan(M, N, Kd, i, o, cus=cus, **epi)
                if p is None:
                    continue
                n += 1
                ctx = (flags, cap, cus, M, N, Kd, epi, i, o, p)
                gw = p['NW'] * p['NT'] * 16
                slots = cus * p['OCC']
                assert (i, o) in pairs, ctx
                assert p['KC'] * 32 == Kd and p['out_bytes'] == (4 if o == F32 else 2), ctx
                assert (p['HAS_R'], p['LN'], p['HAS_A2'], p['CR'], p['PREP']) == \
                    (int('residual' in epi), int('ln' in epi), int('a2' in epi), 0, 0), ctx
                assert p['n_mtiles'] == -(-M // p['BMR']) and p['ng'] == -(-N // gw), ctx
                assert 2 <= p['NS'] <= 4, ctx
                assert 1 <= p['P'] <= p['n_mtiles'], ctx
                if 'ln' in epi:
                    assert p['ng'] == 1, ctx
                if 'a2' in epi:
                    assert p['BMR'] <= 32, ctx
                if cap == 0:
                    assert p['P'] * p['ng'] <= slots, ctx
                    if slots // p['ng'] >= 8 and p['P'] < p['n_mtiles']:
                        assert p['P'] % 8 == 0, ctx
                else:
                    assert p['P'] <= cap, ctx
    assert n > 5000
