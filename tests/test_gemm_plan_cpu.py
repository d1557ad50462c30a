"""CPU-only tests of the GEMM launch planner (csrc/gemm_plan.h through kinet_gemm_plan and
kinet_gemm_ksplit): every tile rule at its boundary against plans worked out by hand from the rule's
own thresholds, the structural property a plan must have whatever the rules say, and ksplit_for
against values recorded from the Python rule it replaced.  256 compute units throughout."""
import itertools

import pytest

BF16, F32, X3 = 1, 0, 4        # kinet_dtype codes (include/kinet_common.h)
F_DMA8, F_DMA4, F_NOSPLIT, F_KEEPSPLIT, F_X3_DEFAULT = 2, 16, 64, 8388608, 33554432


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


@pytest.fixture
def knobs():
    """flags / forced tile / solo policy of this thread for one test, restored afterwards."""
    from kinet_amd import _native
    L = _native.lib()

    class Knobs:
        flags = staticmethod(L.kinet_gemm_set_flags)
        solo = staticmethod(L.kinet_set_solo_launch)

        @staticmethod
        def tile(bm, bn):
            _native.call('kinet_gemm_force_tile', bm, bn)
    yield Knobs
    L.kinet_gemm_force_tile(0, 0)
    L.kinet_gemm_set_flags(0)
    L.kinet_set_solo_launch(0)


def one(fam, bm, bn, M):
    """The plan of one launch of bm x bn tiles over all M rows."""
    return [((fam, bm, bn), 0, -(-M // bm))]


# ------------------------------------------------------------------ the base 4-wave choice
@pytest.mark.parametrize('M,N,bm,bn', [
    (4096, 1024, 32, 64), (4097, 1024, 64, 128), (4096, 1028, 64, 128),     # decoder-sized: M <= 4096 and N <= 1024
    (5000, 64, 128, 64), (5000, 68, 64, 128),                                # N <= 64
    (65536, 512, 128, 128), (65536, 508, 64, 128), (65408, 512, 64, 128),    # N >= 512 and 2048 128x128 tiles
])
def test_base_tile(K, knobs, M, N, bm, bn):
    assert K.gemm_plan(M, N, 8) == one('tiled', bm, bn, M)


def test_conv_128_tile_rule(K, knobs):
    """3x3 convs with K >= 1152, N >= 128 and 1000 128x128 tiles (f32: no 8-wave tiles to pre-empt it)."""
    conv = dict(dtype_code=F32, conv=True, Cin=128)
    assert K.gemm_plan(999 * 128, 128, 1152, **conv) == one('tiled', 64, 128, 999 * 128)
    assert K.gemm_plan(999 * 128 + 1, 128, 1152, **conv) == one('tiled', 128, 128, 999 * 128 + 1)
    assert K.gemm_plan(999 * 128 + 1, 128, 1144, **conv) == one('tiled', 64, 128, 999 * 128 + 1)
    assert K.gemm_plan(2 * 999 * 128 + 1, 64, 1152, **conv) == one('tiled', 128, 64, 2 * 999 * 128 + 1)
    assert K.gemm_plan(999 * 128 + 1, 128, 1152, dtype_code=F32) == one('tiled', 64, 128, 999 * 128 + 1)   # a GEMM


def test_x3_128x64_rule(K, knobs):
    assert K.gemm_plan(5000, 288, 64, dtype_code=X3) == one('tiled', 128, 64, 5000)     # 288 % 128 = 32
    assert K.gemm_plan(5000, 192, 64, dtype_code=X3) == one('tiled', 128, 64, 5000)     # % 128 = 64
    assert K.gemm_plan(5000, 193, 64, dtype_code=X3) == one('tiled', 64, 128, 5000)
    assert K.gemm_plan(5000, 256, 64, dtype_code=X3) == one('tiled', 64, 128, 5000)
    assert K.gemm_plan(5000, 288, 64, dtype_code=F32) == one('tiled', 64, 128, 5000)
    assert K.gemm_plan(4096, 288, 64, dtype_code=X3) == one('tiled', 32, 64, 4096)      # decoder-sized first
    knobs.flags(F_X3_DEFAULT)
    assert K.gemm_plan(5000, 288, 64, dtype_code=X3) == one('tiled', 64, 128, 5000)


def test_layernorm_tiles(K, knobs):
    ln = dict(ln=True)
    assert K.gemm_plan(8192, 256, 64, **ln) == one('tiled', 32, 256, 8192)
    assert K.gemm_plan(8193, 256, 64, **ln) == one('tiled', 64, 256, 8193)
    assert K.gemm_plan(100, 200, 64, **ln) == one('tiled', 32, 256, 100)
    # rows of 257..320: 128 x 320 LDS-DMA tiles from M = 8192 for 16-bit operands without A2
    assert K.gemm_plan(8191, 288, 64, **ln) == one('tiled', 32, 320, 8191)
    assert K.gemm_plan(8192, 288, 64, **ln) == one('tiled-dma', 128, 320, 8192)
    assert K.gemm_plan(8193, 257, 64, **ln) == one('tiled-dma', 128, 320, 8193)
    assert K.gemm_plan(8192, 288, 64, dtype_code=F32, **ln) == one('tiled', 32, 320, 8192)
    assert K.gemm_plan(8193, 288, 64, dtype_code=F32, **ln) == one('tiled', 64, 320, 8193)
    assert K.gemm_plan(8192, 288, 64, a2=True, **ln) == one('tiled', 32, 320, 8192)
    assert K.gemm_plan(8193, 288, 64, a2=True, **ln) == one('tiled', 64, 320, 8193)
    assert K.gemm_plan(8193, 320, 64, dtype_code=X3, **ln) == one('tiled', 64, 320, 8193)
    with pytest.raises(RuntimeError, match='N <= 320'):
        K.gemm_plan(100, 321, 64, **ln)
    # the forced tile is ignored by the fused-LayerNorm launches; flag 16 stages them by LDS-DMA
    knobs.tile(64, 64)
    assert K.gemm_plan(100, 256, 64, **ln) == one('tiled', 32, 256, 100)
    knobs.flags(F_DMA4)
    assert K.gemm_plan(100, 288, 64, **ln) == one('tiled-dma', 32, 320, 100)
    assert K.gemm_plan(100, 288, 64, a2=True, **ln) == one('tiled', 32, 320, 100)


def test_splitk_slices(K, knobs):
    assert K.gemm_plan(4096, 1100, 1024, kchunk=512) == one('tiled', 64, 64, 4096)
    assert K.gemm_plan(8, 1100, 1024, kchunk=256, dtype_code=F32) == one('tiled', 64, 64, 8)
    assert K.gemm_plan(4097, 1100, 1024, kchunk=512) == one('tiled', 64, 128, 4097)
    assert K.gemm_plan(4096, 1100, 1024) == one('tiled', 64, 128, 4096)


def test_empty_problem(K, knobs):
    assert K.gemm_plan(0, 256, 64) == [] and K.gemm_plan(100, 0, 64) == []


# ------------------------------------------------------------------------ the 8-wave tiles
def test_dma8_rule(K, knobs):
    assert K.gemm_plan(4096, 4096, 4096) == one('dma8', 256, 256, 4096)
    assert K.gemm_plan(4096, 128, 4096) == one('tiled', 32, 64, 4096)                  # 16 of 256 slots: eff 1/16
    # one column of 256-wide tiles: eff = m-tiles / 256 -- 231 / 256 = 0.902, 230 / 256 = 0.898
    assert K.gemm_plan(231 * 256, 256, 1024) == one('dma8', 256, 256, 231 * 256)
    assert K.gemm_plan(230 * 256, 256, 1024) == one('tiled', 64, 128, 230 * 256)
    assert K.gemm_plan(231 * 256, 256, 1016) == one('tiled', 64, 128, 231 * 256)       # K < 1024
    assert K.gemm_plan(256 * 256, 128, 1024) == one('dma8', 256, 128, 256 * 256)
    assert K.gemm_plan(4095, 4096, 4096) == one('tiled', 64, 128, 4095)                # M < 4096
    # never for f32 / KINET_F32_X3 operands, a load-time A2 or head-major stores
    for kw in (dict(dtype_code=F32), dict(dtype_code=X3), dict(a2=True), dict(hm_rows=128), dict(kchunk=1024)):
        assert K.gemm_plan(4096 + 1, 4096, 4096, **kw) == one('tiled', 64, 128, 4096 + 1), kw
    assert K.gemm_plan(100000, 256, 1024, ln=True) == one('tiled', 64, 256, 100000)    # not by itself with LayerNorm


def test_dma8_flag_2(K, knobs):
    knobs.flags(F_DMA8)
    assert K.gemm_plan(4096, 128, 64) == one('dma8', 256, 128, 4096)
    assert K.gemm_plan(4096, 129, 64) == one('dma8', 256, 256, 4096)
    assert K.gemm_plan(5000, 256, 64, ln=True) == one('dma8', 256, 256, 5000)
    assert K.gemm_plan(5000, 128, 64, ln=True) == one('dma8', 256, 256, 5000)         # LayerNorm: 256-wide rows
    assert K.gemm_plan(8192, 288, 64, ln=True) == one('tiled-dma', 128, 320, 8192)    # no 8-wave LayerNorm past 256
    assert K.gemm_plan(4095, 128, 64) == one('tiled', 32, 64, 4095)
    assert K.gemm_plan(4096, 127, 64) == one('tiled', 32, 64, 4096)
    for kw in (dict(dtype_code=F32), dict(dtype_code=X3), dict(a2=True), dict(hm_rows=128)):
        assert K.gemm_plan(4096, 128, 64, **kw) == one('tiled', 32, 64, 4096), kw
    knobs.flags(0)
    assert K.gemm_plan(4096, 128, 64) == one('tiled', 32, 64, 4096)


# ------------------------------------------- multi-tap convolutions: whole rounds + remainder
CONV3 = dict(conv=True, Cin=256)      # 3x3, 256 channels: K = 2304


def test_conv_round_split(K, knobs):
    # layer-3 3x3 at batch 24: 394 m-tiles = one round + 138, more than a quarter round -> one launch
    assert K.gemm_plan(394 * 256, 256, 2304, **CONV3) == one('dma8', 256, 256, 394 * 256)
    # a remainder of under a quarter round (60 tiles, the last one ragged): 4-wave tail from row 65536
    M = 316 * 256 - 100
    assert K.gemm_plan(M, 256, 2304, **CONV3) == [(('dma8', 256, 256), 0, 256), (('tiled', 64, 128), 65536, 239)]
    # exactly a quarter round still splits, one tile more does not
    assert K.gemm_plan(320 * 256, 256, 2304, **CONV3) == [(('dma8', 256, 256), 0, 256), (('tiled', 64, 128), 65536, 256)]
    assert K.gemm_plan(321 * 256, 256, 2304, **CONV3) == one('dma8', 256, 256, 321 * 256)
    # N = 512: two column tiles per m-tile, a round is 128 m-tiles
    assert K.gemm_plan(140 * 256, 512, 2304, **CONV3) == [(('dma8', 256, 256), 0, 128), (('tiled', 64, 128), 32768, 48)]
    # whole rounds exactly: no second launch (3x3 of 64 channels, f16: K = 576 is too short for the 8-wave rule,
    # which would take a long-K problem of full rounds before the split is considered)
    assert K.gemm_plan(512 * 256, 256, 576, conv=True, Cin=64, dtype_code=2) == one('dma8', 256, 256, 512 * 256)
    assert K.gemm_plan(512 * 256, 256, 576, dtype_code=2) == one('tiled', 64, 128, 512 * 256)     # the same as a GEMM
    # not for: a single tap, N < 256, M < 8192, f32 operands, flag 64
    assert K.gemm_plan(316 * 256, 256, 2304, conv=True, Cin=2304) == one('tiled', 128, 128, 316 * 256)
    assert K.gemm_plan(316 * 256, 255, 2304, **CONV3) == one('tiled', 128, 128, 316 * 256)
    assert K.gemm_plan(8191, 256, 2304, **CONV3) == one('tiled', 64, 128, 8191)
    assert K.gemm_plan(316 * 256, 256, 2304, dtype_code=F32, **CONV3) == one('tiled', 128, 128, 316 * 256)
    knobs.flags(F_NOSPLIT)
    assert K.gemm_plan(316 * 256, 256, 2304, **CONV3) == one('tiled', 128, 128, 316 * 256)
    # flag 8388608 keeps the split of the 394-tile case
    knobs.flags(F_KEEPSPLIT)
    assert K.gemm_plan(394 * 256, 256, 2304, **CONV3) == [(('dma8', 256, 256), 0, 256), (('tiled', 64, 128), 65536, 552)]
    # flag 16 stages the 4-wave tail by LDS-DMA; the 8-wave launch is the same kernel
    knobs.flags(F_DMA4)
    assert K.gemm_plan(316 * 256, 256, 2304, **CONV3) == [(('dma8', 256, 256), 0, 256), (('tiled-dma', 64, 128), 65536, 240)]
    # a forced tile takes the whole problem
    knobs.flags(0)
    knobs.tile(64, 128)
    assert K.gemm_plan(316 * 256, 256, 2304, **CONV3) == one('tiled', 64, 128, 316 * 256)


def test_conv_half_round_and_solo(K, knobs):
    """Less than one round of 8-wave tiles: from half a round on a single partial round of them, unless one
    batch is in flight and 128 x 256 tiles (at most one round of those) fill the chip better."""
    M = 32640                                   # config 5's stage-3 3x3: 128 m-tiles of 256, 255 of 128
    assert K.gemm_plan(M, 256, 2304, **CONV3) == one('dma8', 256, 256, M)
    assert K.gemm_plan(127 * 256, 256, 2304, **CONV3) == one('tiled', 64, 128, 127 * 256)    # under half a round
    knobs.solo(1)
    assert K.gemm_plan(M, 256, 2304, **CONV3) == one('dma8', 128, 256, M)
    assert K.gemm_plan(32768, 256, 2304, **CONV3) == one('dma8', 128, 256, 32768)             # 256 tiles of 128 rows
    assert K.gemm_plan(32769, 256, 2304, **CONV3) == one('dma8', 256, 256, 32769)             # 257: more than a round
    assert K.gemm_plan(127 * 256, 256, 2304, **CONV3) == one('tiled', 64, 128, 127 * 256)
    assert K.gemm_plan(316 * 256, 256, 2304, **CONV3) == [(('dma8', 256, 256), 0, 256), (('tiled', 64, 128), 65536, 240)]
    knobs.solo(0)
    assert K.gemm_plan(M, 256, 2304, **CONV3) == one('dma8', 256, 256, M)


def test_cu_count_is_an_input(K, knobs):
    """The same rules in rounds of another device's compute units (128: a round is 128 8-wave tiles)."""
    assert K.gemm_plan(140 * 256, 256, 2304, cus=128, **CONV3) == [(('dma8', 256, 256), 0, 128), (('tiled', 64, 128), 32768, 48)]
    assert K.gemm_plan(140 * 256, 256, 2304, **CONV3) == one('dma8', 256, 256, 140 * 256)     # 256 CUs: a partial round
    assert K.gemm_plan(4096, 2048, 4096, cus=128) == one('dma8', 256, 256, 4096)              # 128 tiles: eff 1
    assert K.gemm_plan(4096, 2048, 4096) == one('tiled', 64, 128, 4096)                       # half a round: eff 0.5


# ----------------------------------------------------------------------------- forced tiles
FORCED = [(32, 64), (64, 64), (64, 128), (128, 64), (128, 128), (256, 128), (128, 256), (256, 256)]


@pytest.mark.parametrize('bm,bn', FORCED)
def test_forced_tile(K, knobs, bm, bn):
    wave8 = bm == 256 or bn == 256
    knobs.tile(bm, bn)
    assert K.gemm_plan(300, 128, 64) == one('dma8' if wave8 else 'tiled', bm, bn, 300)
    assert K.gemm_plan(70000, 512, 4096, dtype_code=2) == one('dma8' if wave8 else 'tiled', bm, bn, 70000)
    for kw in (dict(dtype_code=F32), dict(dtype_code=X3), dict(a2=True)):
        if wave8:       # the 8-wave tiles exist for 16-bit operands without A2 only
            with pytest.raises(RuntimeError, match='forced tile'):
                K.gemm_plan(300, 128, 64, **kw)
        else:
            assert K.gemm_plan(300, 128, 64, **kw) == one('tiled', bm, bn, 300), kw
    knobs.flags(F_DMA4)
    assert K.gemm_plan(300, 128, 64) == one('dma8' if wave8 else 'tiled-dma', bm, bn, 300)
    if not wave8:
        assert K.gemm_plan(300, 128, 64, dtype_code=F32) == one('tiled-dma', bm, bn, 300)
        assert K.gemm_plan(300, 128, 64, dtype_code=X3) == one('tiled', bm, bn, 300)
        assert K.gemm_plan(300, 128, 64, a2=True) == one('tiled', bm, bn, 300)


def test_forced_tile_refusals(K, knobs):
    """The three refusals of test_forced_tile_without_instantiation_is_refused, without a device."""
    for bm, bn in ((256, 128), (128, 256), (256, 256)):
        knobs.tile(bm, bn)
        with pytest.raises(RuntimeError, match='forced tile'):
            K.gemm_plan(300, 128, 64, dtype_code=F32)            # f32 operands
        with pytest.raises(RuntimeError, match='forced tile'):
            K.gemm_plan(300, 128, 64, a2=True)                   # the load-time add
    knobs.tile(256, 128)
    with pytest.raises(RuntimeError, match='forced tile'):
        K.gemm_plan(300, 128, 64, dtype_code=X3)                 # KINET_F32_X3
    with pytest.raises(RuntimeError, match='unsupported tile'):
        knobs.tile(48, 64)
    for bm, bn in ((32, 256), (64, 320), (128, 320), (32, 128), (0, 64)):    # LayerNorm tiles are not forcible
        with pytest.raises(RuntimeError, match='unsupported tile'):
            knobs.tile(bm, bn)


# -------------------------------------------------------------------- the structural property
# what exists, written out: tile -> (operand classes, A2 allowed)
TILES4 = {(32, 64), (64, 64), (64, 128), (128, 64), (128, 128)}
TILES4_LN = {(32, 256), (32, 320), (64, 256), (64, 320)}
TILES8 = {(256, 128), (128, 256), (256, 256)}


def _serves(kernel, ln, dt, a2):
    fam, bm, bn = kernel
    if fam == 'tiled':
        return (bm, bn) in (TILES4_LN if ln else TILES4)
    if fam == 'tiled-dma' and (bm, bn) != (128, 320):
        return (bm, bn) in (TILES4_LN if ln else TILES4) and dt != X3 and not a2
    if fam == 'tiled-dma':
        return ln and dt in (1, 2) and not a2
    if fam == 'dma8':
        return ((bm, bn) == (256, 256) if ln else (bm, bn) in TILES8) and dt in (1, 2) and not a2
    return False


def test_every_plan_is_runnable_and_covers_the_rows_once(K, knobs):
    """Whatever the heuristics choose: each launch names an instantiation that exists for the operands, and
    the launches' row ranges tile [0, M) exactly once, in order."""
    Ms = [1, 33, 300, 4096, 4097, 8192, 8193, 32640, 65537, 80796, 100864, 131072 + 5, 262144, 700001]
    Ns = [8, 64, 68, 128, 256, 288, 320, 512, 1028]
    n = 0
    for flags, solo in ((0, 0), (0, 1), (F_DMA8, 0), (F_DMA4, 0), (F_DMA8 | F_DMA4, 1), (F_KEEPSPLIT, 0)):
        knobs.flags(flags)
        knobs.solo(solo)
        for M, N, Kd, conv, ln, a2, dt in itertools.product(Ms, Ns, (64, 1152, 4608), (False, True), (False, True),
                                                            (False, True), (BF16, F32, X3)):
            if ln and N > 320:
                continue
            plan = K.gemm_plan(M, N, Kd, dtype_code=dt, conv=conv, Cin=128 if conv else 0, ln=ln, a2=a2)
            n += 1
            assert 1 <= len(plan) <= 2
            row = 0
            for i, (kernel, m_begin, m_tiles) in enumerate(plan):
                assert _serves(kernel, ln, dt, a2), (M, N, Kd, conv, ln, a2, dt, flags, plan)
                assert m_begin == row and m_tiles >= 1, (M, N, Kd, conv, ln, a2, dt, flags, plan)
                row += m_tiles * kernel[1]
                if i + 1 < len(plan):
                    assert row < M                      # a launch before the last one is all whole tiles
            assert row - plan[-1][0][1] < M <= row, (M, N, Kd, conv, ln, a2, dt, flags, plan)
    assert n > 5000


# ------------------------------------------------------------------------------- ksplit_for
# (M, N, K, ln, split-K factor): the values of the Python rule that kinet_gemm_ksplit replaced, recorded from
# the commit before it.  The first twelve are the shapes the GPU tests assert on.
KSPLIT = [
    (1200, 256, 1024, True, 4), (4200, 256, 2048, False, 4), (1000, 91, 2048, False, 4), (300, 1100, 1024, False, 4),
    (546, 256, 18432, False, 4), (8, 1100, 1024, False, 4), (5, 91, 2048, False, 4), (37, 256, 64, True, 1),
    (33, 200, 72, True, 1), (40, 288, 64, True, 1), (64, 256, 1024, True, 4), (50, 288, 1024, True, 4),
    (0, 256, 1024, False, 1), (300, 256, 1023, False, 1), (300, 256, 1024, False, 4), (300, 256, 768, False, 1),
    (4096, 1024, 1024, False, 1), (4096, 1024, 2048, False, 1), (16352, 64, 1024, False, 4), (16353, 64, 2048, False, 4),
    (65408, 64, 1024, False, 2), (65409, 64, 1024, False, 1), (32704, 128, 1024, False, 2), (32705, 128, 1024, False, 1),
    (16352, 256, 1024, True, 3), (16353, 256, 1024, True, 3), (8192, 288, 2304, True, 3), (8193, 288, 2304, True, 4),
    (32704, 288, 1024, True, 2), (32705, 288, 1024, True, 1), (40000, 288, 1024, True, 1), (65409, 288, 1024, True, 1),
    (300, 512, 1024, True, 4), (9000, 1024, 1024, True, 1), (2000, 512, 4608, False, 3), (2000, 1028, 1024, False, 2),
    (4097, 512, 4608, False, 3), (4097, 1028, 1024, False, 1), (8192, 256, 1152, False, 3), (16384, 256, 1152, False, 1),
    (65536, 512, 1024, False, 1), (65536, 508, 1024, False, 1), (44446, 64, 1024, False, 3), (100, 64, 512, False, 1),
    (100, 64, 600, False, 1), (100, 2048, 1024, False, 4), (6000, 2048, 1024, False, 1),
]


def test_ksplit_for_keeps_its_values(K, knobs):
    assert len(KSPLIT) >= 40
    for flags in (0, F_DMA8 | F_DMA4):            # the rule does not read the thread's knobs
        knobs.flags(flags)
        got = [(M, N, Kd, ln, K.ksplit_for(M, N, Kd, ln)) for M, N, Kd, ln, _ in KSPLIT]
        assert got == KSPLIT
