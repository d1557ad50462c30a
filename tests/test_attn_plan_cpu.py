"""CPU-only tests of the attention-core launch planner (csrc/attn_plan.h through kinet_mha_launch_plan): a
literal table worked by hand from the rules, every rule on both sides of its boundary; the LDS sizes as
structure; the numbers kernels.py reads from the library, pinned once.

The rules: the MFMA kernels take bf16 / f16, head_dim 32 (row strides % 8, 16-byte pointers) or 36 (row strides
% 4, 8-byte pointers), Lk >= 1, batch and heads <= 65535, no dropout, knob != 0; knob 2 -> streaming, else
resident up to Lk 384 / 640 and streaming above; grid (ceil(Lq / 64), heads, batch), 256 threads.  Everything
else: the FMA kernel, grid (ceil(Lq / 16), heads, batch), no dynamic LDS.
LDS by hand: n staged keys hold n key rows of 80 / 144 B, 32 / 48 transposed value rows of 2 (n + 8) B and n
bias floats = 148 n + 512 B at head_dim 32, 244 n + 768 B at 36; resident n = Lk rounded up to 32, streaming two
buffers of n = 128."""
import pytest
import torch

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


def _knob(value):
    from kinet_amd import _native
    return _native.lib().kinet_mha_set_mfma(value)


# (dtype, head_dim, batch, heads, Lq, Lk, ld, align, dropout, knob) -> (kernel, grid x, y, z, block, LDS bytes)
CASES = [
    # the resident caps
    ((BF, 32, 16, 8, 300, 384, 256, 16, 0, 1), ('resident', 5, 8, 16, 256, 148 * 384 + 512)),
    ((BF, 32, 16, 8, 300, 385, 256, 16, 0, 1), ('stream', 5, 8, 16, 256, 38912)),
    ((HF, 36, 16, 8, 500, 640, 288, 16, 0, 1), ('resident', 8, 8, 16, 256, 244 * 640 + 768)),
    ((HF, 36, 16, 8, 500, 641, 288, 16, 0, 1), ('stream', 8, 8, 16, 256, 64000)),
    # the models' resident shapes: Lk rounds up to whole 32-key blocks
    ((BF, 32, 16, 8, 300, 300, 256, 16, 0, 1), ('resident', 5, 8, 16, 256, 148 * 320 + 512)),
    ((BF, 36, 16, 8, 520, 520, 288, 8, 0, 1), ('resident', 9, 8, 16, 256, 244 * 544 + 768)),
    # no key / one key
    ((BF, 32, 3, 8, 65, 0, 256, 16, 0, 1), ('fma', 5, 8, 3, 256, 0)),
    ((BF, 32, 3, 8, 65, 1, 256, 16, 0, 1), ('resident', 2, 8, 3, 256, 148 * 32 + 512)),
    ((BF, 36, 3, 8, 65, 0, 288, 16, 0, 1), ('fma', 5, 8, 3, 256, 0)),
    ((BF, 36, 3, 8, 65, 1, 288, 16, 0, 1), ('resident', 2, 8, 3, 256, 244 * 32 + 768)),
    # row strides: whole 16-byte pieces at head_dim 32, whole 8-byte pieces at 36, every one of the four
    ((BF, 32, 3, 8, 64, 37, 264, 16, 0, 1), ('resident', 1, 8, 3, 256, 148 * 64 + 512)),
    ((BF, 32, 3, 8, 64, 37, 260, 16, 0, 1), ('fma', 4, 8, 3, 256, 0)),
    ((BF, 32, 3, 8, 64, 37, (512, 512, 256, 260), 16, 0, 1), ('fma', 4, 8, 3, 256, 0)),
    ((BF, 32, 3, 8, 64, 37, (512, 512, 256, 256), 16, 0, 1), ('resident', 1, 8, 3, 256, 148 * 64 + 512)),
    ((BF, 36, 3, 8, 64, 37, 292, 8, 0, 1), ('resident', 1, 8, 3, 256, 244 * 64 + 768)),
    ((BF, 36, 3, 8, 64, 37, 290, 8, 0, 1), ('fma', 4, 8, 3, 256, 0)),
    ((BF, 36, 3, 8, 64, 37, (290, 288, 288, 288), 8, 0, 1), ('fma', 4, 8, 3, 256, 0)),
    # pointer alignment
    ((HF, 32, 3, 8, 64, 37, 256, 16, 0, 1), ('resident', 1, 8, 3, 256, 148 * 64 + 512)),
    ((HF, 32, 3, 8, 64, 37, 256, 8, 0, 1), ('fma', 4, 8, 3, 256, 0)),
    ((HF, 32, 3, 8, 64, 37, 256, 4, 0, 1), ('fma', 4, 8, 3, 256, 0)),
    ((HF, 36, 3, 8, 64, 37, 288, 16, 0, 1), ('resident', 1, 8, 3, 256, 244 * 64 + 768)),
    ((HF, 36, 3, 8, 64, 37, 288, 8, 0, 1), ('resident', 1, 8, 3, 256, 244 * 64 + 768)),
    ((HF, 36, 3, 8, 64, 37, 288, 4, 0, 1), ('fma', 4, 8, 3, 256, 0)),
    # dtype, dropout
    ((F32, 32, 3, 8, 64, 37, 256, 16, 0, 1), ('fma', 4, 8, 3, 256, 0)),
    ((F32, 36, 3, 8, 64, 37, 288, 16, 0, 2), ('fma', 4, 8, 3, 256, 0)),
    ((BF, 32, 3, 8, 64, 37, 256, 16, 1, 1), ('fma', 4, 8, 3, 256, 0)),
    ((BF, 36, 3, 8, 64, 700, 288, 16, 1, 2), ('fma', 4, 8, 3, 256, 0)),
    # the knob
    ((BF, 32, 3, 8, 64, 37, 256, 16, 0, 0), ('fma', 4, 8, 3, 256, 0)),
    ((BF, 32, 3, 8, 64, 700, 256, 16, 0, 0), ('fma', 4, 8, 3, 256, 0)),
    ((BF, 32, 3, 8, 64, 37, 256, 16, 0, 2), ('stream', 1, 8, 3, 256, 38912)),
    ((BF, 36, 3, 8, 64, 37, 288, 16, 0, 2), ('stream', 1, 8, 3, 256, 64000)),
    ((BF, 36, 3, 8, 64, 700, 288, 16, 0, 2), ('stream', 1, 8, 3, 256, 64000)),
    # other head dims
    ((BF, 16, 3, 8, 64, 37, 128, 16, 0, 1), ('fma', 4, 8, 3, 256, 0)),
    ((BF, 64, 3, 8, 64, 37, 512, 16, 0, 2), ('fma', 4, 8, 3, 256, 0)),
    # batch and heads ride on grid z / y
    ((BF, 32, 65535, 1, 1, 1, 32, 16, 0, 1), ('resident', 1, 1, 65535, 256, 148 * 32 + 512)),
    ((BF, 32, 65536, 1, 1, 1, 32, 16, 0, 1), ('fma', 1, 1, 65536, 256, 0)),
    ((BF, 36, 1, 65535, 1, 1, 36 * 65535, 8, 0, 2), ('stream', 1, 65535, 1, 256, 64000)),
    ((BF, 36, 1, 65536, 1, 1, 36 * 65536, 8, 0, 2), ('fma', 1, 65536, 1, 256, 0)),
    # an empty call: a zero grid
    ((BF, 32, 0, 8, 64, 37, 256, 16, 0, 1), ('resident', 1, 8, 0, 256, 148 * 64 + 512)),
    ((BF, 32, 3, 8, 0, 37, 256, 16, 0, 1), ('resident', 0, 8, 3, 256, 148 * 64 + 512)),
]


def _id(case):
    p = case[0]
    return '-'.join([str(p[0]).replace('torch.', '')] + [str(x).replace(' ', '') for x in p[1:]])


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_table_plan(K, case):
    (dtype, D, B, H, Lq, Lk, ld, align, dropout, knob), want = case
    got = K.mha_launch_plan(dtype, D, B, H, Lq, Lk, ld=ld, align=align, dropout=dropout, knob=knob)
    assert tuple(got[f] for f in K.MHA_PLAN_FIELDS[:6]) == want


def test_plan_refuses_what_the_entry_point_refuses(K):
    with pytest.raises(RuntimeError, match='head_dim 48 not instantiated'):
        K.mha_launch_plan(BF, 48, 1, 8, 1, 1)
    with pytest.raises(RuntimeError, match='bad sizes'):
        K.mha_launch_plan(BF, 32, 1, 8, 1, -1)


def test_plan_reads_the_threads_knob_unless_overridden(K):
    assert _knob(1) == 1
    assert K.mha_launch_plan(BF, 32, 1, 8, 64, 37)['kernel'] == 'resident'
    for knob, kernel in ((2, 'stream'), (0, 'fma')):
        old = _knob(knob)
        try:
            assert K.mha_launch_plan(BF, 32, 1, 8, 64, 37)['kernel'] == kernel
            assert K.mha_launch_plan(BF, 32, 1, 8, 64, 37, knob=1)['kernel'] == 'resident'
        finally:
            _knob(old)
    assert K.mha_launch_plan(BF, 32, 1, 8, 64, 37)['kernel'] == 'resident'


LDS_LIMIT = 160 * 1024


@pytest.mark.parametrize('D', [32, 36])
def test_resident_lds_fits_up_to_the_cap(K, D):
    cap = K.MHA_RESIDENT_MAXK[D]
    sizes = [K.mha_launch_plan(BF, D, 1, 8, 64, Lk, knob=1) for Lk in range(1, cap + 2)]
    assert all(p['kernel'] == 'resident' for p in sizes[:cap]) and sizes[cap]['kernel'] == 'stream'
    lds = [p['lds'] for p in sizes[:cap]]
    assert all(0 < n <= LDS_LIMIT and n % 16 == 0 for n in lds)
    # one size per 32-key block, growing by the same step
    step = 32 * (148 if D == 32 else 244)
    assert all(lds[Lk - 1] == lds[0] + (Lk - 1) // 32 * step for Lk in range(1, cap + 1))
    if D == 36:     # the cap is the LDS limit: the next block (Lk 641 .. 672) would not fit
        assert lds[-1] + step == 164736 > LDS_LIMIT


def test_stream_lds_is_two_tile_buffers(K):
    for D, want in ((32, 38912), (36, 64000)):
        for Lk in (1, 128, 129, 1050, 100000):
            assert K.mha_launch_plan(HF, D, 1, 8, 64, Lk, knob=2)['lds'] == want
    assert 4 * 38912 <= LDS_LIMIT < 5 * 38912 and 2 * 64000 <= LDS_LIMIT < 3 * 64000   # workgroups per CU


def test_numbers_kernels_py_reads_from_the_library(K):
    assert K.MHA_RESIDENT_MAXK == {32: 384, 36: 640}
    assert K.MHA_STREAM_KT == 128
    from kinet_amd.kernels import MHA_STREAM_KT
    assert MHA_STREAM_KT == 128
    assert K.mha_launch_plan(BF, 64, 1, 8, 1, 1)['resident_maxk'] == 0
