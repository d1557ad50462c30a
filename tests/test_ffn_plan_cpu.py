"""CPU-only tests of the fused FFN / bottleneck-pair launch planner (csrc/ffn_plan.h through
kinet_ffn_launch_plan) and of the packed-weight layout (kinet_ffn_pack_map): the literal tables of
direct_refs.py, worked by hand from the rules, every rule on both sides of its boundary and every table entry
reached; the structural properties a plan must have whatever the rules say; the layout as a bijection.
256 compute units unless stated."""
import contextlib

import pytest
import torch

import direct_refs as R


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


def last_error():
    from kinet_amd import _native
    return _native.lib().kinet_last_error().decode()


@contextlib.contextmanager
def knobs(debug, solo, cap=0):
    from kinet_amd import _native
    L = _native.lib()
    old, old_solo, old_cap = L.kinet_ffn_set_debug(debug), L.kinet_set_solo_launch(solo), L.kinet_ffn_grid_cap(cap)
    try:
        yield
    finally:
        L.kinet_ffn_set_debug(old)
        L.kinet_set_solo_launch(old_solo)
        L.kinet_ffn_grid_cap(old_cap)


def plan(K, kind, M, D, DB, debug=0, solo=0, cus=256, cap=0, F_=None):
    with knobs(debug, solo, cap):
        return K.ffn_launch_plan(kind, M, D, 4 * D if F_ is None else F_, DB, cus)


# --------------------------------------------------------------------------- the literal tables
@pytest.mark.parametrize('case', R.FFN_PLAN_CASES, ids=lambda c: '-'.join(map(str, c[:6] + c[7:])))
def test_table_plan(K, case):
    kind, M, D, DB, debug, solo, want = case[:7]
    got = plan(K, kind, M, D, DB, debug, solo, cap=case[7] if len(case) > 7 else 0)
    if isinstance(want, str):
        assert got is None and last_error() == want
        return
    waves, rows, wg_tiles, wg_per_cu, lds = R.FFN_KERNELS[want[0]]
    assert got == dict(kernel=want[0], tiles=want[1], grid=want[2], block=64 * waves, waves=waves, tile_rows=rows,
                       wg_tiles=wg_tiles, wg_per_cu=wg_per_cu, lds=lds)


def test_table_of_kernels(K):
    """The instantiations that exist are the 17 of FFN_KERNELS, each reached by a case of the plan table, each within
    the LDS a CU has for the workgroups per CU its grid is sized for."""
    names = []
    while K.ffn_kernel_name(len(names)) is not None:
        names.append(K.ffn_kernel_name(len(names)))
    assert K.ffn_kernel_name(-1) is None
    assert sorted(names) == sorted(R.FFN_KERNELS) and len(names) == 17
    assert {c[6][0] for c in R.FFN_PLAN_CASES if not isinstance(c[6], str)} == set(names)
    for waves, rows, wg_tiles, wg_per_cu, lds in R.FFN_KERNELS.values():
        assert lds * wg_per_cu <= R.FFN_LDS_LIMIT and 64 * waves * wg_per_cu <= 1024


@pytest.mark.parametrize('case', R.FFN_DIRECT_CASES, ids=R.ffn_case_id)
def test_direct_table_plan(K, case):
    """Every row of the direct tests' table (tests/test_ffn_direct_gpu.py), under every grid cap it lists: the kernel it
    names, its row tiles and the grid; M is five ragged tiles, the 16384-row floor's 65 / 130, or 2 waves + 3 tiles."""
    kind, D, F_, DB, M, debug, solo, kernel, rows, caps = case
    waves, tile_rows, wg_tiles, wg_per_cu, lds = R.FFN_KERNELS[kernel]
    assert rows == tile_rows and M % rows == rows - 5 and 0 in caps
    tiles = -(-M // rows)
    assert tiles in (5, 65, 130, 2 * waves + 3) and (tiles == 2 * waves + 3) == (wg_tiles > 1)
    assert caps[0] == -(-tiles // wg_tiles) and all(grid == min(cap, caps[0]) for cap, grid in caps.items() if cap)
    for cap, grid in caps.items():
        got = plan(K, kind, M, D, DB, debug, solo, cap=cap, F_=F_)
        assert got == dict(kernel=kernel, tiles=tiles, grid=grid, block=64 * waves, waves=waves, tile_rows=rows,
                           wg_tiles=wg_tiles, wg_per_cu=wg_per_cu, lds=lds), (cap, got)


def test_direct_table_reaches_every_kernel():
    assert {c[7] for c in R.FFN_DIRECT_CASES} == set(R.FFN_KERNELS)
    # the hidden-chunk counts of the FFN entries: 1, 2, 5 on every kernel, FFN_MAX_F on those that run at few rows
    for kernel in {c[7] for c in R.FFN_DIRECT_CASES if c[0] in ('ffn', 'attn_out_ffn')}:
        fs = {c[2] for c in R.FFN_DIRECT_CASES if c[7] == kernel}
        small = {c[4] for c in R.FFN_DIRECT_CASES if c[7] == kernel} != {R.FFN_BIG_ROWS}
        assert fs == ({32, 64, 160, 2048} if small else {32, 64, 160}), kernel


def test_grid_cap_is_per_thread_state_with_the_previous_value_returned(K):
    assert K.ffn_grid_cap(5) == 0 and K.ffn_grid_cap(-1) == 5 and K.ffn_grid_cap(0) == 0
    with knobs(0, 0, 3):
        assert K.ffn_launch_plan('ffn', 1000, 256)['grid'] == 3
    assert K.ffn_launch_plan('ffn', 1000, 256)['grid'] == 16


def test_row_threshold(K):
    """kernels.ATTN_OUT_FFN_MIN_ROWS restates the planner's threshold: kinet_ffn_fused flips to the 8-wave x 32-row
    tile -- the only one kinet_attn_out_ffn_fused runs on -- exactly there."""
    M = K.ATTN_OUT_FFN_MIN_ROWS
    below, at = plan(K, 'ffn', M - 1, 256, 256), plan(K, 'ffn', M, 256, 256)
    assert below['kernel'] == 'ffn_fused_kernel<256, 1, 4>' and at['kernel'] == 'ffn_fused_rt2_kernel<256>'
    pre = plan(K, 'attn_out_ffn', M, 256, 256)
    assert (pre['tile_rows'], pre['waves'], pre['tiles'], pre['grid']) == (at['tile_rows'], at['waves'], at['tiles'], at['grid'])


def test_plan_reads_the_threads_knobs(K):
    """The plan answers under the calling thread's debug bits and the solo policy, as a launch does."""
    from kinet_amd import _native
    assert _native.lib().kinet_ffn_set_debug(0) == 0
    assert K.ffn_launch_plan('pair_ds', 1000, 64)['kernel'] == 'bneck64_ds_kernel<1>'
    with knobs(R.FFN_DBG_DS_RT2, 0):
        assert K.ffn_launch_plan('pair_ds', 1000, 64)['kernel'] == 'bneck64_ds_kernel<2>'
    assert K.ffn_launch_plan('pair_ds', 1000, 64)['kernel'] == 'bneck64_ds_kernel<1>'
    assert K.ffn_launch_plan('pair_ds', 0, 64)['grid'] == 0     # an empty call launches nothing


# ------------------------------------------------------------------ structure, whatever the rules
def _sweep_rows():
    Ms = set(range(1, 40))
    for rows in (16, 32, 64, 128, 256):
        for rounds in (1, 2, 3):
            for cus in (32, 64, 256, 304, 512, 608):
                edge = rows * cus * rounds
                Ms.update((edge - 1, edge, edge + 1))
        Ms.update(rows * k + d for k in (1, 2, 3, 7) for d in (-1, 0, 1))
    # the models' row counts: encoder tokens and decoder queries per batch, the ResNet stages' pixels
    Ms.update((300, 900, 8400, 16383, 16384, 16385, 22223, 32640, 40007, 117600, 134400, 355568, 622244, 1068800))
    return sorted(Ms)


@pytest.mark.parametrize('cus', [32, 64, 256, 304])
def test_structure(K, cus):
    problems = [('ffn', 256, 256, (0, 2, 8)), ('ffn', 288, 288, (0,)), ('attn_out_ffn', 256, 256, (0, 64)),
                ('pair', 64, 64, (0, 16)), ('pair', 64, 128, (0,)), ('pair', 128, 128, (0, 128, 256)),
                ('pair', 256, 256, (0, 128, 256)), ('pair_ds', 64, 64, (0, 512))]
    for kind, D, DB, debugs in problems:
        for debug in debugs:
            for solo, cap in ((0, 0), (1, 0), (0, 1), (1, 7), (0, cus), (0, 1 << 30)):
                with knobs(debug, solo, cap):
                    for M in _sweep_rows():
                        p = K.ffn_launch_plan(kind, M, D, 4 * D, DB, cus)
                        assert 1 <= p['grid'] <= cus * p['wg_per_cu'], (kind, D, DB, debug, solo, cap, M, p)
                        assert p['tiles'] * p['tile_rows'] >= M > (p['tiles'] - 1) * p['tile_rows']
                        assert p['block'] == 64 * p['waves'] <= 1024
                        # a grid below its caps covers every tile at once; kinet_ffn_grid_cap is one more cap
                        assert p['grid'] == min(-(-p['tiles'] // p['wg_tiles']), cus * p['wg_per_cu'], cap or 1 << 30)
                        assert p['lds'] * p['wg_per_cu'] <= R.FFN_LDS_LIMIT
                        assert (p['waves'], p['tile_rows'], p['wg_tiles'], p['wg_per_cu'], p['lds']) == R.FFN_KERNELS[p['kernel']]


# ------------------------------------------------------------------------- the packed layout
@pytest.mark.parametrize('case', R.FFN_PACK_CASES, ids=lambda c: '-'.join(map(str, c[:5])))
def test_pack_map_by_hand(K, case):
    kind, D, F, DB, idx, want = case
    assert tuple(K.ffn_pack_map(kind, D, F, DB)[idx].tolist()) == want


@pytest.mark.parametrize('shape', R.FFN_PACK_SHAPES, ids=lambda s: '-'.join(map(str, s)))
def test_pack_map_is_a_bijection(K, shape):
    """Every element of every source matrix lands in the packed stream exactly once."""
    kind, D, F, DB = shape
    m = K.ffn_pack_map(kind, D, F, DB).long()
    shapes = R.ffn_pack_shapes(kind, D, F, DB)
    assert m.shape[0] == sum(r * c for r, c in shapes)
    for i, (rows, cols) in enumerate(shapes):
        sel = m[m[:, 0] == i]
        assert (sel[:, 1] >= 0).all() and (sel[:, 1] < rows).all() and (sel[:, 2] >= 0).all() and (sel[:, 2] < cols).all()
        assert torch.equal(torch.sort(sel[:, 1] * cols + sel[:, 2]).values, torch.arange(rows * cols))
    assert int(m[:, 0].max()) == len(shapes) - 1


def test_pack_map_refusals(K):
    for kind, D, F, DB in (('ffn', 48, 64, 48), ('ffn', 64, 48, 64), ('pair', 64, 256, 48), ('ffn', 64, 256, 128)):
        with pytest.raises(RuntimeError, match='ffn_pack_map'):
            K.ffn_pack_map(kind, D, F, DB)
