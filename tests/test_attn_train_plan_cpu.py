"""The planner of the f32 attention training pair (csrc/attn_train_plan.h) through its export
kinet_mha_train_plan, the workspace size, and the argument checks of the two entry points -- all on the
host, no GPU call.  The table is worked by hand from the plan's rules, with both sides of every boundary."""
import pytest

from kinet_amd import _native as N
from kinet_amd import kernels as K

QT = KT = 64                    # the literal tile sizes the table below is worked from
GEO = {32: dict(ks=8, dt=2, sa=34, st=36), 36: dict(ks=9, dt=3, sa=38, st=52)}


def _lds(D):
    g = GEO[D]
    row, col = KT * g['sa'] * 4, KT * g['st'] * 4
    return dict(fwd=row + col + KT * 4,                 # K rows, V columns, key bias
                dq=2 * row + col + KT * 4,              # K rows + columns, V rows, key bias
                dkv=2 * row + 2 * col + 2 * QT * 4)     # Q and dO rows + columns, lse and delta of the tile


def _launches(p):
    return {k: (p[k + '_grid_x'], p[k + '_grid_y'], p[k + '_grid_z'], p[k + '_block'], p[k + '_lds'])
            for k in ('fwd', 'dq', 'dkv')}


# (head_dim, batch, heads, Lq, Lk) -> (fwd / dq grid x, dkv grid x); y = heads, z = batch
TABLE = [
    ((32, 2, 8, 1050, 1050), 17, 17),
    ((36, 2, 8, 1050, 1050), 17, 17),
    ((32, 1, 1, 1, 1), 1, 1),
    ((32, 1, 1, QT - 1, KT - 1), 1, 1),
    ((32, 1, 1, QT, KT), 1, 1),
    ((32, 1, 1, QT + 1, KT), 2, 1),
    ((32, 1, 1, QT, KT + 1), 1, 2),
    ((36, 3, 5, 2 * QT, 2 * KT + 1), 2, 3),
    ((36, 8, 8, 2100, 2100), 33, 33),
    ((32, 65535, 65535, 100, 7), 2, 1),
]


@pytest.mark.parametrize('prob,gq,gk', TABLE)
def test_plan_table(prob, gq, gk):
    D, B, H = prob[:3]
    p = K.mha_train_plan(*prob)
    lds = _lds(D)
    assert p['supported'] == 1 and (p['qt'], p['kt']) == (QT, KT)
    assert (p['row_stride'], p['col_stride']) == (GEO[D]['sa'], GEO[D]['st'])
    assert _launches(p) == {'fwd': (gq, H, B, 256, lds['fwd']), 'dq': (gq, H, B, 256, lds['dq']),
                            'dkv': (gk, H, B, 256, lds['dkv'])}


def test_lds_bytes_are_literal_and_fit():
    assert _lds(32) == dict(fwd=18176, dq=26880, dkv=36352)
    assert _lds(36) == dict(fwd=23296, dq=33024, dkv=46592)
    assert all(v <= 160 * 1024 for D in GEO for v in _lds(D).values())
    for D, g in GEO.items():
        # the conflict-free strides: rows c = 0..15 on distinct even banks of 32; rows 4g + r of g = 0, 1
        # sixteen banks apart; the padded tiles hold the head dim
        assert sorted(c * g['sa'] % 32 for c in range(16)) == list(range(0, 32, 2))
        assert 4 * g['st'] % 32 == 16
        assert g['ks'] * 4 == D and g['dt'] * 16 >= D and g['st'] >= g['dt'] * 16 and g['sa'] >= D


@pytest.mark.parametrize('D', [16, 20, 31, 33, 40, 48, 64, 0])
def test_other_head_dims_are_refused(D):
    p = K.mha_train_plan(D, 2, 8, 100, 100)
    assert p['supported'] == 0 and p['dense_default'] == 0
    assert all(v == (0, 0, 0, 0, 0) for v in _launches(p).values())


def test_grid_limits():
    assert K.mha_train_plan(32, 65535, 65535, 1, 1)['supported'] == 1
    assert K.mha_train_plan(32, 65536, 1, 1, 1)['supported'] == 0
    assert K.mha_train_plan(32, 1, 65536, 1, 1)['supported'] == 0


@pytest.mark.parametrize('prob', [(32, 0, 8, 100, 100), (36, 2, 8, 0, 100)])
def test_empty_batch_or_queries_give_zero_grids(prob):
    p = K.mha_train_plan(*prob)
    assert p['supported'] == 1
    assert all(v[:3] == (0, 0, 0) for v in _launches(p).values())


def test_no_keys_launch_the_query_kernels_only():
    """Lk = 0: every row is without a key (O = 0, lse = -inf, dQ = 0); there is no key tile."""
    ln = _launches(K.mha_train_plan(32, 2, 8, 100, 0))
    assert ln['fwd'][:3] == ln['dq'][:3] == (2, 8, 2) and ln['dkv'][:3] == (0, 0, 0)


def test_every_dense_call_takes_the_new_pair():
    """No crossover in profiles/detr_train_bench.jsonl: the planner gives every key count to the pair."""
    assert all(K.mha_train_plan(32, 2, 8, 100, Lk)['dense_default'] == 1 for Lk in (1, 64, 100, 1050, 2100))


def test_backward_workspace_is_linear_in_queries():
    L = N.lib()
    assert L.kinet_mha_train_backward_workspace(2, 1050, 8) == 2 * 8 * 1050
    assert L.kinet_mha_train_backward_workspace(8, 2100, 8) == 8 * 8 * 2100
    assert L.kinet_mha_train_backward_workspace(3, 7, 5) == 105
    assert L.kinet_mha_train_backward_workspace(0, 7, 5) == 0


# --------------------------------------------------------------------------- the C ABI's argument checks
def _err(name, *args):
    with pytest.raises(RuntimeError) as e:
        N.call(name, *args)
    return str(e.value)


def _fwd(B, Lq, Lk, H, D, p=0.0, ld=None, ptr=None):
    ld = H * D if ld is None else ld
    return ('kinet_mha_train_forward', ptr, ld, ptr, ld, ptr, ld, ptr, ld, ptr, B, Lq, Lk, H, D, 0.1, None, p, None, None)


def _bwd(B, Lq, Lk, H, D, p=0.0, ld=None, ptr=None, ws=None):
    ld = H * D if ld is None else ld
    return ('kinet_mha_train_backward', ptr, ld, ptr, ld, ptr, ld, ptr, ld, ptr, ld, ptr, ptr, ptr, ptr, B, Lq, Lk, H, D, 0.1,
            None, ws, p, None, None)


@pytest.mark.parametrize('call', [_fwd, _bwd])
def test_abi_rejects_bad_arguments_before_any_launch(call):
    """Null pointers throughout: every call must fail on its arguments, not reach a launch."""
    assert 'bad sizes' in _err(*call(-1, 4, 4, 2, 32))
    assert 'bad sizes' in _err(*call(1, 4, 4, 0, 32))
    for D in (16, 33, 64):
        assert f'head_dim {D}' in _err(*call(1, 4, 4, 2, D))
    assert 'grid limit' in _err(*call(65536, 4, 4, 2, 32))
    assert 'dropout' in _err(*call(1, 4, 4, 2, 32, p=0.1))          # p > 0 without a seed
    assert 'dropout' in _err(*call(1, 4, 4, 2, 32, p=1.0))
    assert 'null' in _err(*call(1, 4, 4, 2, 32))
    kw = dict(ws=16) if call is _bwd else {}
    assert 'row strides' in _err(*call(1, 4, 4, 2, 36, ld=71, ptr=16, **kw))       # below 2 * 36


def test_abi_backward_needs_its_workspace():
    assert 'workspace' in _err(*_bwd(1, 4, 4, 2, 32, ptr=16))


@pytest.mark.parametrize('call', [_fwd, _bwd])
def test_abi_empty_calls_are_no_ops(call):
    assert N.call(*call(0, 4, 4, 2, 32)) == 0
    assert N.call(*call(2, 0, 4, 2, 36)) == 0


def test_plan_export_checks_its_arguments():
    assert 'invalid' in _err('kinet_mha_train_plan', None, None)
