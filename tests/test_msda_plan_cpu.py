"""CPU-only tests of the MSDA launch planner (csrc/msda_plan.h through kinet_msda_launch_plan): the literal
case tables of direct_refs.py, worked by hand from the rules; every rule at its boundary; the structural
properties a plan must have whatever the rules say; and the kernel names kernels.py derives from a plan
against the strings bench.py and train.py parse.  256 compute units.  (The encoder sampler's strip plans:
MSDA_ENC_CASES in tests/test_direct_refs_cpu.py.)"""
import itertools

import pytest
import torch

import direct_refs as R

DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16, 'f64': torch.float64}
ES = {2: 'bf16', 4: 'f32', 8: 'f64'}


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


def last_error():
    from kinet_amd import _native
    return _native.lib().kinet_last_error().decode()


def bwd(K, dt='f32', D=32, Lq=R.MSDA_BWD_S, tune=(0, 0, 0, 0, 0), N=2, S=R.MSDA_BWD_S, M=8, L=4, P=4):
    return K.msda_launch_plan('backward', N, S, M, D, L, Lq, P, DT[dt], tune=tune)


def fwd(K, dt='f32', D=32, Lq=947, N=2, S=R.MSDA_BWD_S, M=8, L=4, P=4):
    return K.msda_launch_plan('forward', N, S, M, D, L, Lq, P, DT[dt])


def fused(K, value='bf16', out='bf16', offlog='f32', D=32, L=4, P=4, S=890, Lq=947, N=2, M=8, strides=(0, 0, 0), align=0):
    return K.msda_launch_plan('fused', N, S, M, D, L, Lq, P, DT[value], DT[out], DT[offlog], strides, align)


# --------------------------------------------------------------------------- the literal tables
@pytest.mark.parametrize('es,D,M,want', R.MSDA_CFG_CASES)
def test_pick_cfg(K, es, D, M, want):
    """pick_cfg as the plain forward plan shows it (vec, lanes per query, queries per workgroup)."""
    got = fwd(K, ES[es], D, M=M)
    if want[2] == 0:
        assert got is None and last_error() == f'msda: heads*channels/vec ({M}*{want[1]}) exceeds one workgroup'
        assert bwd(K, ES[es], D, M=M) is None and 'exceeds one workgroup' in last_error()
    else:
        assert (got['vec'], got['lpq'], got['qt']) == want


@pytest.mark.parametrize('case', R.MSDA_FWD_CASES, ids=lambda c: f'{c[0]}-{c[1]}-{c[2]}')
def test_table_forward(K, case):
    dt, D, Lq, want = case
    assert fwd(K, dt, D, Lq) == want


@pytest.mark.parametrize('case', R.MSDA_FUSED_CASES, ids=lambda c: c[0].replace(' ', '_'))
def test_table_fused(K, case):
    name, prob, want = case
    got = fused(K, **prob)
    if isinstance(want, str):
        assert got is None and last_error() == want
    else:
        assert got == want


@pytest.mark.parametrize('case', R.MSDA_BWD_CASES, ids=lambda c: c[0].replace(' ', '_'))
def test_table_backward(K, case):
    name, dt, D, Lq, tune, want = case
    assert bwd(K, dt, D, Lq, tune) == want


@pytest.mark.parametrize('case', R.MSDA_BWD_TUNE_CASES, ids=lambda c: '-'.join(map(str, c[0] + c[1:3])))
def test_table_backward_tune(K, case):
    """Every (tune, extra queries, D) of test_backward_list_kernel_vs_oracle: its full plan, f32 and bf16 alike
    (4 channels per lane either way: 36 % 8 != 0, and at D = 32 bf16 takes 8)."""
    tune, extra, D, want = case
    assert bwd(K, 'f32', D, R.MSDA_BWD_S + extra, tune) == want
    got = bwd(K, 'bf16', D, R.MSDA_BWD_S + extra, tune)
    assert got['family'] == want['family'] and [got[k] for k in ('grid_z', 'block', 'QP', 'qc', 'log2ns', 'blocked')] == \
        [want[k] for k in ('grid_z', 'block', 'QP', 'qc', 'log2ns', 'blocked')]


# ------------------------------------------------------------------------- the rules, one by one
def test_list_lane_and_channel_limits(K):
    """The list kernel gives a query 16 lanes (lpq <= 16) and a row 16 x NJ channels (nj <= 4)."""
    assert bwd(K, 'f32', 64)['family'] == 'msda_bwd_list_kernel' and bwd(K, 'f32', 64)['nj'] == 4    # lpq 16, nj 4
    assert bwd(K, 'f32', 34)['family'] == 'msda_bwd_kernel'                                          # lpq 17, nj 3
    assert bwd(K, 'bf16', 64)['family'] == 'msda_bwd_list_kernel'                                    # lpq 8, nj 4
    assert bwd(K, 'bf16', 80)['family'] == 'msda_bwd_kernel'                                         # lpq 10, nj 5


def test_list_needs_a_thread_per_channel(K):
    """D <= threads (phase 3 of the kernel): the smallest workgroup, 64, at the widest head the kernel takes."""
    p = bwd(K, 'f32', 64, tune=(0, 0, 0, 64, 0))
    assert (p['family'], p['block'], p['QP']) == ('msda_bwd_list_kernel', 64, 4)
    assert bwd(K, 'f32', 65, M=2, tune=(0, 0, 0, 64, 0))['family'] == 'msda_bwd_kernel'   # (nj = 5 rules it out first)


def test_tune_knob_ranges(K):
    for threads in (64, 128, 512):
        assert bwd(K, tune=(0, 0, 0, threads, 0))['block'] == threads
    for threads in (-64, -1, 1, 32, 100, 576, 1024):
        assert bwd(K, tune=(0, 0, 0, threads, 0)) is None
        assert last_error() == f'msda backward tune: threads {threads} is no multiple of 64 in [64, 512]'
    for rows in (1, 6, 13):
        assert bwd(K, tune=(0, rows, 0, 0, 0))['log2ns'] == rows
    for rows in (-1, 31, 32, 64):
        assert bwd(K, tune=(0, rows, 0, 0, 0)) is None
        assert last_error() == f'msda backward tune: log2_rows {rows} outside [1, 30]'
    # the knobs are read only where the list kernel is eligible
    assert bwd(K, tune=(-1, 99, 0, -64, 0))['family'] == 'msda_bwd_kernel'
    assert bwd(K, Lq=947, tune=(0, 99, 0, -64, 0))['family'] == 'msda_bwd_kernel'


def test_lds_limit_of_each_family(K):
    lim = R.MSDA_LDS_LIMIT
    # forward, f32 D = 32 M = 8: 32 samples' taps per L*P
    assert fwd(K, L=3, P=53)['lds'] == 256 + 32 * 159 * R.MSDA_TAP4 <= lim
    assert fwd(K, L=16, P=10) is None and last_error() == f'msda: LDS request {256 + 32 * 160 * 32} too large'
    # fused generic, f32 D = 32: 4 heads x 8 queries, taps + staged logits; 142 samples fill the limit exactly
    assert fused(K, 'f32', 'f32', L=2, P=71)['lds'] == 256 + 32 * 142 * (R.MSDA_TAP4 + 4) == lim
    assert fused(K, 'f32', 'f32', L=11, P=13) is None
    assert last_error() == f'msda fused: LDS request {256 + 32 * 143 * 36} too large'
    # direct backward
    assert bwd(K, L=1, P=127, tune=(-1, 0, 0, 0, 0))['lds'] == 256 + 32 * 127 * R.MSDA_BWDTAP32 <= lim
    assert bwd(K, L=1, P=128, tune=(-1, 0, 0, 0, 0)) is None
    assert last_error() == f'msda backward: LDS request {256 + 32 * 128 * 40} too large'
    # list backward: passes of 16 queries
    assert bwd(K, L=4, P=29)['lds'] == R.msda_list_lds(16, 116, 32, 10) <= lim < R.msda_list_lds(16, 117, 32, 10)
    assert bwd(K, L=9, P=13) is None
    assert last_error() == 'msda backward: pass of 16 queries x 117 samples does not fit LDS'
    # ... and the hash rows count: 2^13 fit, 2^14 do not
    assert bwd(K, tune=(0, 13, 0, 0, 0))['lds'] == R.msda_list_lds(16, 16, 32, 13) <= lim
    assert bwd(K, tune=(0, 14, 0, 0, 0)) is None and 'does not fit LDS' in last_error()


def test_size_rules(K):
    S = (1 << 23) - 1                                     # S*M*D = 2^31 - 256
    for kind in ('forward', 'fused', 'backward'):
        assert K.msda_launch_plan(kind, 1, S, 8, 32, 4, 100, 4, torch.float32) is not None
        assert K.msda_launch_plan(kind, 1, S + 1, 8, 32, 4, 100, 4, torch.float32) is None
        assert last_error() == 'msda: S*M*D too large for one image'
        assert K.msda_launch_plan(kind, 1, 890, 8, 32, 17, 100, 4, torch.float32) is None
        assert last_error() == 'msda: num_levels 17 > 16'
        assert K.msda_launch_plan(kind, 1, 890, 0, 32, 4, 100, 4, torch.float32) is None
        assert last_error() == 'msda: invalid sizes N=1 S=890 M=0 D=32 L=4 Lq=100 P=4'
    assert fused(K, 'f32', 'f32', D=260) is None and last_error() == 'msda fused: head_dim/vec (65) exceeds a wave'
    assert fused(K, 'f32', 'f32', D=256, M=1)['lpq'] == 64


def test_empty_calls(K):
    for p in (fwd(K, Lq=0), fwd(K, N=0), fused(K, Lq=0), bwd(K, Lq=0), bwd(K, N=0)):
        assert p['family'] == 'none' and p['block'] == 0
    assert fwd(K, Lq=0)['last'] == R.MSDA_KEEP_LAST and fused(K, N=0)['last'] == -1 and bwd(K, N=0)['last'] == -1


# ------------------------------------------------------------- structure, whatever the rules say
SWEEP_D = (1, 4, 6, 8, 12, 16, 24, 32, 33, 36, 48, 64, 72, 80, 128)
SWEEP_M = (1, 3, 5, 8, 12, 16, 64)
SWEEP_LP = ((1, 1), (4, 4), (8, 4), (4, 2), (3, 5), (16, 4))
SWEEP_LQ = (1, 15, 16, 17, 889, 890, 891, 2048, 22223)


def check_structure(p, Lq, N, M):
    assert 0 <= p['lds'] <= R.MSDA_LDS_LIMIT
    assert p['block'] in (128, 256) or (p['block'] % 64 == 0 and 64 <= p['block'] <= 512)
    assert p['grid_y'] == N and p['grid_x'] >= 1
    fam = p['family']
    if fam == 'msda_bwd_list_kernel' and p['blocked']:
        assert p['grid_z'] == M and p['QP'] % 8 == 0
        return
    per = {'msda_fwd_kernel': p['qt'], 'msda_bwd_kernel': p['qt'], 'msda_fused_kernel': p['QT'],
           'msda_fused_fast_kernel': 16, 'msda_bwd_list_kernel': p['qc']}[fam]
    assert per >= 1 and p['grid_x'] * per >= Lq > (p['grid_x'] - 1) * per       # every query exactly once
    if fam in ('msda_fused_kernel', 'msda_fused_fast_kernel'):
        assert p['grid_z'] * p['MH'] >= M > (p['grid_z'] - 1) * p['MH'] and p['block'] == 64 * p['MH']
    elif fam == 'msda_bwd_list_kernel':
        assert p['grid_z'] == M and p['qc'] % p['QP'] == 0
    else:
        assert p['grid_z'] == 1 and p['qt'] * M * p['lpq'] <= p['block']        # a lane per (query, head, vector)


def test_structure_sweep(K):
    n = 0
    for D, M, (L, P), Lq in itertools.product(SWEEP_D, SWEEP_M, SWEEP_LP, SWEEP_LQ):
        for dt in ('f32', 'bf16', 'f64'):
            plans = [fwd(K, dt, D, Lq, M=M, L=L, P=P)]
            plans += [bwd(K, dt, D, Lq, t, M=M, L=L, P=P) for t in ((0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (2, 6, 64, 512, 16))]
            if dt != 'f64':
                plans.append(fused(K, dt, dt, D=D, L=L, P=P, Lq=Lq, M=M))
            for p in plans:
                if p is not None:
                    check_structure(p, Lq, 2, M)
                    n += 1
    assert n > 20000


# ----------------------------------------------------------------------------- the kernel names
def test_kernel_names(K):
    """work['kernel'] as bench.py / tools parse it: rocprofv3's spelling, default template arguments unprinted."""
    bf, hf, f32 = torch.bfloat16, torch.float16, torch.float32
    assert K.msda_encoder_kernel_name(bf, 0, 2, False, 'offlog') == 'msda_enc_kernel<kinet::bf16_t, 0, 2, false>'
    assert K.msda_encoder_kernel_name(hf, 3, 4, True, 'offlog') == 'msda_enc_kernel<kinet::f16_t, 3, 4, true>'
    assert K.msda_encoder_kernel_name(bf, 1, 4, True, 'split') == 'msda_enc_kernel<kinet::bf16_t, 1, 4, true, false, true, 12>'
    assert K.msda_encoder_kernel_name(bf, 1, 2, False, 'split') == 'msda_enc_kernel<kinet::bf16_t, 1, 2, false, false, true, 12>'
    assert K.msda_encoder_kernel_name(hf, 2, 2, False, 'records') == 'msda_enc_kernel<kinet::f16_t, 2, 2, false, true>'
    hm = (890 * 32, 32, 2 * 890 * 32)
    p4 = fused(K, 'f16', 'bf16', 'f16', strides=hm)
    assert K.msda_fused_kernel_name(p4, hf, bf, hf) == 'msda_fused_fast_kernel<kinet::f16_t, kinet::bf16_t, kinet::f16_t, 4, 4, 2, 2>'
    p8 = fused(K, 'bf16', 'bf16', 'f32', L=8, strides=hm)
    assert K.msda_fused_kernel_name(p8, bf, bf, f32) == 'msda_fused_fast_kernel<kinet::bf16_t, kinet::bf16_t, float, 8, 4>'
    pg = fused(K, 'f32', 'f32', 'f32')
    assert K.msda_fused_kernel_name(pg, f32, f32, f32) == 'msda_fused_kernel<float, *>'
    pg = fused(K, 'bf16', 'bf16', 'f32', D=36, strides=(890 * 288, 288, 36))
    assert K.msda_fused_kernel_name(pg, bf, bf, f32) == 'msda_fused_kernel<kinet::bf16_t, *>'
    assert K.MSDA_BWD_LAST == {1: 'msda_bwd_list_kernel', 0: 'msda_bwd_kernel'}
    assert bwd(K)['family'] == K.MSDA_BWD_LAST[bwd(K)['last']] and bwd(K, Lq=947)['family'] == K.MSDA_BWD_LAST[0]
