"""Direct tests of the fused FFN and bottleneck-pair kernels (csrc/ffn.hip: ffn_fused_kernel, ffn_fused_rt2_kernel
plain / PRE / PRE + RV 1, bneck_pair_kernel, bneck64_kernel, bneck64_ds_kernel), instantiation by instantiation,
against f64 references (tests/direct_refs.py, checked on the CPU by test_direct_refs_cpu.py).

Every row of R.FFN_DIRECT_CASES runs in bf16 and f16 through the public pack entry and the public launch entry under
each grid cap the row lists (kinet_ffn_grid_cap): one tile per workgroup, one workgroup walking every tile, and
uneven splits -- the persistent walk (cnt > 1, the counted vmcnt of the ring, the next tile's x prefetch, the ring
phase carried over a tile boundary, bneck64's refill of the residual registers) at a few tiles.  The expected kernel
of each row is asserted through kinet_ffn_last_kernel; test_ffn_plan_cpu.py checks the rows' kernels and grids
against the planner without a GPU.  The whole output buffers must be bit-identical under every cap, sentinels
included, and the cap-0 output is compared with the reference.

Shapes: ragged last tiles; F = 32, 64, 160 (1, 2 and 5 hidden chunks: the ring's special cases and a count that is a
multiple of neither ring depth) and F = 2048 (the edge of the b1 LDS array); the pairs at F = 4 D.  Strides: ldx =
D + 8 everywhere, ldy = D + 16 (FFN entries), lda = D + 8, ldr = D + 24 (attention entry), ldx0 = 72; input gap
columns hold NaN, outputs are views of a sentinel-filled buffer with rows below M.

Classes: EXACT (dyadic operands: every f32 partial sum, every rounded intermediate and the output are exact, so the
output must EQUAL the f64 value: one dropped, doubled or misplaced product is a failure), EXACT operands with the
final LayerNorm on under test_ln_epilogue_direct_gpu.py's bound at both of its offsets (the offset enters through b2),
and GENERIC (randn) under ffn_generic_bound, kinet_ffn_fused with the LayerNorm on at F = 64 and 2048 and off at F = 32
and 160.  That bound is a worst case over every rounding of the chain (the hidden's two roundings carried through
|W2| without cancellation), so it is wide -- widest for the attention entry, three 16-bit roundings deep, which is
why its generic rows keep the second LayerNorm off: the bound could not be carried through it.  The exact class is
the sharp check; the generic class guards what dyadic operands cannot reach (mantissa bits, rounding places).

The self-checks zero one weight in what is packed but not in the reference: the exact comparison must then report
mismatches in exactly the rows the reference predicts.

KINET_FFN_DIRECT_LOG names a file that receives the module's figures (profiles/ffn_direct.log)."""
import os
import time

import pytest
import torch

import direct_refs as R
from test_ln_epilogue_direct_gpu import OFFSETS

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
SENTINEL = 77.0
TAIL_ROWS = 8               # sentinel rows below each output

_LOG = {'t0': None, 'worst': {}, 'exact_bad': 0, 'exact_n': 0, 'reached': {BF16: {}, F16: {}}, 'self': []}


def _name(dt):
    return str(dt).replace('torch.', '')


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


@pytest.fixture(scope='module', autouse=True)
def _report():
    _LOG['t0'] = time.time()
    yield
    lines = [f'module wall time: {time.time() - _LOG["t0"]:.1f} s',
             f'exact class: {_LOG["exact_bad"]} of {_LOG["exact_n"]} elements not equal to the expected value']
    for dt in (BF16, F16):
        lines.append(f'kernels reached in {_name(dt)} ({len(_LOG["reached"][dt])}), as {{cap: grid}}: cases')
        for k, (grids, cases) in sorted(_LOG['reached'][dt].items()):
            lines.append(f'  {k} {dict(sorted(grids))}: ' + ', '.join(sorted(cases)))
    lines.append('worst err / bound per case (exact class: 0 = every element equal):')
    lines += [f'  {k}: {v:.3f}' for k, v in sorted(_LOG['worst'].items())]
    lines.append('self-checks (one weight zeroed in the packed stream only):')
    lines += ['  ' + s for s in _LOG['self']]
    print('\n'.join(lines))
    path = os.environ.get('KINET_FFN_DIRECT_LOG')
    if path:
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


@pytest.fixture
def knobs(K):
    """The debug bits, the grid cap and the solo policy for one test, restored afterwards."""
    from kinet_amd import _native
    L = _native.lib()
    old = L.kinet_ffn_set_debug(0), K.ffn_grid_cap(0), L.kinet_set_solo_launch(0)

    class Knobs:
        debug = staticmethod(L.kinet_ffn_set_debug)
        cap = staticmethod(K.ffn_grid_cap)
        solo = staticmethod(L.kinet_set_solo_launch)
    yield Knobs
    L.kinet_ffn_set_debug(old[0])
    K.ffn_grid_cap(old[1])
    L.kinet_set_solo_launch(old[2])


def _note(name, ratio):
    _LOG['worst'][name] = max(_LOG['worst'].get(name, 0.0), ratio)


def _strided(v, ld, dtype):
    """v (M, D) as a view of an (M, ld) buffer whose gap columns hold NaN."""
    buf = torch.full((v.shape[0], ld), float('nan'), dtype=dtype, device='cuda')
    buf[:, :v.shape[1]] = v.to(dtype)
    return buf[:, :v.shape[1]]


def _run(K, knobs, case, d, dtype, ln=False, offset=0.0, zero=None):
    """Pack and launch a row of the table under each of its caps.  Returns {output name: (M, N) CPU tensor} of the
    cap-0 run.  zero = (weight key, row, column): that weight is 0 in what is packed."""
    from kinet_amd import _native as N
    kind, D, F_, DB, M, debug, solo, kernel, _, caps = case
    ld = R.ffn_direct_ld(case)
    code, st = N.dtype_code(dtype), N.stream(torch.device('cuda:0'))
    f32 = {k: v.cuda() for k, v in d.items() if torch.is_tensor(v)}
    if zero is not None:
        f32[zero[0]] = f32[zero[0]].clone()
        f32[zero[0]][zero[1], zero[2]] = 0
    ffn_like = kind in ('ffn', 'attn_out_ffn')
    w16 = {k: f32[k].to(dtype).contiguous() for k in ('Wo', 'W1', 'W2') if ffn_like and k in f32}
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if kind == 'ffn':
        packed = torch.empty(2 * D * F_, dtype=dtype, device='cuda')
        N.call('kinet_ffn_pack', N.ptr(w16['W1']), N.ptr(w16['W2']), N.ptr(packed), D, F_, code, st)
        x = _strided(f32['x'], ld['ldx'], dtype)
    elif kind == 'attn_out_ffn':
        packed = torch.empty(D * D + 2 * D * F_, dtype=dtype, device='cuda')
        N.call('kinet_ffn_pack_attn', N.ptr(w16['Wo']), N.ptr(w16['W1']), N.ptr(w16['W2']), N.ptr(packed), D, F_, code, st)
        a, r = _strided(f32['A'], ld['lda'], dtype), _strided(f32['R'], ld['ldr'], dtype)
    elif kind == 'pair':
        packed = torch.empty((D + DB) * F_, dtype=dtype, device='cuda')
        N.call('kinet_bottleneck_pack', N.ptr(f32['W3']), N.ptr(f32['W1']), N.ptr(f32['s3']), N.ptr(f32['s1']), N.ptr(packed),
               D, F_, DB, code, st)
        x, r = _strided(f32['X'], ld['ldx'], dtype), f32['R'].to(dtype).contiguous()
    else:
        packed = torch.empty((2 * D + DB) * F_, dtype=dtype, device='cuda')
        N.call('kinet_bottleneck_pack_ds', N.ptr(f32['W3']), N.ptr(f32['Wds']), N.ptr(f32['W1']), N.ptr(f32['s3']),
               N.ptr(f32['sds']), N.ptr(f32['s1']), N.ptr(packed), D, F_, DB, code, st)
        x, x0 = _strided(f32['X'], ld['ldx'], dtype), _strided(f32['X0'], ld['ldx0'], dtype)
    if ffn_like:
        b2 = f32['b2'] + offset
        g2, be2, eps2 = (d['ln'][0].cuda(), d['ln'][1].cuda(), d['ln'][2]) if ln else (None, None, 0.0)
    knobs.debug(debug)
    knobs.solo(solo)
    first = None
    for cap in caps:
        knobs.cap(cap)
        if ffn_like:
            bufs = [torch.full((M + TAIL_ROWS, ld['ldy']), SENTINEL, dtype=dtype, device='cuda')]
            if kind == 'ffn':
                N.call('kinet_ffn_fused', N.ptr(x), ld['ldx'], N.ptr(packed), N.ptr(f32['b1']), N.ptr(b2), N.ptr(g2), N.ptr(be2),
                       eps2, N.ptr(bufs[0]), ld['ldy'], M, D, F_, code, st)
            else:
                N.call('kinet_attn_out_ffn_fused', N.ptr(a), ld['lda'], N.ptr(r), ld['ldr'], N.ptr(packed), N.ptr(f32['bo']),
                       N.ptr(f32['g1']), N.ptr(f32['be1']), float(d['eps1']), N.ptr(f32['b1']), N.ptr(b2), N.ptr(g2), N.ptr(be2),
                       eps2, N.ptr(bufs[0]), ld['ldy'], M, D, F_, code, st)
        else:
            bufs = [torch.full((M + TAIL_ROWS, n), SENTINEL, dtype=dtype, device='cuda') for n in (F_, DB)]
            if kind == 'pair':
                N.call('kinet_bottleneck_pair', N.ptr(x), ld['ldx'], N.ptr(r), N.ptr(packed), N.ptr(f32['b3']), N.ptr(f32['b1']),
                       N.ptr(bufs[0]), N.ptr(bufs[1]), M, D, F_, DB, code, st)
            else:
                N.call('kinet_bottleneck_pair_ds', N.ptr(x), ld['ldx'], N.ptr(x0), ld['ldx0'], N.ptr(packed), N.ptr(f32['b3']),
                       N.ptr(f32['b1']), N.ptr(bufs[0]), N.ptr(bufs[1]), M, D, F_, DB, code, st)
        torch.cuda.synchronize()
        assert K.ffn_last_kernel() == kernel, f'{R.ffn_case_id(case)} cap {cap}: {K.ffn_last_kernel()} served the call, not {kernel}'
        grid = K.ffn_launch_plan(kind, M, D, F_, DB, cus)['grid']
        grids, cases = _LOG['reached'][dtype].setdefault(kernel, (set(), set()))
        grids.add((cap, grid))
        cases.add(f'F={F_} M={M}')
        if first is None:
            first = bufs
        else:
            for b, b0 in zip(bufs, first):
                assert torch.equal(b, b0), f'{R.ffn_case_id(case)}: grid cap {cap} changed the output'
    outs = {}
    for name, b, n in zip(('y',) if ffn_like else ('Y', 'T'), first, (D,) if ffn_like else (F_, DB)):
        b = b.cpu()
        assert (b[M:] == SENTINEL).all(), f'{R.ffn_case_id(case)} {name}: rows past M were written'
        assert (b[:, n:] == SENTINEL).all(), f'{R.ffn_case_id(case)} {name}: the gap columns were written'
        outs[name] = b[:M, :n]
    return outs


def _tag(case, dtype, what):
    return f'{R.ffn_case_id(case)} {_name(dtype)} {what}'


def _exact(tag, got, want64, dtype):
    """got == want64 rounded once (it is representable: test_direct_refs_cpu.py), element by element."""
    bad = got != want64.cpu().to(dtype)
    n = int(bad.sum())
    _LOG['exact_bad'] += n
    _LOG['exact_n'] += bad.numel()
    _note(tag, float(n > 0))
    print(f'{tag}: {n} of {bad.numel()} differ')
    assert n == 0, f'{tag}: {n} of {bad.numel()} elements differ from the f64 result (rows {bad.any(1).nonzero().flatten()[:8].tolist()})'


def _bounded(tag, got, ref64, tol):
    assert torch.isfinite(got.float()).all(), f'{tag}: non-finite output'
    ratio = float(((got.double() - ref64.cpu()).abs() / tol.cpu()).max())
    _note(tag, ratio)
    print(f'{tag}: worst err / bound {ratio:.3f}')
    assert ratio <= 1.0, f'{tag}: err / bound = {ratio}'


CASES = pytest.mark.parametrize('case', R.FFN_DIRECT_CASES, ids=R.ffn_case_id)
FFN_LIKE = pytest.mark.parametrize('case', [c for c in R.FFN_DIRECT_CASES if c[0] in ('ffn', 'attn_out_ffn')], ids=R.ffn_case_id)
DTYPES = pytest.mark.parametrize('dtype', [BF16, F16], ids=_name)


@DTYPES
@CASES
def test_exact(K, knobs, case, dtype):
    d = R.ffn_direct_inputs(case, 'exact')
    got = _run(K, knobs, case, d, dtype)
    ref = R.ffn_direct_ref(case, d, dtype, dev='cuda')
    for name, want in R.ffn_direct_outputs(case, ref).items():
        _exact(_tag(case, dtype, f'exact {name}'), got[name], want, dtype)


@DTYPES
@FFN_LIKE
def test_exact_operands_layernorm(K, knobs, case, dtype):
    d = R.ffn_direct_inputs(case, 'exact')
    for offset in OFFSETS:
        got = _run(K, knobs, case, d, dtype, ln=True, offset=offset)
        ref = R.ffn_direct_ref(case, d, dtype, ln=True, offset=offset, dev='cuda')
        y, tol = R.ffn_ln_tol(ref['pre'], d['ln'], dtype)
        _bounded(_tag(case, dtype, f'LN +{offset:g}'), got['y'], y, tol)


@DTYPES
@CASES
def test_generic(K, knobs, case, dtype):
    ln = case[0] == 'ffn' and case[2] in (64, 2048)
    d = R.ffn_direct_inputs(case, 'generic', dtype)
    got = _run(K, knobs, case, d, dtype, ln=ln)
    ref = R.ffn_direct_ref(case, d, dtype, ln=ln, dev='cuda')
    tol = R.ffn_direct_generic_tol(case, d, ref, dtype, ln)
    for name, want in R.ffn_direct_outputs(case, ref).items():
        _bounded(_tag(case, dtype, f'generic{" LN" if ln else ""} {name}'), got[name], want, tol[name])


# one row per entry point: the smallest with more than one hidden chunk
SELF_CASES = [next(c for c in R.FFN_DIRECT_CASES if c[0] == kind and c[2] != 32) for kind in R.FFN_KINDS_]


@pytest.mark.parametrize('case', SELF_CASES, ids=R.ffn_case_id)
def test_resolution_self_check(K, knobs, case):
    """One non-zero weight of each GEMM in turn is zeroed in what is packed, not in the reference: the exact
    comparison must report mismatches, in exactly the rows a reference with that weight zeroed predicts."""
    d = R.ffn_direct_inputs(case, 'exact')
    ref = R.ffn_direct_ref(case, d, BF16, dev='cuda')
    want = {k: R.rnd(v, BF16).cpu() for k, v in R.ffn_direct_outputs(case, ref).items()}
    for gi, key in enumerate(R.ffn_direct_gemms(case)):
        g = torch.Generator().manual_seed(17 + gi)
        nz = (d[key] != 0).nonzero()
        row, col = nz[int(torch.randint(0, nz.shape[0], (1,), generator=g))].tolist()
        got = _run(K, knobs, case, d, BF16, zero=(key, row, col))
        d2 = dict(d)
        d2[key] = d[key].clone()
        d2[key][row, col] = 0
        ref2 = R.ffn_direct_ref(case, d2, BF16, dev='cuda')
        pred = {k: R.rnd(v, BF16).cpu() for k, v in R.ffn_direct_outputs(case, ref2).items()}
        rows_pred = sorted(set().union(*[(pred[k] != want[k]).any(1).nonzero().flatten().tolist() for k in want]))
        rows_got = sorted(set().union(*[(got[k].double() != want[k]).any(1).nonzero().flatten().tolist() for k in want]))
        _LOG['self'].append(f'{R.ffn_case_id(case)} {key}[{row}, {col}]: {len(rows_got)} rows differ, {len(rows_pred)} predicted')
        assert rows_pred, f'{key}[{row}, {col}]: the reference itself does not resolve this weight'
        assert rows_got == rows_pred, f'{key}[{row}, {col}]: rows {rows_got[:8]} differ, predicted {rows_pred[:8]}'
        if key == 'Wo':      # LayerNorm1's row is no longer +-1: x is generic there, and may round either way
            continue
        for k in want:
            assert torch.equal(got[k].double(), pred[k]), f'{key}[{row}, {col}]: {k} is not the reference with that weight zeroed'


def test_grid_cap_returns_the_previous_value(K, knobs):
    assert K.ffn_grid_cap(1000) == 0 and K.ffn_grid_cap(-3) == 1000 and K.ffn_grid_cap(0) == 0


def test_every_kernel_was_reached():
    """Closing test: over the module, every instantiation of the table ran in bf16 and in f16."""
    for dt in (BF16, F16):
        assert set(_LOG['reached'][dt]) == set(R.FFN_KERNELS), _name(dt)
