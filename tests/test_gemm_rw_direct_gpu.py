"""Direct tests of the resident-weight GEMM (csrc/gemm_rw.hip gemm_rw_kernel), variant by variant,
against f64 references (tests/direct_refs.py, checked on the CPU by test_direct_refs_cpu.py).

Every case sets flag 8 (the resident-weight kernel from M >= 256) and asserts through
kinet_gemm_rw_last_config the whole instantiation and grid it expects -- KC, NT, BMR, NS, NW, OCC, HAS_R,
LN, HAS_A2, CR, PREP, the output element size, P, ng, n_mtiles.  The expectations are the literal
tables RW_CASES / RW_HM_CASES / RW_CONV_CASES / PREP_CASES of direct_refs.py, written down from reading
the launch rules (now rw_plan and kRwVariants of csrc/gemm_rw_plan.h) and the LDS geometry; nothing in
them comes from the library.  On a machine without a GPU test_gemm_rw_plan_cpu.py checks every row of
them, under every grid cap used here, against the library's planner (kinet_gemm_rw_plan), and
test_direct_refs_cpu.py their shapes, flags and field names.

Shapes: 17 row tiles with a ragged last one (M = 17 * BMR - 5), run under kinet_gemm_rw_grid_cap 0, 1, 3
and 16: one tile per workgroup; one workgroup walking all 17 through its NS <= 4 ring slots; 6 / 6 / 5
tiles; one workgroup with two tiles next to fifteen with one.  The four outputs must be bit-identical
(sentinel rows and gap columns included) and the first is compared with the reference.

Two operand classes as for the tiled kernel: EXACT (the f64 result rounded once, compared for
equality, exact_headroom asserted) and GENERIC (gemm_generic_bound).  LayerNorm rows take exact matrix
operands and test_ln_epilogue_direct_gpu.py's bound at both of its offsets.

The row mask covers a first row, a tile's first and last row, a whole tile and the last ragged row; the
last one is the case of the mask DMA's dword that straddles the end of the mask (DESIGN.md,
profiles/gemm_rw_mask_fix_ab.txt).

Every output is a view of a sentinel-filled buffer: rows below M, gap columns (ldc > N), the third image of
the conv cases and the elements before and after a head-major output's planes must keep the sentinel.

A limit of the record: the LDS-transposed store of 32-column heads is chosen inside the kernel from a
run-time argument (hm_tr, cleared by flag 1073741824), not by the instantiation, so 'hm32 transpose' and
'hm32 direct' assert the same configuration; a launch that fell back from the transpose to the direct
store would pass here (both must give the exact result) and show only in the kernel's time.

kernels.linear expands a shorter x_add to x's rows, so the a2_rows period of the load-time add cannot
be expressed through it; the case here goes through kernels.offsets_proj_headmajor, which can.

KINET_GEMM_RW_LOG names a file that receives the module's figures (profiles/gemm_rw_direct.log)."""
import os
import time

import pytest
import torch

import direct_refs as R
from test_ln_epilogue_direct_gpu import EPS, OFFSETS

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
SENTINEL = 77.0
RW = 8                      # the resident-weight kernel from M >= 256
TAIL_ROWS = 32              # sentinel rows below the output
HM_PAD = 64                 # sentinel elements before and after a head-major output's planes

_LOG = {'t0': None, 'worst': {}, 'exact_bad': 0, 'exact_n': 0, 'configs': {}}


def _name(dt):
    return str(dt).replace('torch.', '')


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


@pytest.fixture(scope='module', autouse=True)
def _report():
    _LOG['t0'] = time.time()       # the module's own wall time: from its first test, not from collection
    yield
    lines = [f'module wall time: {time.time() - _LOG["t0"]:.1f} s',
             f'exact class: {_LOG["exact_bad"]} of {_LOG["exact_n"]} elements not equal to the expected value',
             f'configurations reached ({len(_LOG["configs"])}), as KC NT BMR NS NW OCC HAS_R LN HAS_A2 CR PREP out_bytes '
             '| ng | grids P: variants']
    for key, (ps, names) in sorted(_LOG['configs'].items()):
        lines.append('  ' + ' '.join(map(str, key[:12])) + f' | {key[12]} | {sorted(ps)}: ' + ', '.join(sorted(names)))
    lines.append('worst err / bound per variant (exact class: 0 = every element equal):')
    lines += [f'  {k}: {v:.3f}' for k, v in sorted(_LOG['worst'].items())]
    print('\n'.join(lines))
    path = os.environ.get('KINET_GEMM_RW_LOG')
    if path:
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


@pytest.fixture
def knobs(K):
    """set_flags / the grid cap for one test, restored (flags 0, cap 0) afterwards."""
    from kinet_amd import _native

    class Knobs:
        @staticmethod
        def flags(v):
            _native.lib().kinet_gemm_set_flags(v)

        @staticmethod
        def cap(v):
            K.gemm_rw_grid_cap(v)
    yield Knobs
    _native.lib().kinet_gemm_set_flags(0)
    K.gemm_rw_grid_cap(0)


def _ran(K, name, family, expected):
    fam = K.gemm_last_kernel()
    assert fam == (family, 0, 0), f'{name}: {fam} served the call, not {family}'
    got = K.gemm_rw_last_config()
    assert got == expected, f'{name}: launched {got}, expected {expected}'
    key = tuple(got[f] for f in R.RW_CONFIG_FIELDS[:12]) + (got['ng'],)
    ps, names = _LOG['configs'].setdefault(key, (set(), set()))
    ps.add(got['P'])
    names.add(name)


def _note(name, ratio):
    _LOG['worst'][name] = max(_LOG['worst'].get(name, 0.0), ratio)


def _exact(name, what, got, want64, scale, odt):
    assert R.exact_headroom(want64, scale, odt).all(), f'{name} {what}: the case cannot resolve one dropped product'
    bad = int((got != want64.to(odt)).sum())
    _LOG['exact_bad'] += bad
    _LOG['exact_n'] += want64.numel()
    _note(name, float(bad > 0))
    print(f'{name} {what} exact: {bad} of {want64.numel()} differ')
    assert bad == 0, f'{name} {what}: {bad} of {want64.numel()} elements differ from the f64 result rounded once'


def _same_under_caps(name, run, tiles=R.RW_TILES):
    """run(cap) -> the whole output buffer; bit-identical for every cap.  Returns the cap-0 buffer."""
    caps = {0: tiles, 1: 1, 3: 3, tiles - 1: tiles - 1}
    assert tiles != R.RW_TILES or caps == R.RW_CAPS
    first = None
    for cap in caps:
        buf = run(cap)
        torch.cuda.synchronize()
        if first is None:
            first = buf
        else:
            assert torch.equal(buf, first), f'{name}: grid cap {cap} changed the output'
    return first


# ------------------------------------------------------------------------ the GEMM variants
def _linear(K, knobs, case, cls, offset=0.0):
    name, Kd, N, flags, _, cdt, odt, cfg, ng = case
    o = R.rw_opts(case)
    M = R.rw_rows(cfg[2])
    inp = R.rw_inputs(case, cls, offset)
    dev = {k: inp[k].cuda() for k in ('scale', 'bias', 'mask') if inp[k] is not None}
    x, w = inp['x'].to(cdt).cuda(), inp['w'].to(cdt).cuda()
    kw = dict(bias=dev.get('bias'), scale=dev.get('scale'), relu=inp['relu'], row_mask=dev.get('mask'), out_dtype=odt)
    if inp['x2'] is not None:
        kw['x_add'] = inp['x2'].to(cdt).cuda()
    if inp['res'] is not None:
        rbuf = torch.full((M, N + (8 if 'Rld' in o else 0)), SENTINEL, dtype=odt).cuda()
        rbuf[:, :N] = inp['res'].to(odt).cuda()
        kw['residual'] = rbuf[:, :N]
    if inp['ln'] is not None:
        kw['ln'] = (inp['ln'][0].cuda(), inp['ln'][1].cuda(), EPS)
    ldc = N + (8 if 'ld' in o else 0)
    knobs.flags(RW | flags)

    def run(cap):
        knobs.cap(cap)
        buf = torch.full((M + TAIL_ROWS, ldc), SENTINEL, dtype=odt).cuda()
        K.linear(x, w, out=buf[:M, :N], **kw)
        _ran(K, name, 'rw', R.rw_expected(cfg, ng, 'R' in o, 'LN' in o, 'A2' in o, odt, cap))
        return buf
    buf = _same_under_caps(name, run).cpu()
    assert (buf[M:] == SENTINEL).all(), f'{name}: rows past M were written'
    assert (buf[:, N:] == SENTINEL).all(), f'{name}: the gap columns were written'
    return buf[:M, :N], inp


PLAIN = [c for c in R.RW_CASES if 'LN' not in R.rw_opts(c)]
WITH_LN = [c for c in R.RW_CASES if 'LN' in R.rw_opts(c)]


@pytest.mark.parametrize('cls', ['exact', 'generic'])
@pytest.mark.parametrize('case', PLAIN, ids=lambda c: c[0].replace(' ', '_'))
def test_rw_variant(K, knobs, case, cls):
    name, Kd, odt = case[0], case[1], case[6]
    got, inp = _linear(K, knobs, case, cls)
    want = R.rw_masked(inp['pre'], inp['mask'])
    if cls == 'exact':
        _exact(name, f'({got.shape[0]}, {case[2]}, {Kd}) {_name(case[5])}->{_name(odt)}', got, want, inp['scale'], odt)
    else:
        ratio = R.rw_generic_ratio(got, inp, Kd, odt)
        _note(name + ' generic', ratio)
        print(f'{name} generic: worst err / bound {ratio:.3f}')
        assert ratio <= 1.0, f'{name}: err / bound = {ratio}'


@pytest.mark.parametrize('offset', OFFSETS)
@pytest.mark.parametrize('case', WITH_LN, ids=lambda c: c[0].replace(' ', '_'))
def test_rw_variant_ln(K, knobs, case, offset):
    name, odt = case[0], case[6]
    got, inp = _linear(K, knobs, case, 'exact', offset)
    assert torch.isfinite(got.float()).all()
    ratio, bad = R.rw_ln_check(got, inp, odt, EPS)
    _note(f'{name} +{offset:g}', ratio)
    print(f'{name} +{offset:g}: worst err / bound {ratio:.3f}')
    assert bad == 0, f'{name} +{offset:g}: {bad} elements over the bound, worst err / bound {ratio}'
    if inp['mask'] is not None:
        assert (got[inp['mask']] == 0).all()


# ------------------------------------------------------------------------ head-major stores
@pytest.mark.parametrize('case', R.RW_HM_CASES, ids=lambda c: c[0].replace(' ', '_'))
def test_rw_headmajor(K, knobs, case):
    """value_proj_headmajor / value_proj_headmajor_split against the permuted f64 result, exact class,
    with a row mask; the 32-column heads through the LDS transpose and (flag 1073741824) without it."""
    name, d, hd, flags, cdt, odt, cfg, ng = case
    B, S = R.rw_hm_batch(cfg[2])
    M = B * S
    assert M == R.rw_rows(cfg[2])
    g = torch.Generator().manual_seed(d + cfg[2] + len(name))
    x, w, acc, _ = R.gemm_case(M, d, d, cdt, 'exact')
    bias = R.exact_epilogue(d, g)[1]
    mask = R.rw_mask(M, cfg[2])
    xc, wc, bc, mc = x.to(cdt).cuda().view(B, S, d), w.to(cdt).cuda(), bias.cuda(), mask.cuda().view(B, S)
    if hd == 'split':
        ws, bs = K.split_value_weights(wc, bc, 8)
    knobs.flags(RW | flags)

    h = 36 if hd == 'split' else hd

    def run(cap):
        knobs.cap(cap)
        buf = torch.full((HM_PAD + M * d + HM_PAD,), SENTINEL, dtype=odt).cuda()
        if hd == 'split':
            K.value_proj_headmajor_split(xc, ws, bs, 8, row_mask=mc, out_dtype=odt, out=buf[HM_PAD:HM_PAD + M * d])
        else:
            K.value_proj_headmajor(xc, wc, bc, hd, row_mask=mc, out_dtype=odt,
                                   out=buf[HM_PAD:HM_PAD + M * d].view(d // h, B, S, h))
        _ran(K, name, 'rw', R.rw_expected(cfg, ng, False, False, False, odt, cap))
        return buf
    buf = _same_under_caps(name, run).cpu()
    assert (buf[:HM_PAD] == SENTINEL).all() and (buf[HM_PAD + M * d:] == SENTINEL).all(), f'{name}: wrote outside the planes'
    y = buf[HM_PAD:HM_PAD + M * d]
    if hd == 'split':      # the planes as SplitValue.merged() joins them: (heads, B, S, 32 | 4)
        y = torch.cat([y[:8 * M * 32].view(8, B, S, 32), y[8 * M * 32:].view(8, B, S, 4)], -1)
    else:
        y = y.view(d // h, B, S, h)
    want = R.rw_masked(R.epilogue64(acc, None, bias)[0], mask)
    _exact(name, f'd={d} hd={hd} {_name(cdt)}->{_name(odt)}', R.rw_hm_rows(y), want, None, odt)


@pytest.mark.parametrize('Kd,cfg,ng', [(256, (8, 4, 16, 4, 4, 2), 2), (288, (9, 3, 16, 4, 8, 1), 1)])
def test_rw_a2_period(K, knobs, Kd, cfg, ng):
    """The load-time add with an A2 of a2_rows = 89 rows (one frame's operand shared by 3 frames): 16-row
    tiles straddle the period's end.  offsets_proj_headmajor, 8 heads x 48 columns, exact class."""
    B, Lq, heads = 3, 89, 8
    M, N = B * Lq, heads * 48
    name = f'A2 period 89 k{Kd}'
    g = torch.Generator().manual_seed(Kd)
    x, w, _, _ = R.gemm_case(M, N, Kd, BF16, 'exact')
    x2 = R.exact_x((1, Lq, Kd), g)
    bias = R.exact_epilogue(N, g)[1]
    a = (x.view(B, Lq, Kd) + x2).reshape(M, Kd).double()
    want = a @ w.double().T + bias.double()
    xc, wc, pc, bc = x.bfloat16().cuda().view(B, Lq, Kd), w.bfloat16().cuda(), x2.bfloat16().cuda(), bias.cuda()
    knobs.flags(RW)

    def run(cap):
        knobs.cap(cap)
        buf = torch.full((HM_PAD + M * N + HM_PAD,), SENTINEL, dtype=F16).cuda()
        K.offsets_proj_headmajor(xc, wc, bc, heads, x_add=pc, out_dtype=F16, out=buf[HM_PAD:HM_PAD + M * N].view(heads, B, Lq, 48))
        _ran(K, name, 'rw', R.rw_expected(cfg, ng, False, False, True, F16, cap))
        return buf
    buf = _same_under_caps(name, run).cpu()
    assert (buf[:HM_PAD] == SENTINEL).all() and (buf[HM_PAD + M * N:] == SENTINEL).all(), f'{name}: wrote outside the planes'
    _exact(name, f'({M}, {N}, {Kd})', R.rw_hm_rows(buf[HM_PAD:HM_PAD + M * N].view(heads, B, Lq, 48)), want, None, F16)


# ------------------------------------------------------------------ conv-row mode (family 5)
@pytest.mark.parametrize('cls', ['exact', 'generic'])
@pytest.mark.parametrize('cdt', [BF16, F16], ids=_name)
@pytest.mark.parametrize('case', R.RW_CONV_CASES, ids=lambda c: c[0].replace(' ', '_'))
def test_rw_conv_rows(K, knobs, case, cdt, cls):
    name, (KH, Cin, Cout, stride, pad_h, Hin, Win), flags, opts, cfg, ng = case
    x, w, scale, bias, acc, ap = R.rw_conv_inputs(name, cdt, cls)
    B, M, Wo = R.RW_CONV_BATCH, R.RW_CONV_ROWS, 33
    Ho = M // (B * Wo)
    tiles = -(-M // cfg[2])
    relu = 'relu' in opts.split()
    xc, wc = x.to(cdt).cuda(), w.to(cdt).cuda()
    sc, bc = (None if t is None else t.cuda() for t in (scale, bias))
    st, pd = (stride[0], pad_h) if stride[0] == stride[1] else (stride, (pad_h, 0))
    knobs.flags(RW | flags)

    def run(cap):
        knobs.cap(cap)
        buf = torch.full((B + 1, Ho, Wo, Cout + 8), SENTINEL, dtype=cdt).cuda()     # a third image: the tail rows
        K.conv2d_nhwc(xc, wc, st, pd, scale=sc, bias=bc, relu=relu, out=buf[:B, ..., :Cout], ksplit=1 if isinstance(st, int) else None)
        _ran(K, name, 'rw_conv', R.rw_expected(cfg, ng, False, False, False, cdt, cap, cr=1, tiles=tiles))
        return buf
    buf = _same_under_caps(name, run, tiles).cpu()
    assert (buf[B:] == SENTINEL).all(), f'{name}: rows past M were written'
    assert (buf[..., Cout:] == SENTINEL).all(), f'{name}: the gap columns were written'
    got = buf[:B, ..., :Cout].reshape(M, Cout)
    pre, maj = R.epilogue64(acc, scale, bias, None, relu)
    tag = f'conv {name} {_name(cdt)}'
    if cls == 'exact':
        _exact(tag, '', got, pre, scale, cdt)
        if KH == 3:
            # output rows 0 and 3 of either image lie wholly in the vertical padding
            border = R.epilogue64(torch.zeros_like(acc), scale, bias, None, relu)[0].to(cdt).view(B, Ho, Wo, Cout)
            assert (acc.view(B, Ho, Wo, Cout)[:, [0, 3]] == 0).all()
            assert torch.equal(got.view(B, Ho, Wo, Cout)[:, [0, 3]], border[:, [0, 3]])
    else:
        ratio = float(((got.double() - pre).abs() / R.gemm_generic_bound(ap, KH * Cin, maj, pre, cdt, scale)).max())
        _note(tag + ' generic', ratio)
        print(f'{tag} generic: worst err / bound {ratio:.3f}')
        assert ratio <= 1.0, f'{tag}: err / bound = {ratio}'


# ----------------------------------------------------------------- sampling records (PREP)
@pytest.mark.parametrize('dtype', [BF16, F16], ids=_name)
@pytest.mark.parametrize('case', R.PREP_CASES, ids=lambda c: c[0].replace(' ', '_'))
def test_rw_records_same_under_caps(K, knobs, case, dtype):
    """kinet_msda_sample_records has its oracle test (test_msda_gpu.py); here: the records are
    bit-identical however the 17 row tiles are spread over workgroups."""
    name, flags, add, cfg, ng = case
    B, Lq, heads = 3, 89, 8
    shapes = ((12, 10), (6, 5), (3, 3), (2, 2))
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, Lq, 256, generator=g).to(dtype).cuda()
    pos = (0.5 * torch.randn(B, Lq, 256, generator=g)).to(dtype).cuda() if add else None
    w = (torch.randn(heads * 48, 256, generator=g) / 16).to(dtype).cuda()
    bias = torch.randn(heads * 48, generator=g).cuda()
    ref = torch.rand(B, Lq, 4, 2, generator=g).cuda()
    qmask = R.rw_mask(B * Lq, 16).view(B, Lq).cuda()
    knobs.flags(flags)

    def run(cap):
        knobs.cap(cap)
        rec, _ = K.msda_sample_records(x, w, bias, heads, ref, shapes, x_add=pos, query_attn_mask=qmask)
        got = K.gemm_rw_last_config()
        want = R.rw_expected(cfg, ng, False, False, add, F16, cap, prep=1)
        assert got == want, f'{name}: launched {got}, expected {want}'
        key = tuple(got[f] for f in R.RW_CONFIG_FIELDS[:12]) + (got['ng'],)
        _LOG['configs'].setdefault(key, (set(), set()))[0].add(got['P'])
        _LOG['configs'][key][1].add(name)
        return rec
    rec = _same_under_caps(name, run, tiles=17)
    assert rec.shape == (heads, B, Lq, 24)


# ------------------------------------------------------ the record itself, and the cap's range
def test_rw_last_config_cleared_by_other_families(K, knobs):
    x, w = torch.ones(300, 64, dtype=BF16, device='cuda'), torch.ones(64, 64, dtype=BF16, device='cuda')
    knobs.flags(RW)
    assert (K.linear(x, w) == 64).all()
    assert K.gemm_last_kernel()[0] == 'rw' and K.gemm_rw_last_config()['KC'] == 2
    knobs.flags(4)
    assert (K.linear(x, w) == 64).all()
    assert K.gemm_last_kernel()[0] == 'tiled' and set(K.gemm_rw_last_config().values()) == {0}
    # a cap above the launcher's own P changes nothing; the previous value comes back
    knobs.flags(RW)
    assert K.gemm_rw_grid_cap(1000) == 0
    K.linear(x, w)
    assert K.gemm_rw_last_config()['P'] == K.gemm_rw_last_config()['n_mtiles'] == 10
    assert K.gemm_rw_grid_cap(0) == 1000
