"""The MSDA forward sampling kernels (csrc/msda.hip: msda_fwd_kernel, msda_fused_kernel,
msda_fused_fast_kernel; csrc/msda_enc.hip: msda_enc_kernel behind its three front ends), each against
direct_refs.msda_prep_ref -> direct_refs.msda_sample_ref: plain torch f64 from the raw offsets, logits,
reference points and mask.  Nothing a kernel reports is fed back into a reference.

Two operand classes per path (direct_refs.msda_addr_case / msda_generic_case):
  addressing  integer values, a softmax that is exactly (1, 0, ..., 0), the hot tap on a pixel centre or a
              cell corner chosen from the strip plan (staged / far / window edges / the rows and columns
              around the level).  Records front end: equality.  Offsets front ends: msda_addr_bound.
  generic     random operands under direct_refs.msda_bound, per element, from the reference's magnitudes.
Every case asserts which kernel served it (kernels.msda_fused_last_kernel) and, on the strip kernel, the
plan (direct_refs.MSDA_ENC_CASES, strips forced through msda_encoder_set_strips).  What this module cannot
see is which of the far and common branches a wave took: only the constructed sample counts stand for it.

KINET_MSDA_DIRECT_LOG names a file that receives the module's figures (profiles/msda_direct.log)."""
import os
import time

import numpy as np
import pytest
import torch

import direct_refs as R

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
SENTINEL, PAD = 77.0, 64
_LOG = {'t0': None, 'worst': {}, 'eq_bad': 0, 'eq_n': 0, 'reached': {}, 'counts': {}}


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


@pytest.fixture(scope='module', autouse=True)
def _report():
    _LOG['t0'] = time.time()
    yield
    lines = [f'module wall time: {time.time() - _LOG["t0"]:.1f} s',
             f'equality class (records): {_LOG["eq_bad"]} of {_LOG["eq_n"]} elements differ',
             'kernels and plans reached (kernel: cases):']
    lines += [f'  {k}: {", ".join(sorted(v))}' for k, v in sorted(_LOG['reached'].items(), key=str)]
    lines.append('fewest hot samples per staged level, by category (addressing class, from the f64 locations):')
    lines += [f'  {k}: {v}' for k, v in sorted(_LOG['counts'].items())]
    lines.append('worst err / bound per path:')
    lines += [f'  {k}: {v:.3f}' for k, v in sorted(_LOG['worst'].items())]
    print('\n'.join(lines))
    path = os.environ.get('KINET_MSDA_DIRECT_LOG')
    if path:
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


@pytest.fixture
def strips(K):
    old = K.msda_encoder_set_strips(0)
    yield K.msda_encoder_set_strips
    K.msda_encoder_set_strips(old)


def _ran(K, name, want):
    got = K.msda_fused_last_kernel()
    assert got == want, f'{name}: {got} served the call, not {want}'
    _LOG['reached'].setdefault(want, set()).add(name)


def _check(name, out, ref64, bound):
    ratio = ((out.double().cpu() - ref64).abs() / bound).max().item()
    _LOG['worst'][name] = max(_LOG['worst'].get(name, 0.0), ratio)
    print(f'{name}: worst err / bound {ratio:.3f}')
    assert ratio <= 1.0, f'{name}: err / bound = {ratio}'


class Sent:
    """n outputs of `shape` inside one sentinel-filled buffer: PAD elements before, between and after."""

    def __init__(self, n, shape, dtype):
        numel = int(np.prod(shape))
        self.step = (numel + PAD + 7) // 8 * 8
        self.buf = torch.full((PAD + n * self.step,), SENTINEL, dtype=dtype, device='cuda')
        self.outs = [self.buf[PAD + i * self.step: PAD + i * self.step + numel].view(*shape) for i in range(n)]
        self.numel = numel

    def intact(self):
        ok = bool((self.buf[:PAD] == SENTINEL).all())
        for i in range(len(self.outs)):
            ok = ok and bool((self.buf[PAD + i * self.step + self.numel: PAD + (i + 1) * self.step] == SENTINEL).all())
        return ok


def _hm(value, dtype):
    """(B, S, M, D) -> head-major (M, B, S, D) on the GPU."""
    return value.to(dtype).permute(2, 0, 1, 3).contiguous().cuda()


def _orders(K, shapes, Lq, seed=0):
    """natural, the encoder's row-sorted order (Lq = S), a random permutation."""
    nt = (Lq + 15) // 16
    g = torch.Generator().manual_seed(seed + nt)
    out = [None, torch.randperm(nt, generator=g).int().cuda()]
    if Lq == sum(h * w for h, w in shapes):
        out.insert(1, K.encoder_tile_order(shapes, torch.device('cuda', torch.cuda.current_device())))
    return out


# ------------------------------------------------------------------ plain forward (C-ABI module)
@pytest.mark.parametrize('dtype', [F32, BF16, F16])
@pytest.mark.parametrize('cls', ['addr', 'generic'])
def test_plain_forward(cls, dtype):
    """msda_fwd_kernel (kinet_msda_forward), locations and attention weights given in f32: f32 tap weights
    and accumulation, c_acc = 67 * 2^-24; the location error is the kernel's y H - 0.5 (2 of LOC_OPS)."""
    import kinet_amd  # noqa: F401
    import MultiScaleDeformableAttention as MSDA
    shapes, B, M, Lq = R.MSDA_ENC_GEO['all'], 2, 8, 1001 if cls == 'addr' else 177
    case = R.msda_addr_case(shapes, B, M, Lq, 2) if cls == 'addr' else \
        R.msda_generic_case(shapes, B, M, Lq, 2, 3.0, 'randn', dtype, masked=False)
    prep, _ = R.msda_chain_ref(case, shapes, M)
    loc, aw = prep['loc'].float(), prep['attw'].float()
    samp = R.msda_sample_ref(case['value'], shapes, loc.double(), aw.double())
    ss = torch.tensor(shapes, dtype=torch.int64).cuda()
    out = MSDA.ms_deform_attn_forward(case['value'].to(dtype).cuda(), ss, loc.cuda(), aw.cuda(), 64)
    torch.cuda.synchronize()
    assert out.dtype == dtype
    if cls == 'addr':
        cnt = R.msda_addr_counts(case, loc.double(), shapes)
        assert min(cnt.values()) >= 200, cnt
        bound = R.msda_addr_bound(samp, shapes, 'f32', loc.double().abs())
        assert bound.max().item() < 0.125
    else:
        bound = R.msda_bound(samp, shapes, 'f32', dtype, loc.double().abs())
    _check(f'plain {cls} {dtype}', out, samp['out'], bound)


# ------------------------------------------------------------------ fused kernels
def _fused(K, case, shapes, M, vdt, odt=None, oldt=F32, order=None, out=None, want=False, head_major=True):
    L = len(shapes)
    ss = torch.tensor(shapes, dtype=torch.int64).cuda()
    v = _hm(case['value'], vdt) if head_major else case['value'].to(vdt).flatten(2).cuda()
    qm = case.get('qmask')
    return K.msda_fused(v, ss, case['offlog'].to(oldt).cuda(), case['refs'].cuda(), M, L, 4,
                        qm.cuda() if qm is not None else None, want_loc_attw=want, head_major=head_major,
                        out_dtype=odt, query_tile_order=order, out=out)


def _loc_attw_ok(name, prep, loc, aw, extra):
    """want_loc_attw against msda_prep_ref under its own bounds (+ `extra` roundings: the fast kernel
    multiplies by reciprocals where the generic one divides)."""
    dl = (loc.double().cpu() - prep['loc']).abs()
    assert (dl <= (prep['loc_c'] + extra) * R.U32 * prep['locA']).all(), (name, dl.max().item())
    da = (aw.double().cpu() - prep['attw']).abs()
    assert (da <= (prep['attw_c'] + extra) * R.U32 * prep['attw'] + R.F32_TINY).all(), (name, da.max().item())


@pytest.mark.parametrize('vdt,D,vec,head_major', [(F32, 3, 1, True), (F32, 6, 2, False), (F32, 36, 4, True),
                                                  (F16, 24, 8, True), (BF16, 36, 4, False)])
@pytest.mark.parametrize('cls', ['addr', 'generic'])
def test_generic_fused(K, cls, vdt, D, vec, head_major):
    """msda_fused_kernel at vector widths 1, 2, 4 and 8 (M = 5: the second head group of a workgroup is
    partial; Lq = 37 is no multiple of any queries-per-wave): f32 weights and accumulation, c_acc = 67 * 2^-24."""
    shapes, B, M, Lq = R.MSDA_ENC_GEO['all'], 3, 5, 37 if cls == 'generic' else 533
    rd = 2 if D != 6 else 4
    case = R.msda_addr_case(shapes, B, M, Lq, rd, D=D) if cls == 'addr' else \
        R.msda_generic_case(shapes, B, M, Lq, rd, 3.0, 'pm8' if D == 3 else 'randn', vdt, D=D)
    prep, samp = R.msda_chain_ref(case, shapes, M)
    name = f'generic-fused vec{vec} {cls}'
    s = Sent(1, (B, Lq, M * D), vdt)
    out, loc, aw = _fused(K, case, shapes, M, vdt, want=True, out=s.outs[0], head_major=head_major)
    torch.cuda.synchronize()
    _ran(K, name, ('generic', vec))
    assert s.intact()
    if cls == 'addr':
        cnt = R.msda_addr_counts(case, prep['loc'], shapes)
        assert min(cnt.values()) >= 200, cnt
        bound = R.msda_addr_bound(samp, shapes, 'f32', prep['locA'])
        assert bound.max().item() < 0.125
    else:
        bound = R.msda_bound(samp, shapes, 'f32', vdt, prep['locA'], prep['attw_c'])
        assert (out[case['qmask'].cuda()] == 0).all()
        _loc_attw_ok(name, prep, loc, aw, 0)
    _check(name, out, samp['out'], bound)


FAST = [  # L, M, B, Lq, ref_dim, value, output, offsets / logits
    (4, 3, 1, 1, 2, BF16, BF16, F32), (4, 3, 3, 15, 4, F16, F16, F32), (4, 8, 1, 17, 2, F16, BF16, F16),
    (4, 3, 3, 1009, 2, BF16, BF16, F16), (4, 8, 1, 1009, 4, F16, F16, F16),
    (8, 8, 1, 1009, 2, BF16, BF16, F32), (8, 3, 3, 17, 4, F16, BF16, F16), (8, 5, 1, 1, 2, F16, F16, F32),
]


@pytest.mark.parametrize('L,M,B,Lq,rd,vdt,odt,oldt', FAST)
@pytest.mark.parametrize('cls', ['addr', 'generic'])
def test_fast_fused(K, cls, L, M, B, Lq, rd, vdt, odt, oldt):
    """msda_fused_fast_kernel, L = 4 (two heads per workgroup: M = 3 leaves the second one half empty) and
    L = 8: f32 location and weight arithmetic, the weight rounded to f16 (c_acc = 67 * 2^-24 + 2^-11), f32
    accumulation.  Tile order: natural and a random permutation, bit-identical."""
    shapes = R.MSDA_ENC_GEO['all'] * (L // 4)
    f16ol = oldt == F16
    case = R.msda_addr_case(shapes, B, M, Lq, rd) if cls == 'addr' else \
        R.msda_generic_case(shapes, B, M, Lq, rd, (0.5, 3.0, 25.0)[Lq % 3], 'pm8' if M == 8 else 'randn', vdt,
                            f16_offlog=f16ol)
    prep, samp = R.msda_chain_ref(case, shapes, M)
    name = f'fast L{L} {cls}'
    orders = _orders(K, shapes, Lq)
    s = Sent(len(orders), (B, Lq, M * 32), odt)
    res = [_fused(K, case, shapes, M, vdt, odt, oldt, order=o, out=s.outs[i], want=True) for i, o in enumerate(orders)]
    torch.cuda.synchronize()
    _ran(K, name, ('fast', L))
    assert s.intact()
    out, loc, aw = res[0]
    for o2, l2, a2 in res[1:]:
        assert torch.equal(out, o2) and torch.equal(loc, l2) and torch.equal(aw, a2)
    if cls == 'addr':
        if B * Lq * M >= 8000:
            cnt = R.msda_addr_counts(case, prep['loc'], shapes)
            assert min(cnt.values()) >= 200 // (L // 4), cnt
        bound = R.msda_addr_bound(samp, shapes, 'fast', prep['locA'])
        assert bound.max().item() < 0.125
    else:
        bound = R.msda_bound(samp, shapes, 'fast', odt, prep['locA'], prep['attw_c'])
        assert (out[case['qmask'].cuda()] == 0).all()
        _loc_attw_ok(name, prep, loc, aw, 2)
    _check(name, out, samp['out'], bound)


# ------------------------------------------------------------------ the strip kernel
ENC = [  # geometry, B, M, channels, forced strips, ref_dim, masked, output, noise, logits
    ('all', 1, 8, 32, 1, 2, True, BF16, 3.0, 'randn'), ('all', 1, 8, 32, 2, 4, False, F16, 25.0, 'randn'),
    ('all', 1, 8, 32, 3, 2, True, F16, 25.0, 'pm8'), ('all', 3, 8, 32, 3, 2, False, BF16, 0.5, 'randn'),
    ('all', 2, 5, 32, 3, 2, True, BF16, 3.0, 'pm8'),                 # 30 workgroups: no multiple of 8
    ('all', 1, 8, 32, 0, 2, True, F16, 3.0, 'randn'),
    ('wide1', 1, 8, 32, 0, 2, True, F16, 3.0, 'randn'), ('wide1', 1, 8, 32, 3, 4, True, BF16, 25.0, 'randn'),
    ('wide2', 1, 8, 32, 0, 2, False, BF16, 0.5, 'pm8'), ('wide2', 1, 8, 32, 4, 2, True, F16, 25.0, 'randn'),
    ('wide2s', 1, 8, 32, 0, 2, True, BF16, 3.0, 'randn'),
    ('wide3', 1, 8, 32, 0, 4, True, F16, 3.0, 'randn'), ('wide3', 1, 8, 32, 2, 2, False, BF16, 25.0, 'pm8'),
    ('tall1', 1, 8, 32, 0, 2, True, BF16, 3.0, 'randn'), ('tall1', 1, 8, 32, 4, 2, True, F16, 25.0, 'randn'),
    ('tall1', 1, 8, 32, 13, 2, False, BF16, 25.0, 'pm8'),
    # the split (36-channel) front end
    ('all', 1, 8, 36, 3, 2, True, F16, 25.0, 'randn'), ('wide1', 1, 8, 36, 0, 4, False, BF16, 3.0, 'pm8'),
    ('wide2s', 1, 8, 36, 0, 2, True, BF16, 3.0, 'randn'), ('wide2s', 1, 8, 36, 3, 2, True, F16, 25.0, 'randn'),
    ('tall1', 1, 8, 36, 4, 2, True, BF16, 25.0, 'randn'),
]


def _split(K, value):
    """(B, S, M, 36) f64 -> K.SplitValue planes (M, B, S, 32) + (M, B, S, 4) f16 in one buffer."""
    v = _hm(value, F16)
    M_, B, S, _ = v.shape
    buf = torch.empty(M_ * B * S * 36, dtype=F16, device='cuda')
    main, tail = buf[:M_ * B * S * 32].view(M_, B, S, 32), buf[M_ * B * S * 32:].view(M_, B, S, 4)
    main.copy_(v[..., :32])
    tail.copy_(v[..., 32:])
    return K.SplitValue(main, tail)


def _enc(K, case, shapes, M, ch, odt, order=None, out=None):
    qm = case.get('qmask')
    qm = qm.cuda() if qm is not None else None
    hm = R.msda_hm(case['offlog'], M).cuda()
    if ch == 36:
        return K.msda_encoder_split(_split(K, case['value']), shapes, hm, case['refs'].cuda(), M, qm, out_dtype=odt,
                                    query_tile_order=order, out=out)
    return K.msda_encoder(_hm(case['value'], F16), shapes, hm, case['refs'].cuda(), M, qm, out_dtype=odt,
                          query_tile_order=order, out=out)


@pytest.mark.parametrize('geo,B,M,ch,forced,rd,masked,odt,noise,logits', ENC,
                         ids=lambda v: str(v).replace('torch.', ''))
def test_encoder_strip_kernel(K, strips, geo, B, M, ch, forced, rd, masked, odt, noise, logits):
    """msda_enc_kernel behind f16 offsets / logits (32 channels) and the split planes (36), at the plans of
    MSDA_ENC_CASES.  c_acc: the tap weight rounded to f16, 2^-11; each level's 16 packed-f16 multiply-adds,
    16 * 2^-11 on that level's share of A; the f32 adds of the levels and the tail's quad sum, 8 * 2^-24.
    Addressing targets come from the plan and the row-sorted tile order; the three tile orders and the
    one-strip plan must give the same bits."""
    shapes = R.MSDA_ENC_GEO[geo]
    S = sum(h * w for h, w in shapes)
    want = R.msda_enc_expected(geo, B, M, ch, forced)
    strips(forced)
    plan = K.msda_encoder_plan(shapes, B, M, S, ch)
    assert plan[:3] == want, (plan, want)
    fl, n, _ = want
    front = 'split' if ch == 36 else 'offlog'
    name = f'strip {front} fl{fl}'
    orders = _orders(K, shapes, S)
    sorted_order = tuple(orders[1].cpu().tolist())
    for cls in ('addr', 'generic'):
        if cls == 'addr':
            case = R.msda_addr_case(shapes, B, M, S, rd, D=ch, plan=(fl, n), order=sorted_order)
        else:
            case = R.msda_generic_case(shapes, B, M, S, rd, noise, logits, F16, D=ch, masked=masked, f16_offlog=True)
        prep, samp = R.msda_chain_ref(case, shapes, M)
        s = Sent(len(orders), (B, S, M * ch), odt)
        outs = [_enc(K, case, shapes, M, ch, odt, o, s.outs[i]) for i, o in enumerate(orders)]
        _ran(K, f'{geo} x{n}' + (' auto' if not forced else ''), ('encoder', fl, front))
        torch.cuda.synchronize()
        assert s.intact()
        out = outs[1]
        assert torch.equal(outs[0], out) and torch.equal(outs[2], out), 'tile order changed the result'
        if n > 1 and K.msda_encoder_plan(shapes, B, M, S, ch) is not None:
            strips(1)
            if K.msda_encoder_plan(shapes, B, M, S, ch)[1] == 1:
                assert torch.equal(_enc(K, case, shapes, M, ch, odt, orders[1]), out), 'strips changed the result'
            strips(forced)
        if cls == 'addr':
            cnt = R.msda_addr_counts(case, prep['loc'], shapes, (fl, n), sorted_order)
            for (l, c), v in cnt.items():
                if l >= fl and c not in ('near', 'far'):
                    if c == 'surely_far' and shapes[l][0] <= R.msda_enc_caps(shapes, fl, n)[l] + 2:
                        continue                     # (nearly) the whole level is staged: no row is surely far
                    key = f'{geo} x{n} {front} {c}'
                    _LOG['counts'][key] = min(_LOG['counts'].get(key, 1 << 30), v)
                    assert v >= 200, (geo, l, c, v)
            bound = R.msda_addr_bound(samp, shapes, 'strip', prep['locA'])
            assert bound.max().item() < 0.125
        else:
            bound = R.msda_bound(samp, shapes, 'strip', odt, prep['locA'], prep['attw_c'])
            if masked:
                assert (out[case['qmask'].cuda()] == 0).all()
        _check(f'{name} {cls}', out, samp['out'], bound)


@pytest.mark.parametrize('Lq', [1, 15, 17, 1400 + 21])
@pytest.mark.parametrize('ch', [32, 36])
def test_encoder_strip_kernel_query_counts(K, strips, Lq, ch):
    """Query sets that are not the levels' pixels: one query, a partial tile, a tile and one query, and a
    ragged last tile behind more queries than pixels."""
    shapes, B, M = R.MSDA_ENC_GEO['all'], 3, 8
    case = R.msda_generic_case(shapes, B, M, Lq, 2, 3.0, 'randn', F16, D=ch, f16_offlog=True)
    prep, samp = R.msda_chain_ref(case, shapes, M)
    s = Sent(1, (B, Lq, M * ch), BF16)
    out = _enc(K, case, shapes, M, ch, BF16, None, s.outs[0])
    torch.cuda.synchronize()
    _ran(K, f'all Lq={Lq}', ('encoder', 0, 'split' if ch == 36 else 'offlog'))
    assert s.intact() and (out[case['qmask'].cuda()] == 0).all()
    _check(f'strip {"split" if ch == 36 else "offlog"} Lq edges', out, samp['out'],
           R.msda_bound(samp, shapes, 'strip', BF16, prep['locA'], prep['attw_c']))


RECORDS = [('all', 1, 8, 3, BF16), ('all', 3, 8, 3, F16), ('wide1', 1, 8, 3, BF16), ('wide2s', 1, 8, 0, F16),
           ('wide3', 1, 8, 2, BF16), ('tall1', 1, 8, 4, F16)]


@pytest.mark.parametrize('geo,B,M,forced,odt', RECORDS, ids=lambda v: str(v).replace('torch.', ''))
def test_encoder_records(K, strips, geo, B, M, forced, odt):
    """msda_enc_kernel behind sampling records built on the host (oracle.sample_records of msda_prep_ref's
    f64 locations and weights).  The reference samples the decoded records: no location term.  Addressing
    class: the locations are exact fixed point, the products and sums exact integers -- equality.  Generic:
    two packed-f16 products make a tap weight (2 * 2^-11), then the strip kernel's sums."""
    from oracle import msda_oracle as O
    shapes = R.MSDA_ENC_GEO[geo]
    S = sum(h * w for h, w in shapes)
    fl, n, _ = want = R.msda_enc_expected(geo, B, M, 32, forced)
    strips(forced)
    assert K.msda_encoder_plan(shapes, B, M, S)[:3] == want
    fb = K.msda_record_frac_bits(shapes)
    assert fb == (8 if max(w for _, w in shapes) > 128 else 10)
    orders = _orders(K, shapes, S)
    sorted_order = tuple(orders[1].cpu().tolist())
    for cls in ('addr', 'generic'):
        case = R.msda_addr_case(shapes, B, M, S, 2, plan=(fl, n), order=sorted_order) if cls == 'addr' else \
            R.msda_generic_case(shapes, B, M, S, 2, 25.0 if forced else 3.0, 'randn', F16)
        if cls == 'addr':       # the exact targets: every weight is 0, 1/4, 1/2 or 1, every location on a half pixel
            case = dict(case, refs=case['refs64'])
        prep, _ = R.msda_chain_ref(case, shapes, M)
        rec = O.sample_records(prep['loc'], prep['attw'], case['refs'], shapes, fb)
        loc_d, aw_d = O.decode_records(rec, shapes, fb)
        samp = R.msda_sample_ref(case['value'], shapes, loc_d, aw_d)
        v = _hm(case['value'], F16)
        s = Sent(len(orders), (B, S, M * 32), odt)
        outs = [K.msda_encoder_records(v, shapes, rec.cuda(), fb, out_dtype=odt, query_tile_order=o, out=s.outs[i])
                for i, o in enumerate(orders)]
        torch.cuda.synchronize()
        _ran(K, f'{geo} x{n} fb{fb}', ('encoder', fl, 'records'))
        assert s.intact() and torch.equal(outs[0], outs[1]) and torch.equal(outs[2], outs[1])
        out = outs[1]
        if cls == 'addr':
            cnt = R.msda_addr_counts(case, prep['loc'], shapes, (fl, n), sorted_order)
            assert all(v >= 200 for (l, c), v in cnt.items() if l >= fl and c in ('win_first', 'win_last', 'row-1', 'rowH-1')), cnt
            want = samp['out'].round()          # (the decoded y H - 0.5 carries f64 rounding: 1e-12)
            assert (samp['out'] - want).abs().max().item() <= 1e-9 and want.abs().max().item() <= 32
            bad = int((out.double().cpu() != want).sum())
            _LOG['eq_bad'] += bad
            _LOG['eq_n'] += out.numel()
            assert bad == 0, f'{geo}: {bad} of {out.numel()} elements differ from the expected integer'
        else:
            _check(f'strip records fb{fb} generic', out, samp['out'], R.msda_bound(samp, shapes, 'records', odt))
            assert (out[case['qmask'].cuda()] == 0).all()
