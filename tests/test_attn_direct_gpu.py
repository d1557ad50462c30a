"""Direct tests of the attention forward kernels, path by path: mha_resident_kernel<T, D> and mha_stream_kernel<T, D>
(csrc/attn.hip; bf16 / f16, head_dim 32 / 36) and the FMA kernel mha_kernel<T, D> (csrc/ops.hip; f32 / bf16 / f16,
head_dim 16 / 32 / 36 / 64), against the cases, expected values and the f64 bound of tests/direct_refs.py (checked on
the CPU, with the mutations they must catch, by test_direct_refs_cpu.py).

Every call goes through kernels.mha_core under the knob kinet_mha_set_mfma (0: FMA, 1: by Lk, 2: streaming), with
an explicit scale; the kernel that ran is asserted by name and the knob restored.  q, k, v and the output are views
of wider tensors with four different row strides; the inputs' gap columns hold NaN, the output sits in a sentinel
buffer whose gap columns and guard rows must come back bit for bit.

Class 1 (selection) and class 2 (ties): the expected output is known exactly -- a row of v, or the representable mean
of n rows -- and compared bit for bit.  Class 3 (generic): N(0, 1) operands under the per-element bound
R.attn_fwd_bound, with torch's CPU f32 SDPA under the same bound as the yardstick.

KINET_ATTN_DIRECT_LOG names a file that receives the per-case lines (profiles/attn_direct.log)."""
import os
import time

import pytest
import torch

import direct_refs as R

pytestmark = pytest.mark.gpu

SENTINEL = 77.0
GUARD = 3                                   # sentinel rows before and after the output
OFF = {'q': 8, 'k': 16, 'v': 24, 'o': 8}    # first column of each view: 16-byte aligned
TAIL = {'q': 16, 'k': 16, 'v': 16, 'o': 40}  # row strides E + 24, E + 32, E + 40, E + 48: all different
KNOB = {'fma': 0, 'resident': 1, 'stream': 2}
MFMA = [i for i in R.ATTN_INST if i[0] != 'fma']
_LOG = {'t0': None, 'lines': []}


def _name(dt):
    return str(dt).replace('torch.', '')


def _id(inst):
    return f'{inst[0]}-{_name(inst[1])}-D{inst[2]}'


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    assert kernels.MHA_STREAM_KT == R.ATTN_KT and kernels.MHA_RESIDENT_MAXK == R.ATTN_RESIDENT_MAXK
    return kernels


@pytest.fixture(scope='module', autouse=True)
def _report():
    _LOG['t0'] = time.time()
    yield
    lines = [f'module wall time: {time.time() - _LOG["t0"]:.1f} s'] + _LOG['lines']
    print('\n'.join(lines))
    path = os.environ.get('KINET_ATTN_DIRECT_LOG')
    if path:
        with open(path, 'w') as f:
            f.write('\n'.join(lines) + '\n')


def _log(line):
    _LOG['lines'].append(line)


def _knob(value):
    from kinet_amd import _native
    return _native.lib().kinet_mha_set_mfma(value)


def _wide(t, name, off=None, tail=None):
    """t (B, L, E) as a view of a wider NaN-filled device tensor."""
    off = OFF[name] if off is None else off
    tail = TAIL[name] if tail is None else tail
    B, L, E = t.shape
    w = torch.full((B, L, off + E + tail), float('nan'), dtype=t.dtype, device='cuda')
    w[..., off:off + E] = t.cuda()
    return w[..., off:off + E]


def _run(K, kernel, case, knob=None, views=None, out_off=None, out_tail=None, mask='case', **kw):
    """mha_core on the case under the knob; returns the output (CPU) after checking the kernel's name and that
    nothing outside the output view was written."""
    q, k, v = views if views is not None else (_wide(case['q'], 'q'), _wide(case['k'], 'k'), _wide(case['v'], 'v'))
    B, Lq, E = q.shape
    off = OFF['o'] if out_off is None else out_off
    tail = TAIL['o'] if out_tail is None else out_tail
    buf = torch.full((GUARD + B * Lq + GUARD, off + E + tail), SENTINEL, dtype=q.dtype, device='cuda')
    out = buf[GUARD:GUARD + B * Lq].view(B, Lq, -1)[..., off:off + E]
    m = case['mask'] if isinstance(mask, str) else mask
    old = _knob(KNOB[kernel] if knob is None else knob)
    try:
        K.mha_core(q, k, v, case['heads'], case['scale'], key_mask=None if m is None else m.cuda(), out=out, **kw)
        torch.cuda.synchronize()
        ran = K.mha_last_kernel()
    finally:
        _knob(old)
    assert ran == kernel, (ran, kernel)
    got = out.cpu()
    rest = buf.clone()
    rest[GUARD:GUARD + B * Lq, off:off + E] = SENTINEL
    assert torch.equal(R.attn_bits(rest.cpu()), R.attn_bits(torch.full_like(rest, SENTINEL).cpu())), 'sentinel overwritten'
    return got


def _exact(K, inst, case, tag):
    kernel, _, D = inst
    natural = kernel == 'stream' and case['k'].shape[1] > R.ATTN_RESIDENT_MAXK[D]      # above the cap: the default knob
    got = _run(K, kernel, case, knob=1 if natural else None)
    bad = int((R.attn_bits(got) != R.attn_bits(case['expected'])).sum())
    _log(f'{tag} {_id(inst)} Lq={got.shape[1]} Lk={case["k"].shape[1]}: {bad} of {got.numel()} elements differ')
    return bad


@pytest.mark.parametrize('inst', R.ATTN_INST, ids=_id)
def test_selection_is_bit_exact(K, inst):
    """Class 1 at every (Lq, Lk) of the instantiation, the three mask modes at the three-tile shape."""
    kernel, dtype, D = inst
    bad = {}
    for Lq, Lk in R.attn_shapes(kernel, D):
        for mode in (('pairs', 'edges', 'last') if (Lq, Lk) == R.ATTN_MAIN else ('pairs',)):
            n = _exact(K, inst, R.attn_select_case(D, Lq, Lk, dtype, mode), f'select/{mode}')
            if n:
                bad[(Lq, Lk, mode)] = n
    assert not bad, bad


@pytest.mark.parametrize('inst', R.ATTN_INST, ids=_id)
def test_ties_are_bit_exact(K, inst):
    """Class 2: the mean of the 2 .. 64 tied keys' values, at 129 and 17 queries."""
    kernel, dtype, D = inst
    bad = {Lq: n for Lq in (129, 17) if (n := _exact(K, inst, R.attn_tie_case(D, Lq, dtype), 'tie'))}
    assert not bad, bad


def _generic(K, inst, case, tag, got=None):
    """One class-3 comparison: (worst err / bound, the output)."""
    kernel, dtype, D = inst
    got = _run(K, kernel, case) if got is None else got
    bound = R.attn_fwd_bound(case, kernel, dtype)
    worst, share, zeros = R.attn_ratio(got.double(), case, bound)
    yard = R.attn_ratio(case['sdpa'].to(dtype).double(), case, bound)[0]
    _log(f'{tag} {_id(inst)} Lq={got.shape[1]} Lk={case["k"].shape[1]}: worst err/bound {worst:.3f} '
         f'(f32 sdpa {yard:.3f}), compared {100 * share:.1f} %, rest exactly 0: {zeros}')
    assert torch.isfinite(got.float()).all()
    return (worst if zeros else float('inf')), got


@pytest.mark.parametrize('variant', R.ATTN_VARIANTS)
@pytest.mark.parametrize('inst', R.ATTN_INST, ids=_id)
def test_generic_within_bound(K, inst, variant):
    """Class 3 at every (Lq, Lk), the resident caps and (natural dispatch, knob 1) cap + 1 included; below the caps
    the resident and the forced streaming kernel must agree bit for bit."""
    kernel, dtype, D = inst
    worst = {}
    for Lq, Lk in R.attn_shapes(kernel, D):
        case = R.attn_generic_case(D, Lq, Lk, dtype, variant)
        natural = kernel == 'stream' and Lk > R.ATTN_RESIDENT_MAXK[D]
        got = _run(K, kernel, case, knob=1) if natural else None
        r, got = _generic(K, inst, case, f'generic/{variant}' + ('/natural' if natural else ''), got)
        if not r < 1.0:
            worst[(Lq, Lk)] = r
        if kernel == 'resident':
            assert torch.equal(R.attn_bits(got), R.attn_bits(_run(K, 'stream', case))), (Lq, Lk)
    assert not worst, worst


@pytest.mark.parametrize('inst', R.ATTN_INST, ids=_id)
def test_masks(K, inst):
    """The mask edges at three tiles with a second workgroup of one live row: None and all-False give equal bits; a
    fully masked batch is exactly 0 and leaves the other batch's bits as they are without it."""
    kernel, dtype, D = inst
    Lq, Lk = 65, 2 * R.ATTN_KT + 5
    out, worst = {}, {}
    for mode in R.ATTN_MASKS:
        r, out[mode] = _generic(K, inst, R.attn_generic_case(D, Lq, Lk, dtype, 'plain', mode), f'mask/{mode}')
        if not r < 1.0:
            worst[mode] = r
    assert not worst, worst
    assert torch.equal(R.attn_bits(out['none']), R.attn_bits(out['allfalse']))
    assert (R.attn_bits(out['dead_batch'][1]) == 0).all()
    case = R.attn_generic_case(D, Lq, Lk, dtype, 'plain', 'dead_batch')
    live = case['mask'].clone()
    live[1] = False
    assert torch.equal(R.attn_bits(_run(K, kernel, case, mask=live)[0]), R.attn_bits(out['dead_batch'][0]))


@pytest.mark.parametrize('inst', MFMA, ids=_id)
def test_f16_subnormal_probabilities(K, inst):
    """One key at p = 1, 256 keys near p = 2^-16, all values 1: inside the bound only if the f16 subnormal p survive
    the conversion and the MFMA (flushed, the output is 1 - 2^-8: four times the bound)."""
    r, _ = _generic(K, inst, R.attn_subnormal_case(inst[2], inst[1]), 'subnormal-p')
    assert r < 1.0, r


@pytest.mark.parametrize('inst', MFMA, ids=_id)
def test_rounded_p_bias_stays_in_the_bound(K, inst):
    """R.attn_bias_case: every p of a value-1 key is rounded down by almost u16, so the output is low by almost u16 oA
    -- the systematic part of term (b), inside the bound; summing l from the rounded p would put it outside."""
    r, _ = _generic(K, inst, R.attn_bias_case(inst[2], inst[1]), 'rounded-p bias')
    assert r < 1.0, r


@pytest.mark.parametrize('inst', R.ATTN_INST, ids=_id)
def test_neighbouring_batch_and_qk_halves(K, inst):
    """q | k as the halves of one projection (row stride 2 E + 8), and a call on batch 1 alone of a two-batch output
    buffer: batch 0's rows, as everything else around the view, keep their sentinel bits."""
    kernel, dtype, D = inst
    case = R.attn_generic_case(D, 65, 65, dtype, 'plain')
    E = case['q'].shape[-1]
    w = _wide(torch.cat([case['q'], case['k']], -1), 'q', off=8, tail=0)
    r, _ = _generic(K, inst, case, 'qk-halves', _run(K, kernel, case, views=(w[..., :E], w[..., E:], _wide(case['v'], 'v'))))
    assert r < 1.0, r
    one = {**case, 'q': case['q'][1:], 'k': case['k'][1:], 'v': case['v'][1:], 'mask': case['mask'][1:]}
    q, k, v = _wide(one['q'], 'q'), _wide(one['k'], 'k'), _wide(one['v'], 'v')
    Lq = q.shape[1]
    buf = torch.full((GUARD + 2 * Lq + GUARD, 8 + E + 40), SENTINEL, dtype=dtype, device='cuda')
    out = buf[GUARD + Lq:GUARD + 2 * Lq].view(1, Lq, -1)[..., 8:8 + E]
    old = _knob(KNOB[kernel])
    try:
        K.mha_core(q, k, v, one['heads'], one['scale'], key_mask=one['mask'].cuda(), out=out)
        torch.cuda.synchronize()
        assert K.mha_last_kernel() == kernel
    finally:
        _knob(old)
    whole = _run(K, kernel, case)
    assert torch.equal(R.attn_bits(out.cpu()[0]), R.attn_bits(whole[1]))
    buf[GUARD + Lq:GUARD + 2 * Lq, 8:8 + E] = SENTINEL
    assert torch.equal(R.attn_bits(buf.cpu()), R.attn_bits(torch.full_like(buf, SENTINEL).cpu()))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=_name)
@pytest.mark.parametrize('D', [32, 36])
def test_planner_boundaries(K, D, dtype):
    """Row strides of E + 4 and a q pointer 4 elements off the 16-byte grid: head_dim 32 (16-byte pieces) falls to the
    FMA kernel, head_dim 36 (8-byte pieces) stays on the MFMA kernels; dropout falls to the FMA kernel.  Each by name
    and against the reference."""
    case = R.attn_generic_case(D, 65, R.ATTN_KT + 1, dtype, 'plain')
    want = 'fma' if D == 32 else 'resident'
    inst = (want, dtype, D)
    q4, k4, v4 = (_wide(case[n], n, off=0, tail=4) for n in 'qkv')
    r, _ = _generic(K, inst, case, 'plan/stride E+4', _run(K, want, case, knob=1, views=(q4, k4, v4), out_off=0, out_tail=4))
    assert r < 1.0, r
    r, _ = _generic(K, inst, case, 'plan/q+4', _run(K, want, case, knob=1, views=(_wide(case['q'], 'q', off=4, tail=20),
                                                                                _wide(case['k'], 'k'), _wide(case['v'], 'v'))))
    assert r < 1.0, r
    if D == 36:
        want2 = ('stream', dtype, D)
        r, _ = _generic(K, want2, case, 'plan/stride E+4', _run(K, 'stream', case, views=(q4, k4, v4), out_off=0, out_tail=4))
        assert r < 1.0, r
    # dropout: the FMA kernel under every knob.  p = 1e-9 has threshold 0 and an f32 keep scale of exactly 1, so every
    # probability is kept and the reference is the plain one (the dropout numerics: test_grad_norm_attn_gpu.py)
    seed = torch.tensor([1234], dtype=torch.int64, device='cuda')
    for knob in (1, 2):
        r, _ = _generic(K, ('fma', dtype, D), case, f'plan/dropout knob {knob}',
                        _run(K, 'fma', case, knob=knob, dropout_p=1e-9, seed=seed))
        assert r < 1.0, r


@pytest.mark.parametrize('D', [16, 32, 36, 64])
def test_f32_under_the_stream_knob_runs_fma(K, D):
    case = R.attn_generic_case(D, 65, R.ATTN_KT + 1, torch.float32, 'plain')
    inst = ('fma', torch.float32, D)
    r, got = _generic(K, inst, case, 'plan/f32 knob 2', _run(K, 'fma', case, knob=2))
    assert r < 1.0, r
    assert torch.equal(got, _run(K, 'fma', case))
