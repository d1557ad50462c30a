"""The MFMA attention kernels (csrc/attn.hip: mha_stream_kernel, any Lk in double-buffered tiles of
KT keys, and mha_resident_kernel, the head's keys staged once; head_dim 32 / 36, bf16 / f16) vs
fp32 SDPA with a key padding mask and vs the FMA kernel on the same 16-bit inputs.

kinet_mha_set_mfma(2) sends every eligible call to the streaming kernel, so its tile edges are
reached at small sizes; with the knob at its default (1) the same small shapes run the resident
kernel and the streaming kernel serves Lk above the resident caps (kernels.MHA_RESIDENT_MAXK).
Which kernel ran is asserted by name (kernels.mha_last_kernel).  Both kernels run one block step
(attn_block) over the same 32-key blocks in the same order, so their outputs are equal bit for bit.
Tolerances are test_mha_core_mfma's (tests/test_gemm_gpu.py): the same bound relative to
max |ref| -- 2e-2 bf16, 4e-3 f16.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B, HEADS = 3, 8
TOL = {torch.bfloat16: 2e-2, torch.float16: 4e-3}
DTYPES = [torch.bfloat16, torch.float16]


def _rel(a, b):
    return ((a.float().cpu() - b.float().cpu()).abs().max() / (b.float().abs().max() + 1e-6)).item()


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


def _knob(value):
    from kinet_amd import _native
    return _native.lib().kinet_mha_set_mfma(value)


KNOB = {'fma': 0, 'resident': 1, 'stream': 2}   # below the resident caps


def _run(K, knob, q, k, v, D, mask, kernel=None):
    """mha_core under `knob`; kernel: the kernel the call must have launched."""
    old = _knob(knob)
    try:
        y = K.mha_core(q, k, v, HEADS, D ** -0.5, key_mask=mask)
        torch.cuda.synchronize()
        assert kernel is None or K.mha_last_kernel() == kernel
        return y
    finally:
        _knob(old)


def _inputs(D, Lq, Lk, dtype, seed=0):
    E = HEADS * D
    g = torch.Generator().manual_seed(1000 * seed + 31 * Lq + Lk + D)
    q, k, v = (torch.randn(B, n, E, generator=g).to(dtype) for n in (Lq, Lk, Lk))
    mask = torch.rand(B, Lk, generator=g) < 0.2
    mask[:, 0] = False
    return q, k, v, mask


def _sdpa(q, k, v, D, mask):
    """fp32 SDPA on the (16-bit rounded) inputs; rows of a batch whose keys are all masked -> 0."""
    Lq, Lk = q.shape[1], k.shape[1]

    def split(t, n):
        return t.float().view(B, n, HEADS, D).transpose(1, 2)
    dead = mask.all(1)
    m = mask.clone()
    m[dead] = False
    ref = F.scaled_dot_product_attention(split(q, Lq), split(k, Lk), split(v, Lk),
                                         attn_mask=~m[:, None, None, :]).transpose(1, 2).reshape(B, Lq, HEADS * D)
    ref[dead] = 0
    return ref


def _check(K, D, dtype, q, k, v, mask, knob=2, kernel='stream'):
    ref = _sdpa(q, k, v, D, mask)
    qc, kc, vc, mc = q.cuda(), k.cuda(), v.cuda(), mask.cuda()
    y = _run(K, knob, qc, kc, vc, D, mc, kernel)
    y_fma = _run(K, 0, qc, kc, vc, D, mc, 'fma')
    e_ref, e_fma = _rel(y, ref), _rel(y, y_fma)
    print(f'[mha_stream] D={D} {dtype} Lq={q.shape[1]} Lk={k.shape[1]} knob={knob}: vs sdpa {e_ref:.3g} '
          f'vs fma {e_fma:.3g}')
    assert torch.isfinite(y.float()).all()
    assert e_ref < TOL[dtype]
    assert e_fma < TOL[dtype]
    return y, y_fma


def _shapes():
    from kinet_amd.kernels import MHA_STREAM_KT as KT
    # one key; one partial tile + a second query block with one live row; exactly one tile; one
    # tile + one key; three tiles (both buffers reused) with a ragged tail
    return [(1, 1), (65, 37), (16, KT), (16, KT + 1), (70, 2 * KT + 5)]


# Each case below runs on the streaming kernel (test_stream_*: knob 2) and, every shape here being
# below the resident caps, on the resident kernel (test_resident_*: knob 1).

def _forced(K, D, Lq, Lk, dtype, kernel):
    _check(K, D, dtype, *_inputs(D, Lq, Lk, dtype), knob=KNOB[kernel], kernel=kernel)


@pytest.mark.parametrize('Lq,Lk', _shapes())
@pytest.mark.parametrize('D', [32, 36])
@pytest.mark.parametrize('dtype', DTYPES)
def test_stream_forced(K, D, Lq, Lk, dtype):
    _forced(K, D, Lq, Lk, dtype, 'stream')


@pytest.mark.parametrize('Lq,Lk', _shapes())
@pytest.mark.parametrize('D', [32, 36])
@pytest.mark.parametrize('dtype', DTYPES)
def test_resident_forced(K, D, Lq, Lk, dtype):
    _forced(K, D, Lq, Lk, dtype, 'resident')


def _mask_edges(K, D, dtype, case, kernel):
    """Whole tiles masked (the running max stays -inf through the first tile / is untouched by
    the last) and a batch row with no live key: exactly 0, as the FMA kernel."""
    KT = K.MHA_STREAM_KT
    Lq, Lk = 70, 2 * KT + 5
    q, k, v, mask = _inputs(D, Lq, Lk, dtype, seed=1)
    if case == 'first_tile':
        mask[:, :KT] = True
        mask[:, KT] = False
    elif case == 'last_tile':
        mask[:, 2 * KT:] = True
    else:
        mask[1] = True
    y, y_fma = _check(K, D, dtype, q, k, v, mask, knob=KNOB[kernel], kernel=kernel)
    if case == 'dead_row':
        assert (y[1] == 0).all() and (y_fma[1] == 0).all()
        assert y[0].abs().max() > 0 and y[2].abs().max() > 0


@pytest.mark.parametrize('case', ['first_tile', 'last_tile', 'dead_row'])
@pytest.mark.parametrize('D', [32, 36])
@pytest.mark.parametrize('dtype', DTYPES)
def test_stream_mask_edges(K, D, dtype, case):
    _mask_edges(K, D, dtype, case, 'stream')


@pytest.mark.parametrize('case', ['first_tile', 'last_tile', 'dead_row'])
@pytest.mark.parametrize('D', [32, 36])
@pytest.mark.parametrize('dtype', DTYPES)
def test_resident_mask_edges(K, D, dtype, case):
    _mask_edges(K, D, dtype, case, 'resident')


@pytest.mark.parametrize('D,Lq,Lk', [(32, 300, 385), (36, 500, 641), (32, 651, 651), (36, 651, 651)])
@pytest.mark.parametrize('dtype', DTYPES)
def test_stream_natural_dispatch(K, D, Lq, Lk, dtype):
    """Default knob, Lk above the resident caps: the streaming kernel (bit-equal to the forced
    run), no longer the FMA kernel."""
    assert Lk > K.MHA_RESIDENT_MAXK[D]
    q, k, v, mask = _inputs(D, Lq, Lk, dtype, seed=2)
    y, y_fma = _check(K, D, dtype, q, k, v, mask, knob=1, kernel='stream')
    y2 = _run(K, 2, q.cuda(), k.cuda(), v.cuda(), D, mask.cuda(), 'stream')
    assert torch.equal(y, y2)
    assert not torch.equal(y, y_fma)


def _resident_equals_stream(K, D, dtype, Lk):
    q, k, v, mask = _inputs(D, 40, Lk, dtype, seed=3)
    y, _ = _check(K, D, dtype, q, k, v, mask, knob=1, kernel='resident')
    y2 = _run(K, 2, q.cuda(), k.cuda(), v.cuda(), D, mask.cuda(), 'stream')
    assert torch.equal(y2, y)


@pytest.mark.parametrize('D', [32, 36])
@pytest.mark.parametrize('dtype', DTYPES)
def test_stream_resident_sizes_keep_resident_kernel(K, D, dtype):
    """At the caps the default dispatch still runs the resident kernel: the same block step over
    the same blocks in the same order, so the forced streaming run gives the same bits."""
    _resident_equals_stream(K, D, dtype, K.MHA_RESIDENT_MAXK[D])


@pytest.mark.parametrize('D', [32, 36])
@pytest.mark.parametrize('dtype', DTYPES)
def test_resident_small_equals_stream(K, D, dtype):
    """The same at 37 keys: a ragged second block, a partial first tile."""
    _resident_equals_stream(K, D, dtype, 37)


def _strided_qk(K, D, dtype, kernel):
    """q and k as the two halves of one (B, L, 2E) projection (row stride 2E), as the models'
    fused q|k GEMM produces them."""
    E, L = HEADS * D, K.MHA_STREAM_KT + 1
    g = torch.Generator().manual_seed(7 + D)
    qk = torch.randn(B, L, 2 * E, generator=g).to(dtype)
    v = torch.randn(B, L, E, generator=g).to(dtype)
    mask = torch.rand(B, L, generator=g) < 0.2
    mask[:, 0] = False
    ref = _sdpa(qk[..., :E], qk[..., E:], v, D, mask)
    qkc = qk.cuda()
    y = _run(K, KNOB[kernel], qkc[..., :E], qkc[..., E:], v.cuda(), D, mask.cuda(), kernel)
    y_fma = _run(K, 0, qkc[..., :E], qkc[..., E:], v.cuda(), D, mask.cuda(), 'fma')
    assert _rel(y, ref) < TOL[dtype]
    assert _rel(y, y_fma) < TOL[dtype]


@pytest.mark.parametrize('D', [32, 36])
@pytest.mark.parametrize('dtype', DTYPES)
def test_stream_strided_qk(K, D, dtype):
    _strided_qk(K, D, dtype, 'stream')


@pytest.mark.parametrize('D', [32, 36])
@pytest.mark.parametrize('dtype', DTYPES)
def test_resident_strided_qk(K, D, dtype):
    _strided_qk(K, D, dtype, 'resident')


@pytest.mark.parametrize('D', [32, 36])
def test_stream_knob_leaves_fp32_on_fma(K, D):
    """fp32 is not the streaming kernel's: under knob 2 it still runs the FMA kernel."""
    q, k, v, mask = _inputs(D, 70, 2 * K.MHA_STREAM_KT + 5, torch.float32, seed=4)
    ref = _sdpa(q, k, v, D, mask)
    y = _run(K, 2, q.cuda(), k.cuda(), v.cuda(), D, mask.cuda(), 'fma')
    assert _rel(y, ref) < 1e-5
    assert torch.equal(y, _run(K, 0, q.cuda(), k.cuda(), v.cuda(), D, mask.cuda(), 'fma'))


def _deterministic(K, D, kernel):
    q, k, v, mask = (t.cuda() for t in _inputs(D, 70, 2 * K.MHA_STREAM_KT + 5, torch.bfloat16, seed=5))
    knob = KNOB[kernel]
    assert torch.equal(_run(K, knob, q, k, v, D, mask, kernel), _run(K, knob, q, k, v, D, mask, kernel))


@pytest.mark.parametrize('D', [32, 36])
def test_stream_deterministic(K, D):
    _deterministic(K, D, 'stream')


@pytest.mark.parametrize('D', [32, 36])
def test_resident_deterministic(K, D):
    _deterministic(K, D, 'resident')


def test_knob_returns_previous_setting():
    assert _knob(2) == 1
    assert _knob(0) == 2
    assert _knob(1) == 0
