"""The key-streaming MFMA attention kernel (csrc/attn.hip mha_stream_kernel: head_dim 32 / 36,
bf16 / f16, any Lk in double-buffered tiles of KT keys) vs fp32 SDPA with a key padding mask and
vs the FMA kernel on the same 16-bit inputs.

kinet_mha_set_mfma(2) sends every eligible call to the streaming kernel, so its tile edges are
reached at small sizes; with the knob at its default the kernel serves Lk above the resident
kernels' caps (384 at head_dim 32, 640 at head_dim 36), which ran the FMA kernel before.
Tolerances are test_mha_core_mfma's (tests/test_gemm_gpu.py): the per-32-key block arithmetic is
the resident kernels', so the same bound relative to max |ref| applies -- 2e-2 bf16, 4e-3 f16.
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


def _run(K, knob, q, k, v, D, mask):
    old = _knob(knob)
    try:
        y = K.mha_core(q, k, v, HEADS, D ** -0.5, key_mask=mask)
        torch.cuda.synchronize()
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


def _check(K, D, dtype, q, k, v, mask, knob=2):
    ref = _sdpa(q, k, v, D, mask)
    qc, kc, vc, mc = q.cuda(), k.cuda(), v.cuda(), mask.cuda()
    y = _run(K, knob, qc, kc, vc, D, mc)
    y_fma = _run(K, 0, qc, kc, vc, D, mc)
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


@pytest.mark.parametrize('Lq,Lk', _shapes())
@pytest.mark.parametrize('D', [32, 36])
@pytest.mark.parametrize('dtype', DTYPES)
def test_stream_forced(K, D, Lq, Lk, dtype):
    _check(K, D, dtype, *_inputs(D, Lq, Lk, dtype))


@pytest.mark.parametrize('case', ['first_tile', 'last_tile', 'dead_row'])
@pytest.mark.parametrize('D', [32, 36])
@pytest.mark.parametrize('dtype', DTYPES)
def test_stream_mask_edges(K, D, dtype, case):
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
    y, y_fma = _check(K, D, dtype, q, k, v, mask)
    if case == 'dead_row':
        assert (y[1] == 0).all() and (y_fma[1] == 0).all()
        assert y[0].abs().max() > 0 and y[2].abs().max() > 0


@pytest.mark.parametrize('D,Lq,Lk', [(32, 300, 385), (36, 500, 641), (32, 651, 651), (36, 651, 651)])
@pytest.mark.parametrize('dtype', DTYPES)
def test_stream_natural_dispatch(K, D, Lq, Lk, dtype):
    """Default knob, Lk above the resident caps: the streaming kernel (bit-equal to the forced
    run), no longer the FMA kernel."""
    assert Lk > K.MHA_RESIDENT_MAXK[D]
    q, k, v, mask = _inputs(D, Lq, Lk, dtype, seed=2)
    y, y_fma = _check(K, D, dtype, q, k, v, mask, knob=1)
    y2 = _run(K, 2, q.cuda(), k.cuda(), v.cuda(), D, mask.cuda())
    assert torch.equal(y, y2)
    assert not torch.equal(y, y_fma)


@pytest.mark.parametrize('D', [32, 36])
@pytest.mark.parametrize('dtype', DTYPES)
def test_stream_resident_sizes_keep_resident_kernel(K, D, dtype):
    """At the caps the default dispatch still runs the resident kernel: same block arithmetic in
    the same order, so the forced streaming run agrees to the kernels' common bound."""
    Lk = K.MHA_RESIDENT_MAXK[D]
    q, k, v, mask = _inputs(D, 40, Lk, dtype, seed=3)
    y, _ = _check(K, D, dtype, q, k, v, mask, knob=1)
    y2 = _run(K, 2, q.cuda(), k.cuda(), v.cuda(), D, mask.cuda())
    assert _rel(y2, y) < TOL[dtype]


@pytest.mark.parametrize('D', [32, 36])
@pytest.mark.parametrize('dtype', DTYPES)
def test_stream_strided_qk(K, D, dtype):
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
    y = _run(K, 2, qkc[..., :E], qkc[..., E:], v.cuda(), D, mask.cuda())
    y_fma = _run(K, 0, qkc[..., :E], qkc[..., E:], v.cuda(), D, mask.cuda())
    assert _rel(y, ref) < TOL[dtype]
    assert _rel(y, y_fma) < TOL[dtype]


@pytest.mark.parametrize('D', [32, 36])
def test_stream_knob_leaves_fp32_on_fma(K, D):
    """fp32 is not the streaming kernel's: under knob 2 it still runs the FMA kernel."""
    q, k, v, mask = _inputs(D, 70, 2 * K.MHA_STREAM_KT + 5, torch.float32, seed=4)
    ref = _sdpa(q, k, v, D, mask)
    y = _run(K, 2, q.cuda(), k.cuda(), v.cuda(), D, mask.cuda())
    assert _rel(y, ref) < 1e-5
    assert torch.equal(y, _run(K, 0, q.cuda(), k.cuda(), v.cuda(), D, mask.cuda()))


@pytest.mark.parametrize('D', [32, 36])
def test_stream_deterministic(K, D):
    q, k, v, mask = (t.cuda() for t in _inputs(D, 70, 2 * K.MHA_STREAM_KT + 5, torch.bfloat16, seed=5))
    assert torch.equal(_run(K, 2, q, k, v, D, mask), _run(K, 2, q, k, v, D, mask))


def test_knob_returns_previous_setting():
    assert _knob(2) == 1
    assert _knob(0) == 2
    assert _knob(1) == 0
