"""Direct tests of the training glue kernels of csrc/train_ops.hip -- dropout + add + LayerNorm both
ways, dropout + activation, msda_prep both ways, inverse sigmoid -- against references built on the
CPU from seeded inputs (tests/direct_refs.py): f64 with per-element bounds c * 2^-24 * A_i, bit-exact
where the kernel only selects and scales.  Every keep mask comes from the numpy restatement of the
dropout hash at the documented flat index, never from the kernels.  Shapes sit on both edges of every
template instantiation and dispatch branch of the launchers."""
import pytest
import torch

import direct_refs as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _seed(v):
    return torch.tensor([v], dtype=torch.int64, device='cuda')


def _within(got, ref, A, c, what='', floor=0.0):
    got = got.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    tol = c * R.U32 * A + floor
    err = (got - ref).abs()
    bad = err > tol
    assert not bad.any(), (what, int(bad.sum()), err.max().item(), (err / (tol + 1e-300)).max().item())


def _offset_one(t):
    """The same values, contiguous, one element into a device buffer (not 16-byte aligned)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device='cuda')
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


# ------------------------------------------------------- dropout + add + LayerNorm
DLN_D = [1, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 1024]      # both edges of NV = 1..5, 16
DLN_ROWS = [1, 3, 4, 5, 31, 32, 33]                                    # forward 4 rows a block, backward 32
DLN_SEED = 20240607
DLN_ROWS_CHAIN = 8 + 4 + 1 + 8      # 8 rows per wave serially, 4 waves, the final loop and tree
DLN_Z = 4                           # z = x + r * s: the scale's two roundings, the product, the sum


def _dln_case(rows, d, p):
    g = _gen(rows * 4099 + d)
    x, r, dy = (torch.randn(rows, d, generator=g) for _ in range(3))
    gamma, beta = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
    Zs = R.keep_mask(DLN_SEED, (rows, d), p).double() * R.keep_scale64(p)          # flat index r*d + c
    ref = R.ln_ref(x.double() + r.double() * Zs, gamma, beta, 1e-5, dy=dy, zA=x.double().abs() + r.double().abs() * Zs)
    return x, r, dy, gamma, beta, Zs, ref


def _dln_check(K, rows, d, p, need_x=True, need_r=True, need_params=True):
    x, r, dy, gamma, beta, Zs, ref = _dln_case(rows, d, p)
    c = R.ln_c(d, DLN_ROWS_CHAIN)
    what = (rows, d, p)
    seed = _seed(DLN_SEED)
    y = K.dropout_add_layernorm(x.cuda(), r.cuda(), gamma.cuda(), beta.cuda(), 1e-5, p, seed)
    _within(y, ref['y'], ref['yA'], c['xh'] + 2 + DLN_Z, ('y',) + what)           # xh * gamma + beta: 2
    dx, dr, dg, db = K.dropout_add_layernorm_backward(dy.cuda(), x.cuda(), r.cuda(), gamma.cuda(), 1e-5, p, seed,
                                                      need_x=need_x, need_r=need_r, need_params=need_params)
    assert (dx is None) == (not need_x) and (dr is None) == (not need_r)
    assert (dg is None) == (not need_params) and (db is None) == (not need_params)
    if need_x:
        _within(dx, ref['dz'], ref['dzA'], c['dx'] + DLN_Z, ('dx',) + what)
    if need_r:
        _within(dr, ref['dz'] * Zs, ref['dzA'] * Zs, c['dx'] + DLN_Z + 1, ('dr',) + what)
        assert (dr.cpu()[Zs == 0] == 0).all()
    if need_params:
        _within(dg, ref['dg'], ref['dgA'], c['dg'] + DLN_Z, ('dgamma',) + what)
        _within(db, ref['db'], ref['dbA'], c['db'], ('dbeta',) + what)


@pytest.mark.parametrize('d', DLN_D)
@pytest.mark.parametrize('p', [0.0, 0.3])
def test_dropout_add_layernorm_vs_f64(K, p, d):
    for rows in DLN_ROWS:
        _dln_check(K, rows, d, p)


@pytest.mark.parametrize('off', ['need_x', 'need_r', 'need_params'])
def test_dropout_add_layernorm_backward_optional_outputs(K, off):
    for d in (65, 321):
        _dln_check(K, 33, d, 0.3, **{off: False})


def test_dropout_add_layernorm_no_rows(K):
    d = 193
    x = torch.zeros(0, d, device='cuda')
    gamma, beta = torch.ones(d, device='cuda'), torch.zeros(d, device='cuda')
    y = K.dropout_add_layernorm(x, x, gamma, beta, 1e-5, 0.3, _seed(1))
    assert y.shape == (0, d)
    dx, dr, dg, db = K.dropout_add_layernorm_backward(x, x, x, gamma, 1e-5, 0.3, _seed(1))
    assert dx.shape == dr.shape == (0, d) and (dg == 0).all() and (db == 0).all()


def test_dropout_add_layernorm_repeatable(K):
    x, r, dy, gamma, beta, _, _ = _dln_case(33, 321, 0.3)
    args = (dy.cuda(), x.cuda(), r.cuda(), gamma.cuda(), 1e-5, 0.3, _seed(DLN_SEED))
    a, b = K.dropout_add_layernorm_backward(*args), K.dropout_add_layernorm_backward(*args)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


# ----------------------------------------------------------------------- dropout_act
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 1024, 1025])
@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('p', [0.0, 0.5])
def test_dropout_act_bit_exact(K, p, relu, n):
    """y = Z * act(x) and dx = Z * dy * act'(x) restated in f32 on the CPU (one product each, no
    reassociation possible): equal bit for bit.  Flat index i."""
    seed = 77 + n
    x, dy = torch.randn(n, generator=_gen(n)), torch.randn(n, generator=_gen(n + 1))
    x[::7] = 0.0
    Z = torch.ones(n)
    if p > 0:
        Z = R.keep_mask(seed, (n,), p).float() * torch.tensor(R.keep_scale32(p), dtype=torch.float32)
    act = torch.where(x > 0, x, torch.zeros_like(x)) if relu else x
    y_ref = act * Z if p > 0 else act
    y = K.dropout_act(x.cuda(), p, _seed(seed), relu)
    assert torch.equal(y.cpu(), y_ref)
    g = torch.where(y_ref <= 0, torch.zeros_like(dy), dy) if relu else dy
    dx_ref = g * Z if p > 0 else g
    dx = K.dropout_act_backward(dy.cuda(), y, p, _seed(seed), relu)
    assert torch.equal(dx.cpu(), dx_ref)


# ------------------------------------------------------------------------- msda_prep
PREP_V4 = [(8, 4, 4), (8, 1, 4), (4, 2, 4), (8, 8, 4), (4, 16, 4), (16, 8, 4)]     # (16, 8, 4): backward scalar
PREP_SCALAR = [(1, 1, 1), (2, 3, 2), (64, 1, 1), (32, 2, 3), (8, 4, 3)]
PREP_GEOMS = [(1, 1, 'none'), (2, 37, 'random'), (1, 37, 'all')]                   # (Nb, Lq, query mask)


def _qmask(kind, Nb, Lq):
    if kind == 'none':
        return None
    if kind == 'all':
        return torch.ones(Nb, Lq, dtype=torch.bool)
    m = torch.rand(Nb, Lq, generator=_gen(Nb + Lq)) < 0.4
    m[0, 0], m[-1, -1] = True, False
    return m


def _prep_check(K, Nb, Lq, M, L, P, rd, mask='none', pad=0, logits='randn', offset=False, need_offlog=True,
                need_refs=True):
    offlog, refs, shapes, gloc, gattw = R.msda_case(Nb, Lq, M, L, P, rd, pad=pad, logits=logits)
    qm = _qmask(mask, Nb, Lq)
    n = M * L * P
    what = (Nb, Lq, M, L, P, rd, mask, pad, logits, offset)
    ref = R.msda_prep_ref(offlog, refs, shapes, qm, M, L, P)
    og = _offset_one(offlog) if offset else offlog.cuda()
    loc, attw = K.msda_prep(og, refs.cuda(), shapes.cuda(), None if qm is None else qm.cuda(), M, L, P)
    _within(loc, ref['loc'], ref['locA'], ref['loc_c'], ('loc',) + what)
    _within(attw, ref['attw'], ref['attw'], ref['attw_c'], ('attw',) + what, floor=R.F32_TINY)
    if qm is not None:
        assert (attw.cpu()[qm] == 0).all()
    # backward for the f64 weights rounded to f32 (an input of the kernel, built on the CPU)
    a32 = ref['attw'].float()
    bref = R.msda_prep_bwd_ref(gloc, gattw, a32, offlog, refs, shapes, M, L, P)
    dol, dref = K.msda_prep_backward(gloc.cuda(), gattw.cuda(), a32.cuda(), og, refs.cuda(), shapes.cuda(), M, L, P,
                                     need_offlog=need_offlog, need_refs=need_refs)
    assert (dol is None) == (not need_offlog) and (dref is None) == (not need_refs)
    if need_offlog:
        assert dol.shape == offlog.shape
        _within(dol[..., :3 * n], bref['dol'], bref['dolA'], bref['dol_c'], ('d_offlog',) + what)
        if qm is not None:
            assert (dol.cpu()[..., 2 * n:3 * n][qm] == 0).all()
    if need_refs:
        _within(dref, bref['dref'], bref['drefA'], bref['dref_c'], ('d_refs',) + what)
    return loc, attw, dol, dref


@pytest.mark.parametrize('M,L,P', PREP_V4 + PREP_SCALAR)
@pytest.mark.parametrize('rd', [2, 4])
def test_msda_prep_fwd_bwd_vs_f64(K, rd, M, L, P):
    for Nb, Lq, mask in PREP_GEOMS:
        _prep_check(K, Nb, Lq, M, L, P, rd, mask=mask)


@pytest.mark.parametrize('rd', [2, 4])
@pytest.mark.parametrize('how', ['stride', 'offset'])
def test_msda_prep_misaligned_falls_back(K, how, rd):
    """(8, 4, 4) with a row stride of 385 (not a multiple of 4) or a base pointer one element in: the
    vector kernels' conditions fail and the scalar kernels run."""
    _prep_check(K, 2, 37, 8, 4, 4, rd, mask='random', pad=1 if how == 'stride' else 0, offset=how == 'offset')


@pytest.mark.parametrize('M,L,P', [(8, 4, 4), (2, 3, 2)])
@pytest.mark.parametrize('logits', ['pm80', 'equal'])
def test_msda_prep_extreme_logits(K, logits, M, L, P):
    _prep_check(K, 2, 37, M, L, P, 2, mask='random', logits=logits)


@pytest.mark.parametrize('M,L,P', [(8, 4, 4), (8, 4, 3)])
def test_msda_prep_backward_optional_outputs_and_repeatable(K, M, L, P):
    a = _prep_check(K, 2, 37, M, L, P, 4, need_offlog=False)
    b = _prep_check(K, 2, 37, M, L, P, 4, need_refs=False)
    c = _prep_check(K, 2, 37, M, L, P, 4)
    assert torch.equal(a[3], c[3]) and torch.equal(b[2], c[2]) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_msda_prep_backward_heads_not_power_of_two_raises(K):
    M, L, P = 3, 2, 2
    offlog, refs, shapes, gloc, gattw = R.msda_case(1, 5, M, L, P, 2)
    with pytest.raises(RuntimeError, match='power of two'):
        K.msda_prep_backward(gloc.cuda(), gattw.cuda(), gattw.cuda(), offlog.cuda(), refs.cuda(), shapes.cuda(), M, L, P)


# ------------------------------------------------------------------- inverse_sigmoid
def test_inverse_sigmoid_fwd_bwd_vs_f64(K):
    x = R.inv_sigmoid_inputs()
    dy = torch.randn(x.numel(), generator=_gen(6))
    y_ref, dx_ref = R.inv_sigmoid_fwd_bwd_ref(x, dy)
    y = K.inverse_sigmoid(x.cuda())
    _within(y, y_ref, 1 + y_ref.abs(), 4, 'inverse_sigmoid')
    dx = K.inverse_sigmoid_backward(dy.cuda(), x.cuda())
    _within(dx, dx_ref, dx_ref.abs(), 8, 'inverse_sigmoid_backward')
    outside = (x < 0) | (x > 1)
    assert outside.any() and (dx.cpu()[outside] == 0).all()
