"""Direct tests of the reductions of csrc/grad.hip -- colsum, LayerNorm / GroupNorm backward,
attention backward -- and of the dropout hash every training kernel shares, against f64 references
built on the CPU from seeded inputs (tests/direct_refs.py).  Bounds are per element,
c * 2^-24 * A_i with A_i the reference's formula on absolute values and c the kernel's longest f32
chain; where a fast exponential or a cancellation cannot be bounded that way, 4x the error of torch's
own CPU f32 evaluation of the same operation.  Dropout masks come from the numpy restatement of the
hash at the documented flat index, never from the kernels."""
import pytest
import torch
import torch.nn.functional as F

import direct_refs as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


@pytest.fixture(scope='module')
def N():
    from kinet_amd import _native
    return _native


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _seed(v):
    return torch.tensor([v], dtype=torch.int64, device='cuda')


def _within(got, ref, A, c, out_dtype=torch.float32, what=''):
    """|got - ref| <= c u A (+ one rounding of a 16-bit output), element by element."""
    got = got.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    tol = c * R.U32 * A + R.OUT_ROUND[out_dtype] * ref.abs()
    err = (got - ref).abs()
    bad = err > tol
    assert not bad.any(), (what, int(bad.sum()), err.max().item(), (err / (tol + 1e-300)).max().item())
    return err.max().item()


# ------------------------------------------------------------------------- dropout hash
@pytest.mark.parametrize('p', [0.0, 0.1, 0.5, 0.999])
@pytest.mark.parametrize('seed', [0, 1, -1, 2 ** 63 - 1, 123456789])
def test_dropout_mask_equals_restatement(K, seed, p):
    n = 100003
    got = K.dropout_mask(_seed(seed), n, p).cpu().bool()
    assert torch.equal(got, R.keep_mask(seed, (n,), p))


@pytest.mark.parametrize('p', [0.1, 0.15, 0.5, 0.999])
def test_dropout_threshold_is_exact(K, p):
    """A threshold off by one moves 2^-24 of the draws: no random seed shows it.  Seeds built by
    inverting the hash put element 5's draw exactly on the threshold (kept) and one below (dropped);
    p = 0.15 is where rounding p to f32 first changes the threshold (2516583, not 2516582)."""
    t = R.dropout_thresh_ref(p)
    for draw, kept in [(t, True), (t - 1, False), (t + 1, True)]:
        seed = R.dropout_seed_for_draw(draw, 5)
        got = K.dropout_mask(_seed(seed), 64, p).cpu().bool()
        assert bool(got[5]) == kept, (p, draw)
        assert torch.equal(got, R.keep_mask(seed, (64,), p))


# ------------------------------------------------------------------------------ colsum
COLSUM_F32 = [(0, 4), (0, 3), (1, 1), (2, 3), (3, 4), (4, 12), (5, 255), (6, 256), (7, 257), (8, 260), (9, 4), (9, 3),
              (63, 12), (64, 257), (65, 256), (127, 260), (128, 12), (128, 3), (128, 256), (16389, 12), (16389, 3)]


def _colsum_check(got, a, out0=None, what=''):
    a64 = a.double()
    ref, A = a64.sum(0), a64.abs().sum(0)
    c = R.colsum_c(a.shape[0])
    if out0 is None:
        return _within(got, ref, A, c, what=what)
    total = out0.double() + ref
    # out0 + s: one more rounding, of a sum whose computed value is within c u A of `total`
    return _within(got, total, c * A + total.abs() + c * R.U32 * A, 1, what=what)


@pytest.mark.parametrize('rows,cols', COLSUM_F32)
def test_colsum_f32_vs_f64(K, rows, cols):
    a = torch.randn(rows, cols, generator=_gen(rows * 1000 + cols))
    got = K.colsum(a.cuda())
    assert got.dtype == torch.float32 and got.shape == (cols,)
    _colsum_check(got, a, what=(rows, cols))
    assert torch.equal(got, K.colsum(a.cuda()))


@pytest.mark.parametrize('rows,cols', [(9, 3), (65, 257), (128, 12), (16389, 4)])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_colsum_16bit_vs_f64(K, dtype, rows, cols):
    a = torch.randn(rows, cols, generator=_gen(rows + cols)).to(dtype)
    got = K.colsum(a.cuda())
    assert got.dtype == torch.float32
    _colsum_check(got, a, what=(dtype, rows, cols))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('width,start', [(17, 4), (20, 4), (20, 1)], ids=['lda17', 'lda20_aligned', 'lda20_offset1'])
def test_colsum_column_slice(K, width, start, dtype):
    """A 12-column slice of a wider matrix: lda % 4 != 0 (scalar kernel), lda % 4 == 0 on an aligned
    base (f32: the vector kernel with lda > cols), and a base one element in (scalar fall-back)."""
    rows, cols = 130, 12
    wide = torch.randn(rows, width, generator=_gen(width + start)).to(dtype)
    src = wide.cuda()[:, start:start + cols]
    assert src.stride(0) == width and src.stride(1) == 1
    if dtype == torch.float32:
        assert (src.data_ptr() % 16 == 0) == (start == 4)
    _colsum_check(K.colsum(src), wide[:, start:start + cols], what=(width, start, dtype))


@pytest.mark.parametrize('rows,cols', [(5, 3), (130, 12), (16389, 4)])
def test_colsum_accumulate(K, rows, cols):
    a = torch.randn(rows, cols, generator=_gen(rows))
    out0 = torch.randn(cols, generator=_gen(cols)) * 10
    out = out0.cuda()
    ret = K.colsum(a.cuda(), out=out, accumulate=True)
    assert ret.data_ptr() == out.data_ptr()
    _colsum_check(out, a, out0=out0, what=(rows, cols))
    assert not torch.equal(out.cpu(), out0)


# -------------------------------------------------------------------- LayerNorm backward
LN_ROWS_CHAIN = 16 + 4 + 1 + 8      # 16 rows per wave serially, 4 waves, the final loop and tree


def _ln_bwd_check(K, x, dy, gamma, dtype, need_params=True):
    rows, d = x.shape
    ref = R.ln_ref(x, gamma, None, 1e-5, dy=dy)
    c = R.ln_c(d, LN_ROWS_CHAIN)
    dx, dg, db = K.layernorm_backward(dy.cuda(), x.cuda(), gamma.cuda(), 1e-5, need_params=need_params)
    assert dx.dtype == dtype and dx.shape == x.shape
    _within(dx, ref['dz'], ref['dzA'], c['dx'], dtype, ('dx', rows, d, dtype))
    if not need_params:
        assert dg is None and db is None
        return dx, dg, db
    assert dg.dtype == db.dtype == torch.float32
    _within(dg, ref['dg'], ref['dgA'], c['dg'], what=('dgamma', rows, d, dtype))
    _within(db, ref['db'], ref['dbA'], c['db'], what=('dbeta', rows, d, dtype))
    return dx, dg, db


@pytest.mark.parametrize('d', [1, 63, 64, 65, 256, 288, 1024])
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
def test_layernorm_backward_vs_f64(K, dtype, d):
    for rows in (1, 63, 64, 65, 129):
        x, dy, gamma, _ = R.ln_case(rows, d, dtype)
        _ln_bwd_check(K, x, dy, gamma, dtype)


def test_layernorm_backward_no_params_and_repeatable(K):
    x, dy, gamma, _ = R.ln_case(65, 288, torch.float32)
    _ln_bwd_check(K, x, dy, gamma, torch.float32, need_params=False)
    a = K.layernorm_backward(dy.cuda(), x.cuda(), gamma.cuda(), 1e-5)
    b = K.layernorm_backward(dy.cuda(), x.cuda(), gamma.cuda(), 1e-5)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_layernorm_backward_too_wide_raises(K):
    x = torch.zeros(2, 1025, device='cuda')
    with pytest.raises(RuntimeError, match='layernorm_backward'):
        K.layernorm_backward(x, x, torch.ones(1025, device='cuda'), 1e-5)


def _poison(n, device='cuda'):
    """Leave a freed block of n floats full of 7.0 in the caching allocator: the next torch.empty of
    that size is likely to hand it back."""
    t = torch.full((n,), 7.0, device=device)
    torch.cuda.synchronize()
    del t


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
def test_layernorm_backward_no_rows_gives_zero_param_grads(K, N, dtype):
    d = 288
    gamma = torch.ones(d, device='cuda')
    x = torch.zeros(0, d, dtype=dtype, device='cuda')
    for _ in range(3):
        _poison(d)
        _poison(d)
        dx, dg, db = K.layernorm_backward(x, x, gamma, 1e-5)
        assert dx.shape == (0, d) and (dg == 0).all() and (db == 0).all()
    # the entry point itself, on pre-filled outputs
    dg, db = torch.full((d,), 7.0, device='cuda'), torch.full((d,), -7.0, device='cuda')
    ws = torch.empty(2 * d, device='cuda')
    N.call('kinet_layernorm_backward', N.ptr(x), N.ptr(x), N.ptr(gamma), N.ptr(x), N.ptr(dg), N.ptr(db), 0, d, 1e-5,
           N.dtype_code(dtype), N.ptr(ws), N.stream(x.device))
    torch.cuda.synchronize()
    assert (dg == 0).all() and (db == 0).all()


@pytest.mark.parametrize('d', [288, 256])
def test_layernorm_backward_offset_rows_cancellation_guard(K, d):
    """x = 100 + randn: mean and variance lose ~100 / 1 of their digits.  dx and dgamma within 4x the
    error of torch's CPU f32 layer_norm backward against f64 on the same input; dbeta (a plain sum)
    within its own bound."""
    rows = 64
    x, dy, gamma, beta = R.ln_case(rows, d, torch.float32, seed=5, offset=100.0)
    ref = R.ln_ref(x, gamma, None, 1e-5, dy=dy)
    xt, gt, bt = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    F.layer_norm(xt, (d,), gt, bt, 1e-5).backward(dy)
    t_dx = (xt.grad.double() - ref['dz']).abs().max().item()
    t_dg = (gt.grad.double() - ref['dg']).abs().max().item()
    dx, dg, db = K.layernorm_backward(dy.cuda(), x.cuda(), gamma.cuda(), 1e-5)
    e_dx = (dx.double().cpu() - ref['dz']).abs().max().item()
    e_dg = (dg.double().cpu() - ref['dg']).abs().max().item()
    print(f'layernorm_backward offset-100 d={d} f32: dx torch CPU f32 max err {t_dx:.3e}, bound {4 * t_dx:.3e}, '
          f'kernel {e_dx:.3e}; dgamma torch {t_dg:.3e}, bound {4 * t_dg:.3e}, kernel {e_dg:.3e}')
    assert e_dx <= 4 * t_dx, (e_dx, t_dx)
    assert e_dg <= 4 * t_dg, (e_dg, t_dg)
    _within(db, ref['db'], ref['dbA'], R.ln_c(d, LN_ROWS_CHAIN)['db'], what='dbeta')


# -------------------------------------------------------------------- GroupNorm backward
GN_SHAPES = [(2, 5, 30, 6), (2, 35, 36, 12), (1, 127, 32, 4), (2, 128, 32, 8), (1, 257, 64, 32), (1, 300, 288, 32),
             (1, 3, 1024, 32), (1, 2, 1028, 4), (1, 40, 8, 8), (2, 40, 8, 1), (1, 66000, 4, 2)]
GN_16BIT = [(2, 35, 36, 12), (1, 257, 64, 32), (1, 300, 288, 32)]


def _gn_check(K, x, dy, gamma, G, dtype, xg=None, dyg=None):
    ref = R.gn_bwd_ref(dy, x, gamma, G, 1e-5)
    dx, dg, db = K.groupnorm_backward(dy.cuda() if dyg is None else dyg, x.cuda() if xg is None else xg, gamma.cuda(),
                                      G, 1e-5)
    assert dx.dtype == dtype and dg.dtype == db.dtype == torch.float32
    what = (tuple(x.shape), G, dtype)
    _within(dx, ref['dx'], ref['dxA'], ref['dx_c'], dtype, ('dx',) + what)
    _within(dg, ref['dg'], ref['dgA'], ref['dg_c'], what=('dgamma',) + what)
    _within(db, ref['db'], ref['dbA'], ref['db_c'], what=('dbeta',) + what)
    return dx, dg, db


@pytest.mark.parametrize('N_,HW,C,G', GN_SHAPES)
def test_groupnorm_backward_f32_vs_f64(K, N_, HW, C, G):
    x, dy, gamma = R.gn_case(N_, HW, C, torch.float32)
    a = _gn_check(K, x, dy, gamma, G, torch.float32)
    b = K.groupnorm_backward(dy.cuda(), x.cuda(), gamma.cuda(), G, 1e-5)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    dx, dg, db = K.groupnorm_backward(dy.cuda(), x.cuda(), gamma.cuda(), G, 1e-5, need_params=False)
    assert dg is None and db is None and torch.equal(dx, a[0])


@pytest.mark.parametrize('N_,HW,C,G', GN_16BIT)
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
def test_groupnorm_backward_16bit_vs_f64(K, dtype, N_, HW, C, G):
    x, dy, gamma = R.gn_case(N_, HW, C, dtype)
    _gn_check(K, x, dy, gamma, G, dtype)


def _offset_one(t):
    """The same values, contiguous, one element into a device buffer (not 16-byte aligned)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device='cuda')
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def test_groupnorm_backward_misaligned_takes_scalar_path(K):
    N_, HW, C, G = 2, 35, 36, 12
    x, dy, gamma = R.gn_case(N_, HW, C, torch.float32)
    _gn_check(K, x, dy, gamma, G, torch.float32, xg=_offset_one(x), dyg=_offset_one(dy))


def test_groupnorm_backward_no_images_gives_zero_param_grads(K, N):
    C, HW, G = 288, 40, 32
    gamma = torch.ones(C, device='cuda')
    x = torch.zeros(0, HW, C, device='cuda')
    for _ in range(3):
        _poison(C)
        _poison(C)
        dx, dg, db = K.groupnorm_backward(x, x, gamma, G, 1e-5)
        assert dx.shape == (0, HW, C) and (dg == 0).all() and (db == 0).all()
    dg, db = torch.full((C,), 7.0, device='cuda'), torch.full((C,), -7.0, device='cuda')
    ws = torch.empty(16, device='cuda')
    N.call('kinet_groupnorm_backward', N.ptr(x), N.ptr(x), N.ptr(gamma), N.ptr(x), N.ptr(dg), N.ptr(db), 0, HW, C, G,
           1e-5, N.dtype_code(torch.float32), N.ptr(ws), N.stream(x.device))
    torch.cuda.synchronize()
    assert (dg == 0).all() and (db == 0).all()


def test_groupnorm_backward_offset_conditioning_guard(K):
    """x = 30 + randn on (2, 200, 32, 4): the one-pass variance E[x^2] - mean^2 cancels ~900 / 1.
    dx and dgamma within 4x the error of torch's CPU f32 group_norm backward against f64; dbeta (a
    plain sum) within its own bound."""
    N_, HW, C, G = 2, 200, 32, 4
    x, dy, gamma = R.gn_case(N_, HW, C, torch.float32, seed=3, offset=30.0)
    ref = R.gn_bwd_ref(dy, x, gamma, G, 1e-5)
    xt = x.permute(0, 2, 1).contiguous().requires_grad_()       # (N, C, HW)
    gt, bt = gamma.clone().requires_grad_(), torch.zeros(C, requires_grad=True)
    F.group_norm(xt, G, gt, bt, 1e-5).backward(dy.permute(0, 2, 1).contiguous())
    t_dx = (xt.grad.permute(0, 2, 1).double() - ref['dx']).abs().max().item()
    t_dg = (gt.grad.double() - ref['dg']).abs().max().item()
    dx, dg, db = K.groupnorm_backward(dy.cuda(), x.cuda(), gamma.cuda(), G, 1e-5)
    e_dx = (dx.double().cpu() - ref['dx']).abs().max().item()
    e_dg = (dg.double().cpu() - ref['dg']).abs().max().item()
    print(f'groupnorm_backward offset-30 (2, 200, 32, 4) f32: dx torch CPU f32 max err {t_dx:.3e}, bound '
          f'{4 * t_dx:.3e}, kernel {e_dx:.3e}; dgamma torch {t_dg:.3e}, bound {4 * t_dg:.3e}, kernel {e_dg:.3e}')
    assert e_dx <= 4 * t_dx, (e_dx, t_dx)
    assert e_dg <= 4 * t_dg, (e_dg, t_dg)
    _within(db, ref['db'], ref['dbA'], ref['db_c'], what='dbeta')


# -------------------------------------------------------------------- attention backward
B_, H_ = 2, 2


def _mask(kind, Lk):
    """key_mask (B, Lk) bool, True = masked."""
    if kind == 'none':
        return None
    m = torch.zeros(B_, Lk, dtype=torch.bool)
    if kind == 'tail':
        m[1, Lk - max(1, Lk // 3):] = True
    elif kind == 'scattered':
        m[:] = torch.rand(B_, Lk, generator=_gen(Lk)) < 0.4
        m[:, Lk // 2] = False
    elif kind == 'chunk':                     # keys 64..127 all masked
        m[:, 64:128] = True
    elif kind == 'key0':                      # only key 0 left
        m[:, 1:] = True
    elif kind == 'batch':                     # batch 1 fully masked
        m[1] = True
    return m


def _attn_bounds(ref, f32, names):
    """The fast exponential has no clean bound: the yardstick is torch's CPU f32 evaluation of the same
    operation, its worst |f32 - f64| / A over the named tensors; the kernel gets 4x that on every
    element's own A (where torch's f32 is exact -- one key -- so must the kernel be)."""
    yard = R.attn_yardstick(ref, f32, names)
    return yard, 4 * yard


def _attn_check(got, ref, names, factor, what):
    worst = 0.0
    for n, t in zip(names, got):
        t = t.double().cpu()
        assert torch.isfinite(t).all(), (n, what)
        err, tol = (t - ref[n]).abs(), factor * ref[n + 'A']
        bad = err > tol
        assert not bad.any(), (n, what, int(bad.sum()), err.max().item(), (err / (tol + 1e-300)).max().item())
        ok = ref[n + 'A'] > 0
        if ok.any():
            worst = max(worst, (err[ok] / ref[n + 'A'][ok]).max().item())
    return worst


def _attn_bwd_case(K, D, Lq, Lk, mask='none', p=0.0, seed=None, qscale=1.0, forward=False):
    q, k, v, do = R.attn_case(B_, H_, D, Lq, Lk, qscale=qscale)
    km = _mask(mask, Lk)
    keep = R.keep_mask(seed, (B_, H_, Lq, Lk), p) if p > 0 else None
    scale = D ** -0.5
    ref = R.attn_ref(q, k, v, do, H_, scale, km, keep, p)
    f32 = R.attn_ref(q, k, v, do, H_, scale, km, keep, p, dtype=torch.float32)
    names = ['dq', 'dk', 'dv']
    yard, factor = _attn_bounds(ref, f32, names)
    kmg = None if km is None else km.cuda()
    sd = _seed(seed) if p > 0 else None
    got = K.mha_backward(q.cuda(), k.cuda(), v.cuda(), do.cuda(), H_, scale, kmg, dropout_p=p, seed=sd)
    worst = _attn_check(got, ref, names, factor, (D, Lq, Lk, mask, p))
    msg = (f'mha_backward D={D} {Lq}x{Lk} mask={mask} p={p} qscale={qscale}: torch CPU f32 err/A {yard:.3e}, '
           f'bound/A {factor:.3e}, kernel err/A {worst:.3e}')
    if forward:
        yo, fo = _attn_bounds(ref, f32, ['o'])
        o = K.mha_core(q.cuda(), k.cuda(), v.cuda(), H_, scale, kmg, dropout_p=p, seed=sd)
        wo = _attn_check([o], ref, ['o'], fo, ('o', D, Lq, Lk, mask, p))
        msg += f'; forward o: torch {yo:.3e}, bound {fo:.3e}, kernel {wo:.3e}'
    print(msg)
    return got, ref, (q, k, v, do, kmg)


@pytest.mark.parametrize('D,Lq,Lk', [(20, 1, 1), (30, 65, 63), (32, 64, 130), (33, 130, 64), (36, 7, 200), (40, 65, 63),
                                      (48, 64, 130), (64, 7, 200), (64, 130, 64), (36, 1, 1)])
def test_mha_backward_vs_f64(K, D, Lq, Lk):
    got, _, (q, k, v, do, _) = _attn_bwd_case(K, D, Lq, Lk)
    again = K.mha_backward(q.cuda(), k.cuda(), v.cuda(), do.cuda(), H_, D ** -0.5)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize('D,Lq,Lk,mask', [(30, 65, 63, 'tail'), (33, 130, 64, 'tail'), (64, 64, 130, 'tail'),
                                           (32, 64, 130, 'scattered'), (48, 7, 200, 'scattered'),
                                           (36, 7, 200, 'chunk'), (64, 7, 200, 'chunk'),
                                           (36, 7, 200, 'key0'), (40, 65, 63, 'key0'), (20, 130, 64, 'key0')])
def test_mha_backward_masked_vs_f64(K, D, Lq, Lk, mask):
    _attn_bwd_case(K, D, Lq, Lk, mask=mask)


@pytest.mark.parametrize('D,Lq,Lk', [(36, 65, 63), (64, 7, 200), (20, 64, 130)])
def test_mha_backward_fully_masked_batch_is_exact_zero(K, D, Lq, Lk):
    """Batch 1 has no unmasked key: P = 0 there, so dq / dk / dv are exactly zero (and finite); batch 0
    is within its bounds as usual."""
    got, ref, _ = _attn_bwd_case(K, D, Lq, Lk, mask='batch')
    for t in got:
        assert (t[1] == 0).all() and torch.isfinite(t).all()
        assert (t[0] != 0).any()


@pytest.mark.parametrize('D,Lq,Lk,mask,p,seed', [(36, 65, 63, 'tail', 0.1, 123456789), (64, 64, 130, 'none', 0.5, -1)])
def test_mha_dropout_forward_backward_vs_f64(K, D, Lq, Lk, mask, p, seed):
    """Keep mask from the restatement at flat index ((b*H + h)*Lq + i)*Lk + j, on the f32 forward
    (mha_core) and the backward."""
    _attn_bwd_case(K, D, Lq, Lk, mask=mask, p=p, seed=seed, forward=True)


@pytest.mark.parametrize('D,Lq,Lk', [(32, 65, 63), (64, 64, 130)])
def test_mha_backward_large_scores(K, D, Lq, Lk):
    """q scaled by 8: scores of +-30 and more, the max subtraction at work."""
    _attn_bwd_case(K, D, Lq, Lk, mask='tail', qscale=8.0)


def test_mha_backward_qk_packed_odd_length(K):
    D, L = 36, 65
    E = H_ * D
    q, k, v, do = R.attn_case(B_, H_, D, L, L, seed=9)
    km = _mask('tail', L)
    scale = D ** -0.5
    ref = R.attn_ref(q, k, v, do, H_, scale, km)
    f32 = R.attn_ref(q, k, v, do, H_, scale, km, dtype=torch.float32)
    yard, factor = _attn_bounds(ref, f32, ['dq', 'dk', 'dv'])
    dqk, dv = K.mha_backward_qk(torch.cat([q, k], -1).cuda(), v.cuda(), do.cuda(), H_, scale, km.cuda())
    assert dqk.shape == (B_, L, 2 * E)
    worst = _attn_check([dqk[..., :E], dqk[..., E:], dv], ref, ['dq', 'dk', 'dv'], factor, 'qk')
    print(f'mha_backward_qk D=36 L=65 tail mask: torch CPU f32 err/A {yard:.3e}, bound/A {factor:.3e}, '
          f'kernel err/A {worst:.3e}')


def test_mha_backward_strided_rows_keep_gap_columns(K, N):
    """Row strides E + 4 for q / k / v (hence dq / dk / dv) through the entry point: the gradients land
    in their E columns, the 4 gap columns keep their fill."""
    D, Lq, Lk = 33, 65, 63
    E, fill = H_ * D, 1234.5
    q, k, v, do = R.attn_case(B_, H_, D, Lq, Lk, seed=4)
    km = _mask('tail', Lk)
    scale = D ** -0.5
    ref = R.attn_ref(q, k, v, do, H_, scale, km)
    f32 = R.attn_ref(q, k, v, do, H_, scale, km, dtype=torch.float32)
    _, factor = _attn_bounds(ref, f32, ['dq', 'dk', 'dv'])

    def wide(t):
        w = torch.full((t.shape[0], t.shape[1], E + 4), fill, device='cuda')
        w[..., :E] = t.cuda()
        return w
    qw, kw, vw = wide(q), wide(k), wide(v)
    dqw, dkw, dvw = (torch.full_like(t, fill) for t in (qw, kw, vw))
    dog, kmg = do.cuda(), km.to(torch.uint8).cuda()
    ws = torch.empty(N.lib().kinet_mha_backward_workspace(B_, Lq, Lk, H_), device='cuda')
    N.call('kinet_mha_backward', N.ptr(qw), E + 4, N.ptr(kw), E + 4, N.ptr(vw), E + 4, N.ptr(dog), E, N.ptr(dqw),
           N.ptr(dkw), N.ptr(dvw), B_, Lq, Lk, H_, D, float(scale), N.ptr(kmg), N.ptr(ws), 0.0, None,
           N.stream(dog.device))
    torch.cuda.synchronize()
    for t in (dqw, dkw, dvw):
        assert (t[..., E:] == fill).all()
    _attn_check([dqw[..., :E], dkw[..., :E], dvw[..., :E]], ref, ['dq', 'dk', 'dv'], factor, 'strided')
