"""Direct tests of the f32 attention training pair (csrc/attn_train.hip: kinet_mha_train_forward /
kinet_mha_train_backward) against the f64 reference of tests/direct_refs.py, B = 2, H = 2.

The tolerance is the rule of tests/test_grad_norm_attn_gpu.py's attention tests: the yardstick is torch's
CPU f32 evaluation of the same operation, its worst |f32 - f64| / A; the kernels get 4x that on every
element's own magnitude sum A, so where torch's f32 is exact (one key) the kernels must be exact too.
The saved log-sum-exp is held to the same rule against torch.logsumexp (tests/attn_train_refs.py).
Shapes sit around the tiles the plan export reports; dropout masks come from the numpy restatement of
the hash, never from the kernels."""
import pytest
import torch

import attn_train_refs as T

pytestmark = pytest.mark.gpu

B_, H_ = T.B, T.H


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


@pytest.fixture(scope='module')
def N():
    from kinet_amd import _native
    return _native


def _seed(v):
    return torch.tensor([v], dtype=torch.int64, device='cuda')


def _run(K, c):
    """Forward and backward of the new pair on the case's inputs: (o, lse, dq, dk, dv)."""
    q, k, v, do = (c[n].cuda() for n in ('q', 'k', 'v', 'do'))
    km = None if c['km'] is None else c['km'].cuda()
    sd = _seed(c['seed']) if c['p'] > 0 else None
    o, lse = K.mha_train_forward(q, k, v, H_, c['scale'], km, dropout_p=c['p'], seed=sd)
    dq, dk, dv = K.mha_train_backward(q, k, v, o, do, lse, H_, c['scale'], km, dropout_p=c['p'], seed=sd)
    return o, lse, dq, dk, dv


def _case(K, D, shape, mask='none', **kw):
    Lq, Lk = T.shape(K, shape)
    return T.case(D, Lq, Lk, mask, T.tiles(K)[1], **kw), (D, Lq, Lk, mask)


def _verify(K, c, what):
    o, lse, dq, dk, dv = got = _run(K, c)
    wo = T.check([o], c['ref'], ['o'], 4 * c['yard_o'], what)
    wl = T.check_lse(lse, c, what)
    wg = T.check([dq, dk, dv], c['ref'], ['dq', 'dk', 'dv'], 4 * c['yard_g'], what)
    print(f'mha_train {what} p={c["p"]}: o torch CPU f32 err/A {c["yard_o"]:.3e} bound {4 * c["yard_o"]:.3e} kernel '
          f'{wo:.3e}; lse torch {c["lse_yard"]:.3e} bound {4 * c["lse_yard"]:.3e} kernel {wl:.3e}; grads torch '
          f'{c["yard_g"]:.3e} bound {4 * c["yard_g"]:.3e} kernel {wg:.3e}')
    return got


@pytest.mark.parametrize('shape', list(T.SHAPES))
@pytest.mark.parametrize('D', [32, 36])
def test_pair_vs_f64(K, D, shape):
    c, what = _case(K, D, shape)
    got = _verify(K, c, what)
    again = _run(K, c)
    assert all(torch.equal(a, b) for a, b in zip(got, again))      # o, lse, dq, dk, dv: bit-identical reruns


@pytest.mark.parametrize('shape,mask', [('q-1,k+1', 'tail'), ('2q+2,k', 'tail'), ('few,2k+3', 'tail'),
                                        ('q+1,k-1', 'scattered'), ('few,2k+3', 'scattered'),
                                        ('few,2k+3', 'chunk'),
                                        ('few,2k+3', 'key0'), ('q-1,k+1', 'key0'), ('2q+2,k', 'key0'), ('one', 'key0')])
@pytest.mark.parametrize('D', [32, 36])
def test_pair_masked_vs_f64(K, D, shape, mask):
    c, what = _case(K, D, shape, mask)
    _verify(K, c, what)


@pytest.mark.parametrize('shape', ['q+1,k-1', 'few,2k+3'])
@pytest.mark.parametrize('D', [32, 36])
def test_fully_masked_batch(K, D, shape):
    """Batch 1 has no unmasked key: its O rows are zero (what kinet_mha_core_dropout writes), its lse is
    -inf, its gradients exactly zero and finite; batch 0 is within its bounds as usual."""
    c, what = _case(K, D, shape, 'batch')
    o, lse, dq, dk, dv = _verify(K, c, what)
    assert (o[1] == 0).all() and (lse[1] == float('-inf')).all() and torch.isfinite(lse[0]).all()
    for t in (dq, dk, dv):
        assert (t[1] == 0).all() and torch.isfinite(t).all()
        assert (t[0] != 0).any()
    q, k, v = (c[n].cuda() for n in ('q', 'k', 'v'))
    old = K.mha_core(q, k, v, H_, c['scale'], c['km'].cuda(), dropout_p=0.5, seed=_seed(3))
    assert (old[1] == 0).all()                                     # the convention the new forward follows


@pytest.mark.parametrize('D,shape,mask,p,seed', [(36, 'q+1,k-1', 'tail', 0.1, 123456789), (32, '2q+2,k', 'none', 0.5, -1),
                                                 (32, 'few,2k+3', 'tail', 0.1, 7), (36, 'q-1,k+1', 'none', 0.5, 2 ** 40)])
def test_dropout_forward_backward_vs_f64(K, D, shape, mask, p, seed):
    """Keep mask from the restatement at flat index ((b*H + h)*Lq + i)*Lk + j."""
    c, what = _case(K, D, shape, mask, p=p, seed=seed)
    got = _verify(K, c, what)
    assert all(torch.equal(a, b) for a, b in zip(got, _run(K, c)))


@pytest.mark.parametrize('D,shape', [(32, 'q+1,k-1'), (36, 'few,2k+3')])
def test_large_scores(K, D, shape):
    """q scaled by 8: scores of +-30 and more, the max subtraction at work."""
    c, what = _case(K, D, shape, 'tail', qscale=8.0)
    _verify(K, c, what + ('qscale 8',))


def test_old_and_new_pair_share_one_dropout_mask(K):
    """The same seed through kinet_mha_core_dropout / kinet_mha_backward and through the new pair: both
    pass the same f64 check built on the restated keep mask."""
    c, what = _case(K, 32, 'q+1,k-1', 'tail', p=0.1, seed=987654321)
    _verify(K, c, what)
    q, k, v, do = (c[n].cuda() for n in ('q', 'k', 'v', 'do'))
    km, sd = c['km'].cuda(), _seed(c['seed'])
    o = K.mha_core(q, k, v, H_, c['scale'], km, dropout_p=c['p'], seed=sd)
    T.check([o], c['ref'], ['o'], 4 * c['yard_o'], 'old forward')
    T.check(K.mha_backward(q, k, v, do, H_, c['scale'], km, dropout_p=c['p'], seed=sd), c['ref'], ['dq', 'dk', 'dv'],
            4 * c['yard_g'], 'old backward')


@pytest.mark.parametrize('D', [32, 36])
def test_strided_rows_keep_gap_columns(K, N, D):
    """Row strides E + 4 for q / k / v / o (hence dq / dk / dv) through the entry points: results land in
    their E columns, the 4 gap columns keep their fill."""
    c, what = _case(K, D, 'q+1,k-1', 'tail', inseed=4)
    Lq, Lk = what[1], what[2]
    E, fill = H_ * D, 1234.5

    def wide(t):
        w = torch.full((t.shape[0], t.shape[1], E + 4), fill, device='cuda')
        w[..., :E] = t.cuda()
        return w
    qw, kw, vw = wide(c['q']), wide(c['k']), wide(c['v'])
    ow, dqw, dkw, dvw = (torch.full_like(t, fill) for t in (qw, qw, kw, vw))
    dog, kmg = c['do'].cuda(), c['km'].to(torch.uint8).cuda()
    lse = torch.empty(B_, H_, Lq, device='cuda')
    ws = torch.empty(N.lib().kinet_mha_train_backward_workspace(B_, Lq, H_), device='cuda')
    ld, st = E + 4, N.stream(dog.device)
    N.call('kinet_mha_train_forward', N.ptr(qw), ld, N.ptr(kw), ld, N.ptr(vw), ld, N.ptr(ow), ld, N.ptr(lse), B_, Lq, Lk,
           H_, D, float(c['scale']), N.ptr(kmg), 0.0, None, st)
    N.call('kinet_mha_train_backward', N.ptr(qw), ld, N.ptr(kw), ld, N.ptr(vw), ld, N.ptr(ow), ld, N.ptr(dog), E,
           N.ptr(lse), N.ptr(dqw), N.ptr(dkw), N.ptr(dvw), B_, Lq, Lk, H_, D, float(c['scale']), N.ptr(kmg), N.ptr(ws),
           0.0, None, st)
    torch.cuda.synchronize()
    for t in (ow, dqw, dkw, dvw):
        assert (t[..., E:] == fill).all()
    T.check([ow[..., :E]], c['ref'], ['o'], 4 * c['yard_o'], 'strided o')
    T.check_lse(lse, c, 'strided lse')
    T.check([dqw[..., :E], dkw[..., :E], dvw[..., :E]], c['ref'], ['dq', 'dk', 'dv'], 4 * c['yard_g'], 'strided')


def test_other_head_dims_are_refused(K):
    q = torch.zeros(1, 4, 2 * 20, device='cuda')
    with pytest.raises(RuntimeError, match='head_dim 20'):
        K.mha_train_forward(q, q, q, 2, 1.0)
