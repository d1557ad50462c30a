"""Helpers of the direct tests of the f32 attention training pair (csrc/attn_train.hip,
tests/test_attn_train_direct_gpu.py): the shapes around the kernels' tiles, the key masks, the f64
reference of the saved log-sum-exp, and the shared case cache.  The attention reference itself, its
majorants, the seeded inputs and the dropout keep mask are those of tests/direct_refs.py."""
import functools

import torch

import direct_refs as R

B, H = 2, 2

# the shapes of the tests by name, from the tile sizes the plan export reports (never hard-coded)
SHAPES = {
    'one': lambda qt, kt: (1, 1),
    'q-1,k+1': lambda qt, kt: (qt - 1, kt + 1),
    'q+1,k-1': lambda qt, kt: (qt + 1, kt - 1),
    'few,2k+3': lambda qt, kt: (7, 2 * kt + 3),
    '2q+2,k': lambda qt, kt: (2 * qt + 2, kt),
}


def tiles(K):
    """(queries, keys) per tile of the training pair, from kinet_mha_train_plan."""
    p = K.mha_train_plan(32, 1, 1, 1, 1)
    return p['qt'], p['kt']


def shape(K, name):
    return SHAPES[name](*tiles(K))


def key_mask(kind, Lk, kt):
    """key_mask (B, Lk) bool, True = masked: the kinds of tests/test_grad_norm_attn_gpu.py's _mask, with
    'chunk' as one whole key tile (keys kt .. 2 kt - 1) masked."""
    if kind == 'none':
        return None
    m = torch.zeros(B, Lk, dtype=torch.bool)
    if kind == 'tail':
        m[1, Lk - max(1, Lk // 3):] = True
    elif kind == 'scattered':
        m[:] = torch.rand(B, Lk, generator=torch.Generator().manual_seed(Lk)) < 0.4
        m[:, Lk // 2] = False
    elif kind == 'chunk':
        assert Lk >= 2 * kt
        m[:, kt:2 * kt] = True
    elif kind == 'key0':
        m[:, 1:] = True
    elif kind == 'batch':
        m[1] = True
    else:
        raise ValueError(kind)
    return m


def lse_ref(q, k, heads, scale, km, dtype=torch.float64):
    """lse (B, heads, Lq) = log sum_j exp(scale q_i . k_j) over the unmasked keys (-inf without one) in
    plain torch ops at `dtype`, and at f64 its majorant A: the sum of the magnitudes that enter the value,
        A_i = sum_j P_ij * scale * sum_d |q_id| |k_jd|   (d lse / d s_j = P_ij, s_j a D-term dot product)
              + |lse_i| + 1                               (the max that is subtracted and added back; the
                                                           relative error of the sum inside the log).
    |m| + 1 alone misses scores that are small differences of large products."""
    Bq, Lq, E = q.shape
    D = E // heads

    def sp(t):
        return t.to(dtype).view(Bq, -1, heads, D).transpose(1, 2)
    Q, K_ = sp(q), sp(k)
    S = Q @ K_.transpose(-1, -2) * scale
    if km is not None:
        S = S.masked_fill(km[:, None, None, :], float('-inf'))
    lse = torch.logsumexp(S, -1)
    if dtype != torch.float64:
        return lse, None
    P = torch.where(torch.isinf(lse)[..., None], torch.zeros_like(S), (S - lse[..., None]).exp())
    P = torch.nan_to_num(P, nan=0.0)
    SA = Q.abs() @ K_.abs().transpose(-1, -2) * scale
    A = (P * SA).sum(-1) + torch.where(torch.isinf(lse), torch.zeros_like(lse), lse.abs()) + 1.0
    return lse, A


@functools.lru_cache(maxsize=None)
def case(D, Lq, Lk, mask, kt, p=0.0, seed=None, qscale=1.0, inseed=0):
    """One seeded problem with everything the tests compare against, computed once: inputs, key mask,
    keep mask, the f64 reference with majorants, torch's CPU f32 evaluation (the yardstick: the kernels
    get 4x its worst |f32 - f64| / A, element by element on the element's own A), the same for lse."""
    q, k, v, do = R.attn_case(B, H, D, Lq, Lk, seed=inseed, qscale=qscale)
    km = key_mask(mask, Lk, kt)
    keep = R.keep_mask(seed, (B, H, Lq, Lk), p) if p > 0 else None
    scale = D ** -0.5
    ref = R.attn_ref(q, k, v, do, H, scale, km, keep, p)
    f32 = R.attn_ref(q, k, v, do, H, scale, km, keep, p, dtype=torch.float32)
    lse64, lseA = lse_ref(q, k, H, scale, km)
    lse32, _ = lse_ref(q, k, H, scale, km, dtype=torch.float32)
    fin = torch.isfinite(lse64)
    assert torch.equal(fin, torch.isfinite(lse32))
    lse_yard = ((lse32.double() - lse64).abs()[fin] / lseA[fin]).max().item() if fin.any() else 0.0
    return dict(q=q, k=k, v=v, do=do, km=km, keep=keep, scale=scale, ref=ref, f32=f32, p=p, seed=seed,
                yard_o=R.attn_yardstick(ref, f32, ['o']), yard_g=R.attn_yardstick(ref, f32, ['dq', 'dk', 'dv']),
                lse=lse64, lseA=lseA, lse_yard=lse_yard)


def check(got, ref, names, factor, what):
    """Every element of every named tensor within factor * its own A; returns the worst err / A."""
    worst = 0.0
    for n, t in zip(names, got):
        t = t.double().cpu()
        assert t.shape == ref[n].shape, (n, what, t.shape)
        assert torch.isfinite(t).all(), (n, what)
        err, tol = (t - ref[n]).abs(), factor * ref[n + 'A']
        bad = err > tol
        assert not bad.any(), (n, what, int(bad.sum()), err.max().item(), (err / (tol + 1e-300)).max().item())
        ok = ref[n + 'A'] > 0
        if ok.any():
            worst = max(worst, (err[ok] / ref[n + 'A'][ok]).max().item())
    return worst


def check_lse(got, c, what):
    """-inf exactly where the reference has no unmasked key, elsewhere within 4x the yardstick on A."""
    got = got.double().cpu()
    fin = torch.isfinite(c['lse'])
    assert got.shape == c['lse'].shape, (what, got.shape)
    assert (got[~fin] == float('-inf')).all(), what
    assert torch.isfinite(got[fin]).all(), what
    if not fin.any():
        return 0.0
    ratio = (got - c['lse']).abs()[fin] / c['lseA'][fin]
    assert (ratio <= 4 * c['lse_yard']).all(), (what, ratio.max().item(), c['lse_yard'])
    return ratio.max().item()
