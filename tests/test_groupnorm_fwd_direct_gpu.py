"""Direct tests of the forward GroupNorm (kinet_groupnorm: stats, finalize and apply kernels of
csrc/ops.hip) against an f64 reference built on the CPU from seeded inputs (direct_refs.gn_fwd_ref).
Bounds are per element, c * 2^-24 * A_i, with c the chain of the path the case takes
(direct_refs.gn_fwd_path restates the dispatch) plus one rounding of a 16-bit output; the
conditioning guards bound the f32 kernel by 4x the error of torch's own CPU f32 group_norm on
x = 30 + randn.  The shapes are the smallest that reach each branch."""
import time

import pytest
import torch

import direct_refs as R

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
EPS = 1e-5
_T0 = time.time()


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    yield kernels
    torch.cuda.synchronize()
    print(f'\ntest_groupnorm_fwd_direct_gpu wall time {time.time() - _T0:.1f} s')


@pytest.fixture(scope='module')
def N():
    from kinet_amd import _native
    return _native


def _within(got, ref, what=''):
    """|got - y| <= y_c u yA (+ one rounding of a 16-bit output), element by element."""
    dtype = got.dtype
    got = got.double().cpu()
    assert got.shape == ref['y'].shape, (what, got.shape, ref['y'].shape)
    assert torch.isfinite(got).all(), what
    tol = ref['y_c'] * R.U32 * ref['yA'] + R.OUT_ROUND[dtype] * ref['y'].abs()
    err = (got - ref['y']).abs()
    bad = err > tol
    assert not bad.any(), (what, int(bad.sum()), err.max().item(), (err / (tol + 1e-300)).max().item())
    return err.max().item()


def _offset_one(t):
    """The same values, contiguous, one element into a device buffer (not 16-byte aligned)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device='cuda')
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def _check(K, shape, dtype, path, seed=0):
    N_, HW, C, G = shape
    assert R.gn_fwd_path(dtype, C, G, HW=HW) == path, (shape, dtype, path)
    x, gamma, beta = R.gn_fwd_case(N_, HW, C, dtype, seed)
    ref = R.gn_fwd_ref(x, gamma, beta, G, EPS, path)
    xg = x.cuda()
    assert xg.data_ptr() % 16 == 0
    y = K.groupnorm_nhwc(xg, gamma.cuda(), beta.cuda(), G, EPS)
    assert y.dtype == dtype and y.shape == x.shape
    _within(y, ref, (shape, dtype, path))
    assert torch.equal(y, K.groupnorm_nhwc(xg, gamma.cuda(), beta.cuda(), G, EPS))      # fixed-order sums
    return y, ref


def _id(v):
    return str(v).replace('torch.', '').replace(' ', '')


@pytest.mark.parametrize('shape,dtype', R.gn_fwd_cases('scalar'), ids=_id)
def test_groupnorm_fwd_scalar_path(K, shape, dtype):
    _check(K, shape, dtype, 'scalar')


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
def test_groupnorm_fwd_misaligned_takes_scalar_path(K, dtype):
    """A vector-path shape read from and written to buffers one element off 16-byte alignment."""
    N_, HW, C, G = 2, 128, 32, 4
    assert R.gn_fwd_path(dtype, C, G, HW=HW) == 'vector' and R.gn_fwd_path(dtype, C, G, aligned=False, HW=HW) == 'scalar'
    x, gamma, beta = R.gn_fwd_case(N_, HW, C, dtype)
    ref = R.gn_fwd_ref(x, gamma, beta, G, EPS, 'scalar')
    for xin, off_out in ((_offset_one(x), False), (x.cuda(), True), (_offset_one(x), True)):
        buf = torch.full((x.numel() + 1,), 7.0, dtype=dtype, device='cuda')
        out = buf[1:].view(x.shape) if off_out else buf[:-1].view(x.shape)
        K.groupnorm_nhwc(xin, gamma.cuda(), beta.cuda(), G, EPS, out=out, out_batch_stride=HW * C)
        _within(out, ref, ('misaligned', dtype, off_out))
        assert buf[0 if off_out else -1].item() == 7.0


@pytest.mark.parametrize('shape,dtype', R.gn_fwd_cases('vector'), ids=_id)
def test_groupnorm_fwd_vector_path(K, shape, dtype):
    _check(K, shape, dtype, 'vector')


@pytest.mark.parametrize('shape,dtype', R.gn_fwd_cases('straddle'), ids=_id)
def test_groupnorm_fwd_straddle_path(K, shape, dtype):
    y, ref = _check(K, shape, dtype, 'straddle')
    N_, HW, C, G = shape
    cg, V = C // G, 4 if dtype == F32 else 8
    # every position of the group boundary inside a vector occurs, and the last group's vectors (their
    # second-group lookup is clamped to the last group) are right on their own
    splits = {(g * cg) % V for g in range(1, G)}
    if shape == (1, 129, 72, 8):
        assert splits == set(range(1, 8))
    assert splits - {0}
    last = slice(C - cg, C)
    tol = (ref['y_c'] * R.U32 * ref['yA'] + R.OUT_ROUND[dtype] * ref['y'].abs())[..., last]
    assert ((y.double().cpu() - ref['y'])[..., last].abs() <= tol).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('pad', [64, 3], ids=['vector-stride', 'odd-stride'])
def test_groupnorm_fwd_into_flat_buffer_keeps_poison(K, dtype, pad):
    """out_batch_stride > HW * C into a poisoned flat buffer: the leading rows and the gaps keep the
    poison bit for bit; a stride that is no multiple of V takes the scalar path and is right too."""
    N_, HW, C, G = 2, 129, 32, 4
    lead, stride = 64, HW * C + pad
    path = R.gn_fwd_path(dtype, C, G, y_stride=stride, HW=HW)
    assert path == ('vector' if pad == 64 else 'scalar')
    x, gamma, beta = R.gn_fwd_case(N_, HW, C, dtype)
    ref = R.gn_fwd_ref(x, gamma, beta, G, EPS, path)
    poison = torch.tensor([-12345.0], dtype=dtype).item()
    flat = torch.full((lead + N_ * stride,), poison, dtype=dtype, device='cuda')
    assert flat[lead:].data_ptr() % 16 == 0
    K.groupnorm_nhwc(x.cuda(), gamma.cuda(), beta.cuda(), G, EPS, out=flat[lead:], out_batch_stride=stride)
    body = flat[lead:].view(N_, stride)
    _within(body[:, :HW * C].reshape(N_, HW, C), ref, ('flat', dtype, pad))
    assert (flat[:lead] == poison).all() and (body[:, HW * C:] == poison).all()


def test_groupnorm_fwd_no_images_leaves_output_untouched(K, N):
    HW, C, G = 40, 32, 4
    gamma, beta = torch.ones(C, device='cuda'), torch.zeros(C, device='cuda')
    x = torch.zeros(0, HW, C, device='cuda')
    assert K.groupnorm_nhwc(x, gamma, beta, G, EPS).shape == (0, HW, C)
    out = torch.full((HW * C,), 7.0, device='cuda')
    ws = torch.full((16,), 7.0, device='cuda')
    N.call('kinet_groupnorm', N.ptr(x), N.ptr(gamma), N.ptr(beta), N.ptr(out), 0, HW, C, G, HW * C, EPS,
           N.dtype_code(F32), N.ptr(ws), N.stream(x.device))
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (ws == 7.0).all()


def test_groupnorm_fwd_eps_is_the_f32_value(K):
    """eps dominates: a constant group (var = 0) gives y = beta exactly, and a group with one value off
    follows rsqrt(var + eps32(eps)), the reference taking eps as the f32 value the kernel receives."""
    N_, HW, C, G = 1, 16, 8, 2
    x = torch.full((N_, HW, C), 3.0)
    x[0, 0, 0] = 4.0
    gamma, beta = torch.full((C,), 2.0), torch.full((C,), 0.5)
    for eps in (0.1, 1e-5):
        ref = R.gn_fwd_ref(x, gamma, beta, G, eps, 'vector')
        y = K.groupnorm_nhwc(x.cuda(), gamma.cuda(), beta.cuda(), G, eps)
        _within(y, ref, ('eps', eps))
        assert (y[0, :, 4:] == 0.5).all()          # the constant group


@pytest.mark.parametrize('N_,HW,C,G,path', R.GN_GUARD)
def test_groupnorm_fwd_offset_conditioning_guard(K, N_, HW, C, G, path):
    """x = 30 + randn in f32: a one-pass variance of raw sums cancels ~900 / 1.  The kernel's maximum
    error against f64 is at most 4x that of torch's CPU f32 group_norm on the same input."""
    assert R.gn_fwd_path(F32, C, G, HW=HW) == path
    x, gamma, beta = R.gn_fwd_case(N_, HW, C, F32, R.GN_GUARD_SEED, R.GN_GUARD_OFFSET)
    ref = R.gn_fwd_ref(x, gamma, beta, G, EPS, path)['y']
    t = (R.gn_fwd_torch_f32(N_, HW, C, G, R.GN_GUARD_SEED, R.GN_GUARD_OFFSET).double() - ref).abs().max().item()
    y = K.groupnorm_nhwc(x.cuda(), gamma.cuda(), beta.cuda(), G, EPS)
    e = (y.double().cpu() - ref).abs().max().item()
    print(f'groupnorm_nhwc offset-30 ({N_}, {HW}, {C}, {G}) f32 {path}: torch CPU f32 max err {t:.3e}, bound '
          f'{4 * t:.3e}, kernel {e:.3e}')
    assert e <= 4 * t, (e, t)
