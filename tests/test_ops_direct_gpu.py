"""Direct tests of the small kernels of csrc/ops.hip -- sine position embedding, box refine,
LayerNorm, add -- against plain f64 restatements of the same operations (tests/direct_refs.py,
itself checked on the CPU by test_direct_refs_cpu.py).  Seeded inputs, small shapes chosen at the
kernels' edges (lane splits, block tails, vector / scalar thresholds, misaligned pointers)."""
import functools

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


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ sine position embedding
GEO = R.sine_geometries()
MODES = {'2d': (False, 0, 1), '3d_f0of2': (True, 0, 2), '3d_f1of2': (True, 1, 2), '3d_f1of3': (True, 1, 3)}
# f32 output: 5e-6 absolute.  The same arithmetic evaluated step by step in f32 differs from the
# f64 one by <= 6e-7 at every compared position of the main masks (test_direct_refs_cpu.py measures
# it); the kernel's f32 arithmetic is of the same nature: a margin of ~8x.
SINE_ATOL = 5e-6


@functools.lru_cache(maxsize=None)
def _sine_ref(name, npf, mode, normalize):
    three_d, frame, frames = MODES[mode]
    return R.sine_embed_ref(GEO[name], npf, three_d, frame, frames, normalize)


def _level_embed(C):
    return torch.randn(C, generator=_gen(C))


def _check_sine(got, name, npf, mode, normalize, le, dtype):
    """Compared positions within the tolerance; the excluded (pixel, axis) pairs of the 2-d
    normalised case finite and bounded by 1 + |level_embed|."""
    three_d = MODES[mode][0]
    mask = GEO[name]
    ref = _sine_ref(name, npf, mode, normalize)
    lev = le.double() if le is not None else torch.zeros(ref.shape[-1], dtype=torch.float64)
    ref = ref + lev
    keep = R.sine_compared(mask, npf, three_d, normalize)
    got = got.double().cpu()
    assert got.shape == ref.shape
    assert torch.isfinite(got).all()
    # 16-bit output: one rounding of the output (half an ulp, doubled) on top of the f32 bound
    tol = R.OUT_ROUND[dtype] * ref.abs() + SINE_ATOL
    err = (got - ref).abs()
    bad = (err > tol) & keep
    assert not bad.any(), (name, npf, mode, normalize, dtype, err[keep].max().item())
    # every position, the excluded ones included: |sin| <= 1 plus the level embedding (and the
    # rounding of that sum / of the output)
    bound = (1 + lev.abs()) * (1 + R.OUT_ROUND[dtype] + 2.0 ** -23)
    assert (got.abs() <= bound).all()
    if not (normalize and not three_d):
        assert keep.all()
    return err[keep].max().item() if keep.any() else 0.0


@pytest.mark.parametrize('normalize', [True, False], ids=['norm', 'raw'])
@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('name', sorted(GEO))
def test_sine_position_embed_vs_f64(K, name, mode, normalize):
    three_d, frame, frames = MODES[mode]
    mask = GEO[name].cuda()
    if normalize and not three_d:
        share = R.sine_excluded_share(GEO[name])
        for b in range(mask.shape[0]):
            if (name, b) not in R.FULLY_MASKED:       # compared in 3-d and un-normalised mode instead
                assert share[b].item() <= 0.25
    worst = 0.0
    for npf in (128, 144, 96):
        C = (3 if three_d else 2) * npf
        dim_t = R.sine_dim_t(npf).cuda()
        for le in (None, _level_embed(C)):
            for dtype in DTYPES:
                got = K.sine_position_embed(mask, dim_t, npf, three_d, frame, frames, normalize, 2 * torch.pi,
                                            le.cuda() if le is not None else None, out_dtype=dtype)
                assert got.dtype == dtype
                e = _check_sine(got, name, npf, mode, normalize, le, dtype)
                if dtype == torch.float32:
                    worst = max(worst, e)
    print(f'sine {name} {mode} normalize={normalize}: max f32 err {worst:.3e}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mode', ['2d', '3d_f1of2'])
def test_sine_position_embed_into_flat_buffer(K, mode, dtype):
    """out= a slice of a larger zero-filled (B, S_total, C) buffer at a batch stride: the rows
    before and after the slice stay exactly zero."""
    three_d, frame, frames = MODES[mode]
    npf, name = 96, 'main'
    mask = GEO[name]
    B, H, W = mask.shape
    C = (3 if three_d else 2) * npf
    S_total, off = H * W + 57, 31
    le = _level_embed(C)
    flat = torch.zeros(B, S_total, C, dtype=dtype, device='cuda')
    ret = K.sine_position_embed(mask.cuda(), R.sine_dim_t(npf).cuda(), npf, three_d, frame, frames, True, 2 * torch.pi,
                                le.cuda(), out=flat[:, off:], out_batch_stride=S_total * C)
    torch.cuda.synchronize()
    assert ret.data_ptr() == flat[:, off:].data_ptr()
    assert (flat[:, :off] == 0).all() and (flat[:, off + H * W:] == 0).all()
    _check_sine(flat[:, off:off + H * W], name, npf, mode, True, le, dtype)


def test_sine_position_embed_bad_frame_raises(K):
    mask = GEO['3x2'].cuda()
    dim_t = R.sine_dim_t(96).cuda()
    for frame, frames in ((2, 2), (3, 2), (1, 1)):
        with pytest.raises(RuntimeError, match='frame'):
            K.sine_position_embed(mask, dim_t, 96, True, frame, frames)


# ------------------------------------------------------------------------------ box refine
# 1e-5 absolute on both outputs: __expf has relative error <~ |t| 6e-8 + 1.2e-7 (<= 2e-6 for
# |t| <= 30), the sigmoid's sensitivity to it is <= 0.25, logf and the division add ~1e-7 |t| in
# the argument: < 2e-6 in total, a 5x margin.
BOX_ATOL = 1e-5


@pytest.mark.parametrize('rd', [2, 4])
@pytest.mark.parametrize('L', [1, 4])
@pytest.mark.parametrize('Q', [1, 255, 257, 300])
@pytest.mark.parametrize('B', [1, 3])
def test_box_refine_vs_f64(K, B, Q, L, rd):
    tmp, ref, vr = R.box_case(B, Q, L, rd)
    new_ref, rin_ref = R.box_refine_ref(tmp, ref, vr)
    new, rin = K.box_refine(tmp.cuda(), ref.cuda(), vr.cuda())
    torch.cuda.synchronize()
    assert new.shape == (B, Q, 4) and rin.shape == (B, Q, L, 4)
    e_new = (new.double().cpu() - new_ref).abs().max().item()
    e_rin = (rin.double().cpu() - rin_ref).abs().max().item()
    assert e_new <= BOX_ATOL, e_new
    assert e_rin <= BOX_ATOL, e_rin
    # want_input=False: no second output, the same new_ref
    new2, none = K.box_refine(tmp.cuda(), ref.cuda(), None, want_input=False)
    assert none is None
    assert torch.equal(new2, new)


@pytest.mark.parametrize('rd', [2, 4])
def test_box_refine_out_slice(K, rd):
    B, Q, L = 3, 257, 4
    tmp, ref, vr = R.box_case(B, Q, L, rd)
    new_ref, _ = R.box_refine_ref(tmp, ref, vr)
    buf = torch.full((3, B, Q, 4), -7.0, device='cuda')
    new, rin = K.box_refine(tmp.cuda(), ref.cuda(), vr.cuda(), out=buf[1])
    torch.cuda.synchronize()
    assert new.data_ptr() == buf[1].data_ptr()
    assert (buf[0] == -7.0).all() and (buf[2] == -7.0).all()
    assert (buf[1].double().cpu() - new_ref).abs().max().item() <= BOX_ATOL


# ------------------------------------------------------------------------------ layernorm
LN_DIMS = [8, 36, 90, 256, 288, 512, 1024]
LN_ROWS = [1, 5, 777]


def _ln_inputs(rows, d, dtype, seed=0):
    g = _gen(seed + rows * 1031 + d)
    x = torch.randn(rows, d, generator=g).to(dtype)
    r = torch.randn(rows, d, generator=g).to(dtype)
    gamma = torch.rand(d, generator=g) + 0.5
    beta = torch.randn(d, generator=g)
    return x, r, gamma, beta


def _ln_tol(ref, gamma, dtype):
    # f32 math: element-wise 1e-5 (|ref| + max|gamma|); 16-bit output: plus one output rounding
    return 1e-5 * (ref.abs() + gamma.abs().max().item()) + R.OUT_ROUND[dtype] * ref.abs()


def _offset_view(t, lead=1):
    """The same values in a view that starts `lead` elements into a larger buffer (4- or 2-byte
    aligned only): kinet_layernorm must fall back to the scalar kernel."""
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=t.device)
    v = buf[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


@pytest.mark.parametrize('d', LN_DIMS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_layernorm_vs_f64(K, dtype, d):
    for rows in LN_ROWS:
        x, r, gamma, beta = _ln_inputs(rows, d, dtype)
        xg, rg, gg, bg = x.cuda(), r.cuda(), gamma.cuda(), beta.cuda()
        for res in (None, r):
            ref = R.layernorm_ref(x, gamma, beta, 1e-5, res)
            tol = _ln_tol(ref, gamma, dtype)
            y = K.layernorm(xg, gg, bg, residual=rg if res is not None else None)
            assert y.dtype == dtype and y.shape == x.shape
            err = (y.double().cpu() - ref).abs()
            assert (err <= tol).all(), (rows, res is not None, (err / tol).max().item())
            # out=: written in place, same values
            out = torch.full_like(xg, 3.0)
            ret = K.layernorm(xg, gg, bg, residual=rg if res is not None else None, out=out)
            assert ret.data_ptr() == out.data_ptr()
            assert torch.equal(out, y)
            if R.layernorm_vec_eligible(dtype, d):
                # misaligned x: the scalar kernel; sums in another order, so equal to rounding only
                y_s = K.layernorm(_offset_view(xg), gg, bg, residual=rg if res is not None else None)
                err_s = (y_s.double().cpu() - ref).abs()
                assert (err_s <= tol).all(), (rows, 'scalar', (err_s / tol).max().item())
                # the two kernels agree within the tolerance; two 16-bit roundings of nearly equal
                # f32 values can land one ulp apart (2 OUT_ROUND |ref|): one more output rounding
                agree = tol + R.OUT_ROUND[dtype] * ref.abs()
                diff = (y_s.double() - y.double()).abs().cpu()
                assert (diff <= agree).all(), (rows, 'vec vs scalar', (diff / agree).max().item())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('which', ['x', 'out', 'residual'])
def test_layernorm_misaligned_pointer_takes_scalar_kernel(K, dtype, which):
    """d = 256 is vector-eligible in every dtype; a view one element into a larger buffer (x, out
    or the residual) must still give the right rows, and leave the buffer's other elements alone."""
    rows, d = 37, 256
    x, r, gamma, beta = _ln_inputs(rows, d, dtype, seed=5)
    ref = R.layernorm_ref(x, gamma, beta, 1e-5, r)
    tol = _ln_tol(ref, gamma, dtype)
    xg, rg = x.cuda(), r.cuda()
    out = None
    if which == 'x':
        xg = _offset_view(xg)
    elif which == 'residual':
        rg = _offset_view(rg)
    else:
        buf = torch.full((rows * d + 16,), 9.0, dtype=dtype, device='cuda')
        out = buf[1:1 + rows * d].view(rows, d)
    y = K.layernorm(xg, gamma.cuda(), beta.cuda(), residual=rg, out=out)
    torch.cuda.synchronize()
    err = (y.double().cpu() - ref).abs()
    assert (err <= tol).all(), (err / tol).max().item()
    if which == 'out':
        assert buf[0].item() == 9.0 and (buf[1 + rows * d:] == 9.0).all()


def test_layernorm_offset_rows_cancellation_guard(K):
    """x = 100 + randn at d = 288 (f32, scalar kernel): a one-pass E[x^2] - mean^2 variance loses
    ~1e4 * 2^-24 / 1 of the variance here and misses by orders of magnitude.  The bound is torch's
    own CPU f32 layer_norm error against f64 on the same input, x4, floor 1e-5 -- never the
    kernel's own output."""
    rows, d = 64, 288
    g = _gen(11)
    x = 100 + torch.randn(rows, d, generator=g)
    gamma = torch.rand(d, generator=g) + 0.5
    beta = torch.randn(d, generator=g)
    ref = R.layernorm_ref(x, gamma, beta)
    torch_err = (F.layer_norm(x, (d,), gamma, beta).double() - ref).abs().max().item()
    bound = max(4 * torch_err, 1e-5)
    y = K.layernorm(x.cuda(), gamma.cuda(), beta.cuda())
    err = (y.double().cpu() - ref).abs().max().item()
    print(f'layernorm offset-100 d=288 f32: torch CPU f32 max err {torch_err:.3e}, bound {bound:.3e}, '
          f'kernel max err {err:.3e}')
    assert err <= bound, (err, bound)
    # same guard on the vector kernel (d = 256)
    x2 = x[:, :256].contiguous()
    ref2 = R.layernorm_ref(x2, gamma[:256], beta[:256])
    torch_err2 = (F.layer_norm(x2, (256,), gamma[:256], beta[:256]).double() - ref2).abs().max().item()
    err2 = (K.layernorm(x2.cuda(), gamma[:256].cuda(), beta[:256].cuda()).double().cpu() - ref2).abs().max().item()
    print(f'layernorm offset-100 d=256 f32: torch CPU f32 max err {torch_err2:.3e}, kernel max err {err2:.3e}')
    assert err2 <= max(4 * torch_err2, 1e-5), (err2, torch_err2)


def test_layernorm_too_wide_raises(K):
    x = torch.zeros(2, 1025, device='cuda')
    w = torch.ones(1025, device='cuda')
    with pytest.raises(RuntimeError, match='1024'):
        K.layernorm(x, w, w)


# ------------------------------------------------------------------------------------ add
@pytest.mark.parametrize('n', [1, 255, 1000003])
@pytest.mark.parametrize('dtype', DTYPES)
def test_add_bit_exact(K, dtype, n):
    g = _gen(n)
    a = torch.randn(n, generator=g).to(dtype)
    b = (torch.randn(n, generator=g) * 3).to(dtype)
    ref = a + b                                      # torch on the CPU: f32 sum, one rounding
    y = K.add(a.cuda(), b.cuda())
    assert y.dtype == dtype
    assert torch.equal(y.cpu(), ref)
    out = torch.zeros(n + 2, dtype=dtype, device='cuda')
    ret = K.add(a.cuda(), b.cuda(), out=out[1:n + 1])
    assert ret.data_ptr() == out[1:].data_ptr()
    assert torch.equal(out[1:n + 1].cpu(), ref)
    assert out[0].item() == 0 and out[n + 1].item() == 0


def test_add_grid_stride_loop(K):
    """n = 4 * 2^20 + 3: more elements than the capped grid has threads, so the loop iterates."""
    n = 4 * 2 ** 20 + 3
    g = _gen(7)
    a = torch.randn(n, generator=g)
    b = torch.randn(n, generator=g)
    y = K.add(a.cuda(), b.cuda())
    assert torch.equal(y.cpu(), a + b)
