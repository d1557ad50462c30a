"""kinet_stem_pool_image: the ResNet stem (7x7 / 2 conv + folded BN + ReLU from the f32 image)
and the 3x3 / 2 max-pool as one launch, against the two launches it replaces (bit for bit),
against torch fp32, and inside the ResNet body."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SMALL = [(1, 9, 7), (1, 37, 41), (2, 50, 66), (1, 70, 300), (1, 130, 250)]
DTYPES = [torch.bfloat16, torch.float16]


def _rel(a, b):
    return ((a.float().cpu() - b.float().cpu()).abs().max() / (b.float().abs().max() + 1e-6)).item()


@functools.lru_cache(maxsize=None)
def _case(B, H, W, dtype, big_bias=False):
    """Inputs as in test_stem_conv_image_equals_folded_path and the two-launch result, computed
    once per (shape, dtype) and shared (nothing modifies them)."""
    from kinet_amd import kernels as K
    g = torch.Generator().manual_seed(H * W + B)
    img = torch.randn(B, 3, H, W, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    scale = torch.rand(64, generator=g) + 0.5
    bias = torch.full((64,), 5.0) if big_bias else torch.randn(64, generator=g) * 0.1
    wp = K.pack_stem_weight(w.cuda(), dtype, 24)
    dev = img.cuda(), wp, scale.cuda(), bias.cuda()
    two = K.maxpool_3x3s2(K.stem_conv_image(*dev, dtype))
    torch.cuda.synchronize()
    return (img, w, scale, bias), dev, two


@pytest.mark.parametrize('B,H,W', SMALL + [(2, 800, 1333)])
@pytest.mark.parametrize('dtype', DTYPES)
def test_stem_pool_equals_two_launches(B, H, W, dtype):
    """Bit-identical to maxpool_3x3s2(stem_conv_image(...)) for every segment length: an image
    smaller than one tile; odd Ho / Wo with a ragged tile; two images; three strips with a ragged
    last one (Wo = 150); 17 tiles in several segments with a ragged last one and Wo = 125 on the
    62-column strip boundary; the workload's shape with the launcher's own segment length."""
    from kinet_amd import kernels as K
    _, dev, two = _case(B, H, W, dtype)
    for seg in ((0, 1, 2, 3) if H * W < 10 ** 6 else (0,)):
        got = K.stem_pool_image(*dev, dtype, seg_tiles=seg)
        torch.cuda.synchronize()
        assert got.shape == two.shape
        assert torch.equal(got, two), (seg, (got.float() - two.float()).abs().max().item())


@pytest.mark.parametrize('B,H,W', SMALL)
@pytest.mark.parametrize('dtype', DTYPES)
def test_stem_pool_vs_torch_fp32(B, H, W, dtype):
    """Against torch fp32 conv1 + BN + ReLU + max_pool2d, within the existing stem test's bound."""
    from kinet_amd import kernels as K
    (img, w, scale, bias), dev, _ = _case(B, H, W, dtype)
    ref = F.max_pool2d(F.relu(F.conv2d(img, w, stride=2, padding=3) * scale[None, :, None, None]
                              + bias[None, :, None, None]), 3, 2, 1)
    got = K.stem_pool_image(*dev, dtype)
    torch.cuda.synchronize()
    rel = _rel(got.permute(0, 3, 1, 2), ref)
    print(f'{(B, H, W)} {dtype}: rel = {rel:.3e}')
    assert rel < 2e-2


@pytest.mark.parametrize('dtype', DTYPES)
def test_stem_pool_edge_maxima(dtype):
    """bias = 5: relu(bias) of the conv rows / columns past the ragged edge (a zero-padded input)
    would win the maximum of the last pooled row and column if it were not masked out."""
    from kinet_amd import kernels as K
    _, dev, two = _case(1, 37, 41, dtype, True)
    assert two.float().min().item() > 0
    for seg in (0, 1, 2, 3):
        got = K.stem_pool_image(*dev, dtype, seg_tiles=seg)
        torch.cuda.synchronize()
        assert torch.equal(got, two), seg


def test_stem_pool_argument_errors():
    """Checked like kinet_stem_conv_image: 16-bit dtypes only, no null pointers, N = 0 is a no-op."""
    from kinet_amd import _native
    L = _native.lib()
    x = torch.zeros(4096, device='cuda')
    p = x.data_ptr()
    assert L.kinet_stem_pool_image(p, p, p, p, p, 1, 9, 7, 0, 0, None) == 1        # KINET_ERR_ARG: f32
    assert 'dtype' in L.kinet_last_error().decode()
    assert L.kinet_stem_conv_image(p, p, p, p, p, 1, 9, 7, 0, None) == 1
    assert L.kinet_stem_pool_image(None, p, p, p, p, 1, 9, 7, 1, 0, None) == 1
    assert 'NULL' in L.kinet_last_error().decode()
    assert L.kinet_stem_conv_image(None, p, p, p, p, 1, 9, 7, 1, None) == 1
    assert L.kinet_stem_pool_image(p, p, p, p, None, 1, 9, 7, 1, 0, None) == 1
    assert L.kinet_stem_pool_image(p, p, p, p, p, 1, 9, 7, 1, -1, None) == 1
    assert L.kinet_stem_pool_image(p, p, p, p, p, 0, 9, 7, 1, 0, None) == 0        # KINET_OK
    torch.cuda.synchronize()


@pytest.mark.parametrize('dtype', DTYPES)
def test_backbone_stem_pool_matches_two_launches(dtype):
    """ResNet-50 body with FUSE_STEM_POOL on / off: the four stage outputs are equal bit for bit,
    and the trace shows the fused launch in place of the max-pool (and the reverse)."""
    from kinet_amd import _native
    from kinet_amd.models import backbone as BB
    torch.manual_seed(0)
    body = BB.ResNetBody([3, 4, 6, 3]).cuda().eval()
    img = torch.randn(2, 3, 160, 224, device='cuda')
    old = BB.FUSE_STEM_POOL
    outs, names = [], []
    try:
        for flag in (True, False):
            BB.FUSE_STEM_POOL = flag
            _native.trace_begin()
            try:
                with torch.no_grad():
                    outs.append(body.forward_nhwc(img, dtype))
            finally:
                names.append([n for n, *_ in _native.trace_end()])
    finally:
        BB.FUSE_STEM_POOL = old
    torch.cuda.synchronize()
    assert names[0].count('kinet_stem_pool_image') == 1
    assert 'kinet_maxpool2d_3x3s2' not in names[0] and 'kinet_stem_conv_image' not in names[0]
    assert 'kinet_stem_pool_image' not in names[1]
    assert names[1].count('kinet_maxpool2d_3x3s2') == 1 and names[1].count('kinet_stem_conv_image') == 1
    assert len(outs[0]) == 4
    for a, b in zip(*outs):
        assert a.shape == b.shape and torch.equal(a, b)
