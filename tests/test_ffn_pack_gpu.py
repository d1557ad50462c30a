"""The packed weight streams of the fused FFN and the bottleneck pairs (kinet_ffn_pack, kinet_ffn_pack_attn,
kinet_bottleneck_pack, kinet_bottleneck_pack_ds) against the one definition of their layout: a packed buffer is,
bit for bit, the gather of the source weights through kinet_ffn_pack_map; where the pack folds FrozenBN scales,
the row is scaled in f32 and rounded once.  Shapes: the smallest with more than one hidden chunk and both fragment
kinds at each D the kernels take."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(64, 256), (128, 512), (256, 64), (288, 64)]
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


def gather(K, kind, mats, D, F, DB, dtype, scales=None):
    """The stream as the map defines it: element i = mats[m][row, col] (* scales[m][row] in f32, then one rounding)."""
    m = K.ffn_pack_map(kind, D, F, DB).long().cuda()
    out = torch.empty(m.shape[0], dtype=dtype, device='cuda')
    for i, w in enumerate(mats):
        sel = m[:, 0] == i
        v = w[m[sel, 1], m[sel, 2]]
        if scales is not None:
            assert v.dtype == torch.float32
            v = (v * scales[i][m[sel, 1]]).to(dtype)
        out[sel] = v
    return out


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize('D,F', SHAPES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_ffn_pack(K, D, F, dtype):
    g = torch.Generator().manual_seed(D + F)
    w1, w2 = torch.randn(F, D, generator=g).to(dtype).cuda(), torch.randn(D, F, generator=g).to(dtype).cuda()
    assert same_bits(K.ffn_pack(w1, w2, dtype), gather(K, 'ffn', [w1, w2], D, F, D, dtype))


@pytest.mark.parametrize('D,F', SHAPES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_ffn_pack_attn(K, D, F, dtype):
    g = torch.Generator().manual_seed(D + F + 1)
    wo = torch.randn(D, D, generator=g).to(dtype).cuda()
    w1, w2 = torch.randn(F, D, generator=g).to(dtype).cuda(), torch.randn(D, F, generator=g).to(dtype).cuda()
    got = K.attn_out_ffn_pack(wo, w1, w2, dtype)
    assert same_bits(got, gather(K, 'attn_out_ffn', [wo, w1, w2], D, F, D, dtype))
    assert same_bits(got[D * D:], K.ffn_pack(w1, w2, dtype))   # the tail is kinet_ffn_pack's stream


@pytest.mark.parametrize('D,F,DB', [(D, F, D) for D, F in SHAPES] + [(64, 256, 128)])
@pytest.mark.parametrize('dtype', DTYPES)
def test_bottleneck_pack(K, D, F, DB, dtype):
    g = torch.Generator().manual_seed(D + F + DB)
    w3, w1 = torch.randn(F, D, 1, 1, generator=g).cuda(), torch.randn(DB, F, 1, 1, generator=g).cuda()
    s3, s1 = (torch.rand(F, generator=g) + 0.5).cuda(), (torch.rand(DB, generator=g) + 0.5).cuda()
    want = gather(K, 'pair', [w3.reshape(F, D), w1.reshape(DB, F)], D, F, DB, dtype, [s3, s1])
    assert same_bits(K.bottleneck_pack(w3, w1, s3, s1, dtype), want)


@pytest.mark.parametrize('dtype', DTYPES)
def test_bottleneck_pack_ds(K, dtype):
    D, F, DB = 64, 256, 64
    g = torch.Generator().manual_seed(7)
    w3, wd = torch.randn(F, D, 1, 1, generator=g).cuda(), torch.randn(F, D, 1, 1, generator=g).cuda()
    w1 = torch.randn(DB, F, 1, 1, generator=g).cuda()
    s3, sd, s1 = [(torch.rand(n, generator=g) + 0.5).cuda() for n in (F, F, DB)]
    b = torch.zeros(F).cuda()
    packed, _ = K.bottleneck_pack_ds(w3, wd, w1, s3, sd, s1, b, b, dtype)
    want = gather(K, 'pair_ds', [w3.reshape(F, D), wd.reshape(F, D), w1.reshape(DB, F)], D, F, DB, dtype, [s3, sd, s1])
    assert same_bits(packed, want)
