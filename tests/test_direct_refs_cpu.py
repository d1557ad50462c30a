"""CPU checks of tests/direct_refs.py: the references the direct kernel tests compare against,
so a wrong helper cannot be blamed on a kernel."""
import math

import numpy as np
import pytest
import torch

import direct_refs as R


def _pixelwise_sine(mask, npf, three_d=False, frame=0, frames=1, normalize=True, ft=np.float64):
    """The embedding one pixel at a time, from the formulas in the docstring of
    kinet_amd/models/position_encoding.py: count the unmasked pixels of the pixel's column down to
    its row and of its row up to its column (and, 3-d, of its frame stack up to `frame`), divide by
    the count of the whole column / row / stack (+ 1e-6) times 2 pi when normalising (2-d: after
    taking 0.5 off), then sin (even channels) / cos (odd) of count / dim_t.  Every step in `ft`
    arithmetic (np.float64 or np.float32); returns (B, H*W, C) f64."""
    B, H, W = mask.shape
    free = [[[0 if v else 1 for v in row] for row in img] for img in mask.tolist()]
    dim_t = R.sine_dim_t(npf).numpy().astype(ft)
    even = np.arange(npf) % 2 == 0
    two_pi, tiny, half = ft(2 * math.pi), ft(1e-6), ft(0.5)
    out = np.zeros((B, H * W, (3 if three_d else 2) * npf))
    for b in range(B):
        for h in range(H):
            for w in range(W):
                column = [free[b][i][w] for i in range(H)]
                axes = [(sum(column[:h + 1]), sum(column)), (sum(free[b][h][:w + 1]), sum(free[b][h]))]
                if three_d:
                    axes.insert(0, (free[b][h][w] * (frame + 1), free[b][h][w] * frames))
                blocks = []
                for count, whole in axes:
                    e = ft(count)
                    if normalize:
                        e = (e if three_d else e - half) / (ft(whole) + tiny) * two_pi
                    a = e / dim_t
                    blocks.append(np.where(even, np.sin(a), np.cos(a)))
                out[b, h * W + w] = np.concatenate(blocks)
    return torch.from_numpy(out)


GEO = R.sine_geometries()


@pytest.mark.parametrize('name', sorted(GEO))
@pytest.mark.parametrize('npf', [128, 144, 96])
@pytest.mark.parametrize('normalize', [True, False])
def test_sine_restatement_equals_pixelwise_2d(name, npf, normalize):
    mask = GEO[name]
    ref = R.sine_embed_ref(mask, npf, normalize=normalize)
    naive = _pixelwise_sine(mask, npf, normalize=normalize)
    keep = R.sine_compared(mask, npf, False, normalize)
    assert ref.shape == naive.shape == keep.shape
    # the same f64 arithmetic at every compared position (the excluded ones have arguments
    # ~ -3e6: bounded, not compared)
    assert (ref - naive)[keep].abs().max().item() <= 1e-12
    assert ref.abs().max().item() <= 1.0


@pytest.mark.parametrize('name', sorted(GEO))
@pytest.mark.parametrize('frames,npf', [(2, 96), (3, 128), (2, 144)])
@pytest.mark.parametrize('normalize', [True, False])
def test_sine_restatement_equals_pixelwise_3d(name, frames, npf, normalize):
    mask = GEO[name]
    for f in range(frames):
        ref = R.sine_embed_ref(mask, npf, True, f, frames, normalize)
        assert R.sine_compared(mask, npf, True, normalize).all()
        assert (ref - _pixelwise_sine(mask, npf, True, f, frames, normalize)).abs().max().item() <= 1e-12


def test_sine_dim_t_is_the_modules_own():
    from kinet_amd.models.position_encoding import PositionEmbeddingSine
    for npf in (128, 144, 96):
        assert torch.equal(R.sine_dim_t(npf), PositionEmbeddingSine(npf, normalize=True).dim_t('cpu'))


def test_sine_level_embed_is_added_per_channel():
    mask = GEO['main']
    le = torch.randn(256, generator=torch.Generator().manual_seed(2))
    a = R.sine_embed_ref(mask, 128)
    b = R.sine_embed_ref(mask, 128, level_embed=le)
    assert torch.equal(b, a + le.double())


@pytest.mark.parametrize('npf', [128, 144, 96])
def test_sine_f32_vs_f64_gap_on_main_masks(npf):
    """The same arithmetic evaluated step by step in f32 vs in f64, at the compared positions of
    the main mask set, normalised (arguments up to 2 pi): the f32 tolerance of the GPU test (5e-6)
    is several times this."""
    mask = GEO['main']
    keep = R.sine_compared(mask, npf, False, True)
    g2 = (_pixelwise_sine(mask, npf, ft=np.float32) - _pixelwise_sine(mask, npf))[keep].abs().max().item()
    g3 = max((_pixelwise_sine(mask, npf, True, f, 2, ft=np.float32)
              - _pixelwise_sine(mask, npf, True, f, 2)).abs().max().item() for f in (0, 1))
    print(f'sine f32-vs-f64 gap npf={npf}: 2-d {g2:.3e}, 3-d {g3:.3e}')
    assert g2 < 1e-6 and g3 < 1e-6


def test_sine_excluded_share_caps():
    """Nothing excluded for an unmasked image, <= 25 % for every other image the GPU test compares
    in 2-d normalised mode; the main set gives 20.9 % and 7.5 %."""
    for name, mask in GEO.items():
        share = R.sine_excluded_share(mask)
        for b in range(mask.shape[0]):
            if (name, b) in R.FULLY_MASKED:
                assert mask[b].all() and share[b].item() == 1.0
                continue
            if not mask[b].any():
                assert share[b].item() == 0.0
            assert share[b].item() <= 0.25, (name, b, share[b].item())
    main = R.sine_excluded_share(GEO['main'])
    assert main[0].item() == 0.0
    assert abs(main[1].item() - 0.209) < 1e-3 and abs(main[2].item() - 0.075) < 1e-3


def test_main_mask_set_has_holes_and_a_masked_row_and_column():
    m = GEO['main']
    assert not m[0].any()
    assert (~m[1, :9, :13]).all() and m[1, 9:].all() and m[1, :, 13:].all()
    assert m[2, 4].all() and m[2, :, 6].all()
    inner = m[2, 1:-1, 1:-1]
    assert inner.any() and not inner.all()
    # no other row or column of image 2 is fully masked
    assert m[2].all(1).sum().item() == 1 and m[2].all(0).sum().item() == 1


@pytest.mark.parametrize('KH,KW,stride,pad,H,W,C', [(3, 2, (2, 1), (1, 0), 5, 4, 4), (1, 3, (1, 2), (0, 1), 3, 5, 8)])
def test_unfold_fold_helpers_vs_naive_loop(KH, KW, stride, pad, H, W, C):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, H, W, C, generator=g, dtype=torch.float64)
    cols = R.unfold_nhwc(x, KH, KW, stride, pad)
    assert torch.equal(cols, R.unfold_naive(x, KH, KW, stride, pad))
    c = torch.randn(cols.shape, generator=g, dtype=torch.float64)
    dx = R.fold_nhwc(c, x.shape, KH, KW, stride, pad)
    assert (dx - R.fold_naive(c, x.shape, KH, KW, stride, pad)).abs().max().item() < 1e-12
    # and the two are adjoint
    assert abs((cols * c).sum().item() - (x * dx).sum().item()) < 1e-9


def test_inverse_sigmoid_matches_host_definition_at_clamp_points():
    from kinet_amd.models.misc import inverse_sigmoid
    x = torch.tensor([0.0, 1.0, 1e-7, 1 - 1e-7, -1e-3, 1.001, 1e-5, 1 - 1e-5, 2e-5, 0.5, 0.25], dtype=torch.float32)
    got = R.inverse_sigmoid_ref(x)
    host = inverse_sigmoid(x)                      # the CPU branch: torch f32
    assert (got - host.double()).abs().max().item() < 2e-6
    assert got[0].item() == pytest.approx(math.log(1e-5 / 1.0), abs=1e-12)
    assert got[1].item() == pytest.approx(math.log(1.0 / 1e-5), abs=1e-12)
    assert got[4].item() == got[0].item() and got[5].item() == got[1].item()
    assert got[9].item() == 0.0


def test_box_case_valid_ratios_make_a_wrong_index_visible():
    """The valid ratios of a case differ by far more than the tolerance (1e-5) between batches,
    levels and x / y, so a wrong index in the kernel cannot pass; the clamp points are in `ref`."""
    for B, L in ((1, 1), (1, 4), (3, 1), (3, 4)):
        _, ref, vr = R.box_case(B, 300, L, 4)
        flat = vr.reshape(-1)
        d = (flat[:, None] - flat[None, :]).abs() + torch.eye(flat.numel())
        assert d.min().item() > 1e-2
        for s in R.SPECIAL_REFS:
            assert (ref == torch.tensor(s, dtype=torch.float32)).any()


def test_box_refine_ref_pads_two_column_references():
    g = torch.Generator().manual_seed(4)
    tmp = torch.randn(2, 5, 4, generator=g)
    ref2 = torch.rand(2, 5, 2, generator=g)
    vr = torch.rand(2, 3, 2, generator=g)
    new, rin = R.box_refine_ref(tmp, ref2, vr)
    assert torch.equal(new[..., 2:], torch.sigmoid(tmp[..., 2:].double()))
    assert rin.shape == (2, 5, 3, 4)
    assert torch.equal(rin[1, 2, 1], new[1, 2] * torch.stack([vr[1, 1, 0], vr[1, 1, 1]] * 2).double())


def test_layernorm_vec_eligibility_table():
    f32, bf = torch.float32, torch.bfloat16
    assert [d for d in (8, 36, 90, 256, 288, 512, 1024) if R.layernorm_vec_eligible(f32, d)] == [8, 36, 256]
    assert [d for d in (8, 36, 90, 256, 288, 512, 1024) if R.layernorm_vec_eligible(bf, d)] == [8, 256, 288, 512]
