"""kinet_segm_track_resolve alone (csrc/segm.hip): the tracker's stack / argmax / compare over fresh
probabilities and stale 0/1 planes, written as one int16 label map.

Geometry: logits 26x50, network input at most 104x200, this frame's crop 88x136, original size 131x203
(no integer ratio anywhere), n = 5 rows, T = 7 slots in the order
    [row 3, stale 0, row 0, row 4, stale 2, row 1, row 2]
  * rows 3 and 4 are identical: slot 0 must own what they win, never slot 3;
  * rows 0 and 1 hold a block at +30, where f32 sigmoid is exactly 1.0: there stale slot 1 (before both)
    wins where the previous map held 0, stale slot 4 (after row 0's slot 2) loses where it held 2, and slot 2
    beats slot 5;
  * a NaN row, in a case of its own, turns every pixel into background (argmax takes the NaN, NaN > 0.5 is false).
"""
import pytest
import torch

import segm_refs as R
from kinet_amd import kernels as K

pytestmark = pytest.mark.gpu

H, W = 26, 50
MAX_HW, IMG_HW, OUT_HW = (104, 200), (88, 136), (131, 203)
SLOTS = [3, -1, 0, 4, -3, 1, 2]          # src: >= 0 a row, < 0 stale slot -s-1
DELTA = 2e-6                             # the project's bound on a PostProcessSegm probability
SAT = (slice(8, 12), slice(20, 26))      # the +30 block, in logits pixels (inside the 88x136 crop's 22x34)


def make_logits():
    g = torch.Generator().manual_seed(91)
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    cy = torch.tensor([6.0, 14.0, 10.0, 12.0, 0.0]).view(5, 1, 1)
    cx = torch.tensor([10.0, 26.0, 18.0, 22.0, 0.0]).view(5, 1, 1)
    amp = torch.tensor([6.0, 5.0, 7.0, 5.5, 0.0]).view(5, 1, 1)
    logits = amp * torch.exp(-((ys - cy) / 7.0) ** 2 - ((xs - cx) / 11.0) ** 2) - 2.5 + 0.3 * torch.randn(5, H, W, generator=g)
    logits[4] = logits[3]
    logits[0][SAT] = 30.0
    logits[1][SAT] = 30.0
    return logits


def make_prev(hw, seed=92, slots=4):
    """A blocky previous label map with values -1 .. slots-1."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(-1, slots, (hw[0] // 8 + 1, hw[1] // 8 + 1), generator=g)
    return coarse.repeat_interleave(8, 0).repeat_interleave(8, 1)[:hw[0], :hw[1]].to(torch.int16).contiguous()


def composition(logits, src, prev, max_hw, img_hw, out_hw, thr=0.5):
    """tracker.py:516-525 on the GPU from this project's probabilities: (labels, stacked planes)."""
    probs = K.segm_postprocess(logits, max_hw, img_hw, out_hw, return_probs=True)[:, 0]
    planes = [probs[s] if s >= 0 else (prev == -s - 1).float() for s in src]
    st = torch.stack(planes)
    best = st.argmax(0)
    pbest = st.gather(0, best[None])[0]
    return torch.where(pbest > thr, best, torch.full_like(best, -1)).to(torch.int16), st


def probs64(logits, max_hw, img_hw, out_hw):
    """f64 restatement of PostProcessSegm's probabilities: torch's index rules in f32 (legacy nearest into
    the crop, area_pixel_compute_source_index into the logits), the interpolation and the sigmoid in f64."""
    n, h, w = logits.shape

    def taps(n_in, n_max, n_img, n_out):
        m = R.nearest_index(n_img, n_out).float()
        scale = torch.tensor(n_in, dtype=torch.float32) / torch.tensor(n_max, dtype=torch.float32)
        real = (scale * (m + 0.5) - 0.5).clamp(min=0)
        i0 = real.floor().long().clamp(max=n_in - 1)
        lam = (real - i0.float()).clamp(0, 1).double()
        return i0, (i0 + (i0 < n_in - 1).long()), lam
    y0, y1, ly = taps(h, max_hw[0], img_hw[0], out_hw[0])
    x0, x1, lx = taps(w, max_hw[1], img_hw[1], out_hw[1])
    L = logits.double()
    ly, lx = ly.view(1, -1, 1), lx.view(1, 1, -1)
    top = (1 - lx) * L[:, y0][:, :, x0] + lx * L[:, y0][:, :, x1]
    bot = (1 - lx) * L[:, y1][:, :, x0] + lx * L[:, y1][:, :, x1]
    return torch.sigmoid((1 - ly) * top + ly * bot)


@pytest.fixture(scope='module')
def case():
    logits, prev = make_logits().cuda(), make_prev(OUT_HW).cuda()
    labels = K.segm_track_resolve(logits, SLOTS, prev, MAX_HW, IMG_HW, OUT_HW, 0.5)
    want, st = composition(logits, SLOTS, prev, MAX_HW, IMG_HW, OUT_HW)
    torch.cuda.synchronize()
    return dict(logits=logits, prev=prev, labels=labels, want=want, planes=st)


def test_labels_equal_the_composition_at_every_pixel(case):
    got, want, st = case['labels'], case['want'], case['planes']
    assert got.dtype == torch.int16 and tuple(got.shape) == OUT_HW
    assert torch.equal(got, want)
    # the case holds what it is meant to hold
    assert not (got == 3).any() and (got == 0).any()                       # identical rows: the lower slot
    sat = (st[2] == 1.0) & (st[5] == 1.0)
    prev = case['prev']
    assert sat.any() and (got[sat & (prev == 0)] == 1).all() and (sat & (prev == 0)).any()      # stale before: wins
    assert (sat & (prev == 2)).any() and (got[sat & (prev != 0)] == 2).all()                    # stale after: loses
    assert not (got == 5)[sat].any()
    assert (got == -1).any() and ((st > 0.5).sum(0) >= 2).any()
    assert set(got.unique().tolist()) <= set(range(-1, 7))


def test_labels_against_f64(case):
    """delta = 2e-6 on a probability: an owner's probability is >= max - 2 delta and > 0.5 - delta, a
    background pixel has max <= 0.5 + delta.  Exact ties (identical rows; probabilities that f32 rounds to
    1.0, i.e. >= 1 - 2^-25, against a stale 1.0) go to the lower slot and are no freedom."""
    prev, got = case['prev'].cpu(), case['labels'].cpu().long()
    p = probs64(case['logits'].cpu(), MAX_HW, IMG_HW, OUT_HW)
    p = torch.where(p >= 1 - 2.0 ** -25, torch.ones_like(p), p)
    st = torch.stack([p[s] if s >= 0 else (prev == -s - 1).double() for s in SLOTS])
    mx = st.max(0)[0]
    adm = (st >= mx - 2 * DELTA) & (st > 0.5 - DELTA)
    for t in range(1, len(SLOTS)):       # an exact tie with a lower admissible slot is not a second answer
        adm[t] &= ~((st[:t] == st[t]) & adm[:t]).any(0)
    bg_ok = mx <= 0.5 + DELTA
    owned = got >= 0
    owner_p = st.gather(0, got.clamp(min=0)[None])[0]
    assert (owner_p[owned] >= mx[owned] - 2 * DELTA).all() and (owner_p[owned] > 0.5 - DELTA).all()
    assert adm.gather(0, got.clamp(min=0)[None])[0][owned].all()
    assert bg_ok[~owned].all()
    free = (adm.sum(0) + bg_ok.long()) > 1
    share = free.float().mean().item()
    print(f'track_resolve vs f64: pixels with more than one admissible answer {share:.3e} ({int(free.sum())} of {free.numel()})')
    assert share <= 5e-3


def test_nan_row_makes_everything_background(case):
    logits = case['logits'].clone()
    logits[0] = float('nan')
    got = K.segm_track_resolve(logits, SLOTS, case['prev'], MAX_HW, IMG_HW, OUT_HW, 0.5)
    assert (got == -1).all()
    assert torch.equal(got, composition(logits, SLOTS, case['prev'], MAX_HW, IMG_HW, OUT_HW)[0])


def test_large_output_indexing():
    g = torch.Generator().manual_seed(93)
    logits = (torch.randn(3, H, W, generator=g) * 2).cuda()
    out_hw = (540, 960)
    prev = make_prev(out_hw, 94, 3).cuda()
    src = [2, -2, 0]
    got = K.segm_track_resolve(logits, src, prev, MAX_HW, MAX_HW, out_hw, 0.5)
    want = composition(logits, src, prev, MAX_HW, MAX_HW, out_hw)[0]
    assert torch.equal(got, want)
    assert set(got.unique().tolist()) == {-1, 0, 1, 2} and got[-1, -1] == want[-1, -1]


def test_rerun_is_bit_identical(case):
    out = torch.full(OUT_HW, 77, dtype=torch.int16, device='cuda')
    again = K.segm_track_resolve(case['logits'], SLOTS, case['prev'], MAX_HW, IMG_HW, OUT_HW, 0.5, out=out)
    assert again is out and torch.equal(again, case['labels'])


def test_empty_slots_and_empty_logits(case):
    prev = case['prev']
    none = K.segm_track_resolve(case['logits'], [], None, MAX_HW, IMG_HW, OUT_HW, 0.5)          # T == 0
    assert (none == -1).all()
    empty = case['logits'][:0]
    kept = K.segm_track_resolve(empty, [-1, -4], prev, MAX_HW, IMG_HW, OUT_HW, 0.5)            # n == 0, stale only
    want = torch.where(prev == 0, 0, torch.where(prev == 3, 1, -1)).to(torch.int16)
    assert torch.equal(kept, want)


def test_wrapper_rejects_what_the_host_knows(case):
    with pytest.raises(RuntimeError, match='prev_labels'):
        K.segm_track_resolve(case['logits'], [0, -1], None, MAX_HW, IMG_HW, OUT_HW)
    with pytest.raises(RuntimeError, match='outside'):
        K.segm_track_resolve(case['logits'], [5], None, MAX_HW, IMG_HW, OUT_HW)
    with pytest.raises(RuntimeError, match='inside'):
        K.segm_track_resolve(case['logits'], [0], None, IMG_HW, MAX_HW, OUT_HW)
