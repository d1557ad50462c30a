"""Direct tests of the multi-sequence tracker's kernels (csrc/track.hip, include/kinet_track.h) against the
plain torch restatements of tests/multi_track_refs.py, computed on the CPU."""
import numpy as np
import pytest
import torch

import multi_track_refs as R

pytestmark = pytest.mark.gpu

T_TRACK, T_REID, T_DET = 0.4, 0.6, 0.5
GUARD = 64
SENTINEL = 0xA5


def _decide_inputs():
    """S = 3, Kmax = 5, Q = 7, C = 3, K = (0, 5, 2): N(0, 1.5) logits, boxes partly outside the image, NaN
    in every placeholder row, and one planted row whose best logit is exactly 0 (score exactly 0.5)."""
    g = torch.Generator().manual_seed(4)
    S, kmax, Q, C = 3, 5, 7, 3
    k = [0, 5, 2]
    n = kmax + Q
    logits = torch.randn(S, n, C, generator=g) * 1.5
    boxes = torch.cat([torch.rand(S, n, 2, generator=g) * 1.2 - 0.1, torch.rand(S, n, 2, generator=g) * 0.45 + 0.05], -1)
    logits[0, 6] = torch.tensor([0.0, -1.0, -2.0])
    for s in range(S):
        logits[s, k[s]:kmax] = float('nan')
        boxes[s, k[s]:kmax] = float('nan')
    sizes = torch.tensor([[480., 640.], [375., 1242.], [1080., 1920.]])
    return logits, boxes, sizes, k, kmax, Q


def test_decide_seed_excludes_no_row():
    """(CPU arithmetic, kept beside its users) every real row but the planted one scores farther than 1e-6
    from all three thresholds, so the decision bytes are compared on every row."""
    logits, boxes, sizes, k, kmax, Q = _decide_inputs()
    _, scores, _, _ = R.decide_ref(logits, boxes, sizes, k, kmax, T_TRACK, T_REID, T_DET, True)
    near = torch.stack([(scores - t).abs() <= 1e-6 for t in (T_TRACK, T_REID, T_DET)]).any(0)
    near[0, 6] = False
    row = torch.arange(kmax + Q)[None]
    real = ~((row >= torch.tensor(k)[:, None]) & (row < kmax))
    assert not (near & real).any()
    assert scores[0, 6].item() == 0.5


@pytest.mark.parametrize('clip', [True, False])
def test_decide(clip):
    from kinet_amd import kernels as K
    logits, boxes, sizes, k, kmax, Q = _decide_inputs()
    S, n = logits.shape[:2]
    want = R.decide_ref(logits, boxes, sizes, k, kmax, T_TRACK, T_REID, T_DET, clip)
    nbytes = S * n * 25
    buf = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
    n_act = torch.tensor([0, 3, 1], dtype=torch.int32, device='cuda')
    n_inact = torch.tensor([0, 2, 1], dtype=torch.int32, device='cuda')
    out = K.track_decide(logits.cuda(), boxes.cuda(), sizes.cuda(), n_act, n_inact, kmax, T_TRACK, T_REID, T_DET, clip,
                         out=buf[GUARD:GUARD + nbytes])
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + nbytes:] == SENTINEL).all()
    got = K.track_decide_views(host[GUARD:GUARD + nbytes].copy(), S, n)
    assert out.data_ptr() == buf.data_ptr() + GUARD
    np.testing.assert_allclose(got[0], want[0].numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(got[1], want[1].numpy(), rtol=1e-6, atol=0)
    np.testing.assert_array_equal(got[2], want[2].numpy())
    np.testing.assert_array_equal(got[3], want[3].numpy())
    # strict compare: score exactly 0.5 is above 0.4 and not above 0.5; class 0 is the person class
    assert got[3][0, 6] == R.DEC_TRACK | R.DEC_PERSON
    for s in range(S):          # NaN placeholders: byte 0, zero box / score / label
        for arr in got:
            assert not arr[s, k[s]:kmax].any()
    # bit-identical rerun
    again = K.track_decide(logits.cuda(), boxes.cuda(), sizes.cuda(), n_act, n_inact, kmax, T_TRACK, T_REID, T_DET, clip)
    assert torch.equal(again.cpu(), torch.from_numpy(host[GUARD:GUARD + nbytes].copy()))


def test_decide_refuses_too_many_rows():
    from kinet_amd import kernels as K
    z = torch.zeros(1, 4097, 1, device='cuda')
    with pytest.raises(RuntimeError, match='4096'):
        K.track_decide(z, torch.zeros(1, 4097, 4, device='cuda'), torch.ones(1, 2, device='cuda'),
                       torch.zeros(1, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda'),
                       0, 0.4, 0.4, 0.4, True)


def test_nms_segments():
    from kinet_amd import kernels as K
    g = torch.Generator().manual_seed(11)
    rows, d = 400, 16
    c = torch.rand(rows, 2, generator=g) * 500
    boxes = torch.cat([c, c + torch.rand(rows, 2, generator=g) * 80 + 1], 1)
    scores = torch.rand(rows, generator=g)
    scores[40:160] = scores[160:280]                                    # ties
    scores[0:40:7] = float('nan')
    scores[3], scores[5], scores[10] = float('inf'), -float('inf'), float('inf')
    bank = torch.randn(rows, d + 5, generator=g)                        # the boxes and scores sit in a wider table
    bank[:, d:d + 4], bank[:, d + 4] = boxes, scores
    seg_nan = torch.randperm(40, generator=g)[:37]
    seg_big = torch.randperm(360, generator=g)[:300] + 40
    segs = [torch.zeros(0, dtype=torch.int64), torch.tensor([77]), seg_nan, torch.zeros(0, dtype=torch.int64), seg_big]
    idx = torch.cat(segs).to(torch.int32)
    offsets = torch.tensor([0] + np.cumsum([len(s) for s in segs]).tolist(), dtype=torch.int32)
    total = int(offsets[-1])
    flag = torch.zeros(total, dtype=torch.uint8)
    flag[int(offsets[4]):total:3] = 1                                   # +inf on a third of the big segment
    bank_d = bank.cuda()
    for thr in (0.3, 0.5):
        for fl in (None, flag):
            want = R.nms_segments_ref(boxes, scores, idx, offsets, thr, fl)
            keep = torch.full((total + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device='cuda')
            K.nms_segments(bank_d[:, d:d + 4], bank_d[:, d + 4], idx.cuda(), offsets.cuda(), total, thr,
                           inf_flag=None if fl is None else fl.cuda(), keep=keep[GUARD:GUARD + total])
            host = keep.cpu()
            assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + total:] == SENTINEL).all()
            got = host[GUARD:GUARD + total]
            assert torch.equal(got, want), (thr, fl is not None)
            for s, seg in enumerate(segs):                               # and K.nms on the gathered rows
                lo, hi = int(offsets[s]), int(offsets[s + 1])
                sc = scores[seg].clone()
                if fl is not None:
                    sc[fl[lo:hi].bool()] = float('inf')
                kept = K.nms(boxes[seg].cuda(), sc.cuda(), thr).cpu()
                flags = torch.zeros(hi - lo, dtype=torch.uint8)
                flags[kept] = 1
                assert torch.equal(got[lo:hi], flags), (thr, s)
    assert 0 < int(want[int(offsets[4]):].sum()) < 300                  # the big segment suppresses some, not all


def test_commit_and_gather():
    from kinet_amd import _native as N
    from kinet_amd import kernels as K
    g = torch.Generator().manual_seed(12)
    d, cap = 16, 32
    hs = torch.randn(12, d, generator=g)
    c = torch.rand(12, 2, generator=g) * 500
    boxes = torch.cat([c, c + torch.rand(12, 2, generator=g) * 90 + 1], 1)
    scores = torch.rand(12, generator=g)
    bank = torch.full((cap, d + 5), -7.0)
    rows = torch.tensor([3, 7, 0, 11, 5, 6], dtype=torch.int32)
    slots = torch.tensor([5, 0, 31, 9, 17, 2], dtype=torch.int32)
    want = R.commit_ref(bank.clone(), hs, boxes, scores, rows, slots)
    bank_d = bank.cuda()
    K.track_commit(hs.cuda(), boxes.cuda(), scores.cuda(), rows.cuda(), slots.cuda(), 6, bank_d)
    assert torch.equal(bank_d.cpu(), want)                              # bit-exact, sentinel rows untouched

    # gather: K = (0, 4 = Kmax, 2), three frame sizes, outputs inside sentinel guards
    S, kmax, Q = 3, 4, 7
    lists = [[], [31, 5, 0, 9], [17, 2]]
    gl = torch.tensor([t for l in lists for t in l], dtype=torch.int32)
    off = torch.tensor([0, 0, 4, 6], dtype=torch.int32)
    sizes = torch.tensor([[480., 640.], [375., 1242.], [1080., 1920.]])
    w_emb, w_box, w_mask = R.gather_ref(want, gl, off, sizes, kmax, Q)
    G = 32
    emb = torch.full((S * kmax * d + 2 * G,), -3.0, device='cuda')
    box = torch.full((S * kmax * 4 + 2 * G,), -3.0, device='cuda')
    msk = torch.full((S * (kmax + Q) + 2 * G,), SENTINEL, dtype=torch.uint8, device='cuda')
    args = [gl.cuda(), off.cuda(), sizes.cuda()]
    N.call('kinet_track_gather', N.ptr(bank_d), cap, d, N.ptr(args[0]), N.ptr(args[1]), N.ptr(args[2]),
           N.ptr(emb[G:]), N.ptr(box[G:]), N.ptr(msk[G:]), S, kmax, Q, N.stream(bank_d.device))
    emb, box, msk = emb.cpu(), box.cpu(), msk.cpu()
    for t, sent in ((emb, -3.0), (box, -3.0), (msk, SENTINEL)):
        assert (t[:G] == sent).all() and (t[-G:] == sent).all()
    assert torch.equal(emb[G:-G].view(S, kmax, d), w_emb)
    np.testing.assert_allclose(box[G:-G].view(S, kmax, 4).numpy(), w_box.numpy(), rtol=1e-7, atol=0)
    assert torch.equal(msk[G:-G].view(S, kmax + Q).bool(), w_mask)
    assert w_mask[0, :kmax].all() and not w_mask[1].any()               # K_i = 0 beside K_i = Kmax
    # the wrapper returns the same three tensors
    e2, b2, m2 = K.track_gather(bank_d, *args, kmax, Q)
    assert torch.equal(e2.cpu(), w_emb) and torch.equal(m2.cpu(), w_mask)
    assert torch.equal(b2.cpu(), box[G:-G].view(S, kmax, 4))


@pytest.mark.parametrize('d', [16, 288])
def test_reid_dist(d):
    from kinet_amd import kernels as K
    g = torch.Generator().manual_seed(13 + d)
    cap, R_ = 16, 24
    bank = torch.randn(cap, d + 5, generator=g)
    hs = torch.randn(R_, d, generator=g)
    hs[9] = bank[4, :d] + 0.01 * torch.randn(d, generator=g)            # a near match: cancellation in x - y
    slots = torch.tensor([4, 11, 2, 7], dtype=torch.int32)
    slot_off = torch.tensor([0, 3, 3, 4], dtype=torch.int32)            # sequences of 3, 0 and 1 inactive tracks
    rows = torch.tensor([9, 0, 23, 5, 14, 13, 17], dtype=torch.int32)
    row_off = torch.tensor([0, 5, 6, 7], dtype=torch.int32)             # 5, 1 and 1 detections
    out_off = torch.tensor([0, 15, 15, 16], dtype=torch.int32)
    out = K.track_reid_dist(bank.cuda(), hs.cuda(), slots.cuda(), slot_off.cuda(), rows.cuda(), row_off.cuda(),
                            out_off.cuda(), 16).cpu()
    a = R.reid_dist_ref(bank[slots[:3].long(), :d], hs[rows[:5].long()])
    b = R.reid_dist_ref(bank[slots[3:].long(), :d], hs[rows[6:].long()])
    np.testing.assert_allclose(out[:15].view(3, 5).double().numpy(), a.numpy(), rtol=1e-5, atol=0)
    np.testing.assert_allclose(out[15:].view(1, 1).double().numpy(), b.numpy(), rtol=1e-5, atol=0)
    again = K.track_reid_dist(bank.cuda(), hs.cuda(), slots.cuda(), slot_off.cuda(), rows.cuda(), row_off.cuda(),
                              out_off.cuda(), 16).cpu()
    assert torch.equal(out, again)
