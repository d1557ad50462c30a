"""The kernels behind MultiTracker's masks, alone (csrc/segm.hip):

  * the ragged mask-head entry points (kinet_segm_attention_rows, kinet_segm_lay1_rows,
    kinet_segm_gn_relu_up_add_rows) against the frame-major entry points called per frame on that frame's
    rows the way DETRSegmBase.mask_logits calls them (one frame, Q = its rows, row0 = 0): the kernels are the
    same, so torch.equal, in f32 and bf16; a frame entry outside [0, B) leaves its output row untouched;
  * kinet_segm_track_resolve_segments against kinet_segm_track_resolve per segment (torch.equal on every
    label), its per-slot statistics against numpy's count / min / max of labels == t, reruns byte for byte,
    and a segment with more slots than the workgroups' LDS table holds (the global-atomic path);
  * DETRSegmBase.mask_logits_rows over rows of mixed frames against pred_masks of the full head.
"""
import os

import numpy as np
import pytest
import torch

import segm_refs as R
import test_mots_direct_gpu as D
from kinet_amd import kernels as K

pytestmark = pytest.mark.gpu

B, Q = 2, 5
FRAMES = [1, 0, 0, 1, 1, 0]
ROWS = [3, 0, 0, 4, 1, 2]                 # (frame 0, row 0) twice
DTYPES = [torch.float32, torch.bfloat16]
FILL = 7.0                                # the prefilled output of the out-of-range cases


def _lists(frames=FRAMES):
    f = torch.tensor(frames, dtype=torch.int32, device='cuda')
    sel = [torch.tensor([i for i, b in enumerate(frames) if b == fb], device='cuda') for fb in range(B)]
    return f, sel


def _bad_frames():
    bad = list(FRAMES)
    bad[2], bad[4] = B, -1
    return torch.tensor(bad, dtype=torch.int32, device='cuda'), [2, 4], [0, 1, 3, 5]


def _check_bad_rows(run, good):
    """run(row_frame, out) with two entries outside [0, B): those rows keep the prefill, the others are `good`."""
    f_bad, bad, ok = _bad_frames()
    out = torch.full_like(good, FILL)
    run(f_bad, out)
    assert torch.equal(out[ok], good[ok])
    assert (out[bad] == FILL).all()


@pytest.mark.parametrize('dtype', DTYPES)
def test_attention_rows(dtype):
    d, heads, HW = 32, 8, 7 * 9
    g = torch.Generator().manual_seed(501)
    qp_all = torch.randn(B * Q, d, generator=g).to(dtype).cuda()
    kp = torch.randn(B, HW, d, generator=g).to(dtype).cuda()
    mask = torch.zeros(B, 7, 9, dtype=torch.bool)
    mask[0, :, 7:] = True                                  # the two frames are padded differently
    mask[1, 5:, :] = True
    mask = mask.flatten(1).cuda()
    f, sel = _lists()
    qp = qp_all[f.long() * Q + torch.tensor(ROWS, device='cuda')]
    got = K.segm_attention_rows(qp, kp, mask, f, heads)
    assert got.shape == (len(ROWS), HW, heads) and got.dtype == dtype
    for b in range(B):
        want = K.segm_attention(qp[sel[b]], kp[b:b + 1], mask[b:b + 1], len(sel[b]), heads)
        assert torch.equal(got[sel[b]], want), (dtype, b)
    assert torch.equal(got[1], got[2]) and not torch.equal(got[0], got[3])
    assert (got[sel[0]].view(-1, 7, 9, heads)[:, :, 7:] == 0).all() and (got[sel[1]].view(-1, 7, 9, heads)[:, 5:] == 0).all()
    _check_bad_rows(lambda rf, out: K.segm_attention_rows(qp, kp, mask, rf, heads, out=out), got)


@pytest.mark.parametrize('dtype', DTYPES)
def test_lay1_rows(dtype):
    H, W, Ca, Cout = 7, 9, 8, 40
    g = torch.Generator().manual_seed(502)
    att = torch.rand(len(ROWS), H, W, Ca, generator=g).to(dtype).cuda()
    w_att = (torch.randn(3, 3, Ca, Cout, generator=g) * 0.2).cuda()
    frame = torch.randn(B, H, W, Cout, generator=g).cuda()
    f, sel = _lists()
    got = K.segm_lay1(att, w_att, frame, 0, 1, row_frame=f)
    assert got.shape == (len(ROWS), H, W, Cout) and got.dtype == dtype
    for b in range(B):
        want = K.segm_lay1(att[sel[b]].contiguous(), w_att, frame[b:b + 1], 0, len(sel[b]))
        assert torch.equal(got[sel[b]], want), (dtype, b)
    _check_bad_rows(lambda rf, out: K.segm_lay1(att, w_att, frame, 0, 1, row_frame=rf, out=out), got)


@pytest.mark.parametrize('dtype', DTYPES)
def test_gn_relu_up_add_rows(dtype):
    h, w, H, W, C, groups = 7, 9, 13, 18, 40, 8          # 5 channels per group: an 8-channel vector spans groups
    g = torch.Generator().manual_seed(503)
    x = torch.randn(len(ROWS), h, w, C, generator=g).to(dtype).cuda()
    gamma = (torch.rand(C, generator=g) + 0.5).cuda()
    beta = (torch.randn(C, generator=g) * 0.1).cuda()
    fpn = torch.randn(B, H, W, C, generator=g).to(dtype).cuda()
    f, sel = _lists()
    got = K.segm_gn_relu(x, gamma, beta, groups, fpn=fpn, row_frame=f)
    assert got.shape == (len(ROWS), H, W, C) and got.dtype == dtype
    for b in range(B):
        want = K.segm_gn_relu(x[sel[b]].contiguous(), gamma, beta, groups, fpn=fpn[b:b + 1], row0=0, Q=len(sel[b]))
        assert torch.equal(got[sel[b]], want), (dtype, b)
    _check_bad_rows(lambda rf, out: K.segm_gn_relu(x, gamma, beta, groups, fpn=fpn, row_frame=rf, out=out), got)
    # the form without an FPN operand reads nothing per frame
    plain = K.segm_gn_relu(x, gamma, beta, groups, row_frame=f)
    assert plain.shape == x.shape
    for b in range(B):
        assert torch.equal(plain[sel[b]], K.segm_gn_relu(x[sel[b]].contiguous(), gamma, beta, groups)), (dtype, b)


def test_wrappers_check_the_frame_list():
    x = torch.zeros(2, 7, 9, 8, device='cuda')
    w = torch.zeros(3, 3, 8, 40, device='cuda')
    fr = torch.zeros(1, 7, 9, 40, device='cuda')
    with pytest.raises(RuntimeError, match='int32'):
        K.segm_lay1(x, w, fr, 0, 1, row_frame=torch.zeros(2, dtype=torch.int64, device='cuda'))
    with pytest.raises(RuntimeError, match='one frame per row'):
        K.segm_lay1(x, w, fr, 0, 1, row_frame=torch.zeros(3, dtype=torch.int32, device='cuda'))
    with pytest.raises(RuntimeError, match='GPU only'):
        K.segm_lay1(x, w, fr, 0, 1, row_frame=torch.zeros(2, dtype=torch.int32))


# ---------------------------------------------------------------------------------- segmented resolve
OUT2, STALE_ONLY = (157, 301), [-1, -4, -2]
SEGMENTS = [   # (src, img_hw, out_hw, previous map's seed or None)
    (D.SLOTS, D.IMG_HW, D.OUT_HW, 92),
    ([], D.IMG_HW, (50, 70), None),                        # no slot: all -1
    ([0, 3, 2], D.MAX_HW, OUT2, None),                     # another crop and output size, rows 0 and 3 shared
    (STALE_ONLY, D.IMG_HW, D.OUT_HW, 95),
]


@pytest.fixture(scope='module')
def resolved():
    logits = D.make_logits().cuda()
    prevs = [None if seed is None else D.make_prev(out_hw, seed).cuda() for _, _, out_hw, seed in SEGMENTS]
    prev_off, parts, o = [], [], 0
    for p in prevs:
        prev_off.append(-1 if p is None else o)
        if p is not None:
            parts.append(p.flatten())
            o += p.numel()
    prev_packed = torch.cat(parts)
    src = [s for seg in SEGMENTS for s in seg[0]]
    src_off = np.cumsum([0] + [len(seg[0]) for seg in SEGMENTS])
    geom = [seg[1] + seg[2] for seg in SEGMENTS]
    args = (logits, torch.tensor(src, dtype=torch.int32, device='cuda'), src_off, geom, prev_packed, prev_off, D.MAX_HW)
    buf, stats, labels, pix_off = K.segm_track_resolve_segments(*args)
    want = [K.segm_track_resolve(logits, seg[0], prevs[i], D.MAX_HW, seg[1], seg[2], 0.5) for i, seg in enumerate(SEGMENTS)]
    torch.cuda.synchronize()
    return dict(args=args, buf=buf, stats=stats, labels=labels, pix_off=pix_off, src_off=src_off, want=want)


def test_segments_equal_the_single_resolves(resolved):
    labels, pix_off = resolved['labels'], resolved['pix_off']
    assert labels.dtype == torch.int16 and resolved['stats'].dtype == torch.int32
    assert pix_off.tolist() == np.cumsum([0] + [s[2][0] * s[2][1] for s in SEGMENTS]).tolist()
    assert resolved['buf'].numel() % 4 == 0
    assert resolved['buf'].numel() >= 20 * int(resolved['src_off'][-1]) + 2 * int(pix_off[-1])
    for i, (seg, want) in enumerate(zip(SEGMENTS, resolved['want'])):
        got = labels[pix_off[i]:pix_off[i + 1]].view(seg[2])
        assert torch.equal(got, want), i
    maps = [labels[pix_off[i]:pix_off[i + 1]] for i in range(4)]
    assert (maps[1] == -1).all()
    # the cases hold what they are meant to hold (slot 3 of segment 0 is the shadowed twin of slot 0)
    u0 = set(maps[0].unique().tolist())
    assert 3 not in u0 and {-1, 0, 1, 2} <= u0
    assert set(maps[2].unique().tolist()) >= {-1, 0} and set(maps[3].unique().tolist()) == {-1, 0, 1, 2}


def test_stats_are_the_labels_counts_and_boxes(resolved):
    stats = resolved['stats'].cpu().numpy()
    labels, pix_off, src_off = resolved['labels'].cpu().numpy(), resolved['pix_off'], resolved['src_off']
    assert stats.shape == (int(src_off[-1]), 5)
    empty = 0
    for i, seg in enumerate(SEGMENTS):
        lab = labels[pix_off[i]:pix_off[i + 1]].reshape(seg[2])
        for t in range(len(seg[0])):
            ys, xs = np.nonzero(lab == t)
            want = (len(ys), xs.min(), ys.min(), xs.max() + 1, ys.max() + 1) if len(ys) else (0, 0, 0, 0, 0)
            assert tuple(stats[src_off[i] + t].tolist()) == tuple(int(v) for v in want), (i, t)
            empty += not len(ys)
    assert empty >= 1                       # (slot 3 of segment 0, the identical row: never an owner)


def test_segments_rerun_is_byte_identical(resolved):
    out = torch.full((resolved['buf'].numel() + 64,), 0x5a, dtype=torch.uint8, device='cuda')
    buf, _, _, _ = K.segm_track_resolve_segments(*resolved['args'], out=out)
    used = 20 * int(resolved['src_off'][-1]) + 2 * int(resolved['pix_off'][-1])       # (then padding to 4 bytes)
    assert buf.data_ptr() == out.data_ptr() and torch.equal(buf[:used], resolved['buf'][:used])
    assert (out[buf.numel():] == 0x5a).all()


def test_more_slots_than_the_lds_table():
    """300 stale slots over a 64 x 80 map (five workgroups): the labels are the previous map, and the slots
    from 256 on take the kernel's global-atomic path."""
    T, hw = 300, (64, 80)
    g = torch.Generator().manual_seed(96)
    prev = torch.randint(-1, T, hw, generator=g).to(torch.int16).cuda()
    prev[:, :3] = 299
    src = [-t - 1 for t in range(T)]
    logits = torch.zeros(0, D.H, D.W, device='cuda')
    buf, stats, labels, pix_off = K.segm_track_resolve_segments(
        logits, torch.tensor(src, dtype=torch.int32, device='cuda'), [0, T], [D.IMG_HW + hw], prev.flatten(), [0], D.MAX_HW)
    assert torch.equal(labels.view(hw), prev)
    assert torch.equal(labels.view(hw), K.segm_track_resolve(logits, src, prev, D.MAX_HW, D.IMG_HW, hw, 0.5))
    lab, st = prev.cpu().numpy(), stats.cpu().numpy()
    for t in range(T):
        ys, xs = np.nonzero(lab == t)
        want = (len(ys), xs.min(), ys.min(), xs.max() + 1, ys.max() + 1) if len(ys) else (0, 0, 0, 0, 0)
        assert tuple(st[t].tolist()) == tuple(int(v) for v in want), t
    assert st[299, 0] >= 64 * 3 and (st[256:, 0] > 0).any()


def test_nothing_to_resolve_launches_nothing():
    from kinet_amd import _native as N
    logits = torch.zeros(0, D.H, D.W, device='cuda')
    N.trace_begin()
    buf, stats, labels, pix_off = K.segm_track_resolve_segments(logits, None, [0, 0, 0], [(0, 0, 0, 0)] * 2, None, None,
                                                                D.MAX_HW)
    assert N.trace_end() == [] and stats.shape == (0, 5) and labels.numel() == 0 and pix_off.tolist() == [0, 0, 0]


def test_wrapper_rejects_what_the_host_knows():
    logits = torch.zeros(1, D.H, D.W, device='cuda')
    src = torch.zeros(2, dtype=torch.int32, device='cuda')
    geom = [D.IMG_HW + D.OUT_HW]
    with pytest.raises(RuntimeError, match='int32'):
        K.segm_track_resolve_segments(logits, src.long(), [0, 2], geom, None, None, D.MAX_HW)
    with pytest.raises(RuntimeError, match='32767'):
        K.segm_track_resolve_segments(logits, src, [0, 40000], geom, None, None, D.MAX_HW)
    with pytest.raises(RuntimeError, match='inside'):
        K.segm_track_resolve_segments(logits, src, [0, 2], [D.MAX_HW + D.OUT_HW], None, None, D.IMG_HW)
    with pytest.raises(RuntimeError, match='prev_labels'):
        K.segm_track_resolve_segments(logits, src, [0, 2], geom, None, [0], D.MAX_HW)
    short = torch.zeros(10, dtype=torch.int16, device='cuda')
    with pytest.raises(RuntimeError, match='beyond'):
        K.segm_track_resolve_segments(logits, src, [0, 2], geom, short, [0], D.MAX_HW)


# ---------------------------------------------------------------------------------- the model
@pytest.fixture(scope='module')
def case_b(golden_dir):
    d = np.load(os.path.join(golden_dir, 'segm_b.npz'))
    model, post = R.build_case(golden_dir, 'b', int(d['seed']))
    model = model.cuda()
    model.tracking()
    return model


def test_mask_logits_rows_bit_identical(case_b):
    from kinet_amd import _native as N
    model = case_b
    frames = [f.cuda() for f in R.frames()]
    rows = torch.tensor([16, 3, 3, 0, 11, 7], device='cuda')
    mixed = torch.tensor(FRAMES, dtype=torch.int32, device='cuda')
    one = torch.zeros(len(FRAMES), dtype=torch.int32, device='cuda')
    with torch.no_grad():
        out0 = model(frames)[0]
        targets = []
        for b in range(len(frames)):
            top = out0['pred_logits'][b].sigmoid().max(-1)[0].topk(R.N_TRACK).indices
            targets.append({'track_query_hs_embeds': out0['hs_embed'][b, top], 'track_query_boxes': out0['pred_boxes'][b, top]})
        for dtype in DTYPES:
            model.set_compute_dtype(dtype)
            try:
                full = model(frames, targets)[0]['pred_masks']
                model.defer_masks = True
                assert 'pred_masks' not in model(frames, targets)[0]
                got = model.mask_logits_rows(rows, mixed)
                assert got.dtype == torch.float32 and got.shape == (len(FRAMES),) + R.FEATS[0]
                assert torch.equal(got, full[mixed.long(), rows]), dtype
                for b in range(len(frames)):            # the contract in mask_logits' terms
                    sel = mixed == b
                    assert torch.equal(got[sel], model.mask_logits(rows[sel], b)), (dtype, b)
                # the launches do not depend on how many frames the rows come from
                N.trace_begin()
                again = model.mask_logits_rows(rows, mixed)
                n_mixed = len(N.trace_end())
                N.trace_begin()
                same = model.mask_logits_rows(rows, one)
                n_one = len(N.trace_end())
                assert n_mixed == n_one and n_mixed > 0, (n_mixed, n_one)
                assert torch.equal(again, got) and torch.equal(same, full[0, rows])
                # chunks slice the frame list with the rows
                model.mask_query_chunk = 4
                assert torch.equal(model.mask_logits_rows(rows, mixed), got)
                model.mask_query_chunk = None
                N.trace_begin()
                empty = model.mask_logits_rows(rows[:0], mixed[:0])
                assert N.trace_end() == [] and empty.shape == (0,) + R.FEATS[0]
                with pytest.raises(RuntimeError, match='int32'):
                    model.mask_logits_rows(rows, mixed.long())
                model.defer_masks = False
                model(frames, targets)
                with pytest.raises(RuntimeError, match='defer_masks'):
                    model.mask_logits_rows(rows, mixed)
            finally:
                model.defer_masks = False
                model.mask_query_chunk = None
                model.set_compute_dtype(torch.float32)
