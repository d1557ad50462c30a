"""Masks in the multi-sequence tracker, without a GPU: the ragged mask-head entry points and the segmented
resolve are declared, bound and check their arguments before they touch a device (csrc/segm.hip returns
KINET_ERR_ARG first), and plan_mask_resolve -- the host plan of one frame's resolve -- on hand-written cases."""
import os
import re
import types

import numpy as np
import pytest

from kinet_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['kinet_segm_attention_rows', 'kinet_segm_lay1_rows', 'kinet_segm_gn_relu_up_add_rows',
       'kinet_segm_track_resolve_segments']
F32, BAD_DTYPE = 0, 7
Z = None


def _err(name, *args):
    with pytest.raises(RuntimeError) as e:
        N.call(name, *args)
    return str(e.value)


def test_header_declares_and_native_binds_the_new_names():
    text = open(os.path.join(ROOT, 'include', 'kinet_segm.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in NEW:
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', text, flags=re.S)
        assert m, f'{name} is not declared in kinet_segm.h'
        assert len(m.group(1).split(',')) == len(N._SIGS[name]), name
        assert N.exported(name), name


# ---------------------------------------------------------------------------------- ragged head
def _att(qp=Z, kp=Z, mask=Z, rf=Z, out=Z, rows=3, B=2, HW=63, heads=8, d=32, dtype=F32):
    return ('kinet_segm_attention_rows', qp, kp, mask, rf, out, rows, B, HW, heads, d, 0.5, dtype, Z)


def _lay1(att=Z, w=Z, frame=Z, rf=Z, y=Z, rows=3, B=2, H=7, W=9, Ca=8, Cout=40, dtype=F32):
    return ('kinet_segm_lay1_rows', att, w, frame, rf, y, rows, B, H, W, Ca, Cout, dtype, Z)


def _gn(x=Z, gamma=Z, beta=Z, f=Z, rf=Z, y=Z, rows=3, B=2, h=7, w=9, H=7, W=9, C=40, groups=8, dtype=F32, ws=Z):
    return ('kinet_segm_gn_relu_up_add_rows', x, gamma, beta, f, rf, y, rows, B, h, w, H, W, C, groups, 1e-5, dtype, ws, Z)


def test_ragged_head_rejects_bad_arguments_before_any_launch():
    # null pointers with non-empty work (64, 128, ... stand for non-null pointers that are never followed)
    assert 'null pointer' in _err(*_att())
    assert 'row_frame' in _err(*_att(qp=64, kp=128, out=192))
    assert 'null pointer' in _err(*_att(rf=64))
    assert 'null pointer' in _err(*_lay1())
    assert 'row_frame' in _err(*_lay1(att=64, w=128, frame=192, y=256))
    assert 'null pointer' in _err(*_lay1(rf=64))
    assert 'null pointer' in _err(*_gn())
    assert 'row_frame' in _err(*_gn(x=64, gamma=128, beta=192, f=256, y=320, ws=384))
    assert 'null pointer' in _err(*_gn(rf=64, f=256))
    # a bad dtype
    for call in (_att, _lay1, _gn):
        assert 'dtype' in _err(*call(dtype=BAD_DTYPE, rf=64))
    # geometry
    assert '8 attention channels' in _err(*_lay1(Ca=4, rf=64))
    assert 'geometry' in _err(*_att(rows=-1))
    assert 'frame' in _err(*_att(B=0, rf=64))
    assert 'heads' in _err(*_att(heads=3, rf=64))
    assert 'geometry' in _err(*_lay1(rows=-1))
    assert 'multiple' in _err(*_gn(C=36, rf=64, f=256))
    assert 'FPN' in _err(*_gn(H=13, W=18))           # upsampling without an FPN operand


def test_ragged_head_empty_work_needs_no_pointer():
    assert N.call(*_att(rows=0)) == 0
    assert N.call(*_att(rows=0, B=0)) == 0
    assert N.call(*_lay1(rows=0)) == 0
    assert N.call(*_gn(rows=0)) == 0


# ---------------------------------------------------------------------------------- segmented resolve
GEO = (26, 50, 104, 200)                 # h, w, max_h, max_w


def _tables(src_off, geom, prev_off=None):
    so = np.ascontiguousarray(src_off, np.int32)
    ge = np.ascontiguousarray(geom, np.int32).reshape(-1, 4)
    px = ge[:, 2].astype(np.int64) * ge[:, 3]
    po = np.zeros(len(px) + 1, np.int64)
    po[1:] = np.cumsum(px)
    pv = np.full(len(px), -1, np.int64) if prev_off is None else np.ascontiguousarray(prev_off, np.int64)
    return so, ge, po, pv


def _resolve(tables, logits=Z, src=Z, prev=Z, labels=Z, stats=Z, S=None, total=None, n=1, geo=GEO):
    so, ge, po, pv = tables
    S = len(ge) if S is None else S
    total = int(so[-1]) if total is None else total
    return ('kinet_segm_track_resolve_segments', logits, src, so.ctypes.data, ge.ctypes.data, po.ctypes.data, prev,
            pv.ctypes.data, labels, stats, S, total, n, *geo, 0.5, Z)


def test_segmented_resolve_rejects_bad_arguments_before_any_launch():
    one = _tables([0, 2], [[88, 136, 131, 203]])
    assert 'geometry' in _err(*_resolve(one, S=-1))
    assert 'geometry' in _err(*_resolve(one, n=-1))
    assert 'geometry' in _err(*_resolve(one, geo=(0, 50, 104, 200)))
    assert '32767' in _err(*_resolve(_tables([0, 2, 32770], [[88, 136, 131, 203]] * 2)))
    assert 'ascend' in _err(*_resolve(_tables([0, 2, 1], [[88, 136, 131, 203]] * 2)))
    assert 'inside' in _err(*_resolve(_tables([0, 2], [[105, 136, 131, 203]])))
    assert 'inside' in _err(*_resolve(_tables([0, 2], [[88, 201, 131, 203]])))
    assert 'inside' in _err(*_resolve(_tables([0, 2], [[0, 136, 131, 203]])))
    so, ge, po, pv = one
    assert 'fit' in _err(*_resolve((so, ge, po - np.array([0, 1]), pv)))          # a map larger than its range
    assert 'beyond' in _err(*_resolve(one, total=1))
    assert 'host tables' in _err('kinet_segm_track_resolve_segments', Z, Z, Z, Z, Z, Z, Z, Z, Z, 1, 2, 1, *GEO, 0.5, Z)
    assert 'null pointer (labels)' in _err(*_resolve(one))
    assert 'null pointer (src, stats)' in _err(*_resolve(one, labels=64))
    assert 'null pointer (src, stats)' in _err(*_resolve(one, labels=64, src=128))
    assert 'null pointer (logits)' in _err(*_resolve(one, labels=64, src=128, stats=192))
    stale = _tables([0, 2], [[88, 136, 131, 203]], [0])
    assert 'null pointer (prev_labels)' in _err(*_resolve(stale, labels=64, src=128, stats=192, n=0))
    assert 'two buffers' in _err(*_resolve(stale, labels=64, prev=64, src=128, stats=192, n=0))


def test_segmented_resolve_empty_work_needs_no_pointer():
    assert N.call('kinet_segm_track_resolve_segments', Z, Z, Z, Z, Z, Z, Z, Z, Z, 0, 0, 0, *GEO, 0.5, Z) == 0
    # segments without slots and without a map: nothing to launch
    assert N.call(*_resolve(_tables([0, 0, 0], [[0, 0, 0, 0]] * 2), n=0)) == 0


def test_wrappers_need_gpu_tensors():
    import torch
    from kinet_amd import kernels as K
    with pytest.raises(RuntimeError, match='GPU only'):
        K.segm_attention_rows(torch.zeros(2, 32), torch.zeros(1, 63, 32), None, torch.zeros(2, dtype=torch.int32), 8)
    with pytest.raises(RuntimeError, match='GPU only'):
        K.segm_track_resolve_segments(torch.zeros(1, 26, 50), torch.zeros(1, dtype=torch.int32), [0, 1],
                                      [[88, 136, 131, 203]], None, None, (104, 200))


# ---------------------------------------------------------------------------------- the host plan
def _t(tid, row=None, slot=None, size=None):
    return types.SimpleNamespace(id=tid, mask_row=row, mask_slot=slot, mask_size=size)


def test_plan_mask_resolve():
    from kinet_amd.tracker import plan_mask_resolve
    hw, other = (120, 176), (96, 136)
    # sequence 0: fresh, stale, fresh; sequence 1: no track; sequence 2: one row named by two of its tracks,
    # a stale slot of its own frame size, and a row that sequence 0 named already (computed once)
    tracks = [[_t(0, row=7), _t(1, slot=0, size=hw), _t(2, row=3)],
              [],
              [_t(0, row=27), _t(5, row=27), _t(6, slot=4, size=other), _t(7, row=3)]]
    plan = plan_mask_resolve(tracks, [hw, hw, other])
    assert plan['rows'] == [7, 3, 27]
    assert plan['src'].dtype == np.int32 and plan['src'].tolist() == [0, -1, 1, 2, 2, -5, 1]
    assert plan['src_off'].dtype == np.int32 and plan['src_off'].tolist() == [0, 3, 3, 7]
    empty = plan_mask_resolve([[], []], [hw, hw])
    assert empty['rows'] == [] and empty['src'].size == 0 and empty['src_off'].tolist() == [0, 0, 0]
    with pytest.raises(RuntimeError, match='keeps a mask of size'):
        plan_mask_resolve([[_t(0, row=1)], [_t(3, slot=0, size=hw)]], [hw, other])
    with pytest.raises(RuntimeError, match='neither'):
        plan_mask_resolve([[_t(0, row=1), _t(9)]], [hw])
    # a row wins over a kept slot (Tracker._resolve_masks' order of the two questions)
    assert plan_mask_resolve([[_t(0, row=2, slot=1, size=other)]], [hw])['src'].tolist() == [0]


def test_multi_tracker_mask_refusals_without_a_gpu():
    from fake_detector import TRACKER_CFGS
    from fake_mask_detector import FakeMaskDetector
    from kinet_amd.models import DeformablePostProcess, PostProcessSegm
    from kinet_amd.tracker import MultiTracker
    det = FakeMaskDetector()
    cfg = TRACKER_CFGS['default']
    post = {'bbox': DeformablePostProcess(), 'segm': PostProcessSegm()}
    with pytest.raises(NotImplementedError, match='segm'):
        MultiTracker(det, {'bbox': post['bbox']}, dict(cfg, masks=True), 1)
    with pytest.raises(NotImplementedError, match='masks'):
        MultiTracker(det, post, cfg, 1)
    assert MultiTracker(det, post, dict(cfg, masks=True), 2).masks
