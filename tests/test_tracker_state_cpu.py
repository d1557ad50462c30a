"""The track state machine of Tracker, TrackerKinematic and MultiTracker on the CPU: the six tracker
kernels (K.nms, K.track_decide, K.nms_segments, K.track_commit, K.track_gather, K.track_reid_dist) are
replaced by the restatements of multi_track_refs.py, the detectors by the fixtures' stand-ins, and every
run must reproduce the reference fixtures (tracker.npz, tracker_kinematic.npz) with the comparisons of
test_tracker_gpu.py -- and, line for line, the logger output and the order of the K.* calls recorded in
tests/golden/tracker_logs.json.  That recording is data: it was written by this module's generator
(`python tests/test_tracker_state_cpu.py`) from the tracker as it stood before its per-frame rules were
folded into shared functions, and is regenerated only when the tracker's behaviour is meant to change."""
import json
import os

import numpy as np
import pytest
import torch

import multi_track_refs as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CFG_NAMES = ['default', 'reid_lsa', 'public_iou', 'reid_greedy']
MULTI_SEEDS = [0, 1, 0]
# MultiTracker.sync_count over 20 frames of MULTI_SEEDS with the stand-in kernels
MULTI_SYNCS = {'default': 59, 'reid_lsa': 77, 'public_iou': 35, 'reid_greedy': 59}


def _stand_ins(setattr_):
    """Replace the six kernels through `setattr_(module, name, value)` -> the list every logger line
    ('log: ...') and kernel call ('K.<name>') of the run is appended to, in order."""
    from kinet_amd import kernels as K
    events = []

    def spy(name, fn):
        def call(*a, **kw):
            events.append('K.' + name)
            return fn(*a, **kw)
        return call
    for name, fn in R.KERNEL_ADAPTERS.items():
        setattr_(K, name, spy(name, fn))
    return events, lambda line: events.append('log: ' + line)


def _logs(events):
    return [e for e in events if e.startswith('log: ')]


def run_tracker(setattr_, name, seq):
    from fake_detector import TRACKER_CFGS, FakeDetector, sequence_blobs
    from kinet_amd.models import DeformablePostProcess
    from kinet_amd.tracker import Tracker
    events, logger = _stand_ins(setattr_)
    tracker = Tracker(FakeDetector(seed=seq), {'bbox': DeformablePostProcess()}, TRACKER_CFGS[name], logger=logger)
    tracker.reset()
    for blob in sequence_blobs(seq, 20):
        tracker.step(blob)
    return tracker, events


def run_kinematic(setattr_, name, enc, seq):
    from fake_detector import KINEMATIC_CFGS, FakeKinetDetector, kinematic_args, kinematic_blobs
    from kinet_amd.models import DeformablePostProcess
    from kinet_amd.tracker import TrackerKinematic
    events, logger = _stand_ins(setattr_)
    det = FakeKinetDetector(n_frames=5, encoded=enc == 'sine', seed=seq)
    tracker = TrackerKinematic(det, {'bbox': DeformablePostProcess()}, KINEMATIC_CFGS[name],
                               kinematic_args(enc == 'sine'), logger=logger)
    tracker.reset()
    for blob in kinematic_blobs(seq, 25):
        tracker.step(blob)
    return tracker, events


def run_multi(setattr_, name, seeds):
    from fake_detector import TRACKER_CFGS, sequence_blobs
    from kinet_amd.models import DeformablePostProcess
    from kinet_amd.tracker import MultiTracker
    events, logger = _stand_ins(setattr_)
    tracker = MultiTracker(R.BatchedFakeDetector(seeds), {'bbox': DeformablePostProcess()}, TRACKER_CFGS[name],
                           len(seeds), logger=logger)
    blobs = [sequence_blobs(s, 20) for s in seeds]
    for f in range(20):
        tracker.step([b[f] for b in blobs])
    return tracker, events


def _check_fixture(d, key, results, track_num, num_reids):
    """test_tracker_gpu.py::test_tracker_matches_reference's comparisons."""
    from fake_detector import flatten_results
    ids, vals = flatten_results(results)
    np.testing.assert_array_equal(ids.numpy(), d[f'{key}_ids'])
    np.testing.assert_allclose(vals.numpy(), d[f'{key}_vals'], rtol=1e-5, atol=1e-3)
    assert num_reids == int(d[f'{key}_reids'])
    assert track_num == int(d[f'{key}_tracks'])


@pytest.fixture(scope='module')
def recording():
    with open(os.path.join(GOLDEN, 'tracker_logs.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('name', CFG_NAMES)
@pytest.mark.parametrize('seq', [0, 1])
def test_tracker_matches_reference(monkeypatch, golden_dir, recording, name, seq):
    tracker, events = run_tracker(monkeypatch.setattr, name, seq)
    _check_fixture(np.load(os.path.join(golden_dir, 'tracker.npz')), f'{name}_{seq}', tracker.get_results(),
                   tracker.track_num, tracker.num_reids)
    assert events == recording[f'tracker/{name}/{seq}']


@pytest.mark.parametrize('name', ['kinet', 'kinet_nms'])
@pytest.mark.parametrize('enc', ['id', 'sine'])
@pytest.mark.parametrize('seq', [0, 1])
def test_tracker_kinematic_matches_reference(monkeypatch, golden_dir, recording, name, enc, seq):
    tracker, events = run_kinematic(monkeypatch.setattr, name, enc, seq)
    _check_fixture(np.load(os.path.join(golden_dir, 'tracker_kinematic.npz')), f'{name}_{enc}_{seq}',
                   tracker.get_results(), tracker.track_num, tracker.num_reids)
    assert events == recording[f'kinematic/{name}/{enc}/{seq}']


@pytest.mark.parametrize('name', CFG_NAMES)
def test_multi_tracker_matches_reference(monkeypatch, golden_dir, recording, name):
    tracker, events = run_multi(monkeypatch.setattr, name, MULTI_SEEDS)
    d = np.load(os.path.join(golden_dir, 'tracker.npz'))
    for i, seed in enumerate(MULTI_SEEDS):
        q = tracker.sequence(i)
        _check_fixture(d, f'{name}_{seed}', tracker.get_results()[i], q.track_num, q.num_reids)
    assert tracker.sync_count == MULTI_SYNCS[name]
    assert events == recording[f'multi/{name}']


@pytest.mark.parametrize('name', CFG_NAMES)
@pytest.mark.parametrize('seq', [0, 1])
def test_one_sequence_multi_tracker_logs_what_tracker_logs(monkeypatch, recording, name, seq):
    _, single = run_tracker(monkeypatch.setattr, name, seq)
    _, multi = run_multi(monkeypatch.setattr, name, [seq])
    assert _logs(multi) == _logs(single)
    assert len(_logs(single)) >= 20         # (a FRAME line per frame at the least)
    assert multi == recording[f'multi_one/{name}/{seq}']


def make_recording():
    """Every run of this module -> {run: [event, ...]} (see the module docstring)."""
    rec = {}
    for name in CFG_NAMES:
        for seq in (0, 1):
            rec[f'tracker/{name}/{seq}'] = run_tracker(setattr, name, seq)[1]
            rec[f'multi_one/{name}/{seq}'] = run_multi(setattr, name, [seq])[1]
        rec[f'multi/{name}'] = run_multi(setattr, name, MULTI_SEEDS)[1]
    for name in ('kinet', 'kinet_nms'):
        for enc in ('id', 'sine'):
            for seq in (0, 1):
                rec[f'kinematic/{name}/{enc}/{seq}'] = run_kinematic(setattr, name, enc, seq)[1]
    return rec


if __name__ == '__main__':
    import sys
    sys.path[:0] = [os.path.dirname(GOLDEN), os.path.dirname(os.path.dirname(GOLDEN)), GOLDEN]
    torch.manual_seed(0)
    with open(os.path.join(GOLDEN, 'tracker_logs.json'), 'w') as f:
        json.dump(make_recording(), f, indent=0, sort_keys=True)
        f.write('\n')
