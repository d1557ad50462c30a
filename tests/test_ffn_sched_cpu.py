"""CPU-only proof of the ring schedule of the 8-wave x 32-row FFN kernel (csrc/ffn_sched.h through
kinet_ffn_sched): the schedule is replayed, role by role, against an event model of the ring that knows nothing of
the rules -- an in-order queue of each wave's LDS-DMA operations, retired by the vmcnt waits, and the barrier index as
the only clock.

Asserted for every walk (cnt tiles x (pch pre-chunks + nch hidden chunks)) and both roles:
  RAW   a chunk half is read only after the DMA of every wave has been waited for in front of a barrier that the
        reader has passed (every wave issues the same operations, so one queue per role stands for its waves);
  WAR   a half-slot is restaged only behind a barrier that every role reached after its last read of the slot's
        previous occupant (a read ahead of barrier q counts as made in interval q - 1);
  parity both roles execute the same number of barriers, one per ring chunk, with the indices 0 .. total - 1;
  vmcnt the argument of each wait equals a straight count of the operations younger than chunk q's two halves;
and that each role reads every half of every chunk exactly once between barriers (the reads ahead repeat nothing
else), from the slot it was staged into."""
import ctypes

import pytest

HALF_OPS = 2          # LDS-DMA operations of a wave per chunk half at D = 256 (FR / 8 waves / 2)
SLOTS = 3
F = dict(total=0, barriers=1, barrier=2, slot=3, vmcnt=4, n_issue=5, issue=6, n_early=12, early=13, n_read=19, read=20,
         fields=26)


def sched(role, cnt, pch, nch, q):
    from kinet_amd import _native
    out = (ctypes.c_int * F['fields'])()
    assert _native.lib().kinet_ffn_sched(role, cnt, pch, nch, q, HALF_OPS, ctypes.cast(out, ctypes.c_void_p)) == 0
    rec = list(out)

    def pairs(n, at):
        return [(rec[at + 2 * i], rec[at + 2 * i + 1]) for i in range(rec[n])]
    return dict(total=rec[F['total']], barriers=rec[F['barriers']], barrier=rec[F['barrier']], slot=rec[F['slot']],
                vmcnt=rec[F['vmcnt']], issue=pairs(F['n_issue'], F['issue']), early=pairs(F['n_early'], F['early']),
                read=pairs(F['n_read'], F['read']))


def walk(role, cnt, pch, nch):
    """Replays one role.  Returns (landed, reads, issued_at, barriers): landed[(chunk, half)] = index of the barrier
    in front of which the half's DMA was waited for; reads[(chunk, half)] = intervals in which it is read;
    issued_at[(chunk, half)] = barrier behind which it is issued (-1: prologue)."""
    total = cnt * (pch + nch)
    queue, landed, reads, issued_at = [], {}, {}, {}
    pro = sched(role, cnt, pch, nch, -1)
    assert pro['total'] == total and pro['early'] == [] and pro['read'] == []
    for h in pro['issue']:
        assert h not in issued_at
        issued_at[h] = -1
        queue += [h] * HALF_OPS
    barriers = 0
    for q in range(total):
        s = sched(role, cnt, pch, nch, q)
        assert s['total'] == total and s['barriers'] == total and s['slot'] == q % SLOTS
        # reads ahead of barrier q: made in interval q - 1
        for h in s['early']:
            reads.setdefault(h, []).append(q - 1)
        # the wait: a straight count of what is younger than chunk q's two halves
        assert all((q, x) in landed or (q, x) in queue for x in (0, 1)), 'chunk q was staged'
        younger = len(queue) - 1 - max([i for i, h in enumerate(queue) if h[0] == q], default=-1)
        assert s['vmcnt'] == younger, (q, s['vmcnt'], queue)
        retired, queue = queue[:len(queue) - s['vmcnt']], queue[len(queue) - s['vmcnt']:]
        for h in retired:
            if h not in queue:
                landed.setdefault(h, q)
        assert (q, 0) in landed and (q, 1) in landed
        # the barrier
        assert s['barrier'] == barriers == q
        barriers += 1
        for h in s['issue']:
            assert h not in issued_at, 'a half is staged once'
            issued_at[h] = q
            queue += [h] * HALF_OPS
        for h in s['read']:
            reads.setdefault(h, []).append(q)
    assert queue == [] and len(issued_at) == 2 * total
    return landed, reads, issued_at, barriers


CASES = [(cnt, pch, nch) for cnt in (1, 2, 3, 7) for pch in (0, 4) for nch in (1, 2, 3, 4, 5, 32, 64)]


@pytest.mark.parametrize('cnt,pch,nch', CASES, ids=lambda v: str(v))
def test_ring_schedule(cnt, pch, nch):
    total = cnt * (pch + nch)
    w = [walk(role, cnt, pch, nch) for role in (0, 1)]
    # parity: the same barriers for both roles, and the same DMA
    assert w[0][3] == w[1][3] == total
    assert w[0][2] == w[1][2]
    issued_at = w[0][2]
    for role in (0, 1):
        landed, reads, _, _ = w[role]
        for c in range(total):
            for half in (0, 1):
                h = (c, half)
                at = reads[h]
                # read between barriers exactly once; a read ahead only directly in front of that interval
                assert len(set(at)) <= 2 and max(at) - min(at) <= 1 and at == sorted(at), (role, h, at)
                # RAW: every role's waves waited for the half in front of a barrier the reader has passed
                # (a read in interval i is behind barrier i)
                for other in (0, 1):
                    assert w[other][0][h] <= min(at), (role, h, at, w[other][0][h])
                assert issued_at[h] < min(at)
                # WAR: the next occupant of the half-slot is staged behind a barrier later than the last read
                nxt = (c + SLOTS, half)
                if nxt in issued_at:
                    assert issued_at[nxt] > max(at), (role, h, at, issued_at[nxt])
                # ... and this one was staged after the previous occupant was staged and landed (one slot, in order)
                prev = (c - SLOTS, half)
                if prev in issued_at:
                    assert issued_at[h] >= landed[prev]
        assert set(reads) == {(c, half) for c in range(total) for half in (0, 1)}


def test_roles_differ_only_in_the_lag():
    """Role 0 reads a hidden chunk's two halves in its own interval; role 1 reads W2 (half 1) one interval later, its
    first fragments ahead of that barrier, except at a tile's last chunk; pre-chunks are read whole by both."""
    cnt, pch, nch = 2, 4, 3
    for q in range(cnt * (pch + nch)):
        r0, r1 = sched(0, cnt, pch, nch, q), sched(1, cnt, pch, nch, q)
        assert r0['read'] == [(q, 0), (q, 1)] and r0['early'] == []
        c = q % (pch + nch) - pch
        if c < 0:
            assert r1['read'] == r0['read'] and r1['early'] == []
            continue
        want = ([(q - 1, 1)] if c > 0 else []) + [(q, 0)] + ([(q, 1)] if c == nch - 1 else [])
        assert r1['read'] == want and r1['early'] == ([(q - 1, 1)] if c > 0 else [])
        assert r0['vmcnt'] == r1['vmcnt'] == (HALF_OPS if q + 1 < cnt * (pch + nch) else 0)


def test_refusals():
    from kinet_amd import _native
    out = (ctypes.c_int * F['fields'])()
    p = ctypes.cast(out, ctypes.c_void_p)
    L = _native.lib()
    assert L.kinet_ffn_sched(2, 1, 0, 1, 0, HALF_OPS, p) != 0
    assert L.kinet_ffn_sched(0, 1, 0, 1, 1, HALF_OPS, p) != 0
    assert L.kinet_ffn_sched(0, 1, 0, 1, -2, HALF_OPS, p) != 0
    assert L.kinet_ffn_sched(0, 1, 0, 1, 0, HALF_OPS, None) != 0
