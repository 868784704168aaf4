"""tests/chain_ref.py (the plain model of psn_t2d_chain_begin_device /
psn_t2d_chain_step_device that test_chain_step_gpu.py holds the kernels to)
against the oracle's own schedule, tracker2d_oracle.backward_tracking
(PSNWhere_Tracker2D.cpp:690-838), without a GPU: the LK call is replaced by
prescribed displacements, the model is driven through begin and three steps
with the buffer hand-over of the device pass, and its boxes and point sets
must be the oracle's. Also shown here: the poison comparison of the device
tests fails on a single write outside the promised set."""
import numpy as np
import pytest

import chain_ref
import tracker2d_oracle as ORC

CAP = 100

# detection k has its features at x in [100 k + 30, 100 k + 60): the stand-in LK
# knows the detection from its first point; (n features, plan per chain step)
PLANS = [(40, ("shift", "shift", "shift")),     # the full chain
         (3, ("shift", "shift", "shift")),      # fewer than MIN_FEATURES: no object
         (30, ("shift", "static", "shift")),    # stops at step 2 (fewer than half move)
         (25, ("scatter", "shift", "shift")),   # stops at step 1 (fewer than 4 inliers): set 0 = its features
         (12, ("shift", "shift", "scatter")),   # stops at step 3
         (120, ("shift", "shift", "shift"))]    # more features than the cap: the first 100


def _frames():
    return [np.full((2, 2), i, np.uint8) for i in range(4)]  # ring[-1 - s] carries 3 - s


def _fake_lk(cur_img, prev_img, pts, win):
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    s = 3 - int(prev_img[0, 0])
    assert int(cur_img[0, 0]) == 4 - s
    k = int(pts[0, 0] // 100)
    plan = PLANS[k][1][s - 1]
    i = np.arange(len(pts), dtype=np.float64)
    if plan == "static":
        d = np.zeros((len(pts), 2))
    elif plan == "scatter":
        d = np.stack([5 + 10 * i, 5 - 7 * i], 1)
    else:
        d = np.tile([1.5 + 0.25 * s, -0.75 * s], (len(pts), 1)) + np.stack([(i % 3) * 0.125, (i % 2) * 0.25], 1)
        out = i % 5 == 4
        d[out] = np.stack([15 + 3 * i[out], -20 - 2 * i[out]], 1)
    return (pts + d).astype(np.float32), np.ones(len(pts), np.uint8)


def _inputs():
    rng = np.random.default_rng(11)
    boxes = [(100.0 * k + 20, 50.0, 30.0, 60.0) for k in range(len(PLANS))]
    feats = [np.stack([rng.uniform(100 * k + 30, 100 * k + 60, n), rng.uniform(55, 100, n)], 1).astype(np.float32)
             for k, (n, _) in enumerate(PLANS)]
    return boxes, feats


def _drive_model(ring, boxes, feats, last):
    ndet = len(boxes)
    cnt = [min(len(f), CAP) for f in feats]  # the host upload's clamp (:753-757)
    st = chain_ref.poison(chain_ref.ChainState(ndet, CAP, boxes, cnt, None if last is None else [last] * ndet))
    cur0 = np.full((ndet, CAP, 2), np.nan, np.float32)
    for k, f in enumerate(feats):
        cur0[k, :cnt[k]] = f[:CAP]
    chain_ref.begin(st, cur0, ORC.MIN_FEATURES)
    cur = cur0
    for s in range(1, 4):
        nxt = np.full((ndet, CAP, 2), np.nan, np.float32)
        for k in range(ndet):
            n = int(st.cnt[k])
            if n:
                nxt[k, :n] = _fake_lk(ring[-s], ring[-1 - s], cur[k, :n], None)[0]
        chain_ref.poison_next_in(st)
        chain_ref.step(st, s, cur, nxt)
        cur = st.next_in.copy()  # the pass hands next_in over as the next step's input
    return st


@pytest.mark.parametrize("older", [3, 2])
def test_model_matches_backward_tracking(monkeypatch, older):
    """older = 2: a ring with only two older frames (the chain ends at step 2)."""
    monkeypatch.setattr(ORC, "_lk", _fake_lk)
    ring = _frames()
    for i in range(3 - older):
        ring[i] = None
    boxes, feats = _inputs()
    objs = ORC.backward_tracking(ring, [ORC.Rect(*b) for b in boxes], feats)
    st = _drive_model(ring, boxes, feats, None if older == 3 else older)
    kept = [k for k, f in enumerate(feats) if len(f) >= ORC.MIN_FEATURES]
    assert [o.id for o in objs] == kept == [0, 2, 3, 4, 5]
    for o, k in zip(objs, kept):
        ns = int(st.nsteps[k])
        assert [b.tuple() for b in o.boxes] == [boxes[k]] + [tuple(st.out_boxes[k, s]) for s in range(1, ns + 1)], k
        assert len(o.sets) == ns + 1, k
        for s in range(ns + 1):
            np.testing.assert_array_equal(chain_ref.bits(st.sets[k, s, :st.set_cnt[k, s]]), chain_ref.bits(o.sets[s]),
                                          err_msg=f"detection {k} set {s}")
        assert (st.set_cnt[k, ns + 1:] == 0).all()
    # the scenario holds what it claims (the schedule's branches)
    assert [int(st.nsteps[k]) for k in kept] == [min(3, older), 1, 0, 2, min(3, older)]
    assert st.nsteps[1] == 0 and st.set_cnt[1, 0] == 0 and st.cnt[1] == 0  # 3 features: gated, no set 0
    assert st.set_cnt[3, 0] == 25 and st.set_cnt[5, 0] <= CAP


def test_poison_check_bites():
    """One element written outside the promised set (the slot after the last
    inlier of a point set) fails the comparison the device tests use; the
    promised writes alone pass it."""
    rng = np.random.default_rng(3)
    pre, cur = chain_ref.klt_case(rng, 40, "cluster")
    st = chain_ref.ChainState(2, CAP, [(10.0, 20.0, 10.0, 60.0)] * 2, [40, 0])
    a = np.full((2, CAP, 2), np.nan, np.float32)
    b = a.copy()
    a[0, :40], b[0, :40] = pre, cur
    want, got = chain_ref.poison(st.copy()), chain_ref.poison(st.copy())
    chain_ref.step(want, 2, a, b)
    chain_ref.step(got, 2, a, b)
    ninl = int(want.set_cnt[0, 2])
    assert 4 <= ninl < 40 and want.cnt[1] == 0
    chain_ref.assert_states_equal(got, want)
    for name, at in (("sets", (0, 2, ninl, 0)), ("next_in", (0, ninl, 1)), ("sets", (0, 0, 0, 0)), ("set_cnt", (0, 0)),
                     ("out_boxes", (1, 2, 0)), ("nsteps", (1,))):
        bad = got.copy()
        getattr(bad, name)[at] = 1  # a stray write
        with pytest.raises(AssertionError, match=name):
            chain_ref.assert_states_equal(bad, want)
    neg = got.copy()
    neg.out_boxes[0, 2, 0] = 0.0
    want0 = want.copy()
    want0.out_boxes[0, 2, 0] = -0.0
    with pytest.raises(AssertionError, match="out_boxes"):  # the integer views tell -0.0 from 0.0
        chain_ref.assert_states_equal(neg, want0)
