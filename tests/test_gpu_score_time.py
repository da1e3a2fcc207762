"""GPU (-m gpu): timed live predictions scored by time (stg_score_push_timed / stg_score_push_streams_timed of
csrc/score_time.hip) against the push-by-push restatement tests/score_time_np.py.

Bit-exact scripts of irregular pushes through the C ABI (every branch of the rule); the anchor on the device -- fed on
the grid, the timed pair of kernels reports what stg_track_push_rule + stg_score_push report --; real values through
FramePredictor(time=, score=TimedScoreSpec()), eager against captured and against the float64 restatement inside the
bounds of 5.17; four streams with their own clocks against four lone predictors, reset and capture."""
import argparse

import numpy as np
import pytest
import torch

import score_np
import score_time_inputs as sti
from frames_time_np import OVERFLOW, TIME_ORDER, StreamModelTimed
from live_inputs import _CPush, _model, _pushes
from score_time_np import TABLES, TRAJ, TimedScoreModel
from test_gpu_frames_time import _irregular_feed, _upsampled_eth
from test_gpu_score import U, _assert_cov, _d2_bounds, _real_covariance

pytestmark = pytest.mark.gpu
FLOATS = ("err", "d2", "nll", "best", "traj_ade", "traj_fde", "traj_ade_mean", "traj_fde_mean")
STATUS = {"pending": 1, "retired": 2}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _bits(a, b, name):
    """Two arrays bit for bit (the restatement's float fields are float32 values)."""
    if name in FLOATS:
        a, b = np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32)
    return np.array_equal(a, b)


def _assert_rows(state, s, model, k, what):
    """Stream s of a device ScoreTimedState (numpy) against the restatement's ring: rec_t, rec_status, rec_peds, the
    scene's ids, every table and -- for a retired row -- every trajectory value, the columns v < num_peds, bit for bit."""
    for r, rec in enumerate(model.rows):
        if rec is None:
            assert state["rec_status"][s, r] == 0, (what, r)
            continue
        c = rec["num_peds"]
        assert state["rec_status"][s, r] == STATUS[rec["status"]] and state["rec_t"][s, r] == rec["t"], (what, r)
        assert state["rec_peds"][s, r] == c and np.array_equal(state["rec_ids"][s, r], rec["ids"]), (what, r)
        names = TABLES + (("steps",) if rec["status"] == "pending" else TRAJ)
        for name in names:
            if state[name] is None:
                assert k == 0 and name in ("best", "traj_ade", "traj_fde"), (what, name)
                continue
            assert _bits(state[name][s, r][..., :c], rec[name][..., :c], name), \
                (what, r, name, state[name][s, r][..., :c], rec[name][..., :c])


# ---- 1. exact scripts through the C ABI --------------------------------------------------------------------------
class Harness:
    """ns streams: each stream's timed push (stg_track_push_timed on its slice of the (NS, ...) track state), then ONE
    score launch for the tick -- stg_score_push_streams_timed, or stg_score_push_timed with single=True and ns = 1 --
    beside one sti.StreamRef per stream.  tick(entries): entries[s] = None (not pushed) or (t, ids, xy, prediction)."""

    def __init__(self, dev, ns, p, v, k, thr, pending, r, single=False, m_max=sti.M_MAX, s=sti.SLOTS):
        from social_stgcnn_amd import ops
        self.ops, self.dev, self.ns, self.p, self.v, self.k, self.single = ops, dev, ns, p, v, k, single
        z = lambda shape, dt: torch.zeros(shape, device=dev, dtype=dt)      # noqa: E731
        self.tracks = (torch.full((ns, s), -1, device=dev, dtype=torch.int64), z((ns, s, r), torch.int64),
                       z((ns, s, r, 2), torch.float64), z((ns, s, 2), torch.int32), z((ns, 2), torch.int64),
                       z((ns, 2), torch.int32))
        self.push = []
        for b in range(ns):
            c = _CPush(dev, (2, 3), v, s, m_max, sti.T_OBS, 4, time=(sti.STEP, sti.MAX_DT, r))
            c.state = tuple(x[b] for x in self.tracks)
            c.slot_id, c.head_flags = c.state[0], c.state[5]
            self.push.append(c)
        self.state = ops.score_timed_state(ns, p, v, k, pending, dev, samples=k > 0, q=len(thr))
        self.thr = torch.tensor(list(thr), dtype=torch.float32).to(dev) if len(thr) else None
        self.refs = [sti.StreamRef(p, v, k, thr, pending, r, m_max=m_max, slots=s) for _ in range(ns)]
        self.scenes = [None] * ns                               # what each stream's last push returned on the device

    def snapshot(self):
        return {n: None if x is None else x.cpu().numpy() for n, x in zip(self.state._fields, self.state)}

    def tick(self, entries):
        ns, p, v, k = self.ns, self.p, self.v, self.k
        mean = np.zeros((ns, p, v, 2), np.float32)
        v_pred = np.zeros((ns, 5, p, v), np.float32)
        samples = np.zeros((k, ns, p, v, 2), np.float32)
        ids = np.full((ns, v), -1, np.int64)
        peds = np.zeros(ns, np.int32)
        pushed, want, flags = np.zeros(ns, np.int32), [], []
        for s, e in enumerate(entries):
            if e is None:
                want.append(self.refs[s].idle())
                flags.append(None)
                continue
            t, d_ids, d_xy, pr = e
            self.scenes[s] = self.push[s].push(d_ids, d_xy, t)
            f = self.scenes[s][4]
            f_ref, added = self.refs[s].push(t, d_ids, d_xy, pr)
            assert f == f_ref, (s, t, f, f_ref)
            flags.append(f)
            want.append(added)
            pushed[s] = 1
            mean[s], v_pred[s], ids[s], peds[s] = pr.mean, pr.v_pred, pr.ids, pr.num_peds
            if k:
                samples[:, s] = pr.samples
        t_ = lambda a: torch.from_numpy(a).to(self.dev)        # noqa: E731
        out = self.ops.score_timed_push(self.state, self.thr, t_(mean), t_(v_pred), t_(samples) if k else None, t_(ids),
                                        t_(peds), self.tracks, sti.STEP, sti.MAX_DT, 1e4,
                                        pushed=None if self.single else t_(pushed))
        got = [x.cpu().numpy() for x in out]
        for s in range(ns):                                     # what the push added: bit for bit (sums of float32
            assert np.array_equal(got[0][s], want[s]["push_totals"]), (s, got[0][s], want[s]["push_totals"])   # values
            assert np.array_equal(got[1][s], want[s]["push_traj"]), (s, got[1][s], want[s]["push_traj"])  # are exact)
        return flags

    def assert_state(self, what):
        st = self.snapshot()
        for s, ref in enumerate(self.refs):
            m = ref.score
            _assert_rows(st, s, m, self.k, (what, s))
            assert st["counters"][s].tolist() == [m.accepted, m.evictions], (what, s, st["counters"][s])
            assert np.allclose(st["totals"][s], m.totals, rtol=1e-12, atol=0), (what, s)
            assert np.allclose(st["traj_totals"][s], m.traj_totals, rtol=1e-12, atol=0), (what, s)
        return st


CASES = {                      # v, p, k, thr, r, pending, single
    "v5_p3_k3_q3_r2_pending_p": (5, 3, 3, (0.75, 3.0, 8.0), 2, 3, False),
    "v5_p3_k3_q3_r8_pending_4": (5, 3, 3, (0.75, 3.0, 8.0), 8, 4, False),
    "v5_p12_k3_q3_r8_pending_40": (5, 12, 3, (0.75, 3.0, 8.0), 8, 40, False),
    "v70_p12_k0_q0_r8_pending_40": (70, 12, 0, (), 8, 40, False),
    "v70_p3_k3_q0_r2_pending_40": (70, 3, 3, (), 2, 40, False),
    "v5_p12_k0_q3_r2_pending_4_single": (5, 12, 0, (0.75, 3.0, 8.0), 2, 4, True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_scripts_are_bit_exact(dev, case):
    """S 8 slots, step 4, max_dt 8, 60 irregular pushes a stream (score_time_inputs.script: an id that leaves and
    returns, one that leaves for good, brackets wider than max_dt, two horizons in one bracket, a repeated id, an empty
    push, OVERFLOW, a push back in time).  Three streams; stream 1 sits out the ticks 7, 8 and 41 (its state stays bit
    for bit, its outputs are zero), stream 2 is reset before tick 35.  After every tick what the push added, and every
    fifth tick the whole ring -- tables, retired rows, counters -- equal the restatement evaluated in float32 bit for
    bit; the running totals to 1e-12."""
    from social_stgcnn_amd import ops
    v, p, k, thr, r, pending, single = CASES[case]
    ns = 1 if single else 3
    h = Harness(dev, ns, p, v, k, thr, pending, r, single)
    scripts = [sti.script(s, p, v, k) for s in range(ns)]
    cursor = [0] * ns
    flags_seen = refused = 0
    for n in range(64):
        if n == 35 and ns == 3:
            ops.score_timed_reset(h.state, torch.tensor([2]).to(dev))
            h.refs[2].score.reset()
        entries = []
        for s in range(ns):
            if (s == 1 and n in (7, 8, 41)) or cursor[s] >= len(scripts[s]):
                entries.append(None)
                continue
            entries.append(scripts[s][cursor[s]][:4])
            cursor[s] += 1
        if all(e is None for e in entries):
            break
        before = [x.clone() for x in h.state if x is not None]
        flags = h.tick(entries)
        for s, f in enumerate(flags):
            if f is None or f & TIME_ORDER:                     # not pushed, or refused: nothing moves
                refused += f is not None
                for a, b in zip((x for x in h.state if x is not None), before):
                    assert torch.equal(a[s], b[s]), (case, n, s)
            else:
                flags_seen |= f
        if n % 5 == 4:
            h.assert_state((case, n))
    st = h.assert_state(case)
    assert cursor == [len(x) for x in scripts] and refused == ns and flags_seen & OVERFLOW
    assert st["totals"][:, :, 0].sum() > 150 * ns
    if pending <= 4:
        assert (st["counters"][:, 1] > 3).all()
    else:
        assert not st["counters"][:, 1].any() and st["traj_totals"][:, 0].sum() > 20
    if thr:
        assert 0 < st["totals"][..., 5].sum() < st["totals"][..., 7].sum() < st["totals"][..., 0].sum()


EDGES = {                      # p, v, k, thr: the shapes at which the helpers of score_fn.hpp take another path
    "k0": (3, 5, 0, (0.75, 3.0)),                        # no samples: best, traj_ade and traj_fde are absent
    "q0": (3, 5, 2, ()),
    "p1": (1, 5, 2, (0.75, 3.0)),
    "v65": (3, 65, 2, (0.75, 3.0)),                      # a scene of 65: two lane passes, the second with one live lane
    "peds0": (3, 5, 2, (0.75, 3.0)),                     # every other prediction holds no pedestrian
}


@pytest.mark.parametrize("single", (False, True), ids=("streams", "lone"))
@pytest.mark.parametrize("case", sorted(EDGES))
def test_edge_shapes_are_bit_exact(dev, case, single):
    """S 8 slots, M_max 8, R 2, pending 4, a dozen pushes a stream (score_time_inputs.edge_script) through
    stg_score_push_streams_timed (two streams, stream 1 sits out the ticks 2 and 6) and through stg_score_push_timed
    (one stream): after every tick what the push added, every fourth tick and at the end the whole ring -- tables,
    retired rows, counters -- equal the restatement evaluated in float32, bit for bit."""
    p, v, k, thr = EDGES[case]
    ns = 1 if single else 2
    h = Harness(dev, ns, p, v, k, thr, 4, 2, single, m_max=8)
    scripts = [sti.edge_script(s, p, v, k, case == "peds0") for s in range(ns)]
    last = sti.edge_script(0, p, v, k, case == "peds0", n_push=13)[12]
    cursor = [0] * ns
    for n in range(14):
        entries = []
        for s in range(ns):
            if (s == 1 and n in (2, 6)) or cursor[s] >= len(scripts[s]):
                entries.append(None)
                continue
            entries.append(scripts[s][cursor[s]])
            cursor[s] += 1
        if all(e is None for e in entries):                     # (the lone entry point has no `pushed`)
            break
        assert not any(f for f in h.tick(entries) if f is not None), (case, n)     # (no OVERFLOW, nothing refused)
        if n % 4 == 3:
            h.assert_state((case, n))
    st = h.assert_state(case)
    assert cursor == [12] * ns and st["counters"][:, 0].tolist() == [12] * ns
    assert all((st[name] is None) == (k == 0) for name in ("rec_samples", "acc", "best", "traj_ade", "traj_fde"))
    assert st["totals"].shape[2] == 5 + len(thr) and (st["totals"][:, :, 0].sum(axis=1) > 10).all()
    assert (st["traj_totals"][:, 0] > 2).all()
    if case == "v65":
        assert st["matched"][..., 64].any() and not st["matched"][..., 5:64].any()
    # the covariance sum at this shape on real sigma and rho channels (the scripts hold C_h = h I): a thirteenth push of
    # stream 0, its record against the float64 sum
    h.tick([last[:3] + (_real_covariance(last[3], 5),)] + [None] * (ns - 1))
    row = (int(h.state.counters[0, 0]) - 1) % 4
    assert int(h.state.counters[0, 0]) == 13
    _assert_cov(h.state.rec_cov[0, row].cpu().numpy(), last[3], case)


def test_a_ring_of_two_through_the_push_the_harvest_and_the_score(dev):
    """R = 2, the smallest ring: the search sees at most one old sample, and "the sample before the newest" is the slot
    the push has just overwritten -- the edge of every helper of time_samples.hpp.  S 16, V 8, P 3, K 2, T_obs 8, step 4,
    max_dt 8; the harvest with windows of 9 frames, settle 0.  score_time_inputs.ring2_script through
    stg_track_push_timed, stg_window_harvest_timed and stg_score_push_timed, each against its statement bit for bit
    after every push: the scene, the decoded rings, the history, clock and log, what the score added and, every fourth
    push, its whole ring.  The statements hold interpolated scene positions, entries scored between two pushes and
    harvested windows with interpolated frames."""
    import ctypes
    import harvest_time_np as HT
    from social_stgcnn_amd._lib import check, lib, ptr, stream_ptr
    p, v, k, thr, s, t_all, caps = 3, 8, 2, (0.75, 3.0), 16, 9, (32, 256)
    h = Harness(dev, 1, p, v, k, thr, 4, 2, single=True, s=s)
    ref = h.refs[0]
    z = lambda shape, dt: torch.zeros(shape, device=dev, dtype=dt)      # noqa: E731
    hist = (z(s, torch.int32), z((t_all, s, 2), torch.float64), z(2, torch.int32), z(3, torch.int64))
    log = (torch.full((caps[1], 2, t_all), 7.0, device=dev), torch.full((caps[0] + 1,), -7, device=dev, dtype=torch.int32),
           torch.full((caps[0], 2), -7, device=dev, dtype=torch.int32), z(3, torch.int32))
    log[1][0] = 0
    hv = HT.TimedHarvester(1, t_all, sti.STEP, sti.MAX_DT, 0, *caps)
    hv.log.rel_all[:], hv.log.win_start[1:], hv.log.win_tag[:] = 7.0, -7, -7
    script = sti.ring2_script(p, v, k)
    in_scene = 0
    for n, (t, ids, xy, pred) in enumerate(script):
        assert h.tick([(t, ids, xy, pred)]) == [0], n            # the push, then the score: what it added
        out_ids, peds, obs, seen, _ = h.scenes[0]
        want = ref.scene
        assert peds == len(want[0]) and np.array_equal(out_ids[:peds], want[0]) and np.array_equal(seen[:peds], want[2]), n
        assert obs[:, :peds].tobytes() == want[1].tobytes(), n
        in_scene += sti.interpolated_in_scene(want, ref.track.tracks, t)
        check(lib().stg_window_harvest_timed(*(ptr(x[0]) for x in h.tracks), s, 2, sti.T_OBS, t_all, 2, ctypes.c_double(1e4),
                                             sti.STEP, sti.MAX_DT, 0, 0, *map(ptr, hist), *map(ptr, log), *caps,
                                             stream_ptr()), "stg_window_harvest_timed")
        host = [x[0].cpu().numpy() for x in h.tracks]
        tracks = HT.decode_tracks(*host[:4])
        assert tracks == ref.track.tracks and all(len(smp) <= 2 for smp in tracks.values()), n
        hv.tick({0: (tracks, t, True)})
        for got, wanted in zip(log, (hv.log.rel_all, hv.log.win_start, hv.log.win_tag, hv.log.header)):
            assert got.cpu().numpy().tobytes() == wanted.tobytes(), n
        word, ring, head, clock = (x.cpu().numpy() for x in hist)
        assert head.tolist() == hv.hist[0].head and clock.tolist() == hv.hist[0].clock, n
        assert HT.same_runs(HT.canonical(host[0], word, ring, head, t_all), hv.hist[0].runs), n
        if n % 4 == 3:
            h.assert_state(n)
    h.assert_state("end")
    assert in_scene > 0 and sti.interpolated_in_records(ref.score.rows, [e[0] for e in script]) > 0
    assert int(hv.log.header[0]) >= 1 and int(hv.log.header[2]) == 0 and hv.hist[0].interpolated > 0


# ---- 2. the anchor on the device ---------------------------------------------------------------------------------
@pytest.mark.parametrize("p,pending", [(3, 4), (12, 40)])
def test_on_the_grid_the_timed_kernels_are_the_push_indexed_ones(dev, p, pending):
    """One stream fed at t = 4 f with max_dt = step = 4 (the script's detections and predictions, its times replaced by
    the grid; 16 slots, so no OVERFLOW) through stg_track_push_timed + stg_score_push_timed and through
    stg_track_push_rule + stg_score_push: the entries (record of push m, horizon h) are what the push-indexed kernel
    reports at push m + h in row h - 1, the retired rows its traj_* of push m + P, bit for bit; the totals agree to
    1e-12 (the order of summation differs)."""
    from social_stgcnn_amd import ops
    v, k, thr, s, step = 5, 3, (0.75, 3.0, 8.0), 16, 4
    timed = _CPush(dev, (2, 3), v, s, sti.M_MAX, sti.T_OBS, 4, time=(step, step, 8))
    ruled = _CPush(dev, (2, 3), v, s, sti.M_MAX, sti.T_OBS, 4)
    st_t = ops.score_timed_state(1, p, v, k, pending, dev, q=len(thr))
    st_u = ops.score_state(1, p, v, k, dev, q=len(thr))
    thr_d = torch.tensor(thr, dtype=torch.float32).to(dev)
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    feed = [e for e in sti.script(0, p, v, k) if not e[4]]
    peds, compared, retired = [], 0, 0
    for f, (_, ids, xy, _, _) in enumerate(feed):
        t = step * f - 50
        a, b = timed.push(ids, xy, t), ruled.push(ids, xy)
        assert a[4] == b[4] and not a[4] & OVERFLOW, f
        scene = list(dict.fromkeys(reversed(ids.tolist())))[:v - f % 2]
        pr = sti.exact_prediction(scene, t, p, v, k, step)
        peds.append(pr.num_peds)
        pred = (t_(pr.mean[None]), t_(pr.v_pred[None]), t_(pr.samples[:, None]), t_(pr.ids[None]),
                t_(np.array([pr.num_peds], np.int32)))
        m = max(len(ids), sti.M_MAX)
        det_id, det_xy = np.zeros(m, np.int64), np.zeros((m, 2))
        det_id[:len(ids)], det_xy[:len(ids)] = ids, xy
        ops.score_timed_push(st_t, thr_d, *pred, timed.state, step, step, 1e4)
        out = ops.score_push(st_u, thr_d, *pred, t_(det_id), t_(det_xy), sti.M_MAX, 1e4,
                             det_count=t_(np.array([len(ids)], np.int32)))
        for h in range(1, min(f, p) + 1):
            row, c = (f - h) % pending, peds[f - h]
            for name in TABLES:
                assert torch.equal(getattr(st_t, name)[0, row, h - 1, :c], getattr(out, name)[0, h - 1, :c]), (f, h, name)
                compared += int(getattr(out, name)[0, h - 1, :c].ne(0).sum())
        if f >= p:
            row, c = (f - p) % pending, peds[f - p]
            assert int(st_t.rec_status[0, row]) == 2, f
            for name in TRAJ:
                assert torch.equal(getattr(st_t, name)[0, row, :c], getattr(out, name)[0, :c]), (f, name)
            retired += int((out.traj_steps[0, :c] == p).sum())
    assert compared > 2000 and retired > 50 and not st_t.counters[0, 1].item()
    assert torch.equal(st_t.totals[..., 0], st_u.totals[..., 0]) and torch.equal(st_t.totals[..., 5:], st_u.totals[..., 5:])
    assert np.allclose(st_t.totals.cpu().numpy(), st_u.totals.cpu().numpy(), rtol=1e-12, atol=0)
    assert np.allclose(st_t.traj_totals.cpu().numpy(), st_u.traj_totals.cpu().numpy(), rtol=1e-12, atol=0)


# ---- 3. real values through the frame predictor ------------------------------------------------------------------
def _state_np(pred):
    st = pred._score_state
    return {n: None if x is None else x.cpu().numpy() for n, x in zip(st._fields, st)}


def test_frame_predictor_eager_captured_and_restatement(dev):
    """biwi_eth's first 60 frames upsampled 4x (a push every 5 ticks, step 20, max_dt 20) through
    FramePredictor(time=, score=TimedScoreSpec(pending=256)), k 3, max_peds 16: every record of the 240 pushes stays in
    the ring.  Eager and captured (captured in mid-stream: the records and totals stay) leave bit-equal states.  Against
    the float64 restatement fed the device's own mean, v_pred and samples -- both sides take the truth from the same
    samples by the same IEEE operations, so it is the same float32 --: matched / steps / status exact, err / best 1e-6
    and the trajectory errors 2e-6 relative, d2 / nll inside the per-element bounds of 5.17 (test_gpu_score._d2_bounds);
    the coverage counts are the device's own d2 against the float32 thresholds exactly, and agree with the float64 d2
    outside 1e-3 of a threshold, the comparisons left out for that capped at 0.5 %.  Pedestrians cross this scene in
    a few seconds: 553 entries are scored at h = 1, 16 at h = 12, and 16 trajectories are full.  Measured on the MI355X:
    err 1.3e-7, best 1.2e-7, traj 1.4e-7, d2 1.0e-6 relative (largest bound 8.9e-5), nll 2.5e-5 absolute; 0 of 8,145
    coverage comparisons left out."""
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.predict import TimedScoreSpec
    rows, _ = _upsampled_eth()
    fine, ticks = _pushes(rows), np.unique(rows[:, 0]).astype(np.int64).tolist()
    model = _model("eth", dev)
    k, v, p, pending = 3, 16, 12, 256
    spec = TimedScoreSpec((0.5, 0.9, 0.99), True, pending)
    kw = dict(k=k, capacity=64, max_peds=v, max_detections=32, time=frames.TimeRule(20, 20, 48), score=spec)
    eager, cap = frames.FramePredictor(model, **kw), frames.FramePredictor(model, **kw)
    track = StreamModelTimed(8, 20, 20, 48, max_peds=v, capacity=64, max_detections=32)
    ref = TimedScoreModel(p, v, k, 20, 20, pending, spec.thresholds)
    assert eager.score is None and eager.score_totals[0].shape == (1, p, 8) and eager.score_records.rec_t.shape == (1, 256)
    replay = None
    for n, ((ids, xy), t) in enumerate(zip(fine, ticks)):
        if n == 40:
            before = [x.clone() for x in cap._score_state if x is not None]
            replay = cap.capture()
            for a, b in zip((x for x in cap._score_state if x is not None), before):
                assert torch.equal(a, b)
        e = eager.push(ids, xy, t=t, seed=n)
        c = replay(ids, xy, t=t, seed=n) if replay else cap.push(ids, xy, t=t, seed=n)
        assert torch.equal(e.samples, c.samples) and int(e.flags) == 0
        for a, b, name in zip(eager.score, cap.score, eager.score._fields):
            assert torch.equal(a, b), (n, name)
        track.push(ids, xy, t)
        ref.push(track.tracks, t, score_np.Prediction(e.ids.cpu().numpy(), int(e.num_peds[0]), e.mean.cpu().numpy(),
                                                      e.v_pred.cpu().numpy(), e.samples.cpu().numpy()))
    for a, b, name in zip(eager._score_state, cap._score_state, eager._score_state._fields):
        assert torch.equal(a, b), name
    st = _state_np(eager)
    thr32 = np.asarray(spec.thresholds, np.float32)
    worst = dict(err=0.0, best=0.0, traj=0.0, d2=0.0, d2_bound=0.0, nll=0.0)
    sums = np.zeros((p, 5 + len(thr32)))
    tsum = np.zeros(5)
    left_out = counted = 0
    for r, rec in enumerate(ref.rows[:len(fine)]):
        c = rec["num_peds"]
        assert st["rec_t"][0, r] == rec["t"] and st["rec_status"][0, r] == STATUS[rec["status"]] and st["rec_peds"][0, r] == c
        assert np.array_equal(st["matched"][0, r, :, :c], rec["matched"][:, :c]), r
        assert np.array_equal(st["steps"][0, r, :c], rec["steps"][:c]), r
        on = rec["matched"][:, :c] == 1
        got = {n: st[n][0, r, :, :c].astype(np.float64) for n in TABLES[1:]}
        for name in ("err", "best"):
            assert not got[name][~on].any(), (r, name)
            rel = np.abs(got[name][on] - rec[name][:, :c][on]) / rec[name][:, :c][on]
            worst[name] = max(worst[name], float(rel.max(initial=0.0)))
        assert not got["d2"][~on].any() and not got["nll"][~on].any(), r
        d2_rel, det_rel = _d2_bounds(rec["cov"][:, :c][on], p)
        d2r, nr = rec["d2"][:, :c][on], rec["nll"][:, :c][on]
        rel = np.abs(got["d2"][on] - d2r) / d2r
        assert (rel <= d2_rel).all(), (r, rel.max(initial=0.0), d2_rel.max(initial=0.0))
        mag = 0.5 * d2r + np.abs(nr - 0.5 * d2r - score_np.LOG_2PI) + score_np.LOG_2PI
        bound = 0.5 * d2_rel * d2r + 0.5 * det_rel * 1.01 + 4 * U * mag
        assert (np.abs(got["nll"][on] - nr) <= bound).all(), r
        worst["d2"] = max(worst["d2"], float(rel.max(initial=0.0)))
        worst["d2_bound"] = max(worst["d2_bound"], float(d2_rel.max(initial=0.0)))
        worst["nll"] = max(worst["nll"], float(np.abs(got["nll"][on] - nr).max(initial=0.0)))
        inside_dev = st["d2"][0, r, :, :c][..., None] <= thr32
        near = np.abs(rec["d2"][:, :c][..., None] - thr32.astype(np.float64)) <= 1e-3 * thr32
        assert np.array_equal((inside_dev & on[..., None])[~near], ((rec["d2"][:, :c][..., None] <= thr32) & on[..., None])[~near])
        left_out += int((near & on[..., None]).sum())
        counted += int(on.sum()) * len(thr32)
        sums[:, 0] += on.sum(axis=1)
        for i, name in enumerate(TABLES[1:]):
            sums[:, 1 + i] += np.where(on, got[name], 0.0).sum(axis=1)
        sums[:, 5:] += (inside_dev & on[..., None]).sum(axis=1)
        if rec["status"] == "retired":
            assert np.array_equal(st["traj_steps"][0, r, :c], rec["traj_steps"][:c]), r
            full = rec["traj_steps"][:c] == p
            for i, name in enumerate(TRAJ[1:]):
                a, b = st[name][0, r, :c].astype(np.float64), rec[name][:c]
                nz = b != 0
                assert not a[~nz].any(), (r, name)
                worst["traj"] = max(worst["traj"], float((np.abs(a[nz] - b[nz]) / b[nz]).max(initial=0.0)))
                tsum[1 + i] += a[full].sum()
            tsum[0] += full.sum()
    print("timed score real inputs: worst %s; left out %d of %d" % (worst, left_out, counted))
    assert worst["err"] <= 1e-6 and worst["best"] <= 1e-6 and worst["traj"] <= 2e-6
    assert counted > 5000 and left_out <= 0.005 * counted, (left_out, counted)
    tot, trj = st["totals"][0], st["traj_totals"][0]
    assert np.array_equal(tot[:, 0], sums[:, 0]) and np.array_equal(tot[:, 5:], sums[:, 5:]) and tot[:, 0].min() >= 10
    assert np.allclose(tot, sums, rtol=1e-9, atol=0) and np.allclose(trj, tsum, rtol=1e-9, atol=0) and trj[0] >= 10
    assert np.array_equal(tot[:, 0], ref.totals[:, 0]) and np.allclose(tot[:, [1, 4]], ref.totals[:, [1, 4]], rtol=1e-5)
    assert st["counters"][0].tolist() == [240, 0] and not eager.score_evictions.any()
    s = frames.score_summary(*eager.score_totals, spec.levels)
    assert s.count.shape == (1, p) and s.err[0, -1] > s.err[0, 0] and s.trajectories[0] == trj[0]
    eager.reset()
    assert not eager.score_totals[0].any() and not eager.score_records.rec_status.any()
    assert not eager.score_records.counters.any() and (eager.score_records.rec_ids == -1).all()


# ---- 4. streams --------------------------------------------------------------------------------------------------
def test_streams_with_their_own_clocks_equal_lone_predictors(dev):
    """Four streams, each its own irregular feed and clock (stream 3 in microseconds); stream s sits out the ticks
    n % 5 == s.  With explicit noise the whole score state of stream s is that of a lone FramePredictor fed that
    stream's pushes with noise[:, s:s+1], bit for bit; a stream not pushed keeps its state and adds nothing.  capture()
    leaves records and totals alone, captured ticks go on from them; reset([s]) clears that stream alone."""
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.predict import TimedScoreSpec
    ns, n_ticks, k, v, p = 4, 48, 2, 8, 12
    model = _model("eth", dev)
    feeds = [_irregular_feed(300 + s, n_push=n_ticks, n_ids=8) for s in range(ns)]
    spec = TimedScoreSpec((0.9,), True, 32)
    kw = dict(k=k, capacity=16, max_peds=v, max_detections=8, tracks=(2, 3), time=frames.TimeRule(10, 10, 16), score=spec)
    sp = frames.StreamsPredictor(model, ns, **kw)
    lone = [frames.FramePredictor(model, **kw) for _ in range(ns)]
    cursor = [0] * ns
    gen = torch.Generator()
    gen.manual_seed(5)
    fields = sp._score_state._fields

    def tick_of(n):
        go = [s for s in range(ns) if n % 5 != s]
        tick = {s: feeds[s][cursor[s]] for s in go}
        return tick, {s: (i, q) for s, (t, i, q) in tick.items()}, {s: t for s, (t, i, q) in tick.items()}
    for n in range(36):
        tick, dets, times = tick_of(n)
        noise = torch.randn((k, ns, p, v, 2), generator=gen).to(dev)
        before = [x.clone() for x in sp._score_state]
        sp.push(dets, times=times, noise=noise)
        for s in range(ns):
            if s not in tick:
                assert not sp.score.push_totals[s].any() and not sp.score.push_traj[s].any(), (n, s)
                for a, b in zip(sp._score_state, before):
                    assert torch.equal(a[s], b[s]), (n, s)
                continue
            t, i, q = tick[s]
            lone[s].push(i, q, t=t, noise=noise[:, s:s + 1])
            cursor[s] += 1
            for a, b, name in zip(sp.score, lone[s].score, sp.score._fields):
                assert torch.equal(a[s], b[0]), (n, s, name)
            for a, b, name in zip(sp._score_state, lone[s]._score_state, fields):
                assert torch.equal(a[s], b[0]), (n, s, name)
    assert sp.score_totals[0][..., 0].sum() > 400
    assert torch.equal(sp.score_evictions, sp.score_records.counters[:, 1]) and not sp.score_evictions.any()
    before = [x.clone() for x in sp._score_state]
    replay = sp.capture()
    for a, b in zip(sp._score_state, before):
        assert torch.equal(a, b)
    drawn = ("rec_samples", "acc", "best", "traj_ade", "traj_fde", "totals", "traj_totals")    # in-kernel draws differ
    for n in range(36, n_ticks):
        tick, dets, times = tick_of(n)
        replay(dets, times=times, seed=n)
        for s, (t, i, q) in tick.items():
            lone[s].push(i, q, t=t, seed=n)
            cursor[s] += 1
            for a, b, name in zip(sp._score_state, lone[s]._score_state, fields):
                if name not in drawn:
                    assert torch.equal(a[s], b[0]), (n, s, name)
            assert torch.equal(sp.score_totals[0][s][:, :4], lone[s].score_totals[0][0][:, :4]), (n, s)
    keep = [x.clone() for x in sp._score_state]
    sp.reset([2])
    others = [0, 1, 3]
    for a, b, name in zip(sp._score_state, keep, fields):
        assert torch.equal(a[others], b[others]), name
        assert bool((a[2] == (-1 if name == "rec_ids" else 0)).all()), name
    assert keep[fields.index("totals")][2].any()


# ---- 5. the command ----------------------------------------------------------------------------------------------
def test_the_command_scores_an_upsampled_recording(dev, tmp_path):
    """predict_frames --step 20 --score on 80 pushes of the upsampled recording: the score_* arrays are the summary of a
    FramePredictor(time=, score=TimedScoreSpec(pending=64)) pushed the same way, captured as the command captures it."""
    from social_stgcnn_amd import frames, predict_frames
    from social_stgcnn_amd.predict import TimedScoreSpec
    from social_stgcnn_amd.trainer import Checkpoint
    model = _model("eth", dev)
    rows, _ = _upsampled_eth()
    rows = rows[rows[:, 0] <= np.unique(rows[:, 0])[79]]
    rec = str(tmp_path / "fine.txt")
    np.savetxt(rec, rows, fmt=["%d", "%d", "%.17g", "%.17g"], delimiter="\t")
    args = argparse.Namespace(n_stgcnn=1, n_txpcnn=5, output_size=5, obs_seq_len=8, kernel_size=3, pred_seq_len=12,
                              dataset="eth")
    ck = Checkpoint(str(tmp_path / "social-stgcnn-eth") + "/", args)
    ck.record(0, model, 1.0, 0.5)
    out = str(tmp_path / "scored.npz")
    common = ["--checkpoint", ck.dir, "--recording", rec, "--ksteps", "3", "--seed", "3", "--history", "48",
              "--max_peds", "16", "--out", out]
    predict_frames.main(common + ["--step", "20", "--score", "--pending", "64"])
    npz = np.load(out)
    _, fs, ids, xy = frames.sorted_rows(rows)
    m_max = int(np.diff(fs).max())
    spec = TimedScoreSpec(pending=64)
    fp = frames.FramePredictor(model, k=3, max_peds=16, max_detections=m_max, time=frames.TimeRule(20, None, 48),
                               score=spec)
    replay = fp.capture()
    for n, t in enumerate(np.unique(rows[:, 0]).astype(np.int64).tolist()):
        replay(ids[fs[n]:fs[n + 1]], xy[fs[n]:fs[n + 1]], t=t, seed=3 + n)
    s = frames.score_summary(*fp.score_totals, spec.levels)
    for name, x in zip(s._fields[:-1], s[:-1]):
        assert np.array_equal(npz["score_" + name], np.asarray(x)[0], equal_nan=True), name
    assert npz["score_levels"].tolist() == [0.5, 0.9, 0.99] and int(npz["score_evictions"]) == 0
    assert npz["score_count"].shape == (12,) and npz["score_coverage"].shape == (12, 3) and npz["score_count"][0] > 100
    assert npz["score_count"][7] > 0 and npz["score_count"][-1] == 0           # (the restatement's counts: 128, 108, .., 12 at h = 8, 0 at 11, 12)
    for bad, what in ((["--score"], "--score needs --step"), (["--score", "--associate", "1.0"], "--score needs --step")):
        with pytest.raises(ValueError, match=what):
            predict_frames.main(common + bad)
