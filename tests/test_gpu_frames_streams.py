"""GPU (-m gpu): many live streams in one launch chain per tick (frames.StreamsPredictor, stg_track_push_streams).

Every stream against the push-by-push restatement (frames_np.StreamModel) fed only that stream's pushes, eager and
captured; every stream against a lone FramePredictor -- scenes, flags, track state and predictions --; the Philox draws
against Predictor.predict on the same tick; isolation of the edge cases and of reset; more streams than one round of
push workgroups, with v_pred against lone predictors and the fp64 oracle; the entry point's refusals."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
import frames_np
from live_inputs import Schedule, _assert_scene, _model, _pushes, _recordings, _rows, _xy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _assert_empty(out_np, s, what):
    ids, peds, obs, flags, pushed = out_np
    assert int(peds[s]) == 0 and np.all(ids[s] == -1) and not np.any(obs[s]), what
    assert int(flags[s]) == 0 and not pushed[s], what


def _host(out):
    return (out.ids.cpu().numpy(), out.num_peds.cpu().numpy(), out.obs_abs.cpu().numpy(), out.flags.cpu().numpy(),
            out.pushed.cpu().numpy())


def _check_restatement(out_np, tick, refs, what):
    """Each pushed stream's scene is its restatement's; a stream not pushed has the empty scene."""
    ids, peds, obs, flags, pushed = out_np
    for s, det in enumerate(tick):
        if det is None:
            _assert_empty(out_np, s, (what, s))
            continue
        assert pushed[s], (what, s)
        r_ids, r_obs = refs[s].push(*det)
        _assert_scene(ids[s], peds[s], obs[s], r_ids, r_obs, (what, s))


def test_streams_equal_the_restatement_eager_and_captured(dev):
    """14 streams, one per committed recording, staggered starts, odd streams skipping ticks: every scene is the
    restatement's, no flag is ever raised, and the captured ticks equal the eager ones bit for bit."""
    from social_stgcnn_amd import frames
    recs = _recordings()
    assert len(recs) == 14
    pushes = [_pushes(_rows(*r)) for r in recs]
    n_ticks = max(len(p) for p in pushes)
    model = _model("eth", dev)
    k = 2
    eager = frames.StreamsPredictor(model, 14, k=k)
    cap = frames.StreamsPredictor(model, 14, k=k)
    replay = cap.capture()
    sched = Schedule(pushes, [3 * s for s in range(14)])
    refs = [frames_np.StreamModel() for _ in range(14)]
    most = np.zeros(14, np.int64)
    for t in range(n_ticks):
        tick = sched.tick(t)
        e = eager.push(tick, seed=t)
        c = replay(tick, seed=t)
        for a, b, name in zip(e, c, e._fields):
            assert torch.equal(a, b), (t, name)
        out_np = _host(e)
        assert not np.any(out_np[3]), t
        assert np.array_equal(out_np[4], np.array([d is not None for d in tick])), t
        _check_restatement(out_np, tick, refs, t)
        most = np.maximum(most, out_np[1])
    assert sched.cursor[0] == len(pushes[0])                          # the first stream ran its whole recording
    assert int(most.max()) == 73


def _state(sp, s):
    return [x[s].clone() for x in (sp.slot_id, sp.mask, sp.ring, sp.head_flags)]


def _lone_state(fp):
    return [fp.slot_id, fp.mask, fp.ring, fp.head_flags]


def test_streams_equal_lone_frame_predictors(dev):
    """NS = 6 (students001 twice at different offsets: scenes up to 73 pedestrians, the team kernels; four other
    recordings; an empty push) with explicit noise, max_peds 128: each pushed stream's scene, flags, track state and
    predictions equal a lone FramePredictor fed that stream's pushes with noise[:, s:s+1], bit for bit; a stream not
    pushed keeps its state bit for bit and gets the empty scene and the predictions of an empty scene."""
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.predict import Predictor
    names = [("univ_test", "students001.txt"), ("univ_test", "students001.txt"), ("eth_test", "biwi_eth.txt"),
             ("zara1_test", "crowds_zara01.txt"), ("univ_test", "students003.txt"), ("hotel_test", "biwi_hotel.txt")]
    pushes = [_pushes(_rows(*r)) for r in names]
    pushes[5] = pushes[5][:20] + [(np.zeros(0, np.int64), np.zeros((0, 2)))] + pushes[5][20:]     # an empty push
    ns, k, v, p = 6, 3, 128, 12
    model = _model("univ", dev)
    sp = frames.StreamsPredictor(model, ns, k=k, max_peds=v)
    lone = [frames.FramePredictor(model, k=k, max_peds=v) for _ in range(ns)]
    pred = Predictor(model, k)
    sched = Schedule(pushes, [0, 45, 2, 5, 7, 11])
    gen = torch.Generator()
    gen.manual_seed(5)
    biggest = 0
    for t in range(90):
        tick = sched.tick(t)
        noise = torch.randn((k, ns, p, v, 2), generator=gen).to(dev)
        before = [_state(sp, s) for s in range(ns)]
        out = sp.push(tick, noise=noise)
        out_np = _host(out)
        idle = [s for s in range(ns) if tick[s] is None]
        if idle:
            empty = pred.predict(torch.zeros((len(idle), 8, v, 2), device=dev, dtype=torch.float64),
                                 torch.zeros(len(idle), device=dev, dtype=torch.int32), noise=noise[:, idle])
        for s in range(ns):
            if tick[s] is None:
                _assert_empty(out_np, s, (t, s))
                for a, b in zip(_state(sp, s), before[s]):
                    assert torch.equal(a, b), (t, s)
                j = idle.index(s)
                assert torch.equal(out.v_pred[s], empty.v_pred[j]), (t, s)
                assert torch.equal(out.mean[s], empty.mean[j]), (t, s)
                assert torch.equal(out.samples[:, s], empty.samples[:, j]), (t, s)
                continue
            r = lone[s].push(*tick[s], noise=noise[:, s:s + 1])
            assert out_np[4][s], (t, s)
            assert torch.equal(out.ids[s], r.ids) and torch.equal(out.num_peds[s:s + 1], r.num_peds), (t, s)
            assert torch.equal(out.obs_abs[s:s + 1], r.obs_abs) and torch.equal(out.flags[s:s + 1], r.flags), (t, s)
            for a, b in zip(_state(sp, s), _lone_state(lone[s])):
                assert torch.equal(a, b), (t, s)
            assert torch.equal(out.v_pred[s], r.v_pred), (t, s)
            assert torch.equal(out.mean[s], r.mean), (t, s)
            assert torch.equal(out.samples[:, s], r.samples), (t, s)
            biggest = max(biggest, int(out_np[1][s]))
    assert biggest == 73
    assert sched.cursor[5] > 21                                           # the empty push was made


def test_captured_draws_are_the_predictors(dev):
    """The captured tick's samples are Predictor.predict's on the same tick's obs_abs / num_peds / seed (the draws are
    keyed by the scene's index in the tick); another seed changes the samples and not the mean.  Capture leaves the
    track state as it was."""
    from social_stgcnn_amd import frames
    from social_stgcnn_amd.predict import Predictor
    names = [("eth_test", "biwi_eth.txt"), ("zara2_test", "crowds_zara02.txt"), ("univ_test", "students003.txt"),
             ("zara1_test", "crowds_zara01.txt")]
    pushes = [_pushes(_rows(*r)) for r in names]
    model = _model("zara2", dev)
    sp = frames.StreamsPredictor(model, 4, k=5)
    sched = Schedule(pushes, [0, 1, 0, 2], skip=False)
    for t in range(30):
        sp.push(sched.tick(t))
    before = [x.clone() for x in (sp.slot_id, sp.mask, sp.ring, sp.head_flags)]
    replay = sp.capture()
    for a, b in zip((sp.slot_id, sp.mask, sp.ring, sp.head_flags), before):
        assert torch.equal(a, b)
    pred = Predictor(model, 5)
    seen = 0
    for t in range(30, 36):
        out = replay(sched.tick(t), seed=100 + t)
        ref = pred.predict(out.obs_abs, out.num_peds, seed=100 + t)
        assert torch.equal(out.samples, ref.samples), t
        assert torch.equal(out.mean, ref.mean) and torch.equal(out.v_pred, ref.v_pred), t
        other = pred.predict(out.obs_abs, out.num_peds, seed=200 + t)
        assert torch.equal(other.mean, out.mean), t
        if int(out.num_peds.sum()):
            assert not torch.equal(other.samples, out.samples), t
            seen += 1
    assert seen >= 5


def _device_tick(tick, ns, dev, host_counts=False):
    """A host tick as a frames.DeviceTick (counts -1 where not pushed; a device tensor, or a host list)."""
    from social_stgcnn_amd import frames
    got = [d for d in tick if d is not None]
    ids = np.concatenate([d[0] for d in got]) if got else np.zeros(0, np.int64)
    xy = np.concatenate([d[1] for d in got]) if got else np.zeros((0, 2))
    counts = [len(d[0]) if d is not None else -1 for d in tick]
    return frames.DeviceTick(torch.from_numpy(ids.astype(np.int64)).to(dev), torch.from_numpy(xy).to(dev),
                             counts if host_counts else torch.tensor(counts, dtype=torch.int32).to(dev))


def test_edge_cases_stay_in_their_stream(dev):
    """The scripts of the single-stream edge cases, each in one stream, beside clean streams.  Defaults (capacity
    1024, max_peds 128, max_detections 1024), detections as device tensors (the counts on the device, or on the host
    every other tick): repeated ids (DUPLICATE, the first
    detection wins), a device count of 1,030 (TRUNCATED, the first 1,024 used), 130 fully observed pedestrians
    (TOO_MANY, the 128 smallest ids kept), beside two recordings; reset([s]) restarts that stream alone.  Capacity 3:
    the overflow script (OVERFLOW) beside two clean streams of at most three ids.  Every flag shows in its own stream
    only and every clean stream equals the restatement."""
    from social_stgcnn_amd import frames
    model = _model("eth", dev)
    gen = np.random.default_rng(0)
    recs = [_pushes(_rows("eth_test", "biwi_eth.txt")), _pushes(_rows("univ_test", "students003.txt"))]
    ns = 5
    for mode in ("eager", "captured"):
        sp = frames.StreamsPredictor(model, ns, k=2)
        push = sp.push if mode == "eager" else sp.capture()
        refs = [frames_np.StreamModel() for _ in range(ns)]
        many = np.arange(1000, 1130, dtype=np.int64)[::-1].copy()
        for t in range(40):
            if t == 25:
                sp.reset([3])
                refs[3] = frames_np.StreamModel()
            dup = np.array([4, 9, 4, 1] if t % 3 == 0 else [9, 4, 1], np.int64)
            trunc = np.arange(2000, 3030, dtype=np.int64) if t % 4 == 1 else np.arange(2000, 2010, dtype=np.int64)
            tick = [(dup, _xy(gen, len(dup))), (trunc, _xy(gen, len(trunc))),
                    (many, _xy(gen, len(many))) if t < 10 else None, recs[0][t], recs[1][t]]
            out = push(_device_tick(tick, ns, dev, host_counts=t % 2 == 1))
            ids, peds, obs, flags, pushed = _host(out)
            assert pushed.tolist() == [d is not None for d in tick], (mode, t)
            expect = [frames.DUPLICATE if t % 3 == 0 else 0, frames.TRUNCATED if t % 4 == 1 else 0,
                      frames.TOO_MANY if 7 <= t < 10 else 0, 0, 0]
            assert flags.tolist() == expect, (mode, t)
            for s, det in enumerate(tick):
                if det is None:
                    _assert_empty((ids, peds, obs, flags, pushed), s, (mode, t, s))
                    continue
                d_ids, d_xy = det
                if s == 1:
                    d_ids, d_xy = d_ids[:1024], d_xy[:1024]
                r_ids, r_obs = refs[s].push(d_ids, d_xy)
                _assert_scene(ids[s], peds[s], obs[s], r_ids, r_obs, (mode, t, s))
                if s == 3 and 25 <= t < 32:
                    assert int(peds[s]) == 0, (mode, t)                 # restarted: obs_len - 1 empty pushes
        assert refs[4].hist and len(refs[3].hist) == 15                 # the others went on
        # capacity 3: 1, 2 and 3 arrive first and hold the three slots; every other id finds no free slot
        script = []
        for f in range(40):
            ids = [1, 2]
            if f != 10:
                ids.append(3)
            if f < 3 or 12 <= f < 30:
                ids.append(4)
            if f >= 5:
                ids.append(5 + f % 3)
            if f == 20:
                ids = []
            ids = np.array(ids[::-1] if f % 2 else ids, np.int64)
            script.append((ids, _xy(gen, len(ids))))
        sp = frames.StreamsPredictor(model, 3, k=2, capacity=3, max_detections=8)
        push = sp.push if mode == "eager" else sp.capture()
        refs = [frames_np.StreamModel() for _ in range(3)]
        n_over = 0
        for f, (ids, xy) in enumerate(script):
            clean = np.array([7, 5, 6], np.int64) if f % 5 else np.array([5, 7], np.int64)
            tick = [(ids, xy), (clean, _xy(gen, len(clean))), None if f % 2 else (clean[:2], _xy(gen, 2))]
            out = push(tick)
            o_np = _host(out)
            o_ids, o_peds, o_obs, o_flags, _ = o_np
            keep = np.isin(ids, [1, 2, 3])
            r_ids, r_obs = refs[0].push(ids[keep], xy[keep])
            _assert_scene(o_ids[0], o_peds[0], o_obs[0], r_ids, r_obs, (mode, f))
            assert o_flags[0] in (0, frames.OVERFLOW) and o_flags[1] == 0 and o_flags[2] == 0, (mode, f)
            n_over += int(o_flags[0] == frames.OVERFLOW)
            for s in (1, 2):
                if tick[s] is not None:
                    r_ids, r_obs = refs[s].push(*tick[s])
                    _assert_scene(o_ids[s], o_peds[s], o_obs[s], r_ids, r_obs, (mode, f, s))
                else:
                    _assert_empty(o_np, s, (mode, f, s))
        assert n_over > 20, mode


def _push_groups(threads, m_max, s):
    """Push workgroups of stg_track_push_streams that fit the chip at once: 256 CUs, 32 waves and 160 KiB of LDS per
    CU (the dynamic LDS of the launch plus the kernel's static wave counters and flag)."""
    m2 = 1
    while m2 < m_max:
        m2 <<= 1
    lds = m2 * 12 + m_max * 4 + s * 8 + 4 * (threads // 64) + 4
    return 256 * min(32 // (threads // 64), 160 * 1024 // lds)


def test_more_streams_than_one_round_of_workgroups(dev):
    """800 streams at capacity 2048 / max_detections 2048 (48 KB of LDS per push workgroup: more streams than fit the
    chip at once), the recordings cycled with staggered starts, 60 captured ticks: every scene bit for bit against the
    restatement; v_pred of sampled streams against lone FramePredictors at 1e-5 and of sampled scenes against the fp64
    oracle at 1e-4 (NS >= 384: the team kernels chunk the batch differently from N = 1)."""
    from oracle import stgcnn_oracle as O
    from social_stgcnn_amd import frames
    ns, cap, m_max = 800, 2048, 2048
    threads = frames.STREAM_THREADS
    assert ns >= 600 and ns > _push_groups(threads, m_max, cap), _push_groups(threads, m_max, cap)
    recs = _recordings()
    all_pushes = {r: _pushes(_rows(*r)) for r in recs}
    pushes = [all_pushes[recs[s % 14]][(s // 14) * 3 % 200:] for s in range(ns)]
    model = _model("univ", dev)
    w = load_golden("weights_univ.npz")
    state = {kk: torch.from_numpy(np.array(w[kk])).double() for kk in w.files}
    sp = frames.StreamsPredictor(model, ns, k=1, capacity=cap, max_detections=m_max)
    replay = sp.capture()
    sample = [0, 5, 123, 411, 799]
    lone = {s: frames.FramePredictor(model, k=1, capacity=cap, max_detections=m_max) for s in sample}
    sched = Schedule(pushes, [s % 7 for s in range(ns)])
    refs = [frames_np.StreamModel() for _ in range(ns)]
    worst_lone = worst_oracle = 0.0
    n_oracle = 0
    for t in range(60):
        tick = sched.tick(t)
        out = replay(tick, seed=t)
        out_np = _host(out)
        assert not np.any(out_np[3]), t
        _check_restatement(out_np, tick, refs, t)
        vp = out.v_pred
        for s in sample:
            if tick[s] is None:
                continue
            r = lone[s].push(*tick[s])
            worst_lone = max(worst_lone, float((r.v_pred - vp[s]).abs().max()))
        if t % 10 == 9:
            vp_np = vp.cpu().numpy()
            peds, obs = out_np[1], out_np[2]
            with torch.no_grad():
                for i in (int(np.argmax(peds)), 3 * t, 7 * t + 1):
                    c = int(peds[i])
                    if c == 0:
                        continue
                    rel = np.zeros((8, c, 2))
                    rel[1:] = obs[i, 1:, :c] - obs[i, :-1, :c]
                    rel = rel.astype(np.float32).astype(np.float64)
                    nodes, lap = O.seq_to_graph_np(np.transpose(rel, (1, 2, 0)))
                    x = torch.from_numpy(np.asarray(nodes, np.float64)).unsqueeze(0).permute(0, 3, 1, 2)
                    y = O.social_stgcnn_forward(state, x, torch.from_numpy(np.asarray(lap, np.float64)), False)
                    worst_oracle = max(worst_oracle, float(np.abs(y[0].numpy() - vp_np[i, :, :, :c]).max()))
                    n_oracle += 1
    print("streams %d: v_pred vs lone %.3g, vs fp64 oracle %.3g over %d scenes" % (ns, worst_lone, worst_oracle,
                                                                                    n_oracle))
    assert n_oracle >= 6
    assert worst_lone < 1e-5, worst_lone
    assert worst_oracle < 1e-4, worst_oracle


def test_entry_point_refuses_bad_arguments(dev):
    from social_stgcnn_amd._lib import lib
    L = lib()
    f = ctypes.c_void_p(64)          # never dereferenced: every case fails validation before any HIP call

    def push(ns=4, m_total=16, m_max=8, s=16, t=8, v=4, det=f, start=f, slot=f, out=f, block=0):
        return L.stg_track_push_streams(det, 3, f, 3, m_total, start, f, ns, m_max, slot, f, f, f, s, t, 1e4, v, out,
                                        f, f, None, block, None)
    cases = {"NS=0": dict(ns=0), "NS too large": dict(ns=4097), "M_total<0": dict(m_total=-1),
             "M_total too large": dict(m_total=(1 << 23) + 1), "M_max=0": dict(m_max=0),
             "M_max too large": dict(m_max=4096), "S=0": dict(s=0), "S too large": dict(s=4096), "T_obs=0": dict(t=0),
             "T_obs=33": dict(t=33), "V=0": dict(v=0), "block 128": dict(block=128), "null det_id": dict(det=None),
             "null det_start": dict(start=None), "null slot_id": dict(slot=None), "null obs_abs": dict(out=None)}
    for name, kw in cases.items():
        assert push(**kw) == -1, name
        assert b"stg_track_push_streams" in L.stg_last_error(), name
