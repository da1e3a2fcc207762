"""numpy restatement of the time-indexed scoring rule (csrc/score_time.hip), push by push for ONE
stream, beside tests/score_np.py (the push-indexed rule, whose values these are) and tests/frames_time_np.py (the timed
push, whose track samples are the truth here).  A test helper and the authority on the rule, not the product path.

    TimedScoreModel(p, v, k, step, max_dt, pending, thr, decimals)   the rule in float64 on the float32 inputs
    TimedScoreModel(..., dtype=np.float32)      the rule as the kernel evaluates it: every value in float32 in the
                                                order the header states, log(det) the correctly rounded float32 logarithm
    TimedScoreModel(..., truth32=False)         the truth kept in float64 (the reference's own arithmetic)

push(tracks, t_now, pred, refused=False) runs behind one timed push: `tracks` is the track state AFTER that push, a dict
id -> [(t, x, y)] in ascending t as frames_time_np.StreamModelTimed.tracks holds it (rounded positions, the newest
`history` samples), t_now the push's time, pred a score_np.Prediction (None: the stream is not pushed); refused=True is a
push the track rule refused (TIME_ORDER).  It returns {push_totals (P,5+Q), push_traj (5)}: what the push added.

    rows[r]       the record ring (pending rows): None (empty) or a dict with t, status ("pending" / "retired"), ids,
                  num_peds, mean, cov, samples, acc, acc_mean, steps, the tables matched / err / d2 / nll / best (P,V)
                  and, once retired, traj_steps / traj_ade / traj_fde / traj_ade_mean / traj_fde_mean (V)
    accepted, evictions, totals (P,5+Q), traj_totals (5)    float64 sums in (row, pedestrian, horizon) order"""
import numpy as np

from frames_fill_np import round_pos
from score_np import LOG_2PI, cumulative_cov

TABLES = ("matched", "err", "d2", "nll", "best")
TRAJ = ("traj_steps", "traj_ade", "traj_fde", "traj_ade_mean", "traj_fde_mean")


def truth_at(samples, tau, max_dt, decimals):
    """The rule's truth at the instant tau from a track's samples [(t, x, y)] (ascending t, the newest last), as seen by
    the push that recorded the newest: ("hit", (2,) float64), ("wide", None) -- tau lies inside a bracket wider than
    max_dt and stays unmatched for good -- or (None, None): not this push."""
    tb, xb, yb = samples[-1]
    if tau == tb:
        return "hit", np.array([xb, yb], np.float64)
    if len(samples) < 2:
        return None, None
    ta, xa, ya = samples[-2]
    if not ta < tau < tb:
        return None, None
    if tb - ta > max_dt:
        return "wide", None
    pa, pb = np.array([xa, ya], np.float64), np.array([xb, yb], np.float64)
    return "hit", round_pos(pa + (pb - pa) * (float(tau - ta) / float(tb - ta)), decimals)


class TimedScoreModel:
    def __init__(self, p, v, k, step, max_dt, pending, thr=(), decimals=4, dtype=np.float64, truth32=True):
        self.p, self.v, self.k, self.step, self.max_dt, self.rp = p, v, k, int(step), int(max_dt), int(pending)
        self.decimals, self.f, self.truth32 = decimals, dtype, truth32
        self.thr = np.asarray(thr, np.float32).astype(dtype)      # the kernel compares float32 d2 with float32 thresholds
        assert self.step >= 1 and self.max_dt >= 1 and 1 <= self.rp <= 1024
        self.reset()

    def reset(self):
        self.rows = [None] * self.rp
        self.accepted = self.evictions = 0
        self.totals = np.zeros((self.p, 5 + len(self.thr)))
        self.traj_totals = np.zeros(5)

    def _dist(self, pos, t):
        f = self.f
        dx, dy = f(f(pos[0]) - f(t[0])), f(f(pos[1]) - f(t[1]))
        return f(np.sqrt(f(f(dx * dx) + f(dy * dy))))

    def _score(self, rec, h, v, t, add):
        """score_np.ScoreModel.push's values of one (record, horizon, pedestrian) against the truth t."""
        f, k = self.f, self.k
        mu = rec["mean"][h - 1, v]
        dx, dy = f(f(mu[0]) - f(t[0])), f(f(mu[1]) - f(t[1]))
        err = f(np.sqrt(f(f(dx * dx) + f(dy * dy))))
        cxx, cxy, cyy = (f(x) for x in rec["cov"][h - 1, v])
        det = max(f(f(cxx * cyy) - f(cxy * cxy)), f(f(cxx * cyy) * f(2.0 ** -15)))
        num = f(f(f(cyy * f(dx * dx)) - f(f(f(f(2) * cxy) * dx) * dy)) + f(cxx * f(dy * dy)))
        d2 = f(num / det)
        nll = f(f(f(f(0.5) * d2) + f(f(0.5) * f(np.log(np.float64(det))))) + f(LOG_2PI))
        best = f(0)
        if k:
            e = [self._dist(rec["samples"][kk, h - 1, v], t) for kk in range(k)]
            best = min(e)
            for kk in range(k):
                rec["acc"][kk, v] = f(rec["acc"][kk, v] + e[kk])
        rec["acc_mean"][v] = f(rec["acc_mean"][v] + err)
        rec["steps"][v] += 1
        rec["matched"][h - 1, v] = 1
        rec["err"][h - 1, v], rec["d2"][h - 1, v], rec["nll"][h - 1, v], rec["best"][h - 1, v] = err, d2, nll, best
        row = add[h - 1]
        row[0] += 1
        row[1:5] += (float(err), float(d2), float(nll), float(best))
        row[5:] += d2 <= self.thr

    def push(self, tracks, t_now, pred, refused=False):
        p, f, k = self.p, self.f, self.k
        add, add_traj = np.zeros_like(self.totals), np.zeros(5)
        out = dict(push_totals=add, push_traj=add_traj)
        if pred is None or refused:
            return out
        t_now = int(t_now)
        fresh = {i: s for i, s in tracks.items() if s and s[-1][0] == t_now}
        for rec in self.rows:
            if rec is None or rec["status"] != "pending":
                continue
            for v in range(rec["num_peds"]):
                smp = fresh.get(int(rec["ids"][v]))
                if smp is None:
                    continue
                for h in range(1, p + 1):
                    what, t = truth_at(smp, rec["t"] + h * self.step, self.max_dt, self.decimals)
                    if what == "hit":
                        self._score(rec, h, v, t.astype(np.float32) if self.truth32 else t, add)
            if t_now >= rec["t"] + p * self.step:
                rec["status"] = "retired"
                for v in range(rec["num_peds"]):
                    st = int(rec["steps"][v])
                    ade = f(rec["acc"][:, v].min() / f(st)) if st and k else f(0)
                    adem = f(rec["acc_mean"][v] / f(st)) if st else f(0)
                    fde, fdem = rec["best"][p - 1, v], rec["err"][p - 1, v]
                    rec["traj_steps"][v] = st
                    rec["traj_ade"][v], rec["traj_fde"][v], rec["traj_ade_mean"][v], rec["traj_fde_mean"][v] = \
                        ade, fde, adem, fdem
                    if st == p:
                        add_traj += (1.0, float(ade), float(fde), float(adem), float(fdem))
        self.totals += add
        self.traj_totals += add_traj
        # this push's record, last
        head = self.accepted % self.rp
        if self.rows[head] is not None and self.rows[head]["status"] == "pending":
            assert not (self.rows[head]["steps"] == p).any()        # its last instant has not arrived
            self.evictions += 1
        c = max(0, min(self.v, pred.num_peds))
        ids = np.full(self.v, -1, np.int64)
        ids[:c] = pred.ids[:c]
        cov = cumulative_cov(pred.v_pred, f)
        cov[:, c:] = 0
        rec = dict(t=t_now, status="pending", ids=ids, num_peds=c, mean=pred.mean.copy(), cov=cov,
                   samples=None if not k else pred.samples.copy(), acc=np.zeros((k, self.v), f),
                   acc_mean=np.zeros(self.v, f), steps=np.zeros(self.v, np.int64),
                   matched=np.zeros((p, self.v), np.int32), traj_steps=np.zeros(self.v, np.int32))
        rec.update({n: np.zeros((p, self.v), f) for n in TABLES[1:]})
        rec.update({n: np.zeros(self.v, f) for n in TRAJ[1:]})
        self.rows[head] = rec
        self.accepted += 1
        return out
