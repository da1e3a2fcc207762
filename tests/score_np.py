"""numpy restatement of the scoring rule (csrc/score.hip), push by push for ONE stream, in the style of
frames_np.StreamModel.  A test helper, not the product path.

    ScoreModel(p, v, k, thr, m_max, decimals)   the rule in float64: every operation of the rule in float64 on the
                                                float32 inputs, the truth converted to float32 as the rule says
    ScoreModel(..., dtype=np.float32)           the rule as the kernel evaluates it: every operation in float32 in the
                                                order the header states (numpy does not fuse multiply-adds), log(det)
                                                the correctly rounded float32 logarithm
    ScoreModel(..., truth32=False)              the truth kept in float64 (the reference's own arithmetic: its ADE / FDE
                                                take float64 targets -- tests/test_score_cpu.py pins the rule to it)

push(det_ids, det_xy, pred) scores the pending records against the detections, retires the oldest, enqueues `pred`
(None: the stream is not pushed -- nothing moves, the outputs are empty) and returns the outputs as a dict of arrays
(the float fields in `dtype`);
`totals` (P,5+Q) and `traj_totals` (5) are float64 sums in push order."""
import numpy as np

FIELDS = ("rec_ids", "matched", "err", "d2", "nll", "best", "traj_steps", "traj_ade", "traj_fde", "traj_ade_mean",
          "traj_fde_mean")
LOG_2PI = 1.8378770664093453


def cumulative_cov(v_pred, dtype=np.float64):
    """v_pred (5,P,V) float32 -> C (P,V,3): the running sum over t of [sx^2, rho sx sy, sy^2] in `dtype`."""
    f = dtype
    sx, sy, rho = np.exp(v_pred[2].astype(f)), np.exp(v_pred[3].astype(f)), np.tanh(v_pred[4].astype(f))
    terms = np.stack([sx * sx, rho * sx * sy, sy * sy], axis=-1).astype(f)
    out = np.zeros_like(terms)
    c = np.zeros(terms.shape[1:], f)
    for t in range(terms.shape[0]):
        c = (c + terms[t]).astype(f)
        out[t] = c
    return out


class Prediction:
    """What one push enqueues: ids (V,) int64, num_peds, mean (P,V,2), v_pred (5,P,V), samples (K,P,V,2) or None."""

    def __init__(self, ids, num_peds, mean, v_pred, samples=None):
        self.ids, self.num_peds = np.asarray(ids, np.int64), int(num_peds)
        self.mean, self.v_pred = np.asarray(mean, np.float32), np.asarray(v_pred, np.float32)
        self.samples = None if samples is None else np.asarray(samples, np.float32)


class ScoreModel:
    def __init__(self, p, v, k, thr=(), m_max=1024, decimals=4, dtype=np.float64, truth32=True):
        self.p, self.v, self.k, self.m_max, self.decimals = p, v, k, m_max, decimals
        self.f = dtype
        self.truth32 = truth32
        # the kernel compares float32 d2 with the float32 thresholds
        self.thr = np.asarray(thr, np.float32).astype(dtype)
        self.records = []               # the pending records, oldest first, at most p of them
        self.totals = np.zeros((p, 5 + len(self.thr)))
        self.traj_totals = np.zeros(5)

    def empty(self):
        p, v = self.p, self.v
        out = {n: np.zeros((p, v), self.f) for n in ("err", "d2", "nll", "best")}
        out.update({n: np.zeros(v, self.f) for n in ("traj_ade", "traj_fde", "traj_ade_mean", "traj_fde_mean")})
        out["rec_ids"] = np.full((p, v), -1, np.int64)
        out["matched"] = np.zeros((p, v), np.int32)
        out["traj_steps"] = np.zeros(v, np.int32)
        return out

    def _truth(self, det_ids, det_xy):
        det_ids = np.asarray(det_ids, np.int64).reshape(-1)[:self.m_max]
        det_xy = np.asarray(det_xy, np.float64).reshape(-1, 2)[:self.m_max]
        truth = {}
        for i, q in zip(det_ids.tolist(), det_xy):
            if i not in truth:          # a repeated id: the first detection wins
                q = q if self.decimals is None else np.around(q, self.decimals)
                truth[i] = q.astype(np.float32) if self.truth32 else q
        return truth

    def _dist(self, pos, t):
        f = self.f
        dx, dy = f(f(pos[0]) - f(t[0])), f(f(pos[1]) - f(t[1]))
        return f(np.sqrt(f(f(dx * dx) + f(dy * dy))))

    def push(self, det_ids, det_xy, pred):
        out = self.empty()
        if pred is None:
            return out
        f, p, k = self.f, self.p, self.k
        truth = self._truth(det_ids, det_xy)
        n = len(self.records)
        for h in range(1, min(n, p) + 1):
            rec = self.records[n - h]
            for v in range(rec["num_peds"]):
                i = int(rec["ids"][v])
                if i not in truth:
                    continue
                t = truth[i]
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
                out["rec_ids"][h - 1, v], out["matched"][h - 1, v] = i, 1
                out["err"][h - 1, v], out["d2"][h - 1, v], out["nll"][h - 1, v] = err, d2, nll
                out["best"][h - 1, v] = best
                row = self.totals[h - 1]
                row[0] += 1
                row[1:5] += (float(err), float(d2), float(nll), float(best))
                row[5:] += d2 <= self.thr
        if n == p:                       # the record that turns p pushes old
            rec = self.records.pop(0)
            for v in range(rec["num_peds"]):
                st = int(rec["steps"][v])
                out["traj_steps"][v] = st
                ade = f(rec["acc"][:, v].min() / f(st)) if st and k else f(0)
                adem = f(rec["acc_mean"][v] / f(st)) if st else f(0)
                fde, fdem = out["best"][p - 1, v], out["err"][p - 1, v]
                rec_out = (ade, fde, adem, fdem)
                for name, x in zip(("traj_ade", "traj_fde", "traj_ade_mean", "traj_fde_mean"), rec_out):
                    out[name][v] = x
                if st == p:
                    self.traj_totals += (1.0,) + tuple(float(x) for x in rec_out)
        c = max(0, min(self.v, pred.num_peds))
        ids = np.full(self.v, -1, np.int64)
        ids[:c] = pred.ids[:c]
        cov = cumulative_cov(pred.v_pred, f)
        cov[:, c:] = 0
        rec = dict(ids=ids, num_peds=c, mean=pred.mean.copy(), cov=cov,
                   samples=None if not k else pred.samples.copy(), acc=np.zeros((k, self.v), f),
                   acc_mean=np.zeros(self.v, f), steps=np.zeros(self.v, np.int64))
        self.records.append(rec)
        return out

    def reset(self):
        self.records = []
        self.totals[:] = 0
        self.traj_totals[:] = 0
