"""Calibration of the predicted Gaussians: one positive factor g_t on the covariance of every predicted
step t, fitted on held-out windows on the device (`stg_calib_fit`) and applied as a shift of 0.5 log g_t on the two
log-sigma channels of the model output (`stg_calib_apply`), in front of every consumer of V_pred.

    Calibration        g, mode, level; .shift; .save(path) / Calibration.load(path) (an .npz of g, mode, level)
    fit_calibration    the model over data.SceneWindows, batched as predict.sample_test, then ONE fit on the whole set

A Calibration goes to predict.Predictor, frames.FramePredictor, frames.StreamsPredictor, predict.sample_test,
predict.distribution_test and trainer.evaluate_dist_device as `calibration=`.
"""
import numpy as np
import torch

from . import data, ops
from .predict import Predictor


class Calibration:
    """The fitted factors g (P,) float32 on the covariances of the predicted steps, with the mode ("moment" or
    "coverage") and the level they were fitted at."""

    def __init__(self, g, mode="coverage", level=0.9):
        g = np.array(g.detach().cpu().numpy() if torch.is_tensor(g) else g, dtype=np.float32).reshape(-1)
        if mode not in ops.CALIB_MODES:
            raise ValueError("Calibration: mode must be one of %s, got %r" % (sorted(ops.CALIB_MODES), mode))
        self.g, self.mode, self.level = g, str(mode), float(np.float32(level))
        if not 0.0 < self.level < 1.0:
            raise ValueError("Calibration: level must lie in (0, 1), got %r" % (level,))
        self.shift = ops.calib_shift(g)                      # float32(0.5 log(float64 g)); refuses g <= 0

    def save(self, path):
        """Write an .npz of g, mode, level."""
        with open(path, "wb") as fp:
            np.savez(fp, g=self.g, mode=np.array(self.mode), level=np.array(self.level, dtype=np.float32))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(z["g"], str(z["mode"]), float(z["level"]))

    def __repr__(self):
        return "Calibration(g=%s, mode=%r, level=%s)" % (np.array2string(self.g, precision=4), self.mode, self.level)


@torch.no_grad()
def fit_calibration(model, windows, mode="coverage", level=0.9, batch_size=64):
    """Fit a Calibration of `model` on data.SceneWindows: predict.sample_test's batching without samples (k = 0), every
    batch's v_pred, mean, truth (sample_test's `trgt`) and num_peds packed into one device buffer padded to the set's
    largest V, then ONE ops.calib_fit: the fit is sequential over the horizons and needs the whole set.  Returns
    (Calibration, ops.CalibFit); the CalibFit's flags tell whether the search ran into a clamp."""
    pred = Predictor(model, 0)
    dev = next(model.parameters()).device
    t_obs, p = model.seq_len, model.pred_seq_len
    n_all, v_all = len(windows), int(windows.num_peds.max())
    f32 = dict(device=dev, dtype=torch.float32)
    v_pred = torch.zeros((n_all, 5, p, v_all), **f32)
    mean, truth = torch.zeros((n_all, p, v_all, 2), **f32), torch.zeros((n_all, p, v_all, 2), **f32)
    peds = torch.from_numpy(windows.num_peds.astype(np.int32)).to(dev)
    for lo in range(0, n_all, batch_size):
        idx = np.arange(lo, min(n_all, lo + batch_size))
        _, pred_rel, obs_abs, _, counts = data.pad_batch(windows, idx, obs_len=t_obs)
        v = obs_abs.shape[2]
        obs64 = np.zeros(obs_abs.shape)                    # the dataset's float64 positions (see observed_inputs)
        for j, i in enumerate(idx):
            s0, e0 = windows.seq_start_end[i]
            obs64[j, :, :e0 - s0] = np.transpose(windows.seq[s0:e0, :, :t_obs], (2, 0, 1))
        r = pred.predict(torch.from_numpy(obs64).to(dev), torch.from_numpy(counts).to(dev))
        xl = obs_abs[:, -1].astype(np.float64)             # sample_test's trgt
        trgt = (np.cumsum(pred_rel, axis=1, dtype=np.float32) + xl[:, None]).astype(np.float32)
        hi = lo + len(idx)
        v_pred[lo:hi, :, :, :v] = r.v_pred
        mean[lo:hi, :, :v] = r.mean
        truth[lo:hi, :, :v] = torch.from_numpy(trgt).to(dev)
    fit = ops.calib_fit(v_pred, mean, truth, peds, mode, level)
    return Calibration(fit.g, mode, level), fit
