"""Device-resident windowed dataset: the counterpart of the reference's TrajectoryDataset + DataLoader
(utils.py:88-193, train.py:167-177) with the windows living in HBM and batches gathered by index on the device.

    win = data.load_windows(dir)                 # host ingest (vectorised NumPy, bit-equal to the reference)
    ds = DeviceWindows(win, device)              # ONE upload: 160 bytes per pedestrian-window
    order = ds.shuffled_order(generator)         # device permutation of the windows (DataLoader(shuffle=True))
    batch = ds.gather(order[lo:hi])              # obs_rel / target / num_peds padded to ds.v_max, on the device

`EpochRunner` captures gather -> adj_build -> forward -> loss -> backward -> update as one hipGraph on static buffers
and replays it per group with the index buffer refreshed in place: a training epoch moves nothing over PCIe.  Its
validation epoch does the same with gather -> adj_build -> eval forward -> per-scene NLL -> weighted group total.
"""
import numpy as np
import torch

from . import graphs, ops
from ._lib import call, ptr, require_gpu


class DeviceWindows:
    def __init__(self, windows, device, obs_len=8):
        self.device = torch.device(device)
        self.n_windows = len(windows)
        self.t_all = int(windows.seq_rel.shape[2])
        self.t_obs = int(obs_len)
        self.t_pred = self.t_all - self.t_obs
        self.num_peds_host = np.asarray(windows.num_peds, dtype=np.int32)
        self.v_max = int(self.num_peds_host.max())
        start = np.concatenate([[0], np.cumsum(self.num_peds_host)]).astype(np.int32)
        self.rel_all = torch.from_numpy(np.ascontiguousarray(windows.seq_rel, dtype=np.float32)).to(self.device)
        self.win_start = torch.from_numpy(start).to(self.device)

    @classmethod
    def from_device(cls, rel_all, win_start, num_peds_host, obs_len):
        """A dataset over windows that are on the device already, without a copy: rel_all float32 (R,2,T_all) and
        win_start int32 (W+1,), contiguous device tensors (views are fine) in the layout above -- window w holds rows
        win_start[w] .. win_start[w+1]-1 --, and num_peds_host, the W row counts on the host (they size the batches'
        padding).  What frames.LiveWindows.snapshot() returns."""
        if not (torch.is_tensor(rel_all) and rel_all.dtype == torch.float32 and rel_all.dim() == 3
                and rel_all.shape[1] == 2 and rel_all.is_contiguous()):
            raise ValueError("from_device: rel_all (R,2,T_all) float32, contiguous, expected")
        if not (torch.is_tensor(win_start) and win_start.dtype == torch.int32 and win_start.dim() == 1
                and win_start.is_contiguous()):
            raise ValueError("from_device: win_start (W+1,) int32, contiguous, expected")
        peds = np.asarray(num_peds_host)
        if peds.ndim != 1 or peds.dtype.kind not in "iu" or len(peds) < 1 or len(peds) != win_start.numel() - 1:
            raise ValueError("from_device: num_peds_host must hold the W >= 1 integer row counts of win_start (W+1,)")
        if int(peds.min()) < 1 or int(peds.sum()) != rel_all.shape[0]:
            raise ValueError("from_device: num_peds_host must be >= 1 and sum to the %d rows of rel_all"
                             % rel_all.shape[0])
        t_all = int(rel_all.shape[2])
        if isinstance(obs_len, bool) or int(obs_len) != obs_len or not 1 <= int(obs_len) < t_all:
            raise ValueError("from_device: obs_len must be an integer in [1, T_all = %d), got %r" % (t_all, obs_len))
        if rel_all.device != win_start.device:
            raise ValueError("from_device: rel_all and win_start are on different devices")
        require_gpu(rel_all)
        self = cls.__new__(cls)
        self.device = rel_all.device
        self.n_windows = len(peds)
        self.t_all, self.t_obs = t_all, int(obs_len)
        self.t_pred = t_all - self.t_obs
        self.num_peds_host = peds.astype(np.int32)
        self.v_max = int(peds.max())
        self.rel_all, self.win_start = rel_all, win_start
        return self

    def __len__(self):
        return self.n_windows

    def shuffled_order(self, generator=None):
        """a device permutation of the window indices (int32)"""
        return torch.randperm(self.n_windows, device=self.device, generator=generator).to(torch.int32)

    def buffers(self, n, v_pad=None):
        v = int(v_pad or self.v_max)
        dev = self.device
        return (torch.empty((n, v, 2, self.t_obs), device=dev), torch.empty((n, self.t_pred, v, 2), device=dev),
                torch.empty(n, device=dev, dtype=torch.int32))

    def gather(self, index=None, n=None, v_pad=None, out=None):
        """windows `index` (int32 device tensor; None = the first n) -> (obs_rel (N,V,2,T_obs), target (N,T_pred,V,2),
        num_peds (N)) zero-padded to v_pad (default: the dataset's largest crowd).  One launch, no host sync."""
        if index is not None:
            require_gpu(index)
            if index.dtype != torch.int32 or not index.is_contiguous():
                raise TypeError("index must be a contiguous int32 device tensor")
            n = index.numel()
        obs_rel, target, peds = out if out is not None else self.buffers(n, v_pad)
        v = obs_rel.shape[1]
        call("stg_gather_windows", seq_rel_all=ptr(self.rel_all), win_start=ptr(self.win_start), index=ptr(index),
             n_windows=self.n_windows, N=int(n), V=int(v), T_obs=self.t_obs, T_pred=self.t_pred, obs_rel=ptr(obs_rel),
             target=ptr(target), num_peds=ptr(peds))
        return obs_rel, target, peds


class EpochRunner:
    """Reference-style training epochs (train.py:28-79: groups of `batch_size` scenes, the closing scene forwarded but
    not in the loss) over a DeviceWindows dataset, every group ONE replay of a captured hipGraph:
    gather (by device index) -> adj_build -> forward -> NLL -> backward -> clip/SGD.  The short group at the end of an
    epoch has a graph of its own (captured on leading slices of the same static buffers), so an epoch is graph replays and
    device-to-device index copies only."""

    def __init__(self, trainer, dataset, batch_size, v_pad=None):
        self.trainer, self.ds, self.bs = trainer, dataset, int(batch_size)
        dev = dataset.device
        self.index = torch.zeros(self.bs, device=dev, dtype=torch.int32)
        # pedestrian slots: the dataset's largest crowd rounded up to a multiple of 4 -- rows of the adjacency are then
        # 16-byte aligned and stg_adj_build / the aggregation kernel move them with 16-byte accesses
        v_pad = int(v_pad) if v_pad else (dataset.v_max + 3) & ~3
        self.obs_rel, self.target, self.peds = dataset.buffers(self.bs, v_pad)
        v = self.obs_rel.shape[1]
        self.nodes = torch.empty((self.bs, dataset.t_obs, v, 2), device=dev)
        self.adj = torch.empty((self.bs, dataset.t_obs, v, v), device=dev)
        self._replays = {}                 # group size -> (replay, index slice, loss weights)
        self._val_replays = {}             # group size -> (graph, group total, index slice, loss weights)
        self._dataset_order = None

    def _group(self, cnt):
        """the captured step of a group of `cnt` scenes (cnt <= batch_size): leading slices of the static buffers"""
        g = self._replays.get(cnt)
        if g is None:
            from .trainer import group_weights
            index = self.index[:cnt]
            obs_rel, target, peds = self.obs_rel[:cnt], self.target[:cnt], self.peds[:cnt]
            nodes, adj = self.nodes[:cnt], self.adj[:cnt]
            weights = group_weights(cnt, self.bs, self.ds.device)

            def pre():
                self.ds.gather(index, out=(obs_rel, target, peds))
                ops.adj_build(obs_rel, peds, out=(nodes, adj))
            replay = self.trainer.capture(nodes.permute(0, 3, 1, 2), adj, target, peds, weights, pre=pre)
            # (the graph reads `weights` at every replay: it must stay alive with the graph)
            g = self._replays[cnt] = (replay, index, weights)
        return g

    def train_epoch(self, order):
        """order: int32 device tensor, a permutation (or any list) of window indices.  Returns the epoch loss as
        train() reports it (sum of group losses / scenes seen), accumulated on the device."""
        from .trainer import group_bounds
        self.trainer.model.train()
        n_scenes = order.numel()
        total = torch.zeros((), device=self.ds.device)
        lo = 0
        for b in group_bounds(n_scenes, self.bs):
            cnt = b + 1 - lo
            if cnt not in self._replays:
                self.index[:cnt].copy_(order[lo:b + 1])         # (valid window indices while the group is captured)
            replay, index, _ = self._group(cnt)
            index.copy_(order[lo:b + 1])                        # device -> device
            total = total + replay()[0]
            lo = b + 1
        return total / n_scenes

    @torch.no_grad()
    def _val_group(self, cnt):
        """the captured validation pass of a group of `cnt` scenes: gather -> adj_build -> eval forward -> per-scene NLL
        -> sum_n w_n loss_n (stg_weighted_sum: one fixed summation order), on leading slices of the static buffers"""
        g = self._val_replays.get(cnt)
        if g is None:
            from .trainer import group_weights
            model = self.trainer.model
            index = self.index[:cnt]
            obs_rel, target, peds = self.obs_rel[:cnt], self.target[:cnt], self.peds[:cnt]
            nodes, adj = self.nodes[:cnt], self.adj[:cnt]
            weights = group_weights(cnt, self.bs, self.ds.device)

            def group_total():
                self.ds.gather(index, out=(obs_rel, target, peds))
                ops.adj_build(obs_rel, peds, out=(nodes, adj))
                y, _ = model(nodes.permute(0, 3, 1, 2), adj, peds)
                losses = ops.bivariate_nll(y.permute(0, 2, 3, 1), target, peds)
                return ops.weighted_sum(losses, weights)
            graph, total = graphs.warm_capture(group_total, 1)  # (warm-up: an eval pass changes nothing)
            # (the graph reads `weights` and the index slice at every replay: they live as long as the graph)
            g = self._val_replays[cnt] = (graph, total, index, weights)
        return g

    def val_epoch(self, order=None):
        """vald() (train.py:81-122) over the dataset: the model in eval mode, windows in dataset order (or `order`, an int32
        device tensor of window indices), groups of `batch_size` scenes whose closing scene is forwarded but not in the
        loss, every group ONE replay of a captured graph (one per group size).  Returns the epoch loss as vald() reports
        it (sum of group losses / scenes seen) as a 0-d device tensor; nothing in the epoch waits for the host."""
        from .trainer import group_bounds
        self.trainer.model.eval()
        if order is None:
            if self._dataset_order is None:
                self._dataset_order = torch.arange(self.ds.n_windows, device=self.ds.device, dtype=torch.int32)
            order = self._dataset_order
        n_scenes = order.numel()
        total = torch.zeros((), device=self.ds.device)
        lo = 0
        for b in group_bounds(n_scenes, self.bs):
            cnt = b + 1 - lo
            if cnt not in self._val_replays:
                self.index[:cnt].copy_(order[lo:b + 1])         # (valid window indices while the group is captured)
            graph, group_total, index, _ = self._val_group(cnt)
            index.copy_(order[lo:b + 1])                        # device -> device
            graph.replay()
            total = total + group_total
            lo = b + 1
        return total / n_scenes
