"""On-disk formats of the reference and the training loader, device-resident -- mirror of
``gnn_manip/utils/coffee_dataset.py`` (``read_metadata``, ``CoffeeDataset``) plus the batching the reference
gets from ``torch_geometric.data.DataLoader`` (examples/train_dyn.py:8,49-53).

MI355X layout: every simulation file is parsed once and kept as one ``[T, N, D]`` float32 tensor in HBM
(288 GB per GPU hold whole datasets); a sample is a window view of it, turned into a graph by the HIP
kernels of graph.py when it is requested.  The reference materialises every window on the host instead
(k-fold duplication, coffee_dataset.py:82-102).
"""
import ctypes as C
import json

import numpy as np
import torch

from ._lib import check, current_stream, lib, ptr
from .graph import GraphBoundedMultimaterial, GraphBoundedMultimaterialControl, _ws, make_feature_desc


def read_metadata(metadata_file):
    """coffee_dataset.py:18-43: (data_dim, time_steps, cartesian_idx, control_idx, material_id, bounds, stats)."""
    with open(metadata_file) as fp:
        metadata = json.load(fp)
    b = torch.tensor(metadata["bounds"])
    bounds = {"upper_bounds": b[:, 1], "lower_bounds": b[:, 0]}
    stats = {"velocity_mean": torch.tensor(metadata["vel_mean"]), "velocity_std": torch.tensor(metadata["vel_std"]),
             "acceleration_mean": torch.tensor(metadata["acc_mean"]), "acceleration_std": torch.tensor(metadata["acc_std"])}
    return (metadata["data_dim"], metadata["sequence_length"], metadata["cartesian_idx"], metadata["control_idx"],
            metadata["material_id"], bounds, stats)


def read_simulation(file, time_steps, data_dim):
    """One ``particles_%06d.csv`` (rows = time-major particles, no header) -> float64 [T, N, data_dim]."""
    import pandas as pd
    return np.array(pd.read_csv(file, header=None)).reshape(time_steps, -1, data_dim)


STATS_DOUBLES = 24   # GM_RECORDING_STATS_DOUBLES (include/gnn_manip_hip.h): 8 per axis


def _recordings(sims, who):
    """``sims`` (one tensor or a list) as a list of resident float32 [T, N, D] tensors on one HIP device."""
    sims = [sims] if torch.is_tensor(sims) else list(sims)
    if not sims or any((not torch.is_tensor(s)) or s.dtype != torch.float32 or s.dim() != 3 or not s.is_cuda for s in sims):
        raise RuntimeError(f"{who}: float32 [T, N, data_dim] tensors on the HIP device")
    if len({s.device for s in sims}) != 1 or len({int(s.shape[2]) for s in sims}) != 1:
        raise RuntimeError(f"{who}: the recordings share one device and one data_dim")
    return [s.contiguous() for s in sims]


def _contiguous_columns(cartesian_idx, who, want=None):
    idx = [int(c) for c in cartesian_idx]
    if not 1 <= len(idx) <= 3 or idx != list(range(idx[0], idx[0] + len(idx))) or (want is not None and len(idx) != want):
        raise ValueError(f"{who}: cartesian_idx={idx}: {'1 to 3' if want is None else want} consecutive columns")
    return idx


def chan_merge(a, b):
    """(count, mean, M2) of the union of two samples from theirs (Chan, Golub, LeVeque), in float64; means and M2 may be arrays."""
    (na, ma, Ma), (nb, mb, Mb) = a, b
    n = na + nb
    if n == 0:
        return a
    d = mb - ma
    return n, ma + d * (nb / n), Ma + Mb + d * d * (na * nb / n)


def recording_statistics(sims, cartesian_idx=(2, 3, 4), material_id=None, material=None):
    """The normalisation statistics of recordings that are resident already -- what simulation/generate_metadata.py:24-45 computes
    with numpy on the host: mean and population standard deviation (``np.std``, ddof = 0) of the velocities ``np.diff(p, axis=0)``
    and of the accelerations (``np.diff`` again) over all rows of all recordings.  One gm_recording_stats call per recording, ONE
    transfer at the end; the per-recording (count, mean, M2) records are merged on the host in float64 (``chan_merge``).

    ``material_id`` (a column) and ``material`` (a value), given together, count only the rows that carry that value in frame 0 --
    the sand-only statistics that go with ``Trainer(sand_only=True)``; left None, every row counts, as in the reference.

    Returns ``(stats, info)``: ``stats`` has the keys and dtypes of ``read_metadata``'s; ``info`` the float64 values
    (``velocity_mean``, ``velocity_std``, ``velocity_m2``, ``acceleration_*`` alike), ``velocity_count``, ``acceleration_count``,
    ``position_range`` [dim, 2] and the raw ``records`` [recordings, 3, 8].  ValueError names the recording whose result is not
    finite, and is raised when no row is counted at all."""
    who = "recording_statistics"
    sims = _recordings(sims, who)
    idx = _contiguous_columns(cartesian_idx, who)
    if (material_id is None) != (material is None):
        raise ValueError(f"{who}: material_id (the column) and material (the value) go together")
    mcol, mval = (-1, 0.0) if material_id is None else (int(material_id), float(material))
    L, dev, dim = lib(), sims[0].device, len(idx)
    with torch.cuda.device(dev):
        out = torch.empty((len(sims), STATS_DOUBLES), dtype=torch.float64, device=dev)
        need = max(L.gm_recording_stats_workspace_bytes(int(s.shape[0]), int(s.shape[1])) for s in sims)
        ws = _ws(max(need, 256), dev)
        for r, s in enumerate(sims):
            check(L.gm_recording_stats(ptr(s), int(s.shape[0]), int(s.shape[1]), int(s.shape[2]), idx[0], dim, mcol, mval,
                                       C.c_void_p(out.data_ptr() + r * STATS_DOUBLES * 8), ptr(ws), ws.numel(), current_stream(dev)))
        records = out.cpu().numpy().reshape(len(sims), 3, 8)[:, :dim]
    vel = acc = (0.0, np.zeros(dim), np.zeros(dim))
    lo, hi = np.full(dim, np.inf), np.full(dim, -np.inf)
    for r, rec in enumerate(records):
        if rec[0, 0] == 0:
            continue    # no row of this recording carries the material
        if not np.isfinite(rec).all():
            bad = [a for a in range(dim) if not np.isfinite(rec[a]).all()]
            raise ValueError(f"{who}: recording {r}: non-finite statistics on axis {bad} (a non-finite position in columns "
                             f"{[idx[a] for a in bad]})")
        vel = chan_merge(vel, (float(rec[0, 0]), rec[:, 1], rec[:, 2]))
        acc = chan_merge(acc, (float(rec[0, 3]), rec[:, 4], rec[:, 5]))
        lo, hi = np.minimum(lo, rec[:, 6]), np.maximum(hi, rec[:, 7])
    if vel[0] == 0:
        raise ValueError(f"{who}: no row counted: no row of any recording has column {mcol} == {mval} in frame 0")
    info = {"velocity_count": int(vel[0]), "velocity_mean": vel[1], "velocity_m2": vel[2], "velocity_std": np.sqrt(vel[2] / vel[0]),
            "acceleration_count": int(acc[0]), "acceleration_mean": acc[1], "acceleration_m2": acc[2],
            "acceleration_std": np.sqrt(acc[2] / acc[0]), "position_range": np.stack((lo, hi), axis=1), "records": records}
    stats = {k: torch.tensor([float(v) for v in info[k]]) for k in ("velocity_mean", "velocity_std", "acceleration_mean", "acceleration_std")}
    return stats, info


def write_metadata(path, sims, bounds, cartesian_idx=(2, 3, 4), control_idx=(5, 6, 7), material_id=1):
    """metadata.json of the reference (simulation/generate_metadata.py:33-49) from resident recordings: the statistics are
    ``recording_statistics(sims, cartesian_idx)`` -- every row, as the reference counts them.  ``bounds``: what ``read_metadata``
    returns (``lower_bounds`` / ``upper_bounds``) or [[lower, upper], ...] per axis.  ``read_metadata(path)`` reads it back.
    Returns the dictionary written."""
    sims = _recordings(sims, "write_metadata")
    _, info = recording_statistics(sims, cartesian_idx)
    if isinstance(bounds, dict):
        pairs = [[float(lo), float(hi)] for lo, hi in zip(bounds["lower_bounds"], bounds["upper_bounds"])]
    else:
        pairs = [[float(lo), float(hi)] for lo, hi in bounds]
    metadata = {"cartesian_idx": [int(c) for c in cartesian_idx], "control_idx": [int(c) for c in control_idx],
                "material_id": int(material_id), "bounds": pairs, "sequence_length": int(sims[0].shape[0]),
                "dim": len(list(cartesian_idx)), "data_dim": int(sims[0].shape[2]),
                "vel_mean": [float(v) for v in info["velocity_mean"]], "vel_std": [float(v) for v in info["velocity_std"]],
                "acc_mean": [float(v) for v in info["acceleration_mean"]], "acc_std": [float(v) for v in info["acceleration_std"]]}
    with open(path, "w") as fp:
        json.dump(metadata, fp)
    return metadata


def neighbour_census(sims, conn_r, max_neighbours=20, cartesian_idx=(2, 3, 4), frames=None):
    """How many rows of the recordings the radius graph truncates at ``conn_r`` / ``max_neighbours``.  For every chosen frame,
    gm_neighbour_census counts per node the nodes ``gm_radius_graph_build`` would list without a cap (the node itself included,
    as the build includes it); ``min(count, max_neighbours)`` is the out-degree the build gives the node.  ``frames``: None for
    every frame, or a ``range`` / list of frame numbers applied to each recording.  The summary is formed on the device and comes
    over in one transfer:

    ``max_count``, ``mean_count``, ``rows_over_cap`` (node-frames with count > max_neighbours), ``frames_over_cap`` (frames that
    hold one), ``fraction_over_cap`` (of the node-frames), ``rows``, ``frames`` and ``histogram`` -- ``np.bincount`` of the counts:
    its length minus one is the smallest cap that truncates nothing."""
    who = "neighbour_census"
    sims = _recordings(sims, who)
    idx = _contiguous_columns(cartesian_idx, who, want=3)
    cap = int(max_neighbours)
    if cap < 1:
        raise ValueError(f"{who}: max_neighbours={cap} < 1")
    L, dev = lib(), sims[0].device
    with torch.cuda.device(dev):
        n_max = max(int(s.shape[1]) for s in sims)
        ws = _ws(L.gm_neighbour_census_workspace_bytes(n_max), dev)
        hist = torch.zeros(n_max + 1, dtype=torch.int64, device=dev)      # a node sees at most the n nodes of its frame
        scalars = torch.zeros(3, dtype=torch.int64, device=dev)           # rows over the cap, frames over the cap, the largest count
        rows = n_frames = 0
        for r, s in enumerate(sims):
            t_all, n, d = (int(v) for v in s.shape)
            chosen = list(range(t_all)) if frames is None else [int(t) for t in frames]
            if any(not 0 <= t < t_all for t in chosen):
                raise IndexError(f"{who}: frames outside the {t_all} frames of recording {r}")
            if not chosen:
                continue
            counts = torch.empty((len(chosen), n), dtype=torch.int32, device=dev)
            for j, t in enumerate(chosen):
                check(L.gm_neighbour_census(C.c_void_p(s.data_ptr() + (t * n * d + idx[0]) * 4), d, n, float(conn_r),
                                            C.c_void_p(counts.data_ptr() + j * n * 4), ptr(ws), ws.numel(), current_stream(dev)))
            flat = counts.view(-1).long()
            hist.scatter_add_(0, flat, torch.ones_like(flat))
            over = counts > cap
            scalars += torch.stack((over.sum(), over.any(dim=1).sum(), torch.zeros((), dtype=torch.int64, device=dev)))
            scalars[2] = torch.maximum(scalars[2], flat.max())
            rows += len(chosen) * n
            n_frames += len(chosen)
        if rows == 0:
            raise ValueError(f"{who}: no frame chosen")
        host = torch.cat((scalars, hist)).cpu().numpy()
    over_rows, over_frames, max_count = (int(v) for v in host[:3])
    histogram = host[3:3 + max_count + 1].copy()
    return {"max_count": max_count, "mean_count": float((histogram * np.arange(max_count + 1)).sum()) / rows,
            "rows_over_cap": over_rows, "frames_over_cap": over_frames, "fraction_over_cap": over_rows / rows, "rows": rows,
            "frames": n_frames, "histogram": histogram}


class GraphData:
    """The fields of ``torch_geometric.data.Data`` that train_dyn.py:49-53 reads (x, edge_attr, edge_index, y)."""

    def __init__(self, x, edge_attr, edge_index, y=None):
        self.x, self.edge_attr, self.edge_index, self.y = x, edge_attr, edge_index, y

    def to(self, device):
        mv = lambda t: None if t is None else t.to(device)
        return GraphData(mv(self.x), mv(self.edge_attr), mv(self.edge_index), mv(self.y))

    @property
    def num_nodes(self):
        return int(self.x.shape[0])


def collate_graphs(items):
    """Batch of GraphData -> one GraphData, edge indices offset by the node counts before them (the
    torch_geometric batching rule; for equal-sized graphs the N*i rule of collate_utils.py:75-76)."""
    xs, es, idx, ys, off = [], [], [], [], 0
    for g in items:
        xs.append(g.x)
        es.append(g.edge_attr)
        idx.append(g.edge_index + off)
        ys.append(g.y)
        off += g.x.shape[0]
    y = torch.cat(ys) if ys and ys[0] is not None else None
    return GraphData(torch.cat(xs), torch.cat(es), torch.cat(idx, dim=1), y)


class _QueuedBatch:
    """Phase 1 of one batch, queued: ONE build in one workspace -- gm_train_batch_build where the samples have equal N,
    gm_train_batch_build_ragged where they do not -- the workspace's 16-byte record on its way into a pinned row and an event
    behind the copy: the _HeaderWatch pattern of epd_gnn.py.  ``finish`` waits for that event alone, reads the edge count and
    queues phase 2."""

    def __init__(self, dataset, indices, seed, first_stream, workspaces, pinned):
        """workspaces: a list this batch may grow (the build's uint8 tensor, reused where large enough); pinned: int32 [>= 1, 4]
        in pinned memory.  Both belong to the caller and stay untouched by it until ``finish`` has returned."""
        ds = self.ds = dataset
        L, dev = lib(), ds.device
        self.fd = ds._window_desc()
        f = 3 * (ds.k - 1) + 7 + (3 if ds.use_control else 0)
        # the quirk of the reference kept: the noise-free path builds its graph with the default 20 neighbours (graph.py)
        self.k_nb = 20 if ds.noise is None else int(ds.max_neighbours)
        noise_std = 0.0 if ds.noise is None else float(ds.noise)
        batch = self.batch = len(indices)
        ns = [int(ds.sims[ds.index[int(i)][0]].shape[1]) for i in indices]
        rows = sum(ns)
        # samples of equal N: the equal-sized entry points; a batch that mixes sizes: the ragged ones, with the sizes as a host array
        self.sizes = None if len(set(ns)) == 1 else (C.c_int64 * batch)(*ns)
        self.n, self.pinned = ns[0], pinned
        frames = (C.c_void_p * batch)()
        for b, i in enumerate(indices):
            sim, t = ds.index[int(i)]
            data = ds.sims[sim]
            assert data.is_contiguous() and data.dtype == torch.float32, "resident recordings are row-major float32"
            frames[b] = data.data_ptr() + t * data.shape[1] * data.shape[2] * 4
        with torch.cuda.device(dev):
            if self.sizes is None:
                need = L.gm_train_batch_workspace_bytes(C.byref(self.fd), batch, self.n, self.k_nb)
            else:
                need = L.gm_train_batch_ragged_workspace_bytes(C.byref(self.fd), rows, batch, self.k_nb)
            if not workspaces:
                workspaces.append(None)
            if workspaces[0] is None or workspaces[0].numel() < need:
                workspaces[0] = _ws(need, dev)
            ws = self.ws = workspaces[0]
            self.nodes = torch.empty((rows, f), dtype=torch.float32, device=dev)
            self.target = torch.empty((rows, 3), dtype=torch.float32, device=dev)
            stream = current_stream(dev)
            if self.sizes is None:
                check(L.gm_train_batch_build(frames, batch, self.n, ds.data_dim, C.byref(self.fd), self.k_nb, noise_std, int(seed),
                                             int(first_stream), None, ptr(self.nodes), ptr(self.target), None, ptr(ws), ws.numel(), stream))
            else:
                check(L.gm_train_batch_build_ragged(frames, self.sizes, batch, ds.data_dim, C.byref(self.fd), self.k_nb, noise_std,
                                                    int(seed), int(first_stream), None, ptr(self.nodes), ptr(self.target), None, ptr(ws),
                                                    ws.numel(), stream))
            pinned[0].copy_(ws[:16].view(torch.int32), non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record(torch.cuda.current_stream(dev))

    def finish(self):
        """The batch: waits for the record (not for the stream), then phase 2."""
        L, dev = lib(), self.ds.device
        self.event.synchronize()
        e = C.c_int64(0)
        check(L.gm_train_batch_status(C.c_void_p(self.pinned[0].data_ptr()), C.byref(e)))
        e = int(e.value)
        edge_index = torch.empty((2, e), dtype=torch.int64, device=dev)
        edge_attr = torch.empty((e, 4), dtype=torch.float32, device=dev)
        if self.sizes is None:
            check(L.gm_train_batch_edges(ptr(self.ws), self.batch, self.n, C.byref(self.fd), self.k_nb, e, ptr(edge_index),
                                         ptr(edge_attr), current_stream(dev)))
        else:
            check(L.gm_train_batch_edges_ragged(ptr(self.ws), self.sizes, self.batch, C.byref(self.fd), self.k_nb, e, ptr(edge_index),
                                                ptr(edge_attr), current_stream(dev)))
        return GraphData(self.nodes, edge_attr, edge_index, self.target)


def _pinned_records(rows):
    return torch.zeros((max(int(rows), 1), 4), dtype=torch.int32).pin_memory()


class CoffeeDataset(torch.utils.data.Dataset):
    """Mirror of coffee_dataset.py:46-133 (same constructor arguments); ``device`` must be a HIP device."""

    def __init__(self, root, k, conn_r, split='train', noise=None, device=torch.device('cuda:0'), transform=None,
                 use_control=False, max_neighbours=20):
        assert split in ['train', 'test']
        import pandas as pd
        self.dir, self.split = root, split
        simulation_data = np.array(pd.read_csv(f'{self.dir}{self.split}/sim_data.csv', header=None))
        self.files = [f'{self.dir}{self.split}/particles_{int(sim_id):06d}.csv' for (sim_id, *_) in simulation_data]
        self.metadata_file = f'{self.dir}metadata.json'
        self.k, self.conn_r, self.max_neighbours = k, conn_r, max_neighbours
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("CoffeeDataset: gnn_manip_amd builds graphs on the HIP device only")
        self.noise, self.use_control = noise, use_control
        (self.data_dim, self.time_steps, self.cartesian_idx, self.control_idx, self.material_id, self.bounds,
         self.stats) = read_metadata(self.metadata_file)
        self._load_data(self.files)
        self.graph_attr = self._get_graph_attr()

    @classmethod
    def from_recordings(cls, sims, k, conn_r, stats, bounds, cartesian_idx=(2, 3, 4), material_id=1, control_idx=(5, 6, 7), noise=None,
                        use_control=False, max_neighbours=20):
        """The dataset over recordings that are resident already: ``sims`` a list of float32 [T, N, data_dim] tensors on one HIP
        device (N may differ between them), the other arguments what metadata.json and the constructor give.  ``stats=None``
        computes the statistics from ``sims`` (``recording_statistics(sims, cartesian_idx)``: every row, as the reference's
        metadata script counts them)."""
        self = cls.__new__(cls)
        self.sims = [s.contiguous() for s in sims]
        if not self.sims or any(s.dtype != torch.float32 or s.dim() != 3 or not s.is_cuda for s in self.sims):
            raise RuntimeError("CoffeeDataset.from_recordings: float32 [T, N, data_dim] tensors on the HIP device")
        self.dir = self.split = self.metadata_file = None
        self.files = []
        self.k, self.conn_r, self.max_neighbours, self.device = k, conn_r, max_neighbours, self.sims[0].device
        self.noise, self.use_control = noise, use_control
        self.data_dim, self.time_steps = int(self.sims[0].shape[2]), int(self.sims[0].shape[0])
        self.cartesian_idx, self.control_idx, self.material_id = list(cartesian_idx), list(control_idx), int(material_id)
        self.bounds, self.stats = bounds, (recording_statistics(self.sims, self.cartesian_idx)[0] if stats is None else stats)
        self.index = [(s, t) for s, data in enumerate(self.sims) for t in range(data.shape[0] - k)]
        self.graph_attr = self._get_graph_attr()
        return self

    def _load_data(self, files):
        # one resident [T, N, D] tensor per simulation; samples index (simulation, first frame)
        self.sims, self.index = [], []
        for s, file in enumerate(files):
            data = read_simulation(file, self.time_steps, self.data_dim)
            # row-major whatever layout the parser left: the library reads a sample's frames through one pointer
            self.sims.append(torch.from_numpy(data).float().contiguous().to(self.device))
            self.index += [(s, t) for t in range(self.time_steps - self.k)]

    def __len__(self):
        return len(self.index)

    def sample(self, idx):
        """(obs_seq [k, N, D(+3)], next_pos [N, 3]) of sample idx, as coffee_dataset.py:82-102 stores them."""
        s, t = self.index[idx]
        data = self.sims[s]
        c0 = self.cartesian_idx[0]
        obs_seq = data[t:t + self.k]
        next_pos = data[t + self.k][:, c0:c0 + 3]
        if self.use_control:
            # control input = next position - position for rigid-body particles (material == 1), else 0
            ctr = next_pos.unsqueeze(0) - obs_seq[:, :, c0:c0 + 3]
            ctr = torch.where((obs_seq[:, :, self.material_id] != 1).unsqueeze(-1), torch.zeros_like(ctr), ctr)
            obs_seq = torch.cat((obs_seq, ctr), dim=-1)
        # independent tensors, like the reference's stored samples: an in-place rollout step on a sample must not touch
        # the resident simulation (the windows overlap)
        return obs_seq.clone().contiguous(), next_pos.clone().contiguous()

    def __getitem__(self, idx):
        obs_seq, next_pos = self.sample(idx)
        nodes, edge_attr, senders, receivers, tgt = self.graph_attr.process(obs_seq, next_pos)
        return GraphData(nodes, edge_attr, torch.stack((senders, receivers)).long(), tgt)

    def _window_desc(self):
        """gm_feature_desc of a sample's window: the recording's columns, and with use_control the three control columns behind."""
        return make_feature_desc(self.conn_r, self.stats, self.bounds, self.cartesian_idx, [self.material_id],
                                 self.control_idx if self.use_control else None, self.k, self.data_dim + (3 if self.use_control else 0))

    def batch(self, indices, seed=0, first_stream=0):
        """The collated batch of the samples ``indices`` -- what ``collate_graphs([self[i] for i in indices])`` returns -- built
        in the library (gm_train_batch_build / gm_train_batch_edges) with one wait for the edge counts.  Honours ``noise``,
        ``use_control`` and ``max_neighbours`` like ``__getitem__``.  The noise is the library's counter-based draw: sample j of
        the call draws from stream ``first_stream + j`` of ``seed``, whatever batch it rides in; ``graph_attr.generator`` plays
        no part."""
        indices = [int(i) for i in indices]
        if not indices:
            raise ValueError("CoffeeDataset.batch: no samples")
        return _QueuedBatch(self, indices, seed, first_stream, [], _pinned_records(len(indices))).finish()

    def rollout_sample(self, idx, steps, seed=0, stream=0):
        """(window [k, N, D(+3)], frames [steps, N, data_dim]) of sample idx for training on a rollout (``Trainer.step_rollout``):
        the window as ``batch([idx], seed, stream)`` builds it -- gm_train_batch_build at batch 1: control columns from the clean
        positions, the library's random-walk noise when the dataset has ``noise`` -- and the ``steps`` recorded frames behind it,
        a VIEW into the resident recording.  IndexError when the recording ends before them."""
        idx, steps = int(idx), int(steps)
        if not 0 <= idx < len(self.index):
            raise IndexError(f"CoffeeDataset.rollout_sample: sample {idx} outside the {len(self.index)} samples")
        s, t = self.index[idx]
        data = self.sims[s]
        if steps < 1 or t + self.k + steps > data.shape[0]:
            raise IndexError(f"CoffeeDataset.rollout_sample: frames {t + self.k} .. {t + self.k + steps - 1} of a recording of "
                             f"{int(data.shape[0])} frames")
        L, dev, fd, n = lib(), self.device, self._window_desc(), int(data.shape[1])
        k_nb = 20 if self.noise is None else int(self.max_neighbours)      # _QueuedBatch's: the graph is built and not used
        first = (C.c_void_p * 1)(data.data_ptr() + t * n * int(data.shape[2]) * 4)
        with torch.cuda.device(dev):
            ws = _ws(L.gm_train_batch_workspace_bytes(C.byref(fd), 1, n, k_nb), dev)
            nodes = torch.empty((n, 3 * (self.k - 1) + 7 + (3 if self.use_control else 0)), dtype=torch.float32, device=dev)
            target = torch.empty((n, 3), dtype=torch.float32, device=dev)
            window = torch.empty((self.k, n, fd.data_dim), dtype=torch.float32, device=dev)
            check(L.gm_train_batch_build(first, 1, n, self.data_dim, C.byref(fd), k_nb, 0.0 if self.noise is None else float(self.noise),
                                         int(seed), int(stream), None, ptr(nodes), ptr(target), ptr(window), ptr(ws), ws.numel(),
                                         current_stream(dev)))
        return window, data[t + self.k:t + self.k + steps]

    def _get_graph_attr(self):
        if self.use_control:
            return GraphBoundedMultimaterialControl(conn_r=self.conn_r, stats=self.stats, cartesian_idx=self.cartesian_idx,
                                                    material_idx=[self.material_id], control_idx=self.control_idx,
                                                    bounds=self.bounds, noise=self.noise, max_neighbours=self.max_neighbours)
        return GraphBoundedMultimaterial(conn_r=self.conn_r, stats=self.stats, cartesian_idx=self.cartesian_idx,
                                         material_idx=[self.material_id], bounds=self.bounds, noise=self.noise,
                                         max_neighbours=self.max_neighbours)


class CoffeeTestDataset(CoffeeDataset):
    """Mirror of coffee_dataset.py:136-215: ONE simulation (``sim_id``) of a split; items are the raw
    ``(obs_seq [k, N, D(+3)], next_pos [N, 3])`` pairs the rollout / planner start from (rollout_utils.py:110-130,
    optimise_traj.py:253-259)."""

    def __init__(self, directory, k, conn_r, split='train', noise=None, max_neighbours=20, device=torch.device('cuda:0'),
                 use_control=False, sim_id=1):
        self.dir, self.split = directory, split
        self.files = [f'{self.dir}{self.split}/particles_{sim_id:06d}.csv']
        self.metadata_file = f'{self.dir}metadata.json'
        self.k, self.conn_r, self.max_neighbours = k, conn_r, max_neighbours
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("CoffeeTestDataset: gnn_manip_amd builds graphs on the HIP device only")
        self.noise, self.use_control = noise, use_control
        (self.data_dim, self.time_steps, self.cartesian_idx, self.control_idx, self.material_id, self.bounds,
         self.stats) = read_metadata(self.metadata_file)
        self._load_data(self.files)
        self.graph_attr = self._get_graph_attr()

    def __getitem__(self, index):
        return self.sample(index)


def owned_positions(n_items, shard):
    """The positions in 0 .. n_items - 1 that ``shard`` = (rank, world, group) owns: of every `group` consecutive positions (the
    last group may be shorter) the contiguous block ``planner.shard_range(len(group), world, rank)``.  None owns everything.  Over
    the ranks of a world every position is owned exactly once; a group shorter than the world leaves the last ranks empty."""
    if shard is None:
        return list(range(n_items))
    from .planner import shard_range
    rank, world, group = shard
    owned = []
    for first in range(0, n_items, group):
        lo, hi = shard_range(min(group, n_items - first), world, rank)
        owned += range(first + lo, first + hi)
    return owned


class GraphLoader:
    """What train_dyn.py gets from ``torch_geometric.data.DataLoader(dataset, batch_size, shuffle)``: an iterable of
    collated batches.  Everything stays on the dataset's device.

    ``fused=True`` builds the batches in the library (``CoffeeDataset.batch``'s two phases) instead of sample by sample in torch
    calls.  The noise is then the library's counter-based draw, not torch's: its seed is ``seed`` (or one drawn from the loader's
    ``rng`` when None), and sample i of the run -- counted over all epochs of this loader object, an epoch begun counting in full
    -- draws from stream i, so epochs differ and a run with a given seed repeats.  ``graph_attr.generator`` plays no part in the
    fused path.  ``prefetch=1`` queues the first phase of the next batch, in a second workspace on the same stream, before a
    batch is handed out: when the next batch is asked for, its edge count has long arrived (it was computed before the
    caller's training step began), nothing waits and the stream is never synchronised.  ``prefetch=0`` waits for its own build.
    A batch whose samples differ in N (recordings of different sizes) is one ragged build, like a batch of equal sizes one
    equal-sized build.  A batch larger than 64 (GM_TRAIN_BATCH_MAX) is refused by the library.

    ``shard=(rank, world, group)``: one of ``world`` data-parallel loaders over the same dataset, seed and shuffle.  Of every
    ``group`` consecutive batches (a trainer's global mini-batch; the last group may be shorter) it yields only the contiguous block
    ``planner.shard_range(len(group), world, rank)``; ``len()`` counts those, ``batches_in_all`` all of them.  A batch keeps the
    order and the noise streams of its GLOBAL position, so the noise a sample sees does not depend on ``world``; the prefetch runs
    over the owned batches."""

    def __init__(self, dataset, batch_size=2, shuffle=False, seed=None, fused=False, prefetch=1, shard=None):
        self.dataset, self.batch_size, self.shuffle = dataset, batch_size, shuffle
        self.shard = None
        if shard is not None:
            rank, world, group = (int(v) for v in shard)
            if not (0 <= rank < world and group >= 1):
                raise ValueError(f"GraphLoader: shard=(rank, world, group)={tuple(shard)}: need 0 <= rank < world and group >= 1")
            self.shard = (rank, world, group)
        self.rng = np.random.default_rng(seed)
        self.fused, self.prefetch = bool(fused), int(prefetch)
        if self.prefetch not in (0, 1):
            raise ValueError("GraphLoader: prefetch is 0 or 1")
        if self.fused:
            self.noise_seed = int(seed) if seed is not None else int(self.rng.integers(0, 2 ** 63))
            self._samples_begun = 0                      # samples of the epochs begun so far: the next epoch's first stream
            self._workspaces = ([], [])                  # batch i builds in set i % 2
            self._pinned = _pinned_records(2 * int(batch_size)).view(2, -1, 4)

    @property
    def batches_in_all(self):
        """The batches of an epoch over all shards (``len()`` of the loader without ``shard``)."""
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def owned_batches(self):
        """The positions, among an epoch's ``batches_in_all`` batches, of those this loader yields: all of them without ``shard``."""
        return owned_positions(self.batches_in_all, self.shard)

    def __len__(self):
        return self.batches_in_all if self.shard is None else len(self.owned_batches())

    def __iter__(self):
        order = self.rng.permutation(len(self.dataset)) if self.shuffle else np.arange(len(self.dataset))
        if self.fused:
            yield from self._iter_fused(order)
            return
        for j in self.owned_batches():
            b = j * self.batch_size
            yield collate_graphs([self.dataset[int(i)] for i in order[b:b + self.batch_size]])

    def _iter_fused(self, order):
        base = self._samples_begun
        self._samples_begun += len(order)
        starts = [j * self.batch_size for j in self.owned_batches()]

        def queue(j):
            b = starts[j]
            return _QueuedBatch(self.dataset, [int(i) for i in order[b:b + self.batch_size]], self.noise_seed, base + b,
                                self._workspaces[j % 2], self._pinned[j % 2])

        queued = None
        for j in range(len(starts)):
            batch = (queued or queue(j)).finish()
            # phase 1 of the next batch goes in front of whatever the caller queues for this one, in the other workspaces
            queued = queue(j + 1) if self.prefetch and j + 1 < len(starts) else None
            yield batch
