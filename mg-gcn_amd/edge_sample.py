"""Per-epoch edge sampling drawn on the device (opt-in; the reference trains on every edge): gat(fanout=, edge_keep=) and
sage(aggr="max", fanout=, edge_keep=) train every epoch on a fresh sample of the edges -- DropEdge (Rong et al. 2020; PyG's
dropout_edge) with ``keep``, an expected GraphSAGE fan-out with ``fanout``, or both.

The sample.  For the forward matrix F (rows are destinations, entries are sources; A.transpose()) destination i has the keep
probability q_i = keep * min(1, fanout / deg_i), deg_i the entry count of row i (duplicates counted), and the host computes,
once per setting and in float64, t_i = min(floor(q_i * 2^32), 2^32 - 1).  Entry (i, j) -- global vertex numbers -- is kept in
training forward e iff

    i == j   (a self-loop is always kept: no destination loses itself), or
    t_i == 0xFFFFFFFF, or
    word 0 of Philox4x32-10(counter = (j, i, 0xC0000000, e), key = (seed & 0xFFFFFFFF, seed >> 32)) < t_i.

The third counter word keeps the draw apart from feature dropout (row >> 32), attention dropout (0x80000000 | k >> 2) and
the label mask (first word 0xFFFFFFFF) under one seed.  Duplicate entries share one bit.  ``fanout`` is an EXPECTED fan-out,
not an exact one: "k of deg" cannot be decided from the transposed side without walking the destination's whole row, and
the bit must be a function of the pair alone for F and F^T to be sampled independently ("row = destination" on F, "column =
destination" on F^T) and still be each other's transpose, entry for entry.  Each keeps the entry order of the matrix it was
drawn from (stable compaction), so every downstream kernel's summation order is a function of the sample alone.

The kernels (csrc/edge_sample.hip: ops.edge_sample_count / _scan / _compact) count the kept entries per row, scan the counts
into an indptr and draw the same bits again to write the kept columns; nothing of size nnz is stored between the passes,
the host never reads a sampled size, and no synchronisation is added.  Values are not carried: every consumer -- the
attention kernels and the max aggregator -- reads the pattern only.
"""
from __future__ import annotations

import numbers

import numpy as np

from . import ops
from .matrix import context, csr_matrix

def check_sampling(fanout, keep):
    """option checking of fanout= / keep= (edge_keep=), before any device work: (fanout or None, keep); ValueError naming the
    argument for a keep outside (0, 1] and a fanout that is neither None nor an integer >= 1"""
    if not isinstance(keep, numbers.Real) or isinstance(keep, bool) or not 0.0 < keep <= 1.0:      # no NaN either
        raise ValueError(f"edge sampling: keep must be a number in (0, 1], got {keep!r}")
    if fanout is not None and (not isinstance(fanout, numbers.Integral) or isinstance(fanout, bool) or fanout < 1):
        raise ValueError(f"edge sampling: fanout must be None or an integer >= 1, got {fanout!r}")
    return (None if fanout is None else int(fanout)), float(keep)


def sampling_on(fanout, keep) -> bool:
    """fanout=None, keep=1.0 is OFF (no sampler, no buffer, no launch); any other setting draws, even if every q_i is 1"""
    return fanout is not None or keep != 1.0


def refuse_sampling(model: str, fanout, keep, why: str = "the sweep SpMM's plan is built on the host from host arrays and "
                    "carries the values") -> None:
    """what a model without edge sampling does with fanout= / edge_keep= / set_sampling: the range checks, then ValueError
    naming the argument that switches sampling on.  fanout=None, keep=1.0 passes."""
    fanout, keep = check_sampling(fanout, keep)
    if fanout is not None:
        raise ValueError(f"{model} has no edge sampling: fanout must be None, got {fanout} ({why})")
    if keep != 1.0:
        raise ValueError(f"{model} has no edge sampling: keep (edge_keep) must be 1.0, got {keep} ({why})")


def thresholds(indptr, fanout, keep) -> np.ndarray:
    """t_i = min(floor(q_i * 2^32), 2^32 - 1) as uint32 per row of ``indptr``, q_i = keep * min(1, fanout / deg_i) in float64
    (fanout None: the min is 1; a row without entries has the min 1 too)"""
    fanout, keep = check_sampling(fanout, keep)
    deg = np.diff(np.asarray(indptr).astype(np.int64)).astype(np.float64)
    q = np.full(deg.shape, keep, dtype=np.float64)
    if fanout is not None:
        q = keep * np.minimum(1.0, float(fanout) / np.maximum(deg, 1.0))
    return np.minimum(np.floor(q * 4294967296.0), 4294967295.0).astype(np.uint64).astype(np.uint32)


class sampled_csr:
    """A device-resident CSR pattern as the row-walk ops read their matrix: n(), m() and device() -> (indptr, indices, None).
    indptr has n + 1 words; of indices the first indptr[n] are the sample, the rest of the buffer is not read.  nnz() and
    numpy() synchronise the device and are for tests and reports."""

    def __init__(self, n: int, m: int, indptr, indices):
        self.N_, self.M_ = int(n), int(m)
        self._dev = (indptr, indices, None)

    def n(self) -> int: return self.N_
    def m(self) -> int: return self.M_
    def shape(self): return (self.N_, self.M_)

    def device(self, device=None):
        return self._dev

    def nnz(self) -> int:
        import torch
        torch.cuda.synchronize(self._dev[0].device)
        return int(self._dev[0][self.N_].item()) & 0xFFFFFFFF

    def numpy(self):
        """(indptr, indices) as uint32 host arrays, indices cut to the sample"""
        import torch
        torch.cuda.synchronize(self._dev[0].device)
        indptr = self._dev[0][: self.N_ + 1].cpu().numpy().view(np.uint32)
        return indptr, self._dev[1][: int(indptr[-1])].cpu().numpy().view(np.uint32)


class edge_sampler:
    """edge_sampler(F, F_T, fanout=None, keep=1.0): the sample of a square forward matrix ``F`` (csr_matrix; rows are
    destinations) and of its transpose ``F_T``.  Owns the thresholds on the device and, for each of the two matrices, a counts
    buffer, an indptr buffer and an indices buffer of the parent's nnz -- capacity equals nnz, so there is no overflow case
    (the Reddit-shaped graph: 2 x 459 MB) -- all made with the first draw, when the device is known.  draw(ctx, seed, epoch)
    launches count -> scan -> compact for both matrices and returns the pair (sampled_csr of F, sampled_csr of F_T); the
    same two objects every time, valid until the next draw.  Timers: ``sample-count``, ``sample-scan``, ``sample-compact``,
    each over both matrices."""

    def __init__(self, F: csr_matrix, F_T: csr_matrix, fanout=None, keep: float = 1.0):
        if not (F.n() == F.m() == F_T.n() == F_T.m()):
            raise ValueError(f"edge sampling needs a square matrix and its transpose, got {F.shape()} and {F_T.shape()}")
        self.F, self.F_T = F, F_T
        self._thr = self._bufs = self.pair = None
        self.set(fanout, keep)

    def set(self, fanout, keep) -> None:
        """new thresholds (on the host; uploaded by the next draw)"""
        self.fanout, self.keep = check_sampling(fanout, keep)
        self.thr_host = thresholds(self.F.indptr, self.fanout, self.keep)
        self._thr = None

    def _allocate(self, ctx: context) -> None:
        import torch
        dev, n = ctx.device, self.F.n()
        self._bufs = []
        for M in (self.F, self.F_T):
            self._bufs.append((torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n + 1, dtype=torch.int32, device=dev),
                               torch.empty(max(M.nnz(), 1), dtype=torch.int32, device=dev)))
        self.pair = tuple(sampled_csr(n, n, b[1], b[2]) for b in self._bufs)

    def draw(self, ctx: context, seed: int, epoch: int):
        if self._bufs is None:
            self._allocate(ctx)
        if self._thr is None:
            import torch
            self._thr = torch.from_numpy(self.thr_host.view(np.int32)).to(ctx.device)
            torch.cuda.current_stream(self._thr.device).synchronize()      # visible to every stream afterwards
        n = self.F.n()
        mats = [(M.device(ctx.device), t, b) for t, (M, b) in enumerate(zip((self.F, self.F_T), self._bufs))]
        kw = dict(seed=seed, epoch=epoch)

        def timed(name, call):
            ctx.record(name + "_0", 0)
            for (ip, ix, _), t, b in mats:
                call(ip, ix, t, b)
            ctx.record(name + "_1", 0)
            ctx.register_timer(name, name + "_0", name + "_1")
        timed("sample-count", lambda ip, ix, t, b: ops.edge_sample_count(ctx, n, ip, ix, self._thr, t, b[0], **kw))
        timed("sample-scan", lambda ip, ix, t, b: ops.edge_sample_scan(ctx, b[0], n, b[1]))
        timed("sample-compact", lambda ip, ix, t, b: ops.edge_sample_compact(ctx, n, ip, ix, self._thr, t, b[1], b[2], **kw))
        return self.pair


class sampling_option:
    """set_sampling and its state for a model whose sparse kernels walk rows (gat, sage(aggr="max")).  The model calls
    _init_sampling(fanout, keep) among its option checks, _make_sampler(F, F_T) once its matrices exist, and _draw_sample(ctx,
    training) at the top of every forward: the pair of this forward, or None for the full graph.  A training forward with
    sampling on draws the sample of ``sample_epoch`` and moves it on, exactly as dropout_epoch moves; every other forward --
    a plain call, evaluate(), predict(), attention_weights(ctx, X), correct_and_smooth.predict -- runs on the full graph.
    With fanout=None, keep=1.0 there is no sampler, no buffer, no launch and no timer.  Checkpoints do not store the state: a
    resumed run calls set_sampling(..., epoch=...) itself."""

    sample_fanout = None
    sample_keep = 1.0
    sample_seed = sample_epoch = 0
    sampler = None
    _sample_matrices = None
    sampled_forward = False             # the most recent forward ran on a sample

    def _refuse_sampling(self, fanout, keep) -> None:
        """hook: ValueError for a model option that does not compose with sampling (called only when sampling is on)"""

    def _init_sampling(self, fanout, keep) -> None:
        fanout, keep = check_sampling(fanout, keep)
        if sampling_on(fanout, keep):
            self._refuse_sampling(fanout, keep)
        self.sample_fanout, self.sample_keep = fanout, keep

    def _make_sampler(self, F: csr_matrix, F_T: csr_matrix) -> None:
        self._sample_matrices = (F, F_T)
        if sampling_on(self.sample_fanout, self.sample_keep):
            self.sampler = edge_sampler(F, F_T, self.sample_fanout, self.sample_keep)

    def set_sampling(self, fanout=None, keep: float = 1.0, seed: int = 0, epoch: int = 0) -> None:
        """fanout: None or the expected fan-out per destination (an integer >= 1); keep: the DropEdge keep probability in
        (0, 1]; seed: 64 bits; epoch: the number the next training forward gets (set_sampling(..., epoch=e) replays training
        forward e).  fanout=None, keep=1.0 switches sampling off and frees the buffers.  ValueError naming the argument,
        before any device work and before anything is stored."""
        fanout, keep = check_sampling(fanout, keep)
        if sampling_on(fanout, keep):
            self._refuse_sampling(fanout, keep)
            if self.sampler is None:
                self.sampler = edge_sampler(*self._sample_matrices, fanout, keep)
            else:
                self.sampler.set(fanout, keep)
        else:
            self.sampler = None
        self.sample_fanout, self.sample_keep = fanout, keep
        self.sample_seed, self.sample_epoch = int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch)

    def _draw_sample(self, ctx: context, training: bool):
        if not training or self.sampler is None:
            self.sampled_forward = False
            return None
        pair = self.sampler.draw(ctx, self.sample_seed, self.sample_epoch & 0xFFFFFFFF)
        self.sample_epoch += 1
        self.sampled_forward = True
        return pair
