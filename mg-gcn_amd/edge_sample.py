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
the host never reads a sampled size, and no synchronisation is added.  For gat and sage(aggr="max") values are not carried:
the attention kernels and the max aggregator read the pattern only.

The sample with values.  gcn and sage(aggr="mean") are weighted sums: they take sampling only together with ``edge_rescale``,
which says how the kept values are rescaled -- there is no neutral default.  "row": every kept entry of destination i is
multiplied by r_i = S_i / S'_i, S_i the sum of row i of F and S'_i the sum over its kept entries (row sums are preserved; on the
row-stochastic matrix both models build this is the mean over the sampled neighbours, GraphSAGE's and DropEdge's
re-normalisation; S'_i == 0 gives 0).  "inverse": the Horvitz-Thompson form of FastGCN / GraphSAINT -- a kept entry with i != j
is multiplied by fp32(2^32 / t_i), computed on the host once per setting (t_i == 0xFFFFFFFF gives 1, t_i == 0 gives 0);
self-loops are kept with probability 1 and are not scaled.  The keep bit is the same one, so a sampled gcn and a sampled gat
under one seed train on the same pattern, and the factor is one array per destination that both sides read: the samples of F
and F^T hold the same value bits.  The multiply is the row-split SpMM on a plan built on the device, once per draw and matrix
(ops.spmm_dev_plan_build under the timer ``sample-plan``; csrc/spmm_dev.hip).
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


RESCALES = (None, "row", "inverse")


def check_rescale(rescale):
    """option checking of edge_rescale= / rescale=, before any device work"""
    if rescale is not None and rescale not in RESCALES[1:]:
        raise ValueError(f"edge sampling: edge_rescale (rescale) must be one of {RESCALES}, got {rescale!r}")
    return rescale


def inverse_factors(thr) -> np.ndarray:
    """fp32(2^32 / t_i) per destination, computed in float64: 1 where t_i == 0xFFFFFFFF (kept without a draw), 0 where t_i == 0"""
    t = np.asarray(thr, dtype=np.uint32).astype(np.float64)
    out = np.zeros(t.shape, dtype=np.float64)
    np.divide(4294967296.0, t, out=out, where=t > 0)
    out[t == 4294967295.0] = 1.0
    return out.astype(np.float32)


def refuse_sampling(model: str, fanout, keep, why: str = "a weighted sum needs to be told how the kept values are rescaled: "
                    "pass edge_rescale=") -> None:
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
    """A device-resident CSR pattern as the row-walk ops read their matrix: n(), m() and device() -> (indptr, indices, None) --
    (indptr, indices, values) where the sample was drawn with values (edge_sampler(rescale=...)).
    indptr has n + 1 words; of indices the first indptr[n] are the sample, the rest of the buffer is not read.  nnz() and
    numpy() synchronise the device and are for tests and reports."""

    plan = None                 # with values: the ops.spmm_dev_buffer built for this sample (edge_sampler.draw)

    def __init__(self, n: int, m: int, indptr, indices, values=None):
        self.N_, self.M_ = int(n), int(m)
        self._dev = (indptr, indices, values)

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

    def values_numpy(self):
        """the sample's values as a host fp32 array, cut to the sample (a sample drawn with values)"""
        indptr, _ = self.numpy()
        return self._dev[2][: int(indptr[-1])].cpu().numpy()


class edge_sampler:
    """edge_sampler(F, F_T, fanout=None, keep=1.0, rescale=None, max_d=128): the sample of a square forward matrix ``F``
    (csr_matrix; rows are destinations) and of its transpose ``F_T``.  Owns the thresholds on the device and, for each of the
    two matrices, a counts buffer, an indptr buffer and an indices buffer of the parent's nnz -- capacity equals nnz, so there
    is no overflow case (the Reddit-shaped graph: 2 x 459 MB) -- all made with the first draw, when the device is known.
    draw(ctx, seed, epoch) launches count -> scan -> compact for both matrices and returns the pair (sampled_csr of F,
    sampled_csr of F_T); the same two objects every time, valid until the next draw.  Timers: ``sample-count``,
    ``sample-scan``, ``sample-compact``, each over both matrices.

    ``rescale`` "row" / "inverse" (see the module's text) is the values mode: a values buffer of the parent's nnz per matrix
    beside the indices, one scale array per destination -- written by the count pass over F ("row": ops.edge_sample_rowscale)
    or uploaded with the thresholds ("inverse": inverse_factors) -- and one device-built row-split plan per matrix
    (ops.spmm_dev_plan at the parent's capacity and ``max_d``), built right after compact under ``sample-plan``.  The pair's
    device() is then (indptr, indices, values) and its ``plan`` what ops.spmm_dev takes."""

    def __init__(self, F: csr_matrix, F_T: csr_matrix, fanout=None, keep: float = 1.0, rescale=None, max_d: int = 128):
        if not (F.n() == F.m() == F_T.n() == F_T.m()):
            raise ValueError(f"edge sampling needs a square matrix and its transpose, got {F.shape()} and {F_T.shape()}")
        self.F, self.F_T = F, F_T
        self.rescale, self.max_d = check_rescale(rescale), int(max_d)
        self._thr = self._scale = self._bufs = self.pair = self.plans = None
        self.set(fanout, keep)

    def set(self, fanout, keep) -> None:
        """new thresholds (on the host; uploaded by the next draw)"""
        self.fanout, self.keep = check_sampling(fanout, keep)
        self.thr_host = thresholds(self.F.indptr, self.fanout, self.keep)
        self.inv_host = inverse_factors(self.thr_host) if self.rescale == "inverse" else None
        self._thr = None

    def _allocate(self, ctx: context) -> None:
        import torch
        dev, n = ctx.device, self.F.n()
        self._bufs = []
        for M in (self.F, self.F_T):
            self._bufs.append((torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n + 1, dtype=torch.int32, device=dev),
                               torch.empty(max(M.nnz(), 1), dtype=torch.int32, device=dev),
                               torch.empty(max(M.nnz(), 1), dtype=torch.float32, device=dev) if self.rescale else None))
        self.pair = tuple(sampled_csr(n, n, b[1], b[2], b[3]) for b in self._bufs)
        if self.rescale:
            self._scale = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
            self.plans = tuple(ops.spmm_dev_plan(ctx, M.indptr, self.max_d) for M in (self.F, self.F_T))
            for S, plan in zip(self.pair, self.plans):
                S.plan = plan

    def draw(self, ctx: context, seed: int, epoch: int):
        if self._bufs is None:
            self._allocate(ctx)
        if self._thr is None:
            import torch
            self._thr = torch.from_numpy(self.thr_host.view(np.int32)).to(ctx.device)
            if self.inv_host is not None:
                self._scale.copy_(torch.from_numpy(self.inv_host))
            torch.cuda.current_stream(self._thr.device).synchronize()      # visible to every stream afterwards
        n = self.F.n()
        mats = [(M.device(ctx.device), t, b) for t, (M, b) in enumerate(zip((self.F, self.F_T), self._bufs))]
        kw = dict(seed=seed, epoch=epoch)

        def timed(name, call):
            ctx.record(name + "_0", 0)
            for dev, t, b in mats:
                call(dev, t, b)
            ctx.record(name + "_1", 0)
            ctx.register_timer(name, name + "_0", name + "_1")

        def count(dev, t, b):
            if self.rescale == "row" and t == 0:         # the walk over F leaves the row factors beside the counts
                ops.edge_sample_rowscale(ctx, n, dev[0], dev[1], dev[2], self._thr, b[0], self._scale, **kw)
            else:
                ops.edge_sample_count(ctx, n, dev[0], dev[1], self._thr, t, b[0], **kw)

        def compact(dev, t, b):
            if self.rescale:
                ops.edge_sample_compact_val(ctx, n, dev[0], dev[1], dev[2], self._thr, t, self._scale, self.rescale == "row",
                                            b[1], b[2], b[3], **kw)
            else:
                ops.edge_sample_compact(ctx, n, dev[0], dev[1], self._thr, t, b[1], b[2], **kw)
        timed("sample-count", count)
        timed("sample-scan", lambda dev, t, b: ops.edge_sample_scan(ctx, b[0], n, b[1]))
        timed("sample-compact", compact)
        if self.rescale:
            timed("sample-plan", lambda dev, t, b: ops.spmm_dev_plan_build(ctx, self.plans[t], b[1]))
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
    edge_rescale = None                 # rescaled_sampling_option: how a weighted-sum model rescales the kept values
    _sample_max_d = 128                 # the widest SpMM of a model that samples with values

    def _refuse_sampling(self, fanout, keep) -> None:
        """hook: ValueError for a model option that does not compose with sampling (called only when sampling is on)"""

    def _init_sampling(self, fanout, keep) -> None:
        fanout, keep = check_sampling(fanout, keep)
        if sampling_on(fanout, keep):
            self._refuse_sampling(fanout, keep)
        self.sample_fanout, self.sample_keep = fanout, keep

    def _new_sampler(self, fanout, keep) -> edge_sampler:
        return edge_sampler(*self._sample_matrices, fanout, keep, rescale=self.edge_rescale, max_d=self._sample_max_d)

    def _make_sampler(self, F: csr_matrix, F_T: csr_matrix) -> None:
        self._sample_matrices = (F, F_T)
        if sampling_on(self.sample_fanout, self.sample_keep):
            self.sampler = self._new_sampler(self.sample_fanout, self.sample_keep)

    def set_sampling(self, fanout=None, keep: float = 1.0, seed: int = 0, epoch: int = 0) -> None:
        """fanout: None or the expected fan-out per destination (an integer >= 1); keep: the DropEdge keep probability in
        (0, 1]; seed: 64 bits; epoch: the number the next training forward gets (set_sampling(..., epoch=e) replays training
        forward e).  fanout=None, keep=1.0 switches sampling off and frees the buffers.  ValueError naming the argument,
        before any device work and before anything is stored."""
        fanout, keep = check_sampling(fanout, keep)
        if sampling_on(fanout, keep):
            self._refuse_sampling(fanout, keep)
            if self.sampler is None or self.sampler.rescale != self.edge_rescale:
                self.sampler = self._new_sampler(fanout, keep)
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


class rescaled_sampling_option(sampling_option):
    """sampling_option for the weighted-sum models (gcn, sage): ``edge_rescale`` (None / "row" / "inverse", see the module's
    text) beside the sampling state, ``edge_rescale=`` in the constructor and ``rescale=`` in set_sampling (None there keeps the
    model's).  The model's _refuse_sampling hook reads ``self._rescale_checked()``: the value under check, which is stored as
    ``edge_rescale`` only after every check has passed."""

    _rescale_wanted = ()                # (): no check is running

    def _rescale_checked(self):
        return self.edge_rescale if self._rescale_wanted == () else self._rescale_wanted

    def _refuse_rescale(self, rescale) -> None:
        """hook: ValueError for a model that reads no values (called for any rescale that is not None, sampling on or off)"""

    def _checked(self, fanout, keep, rescale, check) -> None:
        rescale = check_rescale(rescale)
        if rescale is not None:
            self._refuse_rescale(rescale)
        self._rescale_wanted = rescale
        try:
            check(fanout, keep)
        finally:
            self._rescale_wanted = ()

    def _init_sampling(self, fanout, keep, rescale=None) -> None:
        self._checked(fanout, keep, rescale, lambda f, k: sampling_option._init_sampling(self, f, k))
        self.edge_rescale = rescale

    def set_sampling(self, fanout=None, keep: float = 1.0, seed: int = 0, epoch: int = 0, rescale=None) -> None:
        """sampling_option.set_sampling, and ``rescale``: None keeps the model's ``edge_rescale``, "row" / "inverse" replace it.
        A weighted-sum model whose edge_rescale is None refuses any setting that is on, by the argument's name."""
        rescale = self.edge_rescale if rescale is None else rescale

        def check(f, k):
            f, k = check_sampling(f, k)
            if sampling_on(f, k):
                self._refuse_sampling(f, k)
        self._checked(fanout, keep, rescale, check)
        self.edge_rescale = rescale
        sampling_option.set_sampling(self, fanout, keep, seed, epoch)
