"""Link prediction (opt-in; the reference trains node classifiers only): a pairwise head over any single-GPU encoder.

``link_predictor(model, P, neg_ratio=1, seed=0)`` trains ``model`` -- a gcn, sage or gat, any variant and option -- as the
encoder of a graph auto-encoder (Kipf & Welling's GAE, the gcn / sage baselines of the ogbl-* leaderboards): the model's last
layer gives the embeddings H [n x d], a pair (u, v) scores s = H[u] . H[v], and the loss is the mean of softplus(-s) over
the positive pairs plus the mean of softplus(s) over negatives drawn on the device (PyG's ``GAE.recon_loss``).

  Positives   the PATTERN of the csr_matrix P [n x n]: row u, entry v; the values are not read.  An undirected graph lists
              both directions and each is a training example of its own.  M = P.nnz().
  Negatives   ``neg_ratio`` R per positive entry, the head kept and the tail uniform over all vertices: negative (p, r) of
              the entry at position p is (u, v') with v' = (w n) >> 32, w = word r & 3 of
              Philox4x32-10((p, r >> 2, ops.LINK_DOMAIN, epoch), seed).  A negative that happens to be an edge, or v' == u,
              is KEPT: this is the plain uniform sampler of the OGB examples, not a filtered one.  The draw is never stored
              on the head's side -- the loss kernel draws it again inside its walk -- and stored once on the tail's side,
              where a stable radix sort puts it in order of v'.
  Loss        L = (1 / M) sum_pos softplus(-s) + (1 / (M R)) sum_neg softplus(s); accuracy: a pair is predicted a link
              iff s > 0, acc = (#{pos: s > 0} + #{neg: not s > 0}) / (M (1 + R)).

``mlp_link_predictor(model, P, hidden=128, ...)`` is the same head with the decoder of the ogbl-* gcn / sage baselines, an MLP
over H[u] (.) H[v] with one hidden layer, on the matrix cores: see the class.

link_predictor has no parameters: save / load / predict / model_selector of the encoder keep working.  It allocates on first use:
P and P^T on the device, the four sort arrays and the sort's work space, the row pointer of the negatives' transpose, the row
sums and G [n x d].  A program that never constructs one launches, allocates and registers what it did before.  Timers
link-draw, link-sort, link-bounds and link-loss exist once train_step has run.

``head.rank(ctx, X, pos_pairs, neg_pairs=... | neg_tails=...)`` gives the ranking metrics of the leaderboards, MRR and Hits@K,
from exact integers counted on the device (csrc/link_rank.hip): see the method.  It allocates per call and registers the
timer link-rank; a program that never calls it runs what it ran.
"""
from __future__ import annotations

import numbers
from typing import Optional

import numpy as np

from . import ops
from .gcn import _SQRT_1_3, model_base, param_owner
from .matrix import context, csr_matrix, dn_matrix, host_scalars
from .metrics import roc_auc_evaluator


def _torch():
    import torch
    return torch


def check_neg_ratio(neg_ratio, M: int) -> int:
    if not isinstance(neg_ratio, numbers.Integral) or isinstance(neg_ratio, bool) or neg_ratio < 1:
        raise ValueError(f"neg_ratio must be an integer >= 1, not {neg_ratio!r}")
    if M * int(neg_ratio) >= 1 << 31:
        raise ValueError(f"neg_ratio: P.nnz() * neg_ratio must be below 2^31 (the negatives are one sort), got {M * int(neg_ratio)}")
    return int(neg_ratio)


def check_pairs(pairs, n: int, what: str = "pairs") -> np.ndarray:
    """an integer array [m x 2] of vertices in [0, n), as uint32"""
    a = np.asarray(pairs)
    if a.ndim != 2 or a.shape[1] != 2 or a.dtype.kind not in "iu":
        raise ValueError(f"{what} must be an integer array of m x 2, got {a.dtype} of shape {a.shape}")
    if a.shape[0] >= 1 << 31:
        raise ValueError(f"{what}: at most 2^31 - 1 pairs, got {a.shape[0]}")
    if a.size and (int(a.min()) < 0 or int(a.max()) >= n):
        raise ValueError(f"{what} must lie in [0, {n}), got {int(a.min())} .. {int(a.max())}")
    return np.ascontiguousarray(a, dtype=np.uint32)


def pair_metrics(s_pos, s_neg) -> tuple:
    """(loss, acc) of the head's formulas over given scores, in float64 on the host: M = len(s_pos), M R = len(s_neg)"""
    def softplus(x):
        return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))
    s_pos, s_neg = np.asarray(s_pos, dtype=np.float64).reshape(-1), np.asarray(s_neg, dtype=np.float64).reshape(-1)
    loss = (softplus(-s_pos).mean() if s_pos.size else 0.0) + (softplus(s_neg).mean() if s_neg.size else 0.0)
    hits = int((s_pos > 0).sum()) + int((~(s_neg > 0)).sum())
    return float(loss), hits / max(s_pos.size + s_neg.size, 1)


def check_ks(ks) -> tuple:
    if not isinstance(ks, (tuple, list)) or any(not isinstance(k, numbers.Integral) or isinstance(k, bool) or k < 1 for k in ks):
        raise ValueError(f"ks must be a sequence of positive integers, not {ks!r}")
    return tuple(int(k) for k in ks)


def rank_metrics(greater, equal, ks, shared: bool) -> tuple:
    """(mrr, {k: hits@k}) from the device's integers, in int64 and float64 on the host.  rank = 1 + greater + equal / 2 (OGB's
    mean of the optimistic and the pessimistic rank), mrr = mean(1 / rank); per-positive negatives (OGB ``_eval_mrr``):
    hits@k = mean(rank <= k); a shared list (OGB ``_eval_hits``, positive > k-th largest negative): hits@k =
    mean(greater + equal < k), 1.0 by itself with fewer than k negatives."""
    g, e = np.asarray(greater).astype(np.int64).reshape(-1), np.asarray(equal).astype(np.int64).reshape(-1)
    rank = 1.0 + g.astype(np.float64) + e.astype(np.float64) / 2.0
    hits = {int(k): float(np.mean(g + e < k) if shared else np.mean(rank <= k)) for k in ks}
    return float(np.mean(1.0 / rank)), hits


class link_predictor:
    """link_predictor(model, P, neg_ratio=1, seed=0): see the module's text.  ``model``: a single-GPU gcn, sage or gat whose
    last layer's width is the embedding width d (1 <= d <= ops.LINK_MAX_WIDTH; that layer has no activation already).

    train_step(ctx, X, lr, beta1, beta2, weight_decay, eps) -> (loss, acc): the model's training forward (its dropout and its
    own edge sampling behave as in its train_step), draw, sort, bounds, the three loss launches, the layers' backward, Adam,
    ONE synchronisation, the sums.  ``epoch`` advances by one per step; set_negatives(ratio, seed, epoch) replays one.
    score(ctx, X, pairs) -> dn_matrix [m x 1]: a plain forward, then H[u] . H[v] of every pair (an int array [m x 2]).
    evaluate(ctx, X, pos_pairs, neg_pairs) -> {"auc", "loss", "acc"}: exact ROC-AUC on the device (roc_auc_evaluator), loss
    and accuracy by the formulas above with M = len(pos_pairs), M R = len(neg_pairs); no dropout, no sampling, no epoch spent.
    Both upload their pairs (and evaluate its targets) and synchronise on every call: sized for a validation set scored now and
    then, not for a call inside every training step.

    ValueError naming the argument, before any device work: a dist_* model; P not square or not of model.A.n() rows, with
    indptr[0] != 0, without an entry or with a column outside [0, n); neg_ratio < 1 or not an int; P.nnz() * neg_ratio >=
    2^31; pairs outside [0, n)."""

    def __init__(self, model, P: csr_matrix, neg_ratio: int = 1, seed: int = 0):
        if not isinstance(model, model_base):
            raise ValueError(f"model must be a single-GPU gcn, sage or gat (the row-partitioned dist_* models have no link "
                             f"head), not {type(model).__name__}")
        d = int(model._out_width)
        if not 1 <= d <= ops.LINK_MAX_WIDTH:
            raise ValueError(f"model: the last layer's width is the embedding width and must be 1 <= d <= {ops.LINK_MAX_WIDTH}, got {d}")
        n = int(model.A.n())
        if not isinstance(P, csr_matrix) or P.n() != P.m() or P.n() != n:
            got = f"{P.n()} x {P.m()}" if isinstance(P, csr_matrix) else type(P).__name__
            raise ValueError(f"P must be a square csr_matrix of the model's {n} vertices, got {got}")
        if n >= 1 << 31:
            raise ValueError(f"P: n must be below 2^31, got {n}")
        if int(P.indptr[0]) != 0:
            raise ValueError(f"P: indptr[0] must be 0 (an entry's position is its counter), got {int(P.indptr[0])}")
        M = P.nnz()
        if M == 0:
            raise ValueError("P has no entry: there is no positive pair to train on")
        if int(P.indices.max()) >= n:
            raise ValueError(f"P: a column index lies outside [0, {n})")
        self.neg_ratio = check_neg_ratio(neg_ratio, M)
        self.model, self.P, self.n, self.d, self.M = model, P, n, d, M
        self.seed, self.epoch = int(seed), 0
        self.P_T: Optional[csr_matrix] = None
        self._arrays = None
        self._rows = None
        self._auc = None

    def set_negatives(self, ratio=None, seed=None, epoch=None) -> None:
        """the ratio, seed and epoch of the next draw; None leaves one as it is.  The same (ratio, seed, epoch) on the same
        embeddings gives the same bits."""
        if ratio is not None:
            ratio = check_neg_ratio(ratio, self.M)
            if ratio != self.neg_ratio:
                self.neg_ratio, self._arrays = ratio, None
        if seed is not None:
            self.seed = int(seed)
        if epoch is not None:
            self.epoch = int(epoch)

    def sort_bits(self) -> int:
        """the key bits the sort looks at: ceil(log2 n), at least one"""
        return max(1, (self.n - 1).bit_length())

    def _allocate(self, ctx: context) -> None:
        torch = _torch()
        if self.P_T is None:
            self.P_T = self.P.transpose()
        if self._rows is None:
            dev = ctx.device
            self._rows = dict(G=dn_matrix(self.n, self.d, device=dev),
                              nt_indptr=torch.empty(self.n + 1, dtype=torch.int32, device=dev),
                              row_loss=torch.empty(2 * self.n, dtype=torch.float32, device=dev),
                              row_correct=torch.empty(self.n, dtype=torch.int32, device=dev), sums=host_scalars(3))
        if self._arrays is None:
            pairs = self.M * self.neg_ratio
            four = [torch.empty(pairs, dtype=torch.int32, device=ctx.device) for _ in range(4)]
            work = torch.empty(ops.radix_sort_work_bytes(1, pairs) // 8 + 1, dtype=torch.int64, device=ctx.device)
            self._arrays = (four, work)

    def loss_backward(self, ctx: context, H: dn_matrix) -> dn_matrix:
        """draw, sort, bounds, the three loss launches and the sums on the embeddings H, with the negatives of (seed, epoch);
        returns G = dL/dH.  Enqueue-only: read() after a synchronisation."""
        if H.shape() != (self.n, self.d):
            raise ValueError(f"H must be {self.n} x {self.d}, got {H.n()} x {H.m()}")
        self._allocate(ctx)
        n, M, R = self.n, self.M, self.neg_ratio
        (keys, vals, keys_alt, vals_alt), work = self._arrays
        r = self._rows
        p_ip, p_ix, _ = self.P.device(ctx.device)
        t_ip, t_ix, _ = self.P_T.device(ctx.device)
        draw = dict(seed=self.seed, epoch=self.epoch)
        ops.link_neg_draw(ctx, n, p_ip, M, n, R, self.seed, self.epoch, keys, vals, timer="link-draw")
        ops.radix_sort_pairs(ctx, 1, M * R, keys, vals, keys_alt, vals_alt, work, 0, self.sort_bits(), timer="link-sort")
        ops.link_bounds(ctx, keys, M * R, n, r["nt_indptr"], timer="link-bounds")
        w_pos, w_neg = 1.0 / M, 1.0 / (M * R)
        ctx.record("link-loss_0", 0)
        ops.link_dot_loss(ctx, n, n, p_ip, p_ix, M, H, r["G"], True, w_pos, R, w_neg, beta=0.0, row_loss=r["row_loss"],
                          row_correct=r["row_correct"], **draw)
        ops.link_dot_loss(ctx, n, n, t_ip, t_ix, M, H, r["G"], True, w_pos, beta=1.0)
        ops.link_dot_loss(ctx, n, n, r["nt_indptr"], vals, M * R, H, r["G"], False, w_neg, beta=1.0)
        ops.link_sums(ctx, r["row_loss"], r["row_correct"], n, r["sums"])
        ctx.record("link-loss_1", 0)
        ctx.register_timer("link-loss", "link-loss_0", "link-loss_1")
        return r["G"]

    def read(self) -> tuple:
        """(loss, acc) of the last loss_backward, after a synchronisation"""
        words = self._rows["sums"].numpy()
        M, R = self.M, self.neg_ratio
        loss = float(words[0]) / M + float(words[1]) / (M * R)
        return loss, int(words.view(np.uint32)[2]) / (M * (1 + R))

    def train_step(self, ctx: context, X: dn_matrix, lr: float, beta1: float, beta2: float, weight_decay: float, eps: float):
        model = self.model
        H = model(ctx, X, training=True)
        G = self.loss_backward(ctx, H)
        self.epoch += 1
        for layer in reversed(model.layers()):
            G = layer.backward(ctx, G)
        model.adam_update(ctx, lr, beta1, beta2, weight_decay, eps)
        model._launched()
        ctx.sync()
        return self.read()

    def score(self, ctx: context, X: dn_matrix, pairs) -> dn_matrix:
        pairs = check_pairs(pairs, self.n)
        return self._score(ctx, X, pairs)

    def _score(self, ctx: context, X: dn_matrix, pairs: np.ndarray) -> dn_matrix:
        out = self._pair_scores(ctx, self.model(ctx, X), pairs)
        ctx.sync()
        return out

    def _pair_scores(self, ctx: context, H: dn_matrix, pairs: np.ndarray) -> dn_matrix:
        """the decoder's scores [m x 1] of a checked pair list on the embeddings H.  Enqueue-only."""
        m = pairs.shape[0]
        out = dn_matrix(m, 1, device=ctx.device)
        if m:
            src = dn_matrix.from_numpy(pairs[:, 0].view(np.int32), device=ctx.device)
            dst = dn_matrix.from_numpy(pairs[:, 1].view(np.int32), device=ctx.device)
            ops.edge_dot(ctx, src.t.view(-1), dst.t.view(-1), m, H, out.t.view(-1))
        return out

    def _rank_tails(self, ctx: context, H: dn_matrix, src, dst, m: int, tails, K: int, counts) -> None:
        """the fused per-positive kernel of the decoder.  Enqueue-only."""
        ops.link_rank_dot(ctx, src, dst, m, tails, K, H, counts)

    def rank(self, ctx: context, X: dn_matrix, pos_pairs, neg_pairs=None, neg_tails=None, ks=(1, 3, 10, 20, 50, 100)) -> dict:
        """The ranking metrics of the ogbl-* leaderboards -> {"greater": uint32[m], "equal": uint32[m], "mrr", "hits": {k:}}.
        For every positive i the device counts greater[i] / equal[i], its negatives with a score above / equal to its own
        (floats compared, -0.0 == +0.0); rank_metrics turns them into mrr and hits on the host.  Exactly one of
          neg_tails [m x K]      negatives of its own per positive, (pos_pairs[i, 0], neg_tails[i, k]) -- ogbl-citation2's MRR:
                                 one fused kernel scores, compares and counts, H[u] loaded once per positive, no score stored
                                 (ops.link_rank_dot / link_rank_mlp / link_rank_mlp_bf16 by the head's decoder);
          neg_pairs [m_neg x 2]  one list shared by all positives -- Hits@K of ogbl-collab, -ppa, -ddi: score()'s pair kernel
                                 over both lists, the negatives' scores sorted as keys, two bisections per positive.
        Either way the integers are those one would count from score() of the same pairs.  A plain forward: no dropout, no
        sampling, no epoch spent; one synchronisation; timer link-rank.  ValueError naming the argument, before any device work:
        both or neither neg_*; a wrong shape or dtype; a vertex outside [0, n); no positive; m K or m + m_neg >= 2^31; a ks that
        is not a sequence of positive integers."""
        if (neg_pairs is None) == (neg_tails is None):
            raise ValueError("neg_pairs and neg_tails: exactly one of the two must be given")
        pos = check_pairs(pos_pairs, self.n, "pos_pairs")
        m = pos.shape[0]
        if m == 0:
            raise ValueError("pos_pairs has no pair: there is nothing to rank")
        ks = check_ks(ks)
        if neg_tails is not None:
            tails = np.asarray(neg_tails)
            if tails.ndim != 2 or tails.shape[0] != m or tails.dtype.kind not in "iu":
                raise ValueError(f"neg_tails must be an integer array of {m} x K, got {tails.dtype} of shape {tails.shape}")
            K = tails.shape[1]
            if m * K >= 1 << 31:
                raise ValueError(f"neg_tails: m * K must be below 2^31, got {m * K}")
            if tails.size and (int(tails.min()) < 0 or int(tails.max()) >= self.n):
                raise ValueError(f"neg_tails must lie in [0, {self.n}), got {int(tails.min())} .. {int(tails.max())}")
            tails = np.ascontiguousarray(tails, dtype=np.uint32)
        else:
            shape = np.shape(neg_pairs)
            if len(shape) == 2 and m + shape[0] >= 1 << 31:
                raise ValueError(f"pos_pairs and neg_pairs: at most 2^31 - 1 pairs together, got {m + shape[0]}")
            neg = check_pairs(neg_pairs, self.n, "neg_pairs")
            m_neg = neg.shape[0]
        torch = _torch()
        H = self.model(ctx, X)
        counts = torch.empty(2 * m, dtype=torch.int32, device=ctx.device)
        ctx.record("link-rank_0", 0)
        if neg_tails is not None:
            src = dn_matrix.from_numpy(pos[:, 0].view(np.int32), device=ctx.device)
            dst = dn_matrix.from_numpy(pos[:, 1].view(np.int32), device=ctx.device)
            t = dn_matrix.from_numpy(tails.view(np.int32), device=ctx.device)
            self._rank_tails(ctx, H, src.t.view(-1), dst.t.view(-1), m, t.t.view(-1), K, counts)
        else:
            scores = self._pair_scores(ctx, H, np.concatenate([pos, neg]))
            keys, vals, keys_alt, vals_alt = (torch.empty(m_neg, dtype=torch.int32, device=ctx.device) for _ in range(4))
            work = torch.empty(ops.radix_sort_work_bytes(1, m_neg) // 8 + 1, dtype=torch.int64, device=ctx.device)
            zeros = torch.zeros((m_neg, 1), dtype=torch.int32, device=ctx.device)
            ops.roc_auc_keys(ctx, scores.t[m:], zeros, None, 0, 1, keys, vals)
            ops.radix_sort_pairs(ctx, 1, m_neg, keys, vals, keys_alt, vals_alt, work)
            ops.link_rank_sorted(ctx, scores.t.view(-1)[:m], m, keys, m_neg, counts)
        ctx.record("link-rank_1", 0)
        ctx.register_timer("link-rank", "link-rank_0", "link-rank_1")
        ctx.sync()
        words = counts.cpu().numpy().view(np.uint32).reshape(m, 2)
        greater, equal = np.ascontiguousarray(words[:, 0]), np.ascontiguousarray(words[:, 1])
        mrr, hits = rank_metrics(greater, equal, ks, neg_tails is None)
        return {"greater": greater, "equal": equal, "mrr": mrr, "hits": hits}

    def evaluate(self, ctx: context, X: dn_matrix, pos_pairs, neg_pairs) -> dict:
        pos, neg = check_pairs(pos_pairs, self.n, "pos_pairs"), check_pairs(neg_pairs, self.n, "neg_pairs")
        m_pos, m = pos.shape[0], pos.shape[0] + neg.shape[0]
        if m >= 1 << 31:
            raise ValueError(f"pos_pairs and neg_pairs: at most 2^31 - 1 pairs together, got {m}")
        scores = self._score(ctx, X, np.concatenate([pos, neg]))
        if self._auc is None or self._auc.n != m:
            self._auc = roc_auc_evaluator(m, 1)
        Y = dn_matrix.from_numpy(np.concatenate([np.ones(m_pos, np.int32), np.zeros(m - m_pos, np.int32)]), device=ctx.device)
        auc = self._auc(ctx, scores, Y)["all"]
        s = scores.numpy().reshape(-1)
        loss, acc = pair_metrics(s[:m_pos], s[m_pos:])
        return {"auc": auc, "loss": loss, "acc": acc}


def check_mlp_weights(weights, d: int, hidden: int) -> tuple:
    """(W1 [d x hidden], b1 [1 x hidden], w2 [1 x hidden], b2 [1 x 1]) as finite float32 arrays"""
    if not isinstance(weights, (tuple, list)) or len(weights) != 4:
        raise ValueError(f"weights must be (W1, b1, w2, b2), got {type(weights).__name__}"
                         + (f" of {len(weights)}" if isinstance(weights, (tuple, list)) else ""))
    out = []
    for name, w, shape in zip(("W1", "b1", "w2", "b2"), weights, ((d, hidden), (1, hidden), (1, hidden), (1, 1))):
        a = np.asarray(w, dtype=np.float32)
        if a.shape != shape:
            raise ValueError(f"weights: {name} must be {shape[0]} x {shape[1]}, got shape {a.shape}")
        if not np.isfinite(a).all():
            raise ValueError(f"weights: {name} has a non-finite value")
        out.append(np.ascontiguousarray(a))
    return tuple(out)


class _decoder_option(type):
    """mlp_link_predictor(..., decoder_dtype="f32" | "bf16"): the keyword is an option of the call, taken and checked here --
    before __init__ allocates anything -- and left on the instance; __init__ keeps its documented parameter list."""

    def __call__(cls, *args, decoder_dtype: str = "f32", **kw):
        if decoder_dtype not in ("f32", "bf16"):
            raise ValueError(f'decoder_dtype must be "f32" or "bf16", not {decoder_dtype!r}')
        head = super().__call__(*args, **kw)
        head.decoder_dtype = decoder_dtype
        return head


class mlp_link_predictor(link_predictor, metaclass=_decoder_option):
    """mlp_link_predictor(model, P, hidden=128, neg_ratio=1, seed=0, weights=None, decoder_dtype="f32"): link_predictor with
    the decoder of the ogbl-* gcn / sage baselines in place of the dot product -- x = H[u] (.) H[v], z = W1^T x + b1, a = leaky_relu(z) (the
    slope of the gcn layers), s = w2 . a + b2 -- on the matrix cores (csrc/link_mlp.hip).

    Parameters W1 [d x hidden], b1 [1 x hidden], w2 [1 x hidden], b2 [1 x 1], initialised like a linear's W and b (the
    seeded initialiser) or from ``weights`` = (W1, b1, w2, b2); weights() returns them as numpy arrays.  They are not part
    of the encoder's checkpoint: weights() / weights= carry them.  train_step trains them by Adam with the hyper-parameters of
    the call after the model's own update: W1 and w2 decay like a linear's W, b1 and b2 do not, and the step is the fused
    kernel per tensor where the model is fused, the reference's chain otherwise.  The tensors, their gradients and moments
    sit on ``owner``, a plain param_owner described by ``params_table`` (the head is no layer: it has no slot in a checkpoint).

    Positives, negatives, loss, accuracy, set_negatives, evaluate, score and read are the parent's; score and evaluate use
    the MLP.  loss_backward adds one launch after the three walks: the parameters' gradient from one pass over the training
    list of M (1 + R) pairs, the negatives drawn a third time (timer link-wgrad).  On first use it allocates what the parent
    does plus the row of every entry (M words), the packed gradient and its per-workgroup partials.

    decoder_dtype="bf16" (keyword only, opt-in; "f32" constructs, allocates, launches and registers what it always did) runs the decoder on
    the bf16 matrix cores (csrc/link_mlp_b16.hip; the contract in include/mggcn.h): loss_backward and _score round H once into
    a bf16 image of the head's and W1 into its packed image -- the fp32 W1 that Adam has just updated is the master --, then
    launch ops.link_mlp_loss_bf16 / link_mlp_pairs_bf16 in place of their fp32 twins.  x, dz and both operands of the two
    products are bf16 (straight-through in the backward), every sum, the loss, G, the parameters, their gradients and Adam's
    state stay fp32.  score and evaluate use the bf16 decoder too: the model is scored by what it was trained with.  On first
    use it allocates the two images as well (2 n d bytes and at most 68 KiB) and registers the timer link-pack.

    ValueError naming the argument, before any device work: what link_predictor refuses; the model's last width d or
    ``hidden`` not a multiple of 32 in [32, 128] (W1, at most 64 KiB, stays in LDS); ``weights`` of the wrong length or shapes or
    with a non-finite value; a decoder_dtype other than "f32" and "bf16"."""

    params_table = (("W1", "W1", "G_W1", "mW1", "vW1", True), ("b1", "b1", "G_b1", "mb1", "vb1", False),
                    ("w2", "w2", "G_w2", "mw2", "vw2", True), ("b2", "b2", "G_b2", "mb2", "vb2", False))

    decoder_dtype = "f32"                           # the call's keyword (see _decoder_option) overrides it per instance

    def __init__(self, model, P: csr_matrix, hidden: int = 128, neg_ratio: int = 1, seed: int = 0, weights=None):
        link_predictor.__init__(self, model, P, neg_ratio, seed)
        if self.d not in ops.LINK_MLP_WIDTHS:
            raise ValueError(f"model: the MLP decoder needs an embedding width d that is a multiple of 32 in [32, 128], got {self.d}")
        if not isinstance(hidden, numbers.Integral) or isinstance(hidden, bool) or hidden not in ops.LINK_MLP_WIDTHS:
            raise ValueError(f"hidden must be a multiple of 32 in [32, 128], not {hidden!r}")
        self.hidden = hd = int(hidden)
        if weights is not None:
            weights = check_mlp_weights(weights, self.d, hd)
        self.W1, self.b1, self.w2, self.b2 = dn_matrix(self.d, hd), dn_matrix(1, hd), dn_matrix(1, hd), dn_matrix(1, 1)
        if weights is None:
            self.W1.init()
            self.w2.init()
            self.b1.init(_SQRT_1_3)
            self.b2.init(_SQRT_1_3)
        else:
            for t, w in zip(self.params(), weights):
                t.init(w)
        sizes, dev = (self.d * hd, hd, hd, 1), self.W1.t.device
        self._grads = _torch().empty(ops.link_mlp_grad_floats(self.d, hd), dtype=_torch().float32, device=dev)
        cuts = np.concatenate([[0], np.cumsum(sizes)])
        self.G_W1, self.G_b1, self.G_w2, self.G_b2 = (
            dn_matrix(shape, buffer=self._grads[int(lo):int(hi)])
            for shape, lo, hi in zip(((self.d, hd), (1, hd), (1, hd), (1, 1)), cuts[:-1], cuts[1:]))
        o = self.owner = param_owner()
        o.params_table, o.adam_fused = self.params_table, bool(model.fused)
        for _, p, g, m, v, _ in self.params_table:
            setattr(o, p, getattr(self, p))
            setattr(o, g, getattr(self, g))
            setattr(o, m, None)
            setattr(o, v, None)
        self._partials = self._head = self._images = None

    def params(self) -> tuple:
        return self.W1, self.b1, self.w2, self.b2

    def weights(self) -> tuple:
        """(W1, b1, w2, b2) as numpy arrays (synchronise first where a step is in flight)"""
        return tuple(t.numpy() for t in self.params())

    def _allocate(self, ctx: context) -> None:
        link_predictor._allocate(self, ctx)
        if self._head is None:
            torch = _torch()
            rows = np.repeat(np.arange(self.n, dtype=np.uint32), np.diff(self.P.indptr.astype(np.int64)))
            self._head = torch.from_numpy(rows.view(np.int32)).to(ctx.device)
            self._partials = torch.empty(ops.link_mlp_partial_floats(self.d, self.hidden), dtype=torch.float32, device=ctx.device)
            torch.cuda.current_stream(ctx.device).synchronize()

    def _decoder(self, ctx: context, H: dn_matrix) -> tuple:
        """(loss op, pairs op, embeddings, params) of decoder_dtype; bf16 rounds H and W1 into the head's images first"""
        if self.decoder_dtype == "f32":
            return ops.link_mlp_loss, ops.link_mlp_pairs, H, self.params()
        if self._images is None:                    # fresh allocations: the pitch and the bases the kernels' loads assume
            torch = _torch()
            self._images = (torch.empty((self.n, self.d), dtype=torch.bfloat16, device=ctx.device),
                            torch.empty(ops.link_mlp_image_halves(self.d, self.hidden), dtype=torch.bfloat16, device=ctx.device))
        Hb, image = self._images
        ctx.record("link-pack_0", 0)
        ops.convert_bf16(ctx, H, Hb)
        ops.link_mlp_pack_bf16(ctx, self.W1, image)
        ctx.record("link-pack_1", 0)
        ctx.register_timer("link-pack", "link-pack_0", "link-pack_1")
        return ops.link_mlp_loss_bf16, ops.link_mlp_pairs_bf16, Hb, (image, self.b1, self.w2, self.b2)

    def loss_backward(self, ctx: context, H: dn_matrix) -> dn_matrix:
        """draw, sort, bounds, the three link_mlp_loss launches, the parameters' gradient from one link_mlp_pairs launch and
        the sums on the embeddings H; returns G = dL/dH and leaves G_W1, G_b1, G_w2, G_b2.  Enqueue-only."""
        if H.shape() != (self.n, self.d):
            raise ValueError(f"H must be {self.n} x {self.d}, got {H.n()} x {H.m()}")
        self._allocate(ctx)
        n, M, R = self.n, self.M, self.neg_ratio
        (keys, vals, keys_alt, vals_alt), work = self._arrays
        r = self._rows
        p_ip, p_ix, _ = self.P.device(ctx.device)
        t_ip, t_ix, _ = self.P_T.device(ctx.device)
        draw = dict(seed=self.seed, epoch=self.epoch)
        link_mlp_loss, link_mlp_pairs, H, params = self._decoder(ctx, H)
        ops.link_neg_draw(ctx, n, p_ip, M, n, R, self.seed, self.epoch, keys, vals, timer="link-draw")
        ops.radix_sort_pairs(ctx, 1, M * R, keys, vals, keys_alt, vals_alt, work, 0, self.sort_bits(), timer="link-sort")
        ops.link_bounds(ctx, keys, M * R, n, r["nt_indptr"], timer="link-bounds")
        w_pos, w_neg = 1.0 / M, 1.0 / (M * R)
        ctx.record("link-loss_0", 0)
        link_mlp_loss(ctx, n, n, p_ip, p_ix, M, H, params, r["G"], True, w_pos, R, w_neg, beta=0.0,
                      row_loss=r["row_loss"], row_correct=r["row_correct"], **draw)
        link_mlp_loss(ctx, n, n, t_ip, t_ix, M, H, params, r["G"], True, w_pos, beta=1.0)
        link_mlp_loss(ctx, n, n, r["nt_indptr"], vals, M * R, H, params, r["G"], False, w_neg, beta=1.0)
        link_mlp_pairs(ctx, H, params, train=(self._head, p_ix, M, R, n, self.seed, self.epoch), weight=w_pos,
                       neg_weight=w_neg, grads=self._grads, partials=self._partials, timer="link-wgrad")
        ops.link_sums(ctx, r["row_loss"], r["row_correct"], n, r["sums"])
        ctx.record("link-loss_1", 0)
        ctx.register_timer("link-loss", "link-loss_0", "link-loss_1")
        return r["G"]

    def train_step(self, ctx: context, X: dn_matrix, lr: float, beta1: float, beta2: float, weight_decay: float, eps: float):
        model = self.model
        H = model(ctx, X, training=True)
        G = self.loss_backward(ctx, H)
        self.epoch += 1
        for layer in reversed(model.layers()):
            G = layer.backward(ctx, G)
        model.adam_update(ctx, lr, beta1, beta2, weight_decay, eps)
        self.owner.adam_update(ctx, lr, beta1, beta2, weight_decay, eps)
        model._launched()
        ctx.sync()
        return self.read()

    def _pair_scores(self, ctx: context, H: dn_matrix, pairs: np.ndarray) -> dn_matrix:
        m = pairs.shape[0]
        out = dn_matrix(m, 1, device=ctx.device)
        if m:
            src = dn_matrix.from_numpy(pairs[:, 0].view(np.int32), device=ctx.device)
            dst = dn_matrix.from_numpy(pairs[:, 1].view(np.int32), device=ctx.device)
            _, link_mlp_pairs, H, params = self._decoder(ctx, H)
            link_mlp_pairs(ctx, H, params, pairs=(src.t.view(-1), dst.t.view(-1), m), out=out.t.view(-1))
        return out

    def _rank_tails(self, ctx: context, H: dn_matrix, src, dst, m: int, tails, K: int, counts) -> None:
        _, _, H, params = self._decoder(ctx, H)
        rank = ops.link_rank_mlp if self.decoder_dtype == "f32" else ops.link_rank_mlp_bf16
        rank(ctx, src, dst, m, tails, K, H, params, counts)
