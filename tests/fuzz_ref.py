"""The option fuzz on the host: the cases of test_fuzz_options_cpu.py (admission and coverage, no GPU) and
test_gpu_fuzz_options.py (the device run), the composed reference of every case, and the one measure both files use.

gcn_case(seed) / gat_case(seed) return a dict of numpy arrays and options that depends on the seed alone.  What a case draws:
  * the graph: the four laws of test_gpu_fuzz_model._random_graph (restated here with the law passed in) plus "isolated" --
    about a tenth of the rows of A have no entry at all (those vertices are never gathered: F = A^T lists them nowhere),
    another tenth of the columns are never referenced (those vertices' rows of F are empty), no forced self-loop -- and
    "no_loops", the uniform law without the forced self-loop; n from NS;
  * gcn: sizes as the existing fuzz draws them, residual_layer, fused, hoist_first_aggregation, agg_dtype, dropout, norm, loss,
    splits, step (epoch 2 through train_step) and the sweep-form environment knobs; hoist with bf16 is redrawn, never caught;
  * gat: variant, depth 1 to 3, heads as an int or a per-layer list, per-layer (K, dh) so that over the seed set every compiled
    (VEC, NT, U) variant of gat_ref.head_geometry_for is reached by a v1 and by a v2 layer, dropout, attn_dropout (v1 only),
    loss, splits, fused, step; the layers of dh >= 257 go with n <= 200 (the numpy reference holds nnz x K x dh doubles).
    Half of the cases transpose the drawn pattern, so that a law's long rows meet the forward as well as backward_src.
    A tenth of the cases carry one duplicated entry: oracle.transpose, gat_ref.transpose_pattern and the reference models keep
    duplicates as two entries (test_fuzz_options_cpu.py asserts it), as the device promises to.
Law, n, variant, the targeted kernel variant and int-or-list are taken from the seed in turn (so that every value and every
(variant, kernel variant) pair occurs whatever the generator draws); everything else is drawn.

reference(case, oracle, other=False) composes the references the feature tests use, in their order: layernorm_ref.oracle_layer_norm,
then the loss (bce_ref.oracle_bce, or the split-aware softmax below), then dropout_ref.oracle_dropout; bf16_ref.bf16_oracle where
agg_dtype says so; gat_ref.oracle_gat / gat_dropout_ref.oracle_gat_dropout / gatv2_ref.oracle_gatv2 with the loss passed as a
callable.  The device is held to oracle.Gcn(f64acc=True) (the order-free sums) for gcn and to the fp32 twin of the attention
for gat (as in test_gpu_gat.py); ``other`` gives f64acc=False, and for gat the fp64 restatement of the attention between
linears that accumulate in fp64.

distances(case, epoch, got, want) is the measure: (name, value, bar, scalable) per output.  The device run asserts value <= bar;
admission asserts value <= bar / 3 between the two precisions of the reference for every scalable line, and again for a run
whose backward pass takes every activation that is zero within 8 x the two precisions' difference on the other side of zero
(flipped_signs below: leaky_relu' is discontinuous there, and a gradient that hangs on such a sign is no fair question), and
for gat for the twin with D = G . out summed in another order than dalpha (gat_ref.oracle_gat._D: in a one-entry row the two
cancel, exactly only when one order serves both).  The sign-flip line of
the parameters (|P - Po| <= 2.05 lr: Adam's first steps are lr sign(g)) is not scalable: a gradient entry that is rounding
noise flips between any two computations, which is what that bar allows for, so admission holds it at the bar itself.

EXCLUDED holds the seeds that admission refuses, with the reason; at most MAX_EXCLUDED per family."""
import types

import numpy as np

import bce_ref
import dropout_ref
import gat_dropout_ref
import gat_ref
import gatv2_ref
import layernorm_ref
from bf16_ref import GRAD_BAR, GRAD_BAR_REST, W_SOLID_BAR, bf16_oracle

SEEDS = 40
GCN_BASE, GAT_BASE = 7040, 9000       # seed s draws from default_rng(base + s); chosen so that the 40 seeds meet the coverage lines
MAX_EXCLUDED = 4
EXCLUDED = {                               # family -> {seed: why admission (test_fuzz_options_cpu.py) refuses it}; never decided by the device
    "gcn": {6: "the reference's loss is inf: four residual layers under a norm put a vertex's logits 110 apart (fp32 softmax underflows)",
            10: "an activation of layer 0 lies within 8 x the two precisions' difference of zero and its sign moves G_beta[0] by 4e-3",
            11: "activations within 8 x the two precisions' difference of zero: with their signs flipped the gradients move by more than a third of the bar",
            29: "a norm over two columns is sign(a - b): layer 0's gradients differ by 4e-4 between f64acc=True and False"},
    "gat": {3: "almost every row holds one entry, so G_att[0] (512 columns) is what is left of D - dalpha: summing D in another order moves att[0]'s step past its bar",
            26: "G_att of a 130-column head on 16 vertices cancels: the fp32 twin is 9.6e-5 from the fp64 restatement, the bar is 1e-4",
            39: "as seed 3, with a 1023-column layer: G_att[0] is 3e-5 of the model's largest gradient and hangs on the order D is summed in"},
}

TOL = 1e-4
ADAM = layernorm_ref.ADAM
LR = ADAM[0]
GRAPH_LAWS = ("uniform", "power", "giant", "loops_mostly", "isolated", "no_loops")
NS = (8, 16, 40, 64, 200, 520, 1500)
SPLIT_NAMES = bce_ref.SPLIT_NAMES


def admitted(family):
    return [s for s in range(SEEDS) if s not in EXCLUDED[family]]


# ---- graphs ------------------------------------------------------------------------------------------------------------------------
def random_graph(rng, n, law):
    """CSR (indptr, indices, ones) of A by ``law``; columns sorted within a row, no duplicates"""
    loops = law not in ("isolated", "no_loops")
    if law in ("uniform", "no_loops", "isolated"):
        lens = rng.integers(0, min(n, 40), size=n)
    elif law == "power":
        lens = np.minimum((rng.pareto(1.2, size=n) * 4).astype(np.int64), n - 1)
    elif law == "giant":
        lens = rng.integers(0, 6, size=n)
        lens[int(rng.integers(0, n))] = n - 1
    else:
        lens = (rng.random(n) < 0.15) * rng.integers(1, 4, size=n)
    allowed = np.arange(n)
    if law == "isolated":
        k = max(1, n // 10)
        pick = rng.permutation(n)
        lens[pick[:k]] = 0                                       # rows of A without an entry: nobody gathers these vertices
        allowed = np.setdiff1d(allowed, pick[k:2 * k])           # ... and these columns are never referenced: empty rows of F
    rows = []
    for r in range(n):
        k = int(min(lens[r], allowed.size))
        others = rng.choice(allowed, size=k, replace=False) if k else np.zeros(0, np.int64)
        rows.append(np.unique(np.concatenate([others, [r]])) if loops else np.unique(others))
    ip = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.uint32)
    ix = np.concatenate(rows).astype(np.uint32)
    return ip, ix, np.ones(len(ix), np.float32)


def with_duplicate(rng, ip, ix):
    """one entry of A listed twice (next to itself, so the row stays sorted); returns (ip, ix, dv, (row, column))"""
    lens = np.diff(ip.astype(np.int64))
    r = int(rng.choice(np.flatnonzero(lens > 0)))
    e = int(ip[r]) + int(rng.integers(0, lens[r]))
    ix2 = np.insert(ix, e, ix[e]).astype(np.uint32)
    ip2 = ip.astype(np.int64).copy()
    ip2[r + 1:] += 1
    return ip2.astype(np.uint32), ix2, np.ones(len(ix2), np.float32), (r, int(ix[e]))


def graph_facts(ip, ix, n):
    """what the coverage test counts: rows of F = A^T without an entry, vertices nobody gathers"""
    return dict(empty_F_rows=int(n - np.unique(ix).size), never_gathered=int((np.diff(ip.astype(np.int64)) == 0).sum()))


def _splits(rng, n):
    S = rng.choice(np.array([0, 1, 2, 3, -1], dtype=np.int32), size=n, p=(0.5, 0.2, 0.2, 0.05, 0.05)).astype(np.int32)
    S[int(rng.integers(0, n))] = 0                               # set_splits refuses a model nobody trains
    return S


def _targets(rng, loss, n, C):
    if loss == "bce":
        return (rng.random((n, C)) < 0.2).astype(np.int32)
    return rng.integers(0, C, size=(n, 1)).astype(np.int32)


# ---- gcn cases -------------------------------------------------------------------------------------------------------------------------
GCN_OPTIONS = dict(residual_layer=(False, True), fused=(False, True), hoist_first_aggregation=(False, True),
                   agg_dtype=("f32", "bf16"), dropout=(0.0, 0.3, 0.5), norm=(None, "layer"), loss=("softmax", "bce"),
                   splits=(False, True), step=(False, True), sweep=(False, True))
WIDTH1_NORM_SEEDS = (5, 18, 31)            # a width-1 hidden layer under norm="layer": zero variance in every row


def gcn_case(seed):
    rng = np.random.default_rng(GCN_BASE + seed)
    law = GRAPH_LAWS[seed % len(GRAPH_LAWS)]
    n = NS[seed % len(NS)]
    ip, ix, dv = random_graph(rng, n, law)
    F = int(rng.choice([1, 2, 3, 16, 33, 100, 128, 608]))
    C = int(rng.choice([2, 3, 7, 41, 47]))
    hidden = [int(rng.choice([1, 2, 5, 16, 33, 64, 128, 200])) for _ in range(int(rng.integers(0, 4)))]
    opt = {}
    for name in ("residual_layer", "fused", "dropout", "norm", "loss", "splits", "step"):
        opt[name] = GCN_OPTIONS[name][int(rng.integers(0, len(GCN_OPTIONS[name])))]
    while True:                                                  # the one illegal pair: redrawn, never caught
        opt["hoist_first_aggregation"], opt["agg_dtype"] = bool(rng.integers(0, 2)), ("f32", "bf16")[int(rng.integers(0, 2))]
        if not (opt["hoist_first_aggregation"] and opt["agg_dtype"] == "bf16"):
            break
    if seed in WIDTH1_NORM_SEEDS:
        opt["norm"] = "layer"
        hidden = (hidden or [16])
        hidden[int(rng.integers(0, len(hidden)))] = 1
    env = {}
    if rng.random() < 0.4:                                       # the sweep form, exactly as test_gpu_fuzz_model.py sets it
        env = {"MGGCN_SPMM_SWEEP_MIN_NNZ": "1", "MGGCN_SPMM_SWEEP_MIN_RUN_X10": "0",
               "MGGCN_SPMM_PANEL_ROWS": str(int(rng.choice([64, 128]))), "MGGCN_SPMM_PANEL_ROWS_NARROW": "96",
               "MGGCN_SPMM_PERMUTE_COLUMNS": str(int(rng.integers(0, 2)))}
    opt["sweep"] = bool(env)
    if opt["residual_layer"] and hidden and hidden[-1] < 5:
        # a bottleneck of one or two columns under the classifier, fed by a residual branch with the unnormalised sum of the layer
        # below (|h| ~ 18 against a W of +-1.7): some vertex's logits end up more than 100 apart, the p_y of its random label
        # underflows in the oracle's fp32 softmax and the REFERENCE's loss is inf (at width 1 and
        # again at width 2).  The forced width-1 cases of WIDTH1_NORM_SEEDS keep theirs.
        if seed not in WIDTH1_NORM_SEEDS:
            hidden[-1] = 5
    sizes = [F] + hidden + [C]
    opt["dropout_seed"] = int(rng.integers(0, 2 ** 62))
    X = rng.standard_normal((n, F), dtype=np.float32)
    Y = _targets(rng, opt["loss"], n, C)
    S = _splits(rng, n) if opt["splits"] else None
    return dict(family="gcn", seed=seed, n=n, law=law, ip=ip, ix=ix, dv=dv, sizes=sizes, X=X, Y=Y, S=S, opt=opt, env=env,
                facts=graph_facts(ip, ix, n))


def gcn_kwargs(case):
    o = case["opt"]
    return dict(residual_layer=o["residual_layer"], fused=o["fused"], hoist_first_aggregation=o["hoist_first_aggregation"],
                agg_dtype=o["agg_dtype"], dropout=o["dropout"], norm=o["norm"], loss=o["loss"])


def gemm_first(case):
    s = case["sizes"]
    return [s[i + 1] <= s[i] for i in range(len(s) - 1)]


def hoist_effective(case):
    """what gcn.set_hoist_first_aggregation decides: asked for, GEMM-first first layer, no residual branch, no empty row of F"""
    return bool(case["opt"]["hoist_first_aggregation"] and gemm_first(case)[0] and not case["opt"]["residual_layer"]
                and case["facts"]["empty_F_rows"] == 0)


# ---- gat cases -------------------------------------------------------------------------------------------------------------------------
KERNEL_VARIANTS = ((4, 1, 4), (4, 4, 1), (1, 1, 4), (1, 4, 2), (1, 16, 1))
# (K, dh) per compiled variant; every pool has a one-head entry (the last layer of an int ``heads``)
POOLS = {
    (4, 1, 4): [(4, 32), (4, 12), (16, 4), (1, 100), (2, 20), (16, 8), (1, 8), (8, 4)],
    (4, 4, 1): [(1, 260), (2, 264), (1, 512)],
    (1, 1, 4): [(3, 7), (5, 1), (2, 3), (2, 5), (1, 6), (1, 10), (16, 1), (1, 41), (6, 1), (3, 5), (1, 7)],
    (1, 4, 2): [(2, 65), (1, 130), (1, 255)],
    (1, 16, 1): [(1, 257), (3, 341), (2, 258)],
}
NARROW = [kd for v in ((4, 1, 4), (1, 1, 4)) for kd in POOLS[v]]
WIDE_N = (40, 64, 200)                     # the layers of dh >= 257 go with these
GAT_OPTIONS = dict(variant=("v1", "v2"), fused=(False, True), dropout=(0.0, 0.5), attn_dropout=(0.0, 0.3),
                   loss=("softmax", "bce"), splits=(False, True), step=(False, True), heads_list=(False, True))


def layer_variant(dh):
    return gat_ref.head_geometry_for(dh, dh % 4 == 0)[0]


def _pick(rng, pool, K=None):
    pool = [kd for kd in pool if K is None or kd[0] == K]
    return pool[int(rng.integers(0, len(pool)))]


def gat_case(seed):
    rng = np.random.default_rng(GAT_BASE + seed)
    variant = GAT_OPTIONS["variant"][seed % 2]
    target = KERNEL_VARIANTS[(seed // 2) % 5]
    heads_list = bool((seed // 10) % 2)
    depth = int(rng.integers(1, 4))
    law = GRAPH_LAWS[(seed + seed // 6) % len(GRAPH_LAWS)]
    wide = target in ((4, 4, 1), (1, 16, 1))
    n = WIDE_N[seed % len(WIDE_N)] if wide else NS[(seed + seed // 7) % len(NS)]
    ip, ix, dv = random_graph(rng, n, law)
    if rng.random() < 0.5:                                       # the law on F = A^T instead of A: the giant row is then the forward's
        ip, ix = gat_ref.transpose_pattern(ip, ix, n)
    dup = None
    if seed % 10 == 7:
        ip, ix, dv, dup = with_duplicate(rng, ip, ix)
    if heads_list:
        layers = [_pick(rng, NARROW) for _ in range(depth)]
        layers[int(rng.integers(0, depth))] = _pick(rng, POOLS[target])
        heads = [k for k, _ in layers]
    else:                                                        # an int: every hidden layer has it, the last layer one head
        if depth == 1:
            heads, layers = int(rng.choice([1, 4])), [_pick(rng, POOLS[target], K=1)]
        else:
            K, dh = _pick(rng, POOLS[target])
            hidden = [(K, int(rng.choice([1, 3, 4, 5, 8, 12]))) for _ in range(depth - 1)]
            hidden[int(rng.integers(0, depth - 1))] = (K, dh)
            layers = hidden + [(1, int(rng.choice([2, 3, 5, 6, 7, 10, 41])))]
            heads = K
    # no single feature column: every Z would be x w + b, of rank one, and G_att -- a sum of ds_dst Z over rows whose ds cancel --
    # is then within rounding of its own cancellation in BOTH precisions of the reference (admission refuses such cases)
    F = int(rng.choice([3, 16, 33, 100]))
    sizes = [F] + [k * dh for k, dh in layers]
    opt = dict(variant=variant, heads_list=heads_list)
    for name in ("fused", "dropout", "loss", "splits", "step"):
        opt[name] = GAT_OPTIONS[name][int(rng.integers(0, 2))]
    if sizes[-1] > 64:
        # the gradient of the multi-label loss is (p - t) / (n m): over hundreds of columns it sinks to the size of Adam's weight
        # decay term 5e-4 W, g + wd W nearly cancels in entries that |g| > 1e-2 max |g| calls well-conditioned, and the two
        # precisions of the reference step apart by more than the bar there
        opt["loss"] = "softmax"
    opt["attn_dropout"] = GAT_OPTIONS["attn_dropout"][int(rng.integers(0, 2))] if variant == "v1" else 0.0
    opt["dropout_seed"] = int(rng.integers(0, 2 ** 62))
    # att as the engine draws it, shrunk with sqrt(dh) beyond dh = 32 (gat_ref.edge_case's rule: the scores keep the spread
    # they have there, so that the softmax of a long row does not sit on a handful of entries)
    att_scale = [min(1.0, (32.0 / dh) ** 0.5) for _, dh in layers]
    X = rng.standard_normal((n, F), dtype=np.float32)
    Y = _targets(rng, opt["loss"], n, sizes[-1])
    S = _splits(rng, n) if opt["splits"] else None
    return dict(family="gat", seed=seed, n=n, law=law, ip=ip, ix=ix, dv=dv, sizes=sizes, heads=heads, layers=layers,
                per_layer_heads=[k for k, _ in layers], att_scale=att_scale, X=X, Y=Y, S=S, opt=opt, env={}, dup=dup,
                target=target, facts=graph_facts(ip, ix, n))


def gat_kwargs(case):
    o = case["opt"]
    return dict(heads=case["heads"], loss=o["loss"], fused=o["fused"], dropout=o["dropout"], attn_dropout=o["attn_dropout"],
                variant=o["variant"])


def describe(case):
    keys = ("family", "seed", "n", "law", "sizes", "heads", "opt", "env", "dup", "facts")
    return {k: case[k] for k in keys if k in case}


# ---- the split-aware softmax loss on the host ---------------------------------------------------------------------------------------------
class softmax_loss:
    """the oracle's softmax cross-entropy, over all rows or over the training split (test_gpu_splits._oracle_split_epoch's
    composition: scaled by 1 / n_train, the gradient rows of the other sets zeroed; per-split loss in fp64 from the oracle's
    probabilities, first-maximum argmax).  loss(H) -> (G, (loss, acc)); ``per``: name -> (loss, acc, None, rows)"""

    def __init__(self, oracle, Y, S=None, f64acc=False):
        self.orc, self.Y, self.f64acc = oracle, np.asarray(Y), f64acc
        self.S = None if S is None else np.asarray(S).reshape(-1)
        self.per = {}

    def loss(self, H):
        n = H.shape[0]
        if self.S is None:
            ls, ac, G, _ = self.orc.softmax_cross_entropy(H, self.Y, f64acc=self.f64acc)
            nf = np.float32(n)
            return G, (float(np.float32(ls) / nf), float(np.float32(ac) / nf))
        train = self.S == 0
        _, _, G, Pr = self.orc.softmax_cross_entropy(H, self.Y, n_global=int(train.sum()), f64acc=self.f64acc)
        G[~train] = 0
        y = self.Y.reshape(-1)
        with np.errstate(divide="ignore"):
            nll = np.abs(np.log(Pr.astype(np.float64)[np.arange(n), y]))
        hit = Pr.argmax(axis=1) == y
        slot = bce_ref.slot(self.S)
        for k, name in enumerate(SPLIT_NAMES):
            r = slot == k
            c = int(r.sum())
            self.per[name] = ((float(nll[r].sum() / c), float(hit[r].sum() / c)) if c else (float("nan"), float("nan"))) + (None, c)
        return G, self.per["train"][:2]


class _bce_loss:
    """bce_ref.oracle_bce's loss without an oracle.Gcn under it: loss(H) -> (G, (loss, micro-F1)), ``per`` as there"""

    def __init__(self, oracle, T, S):
        self.holder = types.SimpleNamespace(train_forward=None)
        self.B = bce_ref.oracle_bce(oracle, self.holder, T, S, 0)
        self.per = self.B.per

    def loss(self, H):
        res = self.B.loss(H)
        return self.holder.G, res


# ---- the composed reference ----------------------------------------------------------------------------------------------------------------
class Reference:
    """one case's reference model behind one interface: set_state(state) takes over parameters and Adam moments,
    epoch() runs train_forward, backward and adam_update and returns what distances() compares"""

    def __init__(self, case, oracle, exact, reorder=False):
        self.case, self.orc, self.exact = case, oracle, exact
        o = case["opt"]
        ip, ix, dv, n = case["ip"].copy(), case["ix"].copy(), case["dv"].copy(), case["n"]
        self.losser = None
        if case["family"] == "gcn":
            if o["agg_dtype"] == "bf16":
                O = bf16_oracle(oracle, ip, ix, dv, n, case["sizes"], o["residual_layer"], f64acc=exact)
            else:
                O = oracle.Gcn(oracle.Csr(ip, ix, dv, n), case["sizes"], f64acc=exact, residual_layer=o["residual_layer"])
            if o["norm"]:
                layernorm_ref.oracle_layer_norm(oracle, O)
            if o["loss"] == "bce":
                self.losser = bce_ref.oracle_bce(oracle, O, case["Y"], case["S"], 0)
            elif case["S"] is not None:
                self.losser = softmax_loss(oracle, case["Y"], case["S"], f64acc=exact)

                def train_forward(X, Y=None, O=O, L=self.losser):
                    O.G, res = L.loss(O.forward(np.ascontiguousarray(X, dtype=np.float32)))
                    return res
                O.train_forward = train_forward
            if o["dropout"]:
                dropout_ref.oracle_dropout(O, o["dropout"], seed=o["dropout_seed"])
        else:
            self.losser = (_bce_loss(oracle, case["Y"], case["S"]) if o["loss"] == "bce"
                           else softmax_loss(oracle, case["Y"], case["S"]))
            A = oracle.Csr(ip, ix, dv, n)
            kw = dict(loss=self.losser.loss, dtype=np.float64 if exact else np.float32)
            heads = case["per_layer_heads"]
            if o["variant"] == "v2":
                O = gatv2_ref.oracle_gatv2(oracle, A, case["sizes"], heads, p=o["dropout"], seed=o["dropout_seed"], **kw)
            elif o["dropout"] or o["attn_dropout"]:
                O = gat_dropout_ref.oracle_gat_dropout(oracle, A, case["sizes"], heads, p=o["dropout"], attn_p=o["attn_dropout"],
                                                       seed=o["dropout_seed"], **kw)
            else:
                O = gat_ref.oracle_gat(oracle, A, case["sizes"], heads, **kw)
            for L, s in zip(O.layers, case["att_scale"]):
                L.att = (L.att * np.float32(s)).astype(np.float32)
            O.reorder_D = bool(reorder)
            for L in O.layers:
                L.lin.f64acc = bool(exact)                       # the other precision of the linears too: the device's GEMMs round as well
        self.O = O

    # -- state ------------------------------------------------------------------------------------------------------------------------
    def initial(self):
        """what the device model is initialised with beyond its own seed-99 draw: per layer (gamma, beta) / att, or None"""
        out = []
        for L in self.O.layers:
            N = getattr(L, "norm", None)
            out.append(dict(norm=None if N is None else (N.gamma.copy(), N.beta.copy()),
                            att=L.att.copy() if self.case["family"] == "gat" else None))
        return out

    def get_state(self):
        return [_layer_state(L, False) for L in self.O.layers]

    def set_state(self, state):
        for L, s in zip(self.O.layers, state):
            for key, obj in _parts(L):
                if key not in s:
                    continue
                for name, v in s[key].items():
                    setattr(obj, name, v if name == "step" else np.array(v, copy=True))

    # -- one epoch ---------------------------------------------------------------------------------------------------------------------
    def epoch(self):
        O, case = self.O, self.case
        loss, score = O.train_forward(case["X"], case["Y"])
        O.backward()
        res = dict(loss=loss, score=score, grads=_grads(O.layers, False))
        if self.losser is not None:
            res["per"] = dict(self.losser.per)
        O.adam_update()
        res["grads_after"] = _grads(O.layers, False)
        res["params"] = _params(O.layers, False)
        return res


# An activation that the reference's two precisions put closer to zero than 8 x their own difference there (the project's factor
# between a twin's error and a bar, gat_ref.ROW_TOL) may come out on the other side of zero on the device, and leaky_relu' then
# differs by 0.99: a gradient that depends on such a sign is not a fair question at 1e-4.  recorded_signs() keeps the sign
# sources of a backward pass; flipped_signs() runs one with every such activation taken on the other side, and admission
# holds the result against the unflipped run like the second precision.  Exact zeros (an empty row's) agree on both sides.
SIGN_FACTOR = 8.0


class recorded_signs:
    """keeps the ``act`` of every oracle.leaky_relu_backward call made inside the block, in call order"""

    def __init__(self, oracle):
        self.orc, self.acts = oracle, []

    def _call(self, act, G, alpha=0.01):
        self.acts.append(np.array(act, dtype=np.float32, copy=True))
        return self.inner(act, G, alpha)

    def __enter__(self):
        self.inner = self.orc.leaky_relu_backward
        self.orc.leaky_relu_backward = self._call
        return self

    def __exit__(self, *exc):
        self.orc.leaky_relu_backward = self.inner


class flipped_signs(recorded_signs):
    """call k takes act on the other side of zero wherever 0 < |act| <= margins[k] and a gradient arrives"""

    def __init__(self, oracle, margins):
        recorded_signs.__init__(self, oracle)
        self.margins, self.flipped = list(margins), 0

    def _call(self, act, G, alpha=0.01):
        act = np.asarray(act, dtype=np.float32)
        near = (act != 0) & (np.abs(act) <= self.margins[len(self.acts)]) & (np.asarray(G) != 0)
        self.acts.append(act)
        self.flipped += int(near.sum())
        return self.inner(np.where(near, -act, act), G, alpha)


class undetermined_signs(recorded_signs):
    """For the device run.  Call k takes the sign source from ``device[k]`` wherever the reference cannot tell its sign: where
    0 < |act| <= SIGN_FACTOR x |act - other.acts[k]|, ``other`` being the record of the reference's other precision from the
    same state.  Which activations those are depends on the last bits of the state an epoch starts from, and the device's
    second epoch starts from its own Adam step, so admission cannot visit that state; the rule is the same one, applied where
    the state is known, and still decided by the reference alone.  Everywhere else the reference keeps its own sign."""

    def __init__(self, oracle, other, device):
        recorded_signs.__init__(self, oracle)
        self.other, self.device, self.taken = other, device, 0

    def _call(self, act, G, alpha=0.01):
        k = len(self.acts)
        act = np.asarray(act, dtype=np.float32)
        near = (act != 0) & (np.abs(act) <= SIGN_FACTOR * np.abs(act.astype(np.float64) - self.other.acts[k])) & (np.asarray(G) != 0)
        self.acts.append(act)
        self.taken += int(near.sum())
        return self.inner(np.where(near, self.device[k].reshape(act.shape), act), G, alpha)


def sign_margins(held, *others):
    """per recorded call, SIGN_FACTOR x the largest difference of ``held``'s sign source from any of the others'"""
    return [SIGN_FACTOR * np.max([np.abs(a.astype(np.float64) - o.acts[k]) for o in others], axis=0) for k, a in enumerate(held.acts)]


def reference(case, oracle, other=False, reorder=False):
    """the composed reference at the precision the device is held to -- f64acc=True for gcn (test_gpu_bce.py's choice: the
    order-free sums), the fp32 twin of the attention for gat (test_gpu_gat.py's) -- or, with ``other``, at its other one;
    ``reorder`` (gat): the twin with D = G . out summed in another order than dalpha, see gat_ref.oracle_gat._D"""
    return Reference(case, oracle, exact=(case["family"] == "gcn") != bool(other), reorder=reorder)


def _parts(L):
    """(key, object) of everything in a layer that Adam updates, device layer or reference layer alike"""
    out = [("lin", L.lin)]
    if getattr(L, "res_lin", None) is not None:
        out.append(("res", L.res_lin))
    if getattr(L, "norm", None) is not None:
        out.append(("norm", L.norm))
    if hasattr(L, "attn"):
        out.append(("att", L.attn))
    elif hasattr(L, "att") and not callable(L.att):
        out.append(("att", L))
    return out


_STATE = dict(lin=("W", "b", "mW", "vW", "mb", "vb"), res=("W", "b", "mW", "vW", "mb", "vb"),
              norm=("gamma", "beta", "mg", "vg", "mb", "vb"), att=("att", "m", "v"))


def _host(v, dev):
    return v.numpy().copy() if dev else np.array(v, copy=True)


def _layer_state(L, dev):
    s = {}
    for key, obj in _parts(L):
        s[key] = {name: _host(getattr(obj, name), dev) for name in _STATE[key] if getattr(obj, name, None) is not None}
        if len(s[key]) == len(_STATE[key]):                      # the moments exist: their step counts
            s[key]["step"] = obj.step
    return s


def device_state(G):
    return [_layer_state(L, True) for L in G.layers()]


def _grads(layers, dev):
    out = []
    for L in layers:
        row = {"G_W": L.lin.G_W, "G_b": L.lin.G_b}
        if getattr(L, "res_lin", None) is not None:
            row.update(res_G_W=L.res_lin.G_W, res_G_b=L.res_lin.G_b)
        if getattr(L, "norm", None) is not None:
            row.update(G_gamma=L.norm.G_gamma, G_beta=L.norm.G_beta)
        if hasattr(L, "attn"):
            row["G_att"] = L.attn.G_att
        elif hasattr(L, "G_att"):
            row["G_att"] = L.G_att
        out.append({k: _host(v, dev) for k, v in row.items()})
    return out


def _params(layers, dev):
    out = []
    for L in layers:
        row = {"W": L.lin.W, "b": L.lin.b}
        if hasattr(L, "attn"):
            row["att"] = L.attn.att
        elif hasattr(L, "att") and not callable(L.att):
            row["att"] = L.att
        out.append({k: _host(v, dev) for k, v in row.items()})
    return out


def device_grads(G):
    return _grads(G.layers(), True)


def device_params(G):
    return _params(G.layers(), True)


# ---- the measure ------------------------------------------------------------------------------------------------------------------------------
def _rel(got, want):
    if np.isnan(want) and np.isnan(got):
        return 0.0
    return abs(got - want) / max(abs(want), 1e-30)


def distances(case, epoch, got, want):
    """(name, value, bar, scalable) of everything the device is held to in one epoch.  ``got``: loss, score, grads (after the
    Adam step where this epoch went through train_step), params (after the Adam step), and with splits ``per`` (name -> (loss,
    score, (tp, fp, fn) or None, rows)), with bce ``conf`` of the reported split.  ``want``: Reference.epoch()'s."""
    o, n = case["opt"], case["n"]
    bf16 = o.get("agg_dtype") == "bf16"
    out = [("loss", _rel(got["loss"], want["loss"]), TOL, True)]
    per = want.get("per") or {}
    rows = per["train"][3] if case["S"] is not None else n
    if o["loss"] == "bce":
        wconf = per["train"][2]
        out.append(("confusion", float(max(abs(a - b) for a, b in zip(got["conf"], wconf))), 3.0, True))
    else:
        out.append(("accuracy", abs(got["score"] - want["score"]) * rows, 3.0 + 1e-6, True))
    if case["S"] is not None:
        for name in SPLIT_NAMES:
            wl, ws, wc, cnt = per[name]
            gl, gs, gc, gcnt = got["per"][name]
            out.append((f"rows[{name}]", float(abs(gcnt - cnt)), 0.0, False))
            out.append((f"loss[{name}]", _rel(gl, wl), TOL, True))
            if o["loss"] == "bce":
                out.append((f"confusion[{name}]", float(max(abs(a - b) for a, b in zip(gc, wc))), 3.0, True))
            elif cnt:
                out.append((f"accuracy[{name}]", abs(gs - ws) * cnt, 3.0 + 1e-6, True))
    after = bool(o["step"]) and epoch == 1
    wg = want["grads_after"] if after else want["grads"]
    # gradients relative to the largest gradient of the model: a layer whose true gradient is rounding noise next to the others
    # (behind a width-1 bottleneck, or below a zero-variance norm) has no 1e-4 of its own to be held to (test_gpu_fuzz_model.py)
    gmax = max(float(np.abs(v).max()) for row in wg for v in row.values())
    for li, (g, w) in enumerate(zip(got["grads"], wg)):
        assert set(g) == set(w), (li, sorted(g), sorted(w))
        for name in sorted(w):
            bar = TOL
            if bf16:                                             # test_bf16_model_matches_the_bf16_oracle's
                bar = GRAD_BAR.get(li, GRAD_BAR_REST) if name == "G_W" else GRAD_BAR_REST
            err = float(np.abs(g[name].astype(np.float64) - w[name]).max())
            out.append((f"{name}[{li}]", err / max(float(np.abs(w[name]).max()), 1e-2 * gmax, 1e-300), bar, True))
    if case["family"] == "gat" or bf16:
        # test_gat_epochs_match_the_reference / test_bf16_model_matches_the_bf16_oracle: never more than a sign flip, and the
        # well-conditioned entries (by the reference's gradient BEFORE the step) at TOL (bf16, first layer: W_SOLID_BAR)
        for li, (p, w) in enumerate(zip(got["params"], want["params"])):
            for name in sorted(w):
                if name == "b" and not bf16:
                    continue
                d = np.abs(p[name].astype(np.float64) - w[name])
                out.append((f"{name}[{li}] flip", float(d.max()) / (2.05 * LR), 1.0, False))
                g = np.abs(want["grads"][li]["G_" + name])
                solid = g > 1e-2 * g.max()
                if solid.any():
                    bar = W_SOLID_BAR.get(li, TOL) if bf16 else TOL
                    out.append((f"{name}[{li}] solid", float(d[solid].max()) / max(float(np.abs(w[name]).max()), 1e-300), bar, True))
    return out


def worst(lines):
    """the lines folded by output name without its layer index: name -> (largest value / bar, value, bar)"""
    out = {}
    for name, value, bar, _ in lines:
        key = name.split("[")[0] + (" " + name.split("] ")[1] if "] " in name else "")
        q = value / bar if bar else (0.0 if value == 0 else float("inf"))
        if key not in out or q > out[key][0]:
            out[key] = (q, value, bar)
    return out
