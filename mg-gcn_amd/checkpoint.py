"""save / load / predict of gcn, dist.dist_gcn, gat.gat and dist_gat.dist_gat (opt-in; the reference writes nothing to disk).

The file is the one of datasets.write_checkpoint (INTEGRATION.md "Checkpoint file"): the model's configuration, every
parameter tensor, optionally Adam's moments and step count, and the dropout state (p, seed, epoch).  Execution options
(fused, agg_dtype, hoisting, the exchange schedule, P) are not model state and are not stored: weights are replicated and
the dropout masks are counter-based on (seed, epoch, global row, column), so a file written by one form loads into any
other and a resumed run draws the masks the uninterrupted run would have drawn.  The attention models store their layer
type with it (model, variant, heads, attn_slope, the attention dropout probability: version 3 of the file) and per layer
W, b and att; their two masks are counter-based on (seed, epoch * 64 + layer, ...), so the same holds for them.

Which tensors a model has, under which names and in which order, is not listed here: model_params reads it from the layers'
owners() and the owners' params_table (gcn.layer_params, gcn.param_owner), the tables Adam runs from.

Nothing here launches a new kernel: the tensors move through dn_matrix.init (host to device, in place), dn_matrix.zero and
dn_matrix.copy_to.  A model that never calls these members runs exactly what it ran before.
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np

from . import datasets, ops
from .matrix import dn_matrix


def raw_context(ctx):
    """the matrix.context behind a context or a dist.dist_context"""
    return getattr(ctx, "ctx", ctx)


def model_params(model) -> List[tuple]:
    """[(name, owner, parameter attribute, m attribute, v attribute)] in file order (datasets.checkpoint_tensors); the
    owner is the gcn.param_owner that holds the tensor, its Adam moments and its step count.  Nothing is listed here: a
    layer names its owners and their file prefixes (owners()), an owner its tensors (params_table), and a tensor's name
    is prefix + stem + layer index -- W0, b0, att0, res_W0, res_b0, gate0, gamma0, beta0 for a layer that has them all."""
    return [(f"{prefix}{stem}{l}", owner, p, m, v) for l, layer in enumerate(model.layers_)
            for prefix, owner in layer.owners() for stem, p, _, m, v, _ in owner.params_table]


def model_owners(model) -> list:
    """every param_owner of the model that holds a tensor: what carries Adam state"""
    return [p for layer in model.layers_ for p in layer.params()]


def reset_adam(model, ctx) -> None:
    """zero moments (allocated first where the model never stepped), step 0; stream-ordered"""
    rc = raw_context(ctx)
    for owner in model_owners(model):
        owner.adam_state(rc)
        owner.step = 0
    for _, owner, _, m, v in model_params(model):
        getattr(owner, m).zero(rc)
        getattr(owner, v).zero(rc)


def config_mismatch(file_cfg: dict, model_cfg: dict):
    """the first differing field as "<field>: file <x>, model <y>", or None.  The layer type comes first: a gcn
    configuration has no "model" key and counts as "gcn", and has none of variant, heads and attn_slope"""
    defaults = {"model": "gcn"}
    for key in ("model", "variant", "sizes", "heads", "attn_slope", "residual_layer", "norm", "loss"):
        f, m = file_cfg.get(key, defaults.get(key)), model_cfg.get(key, defaults.get(key))
        if f != m:
            return f"{key}: file {f}, model {m}"
    return None


class checkpoint_option:
    """save / load / predict of gcn, dist.dist_gcn, gat.gat and dist_gat.dist_gat.  ``ctx`` is what the model's other
    members take: a context, or the rank's dist_context -- every rank of a dist_gcn or dist_gat calls save and load (rank 0
    alone writes, every rank reads) and predict returns the rank's rows."""

    def checkpoint_config(self) -> dict:
        cfg = {"sizes": [int(s) for s in self.sizes], "residual_layer": bool(getattr(self, "residual_layer", False)),
               "norm": getattr(self, "norm", None), "loss": self.loss,
               "dropout": (self.dropout_p, self.dropout_seed, self.dropout_epoch)}
        if hasattr(self, "variant"):                            # gat, dist_gat: the layer type (version 3 of the file)
            cfg.update(model="gat", variant=self.variant, heads=[int(h) for h in self.heads],
                       attn_slope=float(self.attn_slope), attn_dropout=float(self.attn_dropout_p))
        return cfg

    def _write_checkpoint(self, ctx, path: str, tensors: Dict[str, np.ndarray], optimizer: bool, step: int) -> None:
        """rank 0 writes; the others leave once the file is complete"""
        if getattr(ctx, "rank", 0) == 0 or not hasattr(ctx, "P"):
            datasets.write_checkpoint(path, dict(self.checkpoint_config(), optimizer=optimizer, step=step), tensors)
        if getattr(ctx, "P", 1) > 1:
            ctx.host_all_reduce(np.zeros(1, dtype=np.int64))

    def save(self, ctx, path: str, optimizer: bool = True) -> None:
        """Writes the parameters, the dropout state and (``optimizer``) Adam's moments and step count.  A model that has
        not stepped yet stores zero moments and step 0."""
        ctx.sync()
        tensors, steps = {}, set()
        for name, owner, p, m, v in model_params(self):
            tensors[name] = getattr(owner, p).numpy()
            if optimizer:
                stepped = getattr(owner, m) is not None
                steps.add(int(owner.step) if stepped else 0)
                tensors["m." + name] = getattr(owner, m).numpy() if stepped else np.zeros_like(tensors[name])
                tensors["v." + name] = getattr(owner, v).numpy() if stepped else np.zeros_like(tensors[name])
        if len(steps) > 1:
            raise ValueError(f"the model's tensors disagree on Adam's step count: {sorted(steps)}")
        self._write_checkpoint(ctx, path, tensors, bool(optimizer), steps.pop() if steps else 0)

    def load(self, ctx, path: str) -> None:
        """Reads ``path`` into this model, in place: the parameter and moment buffers keep their addresses (the fused Adam
        table holds raw pointers).  ValueError naming the first differing field of the configuration -- model,
        variant, sizes, heads, attn_slope, residual_layer, norm, loss -- before anything is written or stored.  A file
        without the optimiser section resets Adam (zero moments, step 0).  Restores every step count and calls set_dropout
        with the file's (p, seed, epoch), and the file's attention dropout probability on an attention model."""
        cfg, tensors = datasets.read_checkpoint(path)
        bad = config_mismatch(cfg, self.checkpoint_config())
        if bad is not None:
            raise ValueError(f"{path}: {bad}")
        attn = {"attn": cfg["attn_dropout"]} if "attn_dropout" in cfg else {}
        self.set_dropout(*cfg["dropout"], **attn)               # host state; its own refusals come before any device write
        rc = raw_context(ctx)
        for owner in model_owners(self):
            owner.adam_state(rc)                                # a model that never stepped: allocate (and zero) first
        ctx.sync()                                              # dn_matrix.init copies on torch's stream, then synchronises
        for name, owner, p, m, v in model_params(self):
            getattr(owner, p).init(tensors[name])
            if cfg["optimizer"]:
                getattr(owner, m).init(tensors["m." + name])
                getattr(owner, v).init(tensors["v." + name])
            else:
                getattr(owner, m).zero(rc)
                getattr(owner, v).zero(rc)
        for owner in model_owners(self):
            owner.step = int(cfg["step"])
        ctx.sync()

    def predict(self, ctx, X) -> np.ndarray:
        """Host int32 predictions of a plain forward (it never drops): [n x 1] argmax, the first maximum winning
        (ops.max_row_indices), or [n x C] 0 / 1 for logit > 0 with loss="bce".  dist_gcn, dist_gat: the rank's rows."""
        rc = raw_context(ctx)
        out = self(ctx, X)
        out = getattr(out, "local", out)
        if self.loss == "bce":
            ctx.sync()
            return (out.numpy() > 0).astype(np.int32)
        P = dn_matrix(out.n(), 1, dtype=np.int32, device=rc.device)
        ops.max_row_indices(rc, out, P)
        ctx.sync()
        return P.numpy()
