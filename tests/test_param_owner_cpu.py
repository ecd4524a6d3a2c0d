"""Every trained tensor is described once, in its owner's gcn.param_owner table: the names in the checkpoint file and the
rows of Adam's table are both read from it.  No device: the owners and layers are built with __new__ and hold stand-in
tensors, as the neighbouring CPU tests do."""
from importlib import import_module

import pytest

# file-name stem -> decays like W: what the checkpoint file and Adam have always done (INTEGRATION.md "Checkpoint file")
DECAYS = {"W": True, "b": False, "gamma": False, "beta": False, "att": True, "gate": True}
# owner class -> (layer class, the layer's attribute, its file-name prefix) for every place an owner can sit
SLOTS = [("gcn.linear", "gcn.layer_body", "lin", ""), ("gcn.linear", "gcn.layer_body", "res_lin", "res_"),
         ("gcn.layer_norm", "gcn.layer_body", "norm", ""),
         ("gcn.linear", "gat.gat_layer", "lin", ""), ("gat.attention", "gat.gat_layer", "attn", ""),
         ("gat.attention_v2", "gat.gatv2_layer", "attn", ""), ("gat.attention_dot", "gat.gatdot_layer", "attn", ""),
         ("gcn.linear", "gat.gat_layer", "res_lin", "res_"), ("gat.gated_skip", "gat.gat_layer", "gate", ""),
         ("gcn.layer_norm", "gat.gat_layer", "norm", ""),
         ("dist.dist_row_linear", "dist.dist_gcn_layer", "lin", ""), ("dist_gat.dist_attention", "dist_gat.dist_gat_layer", "attn", ""),
         ("dist_gat.dist_attention_v2", "dist_gat.dist_gatv2_layer", "attn", "")]


def _get(pkg, dotted):
    module, name = dotted.split(".")
    return getattr(import_module(pkg.__name__ + "." + module), name)


def _subclasses(cls):
    return {s for c in cls.__subclasses__() for s in {c} | _subclasses(c)}


def _owner(cls):
    """an instance without __init__ whose parameter, gradient and moments are distinct stand-ins"""
    owner = cls.__new__(cls)
    for row in cls.params_table:
        for attr in row[1:5]:
            setattr(owner, attr, object())
    return owner


def test_every_owner_class_sits_in_a_slot(pkg):
    """a new param_owner has to be given a slot here, so the two tests below see it"""
    for module in ("gat", "dist", "dist_gat"):
        import_module(pkg.__name__ + "." + module)
    assert _subclasses(_get(pkg, "gcn.param_owner")) == {_get(pkg, owner) for owner, *_ in SLOTS}


@pytest.mark.parametrize("owner,layer,attr,prefix", SLOTS)
def test_file_names_are_the_table_stems_with_prefix_and_index(pkg, owner, layer, attr, prefix):
    checkpoint = import_module(pkg.__name__ + ".checkpoint")
    layers = []
    for _ in range(3):                                       # the owner under test alone in its slot, in three layers
        l = _get(pkg, layer).__new__(_get(pkg, layer))
        l.lin = l.attn = l.res_lin = l.gate = l.norm = None
        setattr(l, attr, _owner(_get(pkg, owner)))
        layers.append(l)
    rows = checkpoint.model_params(type("m", (), {"layers_": layers})())
    table = _get(pkg, owner).params_table
    assert [name for name, *_ in rows] == [f"{prefix}{stem}{k}" for k in range(3) for stem, *_ in table]
    assert [(o, p, m, v) for _, o, p, m, v in rows] == [(getattr(l, attr), p, m, v) for l in layers for _, p, _, m, v, _ in table]
    assert [l.params() for l in layers] == [[getattr(l, attr)] if table else [] for l in layers]
    assert all(stem in DECAYS for stem, *_ in table)


@pytest.mark.parametrize("owner", sorted({owner for owner, *_ in SLOTS}))
def test_adam_tensors_decay_exactly_the_rows_marked(pkg, owner):
    cls = _get(pkg, owner)
    o = _owner(cls)
    wd = 5e-4
    rows = o.adam_tensors(wd)
    assert len(rows) == len(cls.params_table)
    for (p, g, m, v, decay), (stem, pa, ga, ma, va, decays) in zip(rows, cls.params_table):
        assert (p, g, m, v) == (getattr(o, pa), getattr(o, ga), getattr(o, ma), getattr(o, va))
        assert decays is DECAYS[stem]
        assert decay == (wd if decays else 0.0) and type(decay) is float
    assert [r[4] for r in o.adam_tensors(0.0)] == [0.0] * len(rows)


def test_a_full_layer_of_each_kind_in_file_order(pkg):
    """gcn's layer: W, b, res_W, res_b, gamma, beta; an attention layer: W, b, att, res_W, res_b, gate, gamma, beta"""
    checkpoint = import_module(pkg.__name__ + ".checkpoint")
    body = _get(pkg, "gcn.layer_body").__new__(_get(pkg, "gcn.layer_body"))
    body.lin, body.res_lin, body.norm = (_owner(_get(pkg, c)) for c in ("gcn.linear", "gcn.linear", "gcn.layer_norm"))
    att = _get(pkg, "gat.gat_layer").__new__(_get(pkg, "gat.gat_layer"))
    att.lin, att.attn, att.res_lin, att.gate, att.norm = (
        _owner(_get(pkg, c)) for c in ("gcn.linear", "gat.attention", "gcn.linear", "gat.gated_skip", "gcn.layer_norm"))
    names = [name for name, *_ in checkpoint.model_params(type("m", (), {"layers_": [body, att]})())]
    assert names == ["W0", "b0", "res_W0", "res_b0", "gamma0", "beta0",
                     "W1", "b1", "att1", "res_W1", "res_b1", "gate1", "gamma1", "beta1"]
    assert body.params() == [body.lin, body.res_lin, body.norm]
    assert att.params() == [att.lin, att.attn, att.res_lin, att.gate, att.norm]
