"""gat(row_split=S) without a device: the refusals, each a ValueError naming row_split before the matrix is looked at, and the
default, which leaves the constructor taking every call it took."""
import inspect
from importlib import import_module

import numpy as np
import pytest

SIZES = [16, 32, 5]
BEFORE = ["self", "A", "sizes", "heads", "attn_slope", "loss", "fused", "weights", "dropout", "attn_dropout", "variant", "skip",
          "norm", "skip_weights", "label_input", "label_weights", "agg_dtype", "edge_attr", "edge_weights", "fanout", "edge_keep"]


@pytest.mark.parametrize("bad", [0, 32, 63, 96, 1000, -64, 64.0, "64", True])
def test_a_value_that_is_no_multiple_of_64_is_refused(pkg, bad):
    with pytest.raises(ValueError, match="row_split"):
        pkg.gat(None, SIZES, row_split=bad)


@pytest.mark.parametrize("more", [dict(variant="v2"), dict(variant="dot"), dict(agg_dtype="bf16"),
                                  dict(edge_attr=np.zeros((8, 3), dtype=np.float32))], ids=["v2", "dot", "bf16", "edge_attr"])
def test_options_without_split_kernels_are_refused(pkg, more):
    with pytest.raises(ValueError, match="row_split"):
        pkg.gat(None, SIZES, row_split=64, **more)


def test_the_default_is_off_and_the_signature_only_grew(pkg):
    gat = import_module(pkg.__name__ + ".gat")
    sig = inspect.signature(gat.gat.__init__).parameters
    assert list(sig) == BEFORE + ["row_split"] and sig["row_split"].default is None
    for variant in gat.VARIANTS:
        assert gat.check_row_split(None, variant, "bf16", object()) is None
    assert gat.attention.row_split is None and gat.attention._split(gat.attention, None, None) is None
    assert "row_split" not in inspect.signature(import_module(pkg.__name__ + ".dist").dist_gat.__init__).parameters
