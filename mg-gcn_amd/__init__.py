"""mg-gcn_amd -- MI355X-native engine for the MG-GCN hot path.

The directory name is not a Python identifier; load it with
``__graft_entry__.load_package()`` (registers it as ``mg_gcn_amd``).

Layout:
  csrc/        HIP kernels + the C ABI of include/mggcn.h  -> lib/libmggcn_hip.so
  host/        C++17 header layer with the reference's class names + the mg_gcn CLI
  _lib.py      ctypes binding (fails loudly when the engine is missing; no CPU path)
  matrix.py    context / csr_matrix / dn_matrix        (reference src/matrix.hpp)
  ops.py       matmul / get_matmul_buffer / kernels     (reference src/cuda_utils.hpp)
  gcn.py       sparse_linear / linear / gcn_layer / gcn (reference src/gcn.hpp); param_owner: one table row per trained
               tensor; layer_params: a layer's owners; model_base: the epoch gcn and gat share
  gat.py       attention / gat_layer / gat: graph attention layers, GAT and (variant="v2": attention_v2 / gatv2_layer)
               GATv2 and (variant="dot": attention_dot / gatdot_layer) dot-product attention; gated_skip: the skip
               connection and gate of skip="add" | "gate" (no reference counterpart); label_input: the table and lists of
               label_input=rate; attention_efeat: the attention of edge_attr=E (edge features in the score,
               csrc/gat_efeat.hip); attention_model: the dropouts and
               the export gat and dist_gat share
  sage.py      max_aggregate / sage_layer / sage: GraphSAGE with the mean (gcn's SpMM) or the max aggregator (csrc/agg_max.hip;
               no reference counterpart)
  edge_sample.py thresholds / sampled_csr / edge_sampler / sampling_option: the per-epoch edge sample of gat and sage(aggr="max"),
               drawn on the device (csrc/edge_sample.hip; no reference counterpart); rescaled_sampling_option: the sample
               with rescaled values of gcn and sage(aggr="mean") (edge_rescale=), multiplied by the row-split SpMM on a plan
               built on the device (csrc/spmm_dev.hip)
  label_mask.py  the host's restatement of the label-input mask: its count per epoch, without a synchronisation
  dist.py      1D row partition, one process per GPU    (reference src/dist_matrix.hpp, gcn.hpp dist_*); dist_model_base:
               the epoch dist_gcn and dist_gat share
  dist_gat.py  dist_attention / dist_gat_layer / dist_gat (and the _v2 / gatv2 twins): gat on the row partition (exported by dist)
  dist_sage.py dist_max_aggregate / dist_sage_layer / dist_sage: sage on the row partition, the max backward on a packed
               (arg, gradient) record (exported by dist)
  datasets.py  on-disk format + synthetic generators    (reference test/data/prep.py); the checkpoint file
  checkpoint.py  save / load / predict of gcn, dist_gcn, gat and dist_gat, named from the owners' tables (no reference
                 counterpart)
  selection.py   model_selector: best epoch on a split, early stopping
  metrics.py     roc_auc_evaluator: ROC-AUC per class and split of a multi-label model as exact integers, on a stable radix
                 sort on the device (csrc/radix_sort.hip, csrc/roc_auc.hip; no reference counterpart)
  smoothing.py   correct_and_smooth: label-propagation post-processing of any model's logits (csrc/propagate.hip around the
                 sweep SpMM; no reference counterpart)
"""
from . import _lib, datasets                                   # noqa: F401
from ._lib import engine_error                                  # noqa: F401
from . import matrix                                            # noqa: F401
from .matrix import context, csr_matrix, dn_matrix, host_scalars, matrix_error  # noqa: F401
from . import ops                                               # noqa: F401
from .ops import get_matmul_buffer, matmul                      # noqa: F401
from .gcn import (gcn, gcn_layer, linear, softmax, softmax_cross_entropy_loss,  # noqa: F401
                  sparse_linear)
from .gat import attention, attention_dot, attention_v2, gat, gat_layer, gatdot_layer, gated_skip, gatv2_layer, label_input  # noqa: F401

from .sage import max_aggregate, sage, sage_layer               # noqa: F401
from . import edge_sample                                       # noqa: F401
from .edge_sample import edge_sampler, sampled_csr              # noqa: F401

from . import dist                                              # noqa: F401
from .dist import (dist_context, dist_gcn, dist_gcn_layer, dist_row_csr_matrix,  # noqa: F401
                   dist_row_dn_matrix, dist_row_linear, dist_sparse_linear, repl_dn_matrix)

from . import checkpoint, selection                             # noqa: F401
from .selection import model_selector                           # noqa: F401
from . import metrics                                           # noqa: F401
from .metrics import roc_auc_evaluator                          # noqa: F401
from . import smoothing                                         # noqa: F401
from .smoothing import correct_and_smooth                       # noqa: F401

__all__ = ["context", "csr_matrix", "dn_matrix", "matrix_error", "engine_error", "ops", "matmul",
           "get_matmul_buffer", "sparse_linear", "linear", "gcn_layer", "softmax",
           "softmax_cross_entropy_loss", "gcn", "attention", "gat_layer", "gat", "attention_v2", "gatv2_layer", "attention_dot", "gatdot_layer", "gated_skip", "label_input", "sage", "sage_layer", "max_aggregate", "edge_sampler", "sampled_csr", "datasets", "model_selector", "correct_and_smooth", "roc_auc_evaluator"]
