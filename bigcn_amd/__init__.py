"""bigcn_amd - MI355X-native (gfx950) BiGCN bidirectional message-passing path.

Drop-in symbols for the reference's hot path (cwkd/BiGCN):

* ``GCNConv``       <- ``from torch_geometric.nn import GCNConv``   (BiGCN_Twitter.py:15)
* ``scatter_mean``  <- ``from torch_scatter import scatter_mean``   (BiGCN_Twitter.py:6)
* ``TDrumorGCN``, ``BUrumorGCN``, ``BiGCN`` (Twitter, 4 classes), ``Net`` (Weibo, 2 classes)
* ``EBGCN`` - the edge-enhanced model (model/Twitter/EBGCN.py): eval forward on the edge-inference
  kernel (``edge_infer``), reference checkpoints load strictly; ``EBGCN.train_forward`` is the
  reference's training forward with autograd, on ``edge_infer_train`` (the five per-edge networks
  with batch-statistics BatchNorm, the Bayesian branch, the KL edge loss and their backward) and
  ``ebgcn_conv2_lin_train`` (batch-statistics bn1 + relu + conv2's lin and their backward without the
  dense [N, 64 + F] concat) followed by ``gcn_aggregate`` (the aggregation half of ``gcn_conv``)
* ``EBGCNTrainStep`` - EBGCN's training-loop body (EBGCN.py:300-312) without a host sync: the training
  forward, the loss / accuracy / skip decision in one launch, backward, and ``MultiAdam`` (one launch for
  all 68 parameter tensors in the reference's five groups, ``ebgcn_adam``)
* ``explain`` / ``segment_rank`` - the reference's analysis (explain_PHEME.py): per-stage node sums and
  per-tree rankings of a whole batch, for ``BiGCN`` / ``Net`` / ``EBGCN`` in eval mode
* ``compare`` / ``tree_centrality`` / ``rank_similarity`` - the reference's comparison
  (compare_similarity.py): the trees' graph centralities and, per tree, five similarity statistics of
  every pair of rankings
* ``metrics`` - the reference's evaluation metrics (tools/evaluate.py): ``confusion`` counts labels against
  predictions on the device, ``class_metrics`` / ``evaluation4class`` / ``evaluationclass`` give the
  reference's numbers from the counts, ``EpochMetrics`` records a validation epoch without a host sync
  (``FusedTrainStep.validate`` is the reference's test loop around it)
* ``LSTM`` - the PHEME comparison's LSTM baseline (model/Twitter/LSTM_Twitter.py): a whole
  batch of trees per native call (``bgcn_lstm_eval``: one GEMM per layer for both directions' input
  projections, one launch per time step for every tree), reference checkpoints load strictly;
  ``LSTM.evaluate`` / ``LSTM.validate`` are the reference's test loop
* ``LSTMTrainStep`` / ``lstm_adam`` - the LSTM baseline's training-loop body (LSTM_Twitter.py:96-126):
  forward, loss and backpropagation through time as one native call (``bgcn_lstm_train_grad``,
  also ``LSTM.grad_batch``), then the reference's Adam as one ``MultiAdam`` launch
* ``TreeBERT`` - the comparison's BERT baseline (model/Twitter/BERT_Twitter.py) in eval mode: the
  class depends on each tree's first row only, so ``evaluate`` / ``validate`` are a chain of
  ``[B, hidden]`` GEMMs (``bgcn_bert_eval``, root-only form); ``explain_batch`` runs the full causal
  encoder with a two-pass MFMA attention kernel and ranks the hidden and attention sums per tree
* ``TreeBERTTrainStep`` / ``bert_adam`` - the BERT baseline's training-loop body (BERT_Twitter.py:89-119):
  the forward with ``BertModel``'s four dropout sites, the loss and the backward on the trees' root rows
  as one native call (``bgcn_bert_train_grad``, also ``TreeBERT.grad_batch``), then the reference's Adam
  as ``MultiAdam`` launches over slices of 128 tensors; ``gemm="skinny"`` runs the chain's products on the
  split fp32 kernels (``bgcn_bert_train_grad_skinny``; alone: ``ops.gemm_xwt_skinny`` / ``gemm_xw_skinny`` /
  ``gemm_tn_skinny``), which put a ``[B, hidden]`` product on 256 or more workgroups
* ``TweetEncoder`` - the step that makes ``data.x`` and ``data.cls`` (Process/getPHEMEgraph.py:104-118): a
  plain bidirectional ``BertModel`` over token ids as one native call per tree of tweets
  (``bgcn_bert_encode``: embeddings gathered by token id, unmasked MFMA attention with its K / V tiles
  staged in LDS, a last layer that runs on the ``[n, hidden]`` first rows only)
* ``FusedTrainStep`` - the training-loop body (BiGCN_Twitter.py:183-189) as one native call
  + the data-parallel all-reduce + fused Adam

all backed by hand-written HIP kernels in ``libbgcn.so`` (C ABI: ``include/bgcn.h``).
"""
from .bigcn import BiGCN, BUrumorGCN, Net, TDrumorGCN, make_optimizer
from .conv import GCNConv
from .compare import compare, rank_similarity, tree_centrality
from .ebgcn import EBGCN
from .explain import explain, segment_rank
from .lstm import LSTM, LSTMTrainStep, lstm_adam
from .bert import TreeBERT, TreeBERTTrainStep, TweetEncoder, bert_adam
from . import metrics
from .metrics import EpochMetrics, class_metrics, confusion, evaluation4class, evaluationclass
from .ops import (Graph, bigcn_encoder, build_graph, ebgcn_conv2_lin_train, edge_infer, edge_infer_train,
                  gcn_aggregate, gcn_conv, scatter_mean, spmm)
from .ops import drop_edges
from .optim import FusedAdam, MultiAdam, bigcn_adam, ebgcn_adam
from .ebgcn_step import EBGCNTrainStep
from .train import FusedTrainStep

__all__ = ["GCNConv", "scatter_mean", "TDrumorGCN", "BUrumorGCN", "BiGCN", "Net", "make_optimizer",
           "Graph", "build_graph", "gcn_conv", "spmm", "bigcn_encoder", "FusedAdam", "bigcn_adam",
           "FusedTrainStep", "EBGCN", "edge_infer", "edge_infer_train", "ebgcn_conv2_lin_train", "gcn_aggregate",
           "MultiAdam", "ebgcn_adam", "EBGCNTrainStep", "drop_edges",
           "explain", "segment_rank",
           "compare", "tree_centrality", "rank_similarity",
           "LSTM", "LSTMTrainStep", "lstm_adam", "TreeBERT", "TreeBERTTrainStep", "bert_adam",
           "TweetEncoder",
           "metrics", "confusion", "class_metrics", "evaluation4class", "evaluationclass", "EpochMetrics"]
__version__ = "0.1.0"
