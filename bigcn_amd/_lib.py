"""ctypes binding of ``libbgcn.so`` (the C ABI declared in ``include/bgcn.h``).

The library is built in-tree (``make -C bigcn_amd/csrc`` or ``__graft_entry__.build()``)
and linked against ``libamdhip64.so.7`` by SONAME, so inside a PyTorch process it
shares the HIP runtime torch already loaded (same streams, same device memory).

There is deliberately no fallback: if the library is missing or no ROCm device is
present, every op raises.  The oracle under ``oracle/`` is test infrastructure and
is never imported from here.
"""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import (POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t,
                    c_uint64, c_void_p)

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BGCN_LIB", os.path.join(_HERE, "libbgcn.so"))

BGCN_DEGREE_ON_COL = 0
BGCN_DEGREE_ON_ROW = 1
BGCN_EPI_NONE = 0
BGCN_EPI_RELU = 1
BGCN_FEAT_AUTO = 0
BGCN_FEAT_DENSE = 1
BGCN_FEAT_SPARSE = 2
BGCN_SPARSE_CAP = 32
BGCN_SPARSE_SPILL_PER_ROW = 32   # spill pool capacity per row (rows over the ELL cap)
BGCN_DTYPE_F32 = 0
BGCN_DTYPE_BF16 = 1
ABI_VERSION = 12   # BGCN_ABI_VERSION of include/bgcn.h
BGCN_STATUS_CROSS_TREE = 16
BGCN_EDGE_INFER_TILE = 32   # edges per workgroup of bgcn_edge_infer
BGCN_SEGMENT_RANK_LDS = 4096   # longest segment bgcn_segment_rank sorts in LDS
BGCN_TREE_CENTRALITY_LDS = 2048   # longest tree bgcn_tree_centrality keeps in LDS
BGCN_RANK_SIMILARITY_MAX = 32   # most rankings, and the largest k, of bgcn_rank_similarity
BGCN_STATUS_TWO_PARENTS = 32
BGCN_STATUS_CYCLE = 64
BGCN_STATUS_BATCH_UNSORTED = 128   # bgcn_ebgcn_eval_step: the batch vector is not sorted (information)
BGCN_STATUS_SEQUENCE = 256   # bgcn_lstm_eval: a bad sequence start, a sequence over max_len, a bad label
BGCN_LSTM_SEQ_TILE = 32   # sequences per workgroup of a step launch of bgcn_lstm_eval
BGCN_LSTM_MAX_LAYERS = 4
BGCN_BERT_MAX_LAYERS = 24
BGCN_BERT_QUERY_TILE = 32   # queries per workgroup of bgcn_bert_eval's attention kernel
BGCN_STATUS_TOKEN = 512   # bgcn_bert_encode: a token id outside [0, vocab)

# every symbol include/bgcn.h declares (checked by tests/test_capi.py)
EXPORTED_SYMBOLS = (
    "bgcn_abi_version", "bgcn_last_error",
    "bgcn_graph_workspace_size", "bgcn_build_graph", "bgcn_graph_dinv",
    "bgcn_edge_weight_grad_workspace_size", "bgcn_edge_weight_grad",
    "bgcn_graph_pair_workspace_size", "bgcn_build_graph_pair", "bgcn_graph_pair_plans",
    "bgcn_spmm_workspace_size", "bgcn_spmm",
    "bgcn_gemm_xwt", "bgcn_gemm_xw", "bgcn_gemm_tn_workspace_size", "bgcn_gemm_tn",
    "bgcn_colsum_workspace_size", "bgcn_colsum",
    "bgcn_scatter_mean_workspace_size", "bgcn_scatter_mean_fwd", "bgcn_scatter_mean_bwd",
    "bgcn_head_forward", "bgcn_head_backward",
    "bgcn_drop_edges_workspace_size", "bgcn_drop_edges",
    "bgcn_bigcn_workspace_size", "bgcn_bigcn_forward", "bgcn_bigcn_backward",
    "bgcn_keep_words", "bgcn_set_kernel_timing", "bgcn_kernel_timing", "bgcn_kernel_span", "bgcn_adam_step",
    "bgcn_prepare_workspace_size", "bgcn_prepare_batch", "bgcn_csr_to_dense",
    "bgcn_train_step_workspace_size", "bgcn_train_step", "bgcn_train_step_dw1", "bgcn_join_side",
    "bgcn_weight_images_size", "bgcn_train_step_saved", "bgcn_eval_step",
    "bgcn_loader_create", "bgcn_loader_slot_bytes", "bgcn_loader_len", "bgcn_loader_next", "bgcn_loader_destroy",
    "bgcn_loader_wait", "bgcn_loader_get_stats",
    "bgcn_bn_fold", "bgcn_edge_infer", "bgcn_ebgcn_conv2_lin_workspace_size", "bgcn_ebgcn_conv2_lin",
    "bgcn_explain_sums_workspace_size", "bgcn_explain_sums", "bgcn_segment_rank_workspace_size", "bgcn_segment_rank",
    "bgcn_tree_centrality_workspace_size", "bgcn_tree_centrality", "bgcn_rank_similarity_workspace_size",
    "bgcn_rank_similarity", "bgcn_confusion",
    "bgcn_ebgcn_eval_workspace_size", "bgcn_ebgcn_eval_step", "bgcn_ebgcn_eval_saved",
    "bgcn_edge_infer_train_workspace_size", "bgcn_edge_infer_train_fwd", "bgcn_edge_infer_train_bwd",
    "bgcn_ebgcn_conv2_lin_train_workspace_size", "bgcn_ebgcn_conv2_lin_train_fwd", "bgcn_ebgcn_conv2_lin_train_bwd",
    "bgcn_adam_multi_table_size", "bgcn_adam_multi_plan", "bgcn_adam_multi_step", "bgcn_ebgcn_train_loss",
    "bgcn_lstm_workspace_size", "bgcn_lstm_eval", "bgcn_lstm_train_workspace_size", "bgcn_lstm_train_grad",
    "bgcn_bert_workspace_size", "bgcn_bert_eval", "bgcn_bert_train_workspace_size", "bgcn_bert_train_grad",
    "bgcn_w16_image_size", "bgcn_w16_pack", "bgcn_gemm_xwt_w16_workspace_size", "bgcn_gemm_xwt_w16",
    "bgcn_bert_w16_workspace_size", "bgcn_bert_eval_w16",
    "bgcn_gemm_skinny_workspace_size", "bgcn_gemm_xwt_skinny", "bgcn_gemm_xw_skinny", "bgcn_gemm_tn_skinny",
    "bgcn_bert_train_skinny_workspace_size", "bgcn_bert_train_grad_skinny",
    "bgcn_bert_encode_workspace_size", "bgcn_bert_encode",
)

BGCN_ADAM_MULTI_MAX_TENSORS = 128
BGCN_ADAM_MULTI_MAX_GROUPS = 8
BGCN_ADAM_MULTI_CHUNK = 1024   # elements per workgroup of bgcn_adam_multi_step


class AdamMultiTensor(Structure):
    """bgcn_adam_multi_tensor (include/bgcn.h): one entry of the many-tensor Adam's table."""
    _fields_ = [("param", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p), ("numel", c_int64),
                ("first_block", c_int64), ("group", c_int32), ("reserved", c_int32)]


class AdamMultiArgs(Structure):
    """bgcn_adam_multi_args (include/bgcn.h)."""
    _fields_ = [("table", c_void_p), ("count", c_int32), ("blocks", c_int64),
                ("grad", c_void_p * BGCN_ADAM_MULTI_MAX_TENSORS), ("lr", c_float * BGCN_ADAM_MULTI_MAX_GROUPS),
                ("beta1", c_float), ("beta2", c_float), ("eps", c_float), ("weight_decay", c_float),
                ("bias_correction1", c_float), ("bias_correction2_sqrt", c_float), ("grad_scale", c_float),
                ("skip_flag", c_void_p), ("skip_count", c_void_p)]


class SpmmPlan(Structure):
    """bgcn_spmm_plan (include/bgcn.h)."""
    _fields_ = [("bnd", c_void_p), ("longs", c_void_p), ("nlong", c_void_p)]


class GraphView(Structure):
    _fields_ = [
        ("t_ptr", c_void_p), ("t_row", c_void_p), ("t_col", c_void_p), ("t_w", c_void_p),
        ("s_ptr", c_void_p), ("s_row", c_void_p), ("s_col", c_void_p), ("s_w", c_void_p),
        ("capacity", c_int64), ("plan", SpmmPlan * 2), ("tree_status", c_void_p),
    ]


class CsrOut(Structure):
    _fields_ = [
        ("t_ptr", c_void_p), ("t_row", c_void_p), ("t_col", c_void_p), ("t_w", c_void_p),
        ("s_ptr", c_void_p), ("s_row", c_void_p), ("s_col", c_void_p), ("s_w", c_void_p),
    ]


class BiGCNArgs(Structure):
    _fields_ = [
        ("x", c_void_p), ("ldx", c_int64), ("num_nodes", c_int64), ("num_graphs", c_int64),
        ("in_feats", c_int64), ("hid", c_int64), ("batch", c_void_p), ("rootindex", c_void_p),
        ("td", GraphView), ("bu", GraphView),
        ("td_w1", c_void_p), ("td_b1", c_void_p), ("td_w2", c_void_p), ("td_b2", c_void_p),
        ("bu_w1", c_void_p), ("bu_b1", c_void_p), ("bu_w2", c_void_p), ("bu_b2", c_void_p),
        ("training", c_int), ("seed", c_uint64), ("keep_words", c_void_p),
        ("feat_mode", c_int), ("x_flags", c_void_p), ("x_nnz", c_void_p), ("x_cols", c_void_p),
        ("x_vals", c_void_p),
        ("tree_ptr", c_void_p), ("h1", c_void_p), ("h2", c_void_p), ("head_in", c_void_p),
        ("dhead_in", c_void_p),
        ("td_dw1", c_void_p), ("td_db1", c_void_p), ("td_dw2", c_void_p), ("td_db2", c_void_p),
        ("bu_dw1", c_void_p), ("bu_db1", c_void_p), ("bu_dw2", c_void_p), ("bu_db2", c_void_p),
        ("save_for_backward", c_int32), ("x_dtype", c_int32),
        ("prepared", c_void_p), ("prepared_bytes", c_size_t),
        ("td_num_edges", c_int64), ("bu_num_edges", c_int64),
    ]


BGCN_STEP_PARAMS = 10


class BatchDesc(Structure):
    """bgcn_batch (include/bgcn.h)."""
    _fields_ = [
        ("x", c_void_p), ("ldx", c_int64), ("num_nodes", c_int64), ("num_graphs", c_int64),
        ("batch", c_void_p), ("rootindex", c_void_p),
        ("td_edge_index", c_void_p), ("td_num_edges", c_int64),
        ("bu_edge_index", c_void_p), ("bu_num_edges", c_int64),
        ("td_droprate", c_double), ("bu_droprate", c_double), ("drop_seed", c_uint64),
        ("x_dtype", c_int32),
        ("x_row_ptr", c_void_p), ("x_col", c_void_p), ("x_val", c_void_p),
    ]


class StepArgs(Structure):
    """bgcn_step_args (include/bgcn.h)."""
    _fields_ = [
        ("cur", BatchDesc), ("in_feats", c_int64), ("num_classes", c_int64), ("y", c_void_p),
        ("degree_on", c_int32), ("training", c_int32), ("seed", c_uint64), ("feat_mode", c_int32),
        ("params", c_void_p * BGCN_STEP_PARAMS), ("grads", c_void_p * BGCN_STEP_PARAMS),
        ("loss", c_void_p), ("logp", c_void_p), ("status", c_void_p),
        ("prepared", c_void_p), ("prepared_bytes", c_size_t), ("prepared_ready", c_int32),
        ("next", POINTER(BatchDesc)), ("next_prepared", c_void_p), ("next_prepared_bytes", c_size_t),
        ("status_flag", c_void_p),
        ("images", c_void_p), ("images_current", c_int32),
        ("status_seen", c_void_p),
        ("defer_dw1", c_int32),
        ("adam", c_void_p),
    ]


class EbgcnDir(Structure):
    """bgcn_ebgcn_dir (include/bgcn.h): one direction's parameters."""
    _fields_ = [
        ("conv1_w", c_void_p), ("conv1_b", c_void_p), ("conv2_w", c_void_p), ("conv2_b", c_void_p),
        ("bn1_weight", c_void_p), ("bn1_bias", c_void_p), ("bn1_mean", c_void_p), ("bn1_var", c_void_p),
        ("sim_conv_w", c_void_p),
        ("sim_norm_weight", c_void_p), ("sim_norm_bias", c_void_p), ("sim_norm_mean", c_void_p),
        ("sim_norm_var", c_void_p),
        ("sim_out_w", c_void_p), ("sim_out_b", c_void_p), ("fc1_w", c_void_p),
        ("bn1_eps", c_float), ("sim_norm_eps", c_float), ("infer", c_int32),
    ]


class EbgcnEvalArgs(Structure):
    """bgcn_ebgcn_eval_args (include/bgcn.h)."""
    _fields_ = [
        ("batch", BatchDesc), ("td", EbgcnDir), ("bu", EbgcnDir), ("fc_w", c_void_p), ("fc_b", c_void_p),
        ("in_feats", c_int64), ("num_classes", c_int64), ("edge_num", c_int32), ("degree_on", c_int32),
        ("y", c_void_p), ("logp", c_void_p), ("loss", c_void_p), ("correct", c_void_p), ("pred", c_void_p),
        ("td_edge_pred", c_void_p), ("bu_edge_pred", c_void_p), ("status", c_void_p),
    ]


class EbgcnEvalView(Structure):
    """bgcn_ebgcn_eval_view (include/bgcn.h)."""
    _fields_ = [("t_ptr", c_void_p), ("t_col", c_void_p), ("t_w", c_void_p), ("t_w2", c_void_p), ("slot", c_void_p)]


class LstmArgs(Structure):
    """bgcn_lstm_args (include/bgcn.h)."""
    _fields_ = [
        ("x", c_void_p), ("ldx", c_int64), ("num_nodes", c_int64), ("in_feats", c_int64), ("hid", c_int64),
        ("num_layers", c_int64), ("out_feats", c_int64),
        ("seq_start", c_void_p), ("num_seqs", c_int64), ("max_len", c_int64),
        ("w_ih", (c_void_p * 2) * BGCN_LSTM_MAX_LAYERS), ("w_hh", (c_void_p * 2) * BGCN_LSTM_MAX_LAYERS),
        ("fc_w", c_void_p), ("fc_b", c_void_p), ("y", c_void_p),
        ("logp", c_void_p), ("h_n", c_void_p), ("out", c_void_p), ("loss", c_void_p), ("correct", c_void_p),
        ("pred", c_void_p), ("status", c_void_p),
    ]


class LstmTrainArgs(Structure):
    """bgcn_lstm_train_args (include/bgcn.h)."""
    _fields_ = [
        ("fwd", LstmArgs),
        ("d_w_ih", (c_void_p * 2) * BGCN_LSTM_MAX_LAYERS), ("d_w_hh", (c_void_p * 2) * BGCN_LSTM_MAX_LAYERS),
        ("d_fc_w", c_void_p), ("d_fc_b", c_void_p), ("dx", c_void_p), ("skip_flag", c_void_p),
    ]


class BertLayer(Structure):
    """bgcn_bert_layer (include/bgcn.h): one encoder layer's weights, in the header's order."""
    _fields_ = [(n, c_void_p) for n in ("q_w", "q_b", "k_w", "k_b", "v_w", "v_b", "ao_w", "ao_b", "ao_ln_w", "ao_ln_b",
                                        "i_w", "i_b", "o_w", "o_b", "o_ln_w", "o_ln_b")]


class BertArgs(Structure):
    """bgcn_bert_args (include/bgcn.h)."""
    _fields_ = [
        ("x", c_void_p), ("ldx", c_int64), ("num_nodes", c_int64), ("seq_start", c_void_p), ("num_seqs", c_int64),
        ("hidden", c_int64), ("heads", c_int64), ("intermediate", c_int64), ("num_layers", c_int64),
        ("max_pos", c_int64), ("out_feats", c_int64), ("ln_eps", c_float), ("reserved", c_int32),
        ("pos_emb", c_void_p), ("type_emb", c_void_p), ("emb_ln_w", c_void_p), ("emb_ln_b", c_void_p),
        ("layer", BertLayer * BGCN_BERT_MAX_LAYERS),
        ("pooler_w", c_void_p), ("pooler_b", c_void_p), ("fc_w", c_void_p), ("fc_b", c_void_p), ("y", c_void_p),
        ("logp", c_void_p), ("loss", c_void_p), ("correct", c_void_p), ("pred", c_void_p),
        ("hidden_out", c_void_p), ("hidden_sum", c_void_p), ("attn_sum", c_void_p), ("status", c_void_p),
    ]


class BertEncodeArgs(Structure):
    """bgcn_bert_encode_args (include/bgcn.h)."""
    _fields_ = [
        ("input_ids", c_void_p), ("num_seqs", c_int64), ("seq_len", c_int64), ("vocab", c_int64),
        ("hidden", c_int64), ("heads", c_int64), ("intermediate", c_int64), ("num_layers", c_int64),
        ("max_pos", c_int64), ("ln_eps", c_float), ("reserved", c_int32),
        ("word_emb", c_void_p), ("pos_emb", c_void_p), ("type_emb", c_void_p), ("emb_ln_w", c_void_p),
        ("emb_ln_b", c_void_p),
        ("layer", BertLayer * BGCN_BERT_MAX_LAYERS),
        ("pooler_w", c_void_p), ("pooler_b", c_void_p), ("embeddings", c_void_p), ("ld_embeddings", c_int64),
        ("cls", c_void_p), ("hidden_out", c_void_p), ("status", c_void_p),
        ("last_layer_full", c_int32), ("embed_only", c_int32),
    ]


class BertW16Args(Structure):
    """bgcn_bert_w16_args (include/bgcn.h): ``base`` and the weight images of the root-only chain."""
    _fields_ = [
        ("base", BertArgs),
        ("v_w16", c_void_p * BGCN_BERT_MAX_LAYERS), ("ao_w16", c_void_p * BGCN_BERT_MAX_LAYERS),
        ("i_w16", c_void_p * BGCN_BERT_MAX_LAYERS), ("o_w16", c_void_p * BGCN_BERT_MAX_LAYERS),
        ("pooler_w16", c_void_p),
    ]


class BertTrainArgs(Structure):
    """bgcn_bert_train_args (include/bgcn.h): ``fwd``, one gradient pointer per weight pointer of
    ``fwd`` (the eight top-level ones, then ``d_layer``), ``dx``, the skip flag and the dropout draw."""
    _fields_ = [
        ("fwd", BertArgs),
        ("d_pos_emb", c_void_p), ("d_type_emb", c_void_p), ("d_emb_ln_w", c_void_p), ("d_emb_ln_b", c_void_p),
        ("d_pooler_w", c_void_p), ("d_pooler_b", c_void_p), ("d_fc_w", c_void_p), ("d_fc_b", c_void_p),
        ("d_layer", BertLayer * BGCN_BERT_MAX_LAYERS),
        ("dx", c_void_p), ("skip_flag", c_void_p), ("drop_seed", c_uint64),
        ("hidden_dropout", c_float), ("attn_dropout", c_float),
    ]


class EdgeNet(Structure):
    """bgcn_edge_net (include/bgcn.h): one per-edge network."""
    _fields_ = [("conv_w", c_void_p), ("norm_weight", c_void_p), ("norm_bias", c_void_p), ("out_w", c_void_p),
                ("out_b", c_void_p), ("eps", c_float)]


class EdgeTrainFwdArgs(Structure):
    """bgcn_edge_train_fwd_args (include/bgcn.h)."""
    _fields_ = [
        ("h", c_void_p), ("ldh", c_int64), ("num_nodes", c_int64), ("hid", c_int64),
        ("edge_index", c_void_p), ("num_edges", c_int64), ("net", EdgeNet * 5),
        ("fc1_w", c_void_p), ("fc2_w", c_void_p), ("edge_num", c_int32), ("noise", c_void_p),
        ("edge_pred", c_void_p), ("edge_loss", c_void_p), ("s", c_void_p), ("p", c_void_p), ("p_y", c_void_p),
        ("sim_mean", c_void_p), ("sim_rstd", c_void_p), ("num_valid", c_void_p),
        ("batch_mean", c_void_p), ("batch_var", c_void_p), ("status", c_void_p),
    ]


class EdgeTrainBwdArgs(Structure):
    """bgcn_edge_train_bwd_args (include/bgcn.h)."""
    _fields_ = [
        ("h", c_void_p), ("ldh", c_int64), ("num_nodes", c_int64), ("hid", c_int64),
        ("edge_index", c_void_p), ("num_edges", c_int64), ("sim", EdgeNet),
        ("fc1_w", c_void_p), ("edge_num", c_int32),
        ("s", c_void_p), ("p", c_void_p), ("p_y", c_void_p), ("sim_mean", c_void_p), ("sim_rstd", c_void_p),
        ("num_valid", c_void_p), ("d_pred", c_void_p), ("d_loss", c_void_p),
        ("d_h", c_void_p), ("ldd", c_int64),
        ("d_conv_w", c_void_p), ("d_norm_weight", c_void_p), ("d_norm_bias", c_void_p),
        ("d_out_w", c_void_p), ("d_out_b", c_void_p), ("d_fc1_w", c_void_p),
    ]


class Conv2LinTrainFwdArgs(Structure):
    """bgcn_conv2_lin_train_fwd_args (include/bgcn.h)."""
    _fields_ = [
        ("h1", c_void_p), ("ldh", c_int64), ("x", c_void_p), ("ldx", c_int64),
        ("batch", c_void_p), ("rootindex", c_void_p),
        ("num_nodes", c_int64), ("num_graphs", c_int64), ("in_feats", c_int64), ("hid", c_int64),
        ("w2", c_void_p), ("gamma", c_void_p), ("beta", c_void_p), ("eps", c_float),
        ("z2", c_void_p), ("ldz", c_int64), ("batch_mean", c_void_p), ("batch_var", c_void_p),
        ("bn_g", c_void_p), ("bn_t", c_void_p), ("a_x", c_void_p),
        ("tree_count", c_void_p), ("num_valid", c_void_p), ("status", c_void_p),
    ]


class Conv2LinTrainBwdArgs(Structure):
    """bgcn_conv2_lin_train_bwd_args (include/bgcn.h)."""
    _fields_ = [
        ("dz2", c_void_p), ("lddz", c_int64), ("h1", c_void_p), ("ldh", c_int64), ("x", c_void_p), ("ldx", c_int64),
        ("batch", c_void_p), ("rootindex", c_void_p),
        ("num_nodes", c_int64), ("num_graphs", c_int64), ("in_feats", c_int64), ("hid", c_int64),
        ("w2", c_void_p), ("eps", c_float), ("batch_mean", c_void_p), ("batch_var", c_void_p),
        ("bn_g", c_void_p), ("bn_t", c_void_p), ("a_x", c_void_p), ("tree_count", c_void_p), ("num_valid", c_void_p),
        ("dh1", c_void_p), ("ldd", c_int64), ("dw2", c_void_p), ("dgamma", c_void_p), ("dbeta", c_void_p),
    ]


_SIGS = {
    "bgcn_abi_version": (c_int, []),
    "bgcn_last_error": (c_char_p, []),
    "bgcn_graph_workspace_size": (c_size_t, [c_int64, c_int64]),
    "bgcn_build_graph": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int,
                                 c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_graph_pair_workspace_size": (c_size_t, [c_int64, c_int64, c_int64]),
    "bgcn_graph_dinv": (c_int, [c_void_p, c_size_t, c_int64, c_int64, POINTER(c_void_p)]),
    "bgcn_edge_weight_grad_workspace_size": (c_size_t, [c_int64]),
    "bgcn_edge_weight_grad": (c_int, [c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_build_graph_pair": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int,
                                      POINTER(CsrOut), POINTER(CsrOut), c_void_p, c_void_p, c_void_p,
                                      c_size_t, c_void_p]),
    "bgcn_spmm_workspace_size": (c_size_t, [c_int64, c_int32]),
    "bgcn_spmm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                          c_int64, c_void_p, c_int64, c_int32, c_void_p, c_int, c_void_p,
                          c_size_t, c_void_p]),
    "bgcn_gemm_xwt": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                              c_int64, c_int64, c_int64, c_int64, c_void_p]),
    "bgcn_gemm_xw": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                             c_int64, c_int64, c_void_p]),
    "bgcn_gemm_tn_workspace_size": (c_size_t, [c_int64, c_int64, c_int64]),
    "bgcn_gemm_tn": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                             c_int64, c_int64, c_int64, c_int64, c_void_p, c_size_t, c_void_p]),
    "bgcn_colsum_workspace_size": (c_size_t, [c_int64, c_int32]),
    "bgcn_colsum": (c_int, [c_void_p, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_size_t,
                            c_void_p]),
    "bgcn_scatter_mean_workspace_size": (c_size_t, [c_int64]),
    "bgcn_scatter_mean_fwd": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int64,
                                      c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_size_t,
                                      c_void_p]),
    "bgcn_scatter_mean_bwd": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int32,
                                      c_int64, c_void_p, c_int64, c_void_p]),
    "bgcn_graph_pair_plans": (c_int, [c_void_p, c_size_t, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "bgcn_head_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "bgcn_head_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p,
                                   c_void_p, c_void_p, c_void_p]),
    "bgcn_bigcn_workspace_size": (c_size_t, [c_int64, c_int64, c_int64, c_int64]),
    "bgcn_bigcn_forward": (c_int, [POINTER(BiGCNArgs), c_void_p, c_size_t, c_void_p]),
    "bgcn_bigcn_backward": (c_int, [POINTER(BiGCNArgs), c_void_p, c_size_t, c_void_p]),
    "bgcn_keep_words": (c_int, [c_uint64, c_int64, c_int32, c_void_p, c_void_p]),
    "bgcn_adam_step": (c_int, [c_void_p, c_void_p]),
    "bgcn_weight_images_size": (c_size_t, [c_int64]),
    "bgcn_drop_edges_workspace_size": (c_size_t, [c_int64]),
    "bgcn_drop_edges": (c_int, [c_void_p, c_int64, c_double, c_void_p, c_int64, c_void_p, c_int64, c_double,
                                c_void_p, c_int64, c_void_p, c_int64, c_int64, c_uint64, c_int32, c_void_p,
                                c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_prepare_workspace_size": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int64]),
    "bgcn_prepare_batch": (c_int, [POINTER(BatchDesc), c_int64, c_int32, c_int32, c_void_p, c_size_t,
                                   c_void_p]),
    "bgcn_csr_to_dense": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int32,
                                  c_void_p, c_void_p]),
    "bgcn_train_step_workspace_size": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int64, c_int64]),
    "bgcn_train_step": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_train_step_dw1": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_eval_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_join_side": (c_int, [c_void_p]),
    "bgcn_train_step_saved": (c_int, [c_void_p, c_size_t, c_int64, c_int64, c_int64, c_int64,
                                      POINTER(c_void_p), POINTER(c_void_p)]),
    "bgcn_loader_create": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_uint64, c_int64,
                                   c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    "bgcn_loader_slot_bytes": (c_int64, [c_void_p]),
    "bgcn_loader_len": (c_int64, [c_void_p]),
    "bgcn_loader_next": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_int64,
                                 POINTER(c_void_p)]),
    "bgcn_loader_destroy": (None, [c_void_p]),
    "bgcn_loader_wait": (c_int, [c_void_p]),
    "bgcn_loader_get_stats": (c_int, [c_void_p, c_void_p, c_int]),
    "bgcn_bn_fold": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int64, c_void_p, c_void_p, c_void_p]),
    "bgcn_edge_infer": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "bgcn_ebgcn_conv2_lin_workspace_size": (c_size_t, [c_int64, c_int64, c_int64]),
    "bgcn_ebgcn_conv2_lin": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64,
                                     c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                     c_void_p, c_size_t, c_void_p]),
    "bgcn_explain_sums_workspace_size": (c_size_t, [c_int64]),
    "bgcn_explain_sums": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                  c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                  c_void_p, c_size_t, c_void_p]),
    "bgcn_segment_rank_workspace_size": (c_size_t, [c_int64]),
    "bgcn_segment_rank": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_size_t, c_void_p]),
    "bgcn_tree_centrality_workspace_size": (c_size_t, [c_int64, c_int64]),
    "bgcn_tree_centrality": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p,
                                     c_void_p, c_size_t, c_void_p]),
    "bgcn_rank_similarity_workspace_size": (c_size_t, [c_int64]),
    "bgcn_rank_similarity": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int32, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_confusion": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "bgcn_ebgcn_eval_workspace_size": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int64, c_int]),
    "bgcn_ebgcn_eval_step": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_ebgcn_eval_saved": (c_int, [c_void_p, c_size_t, c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_int,
                                      POINTER(EbgcnEvalView)]),
    "bgcn_edge_infer_train_workspace_size": (c_size_t, [c_int64, c_int64]),
    "bgcn_edge_infer_train_fwd": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_edge_infer_train_bwd": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_ebgcn_conv2_lin_train_workspace_size": (c_size_t, [c_int64, c_int64, c_int64]),
    "bgcn_ebgcn_conv2_lin_train_fwd": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_ebgcn_conv2_lin_train_bwd": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_adam_multi_table_size": (c_size_t, [c_int]),
    "bgcn_adam_multi_plan": (c_int, [c_void_p, c_int, c_void_p, c_size_t, POINTER(c_int64)]),
    "bgcn_adam_multi_step": (c_int, [c_void_p, c_void_p]),
    "bgcn_ebgcn_train_loss": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_float, c_float,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p]),
    "bgcn_lstm_workspace_size": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int64]),
    "bgcn_lstm_eval": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_lstm_train_workspace_size": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int64]),
    "bgcn_lstm_train_grad": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_bert_workspace_size": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int64, c_int]),
    "bgcn_bert_eval": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_bert_train_workspace_size": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int64]),
    "bgcn_bert_train_grad": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_w16_image_size": (c_size_t, [c_int64, c_int64]),
    "bgcn_w16_pack": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "bgcn_gemm_xwt_w16_workspace_size": (c_size_t, [c_int64, c_int64, c_int64]),
    "bgcn_gemm_xwt_w16": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                  c_void_p, c_size_t, c_void_p]),
    "bgcn_bert_w16_workspace_size": (c_size_t, [c_int64, c_int64, c_int64, c_int64]),
    "bgcn_bert_eval_w16": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_gemm_skinny_workspace_size": (c_size_t, [c_int64, c_int64, c_int64]),
    "bgcn_gemm_xwt_skinny": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64,
                                     c_int64, c_void_p, c_size_t, c_void_p]),
    "bgcn_gemm_xw_skinny": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                    c_void_p, c_size_t, c_void_p]),
    "bgcn_gemm_tn_skinny": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                    c_void_p]),
    "bgcn_bert_train_skinny_workspace_size": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int64]),
    "bgcn_bert_train_grad_skinny": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_bert_encode_workspace_size": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int64, c_int]),
    "bgcn_bert_encode": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "bgcn_set_kernel_timing": (c_int, [c_int]),
    "bgcn_kernel_timing": (c_int, [c_int, POINTER(c_float), POINTER(c_int64)]),
    "bgcn_kernel_span": (c_int, [c_int, POINTER(c_float), POINTER(c_int64)]),
}

_lock = threading.Lock()
_lib = None


class BGCNError(RuntimeError):
    pass


def load_library(path: str = LIB_PATH):
    """Load and type the library (no GPU needed: used by the CPU symbol tests)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(path):
            raise ImportError(
                f"libbgcn.so not found at {path}: build it with `make -C bigcn_amd/csrc` or "
                "`python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)")
        lib = ctypes.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.bgcn_abi_version() != ABI_VERSION:
            raise ImportError("libbgcn.so ABI version mismatch")
        _lib = lib
        return lib


_gpu_seen = False


def lib():
    """The library, for device work: requires a ROCm device (checked until one is seen)."""
    global _gpu_seen
    if not _gpu_seen:
        if not torch.cuda.is_available():
            raise BGCNError("the bigcn_amd HIP path needs a ROCm GPU (no CPU fallback exists)")
        _gpu_seen = True
    return _lib if _lib is not None else load_library()


def check(rc: int) -> None:
    if rc != 0:
        msg = load_library().bgcn_last_error().decode(errors="replace")
        raise BGCNError(f"libbgcn error {rc}: {msg}")


def raise_on_status(word: int, bits: int = 1 | 2 | 8, index_also: str = "", suffix: str = "") -> None:
    """Raise what a status word of the library reports, looking at ``bits`` only: 8 an internal
    hand-off timed out, 1 an index out of range (``index_also`` names what else sets it in the
    caller's kernels), 2 a label out of range, ``BGCN_STATUS_TOKEN`` a token id outside the vocabulary.
    ``suffix`` ends every ``IndexError``'s message."""
    word &= bits
    if word & 8:
        raise RuntimeError("libbgcn: an internal cross-workgroup hand-off timed out")
    if word & BGCN_STATUS_TOKEN:
        raise IndexError("input_ids holds a token id outside [0, vocab)" + suffix)
    if word & 1:
        raise IndexError("the batch holds an edge, root or tree index out of range" + index_also + suffix)
    if word & 2:
        raise IndexError("the batch holds a label outside [0, num_class)" + suffix)


def stream_handle(device=None) -> int:
    """hipStream_t of the current torch stream (of `device`, default the current device).
    The per-call form reads torch's raw current stream (~0.1 us; the Stream object path
    costs ~3 us and runs several times per drop-in training step)."""
    if device is None and _raw_stream is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream(device).cuda_stream


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)
if _cur_device is None:
    _raw_stream = None


def ptr(t) -> int:
    """Device pointer of a tensor (or 0 for None)."""
    if t is None:
        return 0
    return t.data_ptr()


def workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
