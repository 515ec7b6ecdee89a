"""The oracle of TreeBERT's bf16 weight-image mode (``TreeBERT.use_weight_images("bf16")``), shared by
tests/test_bert_w16.py and tests/test_gpu_bert_w16.py: ``bert_ref.run`` in fp64 on a case's state dict
whose GEMM weights of the root-only chain - value, attention-output dense, intermediate, output dense of
every layer and the pooler's - went through ``.bfloat16().float()``; everything else is left as it is.
Only the trees' first rows matter to the class, so the oracle is fed ``x[rootindex]`` as B one-row trees."""
import functools
from types import SimpleNamespace

import torch

import bert_ref as R

BAR = 1e-4   # the project's bar on logp and loss
# the cases of the model tests (bert_ref.CASES / EDGE_CASES; `cap` and the attention-only ones left out)
CASES = ("single", "boundaries", "offset_strided", "many", "full_width", "many_trees", "hidden_1024", "hidden_320",
         "layers_24", "classes_1", "classes_63", "classes_64", "rows_over_switch")
ROUNDED = ("attention.self.value.weight", "attention.output.dense.weight", "intermediate.dense.weight",
           "output.dense.weight")


def case(name):
    return R.case(name) if name in R.CASES else R.edge_case(name)


def rounded_state_dict(sd, layers):
    names = {f"BERT.encoder.layer.{i}.{n}" for i in range(layers) for n in ROUNDED} | {"BERT.pooler.dense.weight"}
    assert names <= set(sd)
    return {k: (v.bfloat16().float() if k in names else v) for k, v in sd.items()}


def root_run(c, sd):
    """bert_ref.run (fp64) on the case's root rows as B one-row trees."""
    roots = c.x[c.rootindex]
    return R.run(sd, roots, torch.arange(c.B), c.cfg["layers"], c.heads, c.y)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The rounded-weight oracle of a case: logp [B, C] fp64, loss, pred, correct; read-only."""
    c = case(name)
    ref = root_run(c, rounded_state_dict(c.sd, c.cfg["layers"]))
    return SimpleNamespace(logp=ref.logp, loss=float(ref.loss), pred=ref.pred, correct=ref.correct)
