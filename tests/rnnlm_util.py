"""Shared helpers of the RNN-LM tests: the tiny model's config and the loading of its fixtures
(tests/golden/rnnlm_tiny*.npz, written by tests/golden/make_golden_rnnlm.py)."""
import torch

from tests.util import golden_npz

RNNLM_CFG = dict(lm_type="rnn", vocab_size=40, embedding_size=48, hidden_size=64, num_layers=2, dropout_rate=0.1, tie_weights=False)
RNNLM_TRAIN_CFG = dict(RNNLM_CFG, learning_rate=2e-3, lr_schedule_type="lindecay", num_warmup_steps=2, weight_decay=0.01,
                       clip_grad_norm=0.5, accum_grad=1, log_step=1)
TRACE_TOTAL_STEPS = 10
YLENS = [17, 12, 9, 5, 2, 1]
PREDICT_STEPS = 6
PREDICT_YLENS = [[3, 1, 2], [4, 2, 2], [4, 3, 5], [5, 3, 6], [6, 5, 6], [7, 5, 8]]     # row lengths at each of the chained steps


def rnnlm_golden(name="rnnlm_tiny"):
    return {k: (torch.from_numpy(v) if v.dtype.kind in "fiu" else v) for k, v in golden_npz(name).items()}


def rnnlm_state(g):
    """the LM's weights (prefixed keys, as LM.state_dict() names them)"""
    return {k[3:]: v for k, v in g.items() if k.startswith("sd/")}
