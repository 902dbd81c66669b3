"""What the CPU and GPU tests of the LAS beam search with the Transformer LM on the device share: the fixture
tests/golden/las_tlm_fusion_tiny.npz (written by tests/golden/make_golden_las_tlm_fusion.py) and the groups it records."""
import json

from tests.las_beam_util import LEN_WEIGHTS, SETS  # noqa: F401
from tests.las_fusion_util import fusion_key  # noqa: F401

SEARCHES = SETS["A"]["searches"]
# (lm_weight, beam widths): the groups whose decision margin stays above 1e-3 on all five searches and both length weights
GROUPS = [[0.1, [3, 4]], [0.3, [3, 4]], [0.5, [3]], [1.0, [1, 3, 4]], [0.2, [8]], [0.05, [10]], [2.0, [8, 10]]]
CASES = [(a, W) for a, widths in GROUPS for W in widths]
# the smallest margin of every (lm_weight, W) pair as the reference gave it on the CPU, to the two digits the record keeps
MARGINS = {(0.1, 3): 3.9e-3, (0.1, 4): 8.9e-3, (0.3, 3): 1.4e-3, (0.3, 4): 4.9e-3, (0.5, 3): 1.3e-3, (1.0, 1): 8.9e-2, (1.0, 3): 3.5e-3,
           (1.0, 4): 4.0e-3, (0.2, 8): 3.9e-3, (0.05, 10): 2.7e-3, (2.0, 8): 3.4e-3, (2.0, 10): 3.4e-3}
MARGIN = 1e-3
LONGEST = 10          # tokens of the longest recorded hypothesis


def load_las_tlm_fusion_golden():
    """-> (the groups as the maker wrote them, all arrays as numpy)"""
    from tests.util import golden_npz
    z = golden_npz("las_tlm_fusion_tiny")
    groups = json.loads(bytes(z.pop("groups")).decode())
    return groups, dict(z)


def fused_nbest(g, u, t, bw, lw, a):
    """the fused N-best list of utterance u cut to t frames at LM weight a -> (hyps, scores), best first"""
    from tests.util import split_ragged
    key = fusion_key(u, t, bw, lw, a)
    return split_ragged(g[key + "/hyps"], g[key + "/lens"]), g[key + "/scores"].tolist()
