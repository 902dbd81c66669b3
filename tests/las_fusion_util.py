"""What the CPU and GPU tests of the fused LAS beam search share: the fixture
tests/golden/las_fusion_tiny.npz (written by tests/golden/make_golden_las_fusion.py) and the groups it records."""
import json

from tests.las_beam_util import LEN_WEIGHTS, SETS  # noqa: F401

SEARCHES = SETS["A"]["searches"]
# (lm_weight, beam widths): the groups whose decision margin stays above 1e-3 on all five searches and both length weights
GROUPS = [[0.5, [1, 3, 4, 8, 10]], [0.3, [1, 3, 10]], [0.1, [3]], [1.0, [1]]]
CASES = [(a, W) for a, widths in GROUPS for W in widths]
MARGIN = 1e-3


def load_las_fusion_golden():
    """-> (the groups as the maker wrote them, all arrays as numpy)"""
    from tests.util import golden_npz
    z = golden_npz("las_fusion_tiny")
    groups = json.loads(bytes(z.pop("groups")).decode())
    return groups, dict(z)


def fusion_key(u, t, bw, lw, a):
    return f"case/u{u}_t{t}/bw{bw}_lw{lw}_lm{a}"


def fused_nbest(g, u, t, bw, lw, a):
    """the fused N-best list of utterance u cut to t frames at LM weight a -> (hyps, scores), best first"""
    from tests.util import split_ragged
    key = fusion_key(u, t, bw, lw, a)
    return split_ragged(g[key + "/hyps"], g[key + "/lens"]), g[key + "/scores"].tolist()
