"""What the CPU and GPU tests of the batched LAS beam search share: the fixture tests/golden/las_beam_tiny.npz (written by
tests/golden/make_golden_las_beam.py) and the sets of searches it records."""
import json

# set -> searches (utterance of las_tiny, its first frames) and beam widths; each set is decoded as ONE batch
SETS = {"A": dict(searches=[[0, 50], [1, 41], [2, 32], [0, 33], [1, 1]], widths=[1, 2, 3, 4, 8, 10]),
        "B": dict(searches=[[0, 1], [1, 1], [2, 1], [0, 33]], widths=[16]),
        "C": dict(searches=[[0, 1], [1, 1]], widths=[32])}
LEN_WEIGHTS = (0.0, 0.1)


def load_las_beam_golden():
    """-> (the sets as the maker wrote them, all arrays as numpy)"""
    from tests.util import golden_npz
    z = golden_npz("las_beam_tiny")
    sets = json.loads(bytes(z.pop("sets")).decode())
    return sets, dict(z)


def golden_nbest(g, u, t, bw, lw):
    """the reference's N-best list of utterance u cut to t frames -> (hyps, scores), best first"""
    from tests.util import split_ragged
    key = f"case/u{u}_t{t}/bw{bw}_lw{lw}"
    return split_ragged(g[key + "/hyps"], g[key + "/lens"]), g[key + "/scores"].tolist()
