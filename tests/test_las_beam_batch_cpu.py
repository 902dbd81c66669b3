"""The fixture of the batched LAS beam search (tests/golden/las_beam_tiny.npz, written by tests/golden/make_golden_las_beam.py)
and the host-side pieces of the search that need no device: the chunk capacity (engine/las.py:las_beam_chunk_capacity)."""
import pytest

from tests import las_beam_util as U
from tests import las_ref

MARGIN = 1e-3


@pytest.fixture(scope="module")
def fx():
    return U.load_las_beam_golden()


def test_sets_are_complete(fx):
    sets, g = fx
    assert sets == U.SETS
    n = 0
    for name, spec in sets.items():
        for u, t in spec["searches"]:
            for bw in spec["widths"]:
                for lw in U.LEN_WEIGHTS:
                    hyps, scores = U.golden_nbest(g, u, t, bw, lw)
                    assert 1 <= len(hyps) <= bw and len(scores) == len(hyps), (name, u, t, bw, lw)
                    assert all(len(h) >= 1 for h in hyps)
                    assert scores == sorted(scores, reverse=True)
                    n += 1
    assert n == 5 * 6 * 2 + 4 * 2 + 2 * 2
    keys = {k.rsplit("/", 1)[0] for k in g if k.startswith("case/")}
    assert len(keys) == n   # no case outside the sets (u0[:1] / u1[:1] appear in B and C at different widths)


def test_every_margin_exceeds_the_bar(fx):
    _, g = fx
    margins = {k: float(v) for k, v in g.items() if k.endswith("/margin")}
    assert len(margins) == 72
    worst = min(margins, key=margins.get)
    print(f"las_beam_tiny: smallest decision margin {margins[worst]:.3e} ({worst})")
    assert margins[worst] > MARGIN, (worst, margins[worst])


def test_frame_counts_and_widths_cover_the_edges(fx):
    sets, _ = fx
    frames = {t for spec in sets.values() for _, t in spec["searches"]}
    assert {1, 32, 33, 41, 50} <= frames            # one frame, one tile, a tile + 1, two tiles (twice)
    widths = {bw for spec in sets.values() for bw in spec["widths"]}
    assert {1, 8, 10, 16, 32} <= widths             # both sides of the 8 / 16 / 24 / 32 row groupings


@pytest.mark.parametrize("bw", [1, 4])
def test_uncut_utterances_equal_the_las_tiny_fixture(fx, bw):
    from tests.util import split_ragged
    _, g = fx
    las = las_ref.load_las_golden()[2]
    for u, t in U.SETS["A"]["searches"][:3]:
        assert las[f"decode/{u}/eouts"].shape[0] == t
        for lw in U.LEN_WEIGHTS:
            key = f"decode/{u}/bw{bw}_lw{lw}"
            hyps, scores = U.golden_nbest(g, u, t, bw, lw)
            assert hyps == split_ragged(las[key + "/hyps"], las[key + "/lens"])
            assert scores == las[key + "/scores"].tolist()


def test_chunk_capacity_edges():
    from emoasr_amd.engine.las import (LAS_BEAM_MAX_ROWS, LAS_BEAM_POOL_BUDGET_BYTES, las_beam_chunk_capacity,
                                       las_beam_pool_bytes)
    assert las_beam_pool_bytes(40, 64) == 2 * 40 * 64 * 4
    assert LAS_BEAM_MAX_ROWS == 1024
    for W in (1, 3, 4, 10, 32):   # small pools: the row limit decides
        S = las_beam_chunk_capacity(W, 64)
        assert S == 1024 // W and S * W <= LAS_BEAM_MAX_ROWS < (S + 1) * W
    # long utterances: the pool budget decides, exactly at its edge
    T = 1 << 19
    S = las_beam_chunk_capacity(32, T)
    assert S == LAS_BEAM_POOL_BUDGET_BYTES // las_beam_pool_bytes(32, T) and 1 <= S < 1024 // 32
    assert las_beam_pool_bytes(S * 32, T) <= LAS_BEAM_POOL_BUDGET_BYTES < las_beam_pool_bytes((S + 1) * 32, T)
    budget = las_beam_pool_bytes(4, 64) * 5
    assert las_beam_chunk_capacity(4, 64, budget=budget) == 5
    assert las_beam_chunk_capacity(4, 64, budget=budget - 1) == 4
    # never below one search, however small the budget or the row limit
    assert las_beam_chunk_capacity(32, 1 << 24) == 1
    assert las_beam_chunk_capacity(4, 64, budget=1) == 1
    assert las_beam_chunk_capacity(8, 64, max_rows=4) == 1
    assert las_beam_chunk_capacity(4, 64, max_rows=8) == 2
    assert las_beam_chunk_capacity(4, 64, max_rows=11) == 2

