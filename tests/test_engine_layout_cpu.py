"""The layout of the engine package (emoasr_amd/engine/): every name CTCEngine and the package had when the engine was one module still
resolves, CTCEngine is assembled by inheritance alone, and the encoder's stash records are one set of classes for the engine and
for layer_rt.  No device needed: importing the engine does not load the library."""
import inspect
import os

import emoasr_amd.engine as engine
from emoasr_amd import layer_rt
from emoasr_amd.engine import CTCEngine

HERE = os.path.dirname(os.path.abspath(__file__))


def test_recorded_names_still_resolve():
    """tests/golden/engine_surface.txt: sorted(n for n in vars(CTCEngine) if not n.startswith("__")) of the one-module engine (91 names)
    and the nine names other code imports from emoasr_amd.engine"""
    with open(os.path.join(HERE, "golden", "engine_surface.txt")) as f:
        names = f.read().split()
    assert len(names) == 100 and len(set(names)) == 100
    missing = [n for n in names if not (hasattr(CTCEngine, n) or hasattr(engine, n))]
    assert not missing, missing
    assert engine.ASREngine is CTCEngine


def test_engine_is_built_from_real_classes():
    mro = {c.__name__ for c in CTCEngine.__mro__}
    strays = []
    for name in dir(CTCEngine):
        f = inspect.getattr_static(CTCEngine, name)
        if inspect.isfunction(f) and f.__qualname__.split(".")[0] not in mro:
            strays.append((name, f.__qualname__))
    assert not strays, strays
    assert not hasattr(engine, "_DecoderMixinPlaceholder")
    assert not hasattr(engine.encoder, "_n") and not hasattr(engine.encoder, "_f")


def test_stash_records_are_shared():
    assert layer_rt.AttnStash is engine.AttnStash is engine.arena.AttnStash
    assert layer_rt.ConvStash is engine.ConvStash is engine.arena.ConvStash
    assert layer_rt.FFNStash is engine.FFNStash and layer_rt.LayerRecord is engine.LayerRecord
    # the output-dropout seed is where the numeric indices 7, 9 and 10 used to read it
    assert engine.FFNStash._fields == ("x", "mean", "rstd", "h", "u", "a", "s_in", "s_out")
    assert len(engine.AttnStash._fields) == 11 and engine.AttnStash._fields.index("s_out") == 9
    assert len(engine.ConvStash._fields) == 11 and engine.ConvStash._fields.index("s_out") == 10
    assert engine.LayerRecord._fields == ("ffm", "att", "conv", "ff", "fin")
