"""The library's run-time options (csrc/common.h: EMO_OPTIONS) through the C ABI and emoasr_amd.lib, without a GPU: the set of
names and every default, the normalisation emoasr_set_option applies, the scoped form lib.options(), the errors and the
environment aliases lib.load() applies."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> default: transcribed from the initialisers and the name chain of emoasr_set_option as they stood before the options
# moved into one table (one option then was a global + a setter + a declaration + a strcmp arm).  An option that is lost, renamed
# or re-defaulted fails here.
DEFAULTS = {
    "tr_read": 1, "gemm_tile": 0, "tn_group_blocks": 0, "tn_group_kb": 0, "tn_place": 0, "tn_big": 1, "tn_big_blocks": 0,
    "gemm_wholek": 1, "gemm_kb": 0, "gemm_xcd": 1, "split_tile": 0, "split_kb": 1, "split_min128": 512, "conv_big": 1,
    "big_bm": 0, "big_korder": 1, "big_min_tiles": 2000, "dwconv_lds": 1, "conv_strip": 0, "conv_fused": 1, "wgrad_side": 0,
    "stack_launch": 1, "ffn_save_dact": 1, "attn_mask_bits": 1, "attn_prelaunch": 0, "conv1_pair": 1, "big_waves": 8,
    "big_n256": 2, "gemm_wide128": 0, "ln_fwd8": 1, "ln_bwd_pf": 1, "ln_bwd_blocks": 512, "rnnt_greedy_coop": 1,
    "rnnt_beam_mfma": 1, "decode_coop": 1, "lstm_coop": 1, "decode_coop_merge": 1, "attn_fw": 0, "attn_fwd4": 1, "attn_q2": 1,
    "attn_bwd_split": 1, "attn_side": 1, "attn_side_prio": 0, "attn_lpt": 1, "attn_fwd_split": 1, "attn_xcd": 1,
    "attn_fwd_waves": 0, "timers": 0, "timer_stride": 1,
}
LN_BWD8_MAXBLK = 2048   # csrc/common.h: the block maximum of the N % 8 == 0 LayerNorm backward

# options whose setter was `v ? 1 : 0` / `v != 0`
ON_OFF = ["tn_place", "tn_big", "gemm_wide128", "conv1_pair", "wgrad_side", "ffn_save_dact", "attn_mask_bits", "attn_prelaunch",
          "attn_q2", "attn_bwd_split", "attn_side", "attn_side_prio", "ln_fwd8", "ln_bwd_pf", "rnnt_beam_mfma"]
# (option, value set, value stored): every setter that was not a plain assignment, out of range and in range
NORMALISED = [
    ("attn_fwd_waves", 3, 0), ("attn_fwd_waves", 2, 2), ("attn_fwd_waves", 1, 1), ("attn_fwd_waves", 4, 4),
    ("attn_fw", 3, 0), ("attn_fw", 4, 4), ("attn_fw", 2, 2),
    ("tn_big_blocks", 32, 0), ("tn_big_blocks", 2000, 0), ("tn_big_blocks", 192, 192), ("tn_big_blocks", 64, 64),
    ("tn_big_blocks", 1024, 1024),
    ("tn_group_kb", 3, 0), ("tn_group_kb", 2, 2),
    ("tn_group_blocks", -5, 0), ("tn_group_blocks", 512, 512),
    ("split_tile", 4, 0), ("split_tile", 3, 3),
    ("split_kb", 3, 1), ("split_kb", 2, 2),
    ("split_min128", 0, 512), ("split_min128", 64, 64),
    ("big_waves", 5, 8), ("big_waves", 4, 4),
    ("big_n256", -1, 0), ("big_n256", 1, 1),
    ("ln_bwd_blocks", 10, 64), ("ln_bwd_blocks", 256, 256), ("ln_bwd_blocks", 1 << 30, LN_BWD8_MAXBLK),
    ("conv_strip", -1, 0), ("conv_strip", 3, 3), ("conv_strip", 1 << 20, 1 << 16),
    ("timer_stride", 0, 1), ("timer_stride", 7, 7),
] + [(n, 7, 1) for n in ON_OFF] + [(n, 0, 0) for n in ON_OFF]


ALIASES = [   # (environment, the options it changes)
    ({}, {}),
    ({"EMOASR_CONV_FUSED": "0"}, {"conv_fused": 0, "dwconv_lds": 0}),
    ({"EMOASR_CONV_FUSED": "1"}, {}),
    ({"EMOASR_FFN_SAVE_DACT": "0"}, {"ffn_save_dact": 0}),
    ({"EMOASR_CONV_BIG": "0"}, {"conv_big": 0}),
    ({"EMOASR_BIG_MIN_TILES": "7"}, {"big_min_tiles": 7}),
    ({"EMOASR_DECODE_COOP": "0"}, {"decode_coop": 0}),
    ({"EMOASR_CONV_BIG": "0", "EMOASR_OPTIONS": "conv_big=1"}, {}),
    ({"EMOASR_BIG_MIN_TILES": "7", "EMOASR_OPTIONS": "big_min_tiles=9,big_waves=5"}, {"big_min_tiles": 9}),
]
_DUMP = ("import json; from emoasr_amd import lib; "
         "print(json.dumps({n: [lib.get_option(n), lib.option_default(n)] for n in lib.option_names()}))")


@pytest.fixture(scope="module")
def fresh():
    """{option: [value, default]} as a fresh Python process sees it, one process per environment of ALIASES -- no earlier test's
    options in it; started together, since each spends its time importing torch"""
    base = {k: v for k, v in os.environ.items() if not k.startswith("EMOASR_") or k == "EMOASR_HIP_LIB"}
    base["PYTHONPATH"] = ROOT + os.pathsep + base.get("PYTHONPATH", "")
    procs = [subprocess.Popen([sys.executable, "-c", _DUMP], env=dict(base, **env), cwd=ROOT, stdout=subprocess.PIPE, text=True)
             for env, _ in ALIASES]
    outs = [p.communicate()[0] for p in procs]
    assert all(p.returncode == 0 for p in procs)
    return [json.loads(o) for o in outs]


def test_names_and_defaults_are_the_pinned_table(fresh):
    from emoasr_amd import lib
    names = lib.option_names()
    assert len(names) == len(set(names))
    assert set(names) == set(DEFAULTS), (set(names) ^ set(DEFAULTS))
    assert {n: lib.option_default(n) for n in names} == DEFAULTS
    handle = lib.load()
    assert handle.emoasr_option_count() == len(DEFAULTS)
    assert handle.emoasr_option_name(-1) is None and handle.emoasr_option_name(len(DEFAULTS)) is None
    # the values a fresh process starts with are the defaults
    assert {n: v[0] for n, v in fresh[0].items()} == DEFAULTS
    assert {n: v[1] for n, v in fresh[0].items()} == DEFAULTS


@pytest.mark.parametrize("name,value,stored", NORMALISED, ids=[f"{n}={v}" for n, v, _ in NORMALISED])
def test_set_option_normalises_as_the_setters_did(name, value, stored):
    from emoasr_amd import lib
    with lib.options(**{name: value}):
        assert lib.get_option(name) == stored
        assert lib.option_default(name) == DEFAULTS[name]


def test_plain_options_store_what_they_are_given():
    from emoasr_amd import lib
    plain = sorted(set(DEFAULTS) - {n for n, _, _ in NORMALISED})
    assert "big_min_tiles" in plain and "tr_read" in plain and "timers" in plain
    for name in plain:
        for value in (0, 1, 7, -3):
            with lib.options(**{name: value}):
                assert lib.get_option(name) == value, name


def test_get_option_takes_null_pointers():
    import ctypes
    from emoasr_amd import lib
    handle = lib.load()
    v = ctypes.c_int(-1)
    assert handle.emoasr_get_option(b"big_waves", None, None) == 0
    assert handle.emoasr_get_option(b"big_waves", None, ctypes.byref(v)) == 0 and v.value == 8
    assert handle.emoasr_get_option(b"split_min128", ctypes.byref(v), None) == 0 and v.value == lib.get_option("split_min128")


def test_options_scope_restores_previous_values():
    from emoasr_amd import lib
    lib.set_option("big_bm", 192)   # a previous value that is not the default
    try:
        with lib.options(big_bm=128, conv_strip=4):
            assert (lib.get_option("big_bm"), lib.get_option("conv_strip")) == (128, 4)
            with lib.options(big_bm=256):   # nested, same option
                assert lib.get_option("big_bm") == 256
                with lib.options():
                    assert lib.get_option("big_bm") == 256
            assert lib.get_option("big_bm") == 128
        assert (lib.get_option("big_bm"), lib.get_option("conv_strip")) == (192, DEFAULTS["conv_strip"])
        with pytest.raises(ZeroDivisionError):
            with lib.options(big_bm=128, tn_place=1):
                assert lib.get_option("tn_place") == 1
                raise ZeroDivisionError
        assert (lib.get_option("big_bm"), lib.get_option("tn_place")) == (192, 0)
    finally:
        lib.set_option("big_bm", lib.option_default("big_bm"))
    assert lib.get_option("big_bm") == DEFAULTS["big_bm"]


def test_unknown_names_are_errors():
    from emoasr_amd import lib
    with pytest.raises(lib.EmoasrHipError, match="unknown option 'no_such_option'"):
        lib.set_option("no_such_option", 1)
    with pytest.raises(lib.EmoasrHipError, match="unknown option 'no_such_option'"):
        lib.get_option("no_such_option")
    with pytest.raises(lib.EmoasrHipError, match="unknown option 'no_such_option'"):
        lib.option_default("no_such_option")
    ran = []
    with pytest.raises(lib.EmoasrHipError, match="unknown option 'no_such_option'"):
        with lib.options(big_bm=128, no_such_option=1, conv_strip=4):
            ran.append(1)
    assert not ran, "the block ran although one name was bad"
    assert lib.get_option("big_bm") == DEFAULTS["big_bm"] and lib.get_option("conv_strip") == DEFAULTS["conv_strip"]


@pytest.mark.parametrize("case", range(1, len(ALIASES)), ids=[",".join(f"{k}={v}" for k, v in e.items()) for e, _ in ALIASES[1:]])
def test_environment_aliases(fresh, case):
    """lib.load() applies the aliases, then EMOASR_OPTIONS (which wins); nothing else in the package sets an option"""
    got, changed = fresh[case], ALIASES[case][1]
    assert {n: v[0] for n, v in got.items()} == dict(DEFAULTS, **changed)
    assert {n: v[1] for n, v in got.items()} == DEFAULTS
