"""CPU: the packed SR compiler's word table (evogp_amd/csrc/sr_tc.hip tc_table_entry), entry by entry.

tests/tc_word_table.py restates the table (`entry`) and, separately, the meaning of the select chains it replaces (`by_selects`: handlers by
NAME, so a handler id that moves in tc_handlers.json without the table following fails here).  For every class code and both halves
of the table (launches without / with reciprocal columns): the engine's entry (evogp_hip_debug_tc_table_entry, host memory) equals the
restated one bit for bit, and what the compiler makes of that entry -- the handler for each of {next word reads a variable or not} x {room
for the in-place form or not}, kept, uses a variable, stack delta, the leaf flag, the room an in-place division asks for -- equals what the
selects give."""
import ctypes
import json
import os

import pytest

import tc_word_table as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def builds():
    return json.load(open(os.path.join(ROOT, "evogp_amd", "lib", "tc_handlers.json")))


@pytest.fixture(scope="module")
def H(builds):
    return T.handler_ids(builds["K8_short"]["handlers"])


def test_every_build_numbers_its_handlers_alike(builds, H):
    for name, build in builds.items():
        assert T.handler_ids(build["handlers"]) == H, name
    assert H["push_v"] == H["push_c"] + 1 and H["leaf_v"] == H["leaf_c"] + 1   # TcCompileParams::leaf_id + 1: the variable's word
    assert max(H.values()) < 255


def engine_entry(recip, code):
    from evogp_amd import _lib

    e = (ctypes.c_uint * 2)()
    assert _lib.lib.evogp_hip_debug_tc_table_entry(recip, code, e) == 0
    return int(e[0]), int(e[1])


@pytest.mark.parametrize("recip", [0, 1])
def test_engine_table_is_the_restated_table(H, recip):
    for code in range(T.CODES):
        assert engine_entry(recip, code) == T.entry(code, recip, H), f"code {code} recip {recip}"


def test_entry_arguments_are_checked():
    from evogp_amd import _lib

    e = (ctypes.c_uint * 2)()
    L = _lib.lib
    assert L.evogp_hip_debug_tc_table_entry(2, 0, e) != 0 and L.evogp_hip_debug_tc_table_entry(0, T.CODES, e) != 0
    assert L.evogp_hip_debug_tc_table_entry(0, -1, e) != 0 and L.evogp_hip_debug_tc_table_entry(0, 0, None) != 0
    assert L.evogp_hip_debug_tc_table(2) != 0 and L.evogp_hip_debug_tc_table(-2) != 0 and L.evogp_hip_debug_tc_table(-1) == 0


@pytest.mark.parametrize("recip", [0, 1])
def test_table_means_what_the_selects_mean(H, recip):
    seen = 0
    for code in range(T.CODES):
        want = T.by_selects(code, recip, H)
        if want is None:
            continue   # (no lane has this code)
        seen += 1
        ids_w, (kept_w, uses_w, delta_w, leaf_w), room_w = want
        ids, bits = T.entry(code, recip, H)
        ids_g, (kept_g, useskept_g, delta_g, leaf_g), room_g = T.from_entry(ids, bits)
        what = f"code {code} (opx {code & 3}, pair {(code & 63) >> 2}, root {code >> 6}) recip {recip}"
        assert kept_g == kept_w and useskept_g == (kept_w and uses_w) and delta_g == delta_w and leaf_g == leaf_w, what
        if kept_w:   # (a lane without a word: its handler is never looked at)
            assert ids_g == ids_w, what
            assert room_g == room_w, what
        else:
            assert delta_w == 0, what
    assert seen == 2 * (36 + 1 + 4 + 3)


def test_without_twins_the_first_handler_of_each_pair_is_the_word(H):
    """a launch without the twins never looks at bytes 1 and 3 of an entry: bytes 0 and 2 are the selects' handlers with the twins off"""
    for recip in (0, 1):
        for code in range(T.CODES):
            want = T.by_selects(code, recip, H, twins_on=False)
            if want is None or not want[1][0]:
                continue
            ids, bits = T.entry(code, recip, H)
            got = T.from_entry(ids, bits)[0]
            assert got[True, True] == want[0][False, True] == want[0][True, True] and got[True, False] == want[0][False, False], (code, recip)
