"""What a context holds as its sky LUT and the transitions that change it: SkyLutHeld of csrc/sky_lut_reuse.h, compiled with g++
(tests/lut_reuse_host/lut_transitions_host.cpp: the header includes nothing of HIP) and walked against a model written from the library's two tables.

  what the context holds      have_sky  sky_in_memory  sky_partial   (the booleans sky_lut_state derives, the input of the reuse decision)
    None                         0          -              -
    Whole                        1          1              0         the only state a whole-form hit needs
    Rows                         1          0              1
    Shared                       1          1              1

  transition                  effect
    touch                       sky_key invalid, the epoch moves
    table replaced              trans_gen + 1, sky_key and rows_key invalid, the epoch moves; what the context holds does NOT change
    drop                        holds None, sky_key invalid, the epoch moves
    became whole (key)          holds Whole, sky_key = key
    became rows (sun, w, h)     holds Rows, sun and size recorded
    became shared (sun, w, h)   holds Shared, sun and size recorded
    reuse switch (v)            the switch set, sky_key and rows_key invalid, the epoch moves

The epoch is only ever compared for equality, so "moves" is "differs from before".  Nothing here touches a GPU."""
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "lut_reuse_host")

NONE, WHOLE, ROWS, SHARED = range(4)
FLAGS_OF = {NONE: (0, None, None), WHOLE: (1, 1, 0), ROWS: (1, 0, 1), SHARED: (1, 1, 1)}   # have_sky, sky_in_memory, sky_partial; None: not stated


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


R2 = float(np.float32(1.0) / np.sqrt(np.float32(2.0)))
SUN_W = (bits(R2), bits(R2), bits(0.0))              # the three suns differ, and so do the three sizes: a record that took the wrong one shows
SUN_R = (bits(0.0), bits(R2), bits(-R2))
SUN_S = (bits(-0.0), bits(1.0), bits(0.0))
KEY = SUN_W + (200, 100, 0, 3)                       # sun bits, w, h, mapping, trans_gen of a whole-form request
KEY_ULP = (SUN_W[0] + 1,) + KEY[1:]                  # the same request with sun[0] one fp32 ulp further from zero

# the seven transitions, each with fixed arguments: (name, command line)
TRANSITIONS = (
    ("touch", "touch"),
    ("table", "table"),
    ("drop", "drop"),
    ("whole", "whole " + " ".join(map(str, KEY))),
    ("rows", "rows %d %d %d 8 4" % SUN_R),
    ("shared", "shared %d %d %d 64 32" % SUN_S),
    ("reuse", "reuse 0"),
)
CACHED = "cached %d %d %d 8 4 0 3 1 3" % SUN_R       # a stored rows key: not a transition, the starting point of the second set of walks


def model_step(s, name):
    """the table above, one line per transition; returns the new state and whether the epoch moved"""
    s = dict(s)
    moved = False
    if name == "touch":
        s["sky"] = 0; moved = True
    elif name == "table":
        s["gen"] += 1; s["sky"] = 0; s["rows"] = 0; moved = True
    elif name == "drop":
        s["holds"] = NONE; s["sky"] = 0; moved = True
    elif name == "whole":
        s["holds"] = WHOLE; s["sky"] = 1
    elif name == "rows":
        s["holds"] = ROWS; s["sun"] = SUN_R; s["size"] = (8, 4)
    elif name == "shared":
        s["holds"] = SHARED; s["sun"] = SUN_S; s["size"] = (64, 32)
    elif name == "reuse":
        s["reuse"] = 0; s["sky"] = 0; s["rows"] = 0; moved = True
    else:
        raise AssertionError(name)
    return s, moved


def parse(line):
    v = [int(x) for x in line.split()]
    assert len(v) == 15, line
    return dict(holds=v[0], sky=v[1], rows=v[2], gen=v[3], moved=v[4], sun=tuple(v[5:8]), size=(v[8], v[9]), reuse=v[10],
                have_sky=v[11], sky_in_memory=v[12], sky_partial=v[13], no_writers=v[14])


def run(text):
    r = subprocess.run([os.path.join(DIR, "lut_transitions_host")], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def tool():
    subprocess.check_call(["make", "-C", DIR, "-s"])
    return run


def sequences():
    for n in range(1, 5):
        yield from itertools.product(range(len(TRANSITIONS)), repeat=n)


def check_flags(got, where):
    have_sky, in_memory, partial = FLAGS_OF[got["holds"]]
    assert got["have_sky"] == have_sky, where
    if in_memory is not None:
        assert (got["sky_in_memory"], got["sky_partial"]) == (in_memory, partial), where
    assert got["reuse"] in (0, 1) and got["no_writers"] == 1, where


@pytest.mark.parametrize("start", ["fresh", "rows key stored"])
def test_every_walk_of_up_to_four_transitions_matches_the_model(tool, start):
    """7 + 49 + 343 + 2401 sequences from a fresh state, every step compared; and the same walks from a state whose rows cache holds a key, where
    'rows_key invalid' is no longer true from the start.  In every state reached the derived booleans are the first table's."""
    seqs = list(sequences())
    assert len(seqs) == 7 + 49 + 343 + 2401
    prefix = "reset\n" + (CACHED + "\n" if start != "fresh" else "")
    lines = tool("".join(prefix + "".join(TRANSITIONS[t][1] + "\n" for t in seq) for seq in seqs))
    per_prefix = prefix.count("\n")
    assert len(lines) == sum(per_prefix + len(seq) for seq in seqs)
    at = 0
    reached = set()
    for seq in seqs:
        fresh = parse(lines[at]); at += 1
        assert (fresh["holds"], fresh["sky"], fresh["rows"], fresh["gen"], fresh["reuse"], fresh["moved"]) == (NONE, 0, 0, 0, 1, 0), seq
        check_flags(fresh, seq)
        s = dict(holds=NONE, sky=0, rows=0, gen=0, reuse=1, sun=fresh["sun"], size=fresh["size"])   # the record of a fresh state is not the tables' business
        if start != "fresh":
            got = parse(lines[at]); at += 1
            s["rows"] = 1
            assert {k: got[k] for k in s} == s and got["moved"] == 0, seq
        for i, t in enumerate(seq):
            s, moved = model_step(s, TRANSITIONS[t][0])
            got = parse(lines[at]); at += 1
            where = ([TRANSITIONS[k][0] for k in seq], i)
            assert {k: got[k] for k in s} == s, (where, got, s)
            assert got["moved"] == int(moved), where
            check_flags(got, where)
            reached.add((got["holds"], got["sky"], got["rows"], got["reuse"]))
    assert at == len(lines)
    assert {r[0] for r in reached} == {NONE, WHOLE, ROWS, SHARED}
    if start != "fresh":
        assert any(r[2] for r in reached) and any(not r[2] for r in reached)


def reach(holds):
    """the commands that leave a state holding `holds` with KEY still stored wherever a transition sequence can leave it stored"""
    whole = TRANSITIONS[3][1]
    return {NONE: ["drop"], WHOLE: [whole], ROWS: [whole, TRANSITIONS[4][1]], SHARED: [whole, TRANSITIONS[5][1]]}[holds]


def test_a_whole_form_hit_needs_whole_the_switch_equal_keys_and_no_writers(tool):
    cases = list(itertools.product((NONE, WHOLE, ROWS, SHARED), (0, 1), (0, 1), (KEY, KEY_ULP)))
    text = ""
    for holds, reuse, nw, req in cases:
        text += "\n".join(["reset", "reuse %d" % reuse] + reach(holds) + ["nw %d" % nw, "hit " + " ".join(map(str, req))]) + "\n"
    lines = tool(text)
    hits = [int(ln.split()[1]) for ln in lines if ln.startswith("hit ")]
    stored = [parse(ln)["sky"] for ln, nxt in zip(lines, lines[1:]) if nxt.startswith("hit ")]
    assert len(hits) == len(cases) == len(stored) == 32
    for (holds, reuse, nw, req), hit, sky in zip(cases, hits, stored):
        assert sky == (0 if holds == NONE else 1), (holds, sky)           # Rows and Shared are asked with the key still stored: the state alone makes them miss
        assert hit == int(holds == WHOLE and reuse == 1 and req == KEY and nw == 1), (holds, reuse, nw, req == KEY)
    assert sum(hits) == 1


def test_the_named_cases(tool):
    whole, rows, shared = TRANSITIONS[3][1], TRANSITIONS[4][1], TRANSITIONS[5][1]
    hit = "hit " + " ".join(map(str, KEY))
    # "table replaced" on a Whole state leaves it Whole with no valid key: the LUT stays readable, and the same request renders again
    out = tool("\n".join(["reset", whole, "table", hit]) + "\n")
    before, after = parse(out[1]), parse(out[2])
    assert (before["holds"], before["sky"]) == (WHOLE, 1) and (after["holds"], after["sky"], after["gen"]) == (WHOLE, 0, 1) and out[3] == "hit 0"
    # "drop" from every state gives None
    for first in ([], [whole], [rows], [shared]):
        out = tool("\n".join(["reset"] + first + ["drop"]) + "\n")
        assert parse(out[-1])["holds"] == NONE and parse(out[-1])["have_sky"] == 0, first
    # "became rows" after "became whole" makes a following whole-form request a miss (and without it the request hits)
    assert tool("\n".join(["reset", whole, hit]) + "\n")[-1] == "hit 1"
    assert tool("\n".join(["reset", whole, rows, hit]) + "\n")[-1] == "hit 0"
    # "touch" leaves rows_key alone
    out = tool("\n".join(["reset", CACHED, whole, "touch"]) + "\n")
    assert parse(out[1])["rows"] == 1 and parse(out[3])["rows"] == 1 and parse(out[3])["sky"] == 0 and parse(out[3])["moved"] == 1
    # a failed launch leaves no key: the touch comes before it, "became whole" only after it
    out = tool("\n".join(["reset", whole, "touch", hit]) + "\n")
    assert parse(out[2])["holds"] == WHOLE and out[3] == "hit 0"
