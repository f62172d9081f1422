"""What one slot of the frame ring remembers about its two cached workgroup orders, and the steps that change it: the keys and states of
csrc/frame_ring.h, compiled with g++ (tests/frame_ring_host/frame_ring_host.cpp: the header includes nothing of HIP) and walked against a model
written from the library's rules.

  order key      tiles_x, slabs, mode, grid.  Two keys match when every field is equal; a default key matches nothing, itself included.
  feedback key   tile_w, band_rows, first_band, band_stride, n_bands; texture_size and update_position, each component truncated toward zero to an
                 integer; mode * 16 + static_mode; seg.  Matching as above.

  step                          answer                                      effect
    order request (key)           hit: the table is allocated and the         on a miss the table is written (so it is allocated) and the key
                                  stored key matches                          recorded; a hit changes nothing
    order forget                  -                                           no key is stored; the table stays allocated
    feedback begin (key)          may the previous order be used: the         a key that does not match the stored one makes the state invalid
                                  state is valid AFTER the effect             and is stored
    sort enqueued                 -                                           the state is valid
    feedback forget               -                                           invalid, no key stored

A launch that is not a feedback launch takes no feedback step.  Nothing here touches a GPU."""
import itertools
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "frame_ring_host")

ORDER_FIELDS = ("tiles_x", "slabs", "mode", "grid")
FEEDBACK_FIELDS = ("tile_w", "band_rows", "first_band", "band_stride", "n_bands", "texture_w", "texture_h", "update_x", "update_y", "modes", "seg")


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def okey(tiles_x, slabs, mode, grid):
    return (tiles_x, slabs, mode, grid)


def fkey(tile_w=256, band_rows=8, first_band=1, band_stride=2, n_bands=16, texture_size=(2048.0, 1024.0), update_position=(512.0, 128.0), mode=7, static_mode=5, seg=1):
    """-> (the twelve numbers of a command line, the eleven values the library's key must hold)"""
    args = (tile_w, band_rows, first_band, band_stride, n_bands, bits(texture_size[0]), bits(texture_size[1]), bits(update_position[0]), bits(update_position[1]),
            mode, static_mode, seg)
    key = (tile_w, band_rows, first_band, band_stride, n_bands, int(texture_size[0]), int(texture_size[1]), int(update_position[0]), int(update_position[1]),
           mode * 16 + static_mode, seg)                     # int() truncates toward zero
    return args, key


def text(numbers):
    return " ".join(str(n) for n in numbers)


# the historic pair: a 33-pixel-wide launch of one slab in mode 1 as whole rays (2 footprints) and as two segments (3), both with a grid of 8
WHOLE_RAYS_33, TWO_SEGMENTS_33 = okey(2, 1, 1, 8), okey(3, 1, 1, 8)
ORDER_KEYS = (WHOLE_RAYS_33, TWO_SEGMENTS_33, okey(2, 1, 5, 8), okey(16, 64, 5, 1024))
FEEDBACK_KEYS = (fkey(), fkey(update_position=(768.0, 128.0)), fkey(seg=2))

# the alphabet of the walk: (name, argument, command line)
STEPS = tuple(("oreq", k, "oreq " + text(k)) for k in ORDER_KEYS) + (("oforget", None, "oforget"),) + \
    tuple(("fbegin", f[1], "fbegin " + text(f[0])) for f in FEEDBACK_KEYS) + (("fsort", None, "fsort"), ("fforget", None, "fforget"))

FRESH = dict(allocated=False, okey=None, fvalid=False, fkey=None)


def model_step(s, name, arg):
    """the table above, one branch per step; returns the new state and the step's answer (0 where it has none)"""
    s = dict(s)
    answer = 0
    if name == "oreq":
        answer = int(s["allocated"] and s["okey"] is not None and s["okey"] == arg)
        if not answer:
            s["allocated"] = True; s["okey"] = arg
    elif name == "oforget":
        s["okey"] = None
    elif name == "fbegin":
        if s["fkey"] is None or s["fkey"] != arg:
            s["fvalid"] = False; s["fkey"] = arg
        answer = int(s["fvalid"])
    elif name == "fsort":
        s["fvalid"] = True
    elif name == "fforget":
        s["fvalid"] = False; s["fkey"] = None
    else:
        raise AssertionError(name)
    return s, answer


def parse(line):
    v = [int(x) for x in line.split()]
    assert len(v) == 21, line
    got = dict(answer=v[0], allocated=bool(v[1]), okey=tuple(v[3:7]) if v[2] else None, fvalid=bool(v[8]), fkey=tuple(v[10:21]) if v[9] else None)
    if got["okey"] is not None:
        assert v[7] == got["okey"][3], line                  # the grid the launch takes from the state is the recorded key's
    return got


def run(text_in):
    r = subprocess.run([os.path.join(DIR, "frame_ring_host")], input=text_in, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def tool():
    subprocess.check_call(["make", "-C", DIR, "-s"])
    return run


def matches(lines):
    assert all(ln.startswith("match ") for ln in lines), lines
    return [tuple(int(x) for x in ln.split()[1:]) for ln in lines]


def test_every_field_of_both_keys_matters(tool):
    base_o = okey(16, 64, 5, 1024)
    cmds = ["omatch %s %s" % (text(base_o), text(base_o))]
    for i in range(len(ORDER_FIELDS)):
        other = list(base_o); other[i] += 1
        cmds.append("omatch %s %s" % (text(base_o), text(other)))
    variants = [dict(tile_w=257), dict(band_rows=9), dict(first_band=2), dict(band_stride=3), dict(n_bands=17), dict(texture_size=(2049.0, 1024.0)),
                dict(texture_size=(2048.0, 1025.0)), dict(update_position=(513.0, 128.0)), dict(update_position=(512.0, 129.0)), dict(mode=6), dict(seg=2)]
    assert len(variants) == len(FEEDBACK_FIELDS)
    base_f = fkey()
    cmds.append("fmatch %s %s" % (text(base_f[0]), text(base_f[0])))
    for i, kw in enumerate(variants):
        other = fkey(**kw)
        assert [j for j in range(11) if other[1][j] != base_f[1][j]] == [i], kw      # the variant differs in that field of the key alone
        cmds.append("fmatch %s %s" % (text(base_f[0]), text(other[0])))
    cmds.append("fmatch %s %s" % (text(base_f[0]), text(fkey(static_mode=2)[0])))   # the other half of mode * 16 + static_mode
    cmds += ["odefault " + text(base_o), "fdefault " + text(base_f[0])]
    got = matches(tool("\n".join(cmds) + "\n"))
    assert got == [(1,)] + [(0,)] * 4 + [(1,)] + [(0,)] * 12 + [(0, 0, 0), (0, 0, 0)], got


def test_the_two_forms_of_a_33_pixel_launch_have_different_order_keys(tool):
    """Until the launch-order tests the order key held tile_w where it needed tiles_x: a 33-pixel-wide launch of one slab in mode 1 has a grid of 8 both
    as whole rays (2 footprints) and as two segments (3 footprints), and the second form found the first one's table and left a footprint out."""
    out = tool("\n".join(["omatch %s %s" % (text(WHOLE_RAYS_33), text(TWO_SEGMENTS_33)), "omatch %s %s" % (text(TWO_SEGMENTS_33), text(WHOLE_RAYS_33)),
                          "reset", "oreq " + text(WHOLE_RAYS_33), "oreq " + text(TWO_SEGMENTS_33), "oreq " + text(TWO_SEGMENTS_33)]) + "\n")
    assert matches(out[:2]) == [(0,), (0,)]
    first, second, third = parse(out[3]), parse(out[4]), parse(out[5])
    assert (first["answer"], second["answer"], third["answer"]) == (0, 0, 1)
    assert first["okey"] == WHOLE_RAYS_33 and second["okey"] == TWO_SEGMENTS_33


def test_the_float_parameters_are_truncated_toward_zero(tool):
    cmds = []
    for name in ("texture_size", "update_position"):
        for comp in (0, 1):
            def key(x):
                v = [256.0, 256.0]; v[comp] = x
                return text(fkey(**{name: tuple(v)})[0])
            cmds += ["fmatch %s %s" % (key(256.0), key(256.5)), "fmatch %s %s" % (key(256.0), key(257.0))]
    # toward zero, not down: -0.5 is 0 (update_position may be any float; texture_size is >= 1 by the launch's argument check)
    cmds.append("fmatch %s %s" % (text(fkey(update_position=(-0.5, 0.0))[0]), text(fkey(update_position=(0.5, 0.0))[0])))
    cmds.append("fmatch %s %s" % (text(fkey(update_position=(-1.0, 0.0))[0]), text(fkey(update_position=(0.5, 0.0))[0])))
    assert matches(tool("\n".join(cmds) + "\n")) == [(1,), (0,)] * 4 + [(1,), (0,)]
    out = tool("reset\nfbegin %s\n" % text(fkey(texture_size=(256.5, 100.9), update_position=(-3.7, 3.7))[0]))
    assert parse(out[1])["fkey"][5:9] == (256, 100, -3, 3)


def test_every_walk_of_up_to_four_steps_matches_the_model(tool):
    """10 + 100 + 1000 + 10000 sequences over the ten steps from a fresh slot, one process: the answer of every step and the state after it."""
    seqs = [seq for n in range(1, 5) for seq in itertools.product(range(len(STEPS)), repeat=n)]
    assert len(STEPS) == 10 and len(seqs) == 11110
    lines = tool("".join("reset\n" + "".join(STEPS[t][2] + "\n" for t in seq) for seq in seqs))
    assert len(lines) == sum(1 + len(seq) for seq in seqs)
    at = 0
    hits = reuses = 0
    for seq in seqs:
        got = parse(lines[at]); at += 1
        s = dict(FRESH)
        assert {k: got[k] for k in s} == s and got["answer"] == 0, seq
        for i, t in enumerate(seq):
            name, arg, _ = STEPS[t]
            s, answer = model_step(s, name, arg)
            got = parse(lines[at]); at += 1
            where = ([STEPS[k][2] for k in seq], i)
            assert {k: got[k] for k in s} == s, (where, got, s)
            assert got["answer"] == answer, (where, got, answer)
            hits += name == "oreq" and answer
            reuses += name == "fbegin" and answer
    assert at == len(lines)
    assert hits > 0 and reuses > 0                           # the walk reaches both kinds of "use what is there"


def test_a_launch_that_is_no_feedback_launch_leaves_the_feedback_state_alone(tool):
    f = "fbegin " + text(FEEDBACK_KEYS[0][0])
    between = ["oreq " + text(ORDER_KEYS[3]), "oforget", "oreq " + text(ORDER_KEYS[0]), "oreq " + text(ORDER_KEYS[0])]
    out = [parse(ln) for ln in tool("\n".join(["reset", f, "fsort"] + between + [f]) + "\n")]
    assert out[1]["answer"] == 0 and out[2]["fvalid"]        # the first launch of a view runs in the static order; its sort makes the state valid
    for got in out[3:7]:
        assert (got["fvalid"], got["fkey"]) == (True, FEEDBACK_KEYS[0][1])
    assert out[7]["answer"] == 1                             # the later feedback launch with the same key still uses the order it finds
    # ... and without the sort in between (a launch that failed) it does not
    out = [parse(ln) for ln in tool("\n".join(["reset", f] + between + [f]) + "\n")]
    assert out[-1]["answer"] == 0
