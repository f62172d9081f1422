"""When a sky-LUT call may reuse what the context holds: the decision of csrc/sky_lut_reuse.h, compiled with g++ (tests/lut_reuse_host: the header
includes nothing of HIP) and checked case by case against the rule as the library's documentation states it.

  whole form (csky_render_sky_lut_device): a hit iff the switch is on, a key is stored, the request's key equals it -- the three sun floats BIT FOR
  BIT, the size, the transmittance mapping and generation -- and the context holds a whole LUT of its own: have_sky, sky_in_memory, not
  sky_partial, no other device's rows in the slot (lut_writers empty).
  rows form (csky_render_sky_lut_rows_device): a hit iff the switch is on and the stored key equals the request's, first_row and row_stride
  included; what the ring holds does not matter, the rows live in a cache of their own.

Nothing here touches a GPU."""
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "lut_reuse_host")

FIELDS = ("valid", "s0", "s1", "s2", "w", "h", "tlut", "gen", "first_row", "row_stride")
FLAGS = ("reuse", "have_sky", "sky_in_memory", "sky_partial", "no_writers")


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def next_up(b):
    """the bit pattern one fp32 ulp further from zero"""
    return b + 1


SUN = [bits(float(v)) for v in (np.float32(1.0) / np.sqrt(np.float32(2.0)), np.float32(1.0) / np.sqrt(np.float32(2.0)), 0.0)]
BASE = dict(valid=1, s0=SUN[0], s1=SUN[1], s2=SUN[2], w=200, h=100, tlut=0, gen=3, first_row=0, row_stride=1)
GOOD = dict(reuse=1, have_sky=1, sky_in_memory=1, sky_partial=0, no_writers=1)
NAN_A, NAN_B = 0x7FC00000, 0x7FC00001            # two quiet NaNs with different payloads
NEG_ZERO = 0x80000000


def key(**changes):
    k = dict(BASE)
    k.update(changes)
    return k


def want(stored, req, flags, form):
    same = stored["valid"] and req["valid"] and all(stored[f] == req[f] for f in FIELDS[1:])
    if form == 1:
        return bool(flags["reuse"] and same)
    return bool(flags["reuse"] and same and flags["have_sky"] and flags["sky_in_memory"] and not flags["sky_partial"] and flags["no_writers"])


def cases():
    out = []

    def add(name, stored, req, flags=GOOD, forms=(0, 1)):
        for form in forms:
            out.append(("%s, %s form" % (name, ("whole", "rows")[form]), stored, req, dict(flags), form))

    add("the same request", key(), key())
    add("nothing stored", key(valid=0), key())
    for i in range(3):
        f = "s%d" % i
        add("sun[%d] one ulp up" % i, key(), key(**{f: next_up(BASE[f])}))
    add("sun[2] -0.0 against 0.0", key(), key(s2=NEG_ZERO))
    add("sun[2] 0.0 against -0.0", key(s2=NEG_ZERO), key())
    add("sun[2] -0.0 both", key(s2=NEG_ZERO), key(s2=NEG_ZERO))
    add("a NaN sun equals itself bit for bit", key(s0=NAN_A, s1=NAN_A, s2=NAN_A), key(s0=NAN_A, s1=NAN_A, s2=NAN_A))
    add("a NaN with another payload", key(s1=NAN_A), key(s1=NAN_B))
    add("a NaN against a number", key(s1=NAN_A), key())
    add("another width", key(), key(w=8))
    add("another height", key(), key(h=4))
    add("width and height swapped", key(), key(w=100, h=200))
    add("another mapping", key(), key(tlut=1))
    add("the transmittance table rendered again", key(), key(gen=4))
    add("a generation past 2^32", key(gen=(1 << 32) + 3), key(gen=3))
    add("another first row", key(first_row=1, row_stride=3), key(first_row=2, row_stride=3))
    add("another row stride", key(first_row=1, row_stride=3), key(first_row=1, row_stride=4))
    add("the same rows", key(first_row=1, row_stride=3), key(first_row=1, row_stride=3))
    add("rows stored, the whole LUT asked for", key(first_row=1, row_stride=3), key())
    # every combination of the switch and the context's flags, with the key equal and with it one ulp off
    for combo in itertools.product((0, 1), repeat=len(FLAGS)):
        flags = dict(zip(FLAGS, combo))
        add("flags %s, equal keys" % (combo,), key(), key(), flags)
        add("flags %s, sun one ulp off" % (combo,), key(), key(s0=next_up(BASE["s0"])), flags)
    return out


@pytest.fixture(scope="module")
def answers():
    subprocess.check_call(["make", "-C", DIR, "-s"])
    cs = cases()
    text = "".join(" ".join(str(int(k[f])) for f in FIELDS) + " " + " ".join(str(int(r[f])) for f in FIELDS) + " " +
                   " ".join(str(int(fl[f])) for f in FLAGS) + " %d\n" % form for _, k, r, fl, form in cs)
    r = subprocess.run([os.path.join(DIR, "lut_reuse_host")], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    got = [int(x) for x in r.stdout.split()]
    assert len(got) == len(cs), (len(got), len(cs))
    return cs, got


def test_every_case_of_the_decision_table(answers):
    cs, got = answers
    wrong = [(name, bool(g), want(k, r, fl, form)) for (name, k, r, fl, form), g in zip(cs, got) if bool(g) != want(k, r, fl, form)]
    assert not wrong, wrong[:8]


def test_the_table_has_hits_and_misses_of_both_forms(answers):
    cs, got = answers
    for form in (0, 1):
        seen = {bool(g) for (_, _, _, _, f), g in zip(cs, got) if f == form}
        assert seen == {True, False}, (form, seen)


def test_the_named_cases(answers):
    """the cases the rule is there for, spelled out: what a reader expects without evaluating want()"""
    cs, got = answers
    by_name = {name: bool(g) for (name, _, _, _, _), g in zip(cs, got)}
    for form in ("whole", "rows"):
        assert by_name["the same request, %s form" % form]
        assert by_name["a NaN sun equals itself bit for bit, %s form" % form]
        assert by_name["sun[2] -0.0 both, %s form" % form]
        for miss in ("nothing stored", "sun[0] one ulp up", "sun[1] one ulp up", "sun[2] one ulp up", "sun[2] -0.0 against 0.0", "sun[2] 0.0 against -0.0",
                     "a NaN with another payload", "another width", "another height", "another mapping", "the transmittance table rendered again",
                     "another first row", "another row stride", "rows stored, the whole LUT asked for"):
            assert not by_name["%s, %s form" % (miss, form)], (miss, form)
    on = (1, 1, 1, 0, 1)
    assert by_name["flags %s, equal keys, whole form" % (on,)]
    for off in range(len(FLAGS)):                                          # each flag alone turns the whole form's hit into a miss
        combo = tuple(v ^ 1 if i == off else v for i, v in enumerate(on))
        assert not by_name["flags %s, equal keys, whole form" % (combo,)], FLAGS[off]
    assert by_name["flags %s, equal keys, rows form" % ((1, 0, 0, 1, 0),)]   # the rows form asks the switch and the key alone
    assert not by_name["flags %s, equal keys, rows form" % ((0, 1, 1, 0, 1),)]


def test_the_header_includes_nothing_of_hip():
    src = open(os.path.join(ROOT, "godot-volumetric-cloud-demo-v2_amd", "csrc", "sky_lut_reuse.h")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert includes == ["<cstring>"], includes
