"""The weather-only step of a context's noise state: NoiseHeld::reweathered (csrc/noise_set.h), compiled with g++ (tests/weather_set_host) and walked
against a model written from the rule:

  reweathered (range)   legal only while a set is had; then the range is replaced and the cached rejects go; the answer says which.
                        Never changes have, cell32, inexact, lod5 or a pending request for exact cells.

The other steps are modelled as tests/test_noise_set_host.py models them; the height windows are bake.h's own, printed by the same program.
Nothing here touches a GPU."""
import itertools
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "weather_set_host")


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


SHIPPED, STRATUS, MIXED, UNBOUND = (151, 231, 255), (75, 115, 200), (100, 180, 230), (0, 255, 255)
COV = bits(0.2)
COV2 = bits(0.35)
LOD5 = bits(0.4375)
OFF = (bits(-1.0), bits(2.0), 0)


def ct_mode(r):
    return 1 if r[0] >= 128 else (2 if r[1] <= 127 else 0)


def run(text_in):
    r = subprocess.run([os.path.join(DIR, "weather_set_host")], input=text_in, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()]


@pytest.fixture(scope="module")
def tool():
    subprocess.check_call(["make", "-C", DIR, "-s"])
    return run


@pytest.fixture(scope="module")
def windows(tool):
    keys = [(c, r) for c in (COV, COV2) for r in (SHIPPED, STRATUS, MIXED, UNBOUND)]
    w = dict(zip(keys, tool("".join("window %d %d %d %d\n" % ((c,) + r) for c, r in keys))))
    assert len(set(w.values())) == len(keys), w                  # an answer for another coverage or range cannot pass for the right one
    return w


class Model:
    def __init__(self, windows):
        self.w = windows
        self.have, self.cell32, self.inexact, self.lod5, self.range, self.requested = False, False, 0, 0, UNBOUND, False

    def step(self, name, arg):
        """-> (answer, rejects)"""
        if name == "request_exact":
            self.requested = arg == 1
        elif name == "begin_rebind":
            self.have = False
        elif name == "bound":
            self.inexact, self.range = arg
            self.lod5 = LOD5
            self.cell32 = self.inexact != 0 or self.requested
            return int(self.cell32), (0, 0, 0)
        elif name == "ready":
            self.have = True
        elif name == "reweathered":
            if not self.have:
                return 0, (0, 0, 0)
            self.range = arg
            return 1, (0, 0, 0)
        elif name == "rejects":
            cov, win = arg
            return 0, (self.w[(cov, self.range)] + (ct_mode(self.range),) if win else OFF)
        return 0, (0, 0, 0)

    def line(self, answer, rej):
        return (int(self.have), int(self.cell32), self.inexact, self.lod5) + self.range + (answer,) + rej


def text(name, arg):
    if name == "bound":
        return "bound %d %d %d %d %d" % ((arg[0],) + arg[1] + (LOD5,))
    if name == "reweathered":
        return "reweathered %d %d %d" % arg
    if name == "rejects":
        return "rejects %d %d" % arg
    return name if arg is None else "%s %d" % (name, arg)


def walk(tool, windows, steps):
    out = tool("reset\n" + "".join(text(*s) + "\n" for s in steps))
    m = Model(windows)
    assert out[0] == m.line(0, (0, 0, 0))
    for k, (s, got) in enumerate(zip(steps, out[1:])):
        answer, rej = m.step(*s)
        assert got == m.line(answer, rej), (k, s, got, m.line(answer, rej))
    return out[1:]


def test_w5_a_bind_a_reweather_a_full_bind_and_requests_in_between(tool, windows):
    ask, ask2, ask_off = ("rejects", (COV, 1)), ("rejects", (COV2, 1)), ("rejects", (COV, 0))
    bind = lambda n, r: [("begin_rebind", None), ("bound", (n, r)), ("ready", None)]
    steps = bind(0, SHIPPED) + [ask, ask, ask2, ask,
                                ("request_exact", 1), ("reweathered", STRATUS), ask, ask2, ask_off, ask,
                                ("reweathered", MIXED), ask,
                                ("request_exact", 0), ("reweathered", SHIPPED), ask] + \
        bind(0, STRATUS) + [ask, ("request_exact", 1), ("reweathered", MIXED), ask] + bind(7, SHIPPED) + [("request_exact", 0), ("reweathered", STRATUS), ask] + \
        bind(0, SHIPPED) + [("request_exact", 1)] + bind(0, SHIPPED) + [("request_exact", 0), ("reweathered", STRATUS), ask, ask2]
    out = walk(tool, windows, steps)
    rej = lambda k: out[k][8:]
    # a reweather at the same coverage answers with the new range's window, not the cached one of the old range
    assert rej(3) == rej(4) == windows[(COV, SHIPPED)] + (1,)
    assert rej(9) == windows[(COV, STRATUS)] + (2,) and rej(9) != rej(4)
    assert rej(14) == windows[(COV, MIXED)] + (0,)
    # a request made before a reweather does not take effect at it (cell32 stays 0), and one withdrawn does not lose the exact cells of the bind (stays 1)
    assert [out[k][1] for k in (7, 8, 13)] == [0, 0, 0]
    assert out[-3][1] == 1 and out[-3][7] == 1 and out[-1][1] == 1
    # textures with inexact coefficients stay on exact cells through a reweather, the count with them
    k = steps.index(("bound", (7, SHIPPED)))
    assert out[k + 3][:3] == (1, 1, 7) and out[k + 3][4:7] == STRATUS


def test_w5_a_reweather_is_legal_only_while_a_set_is_had(tool, windows):
    steps = [("reweathered", STRATUS), ("rejects", (COV, 1)),                                        # never bound
             ("begin_rebind", None), ("bound", (0, SHIPPED)), ("reweathered", STRATUS), ("ready", None), ("rejects", (COV, 1)),   # inside a bind
             ("begin_rebind", None), ("reweathered", MIXED), ("ready", None), ("rejects", (COV, 1))]  # after a failed bind
    out = walk(tool, windows, steps)
    assert [out[k][7] for k in (0, 4, 8)] == [0, 0, 0]
    assert out[1][4:7] == UNBOUND and out[6][4:7] == SHIPPED and out[10][4:7] == SHIPPED


ALPHABET = (("request_exact", 0), ("request_exact", 1), ("begin_rebind", None), ("ready", None), ("bound", (0, SHIPPED)), ("bound", (7, STRATUS)),
            ("reweathered", STRATUS), ("reweathered", MIXED), ("rejects", (COV, 1)), ("rejects", (COV, 0)))


def test_w5_every_walk_of_up_to_three_steps_behind_a_bind_matches_the_model(tool, windows):
    """10 + 100 + 1000 sequences, each from a fresh state and from a bound one: one process, the model line by line."""
    seqs = [seq for n in range(1, 4) for seq in itertools.product(ALPHABET, repeat=n)]
    pre = [[], [("begin_rebind", None), ("bound", (0, SHIPPED)), ("ready", None), ("rejects", (COV, 1))]]
    runs = [p + list(seq) for seq in seqs for p in pre]
    out = tool("".join("reset\n" + "".join(text(*s) + "\n" for s in r) for r in runs))
    at = legal = illegal = 0
    for r in runs:
        m = Model(windows)
        assert out[at] == m.line(0, (0, 0, 0)); at += 1
        for s in r:
            before = (m.have, m.cell32, m.inexact, m.lod5, m.requested)
            answer, rej = m.step(*s)
            assert out[at] == m.line(answer, rej), (r, s, out[at]); at += 1
            if s[0] == "reweathered":
                assert (m.have, m.cell32, m.inexact, m.lod5, m.requested) == before
                legal += answer; illegal += 1 - answer
    assert at == len(out) and legal > 0 and illegal > 0
